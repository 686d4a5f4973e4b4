/* vds.h -- C ABI of the MI355X-native video-DiT train-step kernels (libvds_hip.so).
 *
 * The reference (fal-ai-community/video-diffusion-speedrun) has no FFI layer: its operator
 * surface is the set of torch call sites inside model.py / train.py.
 * Each entry point below replaces one (group of) call site(s), cited as file:line of the
 * reference.  Conventions:
 *   - plain pointers + sizes only, no torch types; all pointers are DEVICE pointers;
 *   - the caller owns/allocates every buffer (inputs, outputs, workspace); kernels never
 *     allocate, free or synchronise;
 *   - every call is asynchronous on the hipStream_t passed last (void* here so that the
 *     header is usable from plain C / ctypes / cgo without the HIP headers);
 *   - return 0 on success, negative VDS_ERR_* on bad arguments / unsupported shapes /
 *     launch failure (the Python host turns that into RuntimeError, matching the
 *     reference's exception convention);
 *   - bf16 tensors are raw uint16 bit patterns; "f32" are IEEE floats;
 *   - thread-compatible: one caller thread per process (one process per GPU).
 */
#ifndef VDS_H
#define VDS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDS_OK 0
#define VDS_ERR_ARG (-1)
#define VDS_ERR_UNSUPPORTED (-2)
#define VDS_ERR_LAUNCH (-3)

typedef void* vds_stream_t; /* hipStream_t */

int vds_version(void);
const char* vds_last_error(void);

/* ------------------------------------------------------------------ GEMM (MFMA) ------
 * C[M,N] = sum_k opA[m,k] * opB[k,n], bf16 operands, fp32 accumulate.
 *   layout VDS_NT: A[M,K] (lda), B[N,K] (ldb)   nn.Linear forward  y = x W^T
 *                  (model.py:125,138,147,150,159,84,86,184,390,90,319,321)
 *   layout VDS_NN: A[M,K] (lda), B[K,N] (ldb)   its input gradient  dx = dy W
 *   layout VDS_TN: A[K,M] (lda), B[K,N] (ldb)   its weight gradient dW = dy^T x  (fp32 out)
 * epilogues fuse the elementwise work the reference runs as separate kernels:
 *   VDS_EPI_STORE      C = bf16(acc + bias[n])
 *   VDS_EPI_BIAS_GELU  C = bf16(pre), C2 = bf16(gelu_erf(pre)), pre = acc + bias[n]  (model.py:84-85)
 *   VDS_EPI_GATE_RES   C = bf16(y), C2 = bf16(aux[m,n] + y*gate[m/rows_per_batch, n]),
 *                      y = acc + bias[n]                         (model.py:138-139,159-160,165)
 *   VDS_EPI_DGELU      C = bf16(acc * gelu'(aux[m,n]))           (backward of model.py:85)
 *   VDS_EPI_F32        C(f32) = acc; a K split (vds_gemm_args.split_k) runs over blockIdx.y and accumulates
 *                      atomically into the pre-zeroed C; the accumulate forms let several calls sum into one C
 * Single-output forms of the two-output epilogues (a forward pass that keeps nothing for a backward: no_grad, and
 * the first forward of a recomputing model): with C == NULL and C2 != NULL, VDS_EPI_BIAS_GELU stores only the
 * activation and VDS_EPI_GATE_RES only the new residual stream, in every tiling and in the partial tiles; what is
 * stored is bit-identical to the two-output launch.  C == NULL with any other epilogue, or with C2 == NULL too, is
 * VDS_ERR_ARG.
 * Requirements (anything else is VDS_ERR_ARG): K % 8 == 0 for NT / NN (any K for TN); N % 8 == 0 (TN: M % 8 == 0
 * too); lda % 8 == 0 and ldb % 8 == 0; and for every other pointer the call uses (non-NULL and read or written by
 * its epilogue) a leading dimension that keeps 16-byte row segments aligned: ldc % 8 == 0 (ldc % 4 == 0 for the
 * fp32 C of VDS_EPI_F32), ldc2 % 8 == 0 (BIAS_GELU, GATE_RES), ldaux % 8 == 0 (GATE_RES, DGELU), ldgate % 4 == 0
 * (GATE_RES).  Base pointers must be 16-byte aligned (not checked); an A or B operand of 4 GiB or more is
 * VDS_ERR_UNSUPPORTED.
 * Six (layout, epilogue) pairs exist: NT + STORE, NT + BIAS_GELU, NT + GATE_RES, NN + STORE, NN + DGELU, TN + F32.  Any
 * other pair is VDS_ERR_UNSUPPORTED -- in every tiling, with or without colsum, before anything is chosen or launched --
 * unless the call also breaks a requirement above: VDS_ERR_ARG wins. */
enum { VDS_NT = 0, VDS_NN = 1, VDS_TN = 2 };
enum { VDS_EPI_STORE = 0, VDS_EPI_BIAS_GELU = 1, VDS_EPI_GATE_RES = 2, VDS_EPI_DGELU = 3, VDS_EPI_F32 = 4 };

typedef struct vds_gemm_args {
  int32_t layout, epilogue;
  int32_t M, N, K;
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  void* C; int64_t ldc;
  void* C2; int64_t ldc2;
  const void* bias;            /* bf16 [N] or NULL */
  const void* aux; int64_t ldaux; /* bf16 [M,N]: residual (GATE_RES) or pre-activation (DGELU) */
  const float* gate; int64_t ldgate; /* f32 [batch, ldgate], column n */
  int32_t rows_per_batch;
  int32_t split_k;             /* TN + F32 only: 0 = the library picks tiling and K split (atomics iff it splits; C
                                  pre-zeroed), -1 = the same but always accumulating atomically into C, 1 = no
                                  split, > 1 = that many splits + atomics, <= -2 = |split_k| splits, accumulate */
  float* colsum;               /* VDS_EPI_DGELU only, may be NULL: colsum[n] += sum_m C[m,n] (f32, atomically; the bias
                                  gradient of the layer below, model.py:84) -- fused into the epilogue of the 256^2
                                  kernel, a pass over C after the GEMM for the smaller tilings.  Needs C != NULL. */
} vds_gemm_args;

int vds_gemm_bf16(const vds_gemm_args* args, vds_stream_t stream);
/* Tests / experiments: pin the tiling vds_gemm_bf16 picks (0 = by its cost model (default), 128 = 128x128 tiles,
 * 256 = 256x256, 2 = 256x128 with two workgroups per CU); returns the previous setting, VDS_ERR_ARG for other
 * values.  Knob "gemm_tile" (VDS_GEMM_TILE sets the initial value).  Results are identical across tilings up
 * to fp32 summation order. */
int vds_gemm_force_tile(int32_t tile);
/* (vds_gemm_plan, below vds_gemm_bf16_grouped, reports the tiling and grid a call would get.) */
/* ------------------------------------------------------------ process-wide settings -----
 * Every tuning knob of the library lives in ONE table (csrc/config.h lists them with their defaults) that is filled from
 * the environment once, when the library is loaded; no entry point reads the environment afterwards.  vds_knob_set
 * changes an entry by name (e.g. "gemm_narrow", "cross_dkv16", "attn_wide_stores": same-process A/B measurements and
 * tests); VDS_ERR_ARG for an unknown name.  vds_knob_get returns the value, NaN for an unknown name.  Besides the
 * communicator this table is the library's only mutable global state. */
int vds_knob_set(const char* name, double value);
double vds_knob_get(const char* name);

/* Deterministic mode (default off).  The default backward accumulates with fp32 atomics in several places -- the split-K
 * slices of the weight-gradient GEMMs, the per-workgroup column sums of the modulation / bias / RMSNorm-weight gradients,
 * the lambda gradients -- so two runs differ in the last bits (autograd's reductions behind the reference's
 * train.py:431-433 have a fixed order).  on = 1: every one of them becomes a fixed-order reduction: partial results go to
 * `workspace` (caller-allocated, 16-byte aligned, `workspace_bytes` long; kept until the mode is switched off) with plain
 * stores and one pass sums them in index order.  Two backward passes over the same inputs then give bit-identical
 * gradients.  A split-K GEMM uses as many splits as fit the workspace (M*N*4 bytes each); row kernels need
 * 3 * D * 4 bytes per workgroup (<= 2048 workgroups).  All deterministic launches must be on one stream.  Returns the
 * previous mode, VDS_ERR_ARG for a bad argument. */
int vds_set_deterministic(int32_t on, void* workspace, size_t workspace_bytes);

/* The same GEMM with OCP fp8 operands (BASELINE config 5; no reference counterpart -- the reference trains in
 * bf16): layout VDS_NT: A[M,K] and B[N,K] one byte per element (a_fmt / b_fmt: 0 = e4m3fn, 1 = e5m2; B must
 * be e4m3fn), K, lda, ldb multiples of 16.  C = epilogue((sum_k A B) * *scale_a * *scale_b) with per-tensor
 * dequantisation factors read from device memory (NULL = 1).  Runs v_mfma_f32_16x16x128_f8f6f4 (2x the bf16
 * MFMA rate).  Input gradients are NT products with the transposed WEIGHT copy written by vds_quant_fp8.
 * The epilogues, their single-output forms (C == NULL with C2 != NULL: VDS_EPI_BIAS_GELU, VDS_EPI_GATE_RES) and the
 * requirements on ldc / ldc2 / ldaux / ldgate are those of vds_gemm_bf16: a leading dimension that breaks the epilogues'
 * 16-byte row segments (ldc % 8, ldc % 4 for the fp32 C of VDS_EPI_F32, ldc2 % 8, ldaux % 8, ldgate % 4, each for the
 * pointers the call uses) is VDS_ERR_ARG, and so is VDS_EPI_GATE_RES without C2.
 * layout VDS_TN (round 4; epilogue VDS_EPI_F32, a_fmt = 1 only): C[M,N] = sum_k A[k,m] B[k,n] with A [K,M] e5m2 and
 * B [K,N] e4m3, both row-major, K, M, lda, ldb multiples of 16 -- the weight gradient dW = dy^T x contracted straight
 * from the token-major fp8 copies (both operands k-major: ds_read_b64_tr_b8 fragments), split_k as vds_gemm_bf16.
 *
 * emit (may be NULL; VDS_EPI_BIAS_GELU / VDS_EPI_DGELU only): the epilogue also writes its result -- gelu(pre) resp.
 * acc * gelu'(aux), rounded to bf16 first -- as fp8 for the next GEMMs, so that no separate quantisation pass reads
 * it back (bit-identical to vds_quant_fp8 of the bf16 result for finite results; any M, the last M % 4 columns of qt
 * written byte by byte): q[M,N] row-major and / or qt[N,M] transposed, scaled by fmax / *amax_in (delayed scaling: the caller
 * passes the amax recorded by the previous step), *dq_out = *amax_in / fmax, *amax_out = max(*amax_out, max |result|)
 * of this launch, colsum[n] += sum_m result[m,n] (bias gradient).  With emit, C2 (BIAS_GELU) / C (DGELU) may be NULL. */
typedef struct vds_fp8_out {
  void* q; int64_t ldq;
  void* qt; int64_t ldqt;
  const float* amax_in;
  float* amax_out;
  float* dq_out;
  int32_t fmt;      /* 0 = e4m3fn, 1 = e5m2 */
  float* colsum;    /* f32 [N] or NULL */
} vds_fp8_out;

int vds_gemm_fp8(const vds_gemm_args* args, const float* scale_a, const float* scale_b, int32_t a_fmt,
                 int32_t b_fmt, const vds_fp8_out* emit, vds_stream_t stream);

/* amax[0] = max(amax[0], max |x|) over a bf16 matrix x[M,K] (row stride ldx elements); the caller zeroes amax. */
int vds_absmax(const void* x, int64_t ldx, int32_t M, int32_t K, float* amax, vds_stream_t stream);

/* Per-tensor fp8 quantisation of a bf16 matrix: q[m,k] = sat(x[m,k] * fmax / *amax) (fmt 0: e4m3fn, fmax 448;
 * fmt 1: e5m2, fmax 57344), written row-major to q[M,K] (ldq, may be NULL) and / or transposed to qt[K,M] (ldt,
 * may be NULL); *dq_out = *amax / fmax is the factor vds_gemm_fp8 multiplies back in.  *amax == 0 -> scale 1.
 * amax_out (may be NULL): *amax_out = max(*amax_out, max |x|) -- with delayed scaling `amax` is the value a previous
 * step recorded and this call records the next one, so that no separate vds_absmax pass reads x.
 * Any M >= 1 is served (K % 8 == 0, ldx % 8 == 0, ldq % 8 == 0, ldt % 4 == 0): the transposed copy is written four
 * rows of x per store, and the last M % 4 of them byte by byte.  The cast is ONE fp32 multiply by fmax / *amax, a clamp to
 * +-fmax and a round-to-nearest-even conversion (subnormals kept, -0 kept); tests/helpers/fp8_census.py restates it. */
int vds_quant_fp8(const void* x, int64_t ldx, int32_t M, int32_t K, int32_t fmt, const float* amax, void* q,
                  int64_t ldq, void* qt, int64_t ldt, float* dq_out, float* amax_out, vds_stream_t stream);

/* qt[k,m] = q[m,k] for a one-byte-per-element matrix q[M,K] (row stride ldq; K, ldq multiples of 16, ldt of 4; any
 * M >= 1, the last M % 4 columns of qt written byte by byte): the
 * k-contiguous copy of an fp8 operand whose row-major copy came straight out of its producer (the *_fp8 entry points
 * below).  1 B read + 1 B written per element against 2 + 1 + 1 of a vds_quant_fp8 pass over the bf16 tensor. */
int vds_transpose_fp8(const void* q, int64_t ldq, int32_t M, int32_t K, void* qt, int64_t ldt, vds_stream_t stream);

/* fp8-emitting forms of three producers of the fp8 GEMMs' operands (config 5): the bf16 result of the plain entry
 * point is not written; instead each value, rounded to bf16 first, is scaled by fmax / *amax_in (delayed scaling:
 * the amax the previous step recorded; 0 -> scale 1) and cast with saturation to q[rows, ldq] (fmt 0 = e4m3fn,
 * 1 = e5m2; ldq a multiple of 8) -- bit-identical to vds_quant_fp8 of the plain result for finite results (what a
 * NaN or an infinity becomes, and what amax it records, differs from site to site: DESIGN.md 25).  *dq_out = *amax_in / fmax
 * (may be NULL).  max |result| is recorded per wave with plain stores (amax_part, f32 [B*L], may be NULL): entry w
 * receives the maximum over the rows wave w handled -- one entry per row / token for the RMSNorm and RoPE kernels (one per
 * four rows, at the first of them, for RMSNorm at D = 384 / 768 / 1152), the entry of the first row a wave walks for gate
 * backward; the other entries are not written -- and the tensor's amax is the maximum over the array
 * (the caller zeroes it before the launch and reduces it afterwards; no atomics: ~10^5 short waves per launch).  All other arguments as in
 * vds_rmsnorm_mod_fwd / vds_gate_bwd / vds_qkv_rope_bwd (the latter needs hdp % 8 == 0, H*hd <= 2048 and ldq >= 3*H*hd,
 * else VDS_ERR_UNSUPPORTED), except that y / ldy, dy / lddy and dqkv are not taken; q or amax_in NULL, ldq % 8 != 0 or
 * another fmt: VDS_ERR_ARG, as is B < 1 or L < 1 in the RMSNorm and gate forms. */
int vds_rmsnorm_mod_fwd_fp8(const void* x, int64_t ldx, const void* w, const float* mod, int64_t ldmod,
                            int32_t shift_col, int32_t scale_col, void* q, int64_t ldq, int32_t fmt,
                            const float* amax_in, float* amax_part, float* dq_out, float* rstd, int32_t B, int32_t L,
                            int32_t D, float eps, vds_stream_t stream);
int vds_gate_bwd_fp8(const void* dxn, int64_t lddxn, const void* y, int64_t ldy, const float* mod, int64_t ldmod,
                     int32_t gate_col, void* q, int64_t ldq, int32_t fmt, const float* amax_in, float* amax_part,
                     float* dq_out, float* dmod, float* dbias, int32_t B, int32_t L, int32_t D, vds_stream_t stream);
int vds_qkv_rope_bwd_fp8(const void* dq, const void* dk, const void* dv, const float* cosb, const float* sinb,
                         const void* qkv_raw, const void* v0, const void* lam, float* dv0_acc, float* dlam, void* q,
                         int64_t ldq, int32_t fmt, const float* amax_in, float* amax_part, float* dq_out, int32_t mix,
                         int32_t add_dv0, int32_t B, int32_t L, int32_t H, int32_t hd, int32_t hdp,
                         vds_stream_t stream);

/* --------------------------------------------------------------- attention (MFMA) ----
 * F.scaled_dot_product_attention(q,k,v) full/non-causal (model.py:136,157), flash style.
 * q/k/v are addressed as base + b*stride_b + h*stride_h + l*stride_l (elements), rows of
 * head_dim contiguous bf16; O/dO the same.  lse [B,H,Lq] f32 = log-sum-exp of the scaled
 * scores (natural log).  head_dim in {64, 72, 128}. */
typedef struct vds_attn_args {
  int32_t B, H, Lq, Lk, head_dim;
  const void* q; int64_t q_sb, q_sh, q_sl;
  const void* k; int64_t k_sb, k_sh, k_sl;
  const void* v; int64_t v_sb, v_sh, v_sl;
  void* o; int64_t o_sb, o_sh, o_sl;
  float* lse;
  /* backward only */
  const void* d_o; int64_t do_sb, do_sh, do_sl;
  void* dq; int64_t dq_sb, dq_sh, dq_sl;
  void* dk; int64_t dk_sb, dk_sh, dk_sl;
  void* dv; int64_t dv_sb, dv_sh, dv_sl;
  float* delta;                /* workspace [2,B,H,Lq] f32: -rowsum(dO*O), then lse*log2(e) */
  /* nonzero = every k row carries 1.0 at columns head_dim and head_dim+1 and every v row 1.0 at columns
   * head_dim and head_dim+4 (zeros in the rest of [head_dim, head_dim+8)), as vds_qkv_rope_fwd writes
   * them for hdp >= hd+8; the kernels then fold the per-query constants of the softmax (max, lse, delta)
   * into their MFMAs instead of spending VALU instructions on them.  With the flag the q rows must be
   * padded to head_dim+8 columns as well: vds_attn_bwd OVERWRITES their columns head_dim, head_dim+1
   * (scratch: -lse*log2(e) as a bf16 hi/lo pair for the dK/dV kernel).
   * 2 (round 5; cross-attention, model.py:157): k / v carry the ones columns (vds_kv_pad_ones) but the q rows have NO pad
   * (token-major views of a linear layer's output): forward and dQ run on the ones-column kernels -- they keep q / dO in
   * registers and set the pad columns there --, dK/dV on the plain kernel; nothing is written into q. */
  int32_t kv_pad_ones;
  /* backward only: number of floats `delta` points to.  0 = exactly 2*B*H*Lq (the statistics).  With the size
   * vds_attn_bwd_workspace_bytes returns, the dK/dV kernel may split the query range over several workgroups per key
   * tile when the key sequence is short (cross-attention, model.py:157: 512 context keys = 4 key tiles per head) and
   * keep its fp32 partial sums behind the statistics. */
  int64_t ws_floats;
} vds_attn_args;

int vds_attn_fwd(const vds_attn_args* args, vds_stream_t stream);
/* Lq <= 0 or Lk <= 0: VDS_ERR_ARG before anything is launched, as in vds_attn_fwd and every masked call below. */
int vds_attn_bwd(const vds_attn_args* args, vds_stream_t stream);
/* The same two calls with per-sample key counts: kv_lens = device pointer to B int32, each in [0, Lk] (values outside
 * are clamped); the kernels read it, never the host, so a captured graph replays with new lengths.  Sample b attends
 * keys 0 .. kv_lens[b]-1 only: o, lse and dq are those of that restricted attention, rows < kv_lens[b] of dk / dv get
 * its gradient and rows kv_lens[b] .. Lk-1 are WRITTEN as exact zeros.  kv_lens[b] == 0 means "no context": o, dq,
 * dk, dv = 0 and lse = 0 for that sample, no NaN.  Key tiles past the count are skipped, not computed and masked; the
 * launch geometry and the workspace (vds_attn_bwd_workspace_bytes) stay functions of Lk.  kv_lens == NULL forwards to
 * vds_attn_fwd / vds_attn_bwd.  kv_pad_ones 0 and 2 (cross-attention); kv_pad_ones == 1 with lengths: VDS_ERR_ARG. */
int vds_attn_fwd_kvlen(const vds_attn_args* args, const int32_t* kv_lens, vds_stream_t stream);
int vds_attn_bwd_kvlen(const vds_attn_args* args, const int32_t* kv_lens, vds_stream_t stream);
/* K / V of a cross-attention, token-major bf16 rows [B*Lk, ld] with head h of K at columns k_col0 + h*hd and of V at
 * v_col0 + h*hd (the context_kv output, model.py:150-156), copied into head-major padded rows kp, vp [B,H,Lk,hdp]
 * (hdp >= hd + 8, multiples of 8) with the ones columns of vds_attn_args.kv_pad_ones and zeros in the rest of the pad. */
int vds_kv_pad_ones(const void* kv, int64_t ld, int32_t k_col0, int32_t v_col0, void* kp, void* vp, int32_t B, int32_t Lk,
                    int32_t H, int32_t hd, int32_t hdp, vds_stream_t stream);
/* Tests / experiments: which of the head_dim-72 (ones-column) kernels run on v_mfma_f32_16x16x32_bf16 instead of
 * v_mfma_f32_32x32x16_bf16 -- bit 0: dK/dV, bit 1: dQ, bit 2: forward; -1 = back to the default (7); knob "attn_mfma16".
 * Returns the previous mask.  Results agree up to fp32 summation order. */
int vds_attn_set_variant(int32_t mask);
/* bytes of the caller-allocated `delta` workspace vds_attn_bwd wants for these B, H, Lq, Lk, head_dim, kv_pad_ones:
 * 2*B*H*Lq floats of statistics + the partial sums of a query-split dK/dV launch (see ws_floats) */
size_t vds_attn_bwd_workspace_bytes(const vds_attn_args* args);

/* ------------------------------------------------------ normalisation / modulation ---
 * y = bf16( rmsnorm(x)[*w] * (1 + scale[b]) + shift[b] ), rstd saved (model.py:34-41,123,144,164,389).
 * x,y [B*L, D] bf16; mod f32 [B, ldmod] with shift at column shift_col, scale at scale_col;
 * w bf16 [D] or NULL; rstd f32 [B*L].  D and ldx, ldy multiples of 8, shift_col, scale_col and ldmod multiples of 4 (the
 * modulation row is read in 16-byte pieces).  B < 1 or L < 1: VDS_ERR_ARG, nothing is launched -- the rule of every RMSNorm and
 * gate entry point below, plain, _grouped and _fp8 alike.  D > 2048 (no instance): VDS_ERR_UNSUPPORTED, likewise. */
int vds_rmsnorm_mod_fwd(const void* x, int64_t ldx, const void* w, const float* mod, int64_t ldmod,
                        int32_t shift_col, int32_t scale_col, void* y, int64_t ldy, float* rstd,
                        int32_t B, int32_t L, int32_t D, float eps, vds_stream_t stream);
/* dx = bf16( dres + d/dx ), dmod[b, shift_col..] += sum_l dy, dmod[b, scale_col..] += sum_l dy*xhat*w,
 * dw (f32 [D], atomically +=) if w != NULL.  dres may be NULL.  Every access is a 16-byte row segment: D, lddy, ldx,
 * lddx and (with dres != NULL) lddres must be multiples of 8, else VDS_ERR_ARG and nothing is written (the grouped
 * call checks the same).  B < 1 or L < 1: VDS_ERR_ARG. */
int vds_rmsnorm_mod_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* w,
                        const float* mod, int64_t ldmod, int32_t shift_col, int32_t scale_col,
                        const float* rstd, const void* dres, int64_t lddres, void* dx, int64_t lddx,
                        float* dmod, float* dw, int32_t B, int32_t L, int32_t D, vds_stream_t stream);

/* gate backward of  x_new = x + y*gate  (model.py:139,160,165):
 *   dy = bf16(dx_new * gate[b]),  dmod[b, gate_col + n] += sum_l dx_new*y,
 *   dbias[n] (f32, atomically +=) += sum_{b,l} dy   if dbias != NULL.
 * D, lddxn, ldy and lddy must be multiples of 8 (16-byte row segments), else VDS_ERR_ARG and nothing is written; the
 * same holds for vds_gate_bwd_grouped and (lddxn, ldy, ldq) vds_gate_bwd_fp8.  B < 1 or L < 1: VDS_ERR_ARG. */
int vds_gate_bwd(const void* dxn, int64_t lddxn, const void* y, int64_t ldy, const float* mod,
                 int64_t ldmod, int32_t gate_col, void* dy, int64_t lddy, float* dmod, float* dbias,
                 int32_t B, int32_t L, int32_t D, vds_stream_t stream);

/* ------------------------------------------- modulation groups (per-frame timesteps) ---
 * The calls above read ONE modulation row per sample.  A group description splits the L rows of a sample into
 * G = 1 + period modulation groups: group 0 is rows 0 .. lead-1 (the register tokens), and row l >= lead belongs to
 * group 1 + (l - lead) % period (the token order is (h w t) with t fastest, so the rows of token-frame f are lead + f,
 * lead + f + period, ...).  The modulation tables then have B*G rows, row b*G + g for group g of sample b.
 * lead < 0, period < 1 or (L - lead) % period != 0: VDS_ERR_ARG; so is B*G > 65535 in the two backward calls (the modulation
 * rows are a grid dimension).  groups == NULL forwards to the per-sample call. */
typedef struct {
  int32_t lead;    /* rows of group 0 at the head of every sample (may be 0: group 0 is empty, its dmod row untouched) */
  int32_t period;  /* number of frame groups */
} vds_mod_groups;
/* Frame-causal self-attention: vds_attn_fwd / vds_attn_bwd restricted by the row groups above (frames = {lead, period},
 * the same validation against L = Lq).  Query row q attends key row k iff group(k) <= group(q): the lead rows attend
 * each other, a row of token-frame f attends the lead rows and every row of frames 0 .. f (its own included); every
 * query has a key, there is no empty row.  o, lse and dq are those of the restricted softmax, a dk / dv row sums over
 * the queries that attend it, and an excluded pair contributes P = 0 exactly (its score never enters a running maximum).
 * The rows of a frame are interleaved with the period, so the mask is applied per element and no key tile is skipped.
 * lead and period travel by value in the kernel arguments (a captured graph replays them).  Self-attention only:
 * Lq != Lk or kv_pad_ones == 2 is VDS_ERR_ARG; kv_pad_ones 0 and 1, every head dim of the dispatcher and every
 * vds_attn_set_variant / knob setting have a masked instance; L > 2^21 rows is VDS_ERR_UNSUPPORTED.  frames == NULL
 * forwards to vds_attn_fwd / vds_attn_bwd, which launch what they always launched; vds_attn_bwd_workspace_bytes is
 * unchanged. */
int vds_attn_fwd_causal(const vds_attn_args* args, const vds_mod_groups* frames, vds_stream_t stream);
int vds_attn_bwd_causal(const vds_attn_args* args, const vds_mod_groups* frames, vds_stream_t stream);
/* Frame-causal forward with a past (inference with a frame KV cache).  The queries are the Lq = lead + n * period rows of
 * one model call (the lead rows, then the call's token rows: the (lead, period) map above, validated against Lq).  The
 * keys and values are Lk = Lq + past rows: j < lead the call's lead rows, lead <= j < lead + past the past (token rows of
 * finished frames, in any order), j >= lead + past the call's own token rows (key j belongs to query row j - past).  A
 * lead query attends the lead keys only; a token query attends the lead keys, every past key and own key j iff
 * group(j - past) <= group(query).  Key 0 is attended by every query: no empty row.  A 32-key sub-block that lies wholly
 * in the past is attended without any mask code by every wave that holds no lead query.  `past` travels by value in the
 * kernel arguments.  past == 0 forwards to vds_attn_fwd_causal (the same bits); past < 0, frames == NULL with past != 0,
 * Lk != Lq + past or kv_pad_ones == 2: VDS_ERR_ARG; Lk > 2^21: VDS_ERR_UNSUPPORTED.  kv_pad_ones 0 and 1, every head dim
 * of the dispatcher and every vds_attn_set_variant setting have an instance.  Forward only. */
int vds_attn_fwd_causal_past(const vds_attn_args* args, const vds_mod_groups* frames, int32_t past, vds_stream_t stream);
/* Frame-major self-attention: vds_attn_fwd_causal / vds_attn_bwd_causal with a frame's rows contiguous, so that the key
 * tiles the mask excludes are skipped, not computed.  Layout contract, with S = (L - lead) / period and fm / tok as under
 * vds_qkv_rope_fwd_fm:
 *   - q, k, v, dq, dk, dv, lse and the delta workspace are indexed by the FRAME-MAJOR row r: group(r) = 0 for r < lead,
 *     1 + (r - lead) / S otherwise, and query r attends key j iff group(j) <= group(r) -- the mask above with the rows
 *     permuted; the results are those of the interleaved calls on the permuted rows up to fp32 summation order.
 *   - o and d_o are addressed by TOKEN row: row r of the computation is stored to / loaded from row tok(r) of o / d_o, in
 *     the attention kernels and in the delta preprocess alike.  No extra pass over them is added; the map costs one fp32
 *     quotient per row where the row pointer is formed (exact below 2^21 rows).
 * What is skipped: a forward / dQ workgroup with query rows [q0, q1) runs its key loop to kend = lead if q1 <= lead, else
 * lead + ((q1 - 1 - lead) / S + 1) * S; a dK/dV workgroup with key rows from k0 starts its query loop at the 64-row tile
 * that holds qstart = 0 if k0 < lead, else lead + ((k0 - lead) / S) * S.  Inside the visited range an element is compared
 * against its row's own bound (masked scores are -inf before the sub-block maxima, P = 0 exactly); a 32 x 32 sub-block in
 * which every pair is attended -- all its keys below the kend of the wave's first query and no lead query in the wave,
 * resp. its first query at or past the qstart of the wave's last key -- is branched around.  Key 0 is attended by every
 * query: no empty row.  The profiler credits the FLOPs of the visited range.
 * Every head dim of the dispatcher and kv_pad_ones 0 and 1 run.  Frame-major instances exist of the plain 32x32x16 kernels
 * (attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel: every head dim) and, for the ones layout at head dim 72
 * (kv_pad_ones = 1), of the 16x16x32 family -- attn_fwd16_kernel, attn_bwd_dq16_kernel with and without the folded
 * preprocess, attn_bwd_dkv16_kernel -- selected by the same vds_attn_set_variant bits (attn_mfma16), attn_delta_fold knob
 * and attn_fwd_wide rule (64 queries per wave from 2048 queries, or forced) as in vds_attn_*_causal.  The
 * 64-queries-per-wave 32x32 forwards and the ones-column 32x32 kernels have no frame-major instance: where those settings
 * would select one of them (variant bit off in the ones layout, attn_fwd_wide at head dims 64 / 96), the plain 32x32x16
 * frame-major kernel runs instead, on the same rows.  The query range of the dK/dV kernel is never split.  The late query
 * tiles of a head are issued first (knob attn_fm_heavy_first = 0: the plain order).
 * frames == NULL, Lq != Lk or kv_pad_ones == 2: VDS_ERR_ARG; L > 2^21 rows, or a (batch, head) slice of o (backward: of d_o
 * too) of 4 GiB or more -- L * o_sl * 2 >= 2^32 bytes, the token rows are reached through 32-bit byte offsets --:
 * VDS_ERR_UNSUPPORTED.  lead and period travel by value (a captured graph replays them).  The workspace is that of
 * vds_attn_bwd_workspace_bytes (2 B H L floats are used). */
int vds_attn_fwd_causal_fm(const vds_attn_args* args, const vds_mod_groups* frames, vds_stream_t stream);
int vds_attn_bwd_causal_fm(const vds_attn_args* args, const vds_mod_groups* frames, vds_stream_t stream);
/* Chunk-causal frame-major self-attention: the calls above with a mask that is causal over CHUNKS of `chunk` token-frames
 * and bidirectional inside a chunk.  group(l) = 0 for l < lead, 1 + ((l - lead) % period) / chunk otherwise (token rows);
 * in frame-major rows that is 1 + (r - lead) / G with G = chunk * S, a contiguous run, so the attended keys of a query stay
 * a prefix and the queries of a key a suffix: the same kernel instances run with the granularity G in place of S --
 * kend(r) = min(L, lead + ((r - lead) / G + 1) * G), qstart(j) = lead + ((j - lead) / G) * G (the lead rows as above);
 * the layout, tok(), the skipped ranges, the variant bits and knobs, the refusals and the workspace are those of the _fm
 * calls.  period % chunk != 0 is allowed (the last chunk is short: kend is clipped to L); chunk >= period is one token
 * group (tokens attend every row, lead rows the lead rows).  chunk == 1 forwards to the _fm call (the same bits);
 * chunk < 1 or frames == NULL: VDS_ERR_ARG.  chunk travels by value.  The profiler credits the visited range. */
int vds_attn_fwd_causal_fm_chunk(const vds_attn_args* args, const vds_mod_groups* frames, int32_t chunk, vds_stream_t stream);
int vds_attn_bwd_causal_fm_chunk(const vds_attn_args* args, const vds_mod_groups* frames, int32_t chunk, vds_stream_t stream);
/* Sliding-window chunk-causal frame-major self-attention: the _fm_chunk calls with a window of `window_chunks` chunks.  A
 * lead query attends the lead keys; a token query of chunk n attends every lead key and the token keys of chunks
 * max(0, n - window_chunks + 1) .. n.  With G = chunk * S, in frame-major rows query r attends [0, lead) and
 * [kbeg(r), kend(r)), kbeg(r) = lead + max(0, (r - lead) / G - window_chunks + 1) * G, and key j is attended by
 * [qstart(j), qend(j)), qend(j) = min(L, lead + ((j - lead) / G + window_chunks) * G) (L for a lead key); kend and qstart
 * are the _fm_chunk bounds.  Every row attends its own chunk: no empty row; lead = 0 is allowed.
 * What is skipped: a forward / dQ workgroup visits the 64-key tiles that hold lead keys and then the tiles from the one
 * that holds kbeg of its first token query to the one below kend of its last query (never one twice); a dK/dV workgroup
 * whose 128 keys include a lead key sweeps every query tile, any other the tiles from qstart of its first key to the one
 * below qend of its last.  A 32 x 32 sub-block runs without mask code if its wave holds no lead query and its keys lie
 * wholly below lead or wholly inside [kbeg of the wave's last query, kend of its first), resp. if its queries lie inside
 * [the wave's largest qstart, its smallest qend).  The profiler credits the visited range.
 * These are WIN instances of the frame-major kernels -- the plain 32x32x16 family at every head dim and the 16x16x32 family
 * of the ones layout at head dim 72 -- selected by the variant bits and knobs of the _fm calls; no atomics, no workspace
 * beyond that of the _fm calls.  window_chunks >= ceil(period / chunk) forwards to the _fm_chunk call (the same bits);
 * window_chunks < 1, chunk < 1 or frames == NULL: VDS_ERR_ARG; the other refusals are those of the _fm calls.  chunk and
 * window_chunks travel by value. */
int vds_attn_fwd_causal_fm_window(const vds_attn_args* args, const vds_mod_groups* frames, int32_t chunk, int32_t window_chunks,
                                  vds_stream_t stream);
int vds_attn_bwd_causal_fm_window(const vds_attn_args* args, const vds_mod_groups* frames, int32_t chunk, int32_t window_chunks,
                                  vds_stream_t stream);
/* Teacher forcing: frame-major self-attention over [lead rows | n clean token-frames | their n noisy copies], frames->period
 * = 2n.  With S = (L - lead) / period rows per frame, G = min(chunk, n) * S and base = lead + n * S, the chunks of G rows
 * restart at base (the last chunk of each half may be short), and query r attends key j iff j < lead, or r and j are clean
 * and chunk(j) <= chunk(r) (the _fm_chunk mask on the first base rows), or r is noisy and j is clean with chunk(j) <
 * chunk(r), or r and j are noisy with chunk(j) == chunk(r).  A lead query attends the lead keys only.
 * Seen from a query the attended keys are [0, pend(r)) plus [kbeg(r), kend(r)):
 *   clean r: pend = min(base, lead + (chunk + 1) G), no run;   noisy r: pend = lead + chunk G, run [base + chunk G,
 *   min(L, base + (chunk + 1) G)).
 * Seen from a key the readers are [qstart(j), qend(j)) plus [q2(j), L): a lead key [0, L); a clean key [lead + chunk G, base)
 * and [base + (chunk + 1) G, L) -- a hole --; a noisy key its own chunk [base + chunk G, min(L, base + (chunk + 1) G)).
 * What is skipped: a forward / dQ workgroup (128 queries) visits the 64-key tiles below its largest pend and then those from
 * its smallest kbeg to its largest kend, never one twice; a dK/dV workgroup (128 keys) with a lead key sweeps every 64-row
 * query tile, any other the tiles from qstart of its first key to qend of its last and then from q2 of its first key to L.
 * Excluded pairs get P = 0 exactly and never enter a running maximum.  The profiler credits the visited tiles.
 * These are TF instances of the plain 32x32x16 frame-major kernels at every head dim of the dispatcher, for kv_pad_ones 0
 * and 1 (the pad columns are not read); the 16x16x32 family has no TF instance.  Layout, tok() (with the period 2n),
 * workspace and the other refusals are those of the _fm calls; no atomics, bit-identical run to run.
 * frames == NULL, an odd period, chunk < 1, (L - lead) % period != 0, Lq != Lk, kv_pad_ones == 2: VDS_ERR_ARG; L > 2^21 rows
 * or a head dim without instance: VDS_ERR_UNSUPPORTED.  lead, period and chunk travel by value. */
int vds_teacher_attn_fwd(const vds_attn_args* args, const vds_mod_groups* frames, int32_t chunk, vds_stream_t stream);
int vds_teacher_attn_bwd(const vds_attn_args* args, const vds_mod_groups* frames, int32_t chunk, vds_stream_t stream);
/* Frame band: frame-major self-attention for the bidirectional model -- not causal.  With S = (L - lead) / period rows per
 * frame, G = min(chunk, period) * S and chunk(x) = (x - lead) / G (the last chunk is short when period % chunk != 0), a
 * token row x has
 *   lo(x) = lead + max(0, chunk(x) - band_chunks) * G,   hi(x) = min(L, lead + (chunk(x) + band_chunks + 1) * G)
 * and query r attends key j iff r < lead, or j < lead, or lo(r) <= j < hi(r).  A lead query attends all L keys (every
 * causal mask here gives it the lead keys only), a lead key is read by all L queries, and the relation is symmetric: the
 * readers of token key j are [0, lead) and [lo(j), hi(j)).  No row is empty.  lead = 0 is allowed; band_chunks = 0 is "own
 * chunk plus lead rows"; band_chunks >= ceil(period / chunk) - 1 attends every pair and runs the same instances.
 * What is skipped: a forward / dQ workgroup with queries [q0, q1) visits every 64-key tile if q0 < lead, else the lead
 * tiles [0, nl) and then [max(nl, lo(q0) >> 6), ceil(hi(q1 - 1) / 64)), never one twice; a dK/dV workgroup with keys
 * [k0, k1) sweeps every 64-row query tile if k0 < lead, else the lead query tiles and then those from lo(k0) to below
 * hi(k1 - 1).  A 32x32 sub-block runs without mask code when the wave holds no lead row and the block lies wholly below lead
 * or wholly inside [lo of the wave's last row, hi of its first), and in a wave of lead rows only.  Excluded pairs get P = 0
 * exactly and never enter a running maximum.  The forward and dQ workgroups run in plain tile order (the first one of a head
 * is its heaviest; attn_fm_heavy_first does not reverse them).  The profiler credits the visited tiles.
 * These are BAND instances of the plain 32x32x16 frame-major kernels at every head dim of the dispatcher, for kv_pad_ones 0
 * and 1 (the pad columns are not read); the variant bits and knobs that select the 16x16x32 or 64-queries-per-wave family
 * elsewhere select nothing here.  Layout, tok(), workspace and the stride, length and 4 GiB refusals are those of the _fm
 * calls; no atomics, bit-identical run to run.
 * band_chunks < 0, chunk < 1, frames == NULL, Lq != Lk, kv_pad_ones == 2, lead < 0, period < 1 or (L - lead) % period != 0:
 * VDS_ERR_ARG; L > 2^21 rows or a head dim without instance: VDS_ERR_UNSUPPORTED (ARG first).  lead, period, chunk and
 * band_chunks travel by value. */
int vds_band_attn_fwd(const vds_attn_args* args, const vds_mod_groups* frames, int32_t chunk, int32_t band_chunks,
                      vds_stream_t stream);
int vds_band_attn_bwd(const vds_attn_args* args, const vds_mod_groups* frames, int32_t chunk, int32_t band_chunks,
                      vds_stream_t stream);
/* vds_rmsnorm_mod_fwd with mod f32 [B*G, ldmod]: the same arithmetic per row, y / rstd bit-identical to the per-sample
 * call run on the rows of one group with that group's mod row.  Every form of the dispatcher is covered. */
int vds_rmsnorm_mod_fwd_grouped(const void* x, int64_t ldx, const void* w, const float* mod, int64_t ldmod,
                                int32_t shift_col, int32_t scale_col, void* y, int64_t ldy, float* rstd,
                                int32_t B, int32_t L, int32_t D, float eps, const vds_mod_groups* groups,
                                vds_stream_t stream);
/* vds_rmsnorm_mod_bwd with mod / dmod [B*G, ldmod]: a workgroup walks rows of ONE group of one sample (stride `period`
 * for a frame group, the contiguous `lead` rows for group 0), the column sums stay in registers and go to dmod row
 * b*G + g; dx as the per-sample call, dw summed over everything.  Deterministic mode: as vds_rmsnorm_mod_bwd. */
int vds_rmsnorm_mod_bwd_grouped(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* w,
                                const float* mod, int64_t ldmod, int32_t shift_col, int32_t scale_col,
                                const float* rstd, const void* dres, int64_t lddres, void* dx, int64_t lddx,
                                float* dmod, float* dw, int32_t B, int32_t L, int32_t D,
                                const vds_mod_groups* groups, vds_stream_t stream);
/* vds_gate_bwd with mod / dmod [B*G, ldmod]: dy = bf16(dx_new * gate[b*G + g]), dmod[b*G + g, gate_col + n] += the sum
 * over the rows of that group; dbias over everything. */
int vds_gate_bwd_grouped(const void* dxn, int64_t lddxn, const void* y, int64_t ldy, const float* mod,
                         int64_t ldmod, int32_t gate_col, void* dy, int64_t lddy, float* dmod, float* dbias,
                         int32_t B, int32_t L, int32_t D, const vds_mod_groups* groups, vds_stream_t stream);
/* vds_gemm_bf16 for VDS_NT + VDS_EPI_GATE_RES with gate f32 [B*G, ldgate] and args->rows_per_batch = L (M % L == 0):
 * output row r takes the gate row of its group.  Every tiling (vds_gemm_force_tile 0 / 128 / 256 / 2), both output
 * forms (C may be NULL).  The gate row changes from row to row, so every sub-tile runs the per-row epilogue -- the
 * path of a rows_per_batch = 1 launch with an expanded [M, N] gate table, to which the result is bit-identical.
 * Any other layout / epilogue with groups != NULL: VDS_ERR_ARG. */
int vds_gemm_bf16_grouped(const vds_gemm_args* args, const vds_mod_groups* groups, vds_stream_t stream);
/* Tests / experiments: what vds_gemm_bf16 (groups == NULL) / vds_gemm_bf16_grouped would do with these arguments under
 * the current knobs and deterministic mode, without launching anything.  Runs the same argument check and the same
 * planning function as the launching entries: returns the code they would refuse the call with (*info is then left
 * alone), else VDS_OK with *info filled.  info == NULL is VDS_ERR_ARG.  In deterministic mode split_k is the count
 * asked of the split-K launch; that launch still lowers it until its slabs fit the workspace. */
typedef struct vds_gemm_plan_info {
  int32_t tiling;            /* 128 = 128x128 tiles, 2 = 256x128, 256 = 256x256 (the values of vds_gemm_force_tile) */
  int32_t tiles_m, tiles_n;  /* the grid is tiles_m * tiles_n x split_k workgroups */
  int32_t split_k, atomic;   /* K splits (1 = none); the epilogue accumulates into C with fp32 atomics */
  int32_t group_m;           /* row tiles per group of the grouped tile order */
  int32_t joint_xcd;         /* split-K: XCD-aware order over the joint (split, tile) list */
  int32_t narrow;            /* 256x256: the last tile column runs the 256 x 128 body */
  int32_t colsum;            /* args->colsum: 0 absent, 1 fused into the epilogue, 2 a vds_colsum_bf16 pass after the GEMM */
} vds_gemm_plan_info;
int vds_gemm_plan(const vds_gemm_args* args, const vds_mod_groups* groups, vds_gemm_plan_info* info);

/* column sums: out[n] (f32, atomically +=) += sum_m x[m,n]  (bias gradients). */
int vds_colsum_bf16(const void* x, int64_t ldx, float* out, int32_t M, int32_t N, vds_stream_t stream);
/* the same over the token rows only of a [B * rows_per_sample] buffer: rows r with r % rows_per_sample < row_offset
 * (the register rows) are skipped; rows_per_sample = 0: every row */
int vds_colsum_bf16_rows(const void* x, int64_t ldx, float* out, int32_t M, int32_t N, int32_t rows_per_sample,
                         int32_t row_offset, vds_stream_t stream);

/* ----------------------------------------------------- qkv split / RoPE / residual-V --
 * forward of model.py:126-134: qkv [B,L,3D] token-major (k h d) ->
 *   q,k [B,H,L,hdp] rotated (fp32 math, half-split, cos/sin [L, hd/2] f32; model.py:266-275)
 *   v   [B,H,L,hdp] = lam*v_raw + (1-lam)*v0  (model.py:129-130) when v0 != NULL else v_raw.
 * hdp >= hd is the padded row length (pad columns are written as zero, except that with hdp >= hd+8
 * k gets 1.0 at columns hd, hd+1 and v 1.0 at columns hd and hd+4: see vds_attn_args.kv_pad_ones). lam: bf16 device scalar
 * (the bf16-cast lambda_param, as under the reference's bf16 param policy). */
int vds_qkv_rope_fwd(const void* qkv, const float* cosb, const float* sinb, const void* v0,
                     const void* lam, void* q, void* k, void* v, int32_t B, int32_t L, int32_t H,
                     int32_t hd, int32_t hdp, vds_stream_t stream);
/* backward: dq,dk,dv [B,H,L,hdp] -> dqkv [B,L,3D] (un-rotated, dv*lam);
 *   dv0_acc (f32 [B,H,L,hdp]) += (1-lam)*dv  when mix == 1;  dlam (f32 scalar) += sum dv*(v_raw - v0) when mix != 0;
 *   mix == 2 (round 5): as 1 without the dv0_acc update (dv0_acc may be NULL) -- the caller sums the blocks' terms in
 *   one pass with vds_dv0_reduce before block 0's call;
 *   when add_dv0 != 0 (block 0): dv_total = dv + dv0_acc. */
int vds_qkv_rope_bwd(const void* dq, const void* dk, const void* dv, const float* cosb,
                     const float* sinb, const void* qkv_raw, const void* v0, const void* lam,
                     float* dv0_acc, float* dlam, void* dqkv, int32_t mix, int32_t add_dv0, int32_t B,
                     int32_t L, int32_t H, int32_t hd, int32_t hdp, vds_stream_t stream);
/* QK-norm: the two calls above with a weightless RMSNorm on every head row of q and k before the rotation
 * (self-attention only; v, residual-V, the pad and the ones columns are those of the plain calls, bit for bit).
 *   forward:  q_n = bf16(q * rsqrt(mean_d(q^2) + eps)) over the hd data columns (fp32 math), then the rotation of q_n
 *             exactly as in vds_qkv_rope_fwd (fp32 math, one rounding); the same for k.
 *   backward: with g = the inverse rotation of dq (fp32), r recomputed from the raw row of qkv_raw and y = q r (fp32):
 *             dq_raw = bf16(r (g - y mean_d(g y))) -- one rounding, at the store; the same for k.  qkv_raw (the forward's
 *             qkv) is required in every call, not only when mix is set.
 * A zero row gives r = eps^-1/2, output 0 and a finite gradient.  No atomics are added: both calls are as reproducible as
 * the plain ones (dlam: see vds_set_deterministic).  Argument checks and kernel selection (token-tile / wave-per-token form
 * under the same conditions and knobs, the element-wise form otherwise) are those of the plain calls, plus eps > 0 and
 * qkv_raw != NULL (VDS_ERR_ARG).  The plain calls launch none of the normed kernel instances. */
int vds_qkv_rope_norm_fwd(const void* qkv, const float* cosb, const float* sinb, const void* v0,
                          const void* lam, void* q, void* k, void* v, int32_t B, int32_t L, int32_t H,
                          int32_t hd, int32_t hdp, float eps, vds_stream_t stream);
/* Cache forms of the two forwards (inference with a frame KV cache): q as above; the k and v rows of token l go to
 * k / v + b * kv_sb + h * kv_sh + (l < lead ? l : l + past) * kv_sl (strides in elements, multiples of 4, kv_sl >= hdp):
 * their place in a [lead rows | past rows | this call's rows] cache buffer.  v0 (block 0's v, residual-V) is read through
 * the same strides and row map.  Same arithmetic, rounding, pad and ones columns as the plain forms (element-wise
 * kernel).  lead < 0, lead > L or past < 0: VDS_ERR_ARG. */
int vds_qkv_rope_fwd_cache(const void* qkv, const float* cosb, const float* sinb, const void* v0, const void* lam,
                           void* q, void* k, void* v, int64_t kv_sb, int64_t kv_sh, int64_t kv_sl, int32_t lead,
                           int32_t past, int32_t B, int32_t L, int32_t H, int32_t hd, int32_t hdp, vds_stream_t stream);
int vds_qkv_rope_norm_fwd_cache(const void* qkv, const float* cosb, const float* sinb, const void* v0, const void* lam,
                                void* q, void* k, void* v, int64_t kv_sb, int64_t kv_sh, int64_t kv_sl, int32_t lead,
                                int32_t past, int32_t B, int32_t L, int32_t H, int32_t hd, int32_t hdp, float eps,
                                vds_stream_t stream);
int vds_qkv_rope_norm_bwd(const void* dq, const void* dk, const void* dv, const float* cosb,
                          const float* sinb, const void* qkv_raw, const void* v0, const void* lam,
                          float* dv0_acc, float* dlam, void* dqkv, int32_t mix, int32_t add_dv0, int32_t B,
                          int32_t L, int32_t H, int32_t hd, int32_t hdp, float eps, vds_stream_t stream);
/* Frame-major forms of the four calls above (frame-major self-attention).  Every token-major tensor -- qkv, qkv_raw, dqkv
 * and the cos / sin table rows -- keeps the model's (h w t) row order; the head-major tensors q, k, v, dq, dk, dv, v0 and
 * dv0_acc [B,H,L,hdp] are addressed with a frame's rows contiguous.  With frames = {lead, period} (validated against L as
 * vds_mod_groups) and S = (L - lead) / period rows per frame, token row l lives at head row
 *   fm(l) = l                                                        for l < lead,
 *           lead + ((l - lead) % period) * S + (l - lead) / period   otherwise
 * (the inverse: tok(r) = r for r < lead, lead + ((r - lead) % S) * period + (r - lead) / S otherwise).
 *   forward:  token l reads table row l; its q / k / v head rows (pad and ones columns included) are written at row
 *             fm(l), and v0 is read at row fm(l).
 *   backward: dq / dk / dv, v0 and dv0_acc are read (dv0_acc updated, mix == 1) at row fm(l); dqkv row l is written.
 * Arithmetic and rounding points are those of the plain calls: the outputs are the plain calls' outputs with the head rows
 * permuted, bit for bit (dlam under vds_set_deterministic).  The token-tile forward writes one complete head row per
 * (token, tensor, head) instead of a run of T rows, still 16 bytes per lane; the wave-per-token backward maps the row
 * once per token; the element-wise kernels are the fallback under the same conditions and knobs as the plain calls.
 * frames == NULL, a frames that does not fit L, or B, L, H <= 0: VDS_ERR_ARG.  No fp8-emitting form.  The plain calls
 * launch none of the frame-major kernel instances. */
int vds_qkv_rope_fwd_fm(const void* qkv, const float* cosb, const float* sinb, const void* v0,
                        const void* lam, void* q, void* k, void* v, int32_t B, int32_t L, int32_t H,
                        int32_t hd, int32_t hdp, const vds_mod_groups* frames, vds_stream_t stream);
int vds_qkv_rope_norm_fwd_fm(const void* qkv, const float* cosb, const float* sinb, const void* v0,
                             const void* lam, void* q, void* k, void* v, int32_t B, int32_t L, int32_t H,
                             int32_t hd, int32_t hdp, float eps, const vds_mod_groups* frames, vds_stream_t stream);
int vds_qkv_rope_bwd_fm(const void* dq, const void* dk, const void* dv, const float* cosb,
                        const float* sinb, const void* qkv_raw, const void* v0, const void* lam,
                        float* dv0_acc, float* dlam, void* dqkv, int32_t mix, int32_t add_dv0, int32_t B,
                        int32_t L, int32_t H, int32_t hd, int32_t hdp, const vds_mod_groups* frames,
                        vds_stream_t stream);
int vds_qkv_rope_norm_bwd_fm(const void* dq, const void* dk, const void* dv, const float* cosb,
                             const float* sinb, const void* qkv_raw, const void* v0, const void* lam,
                             float* dv0_acc, float* dlam, void* dqkv, int32_t mix, int32_t add_dv0, int32_t B,
                             int32_t L, int32_t H, int32_t hd, int32_t hdp, float eps, const vds_mod_groups* frames,
                             vds_stream_t stream);
/* residual-V (/root/reference/model.py:129-130, backward): out[b,h,l,:hd] (f32 [B,H,L,hdp]; + its old value when
 * accumulate != 0) = sum_i (1 - lam_i) dv_i[b,h,l,:hd] over n blocks.  dv / lam: HOST arrays of n DEVICE pointers (dv_i bf16
 * [B,H,L,hdp] contiguous, 16-byte aligned; lam_i one bf16).  Columns >= hd of out are not touched. */
int vds_dv0_reduce(const void* const* dv, const void* const* lam, int32_t n, float* out, int32_t accumulate, int32_t B,
                   int32_t H, int32_t L, int32_t hd, int32_t hdp, vds_stream_t stream);

/* apply_rotary_emb (model.py:266-275) on its own: y = rotate(x) for x, y [B,H,L,hd] bf16 addressed as
 * base + b*sb + h*sh + l*sl (elements, multiples of 4; rows of hd contiguous), cos / sin f32 [L, hd/2];
 * halves are (x1, x2) = (x[:hd/2], x[hd/2:]): y1 = x1 cos + x2 sin, y2 = x2 cos - x1 sin, fp32 math.
 * inverse != 0 applies the transposed rotation (the backward of the forward).  hd % 8 == 0. */
int vds_rope_apply(const void* x, int64_t x_sb, int64_t x_sh, int64_t x_sl, const float* cos, const float* sin,
                   void* y, int64_t y_sb, int64_t y_sh, int64_t y_sl, int32_t B, int32_t H, int32_t L, int32_t hd,
                   int32_t inverse, vds_stream_t stream);

/* cos/sin rows [n_reg + t*h*w, nt + 2*ns] f32 of ThreeDimRotary.forward (model.py:219-263) for
 * the offsets (st,sh,sw): gathered from the per-axis tables tab_t_* [128, nt], tab_s_* [128, ns]
 * (the factors of the reference's freqs_hwt buffers); register rows are cos=1, sin=0. */
int vds_rope_rows(const float* tab_t_cos, const float* tab_t_sin, const float* tab_s_cos,
                  const float* tab_s_sin, int32_t nt, int32_t ns, int32_t t, int32_t h, int32_t w,
                  int32_t st, int32_t sh, int32_t sw, int32_t n_reg, float* cosb, float* sinb,
                  vds_stream_t stream);

/* the same with the offsets (st, sh, sw) read from device memory (int32[3], clamped to the table): nothing
 * per-step remains in the arguments, so a captured whole-step graph can be replayed */
int vds_rope_rows_dev(const float* tab_t_cos, const float* tab_t_sin, const float* tab_s_cos,
                      const float* tab_s_sin, int32_t nt, int32_t ns, int32_t t, int32_t h, int32_t w,
                      const int32_t* start_dev, int32_t n_reg, float* cosb, float* sinb, vds_stream_t stream);

/* ------------------------------------------------------------- small-M linears (B rows) --
 * y[b, n] = act_out( sum_k act_in(x[b,k]) * W[n,k] + bias[n] ), M = B rows (the per-GPU batch; any M >= 1, run
 * in chunks of <= 16 rows that stay in registers): time_embed / adaLN_modulation / final_modulation
 * (model.py:90,318-322,339-341).  x f32 [M,K]; W bf16 [N,K]; bias bf16 [N]; y f32 [M,N].  act: 0 none, 1 SiLU.
 * Requires M, N >= 1, K >= 8, K % 8 == 0.  x, W, y (and dW below) are read / written in 16-byte pieces: 16-byte aligned
 * pointers; bias (may be NULL) 8-byte aligned; dy, dbias, dx 4-byte aligned.  The batched forms check the pointers they
 * are given directly; the pointers inside the device tables must meet the same rule (they cannot be checked on the
 * host), and y_stride % 4 == 0 when N % 16 == 0.  Anything else is VDS_ERR_ARG before any launch. */
int vds_small_linear_fwd(const float* x, const void* W, const void* bias, float* y, int32_t M,
                         int32_t N, int32_t K, int32_t act_in, vds_stream_t stream);
/* dW[n,k] (f32) = sum_b dy[b,n]*act_in(x[b,k]);  dbias[n] (f32) = sum_b dy[b,n]  (overwritten);
 * dx[b,k] (f32) += act_in'(x[b,k]) * sum_n dy[b,n] W[n,k]   (atomically accumulated: the
 * conditioning vector c collects a gradient from every block).  dW (with it dbias) or dx may be NULL; dbias may be
 * NULL on its own; W may be NULL when dx is (dx without W is VDS_ERR_ARG, and then dW is not written either). */
int vds_small_linear_bwd(const float* dy, const float* x, const void* W, float* dW, float* dbias,
                         float* dx, int32_t M, int32_t N, int32_t K, int32_t act_in,
                         vds_stream_t stream);
/* The same for nb weight sets sharing ONE input x (M <= 16 rows): the adaLN modulation linears of every DiT block
 * (model.py:89-94,107) in one launch instead of one per block.  W_ptrs / bias_ptrs / dW_ptrs / dbias_ptrs: device
 * arrays of nb device pointers (bias_ptrs / dbias_ptrs may be NULL); set i writes y + i * y_stride ([M,N] f32) and
 * reads its output gradient at dy + i * dy_stride; dx (shared, f32 [M,K]) accumulates over all sets. */
int vds_small_linear_fwd_batched(const float* x, const void* const* W_ptrs, const void* const* bias_ptrs, float* y,
                                 int64_t y_stride, int32_t nb, int32_t M, int32_t N, int32_t K, int32_t act_in,
                                 vds_stream_t stream);
int vds_small_linear_bwd_batched(const float* dy, int64_t dy_stride, const float* x, const void* const* W_ptrs,
                                 float* const* dW_ptrs, float* const* dbias_ptrs, float* dx, int32_t nb, int32_t M,
                                 int32_t N, int32_t K, int32_t act_in, vds_stream_t stream);
/* sinusoid [cos | sin](t * f_i), t unscaled (model.py:12-22), rounded through bf16 like
 * the reference's .to(x.dtype): out f32 [B, D].  B >= 1, D >= 2, D % 2 == 0. */
int vds_timestep_embedding(const float* t, float* out, int32_t B, int32_t D, vds_stream_t stream);

/* ------------------------------------------------------------ patchify / unpatchify ---
 * latent [B,C,T,H,W] bf16 -> patches [B*N, C*pt*p*p] bf16, token order (h w t)
 * (Conv3d k=stride + rearrange, model.py:182-186); the GEMM with patch_proj follows.
 * All of patchify / unpatchify: B, C, T, H, W, pt, p >= 1, T % pt == 0, H % p == 0, W % p == 0 (else VDS_ERR_ARG);
 * two-byte accesses only, no alignment beyond bf16's. */
int vds_patchify(const void* latent, void* patches, int32_t B, int32_t C, int32_t T, int32_t H,
                 int32_t W, int32_t pt, int32_t p, vds_stream_t stream);
/* tokens y [B*N, p*p*pt*C] bf16 (p1 p2 p3 c) -> out [B,C,T,H,W] bf16 (model.py:392-401) */
int vds_unpatchify(const void* y, void* out, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W,
                   int32_t pt, int32_t p, vds_stream_t stream);
/* gradient wrt tokens: dy[B*N, P] bf16 from dout [B,C,T,H,W] bf16 (inverse permutation) */
int vds_unpatchify_bwd(const void* dout, void* dy, int32_t B, int32_t C, int32_t T, int32_t H,
                       int32_t W, int32_t pt, int32_t p, vds_stream_t stream);
/* The same three with the tokens addressed as rows of the model's [B * (R + N)] token buffer: token n of sample b
 * is row b * rows_per_sample + row_offset + n (rows_per_sample = R + N, row_offset = R = 16 register tokens,
 * model.py:362,386), so that patch embedding and final layer run as ONE GEMM over all B * L rows instead of one
 * per sample; the R rows in front of every sample are not touched.  rows_per_sample = 0 means N (dense).
 * vds_unpatchify_rows: bwd = 0 tokens -> image, bwd != 0 image gradient -> token-row gradient. */
int vds_patchify_rows(const void* latent, void* patches, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W,
                      int32_t pt, int32_t p, int32_t rows_per_sample, int32_t row_offset, vds_stream_t stream);
int vds_unpatchify_rows(const void* y, void* out, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W,
                        int32_t pt, int32_t p, int32_t rows_per_sample, int32_t row_offset, int32_t bwd,
                        vds_stream_t stream);
/* x[b, 0:R] = reg[0:R] ; used to prepend the 16 register tokens (model.py:362).  x holds sample b at
 * x + b * batch_stride (elements); B, R, D >= 1 and batch_stride >= R * D, here and in vds_registers_bwd. */
int vds_fill_registers(const void* reg, void* x, int64_t batch_stride, int32_t B, int32_t R,
                       int32_t D, vds_stream_t stream);
/* dreg[r,d] (f32) += sum_b dx[b, r, d] */
int vds_registers_bwd(const void* dx, int64_t batch_stride, float* dreg, int32_t B, int32_t R,
                      int32_t D, vds_stream_t stream);

/* ------------------------------------------------------------ noising + loss (train.py) --
 * z_t = x(1-t) + n t ; v = x - n  in bf16 (train.py:115-117); t f32 [B] already bf16-rounded.
 * B >= 1, per_sample >= 1; element-wise accesses, no alignment beyond the types'. */
int vds_noise_latents(const void* x, const void* noise, const float* t, void* z_t, void* v,
                      int32_t B, int64_t per_sample, vds_stream_t stream);
/* the same with one noise level per token-frame: x [B,C,T,HW] bf16, t f32 [B, T / time_patch] (bf16-rounded values);
 * latent frame j of sample b uses t[b, j / time_patch].  T % time_patch == 0. */
int vds_noise_latents_frames(const void* x, const void* noise, const float* t, void* z_t, void* v, int32_t B,
                             int32_t C, int32_t T, int64_t HW, int32_t time_patch, vds_stream_t stream);
/* loss = mean_b mean_chw (v - out)^2 in f32 (train.py:121-125), as a FIXED-ORDER two-stage reduction (per-workgroup
 * partial sums -> one pass that sums a sample's partials, divides by per_sample_n, then sums the samples in index order
 * and divides by B): loss_out[0] and per_sample[b] are WRITTEN (no pre-zeroing), bit-identical run to run, and a batch of
 * identical samples gives the single-sample loss to the bit.  workspace: vds_flow_loss_workspace_floats(B, per_sample_n)
 * floats, caller-allocated, contents irrelevant.  dout (may be NULL) = bf16( 2 (out - v) * gscale/(B*per_sample_n) ). */
int64_t vds_flow_loss_workspace_floats(int32_t B, int64_t per_sample_n);
int vds_flow_loss(const void* v, const void* out, float* loss_out, float* per_sample, void* dout,
                  float gscale, int32_t B, int64_t per_sample_n, float* workspace, vds_stream_t stream);
/* its backward for an arbitrary upstream gradient (autograd of train.py:121-125 under `(loss * s).backward()`,
 * loss scaling, micro-batch accumulation): dout = bf16( 2 (out - v) * *gloss_dev / (B*per_sample) ), the upstream
 * scalar read from device memory (no host synchronisation; graph-capturable).  B, per_sample >= 1,
 * B*per_sample % 8 == 0; v, out and dout are read / written in 16-byte pieces: 16-byte aligned pointers. */
int vds_flow_loss_bwd(const void* v, const void* out, const float* gloss_dev, void* dout, int32_t B,
                      int64_t per_sample_n, vds_stream_t stream);

/* Frame-weighted loss over [B,C,T,HW] with w f32 [B, F], F = T / time_patch, w >= 0:
 *   per_sample[b] = sum_f w[b,f] SSE[b,f] / (n_f * sum_f w[b,f]),  n_f = C * time_patch * HW elements per token-frame,
 *   loss = mean_b per_sample[b];  sum_f w[b,f] == 0: per_sample[b] = 0 and dout = 0 for that sample (no NaN).
 * The same fixed-order two-stage reduction (one partial per workgroup of a (sample, frame), then lanes / butterfly /
 * frames / samples in index order): bit-identical run to run; w = 1 is vds_flow_loss up to fp32 summation order.
 * workspace: vds_flow_loss_frames_workspace_floats(B, F, n_f) floats.  dout (may be NULL) =
 * bf16( 2 (out - v) * gscale * w[b,f] / (B * n_f * sum_f w[b,f]) ), exact zeros where the factor is zero. */
int64_t vds_flow_loss_frames_workspace_floats(int32_t B, int32_t F, int64_t n_f);
int vds_flow_loss_frames(const void* v, const void* out, const float* w, float* loss_out, float* per_sample,
                         void* dout, float gscale, int32_t B, int32_t C, int32_t T, int64_t HW, int32_t time_patch,
                         float* workspace, vds_stream_t stream);
/* its backward for an upstream gradient in device memory (as vds_flow_loss_bwd): dout with gscale = *gloss_dev */
int vds_flow_loss_frames_bwd(const void* v, const void* out, const float* w, const float* gloss_dev, void* dout,
                             int32_t B, int32_t C, int32_t T, int64_t HW, int32_t time_patch, vds_stream_t stream);

/* ------------------------------------------------------------ sampler --
 * One Euler step of sampling/sample.py:139-146:  out = uncond + cfg_scale*(cond - uncond) in bf16
 * (uncond may be NULL: out = cond), acc (f32) += dt * out, latents = bf16(acc).  n >= 8, n % 8 == 0; cond, uncond,
 * acc and latents are read / written in 16-byte pieces: 16-byte aligned pointers. */
int vds_cfg_euler_step(const void* cond, const void* uncond, float* acc, void* latents, float cfg_scale,
                       float dt, int64_t n, vds_stream_t stream);

/* -------------------------------------------------------------------- optimizer ------
 * Multi-tensor AdamW on fp32 master shards (torch.optim.AdamW(fused=True) semantics,
 * train.py:340-344,433) + bf16 shadow copy for the next all-gather.
 * desc: one vds_adamw_tensor per parameter (device array). */
typedef struct vds_adamw_tensor {
  float* p; const float* g; float* m; float* v; void* p_bf16; int64_t numel; float lr; float wd;
} vds_adamw_tensor;
/* work list: chunk i updates elements [chunk_start[i], chunk_start[i]+chunk_elems) of tensor
 * chunk_tensor[i]; lr_mult is the LR-schedule multiplier of this step (train.py:349-364,434),
 * step counts from 1, grad_scale multiplies every gradient (1.0 normally).  chunk_elems >= 4, any value.
 * Alignment: every pointer needs only its natural alignment (4 bytes, 2 for the shadow).  A chunk takes the 16-byte
 * path only when ALL of p, g, m, v (and the EMA of the guarded form, where present) are 16-byte aligned at the chunk's
 * first element and p_bf16, where present, is 8-byte aligned there; otherwise it is served element by element.  The
 * results are the same bits either way. */
int vds_adamw_multi(const vds_adamw_tensor* desc_dev, const int32_t* chunk_tensor_dev,
                    const int64_t* chunk_start_dev, int32_t n_chunks, int32_t chunk_elems,
                    float beta1, float beta2, float eps, int32_t step, float lr_mult,
                    float grad_scale, vds_stream_t stream);

/* the same with the per-step scalars in device memory: scalars_dev = { 1 - beta1^step, 1/sqrt(1 - beta2^step),
 * lr_mult } (graph replay: the host refreshes them with a copy before each replay) */
int vds_adamw_multi_dev(const vds_adamw_tensor* desc_dev, const int32_t* chunk_tensor_dev,
                        const int64_t* chunk_start_dev, int32_t n_chunks, int32_t chunk_elems, float beta1,
                        float beta2, float eps, const float* scalars_dev, float grad_scale, vds_stream_t stream);

/* ---- guarded step: global-norm clip, non-finite skip, weight EMA -- all decided on the device (no host
 * synchronisation: the sequence below replays from a captured graph).
 *
 *   vds_grad_sumsq_multi      sum of squares of every gradient element of the chunk table   (+ finalize at world 1)
 *   [all-reduce(sum) of that one float over the shard group, then vds_optim_guard_finalize -- sharded runs only]
 *   vds_adamw_guarded_multi   the AdamW launch, reading the record
 *
 * The record the finalize leaves in device memory (caller-allocated, zeroed once; n_skipped accumulates): */
typedef struct vds_optim_guard {
  float norm;        /* global L2 norm of the gradients before clipping */
  float coef;        /* what the step multiplies the gradients by: min(1, max_norm / (norm + 1e-6)), the arithmetic of
                        torch.nn.utils.clip_grad_norm_; 1 when clipping is off */
  int32_t skipped;   /* 1 = this step is skipped (norm not finite and skip_nonfinite set), 0 = applied */
  int32_t n_skipped; /* running count of skipped steps */
} vds_optim_guard;
/* FIXED-ORDER two-stage reduction over the descriptor / chunk tables of vds_adamw_multi (only desc[i].g and .numel are
 * read): one workgroup per chunk writes one fp32 partial into `workspace` (vds_grad_sumsq_workspace_floats(n_chunks)
 * floats, caller-allocated, contents irrelevant), one workgroup adds the partials in index order and WRITES
 * sumsq_out[0].  No floating-point atomics: bit-identical run to run, with or without vds_set_deterministic.  With
 * guard != NULL the second stage also finalizes (below) from that sum -- the world-size-1 form, one launch fewer.
 * max_norm <= 0 = clipping off; +inf is legal and gives coef == 1 exactly. */
int64_t vds_grad_sumsq_workspace_floats(int32_t n_chunks);
int vds_grad_sumsq_multi(const vds_adamw_tensor* desc_dev, const int32_t* chunk_tensor_dev,
                         const int64_t* chunk_start_dev, int32_t n_chunks, int32_t chunk_elems, float* workspace,
                         float* sumsq_out, float max_norm, int32_t skip_nonfinite, vds_optim_guard* guard_or_null,
                         vds_stream_t stream);
/* norm = sqrt(sumsq_dev[0] * sumsq_scale) (sumsq_scale: `world` after an averaging all-reduce, 1 after a sum), then
 * coef / skipped / n_skipped as described at vds_optim_guard; ordinary stores of one thread. */
int vds_optim_guard_finalize(const float* sumsq_dev, float sumsq_scale, float max_norm, int32_t skip_nonfinite,
                             vds_optim_guard* guard, vds_stream_t stream);
/* vds_adamw_multi / vds_adamw_multi_dev with the record: every gradient is multiplied by grad_scale * guard->coef;
 * when guard->skipped every workgroup returns before its first store (p, m, v, the bf16 shadow and the EMA keep every
 * bit).  ema_tab_dev (may be NULL = no EMA): device array of one fp32 pointer per descriptor (NULL entries allowed),
 * parallel to desc_dev -- vds_adamw_tensor keeps its 56 bytes; ema = d * ema + (1 - d) * p_new in the same pass.
 * d: ema_decay in [0, 1), or scalars_dev[3] for the _dev form (scalars_dev = { 1 - beta1^step,
 * 1/sqrt(1 - beta2^step), lr_mult, ema_decay }: changing it between replays needs no new capture). */
int vds_adamw_guarded_multi(const vds_adamw_tensor* desc_dev, const int32_t* chunk_tensor_dev,
                            const int64_t* chunk_start_dev, int32_t n_chunks, int32_t chunk_elems, float beta1,
                            float beta2, float eps, int32_t step, float lr_mult, float grad_scale,
                            const vds_optim_guard* guard, float* const* ema_tab_dev, float ema_decay,
                            vds_stream_t stream);
int vds_adamw_guarded_multi_dev(const vds_adamw_tensor* desc_dev, const int32_t* chunk_tensor_dev,
                                const int64_t* chunk_start_dev, int32_t n_chunks, int32_t chunk_elems, float beta1,
                                float beta2, float eps, const float* scalars_dev, float grad_scale,
                                const vds_optim_guard* guard, float* const* ema_tab_dev, vds_stream_t stream);

/* ---- Muon for the 2-D hidden matrices: momentum, orthogonalised by a Newton-Schulz iteration (csrc/muon.hip; the
 * reference knows AdamW only).  Every call works on a GROUP of nmat matrices of ONE shape [rows, cols] (row-major fp32,
 * contiguous), each given by one descriptor of a device array -- the row slices of qkv.weight / context_kv.weight are
 * matrices at pointer offsets.  rows, cols: multiples of 8, <= 2^20, rows * cols <= 2^28; 1 <= nmat <= 65535; anything
 * else is VDS_ERR_ARG.  The three calls share one caller-allocated workspace of vds_muon_workspace_bytes(nmat, rows,
 * cols) bytes (16-byte aligned; contents irrelevant before vds_muon_momentum; 0 for a bad shape) in which a matrix is
 * held as bf16 [m, n], m = min(rows, cols), n = max(rows, cols): transposed on the way in and back on the way out when
 * rows > cols.  All launches go to `stream`, nothing is read on the host, no atomics and no split-K: results are
 * bit-identical run to run, in either deterministic mode.
 *
 *   vds_muon_momentum       g' = coef g;  buf = mu buf + g';  u = nesterov ? g' + mu buf : buf  (fp32), u stored as bf16
 *                           [nmat, m, n], and sum u^2 per matrix left in the workspace by a fixed-order two-stage
 *                           reduction.  guard (may be NULL: coef = 1, never skipped): the record of
 *                           vds_optim_guard_finalize; coef = guard->coef, and with guard->skipped nothing is written
 *                           (buf keeps every bit).  0 <= mu < 1.
 *   vds_muon_orthogonalize  X = u / (||u||_F + 1e-7), then `steps` (0 .. 64; Muon uses 5) times  A = X X^T,
 *                           B = b A + c A A,  X = a X + B X  with (a, b, c) = (3.4445, -4.7750, 2.0315); X, A, B stored as
 *                           bf16, fp32 accumulation on the MFMA.  The result O replaces u.
 *   vds_muon_update         p = p (1 - lr wd) - lr sqrt(max(1, rows / cols)) O;  p_bf16 = bf16(p) and
 *                           ema = d ema + (1 - d) p where the descriptor has them.  lr = the base `lr` x lr_mult, d =
 *                           ema_decay; with scalars_dev != NULL (the float[4] of vds_adamw_guarded_multi_dev) lr_mult =
 *                           scalars_dev[2] and d = scalars_dev[3] instead, so that a captured step follows the schedule.
 *                           With guard->skipped nothing is written. */
typedef struct vds_muon_mat {
  float* p; const float* g; float* buf; void* p_bf16; float* ema; /* p_bf16, ema: may be NULL */
} vds_muon_mat;
size_t vds_muon_workspace_bytes(int32_t nmat, int32_t rows, int32_t cols);
/* byte offsets of the workspace's sections (tests, tools): offsets6 = HOST int64[6] = { x0, x1, a, b, sumsq, partials }:
 * x0 / x1 bf16 [nmat, m, n] (x0: u after the momentum call, O after the orthogonalisation), a / b bf16 [nmat, m, m],
 * sumsq f32 [nmat], partials f32 [nmat, ceil(rows / 64) * ceil(cols / 64)] */
int vds_muon_workspace_layout(int32_t nmat, int32_t rows, int32_t cols, int64_t* offsets6);
int vds_muon_momentum(const vds_muon_mat* mats_dev, int32_t nmat, int32_t rows, int32_t cols, float mu,
                      int32_t nesterov, const vds_optim_guard* guard_or_null, void* workspace, vds_stream_t stream);
int vds_muon_orthogonalize(void* workspace, int32_t nmat, int32_t rows, int32_t cols, int32_t steps,
                           vds_stream_t stream);
int vds_muon_update(const vds_muon_mat* mats_dev, int32_t nmat, int32_t rows, int32_t cols, float lr,
                    float weight_decay, float lr_mult, float ema_decay, const float* scalars_dev,
                    const vds_optim_guard* guard_or_null, const void* workspace, vds_stream_t stream);

/* ------------------------------------------- parameter / gradient sharding (model.py:512-542) ------
 * What the reference gets from FSDP2 `fully_shard` (apply_fsdp, model.py:512-542; mesh model.py:475-498): a bf16
 * all-gather of a shard group's parameters before use and an fp32 reduce-scatter-AVERAGE of its gradients after its
 * backward (MixedPrecisionPolicy(bf16, fp32), model.py:516-519), here straight on RCCL over xGMI, one process per
 * GPU, ONE collective per flat group buffer.  RCCL is bound at run time (dlopen of librccl.so.1; VDS_RCCL_PATH
 * overrides), so the library loads without it and these calls return VDS_ERR_UNSUPPORTED when it is missing.
 *
 *   rank 0:  vds_comm_unique_id(id, 128)  -> ship the 128 bytes to every rank (any host channel)
 *   all:     vds_comm_init(rank, world, id, 128)     on the calling thread's current HIP device
 *   per step and group:  vds_all_gather_bf16 / vds_reduce_scatter_f32_avg on the caller's communication stream
 *   end:     vds_comm_destroy()
 *
 * One communicator per process (the only global mutable state of the library).  All collectives are asynchronous
 * on `stream`; every rank must issue the same sequence.  shard_elems = elements per rank; the full buffer is
 * world * shard_elems, rank r's part at offset r * shard_elems (in-place allowed: shard == full + rank*shard_elems).
 * VDS_COMM_SCHEDULE=allpairs (read by vds_comm_init) switches the reduce-scatter from RCCL's algorithm to an explicit
 * all-pairs exchange over the point-to-point xGMI mesh (one ncclSend/ncclRecv per peer + a local averaging kernel
 * with a fixed summation order); it needs vds_reduce_scatter_workspace_bytes(shard_elems) bytes of caller memory. */
#define VDS_COMM_ID_BYTES 128
int vds_comm_available(void); /* VDS_OK when RCCL could be bound (local, no communication): every rank checks this and
                                 the ranks agree on it BEFORE any of them enters the collective vds_comm_init */
int vds_comm_unique_id(void* out, size_t bytes);
int vds_comm_init(int32_t rank, int32_t world, const void* unique_id, size_t bytes);
int vds_comm_info(int32_t* rank, int32_t* world, int32_t* rccl_version, int32_t* allpairs); /* NULLs allowed */
int vds_comm_destroy(void);
int vds_all_gather_bf16(const void* shard, void* full, int64_t shard_elems, vds_stream_t stream);
int vds_all_gather_f32(const float* shard, float* full, int64_t shard_elems, vds_stream_t stream); /* fp32 masters: checkpoints */
size_t vds_reduce_scatter_workspace_bytes(int64_t shard_elems); /* 0 unless the all-pairs schedule is on */
int vds_reduce_scatter_f32_avg(const float* full, float* shard, int64_t shard_elems, void* workspace,
                               size_t ws_bytes, vds_stream_t stream);
/* the local half of the all-pairs schedule: out[i] = (sum over ranks r of chunk_r[i]) / world in rank order, where
 * chunk_rank = own[n] and the other world-1 chunks lie in staged[(world-1) * n] in increasing rank order.  n % 4 == 0. */
int vds_average_chunks_f32(const float* own, const float* staged, float* out, int64_t n, int32_t world,
                           int32_t rank, vds_stream_t stream);
/* utils.py:11-15 avg_scalar_across_ranks (loss logging): buf[i] = mean over ranks, in place */
int vds_all_reduce_f32_avg(float* buf, int64_t n, vds_stream_t stream);
/* buf[i] = sum over ranks, in place (the guarded optimizer step: every gradient element is owned by one rank, so the
 * squared global norm is the sum of the ranks' local sums of squares) */
int vds_all_reduce_f32_sum(float* buf, int64_t n, vds_stream_t stream);

/* f32 -> bf16 cast (FSDP param_dtype cast before all-gather, model.py:516-518), round to nearest even.  n >= 0 (0: no
 * launch).  Serves ANY naturally aligned pointers (optimizer shards start anywhere): 16-byte accesses when src and dst
 * are both 16-byte aligned, one element per thread otherwise -- the same bits either way. */
int vds_cast_f32_bf16(const float* src, void* dst, int64_t n, vds_stream_t stream);
/* bf16 -> f32 */
int vds_cast_bf16_f32(const void* src, float* dst, int64_t n, vds_stream_t stream);

/* ------------------------------------------------ fp8 attention (BASELINE config 5) -------
 * F.scaled_dot_product_attention (model.py:136) and its backward on v_mfma_f32_16x16x128_f8f6f4: Q / K / V / P in
 * OCP e4m3, dO / dS in e5m2, fp32 accumulation and softmax statistics (csrc/attention_fp8.hip; recipe: fp8.py).  The
 * reference trains in bf16 only.  q, k, v, d_o: fp8 rows [B,H,L,128] (contiguous; bytes [0, head_dim) data, byte
 * head_dim of every V row = 1.0 (0x38), all other pad bytes 0) as written by vds_qkv_rope_fwd_fp8 / vds_attn_fp8_delta;
 * deq: device float[8] = {s_q, s_k, s_v, s_do, E, -, -, -}: dequantisation factors (x = x_q * s) and the exponent E with
 * s_q s_k log2(e) / sqrt(head_dim) = 2^-E exactly (the kernels' block-scaled MFMAs rely on it), written by the same two
 * producers.
 * o: bf16, last dim contiguous; lse f32 [B,H,Lq]; dq, dk, dv: bf16 strided like attention's.  Alignment contract of the
 * bf16 outputs (o, dq, dk, dv): strides multiples of 4 elements and 8-byte aligned bases (else VDS_ERR_ARG); when the
 * strides are multiples of 8 elements on a 16-byte aligned base the rows leave with 16-byte stores (faster; same bits).
 * The fp8 outputs o_q / dq_q (below): base and row stride multiples of 8 bytes (else VDS_ERR_ARG).
 * stats: the f32 [2,B,H,Lq] workspace vds_attn_fp8_delta filled (vds_attn_fp8_bwd_workspace_bytes).  head_dim 72. */
typedef struct vds_attn_fp8_args {
  int32_t B, H, Lq, Lk, head_dim;
  const void* q; const void* k; const void* v;
  void* o; int64_t o_sb, o_sh, o_sl;
  float* lse;
  const void* d_o;
  void* dq; int64_t dq_sb, dq_sh, dq_sl;
  void* dk; int64_t dk_sb, dk_sh, dk_sl;
  void* dv; int64_t dv_sb, dv_sh, dv_sl;
  const float* stats;
  const float* deq;
  /* round 4, optional (NULL = off): fp8 copies written by the kernels' epilogues in the layout of the following
   * linear layer's operand -- token-major [B*Lq, H*head_dim] bytes, row stride *_ld bytes -- so that no quantisation
   * pass reads the bf16 tensor back.  vds_attn_fp8_fwd: o_q = O as e4m3; vds_attn_fp8_bwd: dq_q = dQ as e5m2 (dq may
   * then be NULL: no bf16 dQ is written).  Values are the bf16-rounded results scaled by fmax / *e_amax_prev (delayed
   * scaling, saturating; 0 = unscaled), *e_dq_out = the dequantisation factor, *e_amax_cur = max(*e_amax_cur, max |x|). */
  void* o_q; int64_t o_q_ld;
  void* dq_q; int64_t dq_q_ld;
  const float* e_amax_prev; float* e_amax_cur; float* e_dq_out;
} vds_attn_fp8_args;
int vds_attn_fp8_supported(int32_t head_dim); /* 1 / 0 */
int vds_attn_fp8_fwd(const vds_attn_fp8_args* a, vds_stream_t stream);
size_t vds_attn_fp8_bwd_workspace_bytes(const vds_attn_fp8_args* a);
/* backward preprocess over the token-major bf16 O / dO ([B*Lq, H*head_dim], row strides o_sl / do_sl, batch strides
 * o_sb / do_sb, in elements): stats (see above), dO as e5m2 rows into doq ([B,H,Lq,128], pad bytes left untouched: zero
 * the buffer once), scaled by the previous step's amax (*amax_prev; 0 = unscaled) with the current one accumulated
 * into *amax_cur; writes deq[3] and reads deq[2]. */
int vds_attn_fp8_delta(const void* o, int64_t o_sb, int64_t o_sl, const void* d_o, int64_t do_sb, int64_t do_sl,
                       const float* lse, float* stats, void* doq, const float* amax_prev, float* amax_cur, float* deq,
                       int32_t B, int32_t H, int32_t Lq, int32_t head_dim, vds_stream_t stream);
int vds_attn_fp8_bwd(const vds_attn_fp8_args* a, vds_stream_t stream);
/* vds_qkv_rope_fwd with fp8 outputs (the values quantised are that kernel's bf16 results): q8 / k8 / v8 e4m3 rows
 * [B,H,L,128]; v_out (may be NULL): additionally the bf16 v in the padded head-major layout [B,H,L,hdp]; amax_prev /
 * amax_cur: the q, k, v amax entries at element stride amax_stride (delayed scaling: scale = 448 / previous amax);
 * writes deq[0..2] and deq[4] (q's factor is tied to k's: see deq above). */
int vds_qkv_rope_fwd_fp8(const void* qkv, const float* cosb, const float* sinb, const void* v0, const void* lam,
                         void* q8, void* k8, void* v8, void* v_out, const float* amax_prev, float* amax_cur,
                         int32_t amax_stride, float* deq, int32_t B, int32_t L, int32_t H, int32_t hd, int32_t hdp,
                         vds_stream_t stream);
/* The operands of cross-attention (model.py:146-157) as fp8 rows for vds_attn_fp8_*: q = the q_cross output
 * [B*Lq, H*hd] bf16 (contiguous) -> q8 [B,H,Lq,128]; kv = the context_kv output [B*Lk, 2*H*hd] (k columns, then v
 * columns) -> k8, v8 [B,H,Lk,128] with V's ones byte.  No rotation, no residual-V.  amax_prev / amax_cur / deq as in
 * vds_qkv_rope_fwd_fp8 (deq[0..2], deq[4]).  head_dim 72. */
int vds_cross_qkv_fp8(const void* q, const void* kv, void* q8, void* k8, void* v8, const float* amax_prev,
                      float* amax_cur, int32_t amax_stride, float* deq, int32_t B, int32_t Lq, int32_t Lk, int32_t H,
                      int32_t hd, vds_stream_t stream);

/* ------------------------------------------------------- low-rank adapters (LoRA) ----
 * The three tall-skinny products of y += s (x A^T) B^T and its backward (csrc/lowrank.hip).  Operands bf16,
 * accumulation fp32, no atomics: results are bit-identical run to run, with or without vds_set_deterministic.
 * r in {16, 32, 64}.  Every ld and the row widths K / N are multiples of 8 elements and every bf16 / workspace pointer
 * is 16-byte aligned, so every access is a 16-byte row segment; ld may exceed the row width (windows of wider parents;
 * nothing outside the window is read or written).  NULL pointers, non-positive sizes, another r or layout, a misaligned
 * or too small ld, a misaligned pointer or a short workspace: VDS_ERR_ARG before any launch.  The launches are credited
 * to no profiler class.
 *
 * u[m, j] = bf16(scale * sum_k x[m, k] w(j, k)),  x [M, K], u [M, r].
 *   w_layout 0: w is [r, K] (the adapter's A: u = s x A^T);  1: w is [K, r] (the adapter's B, contracted over its
 *   rows: dU = s dY B).  x is read once; w is staged in LDS in chunks of vds_lowrank_chunk(0, r) elements of K. */
int vds_lowrank_down(const void* x, int64_t ldx, const void* w, int64_t ldw, int32_t w_layout, void* u, int64_t ldu,
                     int32_t M, int32_t K, int32_t r, float scale, vds_stream_t stream);
/* y[m, n] = bf16(fma(scale, sum_j u[m, j] w(n, j), float(y[m, n]))), in place: one read and one write of y [M, N].
 *   w_layout 0: w is [N, r] (B: y += s u B^T);  1: w is [r, N] (A: dx += dU A).  A workgroup covers 128 rows and
 *   vds_lowrank_chunk(1, r) columns. */
int vds_lowrank_up_add(const void* u, int64_t ldu, const void* w, int64_t ldw, int32_t w_layout, void* y, int64_t ldy,
                       int32_t M, int32_t N, int32_t r, float scale, vds_stream_t stream);
/* g(n, j) = fma(scale, sum_m a[m, n] u[m, j], g(n, j)) in fp32,  a [M, N], u [M, r].
 *   g_layout 0: g is [N, r] (dB from dY and U);  1: g is [r, N] (dA from x and dU); ldg its row stride in floats.
 * The sum over m is split into chunks of VDS_LOWRANK_WGRAD_CHUNK rows, one fp32 partial [N, r] per chunk in ws
 * (vds_lowrank_wgrad_workspace_floats(M, N, r) floats); a second kernel adds the partials in chunk order.  a is read
 * once. */
#define VDS_LOWRANK_WGRAD_CHUNK 2048
int64_t vds_lowrank_wgrad_workspace_floats(int32_t M, int32_t N, int32_t r);
int vds_lowrank_wgrad(const void* a, int64_t lda, const void* u, int64_t ldu, float* g, int64_t ldg, int32_t g_layout,
                      int32_t M, int32_t N, int32_t r, float scale, float* ws, int64_t ws_floats, vds_stream_t stream);
/* the chunk sizes above for rank r (0 for another r): which = 0 K chunk of down, 1 column chunk of up_add, 2 row chunk
 * of wgrad -- what a test needs to place its shapes across the boundaries */
int32_t vds_lowrank_chunk(int32_t which, int32_t r);

/* ------------------------------------------------- head RMS-norm (QK-norm in cross-attention) ----
 * The weightless RMSNorm of QK-norm on head rows outside the qkv / RoPE kernels (csrc/headnorm.hip), in place: the
 * q_cross output and the k columns of the context_kv output.  The operand is a window [M, H * hd] of a bf16 parent with
 * a row stride of ld elements; head h of row m sits at columns h * hd .. h * hd + hd - 1.  fp32 math, no atomics: results
 * are bit-identical run to run, with or without vds_set_deterministic.  hd is a multiple of 8 up to 128, every ld a
 * multiple of 8 and at least H * hd, every bf16 pointer 16-byte aligned (every access to the rows is a 16-byte row
 * segment; nothing outside the window is read or written), rstd 4-byte aligned, H at most 65536.  NULL pointers,
 * non-positive sizes, another hd, a misaligned or too small ld, a misaligned pointer, eps <= 0 or not finite:
 * VDS_ERR_ARG before any launch.  The launches are credited to no profiler class.
 *
 * forward:  r = rsqrt(mean_d(float(x)^2) + eps);  x[m, h, :] = bf16(float(x[m, h, :]) * r);  rstd[m * H + h] = r.
 *   One rounding, the one of vds_qkv_rope_norm_fwd's normed rows.  A zero row: r = rsqrt(eps), output 0. */
int vds_head_rmsnorm_fwd(void* x, int64_t ldx, float* rstd, int32_t M, int32_t H, int32_t hd, float eps,
                         vds_stream_t stream);
/* backward: y = the forward's output rows, rstd = the forward's;  with g = float(dy), yf = float(y), r = rstd[m * H + h]:
 *   dy[m, h, :] = bf16(r * (g - yf * mean_d(g * yf))), rounded once.  The raw rows are not needed. */
int vds_head_rmsnorm_bwd(void* dy, int64_t lddy, const void* y, int64_t ldy, const float* rstd, int32_t M, int32_t H,
                         int32_t hd, vds_stream_t stream);

/* ------------------------------------------------- row movers of token routing (csrc/route.hip) ----
 * A routed span of DiT blocks runs on a subset of the sequence's rows (DiT.enable_token_routing): rows are picked out of
 * [outer, n, row] tensors by an int32 index table ON THE DEVICE (read by the kernel, never by the host: the launches can
 * be captured in a graph) and put back through its inverse.  Whole rows move in 16-byte pieces; HBM-bound.  No atomics,
 * no workspace: results are bit-identical run to run, with or without vds_set_deterministic.  Every data pointer is
 * 16-byte aligned, every table 4-byte aligned, row_bytes a positive multiple of 16.  NULL or misaligned pointers, another
 * row_bytes, outer <= 0 or a negative count: VDS_ERR_ARG before any launch; rows of 2 GiB or more, or more than 2^31 - 1
 * workgroups of 1024 pieces per outer slice: VDS_ERR_UNSUPPORTED.  The launches are credited to no profiler class.
 *
 * dst[o, i, :] = src[o, idx[i], :]   o < outer, i < n_out; src is [outer, n_in, row_bytes], dst [outer, n_out, row_bytes].
 * idx int32[n_out]; duplicates allowed; dst must not overlap src.  An index outside [0, n_in) reads nothing: its dst row
 * is written as zeros.  n_in > 0; n_out == 0: VDS_OK, nothing is launched. */
int vds_rows_gather(const void* src, void* dst, const int32_t* idx, int32_t outer, int32_t n_in, int32_t n_out,
                    int64_t row_bytes, vds_stream_t stream);
/* dst[o, l, :] = (0 <= inv[l] < n_part) ? part[o, inv[l], :] : full[o, l, :]   l < n_full; inv int32[n_full].
 * dst == full is allowed (every piece is read and written by the same thread; the rows that take no part row are then
 * left untouched); dst must not overlap part.  n_full > 0; n_part == 0: VDS_OK, nothing is launched and dst is not
 * written (with dst != full the copy of `full` is the caller's). */
int vds_rows_merge(const void* full, const void* part, void* dst, const int32_t* inv, int32_t outer, int32_t n_full,
                   int32_t n_part, int64_t row_bytes, vds_stream_t stream);
/* acc[o, idx[i], :] += part[o, i, :]   fp32, one add per element; part is [outer, n_part, row_elems], acc [outer, n_full,
 * row_elems], row_elems a positive multiple of 4.  idx int32[n_part] must be distinct (the caller's contract: a plain
 * read-add-write, no atomics).  An index outside [0, n_full) is skipped.  n_full > 0; n_part == 0: VDS_OK, no launch. */
int vds_rows_scatter_add_f32(const float* part, float* acc, const int32_t* idx, int32_t outer, int32_t n_full,
                             int32_t n_part, int32_t row_elems, vds_stream_t stream);

/* ------------------------------------------------------------------ live profiling ----
 * Per-kernel-class timing with HIP events recorded on the launch stream around each launch of
 * an enabled class (bench.py's roofline leg).  Off by default (no events, no overhead).
 * vds_prof_collect synchronises the recorded events, sums them per class and resets.
 * flops / bytes are the ALGORITHMIC work of the recorded launches (per kernel). */
enum { VDS_PROF_GEMM_NT = 0, VDS_PROF_GEMM_NN, VDS_PROF_GEMM_TN, VDS_PROF_ATTN_FWD, VDS_PROF_ATTN_BWD_DELTA,
       VDS_PROF_ATTN_BWD_DKV, VDS_PROF_ATTN_BWD_DQ, VDS_PROF_RMSNORM_FWD, VDS_PROF_RMSNORM_BWD, VDS_PROF_ADAMW,
       VDS_PROF_QKV_ROPE_FWD, VDS_PROF_QKV_ROPE_BWD, VDS_PROF_GATE_BWD,
       /* the attention kernel instances without the ones-column contract (cross-attention, hd 64/128) */
       VDS_PROF_ATTN_FWD_PLAIN, VDS_PROF_ATTN_BWD_DKV_PLAIN, VDS_PROF_ATTN_BWD_DQ_PLAIN, VDS_PROF_GEMM_FP8,
       VDS_PROF_ATTN_FP8_FWD, VDS_PROF_ATTN_FP8_DKV, VDS_PROF_ATTN_FP8_DQ,
       VDS_PROF_FP8_QUANT, /* vds_quant_fp8 / vds_transpose_fp8 / vds_absmax: the fp8 path's separate operand passes */
       VDS_PROF_NCLASS };
typedef struct vds_prof_stat { int64_t launches; double ms; double flops; double bytes; } vds_prof_stat;
int vds_prof_enable(uint32_t class_mask);
int vds_prof_collect(vds_prof_stat* out /* [VDS_PROF_NCLASS] */);
const char* vds_prof_class_name(int cls);

/* hardware self-test of the MFMA / LDS-transpose / LDS-DMA lane maps the kernels rely on.
 * scratch_dev: >= 2080 bytes of device memory; int32[8] mismatch counts are left at byte
 * offset 2048 (all zero = every map as assumed). */
int vds_selftest_lanemaps(void* scratch_dev, vds_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VDS_H */
