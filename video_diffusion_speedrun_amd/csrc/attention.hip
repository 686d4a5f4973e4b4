// Flash-style full (non-causal) attention for gfx950, forward and backward, bf16 in /
// fp32 softmax, head_dim 32 / 64 / 72 / 96 / 128 (72 = DiT-XL, padded to 80 for the QK contraction and
// to 96 for the 32-wide output blocks).  Replaces F.scaled_dot_product_attention at
// model.py:136 (self, L x L) and model.py:157 (cross, L x 512) and its autograd backward.
//
// All three kernels are built from two MFMA product forms on v_mfma_f32_32x32x16_bf16:
//   F1  X[r, c]   = sum_k A[r,k] B[c,k]      both operands row-major, 16-B fragment reads
//   F2  Y^T[d, c] = sum_r T[r,d] X[r,c]      X = a previous accumulator used in place as the
//                                            B operand (its row index is the contraction),
//                                            T^T read from a row-major LDS tile with the
//                                            transposing read ds_read_b64_tr_b16
// so the softmax statistics always live on the lane that owns the column c and no tile ever
// crosses lanes through LDS:
//   forward   S^T = K Q^T (F1)            O^T  += V^T P^T  (F2)        c = query, lane-local m, l
//   dQ        S^T = K Q^T, dP^T = V dO^T  dQ^T += K^T dS^T (F2)        c = query
//   dK,dV     S = Q K^T,  dP = dO V^T     dV^T += dO^T P, dK^T += Q^T dS (F2)   c = key
// Backward is two kernels (7 products instead of the fused 5) in exchange for no atomics, no
// dS transpose and bitwise-reproducible gradients.
//
// LDS tiles use the 8-row x 32-column sub-tiled, XOR-swizzled image that is conflict-free
// for both the 16-B row reads and the transposing reads (cdna guide T10 image (a)).
// K/V (or Q/dO) tiles go HBM -> LDS by LDS-DMA (buffer_load ... lds issued from inline asm, the
// image swizzle applied to the per-lane source address), one tile ahead, double-buffered, one
// barrier per tile; the forward pass uses a lazy-rescale online softmax per 32-key sub-block.
#include "common.h"
#include <type_traits>
#include "prof.h"
#include "config.h"
#include "../../include/vds.h"
#include <cstdlib>

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

struct AttnP {
  int B, H, Lq, Lk, hd;
  const bf16_t* q; long q_sb, q_sh, q_sl;
  const bf16_t* k; long k_sb, k_sh, k_sl;
  const bf16_t* v; long v_sb, v_sh, v_sl;
  bf16_t* o; long o_sb, o_sh, o_sl;
  float* lse;
  const bf16_t* d_o; long do_sb, do_sh, do_sl;
  bf16_t* dq; long dq_sb, dq_sh, dq_sl;
  bf16_t* dk; long dk_sb, dk_sh, dk_sl;
  bf16_t* dv; long dv_sb, dv_sh, dv_sl;
  float* delta;
  float scale;
  int n_rt;  // row tiles per (b,h) of the stationary operand
  int tail_last;  // decode_block: the partly filled last tile of every head is scheduled after all full tiles
  int kv_pad_ones;
  // dK/dV kernel, short key sequences (cross-attention: 512 context keys = 4 key tiles per head): the query range is
  // split over q_split workgroups per key tile, each writing an fp32 partial [q_split][B*H][Lk][2][hd] that
  // dkv_reduce_kernel sums into the bf16 outputs (run_bwd picks q_split; 1 = the kernel stores bf16 itself)
  int q_split;
  float* dkv_part;
  // 16-byte row stores in the 16x16x32 kernels' epilogues (store_block_bf16_t): rows 16-byte aligned
  int wide_o, wide_dq, wide_dkv;
  // per-sample key counts (vds_attn_*_kvlen): B int32 on the device, read by the KVLEN instances of the kernels only
  const int* kv_lens;
  // frame-causal map (vds_attn_*_causal): by value, read by the CAUSAL instances of the kernels only
  int fc_lead, fc_period;
  // cached key rows behind the lead rows (vds_attn_fwd_causal_past): by value, read by the PAST forward instances only
  int fc_past;
  // frame-major rows (vds_attn_*_causal_fm): rows per frame S = (L - lead) / period (>= 1) next to fc_lead / fc_period, and
  // the heaviest-tiles-first order; by value, read by the FM instances of the kernels only
  int fm_S, fm_rev;
  // chunk-causal granularity (vds_attn_*_causal_fm_chunk): G = c * S rows per chunk of c frames (the last one may be short);
  // G = S (c = 1) is the frame-causal mask.  The mask bounds kend / qstart use G, the row map tok() keeps S
  int fm_G;
  // sliding window (vds_attn_*_causal_fm_window): W chunks, carried in fc_past -- no FM instance reads that field as a past,
  // and the WIN instances are the only readers of the window; the struct keeps its size (its size moves the code objects)
};
static_assert(sizeof(AttnP) == 376, "AttnP: the kernel argument block keeps its size");

// Keys of sample b.  KVLEN: kv_lens[b] clamped to [0, Lk] -- b is the same for the whole workgroup, so this is one
// scalar load; every bound, tile count and mask of the kernel then uses it in place of the launch-wide Lk.
template <bool KVLEN>
__device__ __forceinline__ int kv_len_of(const AttnP& p, int b) {
  if constexpr (KVLEN) return min(max(p.kv_lens[b], 0), p.Lk);
  else return p.Lk;
}

// Frame-causal mask (CAUSAL instances, vds_attn_*_causal).  Row l of a sample belongs to group 0 (l < lead: the register
// tokens) or 1 + (l - lead) % period (token-frame (l - lead) % period: the token order is (h w t), t fastest), and query q
// attends key k iff group(k) <= group(q).  The rows of a frame are interleaved with that period, so every MFMA block holds
// every frame: the mask is applied per element and no tile is skipped.
// x(l) = (l - lead) % period for l >= lead and a value in [-period, -1] for the lead rows, without an integer division:
// the quotient is trunc((l - lead + 0.5) / period) in fp32 -- the half keeps the exact value 0.5 / period away from every
// integer, further than the two fp32 roundings (2^-23 relative) move it while |l - lead| < 2^21 (the entry points refuse
// longer sequences).  Four full-rate VALU instructions per row; a row's x serves every block that shares the row.
struct FcMap {
  int lead, negp;
  float inv, hinv;
  __device__ __forceinline__ explicit FcMap(const AttnP& p) : lead(p.fc_lead), negp(-p.fc_period) {
    inv = 1.0f / (float)p.fc_period;
    hinv = 0.5f * inv;
  }
  __device__ __forceinline__ int x(int l) const {
    const int kk = l - lead;
    return kk + __mul24((int)__builtin_fmaf((float)kk, inv, hinv), negp);
  }
  // a query attends the keys with x(key) <= fq(query): the lead keys always, no token key from a lead query
  __device__ __forceinline__ int fq(int q) const { return max(x(q), -1); }
  // the same test seen from a key (the dK/dV kernels): its gradient comes from the queries with x(query) >= fk(key)
  __device__ __forceinline__ int fk(int k) const { return k < lead ? -0x7fffffff : x(k); }
};
// 32x32 accumulator with the key on the registers (rows row0 + acc_row(r, 0); row0 includes the lane half's 4 h):
// `fill` where the lane's query (f = fq) may not attend the key
__device__ __forceinline__ void fc_fill(const FcMap& fm, int row0, int f, f32x16& s, float fill) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (fm.x(row0 + (r & 3) + 8 * (r >> 2)) > f) s[r] = fill;
}
__device__ __forceinline__ void fc_fill2(const FcMap& fm, int row0, int f0, int f1, f32x16& s0, f32x16& s1, float fill) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int xk = fm.x(row0 + (r & 3) + 8 * (r >> 2));
    if (xk > f0) s0[r] = fill;
    if (xk > f1) s1[r] = fill;
  }
}
// PAST instances (vds_attn_fwd_causal_past): the Lk = Lq + past key rows are [lead rows | past rows | own token rows] and
// key j is compared as row max(j - past, min(j, lead)) of the query map -- itself for a lead key, `lead` (x = 0, which
// every token query attends and no lead query does) for a past key, the key's own query row behind the past.
__device__ __forceinline__ int fc_past_row(const FcMap& fm, int past, int j) { return max(j - past, min(j, fm.lead)); }
__device__ __forceinline__ void fc_fill_past(const FcMap& fm, int past, int row0, int f, f32x16& s, float fill) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (fm.x(fc_past_row(fm, past, row0 + (r & 3) + 8 * (r >> 2))) > f) s[r] = fill;
}
__device__ __forceinline__ void fc_fill2_past(const FcMap& fm, int past, int row0, int f0, int f1, f32x16& s0, f32x16& s1,
                                              float fill) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int xk = fm.x(fc_past_row(fm, past, row0 + (r & 3) + 8 * (r >> 2)));
    if (xk > f0) s0[r] = fill;
    if (xk > f1) s1[r] = fill;
  }
}
// the 32 keys from k0 are all past rows and the wave holds no lead query (q0: its first query row): every pair is attended,
// the mask code is branched around (wave-uniform: k0, q0 and the map are scalars)
__device__ __forceinline__ bool fc_past_open(const FcMap& fm, int past, int k0, int q0) {
  return k0 >= fm.lead && k0 + 32 <= fm.lead + past && q0 >= fm.lead;
}
// 32x32 accumulators with the QUERY on the registers and the lane's key f = fk: P and dS of the pairs that are not attended
__device__ __forceinline__ void fc_zero_q(const FcMap& fm, int row0, int f, f32x16& pm, f32x16& ds) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (fm.x(row0 + (r & 3) + 8 * (r >> 2)) < f) { pm[r] = 0.f; ds[r] = 0.f; }
}

// Frame-major rows (FM instances, vds_attn_*_causal_fm).  q, k, v, dq, dk, dv, lse and delta rows are stored with a
// frame's rows contiguous: row r belongs to group 0 (r < lead) or 1 + (r - lead) / S, and query r attends key j iff
// group(j) <= group(r) -- the CAUSAL mask with the rows permuted.  The attended keys of a query are then a PREFIX of the
// rows, [0, kend(r)), and the queries that attend a key a SUFFIX, [qstart(j), L): the element-wise compare is one integer
// compare against a per-lane bound (one quotient per row, at the top of the kernel), a workgroup's loop runs over the
// tiles below the largest bound of its rows only, and a sub-block below the smallest bound of a wave is attended without
// any mask code.  o and d_o stay token-major: row r of the computation is row tok(r) of those tensors.
// The quotient is FcMap's: trunc((r - lead + 0.5) / S) in fp32, exact while |r - lead| < 2^21.
// Chunks (vds_attn_*_causal_fm_chunk): the groups are runs of G = c * S rows, 1 + (r - lead) / G -- c whole frames, still a
// contiguous run, so the prefix and the suffix stay; only the two bounds take the quotient by G (the same fp32 rule) and
// kend is clipped to L, which a short last chunk (period % c != 0) would pass.  tok() keeps S and the period.
struct FmMap {
  int lead, S, period, G, L;
  float inv, hinv, ginv, ghinv;
  __device__ __forceinline__ explicit FmMap(const AttnP& p)
      : lead(p.fc_lead), S(p.fm_S), period(p.fc_period), G(p.fm_G), L(p.Lq) {
    inv = 1.0f / (float)p.fm_S;
    hinv = 0.5f * inv;
    ginv = 1.0f / (float)p.fm_G;
    ghinv = 0.5f * ginv;
  }
  __device__ __forceinline__ int frame(int r) const { return (int)__builtin_fmaf((float)(r - lead), inv, hinv); }  // r >= lead
  __device__ __forceinline__ int chunk(int r) const { return (int)__builtin_fmaf((float)(r - lead), ginv, ghinv); }  // r >= lead
  // the first key row that query row r does not attend
  __device__ __forceinline__ int kend(int r) const { return r < lead ? lead : min(L, lead + __mul24(chunk(r) + 1, G)); }
  // the first query row that attends key row j
  __device__ __forceinline__ int qstart(int j) const { return j < lead ? 0 : lead + __mul24(chunk(j), G); }
  // window of W chunks (WIN instances): the first token key row that query row r attends (lead for a lead query: none) ...
  __device__ __forceinline__ int kbeg(int r, int W) const {
    return r < lead ? lead : lead + __mul24(max(chunk(r) - W + 1, 0), G);
  }
  // ... and the first query row past the ones that attend key row j (every query attends a lead key)
  __device__ __forceinline__ int qend(int j, int W) const { return j < lead ? L : min(L, lead + __mul24(chunk(j) + W, G)); }
  // the token row of frame-major row r (o / d_o)
  __device__ __forceinline__ int tok(int r) const {
    if (r < lead) return r;
    const int f = frame(r);
    return lead + __mul24(r - lead - __mul24(f, S), period) + f;
  }
};
// Teacher forcing (TF instances of the FM kernels, vds_teacher_attn_*).  The period is 2n token-frames: frames 0 .. n-1 are
// clean, frames n .. 2n-1 their noisy copies, base = lead + n * S is the first noisy row, and chunks of G rows restart at
// base.  Query r attends [0, pend(r)) plus [kbeg(r), kend(r)) -- the WIN form with a per-row prefix end in place of lead:
//   lead query    pend = lead,                              empty run
//   clean query   pend = min(base, lead + (chunk + 1) G),   empty run         (the chunk-causal mask of the first base rows)
//   noisy query   pend = lead + chunk G,                    [base + chunk G, min(L, base + (chunk + 1) G))
// an empty run is kbeg = kend = pend, so that "key >= kend or pend <= key < kbeg" is the one compare of every row.
// Seen from a key, the readers are [qstart(j), qend(j)) plus [q2(j), L) -- a clean key's readers have a hole:
//   lead key      [0, L),                                   q2 = L
//   clean key     [lead + chunk G, base),                   q2 = min(L, base + (chunk + 1) G)
//   noisy key     [base + chunk G, min(L, base + (chunk + 1) G)),   q2 = L
// qstart and q2 (from lead on) grow with the row, and so do pend, kbeg and kend inside a half.  The quotient is FcMap's
// fp32 rule on the row's offset inside its half (< 2^21).
struct TfMap {
  int lead, base, G, L;
  float ginv, ghinv;
  __device__ __forceinline__ explicit TfMap(const AttnP& p)
      : lead(p.fc_lead), base(p.fc_lead + __mul24(p.fc_period >> 1, p.fm_S)), G(p.fm_G), L(p.Lq) {
    ginv = 1.0f / (float)p.fm_G;
    ghinv = 0.5f * ginv;
  }
  // first row of the chunk of row r inside its half, as an offset from the half's first row (r >= lead)
  __device__ __forceinline__ int cg(int r) const {
    return __mul24((int)__builtin_fmaf((float)(r - (r >= base ? base : lead)), ginv, ghinv), G);
  }
  __device__ __forceinline__ int pend(int r) const {
    return r < lead ? lead : (r < base ? min(base, lead + cg(r) + G) : lead + cg(r));
  }
  __device__ __forceinline__ int kbeg(int r) const { return r < base ? pend(r) : base + cg(r); }
  __device__ __forceinline__ int kend(int r) const { return r < base ? pend(r) : min(L, base + cg(r) + G); }
  __device__ __forceinline__ int qstart(int j) const { return j < lead ? 0 : (j < base ? lead : base) + cg(j); }
  __device__ __forceinline__ int qend(int j) const { return j < lead ? L : (j < base ? base : min(L, base + cg(j) + G)); }
  __device__ __forceinline__ int q2(int j) const { return (j >= lead && j < base) ? min(L, base + cg(j) + G) : L; }
};
// Frame band (BAND instances of the FM kernels, vds_band_attn_*; b = p.fc_past chunks on each side).  Not causal: a token
// row x of chunk n attends the lead rows and the token rows of chunks n - b .. n + b, [lo(x), hi(x)) -- the lead rows plus
// one contiguous run, the WIN form -- and a lead row attends every row.  The relation is symmetric: the readers of token
// key j are [0, lead) and [lo(j), hi(j)), those of a lead key [0, L).  lo and hi grow with the row from lead on.
//   lead row    prefix end L (everything), empty run (lo = hi = L)
//   token row   prefix end lead,           run [lead + max(0, n - b) G, min(L, lead + (n + b + 1) G))
// so that fm_win_masked's "key >= hi or pend <= key < lo" is the one compare of every row.  The quotient is FcMap's fp32
// rule; b is clamped to the chunk count by apply_mask, so b G stays below 2^22.
struct BandMap {
  int lead, G, bG, L;
  float ginv, ghinv;
  __device__ __forceinline__ explicit BandMap(const AttnP& p)
      : lead(p.fc_lead), G(p.fm_G), bG(__mul24(p.fc_past, p.fm_G)), L(p.Lq) {
    ginv = 1.0f / (float)p.fm_G;
    ghinv = 0.5f * ginv;
  }
  // first row of the chunk of token row r, as an offset from lead (r >= lead)
  __device__ __forceinline__ int cg(int r) const { return __mul24((int)__builtin_fmaf((float)(r - lead), ginv, ghinv), G); }
  __device__ __forceinline__ int pend(int r) const { return r < lead ? L : lead; }
  __device__ __forceinline__ int lo(int r) const { return r < lead ? L : lead + max(0, cg(r) - bG); }
  __device__ __forceinline__ int hi(int r) const { return r < lead ? L : min(L, lead + cg(r) + bG + G); }
};
__device__ __forceinline__ int fm_kend(const AttnP& p, int r) { return FmMap(p).kend(r); }
__device__ __forceinline__ int fm_qstart(const AttnP& p, int j) { return FmMap(p).qstart(j); }
// row of o / d_o that holds row r of the computation: tok(r) in the FM instances, r itself otherwise
template <bool FM>
__device__ __forceinline__ int out_row(const AttnP& p, int r) {
  if constexpr (FM) return FmMap(p).tok(r);
  else return r;
}
// keys of the workgroup whose query rows are [q0, q0 + rows): FM -- the largest kend of its rows (<= L); else Lk
// (TF: kend of the last row is the largest bound of either range -- a noisy row's run ends past base, where no prefix reaches)
// (BAND: L for the workgroup that holds a lead row, else hi of its last row)
template <bool FM, bool TF = false, bool BAND = false>
__device__ __forceinline__ int fm_keys(const AttnP& p, int q0, int rows, int Lk) {
  if constexpr (BAND) return q0 < p.fc_lead ? p.Lq : BandMap(p).hi(min(q0 + rows, p.Lq) - 1);
  else if constexpr (TF) return TfMap(p).kend(min(q0 + rows, p.Lq) - 1);
  else if constexpr (FM) return fm_kend(p, min(q0 + rows, p.Lq) - 1);
  else return Lk;
}
// first 64-row query tile of the workgroup whose first key row is k0: FM -- the tile that holds qstart(k0); else dflt
template <bool FM>
__device__ __forceinline__ int fm_first_qtile(const AttnP& p, int k0, int dflt) {
  if constexpr (FM) return fm_qstart(p, k0) >> 6;
  else return dflt;
}
// 32x32 accumulator with the key on the registers (rows row0 + acc_row(r, 0)): `fill` at the keys from the lane's kend
__device__ __forceinline__ void fm_fill(int row0, int kend, f32x16& s, float fill) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (row0 + (r & 3) + 8 * (r >> 2) >= kend) s[r] = fill;
}
// 32x32 accumulators with the QUERY on the registers: P and dS of the queries before the lane's qstart
__device__ __forceinline__ void fm_zero_q(int row0, int qstart, f32x16& pm, f32x16& ds) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (row0 + (r & 3) + 8 * (r >> 2) < qstart) { pm[r] = 0.f; ds[r] = 0.f; }
}
// Sliding window (WIN instances of the FM kernels, vds_attn_*_causal_fm_window; W = p.fc_past chunks): query r attends
// [0, lead) and [kbeg(r), kend(r)) -- the lead rows plus one contiguous run -- and key j is attended by [qstart(j), qend(j)).
__device__ __forceinline__ int fm_kbeg(const AttnP& p, int r) { return FmMap(p).kbeg(r, p.fc_past); }
__device__ __forceinline__ int fm_qend(const AttnP& p, int j) { return FmMap(p).qend(j, p.fc_past); }
// Key tiles of a forward / dQ workgroup with query rows [q0, q0 + rows), nkt = the tile count of fm_keys: the tiles that
// hold lead keys, [0, nl), then the tiles from the one that holds kbeg of the workgroup's first token query, [jb, nkt) --
// jb >= nl, so no tile comes twice.  The loop counts visits; tile(it) is the tile of visit it, and the prefetch of the
// next visit follows it across the gap.
// TF: the tiles below the workgroup's largest pend, [0, nl), then those from its smallest kbeg to its largest kend,
// [jb, nkt) -- jb >= nl again, also in the workgroup that straddles base (TfMap).
// BAND: a workgroup with a lead row visits every tile, [0, nkt); any other the lead tiles, [0, nl), then those from lo of
// its first row to hi of its last, [jb, nkt).
template <bool WIN, bool TF = false, bool BAND = false>  // (the other instances build an empty one)
struct FmWinTiles {
  int nl = 0, jb = 0, nit = 0;
  __device__ __forceinline__ FmWinTiles(const AttnP& p, int q0, int rows, int nkt) {
    if constexpr (BAND) {
      nl = q0 < p.fc_lead ? nkt : min(nkt, (p.fc_lead + 63) >> 6);
      jb = q0 < p.fc_lead ? nkt : max(nl, BandMap(p).lo(q0) >> 6);
      nit = nl + nkt - jb;
    } else if constexpr (TF) {
      const TfMap tf(p);
      const int q1 = min(q0 + rows, p.Lq);
      // the largest pend: that of the last clean (or lead) row if there is one -- base for the straddling workgroup, which
      // no noisy row's prefix reaches -- else the last row's
      nl = (tf.pend(q0 < tf.base ? min(q1, tf.base) - 1 : q1 - 1) + 63) >> 6;
      jb = q1 > tf.base ? max(nl, tf.kbeg(max(q0, tf.base)) >> 6) : nkt;
      nit = nl + nkt - jb;
    } else if constexpr (WIN) {
      nl = min(nkt, (p.fc_lead + 63) >> 6);
      const int qf = max(q0, p.fc_lead);  // first token query, if the workgroup holds one
      jb = qf < min(q0 + rows, p.Lq) ? max(nl, fm_kbeg(p, qf) >> 6) : nkt;
      nit = nl + nkt - jb;
    }
  }
  __device__ __forceinline__ int tile(int it) const { return it < nl ? it : it - nl + jb; }
};
// the wave-uniform open test of the WIN forward / dQ kernels: the 32 keys from k0 need no mask code if the wave holds no
// lead query (wlead, wkend are 0 otherwise) and they lie wholly below lead or wholly inside [kbeg of the wave's last query,
// kend of its first)
// TF: wlead is the wave's smallest pend (its first query's) and the run that of a wave of noisy queries only; a wave of
// clean queries only has no run, and a wave with a lead query or with queries of both halves has nothing open.
// BAND: a wave of token queries only has the WIN test on [lo of its last query, hi of its first); a wave of lead queries only
// has everything below L open; a wave that holds both has nothing open.
template <bool WIN, bool TF = false, bool BAND = false>
struct FmWinOpen {
  int wlead = 0, wkbeg = 0, wkend = 0;
  __device__ __forceinline__ FmWinOpen(const AttnP& p, int wq0, int wrows) {
    if constexpr (BAND) {
      const BandMap bm(p);
      const int wq1 = min(wq0 + wrows, p.Lq) - 1;  // the wave's last query
      if (wq1 < bm.lead) {
        wlead = p.Lq;
      } else if (wq0 >= bm.lead) {
        wlead = bm.lead;
        wkbeg = __builtin_amdgcn_readfirstlane(bm.lo(wq1));
        wkend = __builtin_amdgcn_readfirstlane(bm.hi(wq0));
      }
    } else if constexpr (TF) {
      const TfMap tf(p);
      const int wq1 = min(wq0 + wrows, p.Lq) - 1;  // the wave's last query
      const bool noisy = wq0 >= tf.base, clean = wq0 >= tf.lead && wq1 < tf.base;
      wlead = (noisy || clean) ? __builtin_amdgcn_readfirstlane(tf.pend(wq0)) : 0;
      wkbeg = noisy ? __builtin_amdgcn_readfirstlane(tf.kbeg(wq1)) : 0;
      wkend = noisy ? __builtin_amdgcn_readfirstlane(tf.kend(wq0)) : 0;
    } else if constexpr (WIN) {
      const bool tokens = wq0 >= p.fc_lead;
      wlead = tokens ? p.fc_lead : 0;
      wkend = tokens ? __builtin_amdgcn_readfirstlane(fm_kend(p, wq0)) : 0;
      wkbeg = __builtin_amdgcn_readfirstlane(fm_kbeg(p, min(wq0 + wrows, p.Lq) - 1));
    }
  }
  __device__ __forceinline__ bool open(int k0) const { return k0 + 32 <= wlead || (k0 >= wkbeg && k0 + 32 <= wkend); }
};
// key row `key` is masked for a query with the bounds kbeg / kend: a token key outside its run (kbeg >= lead always)
__device__ __forceinline__ bool fm_win_masked(int key, int lead, int kbeg, int kend) {
  return key >= kend || (key >= lead && key < kbeg);
}
__device__ __forceinline__ void fm_fill_win(int row0, int lead, int kbeg, int kend, f32x16& s, float fill) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (fm_win_masked(row0 + (r & 3) + 8 * (r >> 2), lead, kbeg, kend)) s[r] = fill;
}
// 32x32 accumulators with the QUERY on the registers: P and dS of the queries outside [qstart, qend) of the lane's key
__device__ __forceinline__ void fm_zero_q_win(int row0, int qstart, int qend, f32x16& pm, f32x16& ds) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = row0 + (r & 3) + 8 * (r >> 2);
    if (q < qstart || q >= qend) { pm[r] = 0.f; ds[r] = 0.f; }
  }
}
// the key of a dK/dV wave (32 keys from k0) with the smallest qend: its first token key -- qend grows with the row from
// there, and a lead key's is L -- or, in a wave of lead keys only, its last key
__device__ __forceinline__ int fm_win_first_token_key(const AttnP& p, int k0) {
  return min(max(k0, p.fc_lead), min(k0 + 31, p.Lk - 1));
}
// Query tiles of a WIN dK/dV workgroup with key rows [key0, key0 + 128): one past the last 64-row tile it sweeps -- every
// tile if it holds a lead key, else the tiles below qend of its last key
__device__ __forceinline__ int fm_win_qtiles(const AttnP& p, int key0, int nqt) {
  return key0 < p.fc_lead ? nqt : (fm_qend(p, min(key0 + 127, p.Lk - 1)) + 63) >> 6;
}
// Query tiles (64 rows) of a TF dK/dV workgroup with key rows [key0, key0 + 128): [a0, a1) from qstart of its first key to
// qend of its last, then [b0, nqt) from q2 of its first key -- b0 >= a1, no tile twice.  A workgroup with a lead key sweeps
// every tile; one of noisy keys only has q2 = L: it sweeps the tiles of its own chunks and nothing else.
// BAND: the lead query tiles, [0, a1), then the tiles from lo of the first key to below hi of the last, [b0, b1) -- a prefix
// plus a run; a workgroup with a lead key sweeps every tile.
template <bool TF, bool BAND = false>
struct TfQTiles {
  int a0 = 0, na = 0, b0 = 0, nit = 0;
  __device__ __forceinline__ TfQTiles(const AttnP& p, int key0, int nqt) {
    if constexpr (BAND) {
      na = nqt;
      b0 = nqt;
      nit = nqt;
      if (key0 >= p.fc_lead) {
        const BandMap bm(p);
        na = min(nqt, (bm.lead + 63) >> 6);
        b0 = max(na, bm.lo(key0) >> 6);
        nit = na + ((bm.hi(min(key0 + 127, p.Lk - 1)) + 63) >> 6) - b0;
      }
    } else if constexpr (TF) {
      const TfMap tf(p);
      int a1 = nqt;
      b0 = nqt;
      if (key0 >= tf.lead) {
        a0 = tf.qstart(key0) >> 6;
        a1 = (tf.qend(min(key0 + 127, p.Lk - 1)) + 63) >> 6;
        const int q2 = tf.q2(key0);
        b0 = q2 >= p.Lq ? nqt : max(a1, q2 >> 6);
      }
      na = a1 - a0;
      nit = na + nqt - b0;
    }
  }
  __device__ __forceinline__ int tile(int it) const { return it < na ? a0 + it : it - na + b0; }
};
// 32x32 accumulators with the QUERY on the registers: P and dS of the queries outside [qstart, qend) and below q2
__device__ __forceinline__ void fm_zero_q_tf(int row0, int qstart, int qend, int q2, f32x16& pm, f32x16& ds) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = row0 + (r & 3) + 8 * (r >> 2);
    if ((q < qstart || q >= qend) && q < q2) { pm[r] = 0.f; ds[r] = 0.f; }
  }
}
// 32x32 accumulators with the QUERY on the registers: P and dS of the queries from pl on that lie outside [qlo, qhi) (BAND:
// pl = lead for a token key, L for a lead key)
__device__ __forceinline__ void fm_zero_q_band(int row0, int pl, int qlo, int qhi, f32x16& pm, f32x16& ds) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = row0 + (r & 3) + 8 * (r >> 2);
    if (q >= pl && (q < qlo || q >= qhi)) { pm[r] = 0.f; ds[r] = 0.f; }
  }
}
// FM instances of the forward and dQ kernels: the row-tile order of a head is reversed, so that its longest workgroups
// (the late query tiles) are issued first; the dK/dV kernel's natural order already starts with its longest (early keys)
__device__ __forceinline__ int fm_tile(const AttnP& p, int rt) { return p.fm_rev ? p.n_rt - 1 - rt : rt; }

// ---- LDS image (a): rows x HDP bf16, 8x32 sub-tiles of 512 B -------------------------------
template <int HDP>
__device__ __forceinline__ int img_off(int row, int ch) {
  return (row >> 3) * ((HDP / 32) * 512) + (ch >> 2) * 512 + (row & 7) * 64 + ((((ch & 3) ^ ((row >> 2) & 3))) << 4);
}
// F1 operand (A or B): 32 rows x 16 k; lane -> row (l&31), k = 16*ks + 8*(l>>5) .. +7
template <int HDP>
__device__ __forceinline__ bf16x8 frag_row(const char* tile, int row0, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(tile + img_off<HDP>(row0 + (lane & 31), ks * 2 + (lane >> 5)));
}
// F2 A operand = T^T: 32 cols (d0..d0+31) x 16 rows (r0..r0+15) of the row-major tile T,
// k order matching an accumulator used as B: element j of lane-half h is row r0 + 8(j>>2) + 4h + (j&3).
template <int HDP>
__device__ __forceinline__ bf16x8 frag_tr(const char* tile, int r0, int d0, int lane) {
  const int g = lane >> 4, h = g >> 1, i = lane & 15, qq = i >> 2, pp = i & 3;
  const int row = r0 + 4 * h + qq;
  const int ch = (d0 >> 3) + 2 * (g & 1) + (pp >> 1);
  const char* p0 = tile + img_off<HDP>(row, ch) + 8 * (pp & 1);
  const char* p1 = tile + img_off<HDP>(row + 8, ch) + 8 * (pp & 1);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p0));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p1));
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}
// accumulator registers 8s..8s+7 -> bf16 operand fragment of k-step s
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& x, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)x[8 * s + j];
  return r;
}
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
#ifndef VDS_DELTA_NT
#define VDS_DELTA_NT 1  // delta preprocess: non-temporal loads of O / dO (6.7 -> 6.3 ms per step; 0 = plain loads)
#endif
#ifdef VDS_ATTN_PRIO
#define PRIO_HI() __builtin_amdgcn_s_setprio(1)
#define PRIO_LO() __builtin_amdgcn_s_setprio(0)
#else
#define PRIO_HI()
#define PRIO_LO()
#endif
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
// row index inside a 32x32 accumulator: reg -> (reg&3) + 8*(reg>>2) + 4*h
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t slice_rsrc(const bf16_t* base, long sl, int L, int hd) {
  return make_rsrc(base, (unsigned)((((long)(L - 1)) * sl + hd) * 2));
}
__device__ __forceinline__ srd_t slice_srd(const bf16_t* base, long sl, int L, int hd) {
  return make_srd(base, (unsigned)((((long)(L - 1)) * sl + hd) * 2));
}

// Make the compiler retire a prologue load HERE (a use it can see): otherwise its s_waitcnt vmcnt(0)
// for the first use sits inside the main loop, where it also drains the LDS-DMA prefetch of the
// next tile (vmcnt counts every outstanding vector-memory operation, in order).
__device__ __forceinline__ void retire(const bf16x8& f) { asm volatile("" ::"v"(f)); }
__device__ __forceinline__ void retire(float f) { asm volatile("" ::"v"(f)); }

// XCD-aware (b,h,row-tile) decode: all row tiles of a head run on one XCD so that the
// streamed operand (K/V or Q/dO of that head) stays in that XCD's L2.
// Workgroup -> (head, row tile).  blockIdx & 7 is the XCD; each XCD walks its heads one after the other, so that the
// workgroups of a head -- which all stream the same K / V (or Q / dO) rows -- run together and share them in that XCD's
// L2.  tail_last: the sequence length leaves a partly filled last tile (8192 + 16 register tokens = 64 tiles of 128 +
// 1), whose workgroup costs about half a full one (only one of its waves has rows).  Those tail workgroups of all the
// XCD's heads are scheduled after the full ones, so that the partly filled LAST ROUND of the launch is made of cheap
// workgroups: nothing at B = 12 (24 rounds), but at B = 2 the forward launch is 2 rounds + 32 tails instead of 3 rounds.
__device__ __forceinline__ bool decode_block(int n_rt, int tail_last, int BH, int& bh, int& rt) {
  const int pid = blockIdx.x, xcd = pid & 7, idx = pid >> 3;
  if (tail_last && n_rt > 1) {
    const int n_full = n_rt - 1, cut = ((BH + 7) >> 3) * n_full;
    if (idx < cut) {
      bh = (idx / n_full) * 8 + xcd;
      rt = idx % n_full;
    } else {
      bh = (idx - cut) * 8 + xcd;
      rt = n_full;
    }
  } else {
    bh = (idx / n_rt) * 8 + xcd;
    rt = idx % n_rt;
  }
  return bh < BH;
}

// store a transposed accumulator set Y^T[d, c] (c on lanes) as rows Y[c, d] of bf16
template <int NDB>
__device__ __forceinline__ void store_rows(bf16_t* rowp, const f32x16 (&acc)[NDB], float mul, int hd, int h) {
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int d = db * 32 + 8 * rg + 4 * h;
      if (d < hd) {
        u32x2 w;
        w[0] = pack_bf2(acc[db][4 * rg] * mul, acc[db][4 * rg + 1] * mul);
        w[1] = pack_bf2(acc[db][4 * rg + 2] * mul, acc[db][4 * rg + 3] * mul);
        *reinterpret_cast<u32x2*>(rowp + d) = w;
      }
    }
}

// the same accumulator set as fp32 rows (partial sums of the query-split dK/dV kernel)
template <int NDB>
__device__ __forceinline__ void store_rows_f32(float* rowp, const f32x16 (&acc)[NDB], int hd, int h) {
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int d = db * 32 + 8 * rg + 4 * h;
      if (d < hd)
        *reinterpret_cast<f32x4*>(rowp + d) = f32x4{acc[db][4 * rg], acc[db][4 * rg + 1], acc[db][4 * rg + 2], acc[db][4 * rg + 3]};
    }
}
// zero rows in the two store forms above and below (KVLEN instances: a sample without keys, key rows past its length)
template <int NDB>
__device__ __forceinline__ void store_zero_rows(bf16_t* rowp, int hd, int h) {
  f32x16 z[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) z[i] = zero16();
  store_rows<NDB>(rowp, z, 0.0f, hd, h);
}
// (all 64 lanes must call: the wide form of store_block_bf16_t exchanges lanes)
__device__ __forceinline__ void store_zero_block(bf16_t* row, int hd, int g, bool valid, bool wide) {
  float z[5][4];
#pragma unroll
  for (int db = 0; db < 5; ++db)
#pragma unroll
    for (int e = 0; e < 4; ++e) z[db][e] = 0.f;
  store_block_bf16_t(z, 0.0f, row, hd, g, valid, wide);
}
// dk / dv (bf16, strided) = sum over the q_split partials; one thread = 4 consecutive head-dim columns of one
// (b, h, key, dk | dv) row; dk is scaled by the softmax scale here (the bf16 path does it in store_rows)
// KVLEN: rows at or past kv_lens[b] are written as zeros and their partials -- which skipped workgroups never wrote --
// are not read.
template <bool KVLEN = false>
__global__ __launch_bounds__(256) void dkv_reduce_kernel(AttnP p) {
  const int hq = p.hd >> 2;
  const long n = (long)p.B * p.H * p.Lk * 2 * hq;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  const int c = (int)(gid % hq);
  const int which = (int)((gid / hq) & 1);
  const long row = gid / (2 * hq);  // (b * H + h) * Lk + key
  const int key = (int)(row % p.Lk);
  const int bh = (int)(row / p.Lk), b = bh / p.H, hh = bh % p.H;
  const long stride = (long)p.B * p.H * p.Lk * 2 * p.hd;
  const float* src = p.dkv_part + (row * 2 + which) * p.hd + 4 * c;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (!KVLEN || key < kv_len_of<KVLEN>(p, b)) {
    a = *reinterpret_cast<const f32x4*>(src);
    for (int sp = 1; sp < p.q_split; ++sp) a += *reinterpret_cast<const f32x4*>(src + sp * stride);
  }
  const float mul = which == 0 ? p.scale : 1.0f;
  bf16_t* dst = which == 0 ? p.dk + b * p.dk_sb + hh * p.dk_sh + (long)key * p.dk_sl
                           : p.dv + b * p.dv_sb + hh * p.dv_sh + (long)key * p.dv_sl;
  const u32x2 w = {pack_bf2(a[0] * mul, a[1] * mul), pack_bf2(a[2] * mul, a[3] * mul)};
  *reinterpret_cast<u32x2*>(dst + 4 * c) = w;
}

// ===================================== forward ==============================================
// ---- lazy-rescale online softmax per 32-key sub-block ---------------------------------------
// The running maximum is only raised (and O, l rescaled) when some row's sub-block maximum exceeds
// it by more than 2^LAZY_THR (wave-uniform, rare after the first tile), so each 32-key sub-block is
// an independent chain  S (MFMA) -> exp2 (VALU) -> P V (MFMA): the S products of sub-block kb+1
// can issue under the VALU work of sub-block kb inside ONE wave, on top of the overlap between
// the waves that share a SIMD.  P <= 2^LAZY_THR keeps bf16's relative precision; sums are fp32.
constexpr float LAZY_THR = 8.0f;
__device__ __forceinline__ float max_with_other_half(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float add_with_other_half(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---- explicit software pipeline of the LDS fragment reads ------------------------------------
// All operand fragments of a 32-key sub-block are read from LDS one phase before the MFMAs that
// consume them (K fragments of both sub-blocks at the top of the tile, the V^T fragments of a
// sub-block while the S products / the other sub-block's softmax run), so no MFMA waits on an
// LDS round trip, and each sub-block's VALU softmax runs under the other sub-block's MFMAs.
template <int HDP, int KSQ>
__device__ __forceinline__ void load_kfrags(bf16x8 (&kf)[KSQ], const char* tile, int row0, int lane) {
#pragma unroll
  for (int ks = 0; ks < KSQ; ++ks) kf[ks] = frag_row<HDP>(tile, row0, ks, lane);
}
template <int HDP, int NDB>
__device__ __forceinline__ void load_vfrags(bf16x8 (&vf)[2][NDB], const char* tile, int row0, int lane) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int db = 0; db < NDB; ++db) vf[s2][db] = frag_tr<HDP>(tile, row0 + 16 * s2, db * 32, lane);
}

// one 32-key sub-block of the lazy online softmax: s (scores, fp32) -> P fragments (bf16)
// OWN (the FM forward): inside the wave-uniform branch a lane raises its maximum only if its OWN row is over the threshold,
// so a row's m, l and O never depend on what the other queries of its wave hold -- rows of later frames share waves with
// rows of earlier ones there, and o / lse of a row must not move by a bit when a later frame's Q changes.
template <int NDB, bool OWN = false>
__device__ __forceinline__ void lazy_softmax(f32x16& s, float c, float& m, float& l, f32x16 (&o)[NDB],
                                             bf16x8 (&pf)[2]) {
  float mx = fmaxf(s[0], s[1]);
#pragma unroll
  for (int r = 2; r < 16; r += 2) mx = fmaxf(mx, fmaxf(s[r], s[r + 1]));
  mx = max_with_other_half(mx) * c;
  if (__builtin_amdgcn_ballot_w64(mx > m + LAZY_THR) != 0) {  // wave-uniform, rare
    asm volatile("; rescale" ::: "memory");  // keeps this a real branch (no if-conversion)
    const float m_new = (!OWN || mx > m + LAZY_THR) ? fmaxf(m, mx) : m;
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    m = m_new;
    l *= alpha;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
  }
  float ls = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float e = __builtin_amdgcn_exp2f(s[r] * c - m);
    s[r] = e;
    ls += e;
  }
  l += ls;
  pf[0] = acc_frag(s, 0);
  pf[1] = acc_frag(s, 1);
}

// ---- LDS-DMA staging of a ROWS x HDP tile in image (a) ---------------------------------------
// buffer_load ... lds writes 64 lanes x 16 B = 1 KiB contiguously, so the image's swizzle is applied
// to the per-lane SOURCE address (guide rule 21): lane i of piece q fills LDS bytes q*1024 + 16 i,
// i.e. chunk `ch` of row `row` with img_off(row, ch) == that offset.  No staging VGPRs, no
// ds_write traffic (a ds_write_b128 costs 13 LDS-path cycles per KiB, the DMA 4).
// image (b): the same 8 x 32 sub-tiles with the swizzle table T = {0, 2, 3, 1}[(row >> 2) & 3] instead of
// (row >> 2) & 3.  It is the layout of the v_mfma_f32_16x16x32_bf16 kernels below: their fragment reads touch
// 16 rows x 4 chunks (ds_read_b128) resp. 8 rows x 32 B per 32-lane group (ds_read_b64_tr_b16), and T makes both
// conflict-free (the identity table of image (a) is conflict-free for 32 rows x 2 chunks / 4 rows x 64 B).
__device__ __forceinline__ int swz_t(int row) {
  const int h = (row >> 2) & 3;
  return ((((h >> 1) ^ h) & 1) << 1) | (h >> 1);
}
template <int HDP>
__device__ __forceinline__ int imgb_off(int row, int ch) {
  return (row >> 3) * ((HDP / 32) * 512) + (ch >> 2) * 512 + (row & 7) * 64 + (((ch & 3) ^ swz_t(row)) << 4);
}

template <int ROWS, int HDP, int IMG = 0>
struct DmaStage {
  static constexpr int PIECES = ROWS * HDP * 2 / 1024;  // 1-KiB pieces per tile
  static constexpr int PER_WAVE = PIECES / 4;
  unsigned voff[PER_WAVE];  // byte offset of this lane's 16-B chunk relative to the tile's first row
  bool valid[PER_WAVE];
  __device__ __forceinline__ void init(long sl, int hd, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int q = wave * PER_WAVE + i;
      const int st = 2 * q + (lane >> 5);
      const int w = lane & 31, r7 = w >> 2, cs = w & 3;
      const int row = (st / (HDP / 32)) * 8 + r7;
      const int ch = (st % (HDP / 32)) * 4 + (cs ^ (IMG == 0 ? ((row >> 2) & 3) : swz_t(row)));
      voff[i] = (unsigned)(((long)row * sl + ch * 8) * 2);
      valid[i] = ch * 8 < hd;
    }
  }
  __device__ __forceinline__ void issue(srd_t rs, char* tile, unsigned row0_bytes, int wave) const {
    const unsigned base = lds_addr_of(tile) + wave * PER_WAVE * 1024;
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const unsigned off = valid[i] ? voff[i] + row0_bytes : 0xfffffff0u;
      lds_dma16(rs, base + i * 1024, off);
    }
  }
};

// FM instances of the dK/dV kernels: the dO tile of the frame-major query rows row0 .. row0 + ROWS - 1 is gathered from
// the token-major tensor, row r from row tok(r) (one quotient per 16-byte piece and tile); rows at or past Lq are sent
// out of range (zeros) -- tok() of such a row may name a real one.
template <int ROWS, int HDP, int IMG = 0>
struct DmaStageFm {
  static constexpr int PIECES = ROWS * HDP * 2 / 1024;
  static constexpr int PER_WAVE = PIECES / 4;
  int row[PER_WAVE];
  unsigned chb[PER_WAVE];  // byte offset of this lane's 16-B chunk inside its row
  bool valid[PER_WAVE];
  __device__ __forceinline__ void init(int hd, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int q = wave * PER_WAVE + i;
      const int st = 2 * q + (lane >> 5);
      const int w = lane & 31, r7 = w >> 2, cs = w & 3;
      row[i] = (st / (HDP / 32)) * 8 + r7;
      const int ch = (st % (HDP / 32)) * 4 + (cs ^ (IMG == 0 ? ((row[i] >> 2) & 3) : swz_t(row[i])));
      chb[i] = (unsigned)(ch * 16);
      valid[i] = ch * 8 < hd;
    }
  }
  __device__ __forceinline__ void issue(srd_t rs, char* tile, int row0, long sl, const AttnP& p, int wave) const {
    const unsigned base = lds_addr_of(tile) + wave * PER_WAVE * 1024;
    const FmMap fm(p);
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int r = row0 + row[i];
      const unsigned off = (valid[i] && r < p.Lq) ? (unsigned)((long)fm.tok(r) * sl * 2) + chb[i] : 0xfffffff0u;
      lds_dma16(rs, base + i * 1024, off);
    }
  }
};

// ---- forward kernel: lazy softmax + LDS-DMA staging (PIPE: explicit fragment prefetch) ---------
// KVLEN (all forward kernels): sample b attends its first kv_lens[b] keys; the K / V bounds, the tile count and the
// ragged-tile mask follow that count, and a sample without keys gets O = 0, lse = 0 before anything is staged.
// CAUSAL (all forward kernels): the frame-causal mask; masked scores become -inf BEFORE the sub-block maximum, so they
// neither raise the running maximum nor get a nonzero P (their V rows are live, ones columns included).
// PAST (with CAUSAL, all forward kernels): the keys are [lead | past | own] (fc_past_row); a 32-key sub-block that lies
// wholly in the past skips the mask in every wave without a lead query.
// FM (vds_attn_fwd_causal_fm; without KVLEN / CAUSAL / PAST): frame-major rows.  The key loop ends at the largest kend of
// the workgroup's queries (the K / V bounds and the tile count follow it, the way KVLEN's count does), a sub-block is
// compared against the lane's kend unless it lies below the kend of the wave's first query, and the o row goes to tok(row).
// WIN (vds_attn_fwd_causal_fm_window; with FM): the window of p.fc_past chunks.  The key loop visits the lead tiles and
// then the tiles from kbeg of the workgroup's first token query (FmWinTiles); a lane keeps key j iff j < lead or
// kbeg <= j < kend, and a sub-block that FmWinOpen finds open runs without mask code.  A row whose first visited
// sub-blocks are all masked (lead = 0) keeps m = -1e30, l = 0 and O = 0 until its window opens.
// TF (vds_teacher_attn_fwd; with FM, without WIN): teacher forcing (TfMap).  The WIN code with the lane's pend in place of
// lead: the key loop visits the tiles below the workgroup's largest pend, then those from its smallest kbeg to its largest
// kend; a lane keeps key j iff j < pend or kbeg <= j < kend.
// BAND (vds_band_attn_fwd; with FM, without WIN / TF): the frame band (BandMap), not causal.  The WIN code again: a lane keeps
// key j iff j < pend or lo <= j < hi, with pend = L for a lead query.  The workgroup that holds a lead row visits every tile.
template <int HDP, int HDQ, int WPS, bool PIPE, bool KVLEN = false, bool CAUSAL = false, bool PAST = false, bool FM = false,
          bool WIN = false, bool TF = false, bool BAND = false>
__global__ __launch_bounds__(256, WPS) void attn_fwd_kernel(AttnP p) {
  constexpr int KSQ = HDQ / 16, NDB = HDP / 32, TILE = 64 * HDP * 2;
  constexpr bool TWO = WIN || TF || BAND;  // two key-tile ranges
  static_assert(!BAND || (FM && !WIN && !TF), "the frame band: on frame-major rows, its own mask");
  static_assert(!FM || !(KVLEN || CAUSAL || PAST), "frame-major: its own mask");
  static_assert(!WIN || FM, "the window: on frame-major rows");
  static_assert(!TF || (FM && !WIN), "teacher forcing: on frame-major rows, its own mask");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bh, qt;
  if (!decode_block(p.n_rt, p.tail_last, p.B * p.H, bh, qt)) return;
  if constexpr (FM) qt = fm_tile(p, qt);
  const int b = bh / p.H, hh = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qrow = qt * 128 + wave * 32 + (lane & 31);
  const int Lk = fm_keys<FM, TF, BAND>(p, qt * 128, 128, kv_len_of<KVLEN>(p, b));
  if constexpr (KVLEN) {
    if (Lk == 0) {  // no context: O = 0, lse = 0
      if (qrow < p.Lq) {
        store_zero_rows<NDB>(p.o + b * p.o_sb + hh * p.o_sh + (long)qrow * p.o_sl, p.hd, h);
        if (h == 0) p.lse[((long)b * p.H + hh) * p.Lq + qrow] = 0.0f;
      }
      return;
    }
  }

  const __amdgpu_buffer_rsrc_t rq = slice_rsrc(p.q + b * p.q_sb + hh * p.q_sh, p.q_sl, p.Lq, p.hd);
  const srd_t rk = slice_srd(p.k + b * p.k_sb + hh * p.k_sh, p.k_sl, Lk, p.hd);
  const srd_t rv = slice_srd(p.v + b * p.v_sb + hh * p.v_sh, p.v_sl, Lk, p.hd);

  DmaStage<64, HDP> dk, dv;
  dk.init(p.k_sl, p.hd, wave, lane);
  dv.init(p.v_sl, p.hd, wave, lane);
  const unsigned k_step = (unsigned)(64 * p.k_sl * 2), v_step = (unsigned)(64 * p.v_sl * 2);
  const int nkt = (Lk + 63) / 64;
  [[maybe_unused]] const FmWinTiles<WIN, TF, BAND> wt(p, qt * 128, 128, nkt);  // WIN, TF: the two tile ranges of the key loop
  const int nit = TWO ? wt.nit : nkt;                                // visits of the key loop
  if constexpr (TWO) {
    dk.issue(rk, smem, (unsigned)wt.tile(0) * k_step, wave);
    dv.issue(rv, smem + TILE, (unsigned)wt.tile(0) * v_step, wave);
  } else {
  dk.issue(rk, smem, 0, wave);
  dv.issue(rv, smem + TILE, 0, wave);
  }

  bf16x8 qf[KSQ];
#pragma unroll
  for (int ks = 0; ks < KSQ; ++ks) {
    const int e = ks * 16 + 8 * h;
    unsigned off = (unsigned)(((long)qrow * p.q_sl + e) * 2);
    if (e >= p.hd) off = 0xfffffff0u;
    qf[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, 0));
  }

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = zero16();
  float m = -1e30f, l = 0.f;
  const float c = p.scale * LOG2E;
  const FcMap fm(p);
  int fcq = 0;
  if constexpr (CAUSAL) fcq = fm.fq(qrow);
  [[maybe_unused]] const int wq0 = qt * 128 + wave * 32;  // PAST: the wave's first query row
  // FM: the lane's kend, and the wave's smallest (its first query's; 0 with a lead query in the wave: nothing is open)
  [[maybe_unused]] int klim = 0, wklim = 0;
  if constexpr (FM) {
    klim = fm_kend(p, qrow);
    wklim = wq0 >= p.fc_lead ? __builtin_amdgcn_readfirstlane(fm_kend(p, wq0)) : 0;
  }
  // WIN: the lane's kbeg next to its kend, and the wave's open test
  [[maybe_unused]] int kbeg = 0;
  [[maybe_unused]] const FmWinOpen<WIN, TF, BAND> wo(p, wq0, 32);
  if constexpr (WIN) kbeg = fm_kbeg(p, qrow);
  [[maybe_unused]] int pend = p.fc_lead;  // TF: the lane's prefix end, with its run [kbeg, klim)
  if constexpr (TF) {
    const TfMap tf(p);
    pend = tf.pend(qrow);
    kbeg = tf.kbeg(qrow);
    klim = tf.kend(qrow);
  }
  if constexpr (BAND) {  // the lane's prefix end (L for a lead query) and its run [lo, hi)
    const BandMap bm(p);
    pend = bm.pend(qrow);
    kbeg = bm.lo(qrow);
    klim = bm.hi(qrow);
  }
#pragma unroll
  for (int ks = 0; ks < KSQ; ++ks) retire(qf[ks]);
  VDS_WAIT_VM(0);
  __syncthreads();  // tile 0 landed (DMA waited above: the compiler does not see it)

  auto kv_tile = [&](int it, auto PAR) {  // unrolled by two: compile-time LDS buffer parity (see the wide kernel)
    constexpr int par = decltype(PAR)::value;
    int j = it, jn = it + 1;  // this visit's key tile and the next one's (WIN, TF: across the gap between the two ranges)
    if constexpr (TWO) { j = wt.tile(it); jn = wt.tile(it + 1); }
    if (it + 1 < nit) {
      char* nk = smem + (par ^ 1) * 2 * TILE;
      dk.issue(rk, nk, (unsigned)jn * k_step, wave);
      dv.issue(rv, nk + TILE, (unsigned)jn * v_step, wave);
    }
    const char* kt = smem + par * 2 * TILE;
    const char* vt = kt + TILE;
    const bool ragged = (j == nkt - 1) && (Lk & 63);
    if constexpr (PIPE) {
      bf16x8 k0[KSQ], k1[KSQ];
      load_kfrags<HDP, KSQ>(k0, kt, 0, lane);
      load_kfrags<HDP, KSQ>(k1, kt, 32, lane);
      f32x16 s0 = zero16(), s1 = zero16();
#pragma unroll
      for (int ks = 0; ks < KSQ; ++ks) s0 = mfma32(k0[ks], qf[ks], s0);
      bf16x8 v0[2][NDB];
      load_vfrags<HDP, NDB>(v0, vt, 0, lane);
#pragma unroll
      for (int ks = 0; ks < KSQ; ++ks) s1 = mfma32(k1[ks], qf[ks], s1);
      if constexpr (TWO) {
        if (!wo.open(j * 64)) fm_fill_win(j * 64 + 4 * h, pend, kbeg, klim, s0, -INFINITY);
        if (!wo.open(j * 64 + 32)) fm_fill_win(j * 64 + 32 + 4 * h, pend, kbeg, klim, s1, -INFINITY);
      } else if constexpr (FM) {  // (kend <= Lk: the compare covers the ragged tile too)
        if (j * 64 + 32 > wklim) fm_fill(j * 64 + 4 * h, klim, s0, -INFINITY);
        if (j * 64 + 64 > wklim) fm_fill(j * 64 + 32 + 4 * h, klim, s1, -INFINITY);
      } else {
      if (ragged) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (j * 64 + acc_row(r, h) >= Lk) s0[r] = -INFINITY;
          if (j * 64 + 32 + acc_row(r, h) >= Lk) s1[r] = -INFINITY;
        }
      }
      if constexpr (PAST) {
        if (!fc_past_open(fm, p.fc_past, j * 64, wq0)) fc_fill_past(fm, p.fc_past, j * 64 + 4 * h, fcq, s0, -INFINITY);
        if (!fc_past_open(fm, p.fc_past, j * 64 + 32, wq0)) fc_fill_past(fm, p.fc_past, j * 64 + 32 + 4 * h, fcq, s1, -INFINITY);
      } else if constexpr (CAUSAL) {
        fc_fill(fm, j * 64 + 4 * h, fcq, s0, -INFINITY);
        fc_fill(fm, j * 64 + 32 + 4 * h, fcq, s1, -INFINITY);
      }
      }
      bf16x8 pf[2];
      lazy_softmax<NDB, FM>(s0, c, m, l, o, pf);
      bf16x8 v1[2][NDB];
      load_vfrags<HDP, NDB>(v1, vt, 32, lane);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] = mfma32(v0[s2][db], pf[s2], o[db]);
      bf16x8 pg[2];
      lazy_softmax<NDB, FM>(s1, c, m, l, o, pg);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] = mfma32(v1[s2][db], pg[s2], o[db]);
    } else {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        f32x16 s = zero16();
#pragma unroll
        for (int ks = 0; ks < KSQ; ++ks) s = mfma32(frag_row<HDP>(kt, kb * 32, ks, lane), qf[ks], s);
        if constexpr (TWO) {
          if (!wo.open(j * 64 + kb * 32)) fm_fill_win(j * 64 + kb * 32 + 4 * h, pend, kbeg, klim, s, -INFINITY);
        } else if constexpr (FM) {
          if (j * 64 + kb * 32 + 32 > wklim) fm_fill(j * 64 + kb * 32 + 4 * h, klim, s, -INFINITY);
        } else {
        if (ragged) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (j * 64 + kb * 32 + acc_row(r, h) >= Lk) s[r] = -INFINITY;
        }
        if constexpr (PAST) {
          if (!fc_past_open(fm, p.fc_past, j * 64 + kb * 32, wq0))
            fc_fill_past(fm, p.fc_past, j * 64 + kb * 32 + 4 * h, fcq, s, -INFINITY);
        } else if constexpr (CAUSAL) fc_fill(fm, j * 64 + kb * 32 + 4 * h, fcq, s, -INFINITY);
        }
        bf16x8 pf[2];
        lazy_softmax<NDB, FM>(s, c, m, l, o, pf);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int db = 0; db < NDB; ++db)
            o[db] = mfma32(frag_tr<HDP>(vt, kb * 32 + 16 * s2, db * 32, lane), pf[s2], o[db]);
      }
    }
    VDS_WAIT_VM(0);
    __syncthreads();  // next tile landed, everyone done reading this one
  };
  for (int it = 0; it < nit; it += 2) {
    kv_tile(it, std::integral_constant<int, 0>{});
    if (it + 1 < nit) kv_tile(it + 1, std::integral_constant<int, 1>{});
  }

  const float lt = add_with_other_half(l);
  if (qrow < p.Lq) {
    store_rows<NDB>(p.o + b * p.o_sb + hh * p.o_sh + (long)out_row<FM>(p, qrow) * p.o_sl, o, 1.0f / lt, p.hd, h);
    if (h == 0) p.lse[((long)b * p.H + hh) * p.Lq + qrow] = (m + __builtin_amdgcn_logf(lt)) * LN2;
  }
}

// ---- forward, wide kernel: 64 queries per wave (two 32-query blocks) --------------------------
// Every K / V^T fragment read from LDS feeds two MFMAs (one per query block).  The kernel is bound by
// VALU issue slots next to the MFMAs (an MFMA gap hides ~24 cycles of VALU issue; the plain online
// softmax needs ~42), so with ONES (k / v rows carry ones columns in their padding, vds_attn_args
// .kv_pad_ones) the softmax sheds its multiply-add and its row-sum adds:
//   * Q is pre-multiplied by scale*log2(e) in registers and carries -m (the running maximum, kept
//     bf16-representable) at column head_dim, where every K row holds 1.0: the QK^T MFMA delivers
//     log2-domain scores MINUS the running maximum, ready for v_exp_f32;
//   * every V row holds 1.0 at columns head_dim and head_dim+4: row head_dim (+4) of the O^T
//     accumulator IS the softmax denominator (rescaled together with O, for free);
//   * the running maximum is only raised when some score exceeds it by 2^LAZY_THR (wave-uniform
//     branch, rare after the first tile); the common path has no cross-lane operation at all.
__device__ __forceinline__ bf16x8 scale_frag(bf16x8 f, float c) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)((float)f[j] * c);
  return r;
}

template <int NDB>
__device__ __forceinline__ void ones_softmax(f32x16& s, float& m, bf16x8& q_ones, f32x16 (&o)[NDB], bf16x8 (&pf)[2],
                                             bool first, int h) {
  float mx = fmaxf(s[0], s[1]);
#pragma unroll
  for (int r = 2; r < 16; r += 2) mx = fmaxf(mx, fmaxf(s[r], s[r + 1]));
  if (first || __builtin_amdgcn_ballot_w64(mx > LAZY_THR) != 0) {  // wave-uniform, rare
    asm volatile("; rescale" ::: "memory");  // keeps this a real branch: hipcc otherwise if-converts it and
                                             // runs the 48 O multiplies on every sub-block with alpha = 1
    const float mxf = max_with_other_half(mx);                      // both lanes of a query agree
    const float m_new = bf2f(f2bf(m + (first ? mxf : fmaxf(mxf, 0.f))));
    const float delta = m_new - m;
    const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);
    m = m_new;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] *= alpha;  // includes the denominator row
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] -= delta;
    if (h == 1) q_ones[0] = (__bf16)(-m);              // column head_dim of Q' (exact: m is a bf16 value)
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(s[r]);
  pf[0] = acc_frag(s, 0);
  pf[1] = acc_frag(s, 1);
}

template <int HDP, int HDQ, bool ONES, bool KVLEN = false, bool CAUSAL = false, bool PAST = false>
__global__ __launch_bounds__(256, 2) void attn_fwd_wide_kernel(AttnP p) {
  constexpr int KSQ = HDQ / 16, NDB = HDP / 32, TILE = 64 * HDP * 2;
  static_assert(!ONES || (HDP == 96 && HDQ == 80), "ones columns: head_dim 72 layout");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bh, qt;
  if (!decode_block(p.n_rt, p.tail_last, p.B * p.H, bh, qt)) return;
  const int b = bh / p.H, hh = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qrow0 = qt * 256 + wave * 64 + (lane & 31);  // query of block 0; block 1 = + 32
  const int hd_kv = ONES ? p.hd + 8 : p.hd;               // columns of K / V rows that are fetched
  const int Lk = kv_len_of<KVLEN>(p, b);
  if constexpr (KVLEN) {
    if (Lk == 0) {  // no context: O = 0, lse = 0
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        const int qrow = qrow0 + 32 * qb;
        if (qrow < p.Lq) {
          store_zero_rows<NDB>(p.o + b * p.o_sb + hh * p.o_sh + (long)qrow * p.o_sl, p.hd, h);
          if (h == 0) p.lse[((long)b * p.H + hh) * p.Lq + qrow] = 0.0f;
        }
      }
      return;
    }
  }

  const __amdgpu_buffer_rsrc_t rq = slice_rsrc(p.q + b * p.q_sb + hh * p.q_sh, p.q_sl, p.Lq, p.hd);
  const srd_t rk = slice_srd(p.k + b * p.k_sb + hh * p.k_sh, p.k_sl, Lk, hd_kv);
  const srd_t rv = slice_srd(p.v + b * p.v_sb + hh * p.v_sh, p.v_sl, Lk, hd_kv);

  DmaStage<64, HDP> dk, dv;
  dk.init(p.k_sl, hd_kv, wave, lane);
  dv.init(p.v_sl, hd_kv, wave, lane);
  const unsigned k_step = (unsigned)(64 * p.k_sl * 2), v_step = (unsigned)(64 * p.v_sl * 2);
  dk.issue(rk, smem, 0, wave);
  dv.issue(rv, smem + TILE, 0, wave);

  const float c = p.scale * LOG2E;
  bf16x8 qf[2][KSQ];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int ks = 0; ks < KSQ; ++ks) {
      const int e = ks * 16 + 8 * h;
      unsigned off = (unsigned)(((long)(qrow0 + 32 * qb) * p.q_sl + e) * 2);
      if (e >= p.hd) off = 0xfffffff0u;
      qf[qb][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, 0));
    }
  if constexpr (ONES) {
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int ks = 0; ks < KSQ; ++ks) qf[qb][ks] = scale_frag(qf[qb][ks], c);  // also retires the loads
  } else {
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int ks = 0; ks < KSQ; ++ks) retire(qf[qb][ks]);
  }

  f32x16 o[2][NDB];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int i = 0; i < NDB; ++i) o[qb][i] = zero16();
  float m[2], l[2] = {0.f, 0.f};
  m[0] = m[1] = ONES ? 0.f : -1e30f;
  const int nkt = (Lk + 63) / 64;
  const FcMap fm(p);
  int fcq[2] = {0, 0};
  if constexpr (CAUSAL) { fcq[0] = fm.fq(qrow0); fcq[1] = fm.fq(qrow0 + 32); }
  [[maybe_unused]] const int wq0 = qt * 256 + wave * 64;  // PAST: the wave's first query row
  VDS_WAIT_VM(0);
  __syncthreads();

  // the KV loop is unrolled by two so that the LDS buffer parity is a compile-time constant: every fragment
  // read becomes base register + immediate offset instead of one address add per read
  auto kv_tile = [&](int j, auto PAR) {
    constexpr int par = decltype(PAR)::value;
    if (j + 1 < nkt) {
      char* nk = smem + (par ^ 1) * 2 * TILE;
      dk.issue(rk, nk, (unsigned)(j + 1) * k_step, wave);
      dv.issue(rv, nk + TILE, (unsigned)(j + 1) * v_step, wave);
    }
    const char* kt = smem + par * 2 * TILE;
    const char* vt = kt + TILE;
    const bool ragged = (j == nkt - 1) && (Lk & 63);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      bf16x8 kfr[KSQ];
      load_kfrags<HDP, KSQ>(kfr, kt, kb * 32, lane);
      f32x16 s0 = zero16(), s1 = zero16();
#pragma unroll
      for (int ks = 0; ks < KSQ; ++ks) {
        s0 = mfma32(kfr[ks], qf[0][ks], s0);
        s1 = mfma32(kfr[ks], qf[1][ks], s1);
      }
      // keys past Lk: with ONES no mask is needed -- their zero-filled V rows (ones columns included)
      // add nothing to the numerators or to the denominator, whatever exp2 makes of their scores
      if constexpr (!ONES) {
        if (ragged) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (j * 64 + kb * 32 + acc_row(r, h) >= Lk) { s0[r] = -INFINITY; s1[r] = -INFINITY; }
        }
      }
      // (the frame mask cannot lean on zero V rows: with ONES too the scores themselves go to -inf, before the maxima --
      // key 0 is attended by every query, so the first sub-block's maximum is finite)
      if constexpr (PAST) {
        if (!fc_past_open(fm, p.fc_past, j * 64 + kb * 32, wq0))
          fc_fill2_past(fm, p.fc_past, j * 64 + kb * 32 + 4 * h, fcq[0], fcq[1], s0, s1, -INFINITY);
      } else if constexpr (CAUSAL) fc_fill2(fm, j * 64 + kb * 32 + 4 * h, fcq[0], fcq[1], s0, s1, -INFINITY);
      bf16x8 vfr[2][NDB];
      load_vfrags<HDP, NDB>(vfr, vt, kb * 32, lane);
      bf16x8 p0[2], p1[2];
      if constexpr (ONES) {
        const bool first = (j == 0) && (kb == 0);
        ones_softmax<NDB>(s0, m[0], qf[0][KSQ - 1], o[0], p0, first, h);
        ones_softmax<NDB>(s1, m[1], qf[1][KSQ - 1], o[1], p1, first, h);
      } else {
        lazy_softmax<NDB>(s0, c, m[0], l[0], o[0], p0);
        lazy_softmax<NDB>(s1, c, m[1], l[1], o[1], p1);
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          o[0][db] = mfma32(vfr[s2][db], p0[s2], o[0][db]);
          o[1][db] = mfma32(vfr[s2][db], p1[s2], o[1][db]);
        }
    }
    VDS_WAIT_VM(0);
    __syncthreads();
  };
  for (int j = 0; j < nkt; j += 2) {
    kv_tile(j, std::integral_constant<int, 0>{});
    if (j + 1 < nkt) kv_tile(j + 1, std::integral_constant<int, 1>{});
  }

#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int qrow = qrow0 + 32 * qb;
    // ONES: the denominator is row head_dim (lanes 0-31) / head_dim+4 (lanes 32-63) of O^T = register 4 of block 2
    const float lt = ONES ? o[qb][NDB - 1][4] : add_with_other_half(l[qb]);
    if (qrow < p.Lq) {
      store_rows<NDB>(p.o + b * p.o_sb + hh * p.o_sh + (long)qrow * p.o_sl, o[qb], 1.0f / lt, p.hd, h);
      if (h == 0) p.lse[((long)b * p.H + hh) * p.Lq + qrow] = (m[qb] + __builtin_amdgcn_logf(lt)) * LN2;
    }
  }
}

// kv_pad_ones: the (otherwise unused) pad columns hd, hd+1 of the q row receive -lse*log2(e) as a bf16
// (hi, lo) pair; the dK/dV kernel stages Q rows with their pad and holds 1.0 in the matching columns of
// its K fragments, so its QK^T MFMA delivers log2 P directly.
__device__ __forceinline__ void split_bf16(float x, __bf16& hi, __bf16& lo) {
  hi = (__bf16)x;
  lo = (__bf16)(x - (float)hi);
}
__device__ __forceinline__ void annotate_q(const AttnP& p, int b, int hh, int q, float lse2) {
  __bf16 hi, lo;
  split_bf16(-lse2, hi, lo);
  bf16x2 v;
  v[0] = hi;
  v[1] = lo;
  bf16_t* dst = const_cast<bf16_t*>(p.q) + b * p.q_sb + hh * p.q_sh + (long)q * p.q_sl + p.hd;
  *reinterpret_cast<bf16x2*>(dst) = v;
}

// ndelta[b,h,q] = -sum_d dO[q,d] * O[q,d] and lse2 = lse * log2(e) (one wave per row; HBM-bound
// preprocess).  Workspace layout: ndelta[0 .. rows) | lse2[rows .. 2 rows).  The NEGATED delta is
// what the backward kernels load straight into the dP accumulators (dP - delta for free).
// FM: the statistics (and lse) are indexed by the frame-major row, whose O / dO rows are those of token row tok(row).
template <bool FM = false>
__global__ void attn_delta_kernel(AttnP p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long rows = (long)p.B * p.H * p.Lq;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int q = row % p.Lq;
  const int bh = row / p.Lq;
  const int b = bh / p.H, hh = bh % p.H;
  const bf16_t* o = p.o + b * p.o_sb + hh * p.o_sh + (long)out_row<FM>(p, q) * p.o_sl;
  const bf16_t* d = p.d_o + b * p.do_sb + hh * p.do_sh + (long)out_row<FM>(p, q) * p.do_sl;
  float acc = 0.f;
  for (int e = lane * 2; e < p.hd; e += 128) {
    const unsigned a = *reinterpret_cast<const unsigned*>(o + e);
    const unsigned g = *reinterpret_cast<const unsigned*>(d + e);
    acc += bflo(a) * bflo(g) + bfhi(a) * bfhi(g);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const float l2 = p.lse[row] * LOG2E;
    p.delta[row] = -acc;
    p.delta[rows + row] = l2;
    if (p.kv_pad_ones == 1) annotate_q(p, b, hh, q, l2);
  }
}

// token-major fast path of the same preprocess: O and dO are [B*Lq, H*hd] row-major (what the model
// passes), one wave per token reads both rows with 16-byte accesses; each 8-element chunk belongs
// to one head (hd % 8 == 0), the per-chunk partial dots are folded per head through LDS.
// FM: a wave still reads one TOKEN row of O and dO; its statistics go to the frame-major row fm(token row).
template <bool FM = false>
__global__ __launch_bounds__(256) void attn_delta_tokmajor_kernel(AttnP p) {
  __shared__ float part[4][192];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long tok = (long)blockIdx.x * 4 + wave;  // over B*Lq
  if (tok >= (long)p.B * p.Lq) return;
  const int b = (int)(tok / p.Lq), q = (int)(tok % p.Lq);
  int sq = q;  // the row of lse / delta / q
  if constexpr (FM) {
    if (q >= p.fc_lead) {
      const int x = q - p.fc_lead, f = x / p.fc_period;
      sq = p.fc_lead + (x - f * p.fc_period) * p.fm_S + f;
    }
  }
  const int nch = p.H * p.hd / 8, cph = p.hd / 8;
  const bf16_t* o = p.o + b * p.o_sb + (long)q * p.o_sl;
  const bf16_t* d = p.d_o + b * p.do_sb + (long)q * p.do_sl;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
#if VDS_DELTA_NT  // non-temporal loads of O (saved by the forward pass) and dO: read once
      const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(o + c * 8));
      const u32x4 g = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(d + c * 8));
#else
      const u32x4 a = *reinterpret_cast<const u32x4*>(o + c * 8);
      const u32x4 g = *reinterpret_cast<const u32x4*>(d + c * 8);
#endif
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += bflo(a[e]) * bflo(g[e]) + bfhi(a[e]) * bfhi(g[e]);
      part[wave][c] = acc;
    }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's own LDS writes
  __builtin_amdgcn_wave_barrier();
  if (lane < p.H) {
    float acc = 0.f;
    for (int i = 0; i < cph; ++i) acc += part[wave][lane * cph + i];
    const long rows = (long)p.B * p.H * p.Lq;
    const long row = ((long)b * p.H + lane) * p.Lq + sq;
    const float l2 = p.lse[row] * LOG2E;
    p.delta[row] = -acc;
    p.delta[rows + row] = l2;
    if (p.kv_pad_ones == 1) annotate_q(p, b, lane, sq, l2);
  }
}

// ===================================== dQ ===================================================
// ONES (k / v rows carry ones columns in their padding, vds_attn_args.kv_pad_ones; head_dim 72): the
// kernel is bound by the VALU work between its MFMAs, so the per-query constants move into the MFMAs:
// Q is pre-multiplied by scale*log2(e) in registers and carries -lse*log2(e) as a bf16 (hi, lo) pair at
// columns hd, hd+1 (K holds 1.0 there), dO carries -delta as a (hi, lo) pair at columns hd, hd+4 (V holds
// 1.0 there): S' = log2 P and dP - delta come straight out of the two MFMA chains, leaving
// exp2, one multiply and the bf16 pack per element.  Keys past Lk need no mask in either mode.
// KVLEN (all dQ kernels): the sweep covers the first kv_lens[b] keys of sample b; without keys dQ = 0.
// CAUSAL (all dQ kernels): dS of the pairs the frame-causal mask excludes is set to zero (P = 0 exactly).
// FM (vds_attn_bwd_causal_fm; the plain layout only): frame-major rows -- the key sweep ends at the largest kend of the
// workgroup's queries, dS is zeroed from the lane's kend unless the sub-block lies below the kend of the wave's first query,
// and the dO row is that of token row tok(row); q, dq and the statistics are indexed by the frame-major row.
// WIN (vds_attn_bwd_causal_fm_window; with FM): the window -- the two tile ranges, the per-lane compare and the open test
// of the forward kernel, with dS = 0 in place of -inf.
// TF (vds_teacher_attn_bwd; with FM, without WIN): teacher forcing -- as the forward kernel's, with dS = 0 in place of -inf.
// BAND (vds_band_attn_bwd; with FM, without WIN / TF): the frame band -- as the forward kernel's, with dS = 0 in place of -inf.
template <int HDP, int HDQ, bool ONES, bool KVLEN = false, bool CAUSAL = false, bool FM = false, bool WIN = false,
          bool TF = false, bool BAND = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(AttnP p) {
  constexpr int KSQ = HDQ / 16, NDB = HDP / 32, TILE = 64 * HDP * 2;
  constexpr bool TWO = WIN || TF || BAND;  // two key-tile ranges
  static_assert(!BAND || (FM && !WIN && !TF), "the frame band: on frame-major rows, its own mask");
  static_assert(!WIN || FM, "the window: on frame-major rows");
  static_assert(!TF || (FM && !WIN), "teacher forcing: on frame-major rows, its own mask");
  static_assert(!ONES || (HDP == 96 && HDQ == 80), "ones columns: head_dim 72 layout");
  static_assert(!FM || !(ONES || KVLEN || CAUSAL), "frame-major: the plain layout, its own mask");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bh, qt;
  if (!decode_block(p.n_rt, p.tail_last, p.B * p.H, bh, qt)) return;
  if constexpr (FM) qt = fm_tile(p, qt);
  const int b = bh / p.H, hh = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qrow = qt * 128 + wave * 32 + (lane & 31);
  const int hd_kv = ONES ? p.hd + 8 : p.hd;
  const int Lk = fm_keys<FM, TF, BAND>(p, qt * 128, 128, kv_len_of<KVLEN>(p, b));
  if constexpr (KVLEN) {
    if (Lk == 0) {  // no context: dQ = 0
      if (qrow < p.Lq) store_zero_rows<NDB>(p.dq + b * p.dq_sb + hh * p.dq_sh + (long)qrow * p.dq_sl, p.hd, h);
      return;
    }
  }

  const __amdgpu_buffer_rsrc_t rq = slice_rsrc(p.q + b * p.q_sb + hh * p.q_sh, p.q_sl, p.Lq, p.hd);
  const __amdgpu_buffer_rsrc_t rdo = slice_rsrc(p.d_o + b * p.do_sb + hh * p.do_sh, p.do_sl, p.Lq, p.hd);
  const srd_t rk = slice_srd(p.k + b * p.k_sb + hh * p.k_sh, p.k_sl, Lk, hd_kv);
  const srd_t rv = slice_srd(p.v + b * p.v_sb + hh * p.v_sh, p.v_sl, Lk, hd_kv);

  DmaStage<64, HDP> dk, dv;
  dk.init(p.k_sl, hd_kv, wave, lane);
  dv.init(p.v_sl, hd_kv, wave, lane);
  const unsigned k_step = (unsigned)(64 * p.k_sl * 2), v_step = (unsigned)(64 * p.v_sl * 2);
  const int nkt = (Lk + 63) / 64;
  [[maybe_unused]] const FmWinTiles<WIN, TF, BAND> wt(p, qt * 128, 128, nkt);  // WIN, TF: as in the forward kernel
  const int nit = TWO ? wt.nit : nkt;
  if constexpr (TWO) {
    dk.issue(rk, smem, (unsigned)wt.tile(0) * k_step, wave);
    dv.issue(rv, smem + TILE, (unsigned)wt.tile(0) * v_step, wave);
  } else {
  dk.issue(rk, smem, 0, wave);
  dv.issue(rv, smem + TILE, 0, wave);
  }

  bf16x8 qf[KSQ], dof[KSQ];
#pragma unroll
  for (int ks = 0; ks < KSQ; ++ks) {
    const int e = ks * 16 + 8 * h;
    unsigned off = (unsigned)(((long)qrow * p.q_sl + e) * 2);
    unsigned off2 = (unsigned)(((long)out_row<FM>(p, qrow) * p.do_sl + e) * 2);
    if (e >= p.hd) { off = 0xfffffff0u; off2 = 0xfffffff0u; }
    qf[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, 0));
    dof[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rdo, off2, 0, 0));
  }
  const long nrows = (long)p.B * p.H * p.Lq;
  const long srow = ((long)b * p.H + hh) * p.Lq + min(qrow, p.Lq - 1);
  const float ndl = p.delta[srow];  // -delta of this lane's query
  const float lse2 = p.delta[nrows + srow];
  const float c = p.scale * LOG2E;
  if constexpr (ONES) {
#pragma unroll
    for (int ks = 0; ks < KSQ; ++ks) { qf[ks] = scale_frag(qf[ks], c); retire(dof[ks]); }
    if (h == 1) {  // fragment KSQ-1 of lane half 1 holds columns hd .. hd+7
      __bf16 hi, lo;
      split_bf16(-lse2, hi, lo);
      qf[KSQ - 1][0] = hi;
      qf[KSQ - 1][1] = lo;
      split_bf16(ndl, hi, lo);
      dof[KSQ - 1][0] = hi;
      dof[KSQ - 1][4] = lo;
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < KSQ; ++ks) { retire(qf[ks]); retire(dof[ks]); }
    retire(ndl);
    retire(lse2);
  }

  f32x16 dq[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) dq[i] = zero16();
  const FcMap fm(p);
  int fcq = 0;
  if constexpr (CAUSAL) fcq = fm.fq(qrow);
  [[maybe_unused]] int klim = 0, wklim = 0;  // FM: as in the forward kernel
  if constexpr (FM) {
    const int wq0 = qt * 128 + wave * 32;
    klim = fm_kend(p, qrow);
    wklim = wq0 >= p.fc_lead ? __builtin_amdgcn_readfirstlane(fm_kend(p, wq0)) : 0;
  }
  [[maybe_unused]] int kbeg = 0;  // WIN: as in the forward kernel
  [[maybe_unused]] const FmWinOpen<WIN, TF, BAND> wo(p, qt * 128 + wave * 32, 32);
  if constexpr (WIN) kbeg = fm_kbeg(p, qrow);
  [[maybe_unused]] int pend = p.fc_lead;  // TF: as in the forward kernel
  if constexpr (TF) {
    const TfMap tf(p);
    pend = tf.pend(qrow);
    kbeg = tf.kbeg(qrow);
    klim = tf.kend(qrow);
  }
  if constexpr (BAND) {  // the lane's prefix end (L for a lead query) and its run [lo, hi)
    const BandMap bm(p);
    pend = bm.pend(qrow);
    kbeg = bm.lo(qrow);
    klim = bm.hi(qrow);
  }
  VDS_WAIT_VM(0);
  __syncthreads();  // tile 0 landed

  auto kv_tile = [&](int it, auto PAR) {  // unrolled by two: compile-time LDS buffer parity (see the forward kernel)
    constexpr int par = decltype(PAR)::value;
    int j = it, jn = it + 1;  // this visit's key tile and the next one's (WIN, TF: across the gap)
    if constexpr (TWO) { j = wt.tile(it); jn = wt.tile(it + 1); }
    if (it + 1 < nit) {
      char* nk = smem + (par ^ 1) * 2 * TILE;
      dk.issue(rk, nk, (unsigned)jn * k_step, wave);
      dv.issue(rv, nk + TILE, (unsigned)jn * v_step, wave);
    }
    const char* kt = smem + par * 2 * TILE;
    const char* vt = kt + TILE;
    // keys past Lk need no mask: their K rows are zero-filled, so whatever dS they get multiplies a
    // zero row of K in dQ^T += K^T dS^T
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x16 s = zero16(), dp;
      if constexpr (ONES) {
        dp = zero16();
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = ndl;  // accumulator starts at -delta: dP - delta for free
      }
#pragma unroll
      for (int ks = 0; ks < KSQ; ++ks) {
        s = mfma32(frag_row<HDP>(kt, kb * 32, ks, lane), qf[ks], s);
        dp = mfma32(frag_row<HDP>(vt, kb * 32, ks, lane), dof[ks], dp);
      }
      if constexpr (ONES) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(s[r]) * dp[r];  // dS^T (unscaled)
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(s[r] * c - lse2) * dp[r];
      }
      if constexpr (CAUSAL) fc_fill(fm, j * 64 + kb * 32 + 4 * h, fcq, s, 0.f);
      if constexpr (TWO) {
        if (!wo.open(j * 64 + kb * 32)) fm_fill_win(j * 64 + kb * 32 + 4 * h, pend, kbeg, klim, s, 0.f);
      } else if constexpr (FM) {
        if (j * 64 + kb * 32 + 32 > wklim) fm_fill(j * 64 + kb * 32 + 4 * h, klim, s, 0.f);
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 df = acc_frag(s, s2);
#pragma unroll
        for (int db = 0; db < NDB; ++db)
          dq[db] = mfma32(frag_tr<HDP>(kt, kb * 32 + 16 * s2, db * 32, lane), df, dq[db]);
      }
    }
    VDS_WAIT_VM(0);
    __syncthreads();
  };
  for (int it = 0; it < nit; it += 2) {
    kv_tile(it, std::integral_constant<int, 0>{});
    if (it + 1 < nit) kv_tile(it + 1, std::integral_constant<int, 1>{});
  }
  if (qrow < p.Lq)
    store_rows<NDB>(p.dq + b * p.dq_sb + hh * p.dq_sh + (long)qrow * p.dq_sl, dq, p.scale, p.hd, h);
}

// ===================================== dK, dV ===============================================
// Workgroup = 128 keys (4 waves x 32).  Each wave keeps the K and V rows of its 32 keys as MFMA
// B-operand fragments in registers for the whole sweep over 64-row Q/dO tiles; LDS holds only the
// double-buffered Q/dO tiles and their row statistics (lse2, delta), all filled by LDS-DMA.
// Rows past Lq arrive as zeros (SRD bounds): Q = dO = 0 makes their contribution to dV and dK
// vanish whatever P evaluates to.  S and dP have the key on the lane.
// ONES (kv_pad_ones, head_dim 72): Q rows are staged WITH their pad, which the delta preprocess filled
// with -lse*log2(e) (hi, lo); the K fragments are pre-multiplied by scale*log2(e) and hold 1.0 in those
// two columns, so S comes out of the MFMA as log2 P: no multiply-add and no lse reads per element.
// KVLEN: rows at or past kv_lens[b] of dK / dV are zeros.  A workgroup whose 128 keys all lie there stores them and
// leaves (query split: it leaves at once -- dkv_reduce_kernel<true> writes the zeros without reading its partial); the
// workgroup that holds the boundary runs as usual and clears the accumulators of the rows past it before the store.
// CAUSAL (both dK/dV kernels): P and dS of the pairs the frame-causal mask excludes are set to zero, so a key row sums
// over the queries that attend it and nothing is cleared afterwards.
// FM (vds_attn_bwd_causal_fm; the plain layout, no query split): frame-major rows -- the query sweep starts at the tile
// that holds qstart of the workgroup's first key, P and dS are zeroed before the lane's qstart unless the sub-block starts
// at or past the qstart of the wave's last key, and the dO tile is gathered from the token rows tok(row) (DmaStageFm).
// WIN (vds_attn_bwd_causal_fm_window; with FM): the window -- key j is attended by [qstart(j), qend(j)).  A workgroup that
// holds a lead key sweeps every query tile (its token keys are compared per lane); any other sweeps the tiles from qstart of
// its first key to the one below qend of its last.  A sub-block is open from the wave's largest qstart to its smallest qend.
// TF (vds_teacher_attn_bwd; with FM, without WIN): teacher forcing -- key j is attended by [qstart(j), qend(j)) and by
// [q2(j), L) (TfMap).  The sweep visits the query tiles of TfQTiles, counted as visits like the key loop of the forward
// kernel; a sub-block is open between the wave's largest qstart and its smallest qend, or from its largest q2.
// BAND (vds_band_attn_bwd; with FM, without WIN / TF): the frame band -- token key j is attended by [0, lead) and by
// [lo(j), hi(j)), a lead key by every query (BandMap).  The sweep visits the query tiles of TfQTiles<.., BAND>; a sub-block
// is open in a wave of lead keys, or, in a wave of token keys, below lead or inside [lo of its last key, hi of its first).
template <int HDP, int HDQ, bool ONES, bool KVLEN = false, bool CAUSAL = false, bool FM = false, bool WIN = false,
          bool TF = false, bool BAND = false>
// (head dim 64: three waves per SIMD cap the kernel at 168 VGPRs, which the TF instance's third bound and second tile range
// do not fit without scratch -- it runs at two, and so does the BAND instance, which carries the same three bounds)
__global__ __launch_bounds__(256, (HDP > 96 ? 1 : (HDP == 64 && !TF && !BAND ? 3 : 2))) void attn_bwd_dkv_kernel(AttnP p) {
  constexpr int KSQ = HDQ / 16, NDB = HDP / 32, Q_TILE = 64 * HDP * 2;
  constexpr bool TWO = TF || BAND;  // two query-tile ranges, counted as visits
  static_assert(!BAND || (FM && !WIN && !TF), "the frame band: on frame-major rows, its own mask");
  static_assert(!WIN || FM, "the window: on frame-major rows");
  static_assert(!TF || (FM && !WIN), "teacher forcing: on frame-major rows, its own mask");
  static_assert(!FM || !(ONES || KVLEN || CAUSAL), "frame-major: the plain layout, its own mask");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // LDS: [buf0: Q | dO][buf1: Q | dO][stats: 2 bufs x (lse2[64], delta[64])]
  char* qbuf = smem;
  char* stats = smem + 4 * Q_TILE;
  int bh, kt_idx, sp = 0;
  if (p.q_split > 1) {  // (head, key tile, query range): the workgroups of a head stay on one XCD like the unsplit order
    const int per = p.n_rt * p.q_split, pid = blockIdx.x, idx = pid >> 3;
    bh = (idx / per) * 8 + (pid & 7);
    if (bh >= p.B * p.H) return;
    kt_idx = (idx % per) % p.n_rt;
    sp = (idx % per) / p.n_rt;
  } else if (!decode_block(p.n_rt, p.tail_last, p.B * p.H, bh, kt_idx)) {
    return;
  }
  const int b = bh / p.H, hh = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int key0 = kt_idx * 128;
  const int krow = key0 + wave * 32 + (lane & 31);
  const int Lk = kv_len_of<KVLEN>(p, b);
  if constexpr (KVLEN) {
    if (key0 >= Lk) {  // no key of this tile is attended
      if (p.q_split == 1 && krow < p.Lk) {
        store_zero_rows<NDB>(p.dk + b * p.dk_sb + hh * p.dk_sh + (long)krow * p.dk_sl, p.hd, h);
        store_zero_rows<NDB>(p.dv + b * p.dv_sb + hh * p.dv_sh + (long)krow * p.dv_sl, p.hd, h);
      }
      return;
    }
  }

  const int hd_q = ONES ? p.hd + 8 : p.hd;  // Q row columns that are staged
  const srd_t rq = slice_srd(p.q + b * p.q_sb + hh * p.q_sh, p.q_sl, p.Lq, hd_q);
  const srd_t rdo = slice_srd(p.d_o + b * p.do_sb + hh * p.do_sh, p.do_sl, p.Lq, p.hd);
  const __amdgpu_buffer_rsrc_t rk = slice_rsrc(p.k + b * p.k_sb + hh * p.k_sh, p.k_sl, Lk, p.hd);
  const __amdgpu_buffer_rsrc_t rv = slice_rsrc(p.v + b * p.v_sb + hh * p.v_sh, p.v_sl, Lk, p.hd);
  const long nrows = (long)p.B * p.H * p.Lq;
  const long srow0 = ((long)b * p.H + hh) * p.Lq;
  // statistics of this head: delta rows then lse2 rows, each bounded to the head's Lq entries
  const srd_t rdl = make_srd(p.delta + srow0, (unsigned)(p.Lq * 4));
  const srd_t rl2 = make_srd(p.delta + nrows + srow0, (unsigned)(p.Lq * 4));
  const float c = p.scale * LOG2E;

  DmaStage<64, HDP> dq_;
  std::conditional_t<FM, DmaStageFm<64, HDP>, DmaStage<64, HDP>> dd_;
  dq_.init(p.q_sl, hd_q, wave, lane);
  if constexpr (FM) dd_.init(p.hd, wave, lane);
  else dd_.init(p.do_sl, p.hd, wave, lane);
  const unsigned q_step = (unsigned)(64 * p.q_sl * 2), do_step = (unsigned)(64 * p.do_sl * 2);
  auto issue_tile = [&](int j, int par) {
    char* nb = qbuf + par * 2 * Q_TILE;
    dq_.issue(rq, nb, (unsigned)j * q_step, wave);
    if constexpr (FM) dd_.issue(rdo, nb + Q_TILE, j * 64, p.do_sl, p, wave);
    else dd_.issue(rdo, nb + Q_TILE, (unsigned)j * do_step, wave);
    if (wave == 0) {  // 64 rows x 4 B each: lse2 then delta
      char* st = stats + par * 512;
      const unsigned sa = lds_addr_of(st);
      lds_dma4(rl2, sa, (unsigned)((j * 64 + lane) * 4));
      lds_dma4(rdl, sa + 256, (unsigned)((j * 64 + lane) * 4));
    }
  };
  // this workgroup's query tiles [j0, j1) (all of them unless the query range is split)
  const int nqt_all = (p.Lq + 63) / 64, jper = (nqt_all + p.q_split - 1) / (p.q_split > 0 ? p.q_split : 1);
  [[maybe_unused]] const TfQTiles<TF, BAND> tt(p, key0, nqt_all);  // TF, BAND: the two tile ranges; j0 .. j1 then count visits
  const int j0 = TWO ? 0 : fm_first_qtile<FM>(p, key0, sp * jper);
  int j1 = TWO ? tt.nit : min(nqt_all, j0 + jper);
  if constexpr (WIN) j1 = fm_win_qtiles(p, key0, nqt_all);  // the sweep ends below qend of the last key (a lead key: all tiles)
  if constexpr (TWO) issue_tile(tt.tile(0), 0);
  else issue_tile(j0, 0);
  // FM: the lane's qstart, and the wave's largest (its last key's, the sequence's last row at most)
  [[maybe_unused]] int qlim = 0, wqlim = 0;
  if constexpr (FM) {
    qlim = fm_qstart(p, krow);
    wqlim = __builtin_amdgcn_readfirstlane(fm_qstart(p, min(key0 + wave * 32 + 31, p.Lk - 1)));
  }
  // WIN: the lane's qend next to its qstart, and the wave's smallest -- its first TOKEN key's (a lead key's is L)
  [[maybe_unused]] int qhi = 0, wqhi = 0;
  if constexpr (WIN) {
    qhi = fm_qend(p, krow);
    wqhi = __builtin_amdgcn_readfirstlane(fm_qend(p, fm_win_first_token_key(p, key0 + wave * 32)));
  }
  // TF: the lane's three reader bounds; the wave's largest qstart and q2 (its last key's; q2 = L with a lead key in the
  // wave) and its smallest qend (its first token key's)
  [[maybe_unused]] int q2 = 0, wq2 = 0;
  if constexpr (TF) {
    const TfMap tf(p);
    const int wk0 = key0 + wave * 32, wk1 = min(wk0 + 31, p.Lk - 1);
    qlim = tf.qstart(krow);
    qhi = tf.qend(krow);
    q2 = tf.q2(krow);
    wqlim = __builtin_amdgcn_readfirstlane(tf.qstart(wk1));
    wqhi = __builtin_amdgcn_readfirstlane(tf.qend(fm_win_first_token_key(p, wk0)));
    wq2 = wk0 >= tf.lead ? __builtin_amdgcn_readfirstlane(tf.q2(wk1)) : p.Lq;
  }
  // BAND: the lane's run [qlim, qhi) and the row its compare starts at (q2: lead, or L for a lead key); the wave's open
  // prefix (wq2: every row for lead keys only, lead for token keys only, nothing for both) and run [wqlim, wqhi)
  if constexpr (BAND) {
    const BandMap bm(p);
    const int wk0 = key0 + wave * 32, wk1 = min(wk0 + 31, p.Lk - 1);
    qlim = bm.lo(krow);
    qhi = bm.hi(krow);
    q2 = bm.pend(krow);
    if (wk1 < bm.lead) {
      wq2 = 0x3fffffff;
    } else if (wk0 >= bm.lead) {
      wq2 = bm.lead;
      wqlim = __builtin_amdgcn_readfirstlane(bm.lo(wk1));
      wqhi = __builtin_amdgcn_readfirstlane(bm.hi(wk0));
    }
  }

  // this lane's key row as B-operand fragments (rows past Lk / columns past hd read as zero)
  bf16x8 kf[KSQ], vf[KSQ];
#pragma unroll
  for (int ks = 0; ks < KSQ; ++ks) {
    const int e = ks * 16 + 8 * h;
    unsigned offk = (unsigned)(((long)krow * p.k_sl + e) * 2);
    unsigned offv = (unsigned)(((long)krow * p.v_sl + e) * 2);
    if (e >= p.hd) { offk = 0xfffffff0u; offv = 0xfffffff0u; }
    kf[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rk, offk, 0, 0));
    vf[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv, offv, 0, 0));
  }
  if constexpr (ONES) {
#pragma unroll
    for (int ks = 0; ks < KSQ; ++ks) kf[ks] = scale_frag(kf[ks], c);
    if (h == 1) {  // columns hd, hd+1 of every key row: 1.0 (they meet -lse2 hi, lo in the Q pad)
      kf[KSQ - 1][0] = (__bf16)1.0f;
      kf[KSQ - 1][1] = (__bf16)1.0f;
    }
  }

  f32x16 dk[NDB], dv[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) { dk[i] = zero16(); dv[i] = zero16(); }
#pragma unroll
  for (int ks = 0; ks < KSQ; ++ks) { retire(kf[ks]); retire(vf[ks]); }
  VDS_WAIT_VM(0);
  __syncthreads();  // tile j0 landed

  auto q_tile = [&](int it, auto PAR) {  // unrolled by two: compile-time LDS buffer parity (see the forward kernel)
    constexpr int par = decltype(PAR)::value;
    int j = it, jn = it + 1;  // this visit's query tile and the next one's (TF: across the gap between the two ranges)
    if constexpr (TWO) { j = tt.tile(it); jn = tt.tile(it + 1); }
    if (it + 1 < j1) issue_tile(jn, par ^ 1);
    const char* qt = qbuf + par * 2 * Q_TILE;
    const char* dot = qt + Q_TILE;
    const float* stl = reinterpret_cast<const float*>(stats + par * 512);
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      f32x16 s = zero16(), dp;
      // the dP accumulator starts at -delta of its rows (register r <-> row (r&3) + 8 (r>>2) + 4 h:
      // four 16-byte LDS reads land exactly on registers 4 rg .. 4 rg + 3)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(stl + 64 + qb * 32 + 8 * rg + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) dp[4 * rg + e] = d4[e];
      }
      PRIO_HI();
#pragma unroll
      for (int ks = 0; ks < KSQ; ++ks) {
        s = mfma32(frag_row<HDP>(qt, qb * 32, ks, lane), kf[ks], s);
        dp = mfma32(frag_row<HDP>(dot, qb * 32, ks, lane), vf[ks], dp);
      }
      PRIO_LO();
      f32x16 pm;
      if constexpr (ONES) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pr = __builtin_amdgcn_exp2f(s[r]);
          pm[r] = pr;
          s[r] = pr * dp[r];  // dS (unscaled)
        }
      } else {
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(stl + qb * 32 + 8 * rg + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * rg + e;
            const float pr = __builtin_amdgcn_exp2f(s[r] * c - l4[e]);
            pm[r] = pr;
            s[r] = pr * dp[r];  // dS (unscaled)
          }
        }
      }
      // (built here and not in the prologue as in the forward / dQ kernels: a prologue copy, though dead without CAUSAL,
      // changed the register allocation of this kernel's unmasked instances)
      if constexpr (CAUSAL) {  // (the map and the lane's key are loop-invariant: hoisted by the compiler)
        const FcMap fm(p);
        fc_zero_q(fm, j * 64 + qb * 32 + 4 * h, fm.fk(krow), pm, s);
      }
      if constexpr (BAND) {  // open: wholly below the wave's open prefix, or wholly inside the run every key of it shares
        const int s0 = j * 64 + qb * 32;
        if (s0 + 32 > wq2 && (s0 < wqlim || s0 + 32 > wqhi)) fm_zero_q_band(s0 + 4 * h, q2, qlim, qhi, pm, s);
      } else if constexpr (TF) {  // open: inside every key's first range, or at or past the wave's largest q2
        const int s0 = j * 64 + qb * 32;
        if ((s0 < wqlim || s0 + 32 > wqhi) && s0 < wq2) fm_zero_q_tf(s0 + 4 * h, qlim, qhi, q2, pm, s);
      } else if constexpr (WIN) {  // open: at or past the wave's largest qstart and wholly below its smallest qend
        if (j * 64 + qb * 32 < wqlim || j * 64 + qb * 32 + 32 > wqhi)
          fm_zero_q_win(j * 64 + qb * 32 + 4 * h, qlim, qhi, pm, s);
      } else if constexpr (FM) {
        if (j * 64 + qb * 32 < wqlim) fm_zero_q(j * 64 + qb * 32 + 4 * h, qlim, pm, s);
      }
      PRIO_HI();
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pf = acc_frag(pm, s2);
        const bf16x8 df = acc_frag(s, s2);
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          dv[db] = mfma32(frag_tr<HDP>(dot, qb * 32 + 16 * s2, db * 32, lane), pf, dv[db]);
          dk[db] = mfma32(frag_tr<HDP>(qt, qb * 32 + 16 * s2, db * 32, lane), df, dk[db]);
        }
      }
      PRIO_LO();
    }
    VDS_WAIT_VM(0);
    __syncthreads();
  };
  for (int j = j0; j < j1; j += 2) {
    q_tile(j, std::integral_constant<int, 0>{});
    if (j + 1 < j1) q_tile(j + 1, std::integral_constant<int, 1>{});
  }
  if constexpr (KVLEN) {
    if (krow >= Lk) {  // P of a zero key row is not zero: its sums are dropped here
#pragma unroll
      for (int i = 0; i < NDB; ++i) { dk[i] = zero16(); dv[i] = zero16(); }
    }
  }
  if (krow < p.Lk) {
    if (p.q_split > 1) {  // fp32 partial of this query range (an empty range stores zeros); dkv_reduce_kernel finishes
      float* part = p.dkv_part + ((((long)sp * p.B * p.H + bh) * p.Lk + krow) * 2) * p.hd;
      store_rows_f32<NDB>(part, dk, p.hd, h);
      store_rows_f32<NDB>(part + p.hd, dv, p.hd, h);
    } else {
      store_rows<NDB>(p.dk + b * p.dk_sb + hh * p.dk_sh + (long)krow * p.dk_sl, dk, p.scale, p.hd, h);
      store_rows<NDB>(p.dv + b * p.dv_sb + hh * p.dv_sh + (long)krow * p.dv_sl, dv, 1.0f, p.hd, h);
    }
  }
}

// ===================================== dK, dV on v_mfma_f32_16x16x32_bf16 ====================
// The attention kernels run power-throttled (the same instruction stream takes 21-25 % less time on all-zero
// operands: gpurun_out/r02e), so what counts is energy per FLOP; MI355X_MICROARCH.md, DVFS item 7:
// the 16x16x32 shape delivers ~1.12-1.15x the FLOP/s of 32x32x16 at equal cycles because the chip holds a higher
// clock on it.  Same algorithm and data flow as attn_bwd_dkv_kernel<96, 80, true> (head_dim 72, ones columns):
//   F1  S[r, c] = sum_k Q[r,k] K[c,k]        A = 16 query rows from LDS (ds_read_b128), B = 16 key rows in registers,
//                                            k in 3 steps of 32 over the 96 padded columns; output: key c on the lane
//                                            (l & 15), query rows 4 (l >> 4) .. + 3
//   F2  dV^T[d, c] += sum_r dO[r,d] P[r,c]   B = the S / dP accumulators of the two 16-row query blocks of a 32-row
//                                            sub-block, used in place (lane (c, g) holds rows 4g..4g+3 of both blocks
//                                            = the 8 contraction indices the MFMA wants from it); A = dO^T read with
//                                            two transposing 4 x 16 reads at rows R + 4g, R + 16 + 4g
// A wave owns 32 keys as two 16-key column blocks; head_dim pads to 96 for the contractions (3 x 32) and to 80 for
// the outputs (5 x 16): 44 MFMAs of 16 cycles per 32 x 32 block = the 704 cycles of the 32x32x16 kernel.
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <int HDP>
__device__ __forceinline__ bf16x8 frag16_row(const char* tile, int row0, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(tile + imgb_off<HDP>(row0 + (lane & 15), ks * 4 + (lane >> 4)));
}
// A operand of F2: (T^T)[d0 .. d0+15][32 rows r0 ..]: contraction index 8g + j <-> row r0 + 4g + j (j < 4),
// r0 + 16 + 4g + (j - 4) (j >= 4) -- the order in which lane (c, g) holds two stacked 16-row accumulators
template <int HDP>
__device__ __forceinline__ bf16x8 frag16_tr(const char* tile, int r0, int d0, int lane) {
  const int g = lane >> 4, i = lane & 15, qq = i >> 2, pp = i & 3;
  const int row = r0 + 4 * g + qq;
  const int ch = (d0 >> 3) + (pp >> 1);
  const char* p0 = tile + imgb_off<HDP>(row, ch) + 8 * (pp & 1);
  const char* p1 = tile + imgb_off<HDP>(row + 16, ch) + 8 * (pp & 1);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p0));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p1));
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}
__device__ __forceinline__ bf16x8 pack2(const f32x4& a, const f32x4& b) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) { r[j] = (__bf16)a[j]; r[4 + j] = (__bf16)b[j]; }
  return r;
}

// QPAD = false (round 5, cross-attention: vds_attn_args.kv_pad_ones = 2): the q rows carry no annotated pad (token-major
// views of a linear layer's output), so only head_dim columns of a q row are staged and the S accumulators START from
// -lse2 of their queries, read from the statistics this kernel stages beside -delta anyway.
// KVLEN: as in attn_bwd_dkv_kernel; 16-key blocks past kv_lens[b] are not computed at all (NKB).
// CAUSAL: a lane holds one key per 16-key block (fk fixed) and its registers walk the queries 16 rb + 4 g + r of the
// sub-block: x(query) is formed once per register and serves both key blocks; P and dS of excluded pairs become zero.
// FM (vds_attn_bwd_causal_fm, ones layout): as attn_bwd_dkv_kernel's -- the query sweep starts at the tile that holds qstart
// of the workgroup's first key, a lane compares the query row of each register against the qstart of its two keys unless
// the sub-block starts at or past the qstart of the wave's last key, and the dO tile is gathered from the token rows.
// WIN (vds_attn_bwd_causal_fm_window; with FM): as attn_bwd_dkv_kernel's.
template <int HDP, bool QPAD = true, bool KVLEN = false, bool CAUSAL = false, bool FM = false, bool WIN = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv16_kernel(AttnP p) {
  static_assert(HDP == 96, "head_dim 72 layout (ones columns at 72, 73)");
  static_assert(!WIN || FM, "the window: on frame-major rows");
  static_assert(!FM || (QPAD && !KVLEN && !CAUSAL), "frame-major: the ones layout, its own mask");
  constexpr int KS = HDP / 32, NDB = 5, Q_TILE = 64 * HDP * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qbuf = smem;
  char* stats = smem + 4 * Q_TILE;
  int bh, kt_idx;
  if (!decode_block(p.n_rt, p.tail_last, p.B * p.H, bh, kt_idx)) return;
  const int b = bh / p.H, hh = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int key0 = kt_idx * 128 + wave * 32;
  const int Lk = kv_len_of<KVLEN>(p, b);
  if constexpr (KVLEN) {
    if (kt_idx * 128 >= Lk) {  // no key of this tile is attended (all 64 lanes call the store: it exchanges lanes)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int krow = key0 + cb * 16 + (lane & 15);
        store_zero_block(p.dk + b * p.dk_sb + hh * p.dk_sh + (long)krow * p.dk_sl, p.hd, g, krow < p.Lk, p.wide_dkv);
        store_zero_block(p.dv + b * p.dv_sb + hh * p.dv_sh + (long)krow * p.dv_sl, p.hd, g, krow < p.Lk, p.wide_dkv);
      }
      return;
    }
  }

  const int hd_q = QPAD ? p.hd + 8 : p.hd;  // QPAD: Q rows are staged with their pad: -lse*log2(e) as (hi, lo) at columns hd, hd+1
  const srd_t rq = slice_srd(p.q + b * p.q_sb + hh * p.q_sh, p.q_sl, p.Lq, hd_q);
  const srd_t rdo = slice_srd(p.d_o + b * p.do_sb + hh * p.do_sh, p.do_sl, p.Lq, p.hd);
  const __amdgpu_buffer_rsrc_t rk = slice_rsrc(p.k + b * p.k_sb + hh * p.k_sh, p.k_sl, Lk, p.hd);
  const __amdgpu_buffer_rsrc_t rv = slice_rsrc(p.v + b * p.v_sb + hh * p.v_sh, p.v_sl, Lk, p.hd);
  const long nrows = (long)p.B * p.H * p.Lq;
  const long srow0 = ((long)b * p.H + hh) * p.Lq;
  const srd_t rdl = make_srd(p.delta + srow0, (unsigned)(p.Lq * 4));
  const srd_t rl2 = make_srd(p.delta + nrows + srow0, (unsigned)(p.Lq * 4));
  const float c = p.scale * LOG2E;

  DmaStage<64, HDP, 1> dq_;
  std::conditional_t<FM, DmaStageFm<64, HDP, 1>, DmaStage<64, HDP, 1>> dd_;
  dq_.init(p.q_sl, hd_q, wave, lane);
  if constexpr (FM) dd_.init(p.hd, wave, lane);
  else dd_.init(p.do_sl, p.hd, wave, lane);
  const unsigned q_step = (unsigned)(64 * p.q_sl * 2), do_step = (unsigned)(64 * p.do_sl * 2);
  auto issue_tile = [&](int j, int par) {
    char* nb = qbuf + par * 2 * Q_TILE;
    dq_.issue(rq, nb, (unsigned)j * q_step, wave);
    if constexpr (FM) dd_.issue(rdo, nb + Q_TILE, j * 64, p.do_sl, p, wave);
    else dd_.issue(rdo, nb + Q_TILE, (unsigned)j * do_step, wave);
    if (wave == 0) {
      char* st = stats + par * 512;
      const unsigned sa = lds_addr_of(st);
      lds_dma4(rl2, sa, (unsigned)((j * 64 + lane) * 4));
      lds_dma4(rdl, sa + 256, (unsigned)((j * 64 + lane) * 4));
    }
  };
  const int j0 = fm_first_qtile<FM>(p, kt_idx * 128, 0);  // first query tile of the sweep (0 unless FM)
  issue_tile(j0, 0);
  // FM: qstart of the lane's two keys, and the wave's largest (its last key's, the sequence's last row at most)
  [[maybe_unused]] int qlim[2] = {0, 0}, wqlim = 0;
  if constexpr (FM) {
    qlim[0] = fm_qstart(p, key0 + (lane & 15));
    qlim[1] = fm_qstart(p, key0 + 16 + (lane & 15));
    wqlim = __builtin_amdgcn_readfirstlane(fm_qstart(p, min(key0 + 31, p.Lk - 1)));
  }
  // WIN: qend of the lane's two keys, and the wave's smallest -- its first TOKEN key's (a lead key's is L)
  [[maybe_unused]] int qhi[2] = {0, 0}, wqhi = 0;
  if constexpr (WIN) {
    qhi[0] = fm_qend(p, key0 + (lane & 15));
    qhi[1] = fm_qend(p, key0 + 16 + (lane & 15));
    wqhi = __builtin_amdgcn_readfirstlane(fm_qend(p, fm_win_first_token_key(p, key0)));
  }

  // the two 16-key blocks of this wave as B operands: lane (c = l & 15, g) holds columns 32 ks + 8 g .. + 7 of key c
  bf16x8 kf[2][KS], vf[2][KS];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int krow = key0 + cb * 16 + (lane & 15);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int e = ks * 32 + 8 * g;
      unsigned offk = (unsigned)(((long)krow * p.k_sl + e) * 2);
      unsigned offv = (unsigned)(((long)krow * p.v_sl + e) * 2);
      if (e >= p.hd) { offk = 0xfffffff0u; offv = 0xfffffff0u; }
      kf[cb][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rk, offk, 0, 0));
      vf[cb][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv, offv, 0, 0));
    }
  }
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) { kf[cb][ks] = scale_frag(kf[cb][ks], c); retire(vf[cb][ks]); }
    if (g == 1) {  // ks = 2, g = 1: columns 72 .. 79; 1.0 at 72, 73 meets -lse2 (hi, lo) in the Q pad
      kf[cb][KS - 1][0] = (__bf16)1.0f;
      kf[cb][KS - 1][1] = (__bf16)1.0f;
    }
  }

  f32x4 dk[NDB][2], dv[NDB][2];
#pragma unroll
  for (int i = 0; i < NDB; ++i)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) { dk[i][cb] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[i][cb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  int nqt = (p.Lq + 63) / 64;  // one past the last query tile of the sweep
  if constexpr (WIN) nqt = fm_win_qtiles(p, kt_idx * 128, nqt);
  VDS_WAIT_VM(0);
  __syncthreads();  // tile 0 landed

  // NKB: 16-key blocks of this wave that hold keys (2 except in the head's last workgroup, which owns the 16 register
  // tokens at L = 8208: its other waves only stage and synchronise; see attn_fwd16_kernel)
  auto q_tile = [&](int j, auto PAR, auto NKBT) {
    constexpr int par = decltype(PAR)::value;
    constexpr int NKB = decltype(NKBT)::value;
    if (j + 1 < nqt) issue_tile(j + 1, par ^ 1);
    const char* qt = qbuf + par * 2 * Q_TILE;
    const char* dot = qt + Q_TILE;
    const float* stl = reinterpret_cast<const float*>(stats + par * 512);
    if constexpr (NKB > 0)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      f32x4 s[2][2], dp[2][2];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(stl + 64 + qb * 32 + rb * 16 + 4 * g);  // -delta of rows 4g..
        f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (!QPAD) s0 = -*reinterpret_cast<const f32x4*>(stl + qb * 32 + rb * 16 + 4 * g);  // -lse2 of rows 4g..
#pragma unroll
        for (int cb = 0; cb < NKB; ++cb) { s[rb][cb] = s0; dp[rb][cb] = d4; }
      }
      PRIO_HI();
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          const bf16x8 aq = frag16_row<HDP>(qt, qb * 32 + rb * 16, ks, lane);
          const bf16x8 ad = frag16_row<HDP>(dot, qb * 32 + rb * 16, ks, lane);
#pragma unroll
          for (int cb = 0; cb < NKB; ++cb) {
            s[rb][cb] = mfma16(aq, kf[cb][ks], s[rb][cb]);
            dp[rb][cb] = mfma16(ad, vf[cb][ks], dp[rb][cb]);
          }
        }
      PRIO_LO();
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < NKB; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[rb][cb][r] = __builtin_amdgcn_exp2f(s[rb][cb][r]);  // S came out of the MFMA as log2 P
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < NKB; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) dp[rb][cb][r] *= s[rb][cb][r];  // dS (unscaled)
      if constexpr (CAUSAL) {  // (the map and the lane's keys are loop-invariant: hoisted by the compiler)
        const FcMap fm(p);
        const int fck[2] = {fm.fk(key0 + (lane & 15)), fm.fk(key0 + 16 + (lane & 15))};
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int xq = fm.x(j * 64 + qb * 32 + rb * 16 + 4 * g + r);
#pragma unroll
            for (int cb = 0; cb < NKB; ++cb)
              if (xq < fck[cb]) { s[rb][cb][r] = 0.f; dp[rb][cb][r] = 0.f; }
          }
      }
      if constexpr (WIN) {  // open: at or past the wave's largest qstart and wholly below its smallest qend
        if (j * 64 + qb * 32 < wqlim || j * 64 + qb * 32 + 32 > wqhi) {
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int qr = j * 64 + qb * 32 + rb * 16 + 4 * g + r;
#pragma unroll
              for (int cb = 0; cb < NKB; ++cb)
                if (qr < qlim[cb] || qr >= qhi[cb]) { s[rb][cb][r] = 0.f; dp[rb][cb][r] = 0.f; }
            }
        }
      } else if constexpr (FM) {
        if (j * 64 + qb * 32 < wqlim) {
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int qr = j * 64 + qb * 32 + rb * 16 + 4 * g + r;
#pragma unroll
              for (int cb = 0; cb < NKB; ++cb)
                if (qr < qlim[cb]) { s[rb][cb][r] = 0.f; dp[rb][cb][r] = 0.f; }
            }
        }
      }
      bf16x8 pf[2], df[2];
#pragma unroll
      for (int cb = 0; cb < NKB; ++cb) {
        pf[cb] = pack2(s[0][cb], s[1][cb]);
        df[cb] = pack2(dp[0][cb], dp[1][cb]);
      }
      PRIO_HI();
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const bf16x8 ado = frag16_tr<HDP>(dot, qb * 32, db * 16, lane);
        const bf16x8 aqt = frag16_tr<HDP>(qt, qb * 32, db * 16, lane);
#pragma unroll
        for (int cb = 0; cb < NKB; ++cb) {
          dv[db][cb] = mfma16(ado, pf[cb], dv[db][cb]);
          dk[db][cb] = mfma16(aqt, df[cb], dk[db][cb]);
        }
      }
      PRIO_LO();
    }
    VDS_WAIT_VM(0);
    __syncthreads();
  };
  auto run = [&](auto NKBT) {
    for (int j = j0; j < nqt; j += 2) {
      q_tile(j, std::integral_constant<int, 0>{}, NKBT);
      if (j + 1 < nqt) q_tile(j + 1, std::integral_constant<int, 1>{}, NKBT);
    }
  };
  const int nkb = min(2, max(0, (Lk - key0 + 15) >> 4));  // wave-uniform
  if (nkb == 2) run(std::integral_constant<int, 2>{});
  else if (nkb == 1) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 0>{});
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int krow = key0 + cb * 16 + (lane & 15);
    float vk[NDB][4], vv[NDB][4];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) { vk[db][e] = dk[db][cb][e]; vv[db][e] = dv[db][cb][e]; }
    if constexpr (KVLEN) {
      if (krow >= Lk) {  // P of a zero key row is not zero: its sums are dropped here
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int e = 0; e < 4; ++e) { vk[db][e] = 0.f; vv[db][e] = 0.f; }
      }
    }
    store_block_bf16_t(vk, p.scale, p.dk + b * p.dk_sb + hh * p.dk_sh + (long)krow * p.dk_sl, p.hd, g, krow < p.Lk, p.wide_dkv);
    store_block_bf16_t(vv, 1.0f, p.dv + b * p.dv_sb + hh * p.dv_sh + (long)krow * p.dv_sl, p.hd, g, krow < p.Lk, p.wide_dkv);
  }
}

// ===================================== forward on v_mfma_f32_16x16x32_bf16 ====================
// attn_fwd_wide_kernel<96, 80, true> (head_dim 72, ones columns, 64 queries per wave) on the 16x16x32 shape, for the
// reason given at attn_bwd_dkv16_kernel (higher held clock at equal MFMA cycles).  S^T = K Q'^T with 16 key rows from
// LDS as A and 16 queries in registers as B (k in 3 steps of 32); O^T += V^T P^T with V^T read by two transposing
// 4 x 16 reads and the two stacked S accumulators of a 32-key sub-block used in place as B.  A wave owns 4 query
// blocks of 16; lane (c = l & 15, g = l >> 4) holds key rows 4g..4g+3 of each 16-key block of query c.  The ones-column
// softmax is unchanged: -m rides in column head_dim of Q', the denominator comes out of the PV MFMA as rows head_dim
// (lanes g = 2) and head_dim + 4 (g = 3) of O^T, the running maximum is raised lazily (wave-uniform branch).
__device__ __forceinline__ float max3f(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ float max_over_lane_groups(float x) {  // max over the 4 lanes l & 15 + 16 g
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// CAUSAL: a lane holds one query per 16-query block (fq fixed) and its registers walk the keys 16 rb + 4 g + r of the
// sub-block: x(key) is formed once per register and serves all four query blocks.
// FM (vds_attn_fwd_causal_fm, ones layout): as attn_fwd_kernel's -- the key loop ends at the largest kend of the
// workgroup's 256 queries, a lane compares the key row of each register against the kend of its four queries unless the
// sub-block lies below the kend of the wave's first query, the o row goes to tok(row), and a query's running maximum is
// raised only when its OWN scores cross the threshold (rows of several frames share a wave).
// WIN (vds_attn_fwd_causal_fm_window; with FM): as attn_fwd_kernel's -- the two tile ranges, the per-lane compare
// against [kbeg, kend) of the lane's four queries, the open test -- and a first maximum per query (see `unset`).
template <int HDP, bool KVLEN = false, bool CAUSAL = false, bool PAST = false, bool FM = false, bool WIN = false>
__global__ __launch_bounds__(256, 2) void attn_fwd16_kernel(AttnP p) {
  static_assert(HDP == 96, "head_dim 72 layout (ones columns at 72, 73 / 72, 76)");
  static_assert(!WIN || FM, "the window: on frame-major rows");
  static_assert(!FM || !(KVLEN || CAUSAL || PAST), "frame-major: its own mask");
  constexpr int KS = HDP / 32, NDB = 5, TILE = 64 * HDP * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bh, qt;
  if (!decode_block(p.n_rt, p.tail_last, p.B * p.H, bh, qt)) return;
  if constexpr (FM) qt = fm_tile(p, qt);
  const int b = bh / p.H, hh = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qrow0 = qt * 256 + wave * 64 + (lane & 15);  // query of block 0; block cb = + 16 cb
  const int hd_kv = p.hd + 8;
  const int Lk = fm_keys<FM>(p, qt * 256, 256, kv_len_of<KVLEN>(p, b));
  if constexpr (KVLEN) {
    if (Lk == 0) {  // no context: O = 0, lse = 0 (all 64 lanes call the store: it exchanges lanes)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int qrow = qrow0 + 16 * cb;
        store_zero_block(p.o + b * p.o_sb + hh * p.o_sh + (long)qrow * p.o_sl, p.hd, g, qrow < p.Lq, p.wide_o);
        if (qrow < p.Lq && g == 0) p.lse[((long)b * p.H + hh) * p.Lq + qrow] = 0.0f;
      }
      return;
    }
  }

  const __amdgpu_buffer_rsrc_t rq = slice_rsrc(p.q + b * p.q_sb + hh * p.q_sh, p.q_sl, p.Lq, p.hd);
  const srd_t rk = slice_srd(p.k + b * p.k_sb + hh * p.k_sh, p.k_sl, Lk, hd_kv);
  const srd_t rv = slice_srd(p.v + b * p.v_sb + hh * p.v_sh, p.v_sl, Lk, hd_kv);
  DmaStage<64, HDP, 1> dk, dv;
  dk.init(p.k_sl, hd_kv, wave, lane);
  dv.init(p.v_sl, hd_kv, wave, lane);
  const unsigned k_step = (unsigned)(64 * p.k_sl * 2), v_step = (unsigned)(64 * p.v_sl * 2);
  const int nkt = (Lk + 63) / 64;
  [[maybe_unused]] const FmWinTiles<WIN> wt(p, qt * 256, 256, nkt);  // WIN: as in attn_fwd_kernel
  const int nit = WIN ? wt.nit : nkt;
  if constexpr (WIN) {
    dk.issue(rk, smem, (unsigned)wt.tile(0) * k_step, wave);
    dv.issue(rv, smem + TILE, (unsigned)wt.tile(0) * v_step, wave);
  } else {
  dk.issue(rk, smem, 0, wave);
  dv.issue(rv, smem + TILE, 0, wave);
  }

  const float c = p.scale * LOG2E;
  bf16x8 qf[4][KS];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int e = ks * 32 + 8 * g;
      unsigned off = (unsigned)(((long)(qrow0 + 16 * cb) * p.q_sl + e) * 2);
      if (e >= p.hd) off = 0xfffffff0u;
      qf[cb][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, 0));
    }
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[cb][ks] = scale_frag(qf[cb][ks], c);  // also retires the loads

  f32x4 o[NDB][4];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) o[db][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m[4] = {0.f, 0.f, 0.f, 0.f};
  const FcMap fm(p);
  int fcq[4] = {0, 0, 0, 0};
  if constexpr (CAUSAL) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) fcq[cb] = fm.fq(qrow0 + 16 * cb);
  }
  [[maybe_unused]] const int wq0 = qt * 256 + wave * 64;  // PAST: the wave's first query row
  [[maybe_unused]] int klim[4] = {0, 0, 0, 0}, wklim = 0;  // FM: kend of the lane's queries; the wave's smallest (0: none open)
  if constexpr (FM) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) klim[cb] = fm_kend(p, qrow0 + 16 * cb);
    wklim = wq0 >= p.fc_lead ? __builtin_amdgcn_readfirstlane(fm_kend(p, wq0)) : 0;
  }
  // WIN: kbeg of the lane's queries and the wave's open test.  unset[cb]: the query has met no attended key yet -- with
  // lead = 0 the first sub-blocks a wave visits may lie before a later query's window, so each query takes its first
  // maximum from the first sub-block that holds one of ITS keys (m stays 0 and every P is 0 until then)
  [[maybe_unused]] int kbeg[4] = {0, 0, 0, 0};
  [[maybe_unused]] bool unset[4] = {true, true, true, true};
  [[maybe_unused]] const FmWinOpen<WIN> wo(p, wq0, 64);
  if constexpr (WIN) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) kbeg[cb] = fm_kbeg(p, qrow0 + 16 * cb);
  }
  VDS_WAIT_VM(0);
  __syncthreads();

  // NCB: query blocks of this wave that hold queries: 4 except in a head's last workgroup (16 of its 256 queries are
  // real at L = 8208), whose other waves only stage and synchronise -- that workgroup then runs at the pace of the one
  // wave that has a block instead of occupying a CU slot for the time of a full one.  Invisible at B = 12 (12.4 rounds
  // of workgroups either way), but at B = 2 the 33rd workgroup of every head opens a third round.
  auto kv_tile = [&](int it, auto PAR, auto NCBT) {
    constexpr int par = decltype(PAR)::value;
    constexpr int NCB = decltype(NCBT)::value;
    int j = it, jn = it + 1;  // this visit's key tile and the next one's (WIN: across the gap)
    if constexpr (WIN) { j = wt.tile(it); jn = wt.tile(it + 1); }
    if (it + 1 < nit) {
      char* nk = smem + (par ^ 1) * 2 * TILE;
      dk.issue(rk, nk, (unsigned)jn * k_step, wave);
      dv.issue(rv, nk + TILE, (unsigned)jn * v_step, wave);
    }
    const char* kt = smem + par * 2 * TILE;
    const char* vt = kt + TILE;
    if constexpr (NCB > 0)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x4 s[2][4];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) s[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      PRIO_HI();
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          const bf16x8 ak = frag16_row<HDP>(kt, kb * 32 + rb * 16, ks, lane);
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) s[rb][cb] = mfma16(ak, qf[cb][ks], s[rb][cb]);
        }
      PRIO_LO();
      // keys past Lk need no mask: their zero-filled V rows (ones columns included) add nothing to the numerators or
      // to the denominator, whatever exp2 makes of their scores
      // (the frame mask cannot lean on zero V rows: the scores themselves go to -inf, before the maxima -- key 0 is
      // attended by every query, so the first sub-block's maximum is finite)
      if constexpr (PAST) {
        if (!fc_past_open(fm, p.fc_past, j * 64 + kb * 32, wq0)) {
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int xk = fm.x(fc_past_row(fm, p.fc_past, j * 64 + kb * 32 + rb * 16 + 4 * g + r));
#pragma unroll
              for (int cb = 0; cb < NCB; ++cb)
                if (xk > fcq[cb]) s[rb][cb][r] = -INFINITY;
            }
        }
      } else if constexpr (CAUSAL) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int xk = fm.x(j * 64 + kb * 32 + rb * 16 + 4 * g + r);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
              if (xk > fcq[cb]) s[rb][cb][r] = -INFINITY;
          }
      }
      if constexpr (WIN) {
        if (!wo.open(j * 64 + kb * 32)) {
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = j * 64 + kb * 32 + rb * 16 + 4 * g + r;
#pragma unroll
              for (int cb = 0; cb < NCB; ++cb)
                if (fm_win_masked(key, p.fc_lead, kbeg[cb], klim[cb])) s[rb][cb][r] = -INFINITY;
            }
        }
      } else if constexpr (FM) {
        if (j * 64 + kb * 32 + 32 > wklim) {
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = j * 64 + kb * 32 + rb * 16 + 4 * g + r;
#pragma unroll
              for (int cb = 0; cb < NCB; ++cb)
                if (key >= klim[cb]) s[rb][cb][r] = -INFINITY;
            }
        }
      }
      const bool first = !WIN && (j == 0) && (kb == 0);
      float mx[4];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        // 4 instructions per query block as three-operand maxima (the issue port is ~90 % booked: tools/probes)
        mx[cb] = max3f(max3f(s[0][cb][0], s[0][cb][1], s[0][cb][2]), max3f(s[0][cb][3], s[1][cb][0], s[1][cb][1]),
                       fmaxf(s[1][cb][2], s[1][cb][3]));
      }
      float mxa = mx[0];
      if constexpr (NCB == 4) mxa = fmaxf(max3f(mx[0], mx[1], mx[2]), mx[3]);
      else {
#pragma unroll
        for (int cb = 1; cb < NCB; ++cb) mxa = fmaxf(mxa, mx[cb]);
      }
      bool fresh = false;  // WIN: a query of this lane meets its first attended key here
      if constexpr (WIN) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) fresh |= unset[cb] && mx[cb] > -INFINITY;
      }
      if (first || __builtin_amdgcn_ballot_w64(mxa > LAZY_THR || fresh) != 0) {  // wave-uniform, rare after the first tile
        asm volatile("; rescale" ::: "memory");  // keeps this a real branch (no if-conversion of the O multiplies)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const float mxf = max_over_lane_groups(mx[cb]);  // all four lanes of a query agree
          bool first_q = first;  // this query takes its first maximum here
          if constexpr (WIN) {
            first_q = unset[cb] && mxf > -INFINITY;
            unset[cb] = unset[cb] && !first_q;
          }
          float m_new = bf2f(f2bf(m[cb] + (first_q ? mxf : fmaxf(mxf, 0.f))));
          if constexpr (FM) {
            if (!first_q && !(mxf > LAZY_THR)) m_new = m[cb];  // only the query's own scores move its maximum
          }
          const float delta = m_new - m[cb];
          const float alpha = first_q ? 1.0f : __builtin_amdgcn_exp2f(-delta);
          m[cb] = m_new;
#pragma unroll
          for (int db = 0; db < NDB; ++db) o[db][cb] *= alpha;  // includes the denominator rows
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[rb][cb][r] -= delta;
          if (g == 1) qf[cb][KS - 1][0] = (__bf16)(-m_new);  // column head_dim of Q' (exact: m is a bf16 value)
        }
      }
      bf16x8 pf[4];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[rb][cb][r] = __builtin_amdgcn_exp2f(s[rb][cb][r]);
        pf[cb] = pack2(s[0][cb], s[1][cb]);
      }
      PRIO_HI();
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const bf16x8 av = frag16_tr<HDP>(vt, kb * 32, db * 16, lane);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) o[db][cb] = mfma16(av, pf[cb], o[db][cb]);
      }
      PRIO_LO();
    }
    VDS_WAIT_VM(0);
    __syncthreads();
  };
  auto run = [&](auto NCBT) {
    for (int it = 0; it < nit; it += 2) {
      kv_tile(it, std::integral_constant<int, 0>{}, NCBT);
      if (it + 1 < nit) kv_tile(it + 1, std::integral_constant<int, 1>{}, NCBT);
    }
  };
  const int ncb = min(4, max(0, (p.Lq - (qt * 256 + wave * 64) + 15) >> 4));  // wave-uniform
  if (ncb > 2) run(std::integral_constant<int, 4>{});
  else if (ncb == 2) run(std::integral_constant<int, 2>{});
  else if (ncb == 1) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 0>{});

#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int qrow = qrow0 + 16 * cb;
    // the denominator is row head_dim (= 64 + 4*2 + 0: lanes g = 2, register 0 of block 4) of O^T
    const float lt = __shfl(o[NDB - 1][cb][0], (lane & 15) | 32, 64);
    float vo[NDB][4];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) vo[db][e] = o[db][cb][e];
    store_block_bf16_t(vo, 1.0f / lt, p.o + b * p.o_sb + hh * p.o_sh + (long)out_row<FM>(p, qrow) * p.o_sl, p.hd, g, qrow < p.Lq,
                       p.wide_o);
    if (qrow < p.Lq && g == 0) p.lse[((long)b * p.H + hh) * p.Lq + qrow] = (m[cb] + __builtin_amdgcn_logf(lt)) * LN2;
  }
}

// ===================================== dQ on v_mfma_f32_16x16x32_bf16 =========================
// attn_bwd_dq_kernel<96, 80, true> on the 16x16x32 shape (see attn_bwd_dkv16_kernel).  S'^T = K Q'^T and
// dP^T = V dO'^T with 16 key rows from LDS as A and 16 queries in registers as B; dQ^T += K^T dS^T with K^T read by
// transposing reads and the stacked dS^T accumulators used in place as B.  Per 32 x 32 block: 34 MFMAs of 16 cycles
// (544) against 16 of 32 (512) -- the contraction pads 72 -> 96 instead of 80 -- in exchange for the higher clock.
// NQ = 2 16-query blocks per wave (three waves per SIMD) reads every K / V fragment for 2 MFMAs: at the full MFMA rate the
// 12 waves of a CU would keep the LDS 100 % busy (136 LDS cycles per wave and 32-key sub-block against 544 MFMA cycles per
// SIMD and wave) -- the kernel is LDS-bound.
// FOLD (round 6): the kernel is its own preprocess.  It holds the dO rows of its queries as fragments anyway; with the O
// rows loaded beside them (once per workgroup: 18 KiB) every lane forms  -delta = -rowsum(dO o O)  of its query (24 products,
// two cross-lane adds), writes -delta and lse * log2(e) to the workspace and the (hi, lo) pair of -lse2 into the pad of its
// Q row -- what attn_delta_*_kernel did in a pass of its own over O and dO (6.5 ms per C3b step).  The host then runs this
// kernel BEFORE the dK/dV kernel, which reads those statistics.
// FM (vds_attn_bwd_causal_fm, ones layout): as attn_bwd_dq_kernel's -- the key sweep ends at the largest kend of the
// workgroup's queries, dS is zeroed from the kend of the lane's queries unless the sub-block lies below the kend of the wave's
// first query, and the dO row -- with FOLD the O row too -- is that of token row tok(row); q, dq, the statistics written by
// FOLD and the annotated q pad are indexed by the frame-major row.
// WIN (vds_attn_bwd_causal_fm_window; with FM): as attn_bwd_dq_kernel's.
template <int HDP, bool FOLD = false, bool KVLEN = false, bool CAUSAL = false, bool FM = false, bool WIN = false>
__global__ __launch_bounds__(256, 3) void attn_bwd_dq16_kernel(AttnP p) {
  static_assert(HDP == 96, "head_dim 72 layout");
  static_assert(!WIN || FM, "the window: on frame-major rows");
  static_assert(!FM || !(KVLEN || CAUSAL), "frame-major: its own mask");
  constexpr int KS = HDP / 32, NDB = 5, TILE = 64 * HDP * 2, NQ = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bh, qt;
  if (!decode_block(p.n_rt, p.tail_last, p.B * p.H, bh, qt)) return;
  if constexpr (FM) qt = fm_tile(p, qt);
  const int b = bh / p.H, hh = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qrow0 = qt * (64 * NQ) + wave * (16 * NQ) + (lane & 15);  // query of column block 0; block cb = + 16 cb
  const int hd_kv = p.hd + 8;
  const int Lk = fm_keys<FM>(p, qt * (64 * NQ), 64 * NQ, kv_len_of<KVLEN>(p, b));
  if constexpr (KVLEN) {
    // no context: dQ = 0.  (FOLD: the statistics of this sample stay unwritten -- every dK/dV workgroup of a sample
    // without keys leaves before it reads them)
    if (Lk == 0) {
#pragma unroll
      for (int cb = 0; cb < NQ; ++cb) {
        const int qrow = qrow0 + 16 * cb;
        store_zero_block(p.dq + b * p.dq_sb + hh * p.dq_sh + (long)qrow * p.dq_sl, p.hd, g, qrow < p.Lq, p.wide_dq);
      }
      return;
    }
  }

  const __amdgpu_buffer_rsrc_t rq = slice_rsrc(p.q + b * p.q_sb + hh * p.q_sh, p.q_sl, p.Lq, p.hd);
  const __amdgpu_buffer_rsrc_t rdo = slice_rsrc(p.d_o + b * p.do_sb + hh * p.do_sh, p.do_sl, p.Lq, p.hd);
  const srd_t rk = slice_srd(p.k + b * p.k_sb + hh * p.k_sh, p.k_sl, Lk, hd_kv);
  const srd_t rv = slice_srd(p.v + b * p.v_sb + hh * p.v_sh, p.v_sl, Lk, hd_kv);
  DmaStage<64, HDP, 1> dk, dv;
  dk.init(p.k_sl, hd_kv, wave, lane);
  dv.init(p.v_sl, hd_kv, wave, lane);
  const unsigned k_step = (unsigned)(64 * p.k_sl * 2), v_step = (unsigned)(64 * p.v_sl * 2);
  const int nkt = (Lk + 63) / 64;
  [[maybe_unused]] const FmWinTiles<WIN> wt(p, qt * (64 * NQ), 64 * NQ, nkt);  // WIN: as in attn_fwd_kernel
  const int nit = WIN ? wt.nit : nkt;
  if constexpr (WIN) {
    dk.issue(rk, smem, (unsigned)wt.tile(0) * k_step, wave);
    dv.issue(rv, smem + TILE, (unsigned)wt.tile(0) * v_step, wave);
  } else {
  dk.issue(rk, smem, 0, wave);
  dv.issue(rv, smem + TILE, 0, wave);
  }

  const long nrows = (long)p.B * p.H * p.Lq;
  const float c = p.scale * LOG2E;
  bf16x8 qf[NQ][KS], dof[NQ][KS];
#pragma unroll
  for (int cb = 0; cb < NQ; ++cb) {
    const int qrow = qrow0 + 16 * cb;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int e = ks * 32 + 8 * g;
      unsigned off = (unsigned)(((long)qrow * p.q_sl + e) * 2);
      unsigned off2 = (unsigned)(((long)out_row<FM>(p, qrow) * p.do_sl + e) * 2);
      if (e >= p.hd) { off = 0xfffffff0u; off2 = 0xfffffff0u; }
      qf[cb][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, 0));
      dof[cb][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rdo, off2, 0, 0));
    }
    const long srow = ((long)b * p.H + hh) * p.Lq + min(qrow, p.Lq - 1);
    float ndl, lse2;
    if constexpr (FOLD) {
      const __amdgpu_buffer_rsrc_t ro = slice_rsrc(p.o + b * p.o_sb + hh * p.o_sh, p.o_sl, p.Lq, p.hd);
      float acc = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int e = ks * 32 + 8 * g;
        const unsigned off3 = e >= p.hd ? 0xfffffff0u : (unsigned)(((long)out_row<FM>(p, qrow) * p.o_sl + e) * 2);
        const bf16x8 of = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ro, off3, 0, 0));
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __builtin_fmaf((float)of[j], (float)dof[cb][ks][j], acc);
      }
      acc += __shfl_xor(acc, 16);  // the four lanes l, l + 16, l + 32, l + 48 hold the column chunks of one query
      acc += __shfl_xor(acc, 32);
      ndl = -acc;
      lse2 = p.lse[srow] * LOG2E;
      if (g == 0 && qrow < p.Lq) {
        p.delta[srow] = ndl;
        p.delta[nrows + srow] = lse2;
        if (p.kv_pad_ones == 1) annotate_q(p, b, hh, qrow, lse2);
      }
    } else {
      ndl = p.delta[srow];           // -delta of this lane's query
      lse2 = p.delta[nrows + srow];  // lse * log2(e)
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) { qf[cb][ks] = scale_frag(qf[cb][ks], c); retire(dof[cb][ks]); }
    if (g == 1) {  // ks = 2, g = 1: columns 72 .. 79 (K holds 1.0 at 72, 73; V at 72, 76)
      __bf16 hi, lo;
      split_bf16(-lse2, hi, lo);
      qf[cb][KS - 1][0] = hi;
      qf[cb][KS - 1][1] = lo;
      split_bf16(ndl, hi, lo);
      dof[cb][KS - 1][0] = hi;
      dof[cb][KS - 1][4] = lo;
    }
  }

  f32x4 dq[NDB][NQ];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int cb = 0; cb < NQ; ++cb) dq[db][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const FcMap fm(p);
  int fcq[NQ] = {0, 0};
  if constexpr (CAUSAL) {
#pragma unroll
    for (int cb = 0; cb < NQ; ++cb) fcq[cb] = fm.fq(qrow0 + 16 * cb);
  }
  [[maybe_unused]] int klim[NQ] = {0, 0}, wklim = 0;  // FM: as in attn_fwd16_kernel
  if constexpr (FM) {
    const int wq0 = qt * (64 * NQ) + wave * (16 * NQ);
#pragma unroll
    for (int cb = 0; cb < NQ; ++cb) klim[cb] = fm_kend(p, qrow0 + 16 * cb);
    wklim = wq0 >= p.fc_lead ? __builtin_amdgcn_readfirstlane(fm_kend(p, wq0)) : 0;
  }
  [[maybe_unused]] int kbeg[NQ] = {0, 0};  // WIN: as in attn_fwd16_kernel
  [[maybe_unused]] const FmWinOpen<WIN> wo(p, qt * (64 * NQ) + wave * (16 * NQ), 16 * NQ);
  if constexpr (WIN) {
#pragma unroll
    for (int cb = 0; cb < NQ; ++cb) kbeg[cb] = fm_kbeg(p, qrow0 + 16 * cb);
  }
  VDS_WAIT_VM(0);
  __syncthreads();  // tile 0 landed

  // NCB: 16-query blocks of this wave that hold queries (see attn_fwd16_kernel)
  auto kv_tile = [&](int it, auto PAR, auto NCBT) {
    constexpr int par = decltype(PAR)::value;
    constexpr int NCB = decltype(NCBT)::value;
    int j = it, jn = it + 1;  // this visit's key tile and the next one's (WIN: across the gap)
    if constexpr (WIN) { j = wt.tile(it); jn = wt.tile(it + 1); }
    if (it + 1 < nit) {
      char* nk = smem + (par ^ 1) * 2 * TILE;
      dk.issue(rk, nk, (unsigned)jn * k_step, wave);
      dv.issue(rv, nk + TILE, (unsigned)jn * v_step, wave);
    }
    const char* kt = smem + par * 2 * TILE;
    const char* vt = kt + TILE;
    // keys past Lk need no mask: their K rows are zero-filled, so whatever dS they get multiplies a zero row of K
    if constexpr (NCB > 0)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x4 s[2][NQ], dp[2][NQ];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) { s[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          const bf16x8 ak = frag16_row<HDP>(kt, kb * 32 + rb * 16, ks, lane);
          const bf16x8 av = frag16_row<HDP>(vt, kb * 32 + rb * 16, ks, lane);
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) {
            s[rb][cb] = mfma16(ak, qf[cb][ks], s[rb][cb]);
            dp[rb][cb] = mfma16(av, dof[cb][ks], dp[rb][cb]);
          }
        }
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[rb][cb][r] = __builtin_amdgcn_exp2f(s[rb][cb][r]);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[rb][cb][r] *= dp[rb][cb][r];  // dS^T (unscaled)
      if constexpr (CAUSAL) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int xk = fm.x(j * 64 + kb * 32 + rb * 16 + 4 * g + r);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
              if (xk > fcq[cb]) s[rb][cb][r] = 0.f;
          }
      }
      if constexpr (WIN) {
        if (!wo.open(j * 64 + kb * 32)) {
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = j * 64 + kb * 32 + rb * 16 + 4 * g + r;
#pragma unroll
              for (int cb = 0; cb < NCB; ++cb)
                if (fm_win_masked(key, p.fc_lead, kbeg[cb], klim[cb])) s[rb][cb][r] = 0.f;
            }
        }
      } else if constexpr (FM) {
        if (j * 64 + kb * 32 + 32 > wklim) {
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = j * 64 + kb * 32 + rb * 16 + 4 * g + r;
#pragma unroll
              for (int cb = 0; cb < NCB; ++cb)
                if (key >= klim[cb]) s[rb][cb][r] = 0.f;
            }
        }
      }
      bf16x8 df[NQ];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) df[cb] = pack2(s[0][cb], s[1][cb]);
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const bf16x8 akt = frag16_tr<HDP>(kt, kb * 32, db * 16, lane);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) dq[db][cb] = mfma16(akt, df[cb], dq[db][cb]);
      }
    }
    VDS_WAIT_VM(0);
    __syncthreads();
  };
  auto run = [&](auto NCBT) {
    for (int it = 0; it < nit; it += 2) {
      kv_tile(it, std::integral_constant<int, 0>{}, NCBT);
      if (it + 1 < nit) kv_tile(it + 1, std::integral_constant<int, 1>{}, NCBT);
    }
  };
  const int ncb = min(NQ, max(0, (p.Lq - (qt * (64 * NQ) + wave * (16 * NQ)) + 15) >> 4));  // wave-uniform
  if (ncb == NQ) run(std::integral_constant<int, NQ>{});
  else if (ncb == 2) run(std::integral_constant<int, 2>{});
  else if (ncb == 1) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 0>{});
#pragma unroll
  for (int cb = 0; cb < NQ; ++cb) {
    const int qrow = qrow0 + 16 * cb;
    float vq[NDB][4];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) vq[db][e] = dq[db][cb][e];
    store_block_bf16_t(vq, p.scale, p.dq + b * p.dq_sb + hh * p.dq_sh + (long)qrow * p.dq_sl, p.hd, g, qrow < p.Lq, p.wide_dq);
  }
}

bool rows16(const void* base, long sb, long sh, long sl) {
  return base && ((uintptr_t)base % 16 == 0) && (sb % 8 == 0) && (sh % 8 == 0) && (sl % 8 == 0);
}

AttnP to_p(const vds_attn_args* a) {
  AttnP p;
  p.B = a->B; p.H = a->H; p.Lq = a->Lq; p.Lk = a->Lk; p.hd = a->head_dim;
  p.q = (const bf16_t*)a->q; p.q_sb = a->q_sb; p.q_sh = a->q_sh; p.q_sl = a->q_sl;
  p.k = (const bf16_t*)a->k; p.k_sb = a->k_sb; p.k_sh = a->k_sh; p.k_sl = a->k_sl;
  p.v = (const bf16_t*)a->v; p.v_sb = a->v_sb; p.v_sh = a->v_sh; p.v_sl = a->v_sl;
  p.o = (bf16_t*)a->o; p.o_sb = a->o_sb; p.o_sh = a->o_sh; p.o_sl = a->o_sl;
  p.lse = a->lse;
  p.d_o = (const bf16_t*)a->d_o; p.do_sb = a->do_sb; p.do_sh = a->do_sh; p.do_sl = a->do_sl;
  p.dq = (bf16_t*)a->dq; p.dq_sb = a->dq_sb; p.dq_sh = a->dq_sh; p.dq_sl = a->dq_sl;
  p.dk = (bf16_t*)a->dk; p.dk_sb = a->dk_sb; p.dk_sh = a->dk_sh; p.dk_sl = a->dk_sl;
  p.dv = (bf16_t*)a->dv; p.dv_sb = a->dv_sb; p.dv_sh = a->dv_sh; p.dv_sl = a->dv_sl;
  p.delta = a->delta;
  p.scale = 1.0f / sqrtf((float)a->head_dim);
  p.n_rt = 0;
  p.tail_last = 0;
  p.kv_pad_ones = a->kv_pad_ones;
  p.q_split = 1;
  p.dkv_part = nullptr;
  p.kv_lens = nullptr;
  p.fc_lead = 0;
  p.fc_period = 1;
  p.fc_past = 0;
  p.fm_S = 1;
  p.fm_G = 1;
  p.fm_rev = 0;
  const bool wide_on = vdscfg::geti(vdscfg::ATTN_WIDE_STORES) != 0;  // A/B knob
  p.wide_o = wide_on && p.hd > 64 && rows16(p.o, p.o_sb, p.o_sh, p.o_sl);
  p.wide_dq = wide_on && p.hd > 64 && rows16(p.dq, p.dq_sb, p.dq_sh, p.dq_sl);
  p.wide_dkv = wide_on && p.hd > 64 && rows16(p.dk, p.dk_sb, p.dk_sh, p.dk_sl) && rows16(p.dv, p.dv_sb, p.dv_sh, p.dv_sl);
  return p;
}

// The kernels are templates on the PADDED head dim (HDP: the Q K^T / dO V^T contraction, HDQ: the width of O / dQ / dK / dV);
// rows are fetched with every 16-byte chunk at or past head_dim redirected out of range (zeros) and only head_dim columns
// are stored, so any head_dim that is a multiple of 8 runs on the next instance (model.py:57 of the reference takes any
// hidden_size // num_heads): <= 32, <= 64, <= 80 (HDP 96, HDQ 80: DiT-XL's 72), <= 96, <= 128.  0 = no instance.
int kernel_instance(int hd) {
  if (hd <= 0 || (hd & 7) || hd > 128) return 0;
  return hd <= 32 ? 32 : hd <= 64 ? 64 : hd <= 80 ? 80 : hd <= 96 ? 96 : 128;
}

bool strides_ok(const vds_attn_args* a, bool bwd) {
  auto ok = [](int64_t s) { return (s & 7) == 0; };
  bool r = ok(a->q_sb) && ok(a->q_sh) && ok(a->q_sl) && ok(a->k_sb) && ok(a->k_sh) && ok(a->k_sl) &&
           ok(a->v_sb) && ok(a->v_sh) && ok(a->v_sl) && (a->o_sb % 4 == 0) && (a->o_sh % 4 == 0) && (a->o_sl % 4 == 0);
  if (bwd)
    r = r && ok(a->do_sb) && ok(a->do_sh) && ok(a->do_sl) && (a->dq_sl % 4 == 0) && (a->dk_sl % 4 == 0) &&
        (a->dv_sl % 4 == 0) && (a->dq_sh % 4 == 0) && (a->dk_sh % 4 == 0) && (a->dv_sh % 4 == 0) &&
        (a->dq_sb % 4 == 0) && (a->dk_sb % 4 == 0) && (a->dv_sb % 4 == 0);
  return r;
}

// which head-dim-72 kernels run on v_mfma_f32_16x16x32_bf16 instead of 32x32x16 (bit 0: dK/dV, bit 1: dQ,
// bit 2: forward).  Knob attn_mfma16 (VDS_ATTN_MFMA16 at load, vds_attn_set_variant afterwards: tests, A/B); default 7 =
// all three: measured +4 % (dK/dV), +3.4 % (forward), +1.4 % (dQ) on random data, same box
constexpr int ATTN_VARIANT_DEFAULT = 7;
int attn_variant() { return vdscfg::geti(vdscfg::ATTN_MFMA16) & 7; }

// ---- which mask ---------------------------------------------------------------------------------------------------------
// A call travels: entry point (its forwarding rule) -> attn_call: validate -> to_p, apply_mask -> with_head_dim -> a runner
// -> launch.  A mask is one enumerator, the bool template flags of the kernel instances that implement it (flags_of), the
// values it carries (MaskV), its refusals (validate) and the AttnP fields it sets (apply_mask).
//   KVLEN  (vds_attn_*_kvlen): the instances that read p.kv_lens.  The choices and the launch geometry are functions of Lk,
//          never of the device-side lengths.
//   CAUSAL (vds_attn_*_causal): the instances that read p.fc_lead / p.fc_period, same choices and geometry.
//   PAST   (vds_attn_fwd_causal_past): the CAUSAL forward instances that also read p.fc_past.
//   FM     (vds_attn_*_causal_fm, _fm_chunk): the frame-major instances; a chunk is the granularity p.fm_G, no kernel of its own.
//   FM_WIN (vds_attn_*_causal_fm_window): the WIN instances of the FM kernels (p.fc_past = W chunks).
//   FM_TF  (vds_teacher_attn_*): the TF instances of the plain FM kernels (the period is 2n: clean frames, noisy copies).
//   FM_BAND (vds_band_attn_*): the BAND instances of the plain FM kernels (p.fc_past = b chunks on each side; not causal).
enum class Mask { NONE, KVLEN, CAUSAL, PAST, FM, FM_WIN, FM_TF, FM_BAND };
struct MaskFlags {
  bool kvlen, causal, past, fm, win, tf, band;
};
constexpr MaskFlags flags_of(Mask m) {
  return {m == Mask::KVLEN, m == Mask::CAUSAL || m == Mask::PAST, m == Mask::PAST,
          m == Mask::FM || m == Mask::FM_WIN || m == Mask::FM_TF || m == Mask::FM_BAND, m == Mask::FM_WIN, m == Mask::FM_TF,
          m == Mask::FM_BAND};
}
template <Mask M>
constexpr MaskFlags FLAGS = flags_of(M);

struct MaskV {
  const int32_t* kv_lens = nullptr;        // KVLEN: B int32 on the device
  const vds_mod_groups* frames = nullptr;  // CAUSAL, PAST, FM, FM_WIN, FM_TF, FM_BAND
  int past = 0;                            // PAST: cached key rows behind the lead rows
  int chunk = 1;                           // FM, FM_WIN, FM_TF, FM_BAND: token-frames per chunk
  int window_chunks = 0;                   // FM_WIN
  int band_chunks = 0;                     // FM_BAND: chunks on each side of a token's own
};

// The refusals of one call, in this order: NULL pointers and non-positive lengths, strides, the mask's own conditions
// (VDS_ERR_ARG before VDS_ERR_UNSUPPORTED), the head dim.  Nothing is launched before it returns VDS_OK.
int validate(const vds_attn_args* a, Mask kind, const MaskV& m, bool bwd) {
  if (!a || !a->q || !a->k || !a->v || !a->o || !a->lse || a->Lq <= 0 || a->Lk <= 0 ||
      (bwd && (!a->d_o || !a->dq || !a->dk || !a->dv || !a->delta)))
    return VDS_ERR_ARG;
  if (!strides_ok(a, bwd)) return VDS_ERR_ARG;
  const MaskFlags f = flags_of(kind);
  if (f.kvlen && a->kv_pad_ones == 1) return VDS_ERR_ARG;  // self-attention on annotated q rows: no lengths
  if (f.causal || f.fm) {
    // self-attention only: the keys are the queries' own rows, behind m.past cached ones (see fc_past_row for that mask)
    const vds_mod_groups* fr = m.frames;
    if (!fr || (int64_t)a->Lk != (int64_t)a->Lq + m.past || a->kv_pad_ones == 2) return VDS_ERR_ARG;
    if (fr->lead < 0 || fr->period < 1 || a->Lq < fr->lead || (a->Lq - fr->lead) % fr->period != 0) return VDS_ERR_ARG;
    if (f.tf && (fr->period & 1)) return VDS_ERR_ARG;  // clean frames and their noisy copies: an even period
    if (f.band && (m.chunk < 1 || m.band_chunks < 0)) return VDS_ERR_ARG;
    if (a->Lk > (1 << 21)) return VDS_ERR_UNSUPPORTED;  // FcMap / FmMap: the fp32 quotient is exact below 2^21 rows
  }
  if (f.fm) {
    // the token rows of o / d_o are reached through 32-bit byte offsets (tok(r) * row stride * 2): a (b, h) slice of them
    // has to stay below 4 GiB
    const int64_t lim = (int64_t)1 << 32;
    if ((int64_t)a->Lq * a->o_sl * 2 >= lim || (bwd && (int64_t)a->Lq * a->do_sl * 2 >= lim)) return VDS_ERR_UNSUPPORTED;
  }
  return kernel_instance(a->head_dim) ? VDS_OK : VDS_ERR_UNSUPPORTED;
}

// the mask's values into the kernel arguments (to_p leaves the fields of "no mask")
void apply_mask(AttnP& p, Mask kind, const MaskV& m) {
  const MaskFlags f = flags_of(kind);
  if (f.kvlen) p.kv_lens = m.kv_lens;
  if (f.causal || f.fm) {
    p.fc_lead = m.frames->lead;
    p.fc_period = m.frames->period;
  }
  if (f.past) p.fc_past = m.past;
  if (f.fm) {
    const int S = (p.Lq - p.fc_lead) / p.fc_period;
    p.fm_S = S > 0 ? S : 1;  // (no token rows: every row is a lead row and the quotient is never taken)
    // chunk >= period is one token group: G = period * S = L - lead < 2^21, whatever the chunk
    p.fm_G = (m.chunk < p.fc_period ? m.chunk : p.fc_period) * p.fm_S;
    // teacher forcing: chunks of the n = period / 2 frames of a half (chunk >= n: one chunk per half)
    if (f.tf) p.fm_G = (m.chunk < p.fc_period / 2 ? m.chunk : p.fc_period / 2) * p.fm_S;
    p.fm_rev = vdscfg::geti(vdscfg::ATTN_FM_HEAVY_FIRST) ? 1 : 0;
  }
  if (f.win) p.fc_past = m.window_chunks;  // (< the chunk count <= period: W * G stays below L)
  if (f.band) {
    // b at most the chunk count (every larger band attends the same pairs): b * G <= L - lead + G stays below 2^22
    const int nch = (p.fc_period + m.chunk - 1) / m.chunk;
    p.fc_past = m.band_chunks < nch ? m.band_chunks : nch;
    p.fm_rev = 0;  // the first workgroup of a head is its heaviest (the lead rows sweep everything): plain tile order
  }
}

// The one place that maps a head dim to its instance <HDP, HDQ>: f(HDP, HDQ) with both as std::integral_constant.
template <typename F>
int with_head_dim(int hd, F&& f) {
  using std::integral_constant;
  switch (kernel_instance(hd)) {
    // (32: the reference's own smoke test, width 512 / 16 heads, model.py:545-565)
    case 32: return f(integral_constant<int, 32>{}, integral_constant<int, 32>{});
    case 64: return f(integral_constant<int, 64>{}, integral_constant<int, 64>{});
    case 80: return f(integral_constant<int, 96>{}, integral_constant<int, 80>{});
    case 96: return f(integral_constant<int, 96>{}, integral_constant<int, 96>{});
    case 128: return f(integral_constant<int, 128>{}, integral_constant<int, 128>{});
    default: return VDS_ERR_UNSUPPORTED;
  }
}

// ---- launching ----------------------------------------------------------------------------------------------------------
// One launch of 256-thread workgroups that take exactly LDS bytes of dynamic LDS: vds_launch (common.h) raises the kernel's
// limit to that before its first launch.  The tiles of head dim 128 take 64 KiB and more, past the default limit.
template <auto KERNEL, int LDS>
void launch(unsigned grid, hipStream_t s, const AttnP& p) {
  vds_launch<KERNEL, LDS>(dim3(grid), dim3(256), LDS, s, p);
}

// what every runner returns after its last launch
int launched() { return hipGetLastError() == hipSuccess ? VDS_OK : VDS_ERR_LAUNCH; }

// The geometry of a kernel whose workgroups hold `tile` of the L rows of its stationary operand: p.n_rt and p.tail_last,
// and the grid -- the (b, h) pairs rounded up to a multiple of 8, times the row tiles.
// (knob attn_tail_last = 0 keeps the head-major order for ragged lengths too (A/B))
unsigned tile_grid(AttnP& p, int L, int tile) {
  p.n_rt = cdiv(L, tile);
  p.tail_last = (vdscfg::geti(vdscfg::ATTN_TAIL_LAST) && L > tile && (L % tile) != 0) ? 1 : 0;
  return (unsigned)(cdiv(p.B * p.H, 8) * 8 * p.n_rt);
}

// the preprocess of the backward (delta = rowsum(dO * O), lse * log2 e): one read of token-major o / d_o rows where the
// layout allows it.  FM: o / d_o rows by tok(r).
template <bool FM>
void launch_delta(const AttnP& p, hipStream_t s) {
  const long rows = (long)p.B * p.H * p.Lq;
  vdsprof::Scope ps(VDS_PROF_ATTN_BWD_DELTA, s, 2.0 * rows * p.hd, 2.0 * (2.0 * p.B * p.H * p.hd * (double)p.Lq));
  const bool tokmajor = p.o_sh == p.hd && p.do_sh == p.hd && p.o_sl == (long)p.H * p.hd && p.do_sl == p.o_sl &&
                        (p.o_sl & 7) == 0 && (p.o_sb & 7) == 0 && (p.do_sb & 7) == 0 && p.H * p.hd <= 1536 && p.H <= 64;
  if (tokmajor) launch<attn_delta_tokmajor_kernel<FM>, 0>((unsigned)(((long)p.B * p.Lq + 3) / 4), s, p);
  else launch<attn_delta_kernel<FM>, 0>((unsigned)((rows + 3) / 4), s, p);
}

// ---- the runners of the interleaved masks (NONE, KVLEN, CAUSAL, PAST) ---------------------------------------------------
// (KVLEN: the host does not know the lengths -- the profiler credits the work of all Lk keys, here and in run_bwd, so its
// FLOP/s and byte rates of a masked call are overstated by Lk / mean length.  CAUSAL: the profiler credits the unmasked
// FLOPs: in the (h w t) row order no tile is skipped, so that is the work executed.  PAST: those of all Lq x Lk pairs.)
template <int HDP, int HDQ, Mask M>
int run_fwd(AttnP p, hipStream_t s) {
  constexpr bool KVLEN = FLAGS<M>.kvlen, CAUSAL = FLAGS<M>.causal, PAST = FLAGS<M>.past;
  constexpr int LDS = 4 * 64 * HDP * 2;
  const int wide = vdscfg::geti(vdscfg::ATTN_FWD_WIDE);  // 0 / 1 forces (experiments); 2 (default): head_dim 64 / 72, long query sequences
  bool use_wide = false;
  if constexpr (HDP == 96 || HDP == 64) use_wide = wide == 1 || (wide == 2 && p.Lq >= 2048);  // (+2.7 % at head_dim 64)
  const unsigned grid = tile_grid(p, p.Lq, use_wide ? 256 : 128);
  const double fl = 4.0 * p.B * p.H * (double)p.Lq * p.Lk * p.hd;
  const bool ones_fwd = HDP == 96 && HDQ == 80 && use_wide && p.kv_pad_ones && p.hd == 72;
  // (kv_pad_ones == 2: cross-attention on the ones-column kernels -- keeps its own profiler class)
  vdsprof::Scope ps(ones_fwd && p.kv_pad_ones == 1 ? VDS_PROF_ATTN_FWD : VDS_PROF_ATTN_FWD_PLAIN, s, fl,
                    2.0 * p.B * p.H * p.hd * (2.0 * p.Lq + 2.0 * p.Lk));
  if constexpr (HDP == 96 && HDQ == 80) {
    if (ones_fwd) {
      // (round 5 measured a form of this kernel software-pipelined inside the wave: +9.5 % slower, removed in round 6;
      // profiles/r05/attn_fwd_software_pipelined.log)
      if (attn_variant() & 4) launch<attn_fwd16_kernel<HDP, KVLEN, CAUSAL, PAST>, LDS>(grid, s, p);
      else launch<attn_fwd_wide_kernel<HDP, HDQ, true, KVLEN, CAUSAL, PAST>, LDS>(grid, s, p);
      return launched();
    }
  }
  if constexpr (HDP == 96 || HDP == 64) {
    if (use_wide) {
      launch<attn_fwd_wide_kernel<HDP, HDQ, false, KVLEN, CAUSAL, PAST>, LDS>(grid, s, p);
      return launched();
    }
  }
  launch<attn_fwd_kernel<HDP, HDQ, 2, true, KVLEN, CAUSAL, PAST>, LDS>(grid, s, p);
  return launched();
}

// query-range split of the plain dK/dV kernel: target ~3 rounds of the 512 co-resident workgroups, each range at
// least 8 query tiles of 64 (the prologue -- K / V fragments, first tile -- is ~2 tile times)
int dkv_qsplit(int B, int H, int Lq, int Lk) {
  const long wgs = (long)cdiv(B * H, 8) * 8 * cdiv(Lk, 128);
  const int nqt = cdiv(Lq, 64);
  if (wgs >= 3 * 512 || nqt < 16) return 1;
  long sp = (3 * 512 + wgs - 1) / wgs;
  if (sp > nqt / 8) sp = nqt / 8;
  return (int)(sp < 1 ? 1 : sp > 16 ? 16 : sp);
}

template <int HDP, int HDQ, Mask M>
int run_bwd(AttnP p, hipStream_t s, size_t ws_floats) {
  constexpr bool KVLEN = FLAGS<M>.kvlen, CAUSAL = FLAGS<M>.causal;
  constexpr bool HD72 = HDP == 96 && HDQ == 80;  // the instance of the ones-column kernels
  constexpr int LDS_DQ = 4 * 64 * HDP * 2;
  constexpr int LDS_DKV = 4 * 64 * HDP * 2 + 2 * 128 * 4;
  const long rows = (long)p.B * p.H * p.Lq;
  // ALGORITHMIC backward = 2 x forward = 4 products of 2*Lq*Lk*hd (train step = 3 x forward FLOPs, no
  // credit for the recomputed S, nor for the dP the split backward computes twice): dK/dV kernel 2 (dV, dK), dQ
  // kernel 2 (dP, dQ).  The kernels EXECUTE 4 + 3 = 7 products (and head-dim padding on top).
  const double prod = 2.0 * p.B * p.H * (double)p.Lq * p.Lk * p.hd;
  const double qb = 2.0 * p.B * p.H * p.hd * (double)p.Lq, kb = 2.0 * p.B * p.H * p.hd * (double)p.Lk;
  // the 16x16x32 dQ kernel of the ones-column path computes the statistics itself and runs first (attn_bwd_dq16_kernel, FOLD)
  bool fold = false;
  if constexpr (HD72) fold = p.kv_pad_ones && p.hd == 72 && (attn_variant() & 2) && vdscfg::geti(vdscfg::ATTN_DELTA_FOLD);
  auto launch_dq = [&]() {
    const unsigned grid = tile_grid(p, p.Lq, 128);
    bool ones = false;
    if constexpr (HD72) ones = p.kv_pad_ones && p.hd == 72;
    vdsprof::Scope ps(ones && p.kv_pad_ones == 1 ? VDS_PROF_ATTN_BWD_DQ : VDS_PROF_ATTN_BWD_DQ_PLAIN, s, 2.0 * prod,
                      (fold ? 4.0 : 3.0) * qb + 2.0 * kb);
    if constexpr (HD72) {
      // (48 queries per wave -- every fragment read feeds 3 MFMAs, two waves per SIMD instead of three -- measured 2-6 %
      // slower in round 5, removed in round 6; profiles/r05/attn_dq_three_blocks_per_wave.log)
      if (fold) launch<attn_bwd_dq16_kernel<HDP, true, KVLEN, CAUSAL>, LDS_DQ>(grid, s, p);
      else if (ones && (attn_variant() & 2)) launch<attn_bwd_dq16_kernel<HDP, false, KVLEN, CAUSAL>, LDS_DQ>(grid, s, p);
      else if (ones) launch<attn_bwd_dq_kernel<HDP, HDQ, true, KVLEN, CAUSAL>, LDS_DQ>(grid, s, p);
    }
    if (!ones) launch<attn_bwd_dq_kernel<HDP, HDQ, false, KVLEN, CAUSAL>, LDS_DQ>(grid, s, p);
  };
  if (fold) launch_dq();
  else launch_delta<false>(p, s);
  // (a 64-keys-per-wave, one-wave-per-SIMD variant of this kernel -- half the LDS reads per MFMA -- was
  // measured at 0.55-0.8x: hipcc's single-wave schedule does not overlap the VALU softmax with the MFMAs)
  const unsigned grid = tile_grid(p, p.Lk, 128);
  {
    bool ones_kv = false;
    // (kv_pad_ones == 2: the q rows carry no annotated pad -- token-major cross-attention queries -- so the dK/dV pass takes
    // the plain kernel, which stages -lse2 itself and masks the K / V pad columns)
    if constexpr (HD72) ones_kv = p.kv_pad_ones == 1 && p.hd == 72;
    vdsprof::Scope ps(ones_kv ? VDS_PROF_ATTN_BWD_DKV : VDS_PROF_ATTN_BWD_DKV_PLAIN, s, 2.0 * prod, 2.0 * qb + 4.0 * kb);
    if constexpr (HD72) {
      // (round 6 measured this kernel as an explicit MFMA / VALU ping-pong -- one 512-thread workgroup per CU, the two wave
      // groups in alternating MFMA and VALU / LDS segments under s_barrier: bit-identical, +5 % slower; the kernel executes 77 %
      // of what a bare MFMA loop reaches at the board's power limit.  profiles/r06/negative_attn_dkv_pingpong.log)
      if (ones_kv && (attn_variant() & 1)) launch<attn_bwd_dkv16_kernel<HDP, true, false, CAUSAL>, LDS_DKV>(grid, s, p);
      else if (ones_kv) launch<attn_bwd_dkv_kernel<HDP, HDQ, true, false, CAUSAL>, LDS_DKV>(grid, s, p);
    }
    bool done16 = false;
    if constexpr (HD72 && !CAUSAL) {
      // cross-attention with padded K / V (kv_pad_ones = 2) and enough workgroups to fill the chip once (B*H*n_rt >= 512;
      // the query-range split below exists in the plain kernel only): the 16x16x32 kernel with S started from -lse2
      const int x16 = vdscfg::geti(vdscfg::CROSS_DKV16);  // 0 = plain kernel, 1 = rule, 2 = also for small grids (tests)
      if (!ones_kv && p.kv_pad_ones == 2 && p.hd == 72 && x16 && (grid >= 512 || x16 == 2) && (attn_variant() & 1)) {
        launch<attn_bwd_dkv16_kernel<HDP, false, KVLEN>, LDS_DKV>(grid, s, p);
        done16 = true;
      }
    }
    if (!ones_kv && !done16) {
      // few key tiles per head (cross-attention): B*H*n_rt workgroups leave most of the 2 x 256 slots empty (B = 2: 128
      // of 512) or end on a half-filled round (B = 12: 768 = 1.5 rounds).  The query range is then split so that the
      // launch is ~3 rounds of proportionally shorter workgroups; the fp32 partials (q_split x B*H*Lk*2*hd floats, at
      // the end of the caller's workspace) are summed by dkv_reduce_kernel.  Needs the workspace vds_attn_bwd_workspace_
      // bytes asks for (args->ws_floats); knob attn_qsplit = 1 turns it off, = N forces N.
      const int force = vdscfg::geti(vdscfg::ATTN_QSPLIT);
      const int split = force > 0 ? force : dkv_qsplit(p.B, p.H, p.Lq, p.Lk);
      const size_t need = (size_t)2 * rows + (size_t)split * p.B * p.H * p.Lk * 2 * p.hd;
      if (split > 1 && (p.hd & 3) == 0 && ws_floats >= need && (p.dk_sl & 3) == 0) {
        p.q_split = split;
        p.dkv_part = p.delta + 2 * rows;
        p.tail_last = 0;
        launch<attn_bwd_dkv_kernel<HDP, HDQ, false, KVLEN, CAUSAL>, LDS_DKV>(grid * split, s, p);
        const long n = (long)p.B * p.H * p.Lk * 2 * (p.hd >> 2);
        launch<dkv_reduce_kernel<KVLEN>, 0>((unsigned)((n + 255) / 256), s, p);
        p.q_split = 1;
        p.dkv_part = nullptr;
      } else {
        launch<attn_bwd_dkv_kernel<HDP, HDQ, false, KVLEN, CAUSAL>, LDS_DKV>(grid, s, p);
      }
    }
  }
  if (!fold) launch_dq();
  return launched();
}

// ---- the runners of the frame-major masks (FM, FM_WIN; include/vds.h) ---------------------------------------------------
// FM instances exist of the plain 32x32x16 kernels (every head dim; kv_pad_ones 0, and 1 where a 16x16x32 kernel is
// switched off: the pad columns are not read) and, for the ones layout at head dim 72, of the 16x16x32 family --
// attn_fwd16_kernel, attn_bwd_dq16_kernel with and without FOLD, attn_bwd_dkv16_kernel -- under the same attn_mfma16 bits
// (vds_attn_set_variant), attn_delta_fold knob and attn_fwd_wide rule as their CAUSAL siblings.  There is no frame-major
// instance of the 64-queries-per-wave 32x32 forwards nor of the ones-column 32x32 kernels: where run_fwd / run_bwd would
// take one of those, these runners take the plain 32x32x16 FM kernel.  The query range of the dK/dV kernel is never split.
// The profiler credits the pairs of the key range actually visited, not the unmasked L x L.
// (G: rows per chunk, fm_G)
int fm_kend_host(int r, int lead, int G, int L) {
  if (r < lead) return lead;
  const int e = lead + ((r - lead) / G + 1) * G;
  return e < L ? e : L;
}
int fm_qstart_host(int j, int lead, int G) { return j < lead ? 0 : lead + ((j - lead) / G) * G; }
// window of W chunks (W = 0: none)
int fm_kbeg_host(int r, int lead, int G, int W) {
  if (r < lead) return lead;
  const int n = (r - lead) / G - W + 1;
  return lead + (n > 0 ? n : 0) * G;
}
int fm_qend_host(int j, int lead, int G, int L, int W) {
  if (j < lead) return L;
  const long e = lead + ((long)(j - lead) / G + W) * G;
  return e < L ? (int)e : L;
}
// (query, key) pairs the forward / dQ kernels visit: `tile` queries per workgroup, keys [0, kend of its last query); with
// a window, less the keys between the lead tiles and the tile that holds kbeg of its first token query
double fm_pairs_q(int L, int lead, int G, int tile, int W = 0) {
  double n = 0;
  for (int q0 = 0; q0 < L; q0 += tile) {
    const int q1 = q0 + tile < L ? q0 + tile : L;
    int keys = fm_kend_host(q1 - 1, lead, G, L);
    if (W > 0 && q1 > lead) {
      const int nl = ((lead + 63) >> 6) * 64, kb = fm_kbeg_host(q0 > lead ? q0 : lead, lead, G, W) & ~63;
      if (kb > nl) keys -= kb - nl;
    }
    n += (double)(q1 - q0) * keys;
  }
  return n;
}
// ... and the dK/dV kernel: `tile` keys per workgroup, queries from the 64-row tile that holds qstart of its first key; with
// a window, up to qend of its last key unless it holds a lead key
double fm_pairs_k(int L, int lead, int G, int tile, int W = 0) {
  double n = 0;
  for (int k0 = 0; k0 < L; k0 += tile) {
    const int k1 = k0 + tile < L ? k0 + tile : L;
    const int qe = (W > 0 && k0 >= lead) ? fm_qend_host(k1 - 1, lead, G, L, W) : L;
    n += (double)(k1 - k0) * (qe - (fm_qstart_host(k0, lead, G) & ~63));
  }
  return n;
}

// Teacher forcing (TfMap): the bounds on the host, for the pair counts of the two-range sweeps.  base = lead + n S.
struct TfHost {
  int L, lead, base, G;
  int cg(int r) const { return (r - (r >= base ? base : lead)) / G * G; }
  int clip(long e) const { return e < L ? (int)e : L; }
  int pend(int r) const { return r < lead ? lead : r < base ? (lead + cg(r) + G < base ? lead + cg(r) + G : base) : lead + cg(r); }
  int kbeg(int r) const { return r < base ? pend(r) : base + cg(r); }
  int kend(int r) const { return r < base ? pend(r) : clip((long)base + cg(r) + G); }
  int qstart(int j) const { return j < lead ? 0 : (j < base ? lead : base) + cg(j); }
  int qend(int j) const { return j < lead ? L : j < base ? base : clip((long)base + cg(j) + G); }
  int q2(int j) const { return (j >= lead && j < base) ? clip((long)base + cg(j) + G) : L; }
};
// pairs of the key tiles (64 rows, the last one up to the workgroup's key bound) a TF forward / dQ workgroup visits
double fm_pairs_q_tf(const TfHost& t, int tile) {
  double n = 0;
  for (int q0 = 0; q0 < t.L; q0 += tile) {
    const int q1 = q0 + tile < t.L ? q0 + tile : t.L;
    const int keys = t.kend(q1 - 1);
    const int nl = (t.pend(q0 < t.base ? (q1 < t.base ? q1 : t.base) - 1 : q1 - 1) + 63) >> 6;
    int skipped = 0;  // the tiles [nl, jb) between the two ranges
    if (q1 > t.base) {
      const int jb = t.kbeg(q0 > t.base ? q0 : t.base) >> 6;
      if (jb > nl) skipped = (jb - nl) * 64;
    }
    n += (double)(q1 - q0) * (keys - skipped);
  }
  return n;
}
// ... and of the query tiles a TF dK/dV workgroup visits (rows up to L)
double fm_pairs_k_tf(const TfHost& t, int tile) {
  double n = 0;
  const int nqt = (t.L + 63) >> 6;
  for (int k0 = 0; k0 < t.L; k0 += tile) {
    const int k1 = k0 + tile < t.L ? k0 + tile : t.L;
    int a0 = 0, a1 = nqt, b0 = nqt;
    if (k0 >= t.lead) {
      a0 = t.qstart(k0) >> 6;
      a1 = (t.qend(k1 - 1) + 63) >> 6;
      const int q2 = t.q2(k0);
      b0 = q2 >= t.L ? nqt : (a1 > (q2 >> 6) ? a1 : q2 >> 6);
    }
    auto rows = [&](int j0, int j1) { return (j1 * 64 < t.L ? j1 * 64 : t.L) - (j0 * 64 < t.L ? j0 * 64 : t.L); };
    n += (double)(k1 - k0) * (rows(a0, a1) + rows(b0, nqt));
  }
  return n;
}

// Frame band (BandMap): the bounds on the host, for the pair counts of the tiles the BAND kernels visit.  b: chunks a side.
struct BandHost {
  int L, lead, G, b;
  long cg(int r) const { return (long)((r - lead) / G) * G; }
  int lo(int r) const { const long o = cg(r) - (long)b * G; return lead + (int)(o > 0 ? o : 0); }
  int hi(int r) const { const long e = lead + cg(r) + ((long)b + 1) * G; return e < L ? (int)e : L; }
};
// pairs of the 64-row tiles a BAND workgroup of `tile` rows visits -- the same count for the key tiles of the forward / dQ
// kernels and the query tiles of the dK/dV kernel (the relation is symmetric and so are the two walks): every tile for the
// workgroup that holds a lead row, else the lead tiles and those from lo of its first row to below hi of its last
double fm_pairs_band(const BandHost& t, int tile) {
  double n = 0;
  auto rows = [&](int j0, int j1) { return (j1 * 64 < t.L ? j1 * 64 : t.L) - (j0 * 64 < t.L ? j0 * 64 : t.L); };
  for (int r0 = 0; r0 < t.L; r0 += tile) {
    const int r1 = r0 + tile < t.L ? r0 + tile : t.L;
    if (r0 < t.lead) {
      n += (double)(r1 - r0) * t.L;
      continue;
    }
    const int e = (t.hi(r1 - 1) + 63) >> 6;
    const int nl = (t.lead + 63) >> 6 < e ? (t.lead + 63) >> 6 : e;
    const int jb = nl > (t.lo(r0) >> 6) ? nl : t.lo(r0) >> 6;
    n += (double)(r1 - r0) * (rows(0, nl) + rows(jb, e));
  }
  return n;
}

template <int HDP, int HDQ, Mask M>
int run_fwd_fm(AttnP p, hipStream_t s) {
  constexpr bool WIN = FLAGS<M>.win;
  constexpr int LDS = 4 * 64 * HDP * 2;
  const int W = WIN ? p.fc_past : 0;
  if constexpr (FLAGS<M>.band) {  // the plain 32x32x16 BAND kernel, whatever the layout and the variant bits
    const unsigned grid = tile_grid(p, p.Lq, 128);
    const BandHost t{p.Lq, p.fc_lead, p.fm_G, p.fc_past};
    vdsprof::Scope ps(VDS_PROF_ATTN_FWD_PLAIN, s, 4.0 * p.B * p.H * p.hd * fm_pairs_band(t, 128),
                      2.0 * p.B * p.H * p.hd * (2.0 * p.Lq + 2.0 * p.Lk));
    launch<attn_fwd_kernel<HDP, HDQ, 2, true, false, false, false, true, false, false, true>, LDS>(grid, s, p);
    return launched();
  }
  if constexpr (FLAGS<M>.tf) {  // the plain 32x32x16 TF kernel, whatever the layout (no TF instance of the 16x16x32 family)
    const unsigned grid = tile_grid(p, p.Lq, 128);
    const TfHost t{p.Lq, p.fc_lead, p.fc_lead + (p.fc_period / 2) * p.fm_S, p.fm_G};
    vdsprof::Scope ps(VDS_PROF_ATTN_FWD_PLAIN, s, 4.0 * p.B * p.H * p.hd * fm_pairs_q_tf(t, 128),
                      2.0 * p.B * p.H * p.hd * (2.0 * p.Lq + 2.0 * p.Lk));
    launch<attn_fwd_kernel<HDP, HDQ, 2, true, false, false, false, true, false, true>, LDS>(grid, s, p);
    return launched();
  }
  // the ones layout on the 16x16x32 forward, where run_fwd takes it: 64 queries per wave by the attn_fwd_wide rule (0 / 1
  // forces, 2: from 2048 queries) and bit 2 of the variant mask
  bool fwd16 = false;
  if constexpr (HDP == 96 && HDQ == 80) {
    const int wide = vdscfg::geti(vdscfg::ATTN_FWD_WIDE);
    fwd16 = p.kv_pad_ones == 1 && p.hd == 72 && (attn_variant() & 4) && (wide == 1 || (wide == 2 && p.Lq >= 2048));
  }
  const int tile = fwd16 ? 256 : 128;
  const unsigned grid = tile_grid(p, p.Lq, tile);
  const double fl = 4.0 * p.B * p.H * p.hd * fm_pairs_q(p.Lq, p.fc_lead, p.fm_G, tile, W);
  vdsprof::Scope ps(fwd16 ? VDS_PROF_ATTN_FWD : VDS_PROF_ATTN_FWD_PLAIN, s, fl, 2.0 * p.B * p.H * p.hd * (2.0 * p.Lq + 2.0 * p.Lk));
  if constexpr (HDP == 96 && HDQ == 80) {
    if (fwd16) {
      launch<attn_fwd16_kernel<HDP, false, false, false, true, WIN>, LDS>(grid, s, p);
      return launched();
    }
  }
  launch<attn_fwd_kernel<HDP, HDQ, 2, true, false, false, false, true, WIN>, LDS>(grid, s, p);
  return launched();
}

template <int HDP, int HDQ, Mask M>
int run_bwd_fm(AttnP p, hipStream_t s) {
  constexpr bool WIN = FLAGS<M>.win;
  constexpr int LDS_DQ = 4 * 64 * HDP * 2;
  constexpr int LDS_DKV = 4 * 64 * HDP * 2 + 2 * 128 * 4;
  const int W = WIN ? p.fc_past : 0;
  const double per = 2.0 * p.B * p.H * p.hd;  // FLOPs of one product per (query, key) pair
  const double qb = 2.0 * p.B * p.H * p.hd * (double)p.Lq, kb = qb;
  if constexpr (FLAGS<M>.band) {  // the plain 32x32x16 BAND kernels: preprocess, dK/dV, dQ
    const BandHost t{p.Lq, p.fc_lead, p.fm_G, p.fc_past};
    const double pairs = fm_pairs_band(t, 128);
    launch_delta<true>(p, s);
    {
      const unsigned grid = tile_grid(p, p.Lk, 128);
      vdsprof::Scope ps(VDS_PROF_ATTN_BWD_DKV_PLAIN, s, 2.0 * per * pairs, 2.0 * qb + 4.0 * kb);
      launch<attn_bwd_dkv_kernel<HDP, HDQ, false, false, false, true, false, false, true>, LDS_DKV>(grid, s, p);
    }
    const unsigned grid = tile_grid(p, p.Lq, 128);
    vdsprof::Scope ps(VDS_PROF_ATTN_BWD_DQ_PLAIN, s, 2.0 * per * pairs, 3.0 * qb + 2.0 * kb);
    launch<attn_bwd_dq_kernel<HDP, HDQ, false, false, false, true, false, false, true>, LDS_DQ>(grid, s, p);
    return launched();
  }
  if constexpr (FLAGS<M>.tf) {  // the plain 32x32x16 TF kernels: preprocess, dK/dV, dQ
    const TfHost t{p.Lq, p.fc_lead, p.fc_lead + (p.fc_period / 2) * p.fm_S, p.fm_G};
    launch_delta<true>(p, s);
    {
      const unsigned grid = tile_grid(p, p.Lk, 128);
      vdsprof::Scope ps(VDS_PROF_ATTN_BWD_DKV_PLAIN, s, 2.0 * per * fm_pairs_k_tf(t, 128), 2.0 * qb + 4.0 * kb);
      launch<attn_bwd_dkv_kernel<HDP, HDQ, false, false, false, true, false, true>, LDS_DKV>(grid, s, p);
    }
    const unsigned grid = tile_grid(p, p.Lq, 128);
    vdsprof::Scope ps(VDS_PROF_ATTN_BWD_DQ_PLAIN, s, 2.0 * per * fm_pairs_q_tf(t, 128), 3.0 * qb + 2.0 * kb);
    launch<attn_bwd_dq_kernel<HDP, HDQ, false, false, false, true, false, true>, LDS_DQ>(grid, s, p);
    return launched();
  }
  // the ones layout at head dim 72: the 16x16x32 kernels under the variant bits of their CAUSAL siblings (bit 0 dK/dV, bit 1
  // dQ; with attn_delta_fold the dQ kernel is its own preprocess and runs first)
  bool ones = false;
  if constexpr (HDP == 96 && HDQ == 80) ones = p.kv_pad_ones == 1 && p.hd == 72;
  const bool dq16 = ones && (attn_variant() & 2), dkv16 = ones && (attn_variant() & 1);
  const bool fold = dq16 && vdscfg::geti(vdscfg::ATTN_DELTA_FOLD);
  auto launch_dq = [&]() {
    const unsigned grid = tile_grid(p, p.Lq, 128);
    vdsprof::Scope ps(ones ? VDS_PROF_ATTN_BWD_DQ : VDS_PROF_ATTN_BWD_DQ_PLAIN, s,
                      2.0 * per * fm_pairs_q(p.Lq, p.fc_lead, p.fm_G, 128, W), (fold ? 4.0 : 3.0) * qb + 2.0 * kb);
    if constexpr (HDP == 96 && HDQ == 80) {
      if (fold) launch<attn_bwd_dq16_kernel<HDP, true, false, false, true, WIN>, LDS_DQ>(grid, s, p);
      else if (dq16) launch<attn_bwd_dq16_kernel<HDP, false, false, false, true, WIN>, LDS_DQ>(grid, s, p);
    }
    if (!dq16) launch<attn_bwd_dq_kernel<HDP, HDQ, false, false, false, true, WIN>, LDS_DQ>(grid, s, p);
  };
  if (fold) launch_dq();
  else launch_delta<true>(p, s);
  {
    const unsigned grid = tile_grid(p, p.Lk, 128);
    vdsprof::Scope ps(ones ? VDS_PROF_ATTN_BWD_DKV : VDS_PROF_ATTN_BWD_DKV_PLAIN, s,
                      2.0 * per * fm_pairs_k(p.Lq, p.fc_lead, p.fm_G, 128, W), 2.0 * qb + 4.0 * kb);
    if constexpr (HDP == 96 && HDQ == 80) {
      if (dkv16) launch<attn_bwd_dkv16_kernel<HDP, true, false, false, true, WIN>, LDS_DKV>(grid, s, p);
    }
    if (!dkv16) launch<attn_bwd_dkv_kernel<HDP, HDQ, false, false, false, true, WIN>, LDS_DKV>(grid, s, p);
  }
  if (!fold) launch_dq();
  return launched();
}

// ---- the shared path of the 13 entry points -----------------------------------------------------------------------------
template <Mask M, bool BWD>
int attn_call(const vds_attn_args* a, const MaskV& m, vds_stream_t stream) {
  if (const int e = validate(a, M, m, BWD)) return e;
  AttnP p = to_p(a);
  apply_mask(p, M, m);
  hipStream_t s = (hipStream_t)stream;
  return with_head_dim(a->head_dim, [&](auto hdp, auto hdq) {
    constexpr int HDP = decltype(hdp)::value, HDQ = decltype(hdq)::value;
    if constexpr (BWD && FLAGS<M>.fm) {
      return run_bwd_fm<HDP, HDQ, M>(p, s);
    } else if constexpr (BWD) {
      // floats in `delta`: 2*B*H*Lq when the caller does not say (ws_floats = 0: the pre-round-4 contract, no query split)
      const size_t ws = a->ws_floats > 0 ? (size_t)a->ws_floats : (size_t)2 * a->B * a->H * a->Lq;
      return run_bwd<HDP, HDQ, M>(p, s, ws);
    } else if constexpr (FLAGS<M>.fm) {
      return run_fwd_fm<HDP, HDQ, M>(p, s);
    } else {
      return run_fwd<HDP, HDQ, M>(p, s);
    }
  });
}

}  // namespace

// K / V of a cross-attention (token-major [B*Lk, ld] rows, head h at columns col0 + h*hd) -> head-major padded rows
// [B,H,Lk,hdp] WITH the ones columns of the head_dim-72 kernels (K: 1.0 at hd, hd+1; V: 1.0 at hd, hd+4; zeros elsewhere
// in the pad), so that the forward and dQ passes of the cross-attention run on the ones-column 16x16x32 kernels
// (vds_attn_args.kv_pad_ones = 2).  One thread per 16-byte chunk of an output row.
__global__ __launch_bounds__(256) void kv_pad_ones_kernel(const bf16_t* kv, long ld, int kcol0, int vcol0, bf16_t* kp,
                                                          bf16_t* vp, int B, int Lk, int H, int hd, int hdp) {
  const int cpr = hdp >> 3;  // chunks per output row
  const long n = (long)B * H * Lk * cpr;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  const int which = blockIdx.y;  // 0 K, 1 V
  const int c = (int)(gid % cpr);
  const long row = gid / cpr;  // (b, h, l)
  const int l = (int)(row % Lk);
  const int h = (int)((row / Lk) % H);
  const int b = (int)(row / ((long)Lk * H));
  u32x4 w = {0u, 0u, 0u, 0u};
  if (c * 8 < hd) {
    w = *reinterpret_cast<const u32x4*>(kv + ((long)b * Lk + l) * ld + (which ? vcol0 : kcol0) + h * hd + c * 8);
  } else if (c * 8 == hd) {
    w[0] = which ? 0x00003f80u : 0x3f803f80u;  // K: 1.0 at hd, hd+1; V: 1.0 at hd ...
    w[2] = which ? 0x00003f80u : 0u;           // ... and hd+4
  }
  *reinterpret_cast<u32x4*>((which ? vp : kp) + row * hdp + c * 8) = w;
}

extern "C" int vds_kv_pad_ones(const void* kv, int64_t ld, int32_t k_col0, int32_t v_col0, void* kp, void* vp, int32_t B,
                               int32_t Lk, int32_t H, int32_t hd, int32_t hdp, vds_stream_t stream) {
  if (!kv || !kp || !vp || B <= 0 || Lk <= 0 || H <= 0 || hd <= 0) return VDS_ERR_ARG;
  if ((hd & 7) || (hdp & 7) || hdp < hd + 8 || (ld & 7) || (k_col0 & 7) || (v_col0 & 7)) return VDS_ERR_ARG;
  const long n = (long)B * H * Lk * (hdp >> 3);
  hipLaunchKernelGGL(kv_pad_ones_kernel, dim3((unsigned)((n + 255) / 256), 2), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)kv, (long)ld, k_col0, v_col0, (bf16_t*)kp, (bf16_t*)vp, B, Lk, H, hd, hdp);
  return launched();
}

extern "C" int vds_attn_set_variant(int32_t mask) {
  const int prev = attn_variant();
  if (mask < -1 || mask > 7) return VDS_ERR_ARG;
  vdscfg::g_val[vdscfg::ATTN_MFMA16] = mask < 0 ? ATTN_VARIANT_DEFAULT : mask;  // -1: back to the default
  return prev;
}

extern "C" size_t vds_attn_bwd_workspace_bytes(const vds_attn_args* a) {
  if (!a || a->B <= 0 || a->H <= 0 || a->Lq <= 0) return 0;
  size_t fl = (size_t)2 * a->B * a->H * a->Lq;
  if (a->Lk > 0 && a->head_dim > 0 && a->kv_pad_ones != 1)  // fp32 partials of the query-split dK/dV kernel (short key sequences)
    fl += (size_t)dkv_qsplit(a->B, a->H, a->Lq, a->Lk) * a->B * a->H * a->Lk * 2 * a->head_dim;
  return fl * sizeof(float);
}

// ---- the 13 entry points: each its forwarding rule (include/vds.h), then one call into the shared path --------------------
extern "C" int vds_attn_fwd(const vds_attn_args* a, vds_stream_t stream) {
  return attn_call<Mask::NONE, false>(a, {}, stream);
}

// (non-positive Lq / Lk are VDS_ERR_ARG here as in every other entry point: validate)
extern "C" int vds_attn_bwd(const vds_attn_args* a, vds_stream_t stream) {
  return attn_call<Mask::NONE, true>(a, {}, stream);
}

// per-sample key counts (kv_lens == NULL: the calls above, unchanged)
extern "C" int vds_attn_fwd_kvlen(const vds_attn_args* a, const int32_t* kv_lens, vds_stream_t stream) {
  if (!kv_lens) return vds_attn_fwd(a, stream);
  return attn_call<Mask::KVLEN, false>(a, {kv_lens}, stream);
}

extern "C" int vds_attn_bwd_kvlen(const vds_attn_args* a, const int32_t* kv_lens, vds_stream_t stream) {
  if (!kv_lens) return vds_attn_bwd(a, stream);
  return attn_call<Mask::KVLEN, true>(a, {kv_lens}, stream);
}

// frame-causal self-attention (frames == NULL: the plain calls, unchanged)
extern "C" int vds_attn_fwd_causal(const vds_attn_args* a, const vds_mod_groups* frames, vds_stream_t stream) {
  if (!frames) return vds_attn_fwd(a, stream);
  return attn_call<Mask::CAUSAL, false>(a, {nullptr, frames}, stream);
}

extern "C" int vds_attn_bwd_causal(const vds_attn_args* a, const vds_mod_groups* frames, vds_stream_t stream) {
  if (!frames) return vds_attn_bwd(a, stream);
  return attn_call<Mask::CAUSAL, true>(a, {nullptr, frames}, stream);
}

// frame-causal forward with a past (the cached rollout): the queries are the Lq rows of one call, the keys
// [lead rows | past cached rows | the call's own token rows]; see fc_past_row for the mask.  past == 0: the call above.
extern "C" int vds_attn_fwd_causal_past(const vds_attn_args* a, const vds_mod_groups* frames, int32_t past,
                                        vds_stream_t stream) {
  if (past < 0) return VDS_ERR_ARG;
  if (past == 0) return vds_attn_fwd_causal(a, frames, stream);
  return attn_call<Mask::PAST, false>(a, {nullptr, frames, past}, stream);
}

// frame-major self-attention (frames == NULL is refused: validate)
extern "C" int vds_attn_fwd_causal_fm(const vds_attn_args* a, const vds_mod_groups* frames, vds_stream_t stream) {
  return attn_call<Mask::FM, false>(a, {nullptr, frames}, stream);
}

extern "C" int vds_attn_bwd_causal_fm(const vds_attn_args* a, const vds_mod_groups* frames, vds_stream_t stream) {
  return attn_call<Mask::FM, true>(a, {nullptr, frames}, stream);
}

// chunk-causal: the FM instances with fm_G = chunk * S, no kernel of its own.  chunk == 1 IS the _fm entry point.
extern "C" int vds_attn_fwd_causal_fm_chunk(const vds_attn_args* a, const vds_mod_groups* frames, int32_t chunk,
                                            vds_stream_t stream) {
  if (chunk < 1) return VDS_ERR_ARG;
  if (chunk == 1) return vds_attn_fwd_causal_fm(a, frames, stream);
  return attn_call<Mask::FM, false>(a, {nullptr, frames, 0, chunk}, stream);
}

extern "C" int vds_attn_bwd_causal_fm_chunk(const vds_attn_args* a, const vds_mod_groups* frames, int32_t chunk,
                                            vds_stream_t stream) {
  if (chunk < 1) return VDS_ERR_ARG;
  if (chunk == 1) return vds_attn_bwd_causal_fm(a, frames, stream);
  return attn_call<Mask::FM, true>(a, {nullptr, frames, 0, chunk}, stream);
}

// sliding window: a token query of chunk n attends the lead keys and the token keys of chunks max(0, n - window_chunks + 1)
// .. n.  A window that covers every chunk -- ceil(period / chunk) of them -- IS the _fm_chunk entry point.
static bool window_covers(const vds_mod_groups* f, int32_t chunk, int32_t window_chunks) {
  return f->period < 1 || window_chunks >= (f->period + chunk - 1) / chunk;
}

extern "C" int vds_attn_fwd_causal_fm_window(const vds_attn_args* a, const vds_mod_groups* frames, int32_t chunk,
                                             int32_t window_chunks, vds_stream_t stream) {
  if (!frames || chunk < 1 || window_chunks < 1) return VDS_ERR_ARG;
  if (window_covers(frames, chunk, window_chunks)) return vds_attn_fwd_causal_fm_chunk(a, frames, chunk, stream);
  return attn_call<Mask::FM_WIN, false>(a, {nullptr, frames, 0, chunk, window_chunks}, stream);
}

extern "C" int vds_attn_bwd_causal_fm_window(const vds_attn_args* a, const vds_mod_groups* frames, int32_t chunk,
                                             int32_t window_chunks, vds_stream_t stream) {
  if (!frames || chunk < 1 || window_chunks < 1) return VDS_ERR_ARG;
  if (window_covers(frames, chunk, window_chunks)) return vds_attn_bwd_causal_fm_chunk(a, frames, chunk, stream);
  return attn_call<Mask::FM_WIN, true>(a, {nullptr, frames, 0, chunk, window_chunks}, stream);
}

// teacher forcing: the rows are [lead | clean frames | their noisy copies], frames->period = 2n token-frames; a noisy query
// attends the lead keys, the clean chunks before its own and its own noisy chunk (TfMap).  Self-attention on frame-major
// rows only; frames == NULL, an odd period and chunk < 1 are refused.
extern "C" int vds_teacher_attn_fwd(const vds_attn_args* a, const vds_mod_groups* frames, int32_t chunk,
                                    vds_stream_t stream) {
  if (!frames || chunk < 1) return VDS_ERR_ARG;
  return attn_call<Mask::FM_TF, false>(a, {nullptr, frames, 0, chunk}, stream);
}

extern "C" int vds_teacher_attn_bwd(const vds_attn_args* a, const vds_mod_groups* frames, int32_t chunk,
                                    vds_stream_t stream) {
  if (!frames || chunk < 1) return VDS_ERR_ARG;
  return attn_call<Mask::FM_TF, true>(a, {nullptr, frames, 0, chunk}, stream);
}

// frame band (not causal): a token row of chunk n attends the lead rows and the token rows of chunks n - band_chunks ..
// n + band_chunks, a lead row every row (BandMap).  Self-attention on frame-major rows only; the refusals are validate's.
// A band that covers every pair runs the same instances: there is no frame-major unmasked entry to forward to.
extern "C" int vds_band_attn_fwd(const vds_attn_args* a, const vds_mod_groups* frames, int32_t chunk, int32_t band_chunks,
                                 vds_stream_t stream) {
  return attn_call<Mask::FM_BAND, false>(a, {nullptr, frames, 0, chunk, 0, band_chunks}, stream);
}

extern "C" int vds_band_attn_bwd(const vds_attn_args* a, const vds_mod_groups* frames, int32_t chunk, int32_t band_chunks,
                                 vds_stream_t stream) {
  return attn_call<Mask::FM_BAND, true>(a, {nullptr, frames, 0, chunk, 0, band_chunks}, stream);
}
