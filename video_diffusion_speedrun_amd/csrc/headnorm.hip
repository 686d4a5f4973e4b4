// Head RMS-norm kernels for gfx950: the weightless RMSNorm of QK-norm on head rows that no qkv / RoPE kernel touches --
// the cross-attention's q rows (the q_cross output, token-major) and the k columns of the context_kv output.
//
//   vds_head_rmsnorm_fwd   x[m, h, :] <- bf16(float(x) * r),  r = rsqrt(mean_d(x^2) + eps),  rstd[m * H + h] = r
//   vds_head_rmsnorm_bwd   dy[m, h, :] <- bf16(r * (g - y * mean_d(g * y))),  g = float(dy), y = the forward's output
//
// Both work in place on a window [M, H * hd] of a parent with a row stride, in bf16 with fp32 math, and are bound by HBM:
// one read and one write of the rows (the backward reads the stored normed rows as well).
//
// Geometry.  The M * H head rows of the window are numbered m * H + h; a workgroup of 256 threads owns 64 consecutive
// ones.  A head row is hd / 8 sixteen-byte chunks (9 at head_dim 72: no power-of-two lane group), so the chunks of a
// workgroup's rows are dealt to its threads round robin -- chunk c of the tile to thread c % 256, trip c / 256 -- and
// every global access is one 16-byte segment of a row; all loads of a thread are issued before the first use.  The
// per-row sums meet in LDS:
//   forward   the chunks are written to LDS as dense head rows and ropestage::row_rstd -- the function the self-attention's
//             normed qkv / RoPE kernel uses: four lanes per row, a fixed two-step butterfly -- leaves r per row; every
//             thread then scales the chunks it still holds in registers and stores them.  hd * 128 + 256 bytes of LDS.
//   backward  every thread leaves the partial sum of g * y of each of its chunks in LDS (4 bytes per chunk); one thread
//             per row adds the hd / 8 partials in chunk order.  3.5 KiB of LDS at head_dim 72.
// No atomics and no order that depends on the launch: results are bit-identical run to run in either determinism mode.
#include "rope_stage.h"
#include "../../include/vds.h"

namespace {

inline int ok() { return hipGetLastError() == hipSuccess ? VDS_OK : VDS_ERR_LAUNCH; }

constexpr int HN_THREADS = 256;
constexpr int HN_ROWS = 64;  // head rows per workgroup (one 64-row trip of ropestage::row_rstd with 256 threads)

// where chunk c of a workgroup's tile lives: head row rl = c / HQ of the tile (head row h0 + rl counted from token row
// m0), chunk j = c % HQ of that row
template <int HD>
__device__ __forceinline__ long chunk_offset(int c, unsigned h0, int H, long ld, const ropestage::Div& by_h, int& rl) {
  constexpr int HQ = HD >> 3;
  rl = c / HQ;
  const int j = c - rl * HQ;
  unsigned h;
  const unsigned dm = by_h.div(h0 + (unsigned)rl, h);
  return (long)dm * ld + (long)h * HD + j * 8;
}

template <int HD>
__global__ __launch_bounds__(HN_THREADS) void head_rmsnorm_fwd_kernel(bf16_t* x, long ldx, float* __restrict__ rstd,
                                                                      long nrows, int H, float eps) {
  constexpr int HQ = HD >> 3, TRIPS = (HN_ROWS * HQ + HN_THREADS - 1) / HN_THREADS;
  __shared__ __attribute__((aligned(16))) char rows[HN_ROWS * HD * 2];
  __shared__ float rs[HN_ROWS];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * HN_ROWS;
  const int nr = (int)(nrows - r0 < HN_ROWS ? nrows - r0 : HN_ROWS);
  const long m0 = r0 / H;
  const unsigned h0 = (unsigned)(r0 - m0 * H);
  const ropestage::Div by_h((unsigned)H);
  bf16_t* base = x + m0 * ldx;
  u32x4 w[TRIPS];
  long off[TRIPS];
  int row[TRIPS];
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    const int c = tid + t * HN_THREADS;
    off[t] = chunk_offset<HD>(c, h0, H, ldx, by_h, row[t]);
    if (row[t] < nr) w[t] = *reinterpret_cast<const u32x4*>(base + off[t]);
  }
#pragma unroll
  for (int t = 0; t < TRIPS; ++t)
    if (row[t] < nr) *reinterpret_cast<u32x4*>(rows + (tid + t * HN_THREADS) * 16) = w[t];
  __syncthreads();
  // the staged head rows are dense: row_rstd's (token, 2 H rows) addressing with one "head" and "token" rows of two head
  // rows walks them in order.  An odd nr makes it read one row more (inside the array; its value is not used).
  ropestage::row_rstd<HD>(rows, rs, (nr + 1) >> 1, 1, 4 * HD, eps, tid);
  __syncthreads();
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    if (row[t] >= nr) continue;
    const float r = rs[row[t]];
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf2(bflo(w[t][e]) * r, bfhi(w[t][e]) * r);
    *reinterpret_cast<u32x4*>(base + off[t]) = o;
  }
  if (tid < nr) rstd[r0 + tid] = rs[tid];
}

template <int HD>
__global__ __launch_bounds__(HN_THREADS) void head_rmsnorm_bwd_kernel(bf16_t* dy, long lddy, const bf16_t* __restrict__ y,
                                                                      long ldy, const float* __restrict__ rstd,
                                                                      long nrows, int H) {
  constexpr int HQ = HD >> 3, TRIPS = (HN_ROWS * HQ + HN_THREADS - 1) / HN_THREADS;
  __shared__ float part[TRIPS * HN_THREADS];
  __shared__ float mean[HN_ROWS], rs[HN_ROWS];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * HN_ROWS;
  const int nr = (int)(nrows - r0 < HN_ROWS ? nrows - r0 : HN_ROWS);
  const long m0 = r0 / H;
  const unsigned h0 = (unsigned)(r0 - m0 * H);
  const ropestage::Div by_h((unsigned)H);
  bf16_t* gbase = dy + m0 * lddy;
  const bf16_t* ybase = y + m0 * ldy;
  u32x4 g[TRIPS], v[TRIPS];
  long off[TRIPS];
  int row[TRIPS];
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    const int c = tid + t * HN_THREADS;
    off[t] = chunk_offset<HD>(c, h0, H, lddy, by_h, row[t]);
    if (row[t] < nr) {
      int rl;
      g[t] = *reinterpret_cast<const u32x4*>(gbase + off[t]);
      v[t] = *reinterpret_cast<const u32x4*>(ybase + chunk_offset<HD>(c, h0, H, ldy, by_h, rl));
    }
  }
  if (tid < nr) rs[tid] = rstd[r0 + tid];
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    if (row[t] >= nr) continue;
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s = __builtin_fmaf(bflo(g[t][e]), bflo(v[t][e]), s);
      s = __builtin_fmaf(bfhi(g[t][e]), bfhi(v[t][e]), s);
    }
    part[tid + t * HN_THREADS] = s;
  }
  __syncthreads();
  if (tid < nr) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < HQ; ++j) s += part[tid * HQ + j];
    mean[tid] = s / (float)HD;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    if (row[t] >= nr) continue;
    const float r = rs[row[t]], mu = mean[row[t]];
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = pack_bf2(r * (bflo(g[t][e]) - bflo(v[t][e]) * mu), r * (bfhi(g[t][e]) - bfhi(v[t][e]) * mu));
    *reinterpret_cast<u32x4*>(gbase + off[t]) = o;
  }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the checks both entry points share; `who` names the entry point in the message
bool shape_ok(const char* who, int32_t M, int32_t H, int32_t hd) {
  if (M <= 0 || H <= 0 || hd <= 0) {
    vdserr::set("%s: M = %d, H = %d and hd = %d must be positive", who, (int)M, (int)H, (int)hd);
    return false;
  }
  if ((hd & 7) || hd > 128) {
    vdserr::set("%s: hd = %d must be a multiple of 8 up to 128 (a head row is hd / 8 sixteen-byte chunks)", who, (int)hd);
    return false;
  }
  if (H > 65536 || ((int64_t)M * H + HN_ROWS - 1) / HN_ROWS > 0x7fffffffLL) {
    vdserr::set("%s: H = %d above 65536 or more than 2^31 workgroups of %d head rows", who, (int)H, HN_ROWS);
    return false;
  }
  return true;
}

bool window_ok(const char* who, const char* what, const void* p, int64_t ld, int32_t H, int32_t hd) {
  if ((ld & 7) || ld < (int64_t)H * hd) {
    vdserr::set("%s: the row stride of %s (%lld) must be a multiple of 8 elements and at least H * hd = %lld", who, what,
                (long long)ld, (long long)H * hd);
    return false;
  }
  if (!al16(p)) {
    vdserr::set("%s: %s must be 16-byte aligned", who, what);
    return false;
  }
  return true;
}

// one instance per head size (shape_ok has left the multiples of 8 up to 128)
#define HN_SWITCH(hd, CALL)                                                                                       \
  switch (hd) {                                                                                                   \
    case 8: CALL(8); break; case 16: CALL(16); break; case 24: CALL(24); break; case 32: CALL(32); break;         \
    case 40: CALL(40); break; case 48: CALL(48); break; case 56: CALL(56); break; case 64: CALL(64); break;       \
    case 72: CALL(72); break; case 80: CALL(80); break; case 88: CALL(88); break; case 96: CALL(96); break;       \
    case 104: CALL(104); break; case 112: CALL(112); break; case 120: CALL(120); break; case 128: CALL(128); break; \
  }

}  // namespace

extern "C" int vds_head_rmsnorm_fwd(void* x, int64_t ldx, float* rstd, int32_t M, int32_t H, int32_t hd, float eps,
                                    vds_stream_t stream) {
  static const char who[] = "vds_head_rmsnorm_fwd";
  if (!x || !rstd) {
    vdserr::set("%s: NULL x or rstd", who);
    return VDS_ERR_ARG;
  }
  if (!shape_ok(who, M, H, hd) || !window_ok(who, "x", x, ldx, H, hd)) return VDS_ERR_ARG;
  if ((uintptr_t)rstd & 3) {
    vdserr::set("%s: rstd must be 4-byte aligned", who);
    return VDS_ERR_ARG;
  }
  if (!(eps > 0.f) || !(eps <= 3.4028234e38f)) {
    vdserr::set("%s: eps = %g must be positive and finite", who, (double)eps);
    return VDS_ERR_ARG;
  }
  const long nrows = (long)M * H;
  const dim3 grid((unsigned)((nrows + HN_ROWS - 1) / HN_ROWS));
#define CALL(HD)                                                                                              \
  hipLaunchKernelGGL(head_rmsnorm_fwd_kernel<HD>, grid, dim3(HN_THREADS), 0, (hipStream_t)stream, (bf16_t*)x, \
                     (long)ldx, rstd, nrows, (int)H, eps)
  HN_SWITCH(hd, CALL)
#undef CALL
  return ok();
}

extern "C" int vds_head_rmsnorm_bwd(void* dy, int64_t lddy, const void* y, int64_t ldy, const float* rstd, int32_t M,
                                    int32_t H, int32_t hd, vds_stream_t stream) {
  static const char who[] = "vds_head_rmsnorm_bwd";
  if (!dy || !y || !rstd) {
    vdserr::set("%s: NULL dy, y or rstd", who);
    return VDS_ERR_ARG;
  }
  if (!shape_ok(who, M, H, hd) || !window_ok(who, "dy", dy, lddy, H, hd) || !window_ok(who, "y", y, ldy, H, hd))
    return VDS_ERR_ARG;
  if ((uintptr_t)rstd & 3) {
    vdserr::set("%s: rstd must be 4-byte aligned", who);
    return VDS_ERR_ARG;
  }
  const long nrows = (long)M * H;
  const dim3 grid((unsigned)((nrows + HN_ROWS - 1) / HN_ROWS));
#define CALL(HD)                                                                                               \
  hipLaunchKernelGGL(head_rmsnorm_bwd_kernel<HD>, grid, dim3(HN_THREADS), 0, (hipStream_t)stream, (bf16_t*)dy, \
                     (long)lddy, (const bf16_t*)y, (long)ldy, rstd, nrows, (int)H)
  HN_SWITCH(hd, CALL)
#undef CALL
  return ok();
}
