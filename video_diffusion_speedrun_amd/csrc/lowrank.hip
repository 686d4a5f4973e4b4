// Low-rank adapter (LoRA) kernels for gfx950: y += s (x A^T) B^T and its backward, rank r in {16, 32, 64}.
//
// The three products of an adapter are tall-skinny: one operand has M = B*L rows (~10^5) and is streamed ONCE from
// HBM, the other is the adapter matrix (r x K, a few hundred KB at most) and the result or the second operand is the
// [M, r] activation u.  The 128 / 256 wide tiles of gemm.hip would spend > 90 % of their MFMA work on padding, and
// what these kernels cost is the one pass over the [M, .] operand -- they are built like the row kernels of
// elementwise.hip (a workgroup owns a band of rows, wide 16-byte accesses, no atomics), with
// v_mfma_f32_16x16x32_bf16 for the arithmetic so that r = 64 stays bound by HBM and not by the VALU.
//
//   vds_lowrank_down     u[m, j]  = bf16(s * sum_k x[m, k] w(j, k))         x read once; w staged in LDS in K chunks
//   vds_lowrank_up_add   y[m, n]  = bf16(y[m, n] + s * sum_j u[m, j] w(n, j))   one read + one write of y
//   vds_lowrank_wgrad    g(n, j) += s * sum_m a[m, n] u[m, j]               a read once; fp32 partials per M chunk in the
//                                                                           caller's workspace, added in chunk order
//
// Operand orientation.  The MFMA takes the SMALL matrix as its A operand (rows = j or n) and the streamed rows as its B
// operand (columns = m), so the result comes out transposed: lane (i = lane & 15, g = lane >> 4) holds row m = i and
// four CONSECUTIVE columns 4 g + 0..3 -- packed bf16 / fp32 stores instead of 2-byte scatters.  vds_lowrank_up_add
// additionally orders the rows of its A tiles so that the four tiles of a 64-column group leave 16 consecutive columns
// of y in each lane (two 16-byte accesses; the four g-lanes of a row cover 128 contiguous bytes).
//
// Every sum is over a fixed index order inside one lane / one workgroup and the M split of the weight gradient is
// reduced by a second kernel in chunk order: results are bit-identical run to run, in either determinism mode.
#include "common.h"
#include "../../include/vds.h"

namespace {

inline int ok() { return hipGetLastError() == hipSuccess ? VDS_OK : VDS_ERR_LAUNCH; }

constexpr int LR_THREADS = 256;
constexpr int LR_ROWS = 128;         // rows of x / y per workgroup: 4 waves x 2 MFMA row tiles of 16
constexpr int LR_LDS = 32 * 1024;    // staged piece of the small matrix: five workgroups share a CU's 160 KB of LDS
constexpr int WG_COLS = 128;         // vds_lowrank_wgrad: columns of a per workgroup (4 waves x 2 tiles of 16)
constexpr int WG_STEP = 64;          // ... and rows of a / u per LDS stage

// elements of K (down) / columns of y (up_add) whose part of the small matrix one LDS stage holds: rows of 2 r + 16
// bytes (k-major image) resp. r rows of 2 KC + 16 bytes (k-contiguous image; smaller) inside LR_LDS
__host__ __device__ constexpr int down_kc(int r) { return LR_LDS / (2 * r + 16) / 32 * 32; }   // 672 | 384 | 224
__host__ __device__ constexpr int up_nc(int r) { return LR_LDS / (2 * r + 16) / 64 * 64; }     // 640 | 384 | 192

typedef __attribute__((address_space(3))) s16x4* lds_s16x4_p;

// fragment (8 k for one column per lane) of a k-major LDS image via the transposing read: lane (g, i) gets rows
// k0 + 8 g .. + 7 of column c0 + i; `stride` bytes per row (a multiple of 8).  The addressing of gemm.hip's frag_km.
__device__ __forceinline__ bf16x8 frag_tr(const char* img, int k0, int c0, int stride, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const char* p = img + (k0 + 8 * g + (i >> 2)) * stride + (c0 + 4 * (i & 3)) * 2;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)LDS_PTR(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)LDS_PTR(p + 4 * stride));
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

__device__ __forceinline__ s16x8 ld8(const bf16_t* p) { return *reinterpret_cast<const s16x8*>(p); }
__device__ __forceinline__ s16x8 zero8() { return s16x8{0, 0, 0, 0, 0, 0, 0, 0}; }

// ------------------------------------------------------------------------------------------------ down
// LAYOUT 0: w [R, K] (k contiguous; LDS image [R][kc] with 16 bytes of row padding, fragments by 16-byte reads)
// LAYOUT 1: w [K, R] (k-major; LDS image [kc][R] as in memory, fragments by the transposing read)
template <int R, int LAYOUT>
__global__ __launch_bounds__(LR_THREADS) void lowrank_down_kernel(const bf16_t* __restrict__ x, long ldx,
                                                                 const bf16_t* __restrict__ w, long ldw,
                                                                 bf16_t* __restrict__ u, long ldu, int M, int K,
                                                                 float scale) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int KC = down_kc(R), JT = R / 16, S1 = 2 * R + 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
  const int Kpad = (K + 31) & ~31;
  const int kca = Kpad < KC ? Kpad : KC;  // the launch sized the LDS for this many k
  const int S0 = 2 * kca + 16;
  const int m0 = blockIdx.x * LR_ROWS + wave * 32;
  const bf16_t* xr[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int m = m0 + rt * 16 + i;
    xr[rt] = x + (long)(m < M ? m : M - 1) * ldx;  // rows past the end re-read the last row; never stored
  }
  f32x4 acc[2][JT];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) acc[rt][jt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kc0 = 0; kc0 < Kpad; kc0 += KC) {
    const int kcn = (Kpad - kc0) < KC ? (Kpad - kc0) : KC;
    if (kc0) __syncthreads();  // everyone is done reading the previous chunk
    if constexpr (LAYOUT == 0) {
      const int pr = kcn >> 3;
      for (int p = tid; p < R * pr; p += LR_THREADS) {
        const int row = p / pr, c = p - row * pr, k = kc0 + 8 * c;
        *reinterpret_cast<s16x8*>(lds + row * S0 + c * 16) = k < K ? ld8(w + (long)row * ldw + k) : zero8();
      }
    } else {
      constexpr int PR = R / 8;
      for (int p = tid; p < kcn * PR; p += LR_THREADS) {
        const int krow = p / PR, c = p % PR, k = kc0 + krow;
        *reinterpret_cast<s16x8*>(lds + krow * S1 + c * 16) = k < K ? ld8(w + (long)k * ldw + 8 * c) : zero8();
      }
    }
    __syncthreads();
    const int nks = kcn >> 5;
    for (int ks0 = 0; ks0 < nks; ks0 += 4) {  // four k steps per round: eight 16-byte loads of x in flight per lane
      bf16x8 xf[4][2];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = kc0 + 32 * (ks0 + q) + 8 * g;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
          xf[q][rt] = __builtin_bit_cast(bf16x8, (ks0 + q < nks && k < K) ? ld8(xr[rt] + k) : zero8());
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ks = ks0 + q;
        if (ks >= nks) break;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
          bf16x8 wf;
          if constexpr (LAYOUT == 0)
            wf = *reinterpret_cast<const bf16x8*>(lds + (jt * 16 + i) * S0 + (32 * ks + 8 * g) * 2);
          else
            wf = frag_tr(lds, 32 * ks, jt * 16, S1, lane);
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
            acc[rt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[q][rt], acc[rt][jt], 0, 0, 0);
        }
      }
    }
  }
  // acc[rt][jt][e] = sum_k x[m, k] w(16 jt + 4 g + e, k) for m = m0 + 16 rt + i
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int m = m0 + rt * 16 + i;
    if (m >= M) continue;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
      const f32x4 a = acc[rt][jt];
      *reinterpret_cast<u32x2*>(u + (long)m * ldu + jt * 16 + 4 * g) =
          u32x2{pack_bf2(scale * a[0], scale * a[1]), pack_bf2(scale * a[2], scale * a[3])};
    }
  }
}

// ---------------------------------------------------------------------------------------------- up_add
// LDS image of the workgroup's columns of w: [n][R] (j contiguous), rows of 2 R + 16 bytes, zero past N.
// LAYOUT 0: w [N, R] is copied row by row; LAYOUT 1: w [R, N] is transposed by the staging pass (2-byte LDS writes).
template <int R, int LAYOUT>
__global__ __launch_bounds__(LR_THREADS) void lowrank_up_add_kernel(const bf16_t* __restrict__ u, long ldu,
                                                                   const bf16_t* __restrict__ w, long ldw, bf16_t* y,
                                                                   long ldy, int M, int N, float scale) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int NC = up_nc(R), KS = R > 32 ? 2 : 1, SR = 2 * R + 16, PR = R / 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
  const int n0 = blockIdx.y * NC;
  const int nreal = (N - n0) < NC ? (N - n0) : NC;
  const int ncols = (nreal + 63) & ~63;
  if constexpr (LAYOUT == 0) {
    for (int p = tid; p < ncols * PR; p += LR_THREADS) {
      const int n = p / PR, c = p % PR;
      *reinterpret_cast<s16x8*>(lds + n * SR + c * 16) = n < nreal ? ld8(w + (long)(n0 + n) * ldw + 8 * c) : zero8();
    }
  } else {
    const int pr = ncols >> 3;
    for (int p = tid; p < R * pr; p += LR_THREADS) {
      const int j = p / pr, c = p - j * pr;
      const s16x8 v = 8 * c < nreal ? ld8(w + (long)j * ldw + n0 + 8 * c) : zero8();
#pragma unroll
      for (int e = 0; e < 8; ++e) *reinterpret_cast<short*>(lds + (8 * c + e) * SR + 2 * j) = v[e];
    }
  }
  const int m0 = blockIdx.x * LR_ROWS + wave * 32;
  bf16x8 uf[2][KS];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int m = m0 + rt * 16 + i;
    const bf16_t* ur = u + (long)(m < M ? m : M - 1) * ldu;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      uf[rt][s] = __builtin_bit_cast(bf16x8, (32 * s + 8 * g) < R ? ld8(ur + 32 * s + 8 * g) : zero8());
  }
  __syncthreads();
  for (int cg = 0; cg < ncols; cg += 64) {
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[0][t] = acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        // row i of A tile t is column cg + 16 (i >> 2) + 4 t + (i & 3): result row 4 g + e -> column cg + 16 g + 4 t + e
        const bf16x8 wf = __builtin_bit_cast(
            bf16x8, (32 * s + 8 * g) < R
                        ? *reinterpret_cast<const s16x8*>(lds + (cg + 16 * (i >> 2) + 4 * t + (i & 3)) * SR +
                                                          (32 * s + 8 * g) * 2)
                        : zero8());
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
          acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, uf[rt][s], acc[rt][t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int m = m0 + rt * 16 + i;
      if (m >= M) continue;
      bf16_t* yp = y + (long)m * ldy + n0 + cg + 16 * g;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (cg + 16 * g + 8 * h >= nreal) continue;  // N % 8 == 0: an 8-column piece is inside or outside
        const u32x4 old = *reinterpret_cast<const u32x4*>(yp + 8 * h);
        u32x4 out;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 a = acc[rt][2 * h + (q >> 1)];
          const float lo = __builtin_fmaf(scale, a[2 * (q & 1)], bflo(old[q]));
          const float hi = __builtin_fmaf(scale, a[2 * (q & 1) + 1], bfhi(old[q]));
          out[q] = pack_bf2(lo, hi);
        }
        *reinterpret_cast<u32x4*>(yp + 8 * h) = out;
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------- wgrad
// grid (column slabs of WG_COLS, M chunks of VDS_LOWRANK_WGRAD_CHUNK rows): partial[c][n][j] = sum over the chunk's
// rows of a[m, n] u[m, j].  Both operands are k-major (k = m): row tiles of WG_STEP rows go to LDS as they lie in
// memory -- the next tile's global loads are in flight while this one is multiplied -- and are read with the
// transposing LDS read.
template <int R>
__global__ __launch_bounds__(LR_THREADS) void lowrank_wgrad_kernel(const bf16_t* __restrict__ a, long lda,
                                                                  const bf16_t* __restrict__ u, long ldu,
                                                                  float* __restrict__ ws, int M, int N) {
  constexpr int SA = 2 * WG_COLS + 16, SU = 2 * R + 16, JT = R / 16, PR = R / 8;
  constexpr int UP = WG_STEP * PR;                              // 16-byte pieces of a u tile
  constexpr int UQ = (UP + LR_THREADS - 1) / LR_THREADS;
  __shared__ __attribute__((aligned(16))) char lds[WG_STEP * SA + WG_STEP * SU];
  char* la = lds;
  char* lu = lds + WG_STEP * SA;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
  const int nb = blockIdx.x * WG_COLS;
  const int mlo = blockIdx.y * VDS_LOWRANK_WGRAD_CHUNK;
  const int mhi = (M - mlo) < VDS_LOWRANK_WGRAD_CHUNK ? M : mlo + VDS_LOWRANK_WGRAD_CHUNK;
  f32x4 acc[2][JT];
#pragma unroll
  for (int at = 0; at < 2; ++at)
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) acc[at][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  s16x8 ra[4], ru[UQ];
  auto fetch = [&](int mt) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = tid + LR_THREADS * q, row = p >> 4, c = p & 15, m = mt + row, n = nb + 8 * c;
      ra[q] = (m < mhi && n < N) ? ld8(a + (long)m * lda + n) : zero8();
    }
#pragma unroll
    for (int q = 0; q < UQ; ++q) {
      const int p = tid + LR_THREADS * q, row = p / PR, c = p % PR, m = mt + row;
      ru[q] = (p < UP && m < mhi) ? ld8(u + (long)m * ldu + 8 * c) : zero8();
    }
  };
  fetch(mlo);
  for (int mt = mlo; mt < mhi; mt += WG_STEP) {
    if (mt != mlo) __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = tid + LR_THREADS * q;
      *reinterpret_cast<s16x8*>(la + (p >> 4) * SA + (p & 15) * 16) = ra[q];
    }
#pragma unroll
    for (int q = 0; q < UQ; ++q) {
      const int p = tid + LR_THREADS * q;
      if (p < UP) *reinterpret_cast<s16x8*>(lu + (p / PR) * SU + (p % PR) * 16) = ru[q];
    }
    __syncthreads();
    if (mt + WG_STEP < mhi) fetch(mt + WG_STEP);
#pragma unroll
    for (int ks = 0; ks < WG_STEP / 32; ++ks) {
      bf16x8 af[2];
#pragma unroll
      for (int at = 0; at < 2; ++at) af[at] = frag_tr(la, 32 * ks, wave * 32 + at * 16, SA, lane);
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) {
        const bf16x8 uf = frag_tr(lu, 32 * ks, jt * 16, SU, lane);
#pragma unroll
        for (int at = 0; at < 2; ++at)
          acc[at][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(uf, af[at], acc[at][jt], 0, 0, 0);
      }
    }
  }
  // acc[at][jt][e] = partial(n = nb + 32 wave + 16 at + i, j = 16 jt + 4 g + e)
  float* out = ws + (long)blockIdx.y * N * R;
#pragma unroll
  for (int at = 0; at < 2; ++at) {
    const int n = nb + wave * 32 + at * 16 + i;
    if (n >= N) continue;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) *reinterpret_cast<f32x4*>(out + (long)n * R + jt * 16 + 4 * g) = acc[at][jt];
  }
}

// g(n, j) = g(n, j) + scale * (partial[0] + partial[1] + ...)(n, j), the chunks in index order
__global__ __launch_bounds__(LR_THREADS) void lowrank_wgrad_reduce_kernel(const float* __restrict__ ws, float* g,
                                                                         long ldg, int g_layout, int N, int R,
                                                                         int chunks, float scale) {
  const long e = (long)blockIdx.x * LR_THREADS + threadIdx.x, total = (long)N * R;
  if (e >= total) return;
  float s = ws[e];
  for (int c = 1; c < chunks; ++c) s += ws[c * total + e];
  const int n = (int)(e / R), j = (int)(e % R);
  float* p = g + (g_layout == 0 ? (long)n * ldg + j : (long)j * ldg + n);
  *p = __builtin_fmaf(scale, s, *p);
}

bool rank_ok(int r) { return r == 16 || r == 32 || r == 64; }
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int vds_lowrank_down(const void* x, int64_t ldx, const void* w, int64_t ldw, int32_t w_layout, void* u,
                                int64_t ldu, int32_t M, int32_t K, int32_t r, float scale, vds_stream_t stream) {
  if (!x || !w || !u || M <= 0 || K <= 0 || !rank_ok(r) || (w_layout != 0 && w_layout != 1)) {
    vdserr::set("vds_lowrank_down: NULL operand, M or K <= 0, r = %d not in {16, 32, 64} or w_layout = %d not 0 / 1", (int)r,
                (int)w_layout);
    return VDS_ERR_ARG;
  }
  const int64_t wcols = w_layout == 0 ? K : r;
  if ((K & 7) || (ldx & 7) || (ldw & 7) || (ldu & 7) || ldx < K || ldw < wcols || ldu < r || !al16(x) || !al16(w) ||
      !al16(u)) {
    vdserr::set("vds_lowrank_down: K and every ld must be multiples of 8 elements, ld >= the row width, pointers "
                "16-byte aligned");
    return VDS_ERR_ARG;
  }
  const int Kpad = (K + 31) & ~31;
  const int kca = Kpad < down_kc(r) ? Kpad : down_kc(r);
  const size_t lds = w_layout == 0 ? (size_t)r * (2 * kca + 16) : (size_t)kca * (2 * r + 16);
  const dim3 grid((M + LR_ROWS - 1) / LR_ROWS);
  hipStream_t s = (hipStream_t)stream;
#define CALL(RR, LL)                                                                                              \
  hipLaunchKernelGGL((lowrank_down_kernel<RR, LL>), grid, dim3(LR_THREADS), lds, s, (const bf16_t*)x, (long)ldx, \
                     (const bf16_t*)w, (long)ldw, (bf16_t*)u, (long)ldu, M, K, scale)
  if (w_layout == 0) {
    if (r == 16) CALL(16, 0); else if (r == 32) CALL(32, 0); else CALL(64, 0);
  } else {
    if (r == 16) CALL(16, 1); else if (r == 32) CALL(32, 1); else CALL(64, 1);
  }
#undef CALL
  return ok();
}

extern "C" int vds_lowrank_up_add(const void* u, int64_t ldu, const void* w, int64_t ldw, int32_t w_layout, void* y,
                                  int64_t ldy, int32_t M, int32_t N, int32_t r, float scale, vds_stream_t stream) {
  if (!u || !w || !y || M <= 0 || N <= 0 || !rank_ok(r) || (w_layout != 0 && w_layout != 1)) {
    vdserr::set("vds_lowrank_up_add: NULL operand, M or N <= 0, r = %d not in {16, 32, 64} or w_layout = %d not 0 / 1",
                (int)r, (int)w_layout);
    return VDS_ERR_ARG;
  }
  const int64_t wcols = w_layout == 0 ? r : N;
  if ((N & 7) || (ldu & 7) || (ldw & 7) || (ldy & 7) || ldu < r || ldw < wcols || ldy < N || !al16(u) || !al16(w) ||
      !al16(y)) {
    vdserr::set("vds_lowrank_up_add: N and every ld must be multiples of 8 elements, ld >= the row width, pointers "
                "16-byte aligned");
    return VDS_ERR_ARG;
  }
  const int nc = up_nc(r);
  const int ncols = ((N < nc ? N : nc) + 63) & ~63;
  const size_t lds = (size_t)ncols * (2 * r + 16);
  const dim3 grid((M + LR_ROWS - 1) / LR_ROWS, (N + nc - 1) / nc);
  hipStream_t s = (hipStream_t)stream;
#define CALL(RR, LL)                                                                                                \
  hipLaunchKernelGGL((lowrank_up_add_kernel<RR, LL>), grid, dim3(LR_THREADS), lds, s, (const bf16_t*)u, (long)ldu, \
                     (const bf16_t*)w, (long)ldw, (bf16_t*)y, (long)ldy, M, N, scale)
  if (w_layout == 0) {
    if (r == 16) CALL(16, 0); else if (r == 32) CALL(32, 0); else CALL(64, 0);
  } else {
    if (r == 16) CALL(16, 1); else if (r == 32) CALL(32, 1); else CALL(64, 1);
  }
#undef CALL
  return ok();
}

extern "C" int64_t vds_lowrank_wgrad_workspace_floats(int32_t M, int32_t N, int32_t r) {
  if (M <= 0 || N <= 0 || !rank_ok(r)) return 0;
  return (int64_t)((M + VDS_LOWRANK_WGRAD_CHUNK - 1) / VDS_LOWRANK_WGRAD_CHUNK) * N * r;
}

extern "C" int vds_lowrank_wgrad(const void* a, int64_t lda, const void* u, int64_t ldu, float* g, int64_t ldg,
                                 int32_t g_layout, int32_t M, int32_t N, int32_t r, float scale, float* ws,
                                 int64_t ws_floats, vds_stream_t stream) {
  if (!a || !u || !g || !ws || M <= 0 || N <= 0 || !rank_ok(r) || (g_layout != 0 && g_layout != 1)) {
    vdserr::set("vds_lowrank_wgrad: NULL operand or workspace, M or N <= 0, r = %d not in {16, 32, 64} or g_layout = %d "
                "not 0 / 1", (int)r, (int)g_layout);
    return VDS_ERR_ARG;
  }
  const int64_t gcols = g_layout == 0 ? r : N;
  if ((N & 7) || (lda & 7) || (ldu & 7) || lda < N || ldu < r || ldg < gcols || !al16(a) || !al16(u) || !al16(ws) ||
      ((uintptr_t)g & 3)) {
    vdserr::set("vds_lowrank_wgrad: N, lda and ldu must be multiples of 8 elements, ld >= the row width, a / u / ws "
                "16-byte aligned");
    return VDS_ERR_ARG;
  }
  const int64_t need = vds_lowrank_wgrad_workspace_floats(M, N, r);
  if (ws_floats < need) {
    vdserr::set("vds_lowrank_wgrad: workspace of %lld floats, %lld needed (vds_lowrank_wgrad_workspace_floats)",
                (long long)ws_floats, (long long)need);
    return VDS_ERR_ARG;
  }
  const int chunks = (M + VDS_LOWRANK_WGRAD_CHUNK - 1) / VDS_LOWRANK_WGRAD_CHUNK;
  const dim3 grid((N + WG_COLS - 1) / WG_COLS, chunks);
  hipStream_t s = (hipStream_t)stream;
#define CALL(RR)                                                                                               \
  hipLaunchKernelGGL((lowrank_wgrad_kernel<RR>), grid, dim3(LR_THREADS), 0, s, (const bf16_t*)a, (long)lda, \
                     (const bf16_t*)u, (long)ldu, ws, M, N)
  if (r == 16) CALL(16); else if (r == 32) CALL(32); else CALL(64);
#undef CALL
  const long total = (long)N * r;
  hipLaunchKernelGGL(lowrank_wgrad_reduce_kernel, dim3((unsigned)((total + LR_THREADS - 1) / LR_THREADS)),
                     dim3(LR_THREADS), 0, s, (const float*)ws, g, (long)ldg, g_layout, N, r, chunks, scale);
  return ok();
}

extern "C" int32_t vds_lowrank_chunk(int32_t which, int32_t r) {
  if (!rank_ok(r)) return 0;
  return which == 0 ? down_kc(r) : which == 1 ? up_nc(r) : which == 2 ? VDS_LOWRANK_WGRAD_CHUNK : 0;
}
