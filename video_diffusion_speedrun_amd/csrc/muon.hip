// Muon for the 2-D hidden matrices: momentum -> Newton-Schulz orthogonalisation -> parameter update, batched over a
// GROUP of `nmat` matrices of one shape [rows, cols] (fp32 parameter / gradient / momentum storage, each matrix given
// by pointers: the row slices of qkv.weight / context_kv.weight are matrices at pointer offsets).
//
// Inside the workspace a matrix is held as [m, n] with m = min(rows, cols): a tall matrix (rows > cols) is transposed on
// the way in (momentum kernel) and back on the way out (update kernel), both through a 64 x 64 LDS tile, so that the
// Gram matrix of the iteration is the small one.  Workspace sections (see muon_layout):
//     x0, x1   bf16 [nmat, m, n]   the iterate, ping-pong; x0 receives u from the momentum kernel and holds O at the end
//     a,  b    bf16 [nmat, m, m]   A = X X^T and B = b A + c A A
//     sumsq    f32  [nmat]         ||u||_F^2 per matrix;  partials f32 [nmat, tiles]: its first stage
//
// The iteration's three products run on ONE tile kernel (ns_gemm_kernel): 128 x 128 x 64 tiles, 4 waves of 4 x 4
// v_mfma_f32_16x16x32_bf16, operand tiles by LDS-DMA into a double-buffered, source-swizzled LDS image -- the structure
// and the tile formats of the 128^2 kernel of gemm.hip --, the matrix index on blockIdx.y, and the epilogue
// C = bf16(alpha * acc + beta * addend).  A = X X^T and A A (= A A^T: A is symmetric) are "NT" products of a matrix with
// itself: only the tiles on or above the diagonal are computed and every off-diagonal tile is stored twice, the second
// time mirrored.  B X is the "NN" product (X is read k-major with ds_read_b64_tr_b16).  No split-K, no atomics: every
// output element is one fixed-order fp32 sum, bit-identical run to run.
#include "common.h"
#include "../../include/vds.h"

namespace {

struct MuonMat {  // vds_muon_mat
  float* p; const float* g; float* buf; bf16_t* pb; float* ema;
};
struct Guard {  // vds_optim_guard
  float norm; float coef; int skipped; int n_skipped;
};

constexpr int ET = 64;  // tile edge of the element-wise kernels

struct Layout {
  int m, n, tiles;
  size_t x0, x1, a, b, sumsq, partials, total;  // byte offsets
};
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline Layout muon_layout(int nmat, int rows, int cols) {
  Layout L;
  L.m = rows < cols ? rows : cols;
  L.n = rows < cols ? cols : rows;
  L.tiles = cdiv(rows, ET) * cdiv(cols, ET);
  const size_t xb = up256((size_t)nmat * L.m * L.n * 2), gb = up256((size_t)nmat * L.m * L.m * 2);
  L.x0 = 0;
  L.x1 = xb;
  L.a = 2 * xb;
  L.b = L.a + gb;
  L.sumsq = L.b + gb;
  L.partials = L.sumsq + up256((size_t)nmat * 4);
  L.total = L.partials + up256((size_t)nmat * L.tiles * 4);
  return L;
}

inline bool shape_ok(int nmat, int rows, int cols) {
  return nmat >= 1 && nmat <= 65535 && rows >= 8 && cols >= 8 && rows % 8 == 0 && cols % 8 == 0 &&
         rows <= (1 << 20) && cols <= (1 << 20) && (size_t)rows * cols <= ((size_t)1 << 28);  // 32-bit tile offsets
}

// ------------------------------------------------------------------------------------ momentum ---
// One workgroup per 64 x 64 tile of the [rows, cols] matrix (blockIdx.x) and matrix (blockIdx.y):
//   g' = coef g;  buf = mu buf + g';  u = nesterov ? g' + mu buf : buf;  x0 = bf16(u)  (transposed when rows > cols)
// and one fp32 partial of sum u^2 per workgroup (per-thread sums in element order, wave butterfly, four adds).
__global__ __launch_bounds__(256) void muon_momentum_kernel(const MuonMat* mats, int rows, int cols, float mu,
                                                            int nesterov, const Guard* guard, bf16_t* x0,
                                                            float* partials, int tiles_c) {
  __shared__ float tile[ET][ET + 1];
  __shared__ float red[4];
  float coef = 1.0f;
  if (guard) {
    if (guard->skipped) return;  // uniform over the grid: the momentum keeps every bit
    coef = guard->coef;
  }
  const MuonMat t = mats[blockIdx.y];
  const int r0 = (blockIdx.x / tiles_c) * ET, c0 = (blockIdx.x % tiles_c) * ET;
  const bool tall = rows > cols;
  const int n = tall ? rows : cols;
  bf16_t* X = x0 + (size_t)blockIdx.y * rows * cols;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  float s = 0.f;
#pragma unroll 4
  for (int i = 0; i < ET / 4; ++i) {
    const int r = r0 + ty + 4 * i, c = c0 + tx;
    float u = 0.f;
    if (r < rows && c < cols) {
      const size_t idx = (size_t)r * cols + c;
      const float g = t.g[idx] * coef;
      const float b = mu * t.buf[idx] + g;
      t.buf[idx] = b;
      u = nesterov ? g + mu * b : b;
      s += u * u;
      if (!tall) X[(size_t)r * n + c] = f2bf(u);
    }
    if (tall) tile[ty + 4 * i][tx] = u;
  }
  if (tall) {  // (uniform) write the tile transposed: workspace row = column of the matrix
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < ET / 4; ++i) {
      const int c = c0 + ty + 4 * i, r = r0 + tx;
      if (r < rows && c < cols) X[(size_t)c * n + r] = f2bf(tile[tx][ty + 4 * i]);
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// second stage: one workgroup per matrix adds its partials in a fixed lane / butterfly order
__global__ __launch_bounds__(256) void muon_sumsq_final_kernel(const float* partials, int n, float* sumsq,
                                                               const Guard* guard) {
  __shared__ float red[4];
  if (guard && guard->skipped) return;
  float s = 0.f;
  for (int j = threadIdx.x; j < n; j += 256) s += partials[(size_t)blockIdx.x * n + j];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) sumsq[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// X = bf16(u / (||u||_F + 1e-7)), 8 elements per thread; src == dst allowed (every thread rewrites what it read)
__global__ __launch_bounds__(256) void muon_normalize_kernel(const bf16_t* src, bf16_t* dst, const float* sumsq,
                                                             long per_mat) {
  const float inv = 1.0f / (sqrtf(sumsq[blockIdx.y]) + 1e-7f);
  const bf16_t* s = src + (size_t)blockIdx.y * per_mat;
  bf16_t* d = dst + (size_t)blockIdx.y * per_mat;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8; i < per_mat; i += (long)gridDim.x * 256 * 8) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(s + i);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf2(bflo(v[e]) * inv, bfhi(v[e]) * inv);
    *reinterpret_cast<u32x4*>(d + i) = o;
  }
}

// -------------------------------------------------------------------------------------- update ---
//   p = p (1 - lr wd) - lr scale O   (O = x0, un-transposed when rows > cols), shadow = bf16(p), ema = d ema + (1-d) p
// lr = base lr x the schedule multiplier; with sc_dev the multiplier and the EMA decay are scalars_dev[2], [3] of
// MuAdamW.use_device_scalars.  A skipped step writes nothing.
__global__ __launch_bounds__(256) void muon_update_kernel(const MuonMat* mats, int rows, int cols, float lr, float wd,
                                                          float scale, float lr_mult, float ema_decay,
                                                          const float* sc_dev, const Guard* guard, const bf16_t* x0,
                                                          int tiles_c) {
  __shared__ float tile[ET][ET + 1];
  if (guard && guard->skipped) return;
  if (sc_dev) {
    lr_mult = sc_dev[2];
    ema_decay = sc_dev[3];
  }
  const float lr_eff = lr * lr_mult;
  const float decay = 1.0f - lr_eff * wd, step = lr_eff * scale, ema_in = 1.0f - ema_decay;
  const MuonMat t = mats[blockIdx.y];
  const int r0 = (blockIdx.x / tiles_c) * ET, c0 = (blockIdx.x % tiles_c) * ET;
  const bool tall = rows > cols;
  const int n = tall ? rows : cols;
  const bf16_t* X = x0 + (size_t)blockIdx.y * rows * cols;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  if (tall) {
#pragma unroll 4
    for (int i = 0; i < ET / 4; ++i) {
      const int c = c0 + ty + 4 * i, r = r0 + tx;
      tile[ty + 4 * i][tx] = (r < rows && c < cols) ? bf2f(X[(size_t)c * n + r]) : 0.f;
    }
    __syncthreads();
  }
#pragma unroll 4
  for (int i = 0; i < ET / 4; ++i) {
    const int r = r0 + ty + 4 * i, c = c0 + tx;
    if (r < rows && c < cols) {
      const size_t idx = (size_t)r * cols + c;
      const float o = tall ? tile[tx][ty + 4 * i] : bf2f(X[(size_t)r * n + c]);
      const float p = t.p[idx] * decay - step * o;
      t.p[idx] = p;
      if (t.pb) t.pb[idx] = f2bf(p);
      if (t.ema) t.ema[idx] = ema_decay * t.ema[idx] + ema_in * p;
    }
  }
}

// ----------------------------------------------------------------------------- the tile kernel ---
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 16384;     // one operand tile, either format
constexpr int LDS_BYTES = 4 * TILE_BYTES;  // two buffers of (A tile | B tile)

struct NsP {
  const bf16_t* A; long sA; int lda;      // [M, K], k contiguous; matrix i at A + i * sA
  const bf16_t* B; long sB; int ldb;      // B_KM ? [K, N] : [N, K]
  bf16_t* C; long sC; int ldc;            // [M, N]
  const bf16_t* add; long sAdd; int ldadd;  // [M, N] or NULL
  float alpha, beta;
  int M, N, K;
  int tiles_m, tiles_n;
};

// Tile formats and swizzles of the 128^2 GEMM (gemm.hip): a k-contiguous tile is [128 rows][64 k] with 128-byte rows of
// 8 16-byte chunks, a k-major tile [64 k][128 cols] with 256-byte rows of 8 32-byte segments.  The LDS-DMA writes LDS
// lane-linearly, so the swizzle goes on the per-lane SOURCE address and again on the fragment read.
__device__ __forceinline__ int swz_kc(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
__device__ __forceinline__ int swz_km(int krow) { return (krow & 3) | (((krow >> 3) & 1) << 2); }

template <bool KMAJOR>
__device__ __forceinline__ void stage_offsets(unsigned voff[4], int wave, int lane, long ld, int origin) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = wave * 4 + j;
    if constexpr (!KMAJOR) {
      const int row = q * 8 + (lane >> 3);
      const int chunk = swz_kc(row, lane & 7);
      voff[j] = (unsigned)(((long)(origin + row) * ld + chunk * 8) * 2);
    } else {
      const int krow = q * 4 + (lane >> 4);
      const int pc = lane & 15;
      const int chunk = (((pc >> 1) ^ swz_km(krow)) << 1) | (pc & 1);
      voff[j] = (unsigned)(((long)krow * ld + origin + chunk * 8) * 2);
    }
  }
}

// `krem` (k-contiguous operands only): elements of K left in this tile; 16-byte chunks at or past it are redirected out of
// the SRD's range (-> zero).  Rows past the end of a matrix -- the K tail of a k-major operand too -- read as zero
// through the SRD's num_records, which is set per matrix of the group.
template <bool KMAJOR>
__device__ __forceinline__ void stage_tile(srd_t rsrc, char* lds_tile, const unsigned voff[4], unsigned koff, int wave,
                                           int lane, int krem) {
  const unsigned base = lds_addr_of(lds_tile) + wave * 4096;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned off = voff[j] + koff;
    if constexpr (!KMAJOR) {
      if (krem < BK) {
        const int row = (wave * 4 + j) * 8 + (lane >> 3);
        if (swz_kc(row, lane & 7) * 8 >= krem) off = 0xfffffff0u;
      }
    }
    lds_dma16(rsrc, base + j * 1024, off);
  }
}

// fragment of a k-contiguous tile: 16 rows x 32 k, lane -> row (l & 15), k 8 (l >> 4) .. + 7
__device__ __forceinline__ bf16x8 frag_kc(const char* tile, int row0, int ks, int lane) {
  const int row = row0 + (lane & 15);
  const int chunk = swz_kc(row, ks * 4 + (lane >> 4));
  return *reinterpret_cast<const bf16x8*>(tile + row * 128 + chunk * 16);
}
// fragment of a k-major tile through the transposing read: 16 cols x 32 k
__device__ __forceinline__ bf16x8 frag_km(const char* tile, int col0, int ks, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const int krow = ks * 32 + 8 * g + (i >> 2);
  const int seg = (col0 >> 4) ^ swz_km(krow);
  const char* p = tile + krow * 256 + seg * 32 + (i & 3) * 8;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p + 4 * 256));
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// C[M,N] = bf16(alpha * sum_k A[m,k] opB[k,n] + beta * add[m,n]) for matrix blockIdx.y of the group.
// SYM (NT product of a matrix with itself, M == N, C symmetric): blockIdx.x enumerates the tiles with tile_m <= tile_n
// row by row; a tile off the diagonal is also stored mirrored.
template <bool B_KM, bool SYM>
__global__ __launch_bounds__(256, 2) void ns_gemm_kernel(NsP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  int tile_m, tile_n;
  if constexpr (SYM) {
    int rem = blockIdx.x;
    tile_m = 0;
    while (rem >= p.tiles_n - tile_m) {
      rem -= p.tiles_n - tile_m;
      ++tile_m;
    }
    tile_n = tile_m + rem;
  } else {
    tile_m = blockIdx.x % p.tiles_m;
    tile_n = blockIdx.x / p.tiles_m;
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const long mat = blockIdx.y;
  const bf16_t* A = p.A + mat * p.sA;
  const bf16_t* B = p.B + mat * p.sB;

  const srd_t ra = make_srd(A, (unsigned)((size_t)p.M * p.lda * 2));
  const srd_t rb = make_srd(B, (unsigned)((size_t)(B_KM ? p.K : p.N) * p.ldb * 2));
  unsigned va[4], vb[4];
  stage_offsets<false>(va, wave, lane, p.lda, m0);
  stage_offsets<B_KM>(vb, wave, lane, p.ldb, n0);
  const unsigned a_step = BK * 2;
  const unsigned b_step = B_KM ? (unsigned)(BK * p.ldb * 2) : BK * 2;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kt_end = (p.K + BK - 1) / BK;
  // LDS: [buf0: A | B][buf1: A | B]
  stage_tile<false>(ra, smem, va, 0, wave, lane, p.K);
  stage_tile<B_KM>(rb, smem + TILE_BYTES, vb, 0, wave, lane, p.K);
  VDS_WAIT_VM(0);
  __syncthreads();  // tile 0 landed (the DMA is invisible to the compiler: waited above)

  int cur = 0;
  for (int kt = 0; kt < kt_end; ++kt) {
    if (kt + 1 < kt_end) {
      char* nxt = smem + (cur ^ 1) * 2 * TILE_BYTES;
      stage_tile<false>(ra, nxt, va, (kt + 1) * a_step, wave, lane, p.K - (kt + 1) * BK);
      stage_tile<B_KM>(rb, nxt + TILE_BYTES, vb, (kt + 1) * b_step, wave, lane, p.K - (kt + 1) * BK);
    }
    const char* ta = smem + cur * 2 * TILE_BYTES;
    const char* tb = ta + TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = frag_kc(ta, wm * 64 + i * 16, ks, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (B_KM) fb[j] = frag_km(tb, wn * 64 + j * 16, ks, lane);
        else fb[j] = frag_kc(tb, wn * 64 + j * 16, ks, lane);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    VDS_WAIT_VM(0);
    __syncthreads();  // next tile landed and everyone is done reading `cur`
    cur ^= 1;
  }

  // ---- epilogue, straight from the accumulators: lane (g = l >> 4, c = l & 15) holds rows 4g .. 4g+3 of column c of
  // every 16 x 16 block.  M, N are multiples of 8, so the four rows are valid together.
  bf16_t* C = p.C + mat * p.sC;
  const bf16_t* add = p.add ? p.add + mat * p.sAdd : nullptr;
  const bool mirror = SYM && tile_m != tile_n;
  const int g = lane >> 4, c16 = lane & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = m0 + wm * 64 + i * 16 + 4 * g;
      const int col = n0 + wn * 64 + j * 16 + c16;
      if (row < p.M && col < p.N) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = p.alpha * acc[i][j][r];
          if (add) v[r] += p.beta * bf2f(add[(size_t)(row + r) * p.ldadd + col]);
        }
        const u32x2 w = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
#pragma unroll
        for (int r = 0; r < 4; ++r)
          C[(size_t)(row + r) * p.ldc + col] = (bf16_t)((r & 1) ? (w[r >> 1] >> 16) : (w[r >> 1] & 0xffffu));
        if (mirror) *reinterpret_cast<u32x2*>(C + (size_t)col * p.ldc + row) = w;  // C^T: four rows = 8 contiguous bytes
      }
    }
}

template <bool B_KM, bool SYM>
int launch_ns(const NsP& p, int nmat, hipStream_t s) {
  const int tiles = SYM ? p.tiles_n * (p.tiles_n + 1) / 2 : p.tiles_m * p.tiles_n;
  vds_launch<ns_gemm_kernel<B_KM, SYM>, LDS_BYTES>(dim3(tiles, nmat), dim3(256), LDS_BYTES, s, p);
  return hipGetLastError() == hipSuccess ? VDS_OK : VDS_ERR_LAUNCH;
}

}  // namespace

extern "C" size_t vds_muon_workspace_bytes(int32_t nmat, int32_t rows, int32_t cols) {
  if (!shape_ok(nmat, rows, cols)) return 0;
  return muon_layout(nmat, rows, cols).total;
}

extern "C" int vds_muon_workspace_layout(int32_t nmat, int32_t rows, int32_t cols, int64_t* offsets6) {
  if (!shape_ok(nmat, rows, cols) || !offsets6) return VDS_ERR_ARG;
  const Layout L = muon_layout(nmat, rows, cols);
  offsets6[0] = (int64_t)L.x0; offsets6[1] = (int64_t)L.x1; offsets6[2] = (int64_t)L.a; offsets6[3] = (int64_t)L.b;
  offsets6[4] = (int64_t)L.sumsq; offsets6[5] = (int64_t)L.partials;
  return VDS_OK;
}

extern "C" int vds_muon_momentum(const vds_muon_mat* mats_dev, int32_t nmat, int32_t rows, int32_t cols, float mu,
                                 int32_t nesterov, const vds_optim_guard* guard_or_null, void* workspace,
                                 vds_stream_t stream) {
  static_assert(sizeof(vds_muon_mat) == sizeof(MuonMat), "descriptor layout");
  static_assert(sizeof(vds_optim_guard) == sizeof(Guard), "guard record layout");
  if (!mats_dev || !workspace || !shape_ok(nmat, rows, cols) || !(mu >= 0.f && mu < 1.f)) return VDS_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return VDS_ERR_ARG;
  const Layout L = muon_layout(nmat, rows, cols);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(muon_momentum_kernel, dim3(L.tiles, nmat), dim3(256), 0, s, (const MuonMat*)mats_dev, rows, cols,
                     mu, nesterov, (const Guard*)guard_or_null, (bf16_t*)(ws + L.x0), (float*)(ws + L.partials),
                     cdiv(cols, ET));
  hipLaunchKernelGGL(muon_sumsq_final_kernel, dim3(nmat), dim3(256), 0, s, (const float*)(ws + L.partials), L.tiles,
                     (float*)(ws + L.sumsq), (const Guard*)guard_or_null);
  return hipGetLastError() == hipSuccess ? VDS_OK : VDS_ERR_LAUNCH;
}

extern "C" int vds_muon_orthogonalize(void* workspace, int32_t nmat, int32_t rows, int32_t cols, int32_t steps,
                                      vds_stream_t stream) {
  if (!workspace || !shape_ok(nmat, rows, cols) || steps < 0 || steps > 64) return VDS_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return VDS_ERR_ARG;
  const Layout L = muon_layout(nmat, rows, cols);
  const int m = L.m, n = L.n;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  bf16_t* x[2] = {(bf16_t*)(ws + L.x0), (bf16_t*)(ws + L.x1)};
  bf16_t* ga = (bf16_t*)(ws + L.a);
  bf16_t* gb = (bf16_t*)(ws + L.b);
  const long per = (long)m * n;
  // the iterate starts in the slot from which `steps` ping-pong moves end in x0
  int cur = steps & 1;
  {
    const int blocks = (int)((per / 8 + 255) / 256);
    hipLaunchKernelGGL(muon_normalize_kernel, dim3(blocks < 1024 ? blocks : 1024, nmat), dim3(256), 0, s,
                       (const bf16_t*)x[0], x[cur], (const float*)(ws + L.sumsq), per);
  }
  const float ca = 3.4445f, cb = -4.7750f, cc = 2.0315f;
  const int tm = cdiv(m, BM), tn = cdiv(n, BN);
  for (int it = 0; it < steps; ++it) {
    NsP p;
    // A = X X^T
    p = NsP{x[cur], per, n, x[cur], per, n, ga, (long)m * m, m, nullptr, 0, 0, 1.0f, 0.0f, m, m, n, tm, tm};
    int rc = launch_ns<false, true>(p, nmat, s);
    if (rc != VDS_OK) return rc;
    // B = b A + c A A
    p = NsP{ga, (long)m * m, m, ga, (long)m * m, m, gb, (long)m * m, m, ga, (long)m * m, m, cc, cb, m, m, m, tm, tm};
    rc = launch_ns<false, true>(p, nmat, s);
    if (rc != VDS_OK) return rc;
    // X' = a X + B X
    p = NsP{gb, (long)m * m, m, x[cur], per, n, x[cur ^ 1], per, n, x[cur], per, n, 1.0f, ca, m, n, m, tm, tn};
    rc = launch_ns<true, false>(p, nmat, s);
    if (rc != VDS_OK) return rc;
    cur ^= 1;
  }
  return hipGetLastError() == hipSuccess ? VDS_OK : VDS_ERR_LAUNCH;
}

extern "C" int vds_muon_update(const vds_muon_mat* mats_dev, int32_t nmat, int32_t rows, int32_t cols, float lr,
                               float weight_decay, float lr_mult, float ema_decay, const float* scalars_dev,
                               const vds_optim_guard* guard_or_null, const void* workspace, vds_stream_t stream) {
  if (!mats_dev || !workspace || !shape_ok(nmat, rows, cols)) return VDS_ERR_ARG;
  if (!scalars_dev && !(ema_decay >= 0.f && ema_decay < 1.f)) return VDS_ERR_ARG;
  const Layout L = muon_layout(nmat, rows, cols);
  const float ratio = (float)rows / (float)cols;
  const float scale = sqrtf(ratio > 1.0f ? ratio : 1.0f);
  hipLaunchKernelGGL(muon_update_kernel, dim3(L.tiles, nmat), dim3(256), 0, (hipStream_t)stream,
                     (const MuonMat*)mats_dev, rows, cols, lr, weight_decay, scale, lr_mult, ema_decay, scalars_dev,
                     (const Guard*)guard_or_null, (const bf16_t*)((const char*)workspace + L.x0), cdiv(cols, ET));
  return hipGetLastError() == hipSuccess ? VDS_OK : VDS_ERR_LAUNCH;
}
