// Row movers of token routing (DiT.enable_token_routing) for gfx950: a span of blocks runs on a subset of the
// sequence's rows, so rows are picked out of [outer, n, row] tensors by an index table and put back through its inverse.
//
//   vds_rows_gather           dst[o, i, :]  = src[o, idx[i], :]                       (a row of zeros for an index out of range)
//   vds_rows_merge            dst[o, l, :]  = 0 <= inv[l] < n_part ? part[o, inv[l], :] : full[o, l, :]
//   vds_rows_scatter_add_f32  acc[o, idx[i], :] += part[o, i, :]                      (fp32; an index out of range is skipped)
//
// All three move whole rows in 16-byte pieces and are bound by HBM.  The first two are written in bytes: one kernel serves
// the bf16 token buffer [B, L, D], residual-V's v_0 [B*H, L, hdp] and the fp32 cos / sin rows [1, L, hd/2].
//
// Geometry.  A row is Q = row_bytes / 16 pieces; the n * Q pieces of one outer slice are numbered row * Q + piece, and a
// workgroup of 256 threads owns RT_TILE = 1024 consecutive ones (16 KiB of destination whatever the row length: a 16-byte
// row and a 2304-byte row fill the chip alike).  Piece c of the tile goes to thread c % 256, trip c / 256, so a wave's
// access is 1 KiB of consecutive destination bytes and at most 1 + 1024 / row_bytes runs of consecutive source bytes.  The
// tile's first (row, piece) pair comes from one wave-uniform 64-bit division; a thread's own pair from one 32-bit one.  All
// loads of a thread are issued before its first store.  blockIdx.y is the outer slice (one workgroup per tile and slice:
// the table entry of a piece is re-read per slice, from L2; only past 65535 slices does a workgroup walk several, reusing
// its pairs); offsets are 64-bit.
// The index table lives on the device and is read by the kernel (no host read: the launches can be captured in a graph).
// No atomics, no workspace and no order that depends on the launch: results are bit-identical run to run.  The scatter-add
// is a plain read-add-write, which is only correct for distinct indices: the caller's contract.
#include "common.h"
#include "../../include/vds.h"

namespace {

inline int ok() { return hipGetLastError() == hipSuccess ? VDS_OK : VDS_ERR_LAUNCH; }

constexpr int RT_THREADS = 256;
constexpr int RT_TRIPS = 4;
constexpr int RT_TILE = RT_THREADS * RT_TRIPS;  // 16-byte pieces per workgroup

// (row, piece) of the tile's first piece; a thread adds its own offset with rt_piece
struct TileOrigin {
  long row0;
  unsigned j0;
  __device__ __forceinline__ TileOrigin(unsigned Q) {
    const unsigned long p0 = (unsigned long)blockIdx.x * RT_TILE;
    row0 = (long)(p0 / Q);
    j0 = (unsigned)(p0 - (unsigned long)row0 * Q);
  }
  // piece c of the tile -> its row (returned) and its piece j inside the row
  __device__ __forceinline__ long at(unsigned c, unsigned Q, unsigned& j) const {
    const unsigned x = j0 + c;  // < Q + RT_TILE <= 2^27 + 2^10
    const unsigned r = x / Q;
    j = x - r * Q;
    return row0 + (long)r;
  }
};

__global__ __launch_bounds__(RT_THREADS) void rows_gather_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                                 const int* __restrict__ idx, int outer, int n_in,
                                                                 int n_out, unsigned Q) {
  const TileOrigin org(Q);
  const long row_b = (long)Q * 16;
  long so[RT_TRIPS], dofs[RT_TRIPS];  // byte offsets inside an outer slice; so < 0: zeros, dofs < 0: past the end
#pragma unroll
  for (int t = 0; t < RT_TRIPS; ++t) {
    unsigned j;
    const long i = org.at((unsigned)(threadIdx.x + t * RT_THREADS), Q, j);
    dofs[t] = so[t] = -1;
    if (i < n_out) {
      const int s = idx[i];
      dofs[t] = i * row_b + (long)j * 16;
      if (s >= 0 && s < n_in) so[t] = (long)s * row_b + (long)j * 16;
    }
  }
  for (int o = blockIdx.y; o < outer; o += gridDim.y) {
    const char* sb = src + (long)o * n_in * row_b;
    char* db = dst + (long)o * n_out * row_b;
    u32x4 w[RT_TRIPS];
#pragma unroll
    for (int t = 0; t < RT_TRIPS; ++t) {
      w[t] = u32x4{0u, 0u, 0u, 0u};
      if (so[t] >= 0) w[t] = *reinterpret_cast<const u32x4*>(sb + so[t]);
    }
#pragma unroll
    for (int t = 0; t < RT_TRIPS; ++t)
      if (dofs[t] >= 0) *reinterpret_cast<u32x4*>(db + dofs[t]) = w[t];
  }
}

// full and dst are not __restrict__: they may be the same buffer.  A piece is then read and written by the same thread,
// and a row that takes no part row is left as it is (SAME: neither read nor written).
template <bool SAME>
__global__ __launch_bounds__(RT_THREADS) void rows_merge_kernel(const char* full, const char* __restrict__ part, char* dst,
                                                                const int* __restrict__ inv, int outer, int n_full,
                                                                int n_part, unsigned Q) {
  const TileOrigin org(Q);
  const long row_b = (long)Q * 16;
  long po[RT_TRIPS], dofs[RT_TRIPS];  // po >= 0: the part row's piece; po < 0: the full row's own piece (at dofs)
#pragma unroll
  for (int t = 0; t < RT_TRIPS; ++t) {
    unsigned j;
    const long l = org.at((unsigned)(threadIdx.x + t * RT_THREADS), Q, j);
    dofs[t] = po[t] = -1;
    if (l < n_full) {
      const int s = inv[l];
      const bool routed = s >= 0 && s < n_part;
      if (routed) po[t] = (long)s * row_b + (long)j * 16;
      if (routed || !SAME) dofs[t] = l * row_b + (long)j * 16;
    }
  }
  for (int o = blockIdx.y; o < outer; o += gridDim.y) {
    const char* fb = full + (long)o * n_full * row_b;
    const char* pb = part + (long)o * n_part * row_b;
    char* db = dst + (long)o * n_full * row_b;
    u32x4 w[RT_TRIPS];
#pragma unroll
    for (int t = 0; t < RT_TRIPS; ++t)
      if (dofs[t] >= 0) w[t] = *reinterpret_cast<const u32x4*>(po[t] >= 0 ? pb + po[t] : fb + dofs[t]);
#pragma unroll
    for (int t = 0; t < RT_TRIPS; ++t)
      if (dofs[t] >= 0) *reinterpret_cast<u32x4*>(db + dofs[t]) = w[t];
  }
}

__global__ __launch_bounds__(RT_THREADS) void rows_scatter_add_kernel(const float* __restrict__ part,
                                                                      float* __restrict__ acc,
                                                                      const int* __restrict__ idx, int outer, int n_full,
                                                                      int n_part, unsigned Q) {
  const TileOrigin org(Q);
  const long row_e = (long)Q * 4;
  long po[RT_TRIPS], ao[RT_TRIPS];  // element offsets inside an outer slice; ao < 0: nothing to add
#pragma unroll
  for (int t = 0; t < RT_TRIPS; ++t) {
    unsigned j;
    const long i = org.at((unsigned)(threadIdx.x + t * RT_THREADS), Q, j);
    po[t] = ao[t] = -1;
    if (i < n_part) {
      const int s = idx[i];
      if (s >= 0 && s < n_full) {
        po[t] = i * row_e + (long)j * 4;
        ao[t] = (long)s * row_e + (long)j * 4;
      }
    }
  }
  for (int o = blockIdx.y; o < outer; o += gridDim.y) {
    const float* pb = part + (long)o * n_part * row_e;
    float* ab = acc + (long)o * n_full * row_e;
    f32x4 a[RT_TRIPS], p[RT_TRIPS];
#pragma unroll
    for (int t = 0; t < RT_TRIPS; ++t)
      if (ao[t] >= 0) {
        p[t] = *reinterpret_cast<const f32x4*>(pb + po[t]);
        a[t] = *reinterpret_cast<const f32x4*>(ab + ao[t]);
      }
#pragma unroll
    for (int t = 0; t < RT_TRIPS; ++t)
      if (ao[t] >= 0) *reinterpret_cast<f32x4*>(ab + ao[t]) = a[t] + p[t];
  }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the checks the three entry points share.  rows = the row count the grid walks (n_out, n_full, n_part), other = the
// other tensor's.  Returns VDS_OK with grid filled, or the error code (message set).
int plan(const char* who, int32_t outer, int32_t rows, const char* rows_name, int32_t other, const char* other_name,
         int64_t row_bytes, const void* tab, dim3& grid) {
  if (outer <= 0 || rows < 0 || other <= 0) {
    vdserr::set("%s: outer = %d and %s = %d must be positive, %s = %d must not be negative", who, (int)outer, other_name,
                (int)other, rows_name, (int)rows);
    return VDS_ERR_ARG;
  }
  if (row_bytes <= 0 || (row_bytes & 15)) {
    vdserr::set("%s: a row of %lld bytes is no whole number of 16-byte pieces", who, (long long)row_bytes);
    return VDS_ERR_ARG;
  }
  if ((uintptr_t)tab & 3) {
    vdserr::set("%s: the index table must be 4-byte aligned", who);
    return VDS_ERR_ARG;
  }
  if (row_bytes >= (1LL << 31)) {
    vdserr::set("%s: rows of %lld bytes (2 GiB or more) are not supported", who, (long long)row_bytes);
    return VDS_ERR_UNSUPPORTED;
  }
  const int64_t tiles = ((int64_t)rows * (row_bytes >> 4) + RT_TILE - 1) / RT_TILE;
  if (tiles > 0x7fffffffLL) {
    vdserr::set("%s: %s * row_bytes / 16 = %lld pieces per outer slice need more than 2^31 - 1 workgroups of %d", who,
                rows_name, (long long)((int64_t)rows * (row_bytes >> 4)), RT_TILE);
    return VDS_ERR_UNSUPPORTED;
  }
  grid = dim3((unsigned)tiles, (unsigned)(outer < 65535 ? outer : 65535));
  return VDS_OK;
}

}  // namespace

extern "C" int vds_rows_gather(const void* src, void* dst, const int32_t* idx, int32_t outer, int32_t n_in, int32_t n_out,
                               int64_t row_bytes, vds_stream_t stream) {
  static const char who[] = "vds_rows_gather";
  if (!src || !dst || !idx) {
    vdserr::set("%s: NULL src, dst or idx", who);
    return VDS_ERR_ARG;
  }
  if (!al16(src) || !al16(dst)) {
    vdserr::set("%s: src and dst must be 16-byte aligned", who);
    return VDS_ERR_ARG;
  }
  dim3 grid;
  const int rc = plan(who, outer, n_out, "n_out", n_in, "n_in", row_bytes, idx, grid);
  if (rc != VDS_OK) return rc;
  if (n_out == 0) return VDS_OK;
  hipLaunchKernelGGL(rows_gather_kernel, grid, dim3(RT_THREADS), 0, (hipStream_t)stream, (const char*)src, (char*)dst,
                     (const int*)idx, (int)outer, (int)n_in, (int)n_out, (unsigned)(row_bytes >> 4));
  return ok();
}

extern "C" int vds_rows_merge(const void* full, const void* part, void* dst, const int32_t* inv, int32_t outer,
                              int32_t n_full, int32_t n_part, int64_t row_bytes, vds_stream_t stream) {
  static const char who[] = "vds_rows_merge";
  if (!full || !part || !dst || !inv) {
    vdserr::set("%s: NULL full, part, dst or inv", who);
    return VDS_ERR_ARG;
  }
  if (!al16(full) || !al16(part) || !al16(dst)) {
    vdserr::set("%s: full, part and dst must be 16-byte aligned", who);
    return VDS_ERR_ARG;
  }
  if (n_full <= 0 || n_part < 0) {
    vdserr::set("%s: n_full = %d must be positive and n_part = %d not negative", who, (int)n_full, (int)n_part);
    return VDS_ERR_ARG;
  }
  dim3 grid;
  const int rc = plan(who, outer, n_full, "n_full", n_full, "n_full", row_bytes, inv, grid);
  if (rc != VDS_OK) return rc;
  if (n_part == 0) return VDS_OK;  // nothing to merge: dst is not written (dst != full: the caller's copy)
  const unsigned Q = (unsigned)(row_bytes >> 4);
  if (dst == full)
    hipLaunchKernelGGL(rows_merge_kernel<true>, grid, dim3(RT_THREADS), 0, (hipStream_t)stream, (const char*)full,
                       (const char*)part, (char*)dst, (const int*)inv, (int)outer, (int)n_full, (int)n_part, Q);
  else
    hipLaunchKernelGGL(rows_merge_kernel<false>, grid, dim3(RT_THREADS), 0, (hipStream_t)stream, (const char*)full,
                       (const char*)part, (char*)dst, (const int*)inv, (int)outer, (int)n_full, (int)n_part, Q);
  return ok();
}

extern "C" int vds_rows_scatter_add_f32(const float* part, float* acc, const int32_t* idx, int32_t outer, int32_t n_full,
                                        int32_t n_part, int32_t row_elems, vds_stream_t stream) {
  static const char who[] = "vds_rows_scatter_add_f32";
  if (!part || !acc || !idx) {
    vdserr::set("%s: NULL part, acc or idx", who);
    return VDS_ERR_ARG;
  }
  if (!al16(part) || !al16(acc)) {
    vdserr::set("%s: part and acc must be 16-byte aligned", who);
    return VDS_ERR_ARG;
  }
  if (row_elems <= 0 || (row_elems & 3)) {
    vdserr::set("%s: row_elems = %d must be a positive multiple of 4 (16-byte pieces of fp32)", who, (int)row_elems);
    return VDS_ERR_ARG;
  }
  dim3 grid;
  const int rc = plan(who, outer, n_part, "n_part", n_full, "n_full", (int64_t)row_elems * 4, idx, grid);
  if (rc != VDS_OK) return rc;
  if (n_part == 0) return VDS_OK;
  hipLaunchKernelGGL(rows_scatter_add_kernel, grid, dim3(RT_THREADS), 0, (hipStream_t)stream, part, acc, (const int*)idx,
                     (int)outer, (int)n_full, (int)n_part, (unsigned)(row_elems >> 2));
  return ok();
}
