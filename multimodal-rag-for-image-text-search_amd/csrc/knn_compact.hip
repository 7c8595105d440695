// knn_compact.hip — K15: compaction of a flat index after deletes.
//
//   K15a  row remap: remap[r] = number of live rows before r (label != MRAG_LABEL_DELETED), or
//         -1 for a deleted row: an exclusive prefix sum over up to 2^31 - 1 flags. Three kinds
//         of launch and no hand-off between workgroups inside one: (1) each workgroup counts the
//         live flags of its 4096 labels, (2) the block counts are scanned by the same two
//         kernels, recursing until one workgroup holds them all (4096^3 > 2^31: at most three
//         levels), (3) each workgroup scans its labels again, adds its block's offset and writes.
//         No look-back and no spinning on another workgroup's flag: the launches order the levels.
//   K15b  gather: every live row's x16 / x32 / xn / label bytes go to row remap[r] of new
//         buffers, a wave (a half-wave at DP 128) per row, 16 bytes per lane and instruction.
//
// Both are memory-bound: K15a moves 12 bytes per row (labels twice, remap once), K15b reads and
// writes 6 DP + 12 bytes per live row.
#include "knn_compact.h"
#include "devbuf.h"

#include <algorithm>

namespace mrag_knn {
namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

constexpr int REMAP_THREADS = 256;
constexpr int REMAP_CHUNK = REMAP_THREADS * 4;         // labels per pass of a workgroup
constexpr int REMAP_PASSES = REMAP_BLOCK / REMAP_CHUNK;  // 4
static_assert(REMAP_PASSES * REMAP_CHUNK == REMAP_BLOCK, "block = passes x chunk");

// Four consecutive values from index i (a multiple of 4; `in` 16-byte aligned): labels become
// live flags, block sums stay as they are; past n the value is 0.
template <bool FLAGS>
__device__ __forceinline__ i32x4 remap_load4(const int32_t* __restrict__ in, int64_t i, int64_t n) {
  i32x4 v;
  if (i + 3 < n) {
    v = *(const i32x4*)(in + i);
  } else {
    const int32_t pad = FLAGS ? (int32_t)MRAG_LABEL_DELETED : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (i + e < n) ? in[i + e] : pad;
  }
  if (FLAGS) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] != (int32_t)MRAG_LABEL_DELETED ? 1 : 0;
  }
  return v;
}

// sums[b] = sum over block b of the flags (FLAGS) or values of in[0..n)
template <bool FLAGS>
__global__ __launch_bounds__(REMAP_THREADS) void remap_reduce_kernel(const int32_t* __restrict__ in, int64_t n,
                                                                     int32_t* __restrict__ sums) {
  __shared__ int32_t wsum[REMAP_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * REMAP_BLOCK;
  int32_t s = 0;
#pragma unroll
  for (int j = 0; j < REMAP_PASSES; ++j) {
    const i32x4 v = remap_load4<FLAGS>(in, base + j * REMAP_CHUNK + threadIdx.x * 4, n);
    s += v[0] + v[1] + v[2] + v[3];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// out[i] = offsets[block] + exclusive prefix inside the block (offsets null: 0). FLAGS: the
// prefix counts live labels and a deleted row gets -1. total (optional, one-block grids):
// the sum of everything.
template <bool FLAGS>
__global__ __launch_bounds__(REMAP_THREADS) void remap_scan_kernel(const int32_t* __restrict__ in, int64_t n,
                                                                   const int32_t* __restrict__ offsets,
                                                                   int32_t* __restrict__ out,
                                                                   int32_t* __restrict__ total) {
  constexpr int NW = REMAP_THREADS / 64;
  __shared__ int32_t wsum[REMAP_PASSES * NW];  // [pass][wave]: the order of the labels
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * REMAP_BLOCK;
  i32x4 v[REMAP_PASSES];
  int32_t own[REMAP_PASSES], inc[REMAP_PASSES];
#pragma unroll
  for (int j = 0; j < REMAP_PASSES; ++j) {
    v[j] = remap_load4<FLAGS>(in, base + j * REMAP_CHUNK + threadIdx.x * 4, n);
    own[j] = v[j][0] + v[j][1] + v[j][2] + v[j][3];
  }
#pragma unroll
  for (int j = 0; j < REMAP_PASSES; ++j) {  // inclusive scan across the wave
    int32_t x = own[j];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    inc[j] = x;
    if (lane == 63) wsum[j * NW + wave] = x;
  }
  __syncthreads();
  int32_t before[REMAP_PASSES];  // everything in front of this wave's part of pass j
  int32_t run = offsets ? offsets[blockIdx.x] : 0;
#pragma unroll
  for (int q = 0; q < REMAP_PASSES * NW; ++q) {
    if ((q % NW) == 0) {
#pragma unroll
      for (int j = 0; j < REMAP_PASSES; ++j)
        if (j == q / NW) before[j] = run;
    }
    const int32_t w = wsum[q];
    if ((q % NW) < wave) {
#pragma unroll
      for (int j = 0; j < REMAP_PASSES; ++j)
        if (j == q / NW) before[j] += w;
    }
    run += w;
  }
  if (total && blockIdx.x == 0 && threadIdx.x == 0) *total = run;
#pragma unroll
  for (int j = 0; j < REMAP_PASSES; ++j) {
    const int64_t i = base + j * REMAP_CHUNK + threadIdx.x * 4;
    int32_t p = before[j] + inc[j] - own[j];
    i32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = (!FLAGS || v[j][e]) ? p : -1;
      p += v[j][e];
    }
    if (i + 3 < n) {
      *(i32x4*)(out + i) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < n) out[i + e] = o[e];
    }
  }
}

inline int64_t pad4(int64_t x) { return (x + 3) / 4 * 4; }

// Exclusive scan of in[0..n) into out (FLAGS: of the live flags, as the remap), total optional.
template <bool FLAGS>
int scan_level(const int32_t* in, int64_t n, int32_t* out, int32_t* total, int32_t* scratch, hipStream_t s) {
  const int64_t nb = (n + REMAP_BLOCK - 1) / REMAP_BLOCK;
  if (nb <= 1) {
    hipLaunchKernelGGL(remap_scan_kernel<FLAGS>, dim3(1), dim3(REMAP_THREADS), 0, s, in, n, (const int32_t*)nullptr,
                       out, total);
    MRAG_CHECK_LAUNCH();
    return MRAG_OK;
  }
  int32_t* sums = scratch;
  int32_t* offs = scratch + pad4(nb);
  hipLaunchKernelGGL(remap_reduce_kernel<FLAGS>, dim3((unsigned)nb), dim3(REMAP_THREADS), 0, s, in, n, sums);
  MRAG_CHECK_LAUNCH();
  if (int rc = scan_level<false>(sums, nb, offs, total, scratch + 2 * pad4(nb), s)) return rc;
  hipLaunchKernelGGL(remap_scan_kernel<FLAGS>, dim3((unsigned)nb), dim3(REMAP_THREADS), 0, s, in, n,
                     (const int32_t*)offs, out, (int32_t*)nullptr);
  MRAG_CHECK_LAUNCH();
  return MRAG_OK;
}

// LPR lanes copy one row: a wave (64) or, at DP 128 where an x32 row is 32 chunks of 16 bytes,
// a half-wave (32).
template <int LPR>
__global__ __launch_bounds__(256) void gather_rows_kernel(const u32x4* __restrict__ x16, const u32x4* __restrict__ x32,
                                                          const double* __restrict__ xn,
                                                          const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ remap, int64_t n, int DP,
                                                          u32x4* __restrict__ o16, u32x4* __restrict__ o32,
                                                          double* __restrict__ oxn, int32_t* __restrict__ olab) {
  constexpr int RPW = 64 / LPR;  // rows per wave and step
  const int lane = threadIdx.x & 63, sub = lane % LPR;
  const int c16 = DP / 8, c32 = DP / 4;  // 16-byte chunks of a row
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t r0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW; r0 < n; r0 += nwaves * RPW) {
    const int64_t r = r0 + lane / LPR;
    if (r >= n) continue;
    const int64_t d = remap[r];
    if (d < 0) continue;
    const u32x4* s32 = x32 + r * c32;
    u32x4* d32 = o32 + d * c32;
    for (int c = sub; c < c32; c += LPR) d32[c] = s32[c];
    const u32x4* s16 = x16 + r * c16;
    u32x4* d16 = o16 + d * c16;
    for (int c = sub; c < c16; c += LPR) d16[c] = s16[c];
    if (sub == 0) {
      oxn[d] = xn[r];
      olab[d] = labels[r];
    }
  }
}

}  // namespace

size_t remap_scratch_words(int64_t n) {
  size_t words = 4;
  for (int64_t nb = (n + REMAP_BLOCK - 1) / REMAP_BLOCK; nb > 1; nb = (nb + REMAP_BLOCK - 1) / REMAP_BLOCK)
    words += 2 * (size_t)pad4(nb);
  return words;
}

int row_remap(const int32_t* labels, int64_t n, int32_t* remap, int32_t* live_dev, int32_t* scratch, hipStream_t s) {
  if (n <= 0) {
    MRAG_HIP(hipMemsetAsync(live_dev, 0, 4, s));
    return MRAG_OK;
  }
  return scan_level<true>(labels, n, remap, live_dev, scratch, s);
}

int gather_rows(const GatherRows& g, hipStream_t s) {
  if (g.n <= 0) return MRAG_OK;
  const bool half = g.DP == 128;
  const int64_t rows_per_block = half ? 8 : 4;
  const unsigned blocks = (unsigned)std::min<int64_t>((g.n + rows_per_block - 1) / rows_per_block, 2048);
  auto fn = half ? gather_rows_kernel<32> : gather_rows_kernel<64>;
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(256), 0, s, (const u32x4*)g.x16, (const u32x4*)g.x32, g.xn, g.labels,
                     g.remap, g.n, g.DP, (u32x4*)g.out_x16, (u32x4*)g.out_x32, g.out_xn, g.out_labels);
  MRAG_CHECK_LAUNCH();
  return MRAG_OK;
}

}  // namespace mrag_knn

extern "C" int mrag_knn_row_remap(const int32_t* labels, int64_t n, int32_t* remap, int64_t* live, void* stream) {
  MRAG_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n=%lld out of range [0, 2^31)", (long long)n);
  MRAG_REQUIRE(live != nullptr, "live is NULL");
  *live = 0;
  if (n == 0) return MRAG_OK;
  MRAG_REQUIRE(labels != nullptr && remap != nullptr, "NULL labels/remap");
  MRAG_REQUIRE(((uintptr_t)labels & 15) == 0 && ((uintptr_t)remap & 15) == 0, "labels and remap must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  mrag::DevBuf buf;  // exactly these bytes (a fresh buffer); freed on every path, after the wait below
  if (int rc = mrag::ensure_doubling(buf, mrag_knn::remap_scratch_words(n) * 4)) return rc;
  int32_t* scratch = (int32_t*)buf.p;  // [0]: the live count; from word 4: the block sums
  int rc = mrag_knn::row_remap(labels, n, remap, scratch, scratch + 4, s);
  int32_t got = 0;
  hipError_t e = hipSuccess;
  if (rc == MRAG_OK) e = hipMemcpyAsync(&got, scratch, 4, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // before the scratch is freed, on every path
  if (rc != MRAG_OK) return rc;
  MRAG_HIP(e);
  MRAG_HIP(e2);
  *live = got;
  return MRAG_OK;
}
