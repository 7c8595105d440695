// knn_mmr.hip — K16: diverse top-k by maximal marginal relevance.
//
// One 256-thread workgroup per query selects k of its m <= 1024 candidates greedily. The
// candidates' scores, their running penalty p (the largest cosine to a selected row) and their
// rows live in LDS. Per step the row selected last is staged into LDS as f32, and each aligned
// 16-lane group computes its exact f64 cosine to one unselected candidate (exact_cosine16, the
// routine the search rescored them with: the staged row in the query role), 16 candidates per
// pass, updates p and evaluates v (knn_mmr_select.h). A block arg-max on (v descending, position
// ascending) names the next row. Built with -ffp-contract=off: v is two products and one
// subtraction.
#include "knn_mmr.h"

#include "knn_generic.h"

namespace mrag_knn {

namespace {

constexpr int MMR_THREADS = 256;
constexpr int MMR_WAVES = MMR_THREADS / 64;

// LDS of one workgroup: s[mp] and p[mp] (f64), the staged row (DP f32), rows[mp] (int32) and the
// arg-max's per-wave results; every offset a multiple of 16 (mp is a multiple of 4).
__host__ __device__ inline int mmr_mp(int m) { return (m + 3) & ~3; }
__host__ __device__ inline size_t mmr_lds_bytes(int m, int DP) {
  return (size_t)mmr_mp(m) * 20 + (size_t)DP * 4 + MMR_WAVES * 8 + 16;
}

// The best (v, pos) of the workgroup on every thread. On entry the 16 lanes of a group agree.
__device__ __forceinline__ void block_argmax(double& bv, int32_t& bp, double* red_v, int32_t* red_p, int tid) {
#pragma unroll
  for (int off = 16; off < 64; off <<= 1) {
    const double ov = __shfl_xor(bv, off);
    const int32_t op = __shfl_xor(bp, off);
    if (mrag_mmr::better(ov, op, bv, bp)) {
      bv = ov;
      bp = op;
    }
  }
  if ((tid & 63) == 0) {
    red_v[tid >> 6] = bv;
    red_p[tid >> 6] = bp;
  }
  __syncthreads();
  bv = red_v[0];
  bp = red_p[0];
#pragma unroll
  for (int w = 1; w < MMR_WAVES; ++w) {
    const double ov = red_v[w];
    const int32_t op = red_p[w];
    if (mrag_mmr::better(ov, op, bv, bp)) {
      bv = ov;
      bp = op;
    }
  }
}

__global__ __launch_bounds__(MMR_THREADS) void knn_mmr_kernel(MmrSelect a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int m = a.m, k = a.k, mp = mmr_mp(m);
  double* s = (double*)smem;
  double* p = s + mp;
  float* xs = (float*)(p + mp);
  int32_t* rows = (int32_t*)(xs + a.DP);
  double* red_v = (double*)(rows + mp);
  int32_t* red_p = (int32_t*)(red_v + MMR_WAVES);

  const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;
  const int64_t q = blockIdx.x;
  const int64_t* crow = a.cand_rows + q * m;
  const double* cs = a.cand_s64 + q * m;
  int32_t* opos = a.out_pos + q * k;
  double* ov = a.out_v ? a.out_v + q * k : nullptr;

  // the candidates; step 0's arg-max is over a constant, so it finds the first valid position
  double bv = mrag_mmr::NEG_INF;
  int32_t bp = mrag_mmr::NO_POS;
  for (int i = tid; i < m; i += MMR_THREADS) {
    const int64_t r = crow[i];
    const double sc = cs[i];
    bool ok = mrag_mmr::valid(r, sc);
    if (ok && r >= a.n) {  // never read: the entry point reports it
      ok = false;
      if (a.bad_row) *a.bad_row = 1;
    }
    rows[i] = ok ? (int32_t)r : -1;
    s[i] = sc;
    p[i] = mrag_mmr::NEG_INF;
    if (ok && mrag_mmr::better(0.0, i, bv, bp)) {
      bv = 0.0;
      bp = i;
    }
  }
  // the lanes of a group hold different positions here: agree within the group first
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
    const double v2 = __shfl_xor(bv, off);
    const int32_t p2 = __shfl_xor(bp, off);
    if (mrag_mmr::better(v2, p2, bv, bp)) {
      bv = v2;
      bp = p2;
    }
  }
  block_argmax(bv, bp, red_v, red_p, tid);  // its barrier also publishes s, p and rows
  int32_t cur = bp;
  double curv = cur == mrag_mmr::NO_POS ? mrag_mmr::NEG_INF : mrag_mmr::value(a.lam, s[cur], 0.0);

  for (int t = 0; t < k; ++t) {
    if (tid == 0) mrag_mmr::emit(opos, ov, t, cur, curv);
    if (cur == mrag_mmr::NO_POS || t + 1 == k) continue;  // uniform: cur comes from LDS
    const int32_t srow = rows[cur];
    __syncthreads();  // every thread has srow (and last step's arg-max results) before they change
    if (tid == 0) rows[cur] = -1;  // taken
    {
      const f32x4* src = (const f32x4*)(a.x32 + (size_t)srow * a.DP);
      f32x4* dst = (f32x4*)xs;
      for (int c = tid; c < (a.DP >> 2); c += MMR_THREADS) dst[c] = src[c];
    }
    const double sn = a.xn[srow];
    __syncthreads();
    bv = mrag_mmr::NEG_INF;
    bp = mrag_mmr::NO_POS;
    for (int i = grp; i < m; i += MMR_THREADS / 16) {
      const int32_t r = rows[i];
      if (r < 0) continue;  // the whole group skips
      const double c = exact_cosine16(xs, sn, a.x32, a.xn, r, a.D, a.DP, sub);
      double pi = p[i];
      if (c > pi) {
        pi = c;
        if (sub == 0) p[i] = pi;  // read again by this group only, a step later
      }
      const double v = mrag_mmr::value(a.lam, s[i], pi);
      if (mrag_mmr::better(v, i, bv, bp)) {
        bv = v;
        bp = i;
      }
    }
    block_argmax(bv, bp, red_v, red_p, tid);
    cur = bp;
    curv = bv;
  }
}

__global__ __launch_bounds__(256) void knn_mmr_gather_kernel(MmrGather g) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= g.nq * g.k) return;
  const int64_t q = o / g.k;
  const int32_t pos = g.pos[o];
  const bool has = pos >= 0 && pos < g.m;
  const int64_t src = q * g.m + (has ? pos : 0);
  const int64_t r = has ? g.cand_rows[src] : -1;
  g.out_s[o] = has ? g.cand_s[src] : -INFINITY;
  if (g.out_s64) g.out_s64[o] = has ? g.cand_s64[src] : -INFINITY;
  g.out_r[o] = r >= 0 ? r + g.row_offset : -1;
}

}  // namespace

int mmr_select(const MmrSelect& a, hipStream_t s) {
  if (a.nq <= 0) return MRAG_OK;
  if (a.m < 1 || a.m > mrag_mmr::MAX_FETCH || a.k < 1 || a.k > a.m || a.DP < a.D || (a.DP & 3))
    return mrag::fail(MRAG_ERR_ARG, "K16: bad shape m=%d k=%d D=%d DP=%d", a.m, a.k, a.D, a.DP);
  const size_t lds = mmr_lds_bytes(a.m, a.DP);  // <= 36.9 KB at m = 1024, DP = 4096
  hipLaunchKernelGGL(knn_mmr_kernel, dim3((unsigned)a.nq), dim3(MMR_THREADS), lds, s, a);
  MRAG_CHECK_LAUNCH();
  return MRAG_OK;
}

int mmr_gather(const MmrGather& g, hipStream_t s) {
  const int64_t n = g.nq * g.k;
  if (n <= 0) return MRAG_OK;
  hipLaunchKernelGGL(knn_mmr_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g);
  MRAG_CHECK_LAUNCH();
  return MRAG_OK;
}

}  // namespace mrag_knn
