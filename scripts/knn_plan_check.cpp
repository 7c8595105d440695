// The kNN search plan (csrc/knn_plan.h) on the CPU, for tests/test_knn_plan_cpu.py: a plan's
// fields as an integer array, and a sweep that checks the conditions the kernels rely on over a
// grid of (rows, queries, k, dim). Test infrastructure: nothing in the library calls it.
//   c++ -std=c++17 -O1 -fPIC -shared -I<pkg>/csrc scripts/knn_plan_check.cpp -o <out>.so
// Stand-alone sweep (e.g. under -fsanitize=address,undefined), exit status 1 on a violation:
//   c++ -std=c++17 -DKNN_PLAN_CHECK_MAIN -I<pkg>/csrc scripts/knn_plan_check.cpp -o scripts/knn_plan_check
#include <cstdint>
#include <cstdio>

#include "knn_plan.h"

using namespace mrag_knn;

namespace {

bool is_pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

const char* const CONDITIONS[] = {
    "ok",
    "fused path for n >= 1, DP <= 512, k <= 256 (v3 iff k <= 64)",
    "1 <= S <= ntiles, S * KL <= 4096, S >= 8 implies S % 8 == 0",
    "Qp >= nq, a whole number of query groups on v3",
    "M <= S * KL; R a power of two >= (S + SX) * KL; Mp a power of two >= max(M, 2)",
    "sel implies M + 1 <= 64 sel and R >= 256 sel",
    "sampled implies v3, qb == 4 and sample_tiles >= 4",
    "counting implies sampled, idbits <= REC_ID_BITS_MAX, 4 max_sample_tiles <= 2^idbits, stride > 1",
    "K8's LDS bytes <= 65536 (the launch sets no larger limit)",
    "per-query labels: K7g where v1's top-k scan has no such instance (k > 64, DP > PQL_V1_MAX_DP), pql set",
};

// 0, or the index in CONDITIONS of the first condition the plan of (n, nq, k, dim) violates
// (labelled: the plan of a search with per-query labels).
int violation(int64_t n, int64_t nq, int k, int dim, bool labelled = false) {
  const int DP = (dim + 127) / 128 * 128;
  const SearchPlan p = labelled ? plan_search(n, nq, k, DP, true) : plan_search(n, nq, k, DP);
  if (p.pql != labelled) return 9;
  if (labelled && k > 64 && DP > PQL_V1_MAX_DP) return p.path == SearchPath::Generic && p.Qp == nq ? 0 : 9;
  const bool v3 = p.path == SearchPath::V3;
  if (!(v3 || p.path == SearchPath::V1) || v3 != (k <= 64)) return 1;
  if (!(1 <= p.S && p.S <= p.ntiles && p.S * p.KL <= MAX_MERGE_ENTRIES && (p.S < 8 || p.S % 8 == 0))) return 2;
  if (!(p.Qp >= nq && (!v3 || (p.Qp % p.qpg == 0 && p.Qp / p.qpg == p.qgroups)))) return 3;
  if (!(p.M <= p.S * p.KL && is_pow2(p.R) && p.R >= (p.S + p.SX) * p.KL && is_pow2(p.Mp) &&
        p.Mp >= std::max(p.M, 2)))
    return 4;
  if (p.sel && !(p.M + 1 <= 64 * p.sel && p.R >= 256 * p.sel)) return 5;
  if (p.sampled && !(v3 && p.qb == 4 && p.sample_tiles >= 4)) return 6;
  if (p.counting && !(p.sampled && p.idbits <= REC_ID_BITS_MAX &&
                      4 * (int64_t)p.max_sample_tiles <= ((int64_t)1 << p.idbits) && p.stride > 1))
    return 7;
  if (p.merge_lds > 65536) return 8;
  return 0;
}

void plan_fields(const SearchPlan& p, int64_t* out) {
  const int64_t f[] = {(int64_t)p.path, p.qb,      p.qpg,          p.Qp,
                       p.qgroups,       p.ntiles,  p.KL,           p.S,
                       p.stride,        p.sampled, p.sample_tiles, p.max_sample_tiles,
                       p.idbits,        p.counting, p.SX,          p.rec_keep,
                       p.skip_magic,    p.M,       p.R,            p.Mp,
                       p.sel,           (int64_t)p.merge_lds};
  for (int i = 0; i < (int)(sizeof(f) / sizeof(f[0])); ++i) out[i] = f[i];
}

// knn_plan_sweep's grid over the plans of unlabelled or labelled searches.
int64_t sweep(bool labelled, int64_t* out) {
  const int64_t ns[] = {1,      63,     64,      65,      4095,    4096,    5000,   100000,
                        262143, 262144, 270000, 1 << 20, 1 << 24, 1 << 26, 1 << 30};
  const int64_t nqs[] = {1, 31, 32, 33, 64, 65, 255, 256, 257, 1000, 4096, 65536, (1 << 24) - 1};
  const int ks[] = {1, 8, 9, 16, 17, 32, 33, 64, 65, 100, 256};
  const int dims[] = {1, 100, 128, 129, 256, 384, 512};
  int64_t points = 0, bad = 0, max_lds = 0;
  for (int64_t n : ns)
    for (int64_t nq : nqs)
      for (int k : ks)
        for (int dim : dims) {
          ++points;
          const int DP = (dim + 127) / 128 * 128;
          const SearchPlan p = labelled ? plan_search(n, nq, k, DP, true) : plan_search(n, nq, k, DP);
          max_lds = std::max<int64_t>(max_lds, (int64_t)p.merge_lds);
          const int v = violation(n, nq, k, dim, labelled);
          if (v && bad++ == 0) {
            out[2] = n;
            out[3] = nq;
            out[4] = k;
            out[5] = dim;
            out[6] = v;
          }
        }
  out[0] = points;
  out[1] = max_lds;
  return bad;
}

}  // namespace

extern "C" {

const char* knn_plan_field_names() {
  return "path,qb,qpg,Qp,qgroups,ntiles,KL,S,stride,sampled,sample_tiles,max_sample_tiles,idbits,counting,SX,"
         "rec_keep,skip_magic,M,R,Mp,sel,merge_lds";
}

// The plan of (n, nq, k, DP), in the order of knn_plan_field_names(); path as in SearchPath.
void knn_plan_fields(int64_t n, int64_t nq, int k, int DP, int64_t* out) {
  plan_fields(plan_search(n, nq, k, DP), out);
}

// The plan with plan_search's last argument given: the fields of knn_plan_field_names(), then
// SearchPlan::pql (per_query_labels != 0: a search with one label filter per query).
void knn_plan_fields_labels(int64_t n, int64_t nq, int k, int DP, int per_query_labels, int64_t* out) {
  const SearchPlan p = plan_search(n, nq, k, DP, per_query_labels != 0);
  plan_fields(p, out);
  out[22] = p.pql;
}

// The collect stage's plan for `uncertified` failing queries of that search: cgroups, Sc, ccap.
void knn_plan_collect_fields(int64_t uncertified, int64_t n, int64_t nq, int k, int DP, int64_t* out) {
  const CollectPlan c = plan_collect(uncertified, plan_search(n, nq, k, DP));
  out[0] = c.cgroups;
  out[1] = c.Sc;
  out[2] = c.ccap;
}

const char* knn_plan_condition(int i) { return CONDITIONS[i]; }

// Checks every point of the grid; returns the number of violating points. out[0] = points,
// out[1] = largest K8 LDS figure, out[2..6] = n, nq, k, dim and condition of the first violation.
int64_t knn_plan_sweep(int64_t* out) { return sweep(false, out); }

// The same grid and conditions over the plans of searches with per-query labels.
int64_t knn_plan_sweep_labels(int64_t* out) { return sweep(true, out); }

}  // extern "C"

#ifdef KNN_PLAN_CHECK_MAIN
int main() {
  int64_t out[7] = {0, 0, 0, 0, 0, 0, 0};
  const int64_t bad = knn_plan_sweep(out);
  std::printf("%lld points, %lld violations, largest K8 LDS %lld bytes\n", (long long)out[0], (long long)bad,
              (long long)out[1]);
  if (bad)
    std::printf("first: n=%lld nq=%lld k=%lld dim=%lld: %s\n", (long long)out[2], (long long)out[3],
                (long long)out[4], (long long)out[5], CONDITIONS[out[6]]);
  return bad ? 1 : 0;
}
#endif
