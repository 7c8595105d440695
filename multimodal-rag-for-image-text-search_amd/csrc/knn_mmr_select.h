// knn_mmr_select.h — the step logic of maximal marginal relevance that needs no
// device: which candidates are valid, the value of a candidate, the tie rule, the padding of a
// short list, and a serial selection built from exactly those pieces. K16 (knn_mmr.hip) calls the
// pieces; scripts/knn_mmr_check.cpp compiles the serial selection for the CPU, where
// tests/test_knn_mmr_cpu.py holds it against the numpy oracle. Plain C++: no HIP header.
//
// Both users compile with -ffp-contract=off: a value is two products and one subtraction, each
// rounded to f64 on its own.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRAG_MMR_HD __host__ __device__
#else
#define MRAG_MMR_HD
#endif

namespace mrag_mmr {

constexpr int MAX_FETCH = 1024;           // MRAG_KNN_MMR_MAX_FETCH: the candidates K16 keeps in LDS
constexpr int32_t NO_POS = 0x7fffffff;    // "no candidate": loses every tie
constexpr double NEG_INF = -__builtin_huge_val();

// A candidate slot takes part when it names a row and has a score: the search marks the slots
// past the matching rows with row -1 and score -inf (a NaN score is no score either).
MRAG_MMR_HD inline bool valid(int64_t row, double s) { return row >= 0 && s > NEG_INF; }

// v = lam * s - (1 - lam) * p, p = the largest cosine to a row selected so far (0 at step 0,
// where nothing is selected yet).
MRAG_MMR_HD inline double value(double lam, double s, double p) {
  const double rel = lam * s;
  const double pen = (1.0 - lam) * p;
  return rel - pen;
}

// Whether (v, pos) beats the best so far: larger v, ties to the smaller candidate position.
MRAG_MMR_HD inline bool better(double v, int32_t pos, double bv, int32_t bpos) {
  return v > bv || (v == bv && pos < bpos);
}

// Output slot t of a query: the selected position and its value, or the padding of a list with
// fewer valid candidates than k (-1 / -inf). out_v may be null.
MRAG_MMR_HD inline void emit(int32_t* out_pos, double* out_v, int t, int32_t pos, double v) {
  const bool none = pos == NO_POS;
  out_pos[t] = none ? -1 : pos;
  if (out_v) out_v[t] = none ? NEG_INF : v;
}

// Step 0 takes the first valid position (position 0 of every list a search returns: its empty
// slots are at the tail). NO_POS when the list has none.
MRAG_MMR_HD inline int32_t first_valid(const int64_t* rows, const double* s, int m) {
  for (int i = 0; i < m; ++i)
    if (valid(rows[i], s[i])) return i;
  return NO_POS;
}

// The whole selection for one query, serially. cos(i, j) is the pairwise score of candidate
// positions i and j. p[m] and taken[m] are scratch. K16 runs the same steps with the loop over i
// spread over a workgroup.
template <class Cos>
MRAG_MMR_HD inline void select_serial(const int64_t* rows, const double* s, int m, int k, double lam, Cos cos,
                                      double* p, unsigned char* taken, int32_t* out_pos, double* out_v) {
  for (int i = 0; i < m; ++i) {
    p[i] = NEG_INF;
    taken[i] = 0;
  }
  int32_t cur = first_valid(rows, s, m);
  double curv = cur == NO_POS ? NEG_INF : value(lam, s[cur], 0.0);
  for (int t = 0; t < k; ++t) {
    emit(out_pos, out_v, t, cur, curv);
    if (cur == NO_POS || t + 1 == k) continue;  // an exhausted list pads; no penalty pass after the last step
    taken[cur] = 1;
    int32_t bpos = NO_POS;
    double bv = NEG_INF;
    for (int i = 0; i < m; ++i) {
      if (taken[i] || !valid(rows[i], s[i])) continue;
      const double c = cos(i, (int)cur);
      if (c > p[i]) p[i] = c;
      const double v = value(lam, s[i], p[i]);
      if (better(v, i, bv, bpos)) {
        bv = v;
        bpos = i;
      }
    }
    cur = bpos;
    curv = bv;
  }
}

}  // namespace mrag_mmr
