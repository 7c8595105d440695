// knn_mmr.h — K16: greedy maximal-marginal-relevance selection among the candidates of a search
// (DESIGN.md §3.5), and the gather of the selected slots into a search's output layout. The
// step logic is knn_mmr_select.h; the entry points are in knn.hip (mrag_knn_mmr_select,
// mrag_knn_search_mmr).
#pragma once

#include "common.h"
#include "knn_mmr_select.h"

namespace mrag_knn {

struct MmrSelect {
  // corpus (the index's buffers)
  const float* x32;
  const double* xn;
  int64_t n;  // rows handed out: a candidate row >= n is refused
  int D, DP;
  // candidates (device): [nq][m] local row ids (-1: empty slot) and their exact f64 scores
  const int64_t* cand_rows;
  const double* cand_s64;
  int64_t nq;
  int m, k;  // 1 <= k <= m <= mrag_mmr::MAX_FETCH
  double lam;
  // outputs (device): [nq][k] candidate positions in selection order (-1 past the valid
  // candidates) and, when not null, the value each was selected with (-inf there)
  int32_t* out_pos;
  double* out_v;
  int32_t* bad_row;  // device word, or null: set to 1 when a candidate row >= n is met (the slot counts as empty)
};

// K16: one 256-thread workgroup per query. Launch only.
int mmr_select(const MmrSelect& a, hipStream_t s);

struct MmrGather {
  const int32_t* pos;  // [nq][k], K16's output
  // the candidates' search output [nq][m]
  const float* cand_s;
  const double* cand_s64;
  const int64_t* cand_rows;  // local row ids
  int64_t nq;
  int m, k;
  int64_t row_offset;
  // [nq][k]: slot t = the candidate at pos[t] (row + row_offset), or -inf / -1
  float* out_s;
  double* out_s64;  // may be null
  int64_t* out_r;
};

int mmr_gather(const MmrGather& g, hipStream_t s);

}  // namespace mrag_knn
