// The MMR step logic (csrc/knn_mmr_select.h) on the CPU, for tests/test_knn_mmr_cpu.py: the serial
// selection over a table of scores and pairwise cosines the caller supplies. Test infrastructure:
// nothing in the library calls it.
//   c++ -std=c++17 -O1 -ffp-contract=off -fPIC -shared -I<pkg>/csrc scripts/knn_mmr_check.cpp -o <out>.so
// Stand-alone self-check (e.g. under -fsanitize=address,undefined), exit status 1 on a failure:
//   c++ -std=c++17 -ffp-contract=off -DKNN_MMR_CHECK_MAIN -I<pkg>/csrc scripts/knn_mmr_check.cpp -o scripts/knn_mmr_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "knn_mmr_select.h"

extern "C" {

int knn_mmr_max_fetch() { return mrag_mmr::MAX_FETCH; }

// One query: rows[m] (-1: empty slot), s[m], c[m][m] (the pairwise scores, row-major), k <= m.
// out_pos[k], out_v[k] (may be null). Returns 0, or 1 on a bad shape.
int knn_mmr_check_select(const int64_t* rows, const double* s, const double* c, int m, int k, double lam,
                         int32_t* out_pos, double* out_v) {
  if (m < 1 || k < 1 || k > m) return 1;
  std::vector<double> p((size_t)m);
  std::vector<unsigned char> taken((size_t)m);
  mrag_mmr::select_serial(
      rows, s, m, k, lam, [c, m](int i, int j) { return c[(size_t)i * m + j]; }, p.data(), taken.data(), out_pos,
      out_v);
  return 0;
}

double knn_mmr_value(double lam, double s, double p) { return mrag_mmr::value(lam, s, p); }

int knn_mmr_valid(int64_t row, double s) { return mrag_mmr::valid(row, s) ? 1 : 0; }

int knn_mmr_better(double v, int32_t pos, double bv, int32_t bpos) { return mrag_mmr::better(v, pos, bv, bpos) ? 1 : 0; }

}  // extern "C"

#ifdef KNN_MMR_CHECK_MAIN
int main() {
  int bad = 0;
  // three candidates, 1 a copy of 0: at lam = 0.5 the copy goes last; the fourth slot is empty
  const int64_t rows[4] = {10, 11, 12, -1};
  const double s[4] = {0.9, 0.9, 0.5, -__builtin_huge_val()};
  const double c[16] = {1, 1, 0.1, 0, 1, 1, 0.1, 0, 0.1, 0.1, 1, 0, 0, 0, 0, 1};
  int32_t pos[4];
  double v[4];
  bad += knn_mmr_check_select(rows, s, c, 4, 4, 0.5, pos, v);
  bad += !(pos[0] == 0 && pos[1] == 2 && pos[2] == 1 && pos[3] == -1);
  bad += !(v[0] == 0.45 && v[3] == -__builtin_huge_val());
  bad += knn_mmr_check_select(rows, s, c, 4, 3, 1.0, pos, v);
  bad += !(pos[0] == 0 && pos[1] == 1 && pos[2] == 2);
  const int64_t none[2] = {-1, -1};
  bad += knn_mmr_check_select(none, s, c, 2, 2, 0.5, pos, nullptr);
  bad += !(pos[0] == -1 && pos[1] == -1);
  std::printf("%d failures\n", bad);
  return bad ? 1 : 0;
}
#endif
