// knn_compact.h — K15: the two kernels behind mrag_knn_compact (knn.hip): the row remap (an
// exclusive prefix sum over the live flags) and the gather of the live rows into new buffers.
#pragma once

#include "common.h"

namespace mrag_knn {

constexpr int REMAP_BLOCK = 4096;  // labels per workgroup of K15a (256 threads x 4 x int4)

// int32 words of scratch that row_remap needs for n labels: per level of the recursion the
// block sums and their scan, each padded to 4 words (16-byte loads).
size_t remap_scratch_words(int64_t n);

// K15a. labels int32 [n] -> remap int32 [n]: the number of live rows (label !=
// MRAG_LABEL_DELETED) before r for a live r, -1 for a deleted one; *live_dev (device int32)
// gets the live count. Launches only: reduce per block, scan of the block sums (recursing, so
// any n < 2^31 is covered), scan per block and write. labels, remap and scratch 16-byte aligned.
int row_remap(const int32_t* labels, int64_t n, int32_t* remap, int32_t* live_dev, int32_t* scratch,
              hipStream_t s);

struct GatherRows {
  const _Float16* x16;
  const float* x32;
  const double* xn;
  const int32_t* labels;
  const int32_t* remap;  // K15a's output
  int64_t n;
  int DP;  // a multiple of 128
  _Float16* out_x16;
  float* out_x32;
  double* out_xn;
  int32_t* out_labels;
};

// K15b. Copies every live row r (remap[r] >= 0) to row remap[r] of the out buffers.
int gather_rows(const GatherRows& g, hipStream_t s);

}  // namespace mrag_knn
