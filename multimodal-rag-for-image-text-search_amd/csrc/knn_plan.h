// knn_plan.h — the shape of one fused kNN search (knn.hip K7/K8/K7c/K10), decided on the host from
// (rows, queries, k, padded width) alone: which scan runs, its grid, whether the sample pass
// runs and in which form, and the sizes K8 works with. Plain C++ (no HIP), so the policy can be
// compiled and checked without a GPU (scripts/knn_plan_check.cpp, tests/test_knn_plan_cpu.py).
// knn.hip's kernels read the constants below; its host code sizes buffers, fills the kernel
// parameters and picks the kernel instances from a SearchPlan and decides nothing itself.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace mrag_knn {

constexpr int TILE_ROWS = 64;
constexpr int QPW = 32;                  // v1: queries per wave (MFMA 32x32 N dim)
constexpr int QPG = 8 * QPW;             // v1 / K7c: queries per workgroup (8 waves)
constexpr int MAX_MERGE_ENTRIES = 4096;  // splits * KL cap (LDS sort in K8)
constexpr int MAX_K = 256;               // deepest k of the fused scan (K7g above)
constexpr int MAX_DP = 512;              // widest padded row of the fused scan (K7g above)
constexpr int PQL_V1_MAX_DP = 256;       // per-query labels: widest row of v1's top-k scan (K7g above)
#ifndef MRAG_SAMPLE_STRIDE
#define MRAG_SAMPLE_STRIDE 16
#endif
constexpr int SAMPLE_STRIDE = MRAG_SAMPLE_STRIDE;  // K7 sample pre-pass: every 16th tile of a split (A/B builds: -D)
constexpr int XLISTS = 4;            // extra 8-entry lists per query for the counting pass's rows
constexpr int REC_ID_BITS_MAX = 10;  // id field of a packed record entry (qrec packs beside it)

enum class SearchPath : int {
  Empty = 0,    // no rows: the outputs are filled with -inf / -1
  Generic = 1,  // K7g (knn_generic.hip): widths and depths the fused scan does not instantiate
  V1 = 2,       // MFMA 32x32, per-lane lists of KL = 8 / 16 / 32
  V3 = 3,       // MFMA 16x16x32, per-lane lists of 6 folded to 8 per split
};

struct SearchPlan {
  SearchPath path;
  // scan grid: qgroups x S workgroups, split s owns tiles s, s + S, ...
  int qb;       // v3: 16-query blocks per wave, 1 (K7s, 64 queries per workgroup) or 4 (256)
  int qpg;      // queries per scan workgroup
  int64_t Qp;   // query slots (padded)
  int qgroups;  // query groups
  int ntiles;   // corpus tiles of TILE_ROWS rows
  int KL;       // entries per (query, split) list
  int S;        // splits
  // sample pass
  int stride;            // every stride-th tile of a split is a sample tile
  bool sampled;          // the sample pass runs
  int sample_tiles;      // seed-only pass: tiles it reads per split (0 when not sampled)
  int max_sample_tiles;  // sample tiles of the longest split
  int idbits;            // bits of a record entry's group id (4 groups per sample tile)
  bool counting;         // the pass is the counting one: its tiles are skipped by the main scan
  int SX;                // extra lists per query that carry the counting pass's rows to K8
  uint32_t rec_keep;     // counting: mask that clears the id bits of a record entry
  uint32_t skip_magic;   // counting: 2^32 / (stride - 1) rounded up (ScanParams), else 0
  // K8
  int M;             // candidates rescored exactly
  int R;             // sort width: a power of two >= (S + SX) * KL, widened for the fold
  int Mp;            // M rounded up to a power of two
  int sel;           // key selection: register top-64 (1) / top-128 (2) fold, or 0 = bitonic sort
  size_t merge_lds;  // dynamic LDS bytes of the K8 launch
  // per-query labels (mrag_knn_search_labels): the scan, sample, resolve, K7c and K7g kernels run
  // as their PQL instances, which mask rows per query; every other field is what the unlabelled
  // search of the same shape gets
  bool pql;
};

inline int64_t next_pow2(int64_t x) {
  int64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// v1's per-lane list depth: >= k where registers allow (DP/4 VGPRs hold the query fragments;
// deeper lists keep 2*KL more VGPRs live next to them, so KL is capped where it would spill;
// the certificate stays exact either way).
inline int kl_for(int k, int DP) {
  if (k <= 8 || DP >= 512) return 8;
  if (k <= 16 || DP >= 256) return 16;
  return 32;
}

// Query blocks per wave of the v3 scan for a batch: 1 (K7s, 64 queries per workgroup) while the
// batch fits one small group, else 4 (256 per workgroup).
inline int scan3_qb(int64_t nq) { return nq <= 64 ? 1 : 4; }

// Sample pre-pass stride for k: the main scan's fires grow with the rows above the seed, about
// k x stride, so k > 16 samples every 4th tile (512k x 512, k = 50: search 0.824 -> 0.736 ms,
// scan 0.659 -> 0.501; stride 8: 0.748; notes/knn_scan_experiments.md).
inline int sample_stride_for(int k) { return k > 16 ? 4 : SAMPLE_STRIDE; }

// k <= 16: the counting sample pass (MODE 2 + sample_resolve_kernel) takes its tiles for good and
// the main scan skips them; k > 16 keeps the seed-only pass over every 4th tile and a main scan
// over all tiles (the rows above its seed, about k x stride, would not fit the extra lists).
inline bool counting_sample_for(int k) { return k <= 16; }

// The plan of a search of nq >= 1 queries for the k best of n rows of padded width DP;
// per_query_labels: every query carries its own label filter. The PQL instances of the v3 scan
// (every DP, QB and MODE), of the resolve kernel and of K7c build without scratch (DESIGN.md §4
// "Kernel resources"), so a labelled search keeps the geometry, the sample pass and K8's sizes of
// the unlabelled one. The one exception is v1's top-k scan (k > 64) at DP = 384 and 512: with the
// lane's filter next to its lists and query fragments it needs 60 / 68 bytes of scratch per lane,
// so labelled searches of those shapes take K7g, which filters per query at no register cost.
inline SearchPlan plan_search(int64_t n, int64_t nq, int k, int DP, bool per_query_labels = false) {
  SearchPlan p{};
  p.pql = per_query_labels;
  if (n == 0) {
    p.path = SearchPath::Empty;
    return p;
  }
  if (DP > MAX_DP || k > MAX_K || (per_query_labels && k > 64 && DP > PQL_V1_MAX_DP)) {
    p.path = SearchPath::Generic;
    p.Qp = nq;  // K7g pads nothing
    return p;
  }
  // v3 (MFMA 16x16x32, 64 queries per wave, per-lane lists of 6 folded to 8 per split) unless
  // k is deep enough to want longer per-lane lists (v1). For 32 < k <= 64 the union of the S
  // split lists still holds S * 8 >= k + 32 candidates at the batch sizes that matter, and the
  // certificate sends any query whose top-k a list could not hold to the collect pass.
  const bool v3 = k <= 64;
  p.path = v3 ? SearchPath::V3 : SearchPath::V1;
  p.qb = v3 ? scan3_qb(nq) : 4;
  p.qpg = v3 ? 64 * p.qb : QPG;
  // query slots: v3 reads every slot of its query group (no lane guard), so pad to a whole
  // group; padding rows are zero (prep) and never reach the output
  const int64_t qpad = v3 ? p.qpg : QPW;
  p.Qp = (nq + qpad - 1) / qpad * qpad;
  p.qgroups = (int)((p.Qp + p.qpg - 1) / p.qpg);
  p.ntiles = (int)((n + TILE_ROWS - 1) / TILE_ROWS);
  p.KL = v3 ? 8 : kl_for(k, DP);
  // about 256 scan workgroups, at most one split per tile, and a union K8 can sort in LDS
  p.S = std::max(1, 256 / p.qgroups);
  p.S = std::min(p.S, p.ntiles);
  p.S = std::min(p.S, MAX_MERGE_ENTRIES / p.KL);
  if (p.S >= 8) p.S &= ~7;

  // Sample pass (v3, 256-query groups, when every split has >= 4 * stride tiles): seeds the
  // shared threshold near the k-th best so the main scan's list insertions stay rare. Four
  // maxima per (split, query), one per lane group (merging them in pairs, the round-1 seed,
  // measured 0.2 % slower in the main scan); stride 16 (32: +5 %, 64: +14 %, none: +70 % scan
  // time). K7s (qb == 1) streams at the HBM rate, where the pre-pass costs more than the
  // inserts it saves (Q = 1: 0.270 -> 0.247 ms without it, notes/knn_scan_experiments.md).
  // The counting pass (k <= 16, while the group ids fit the record) keeps a per-lane record
  // instead of the maxima; the resolve kernel seeds the threshold from it and lists the sampled
  // rows above the seed in XLISTS extra lists, and the main scan walks the other tiles only.
  const int min_tiles = p.ntiles / p.S;
  p.stride = sample_stride_for(k);  // the main scan reads it too (skip_sampled)
  p.sampled = v3 && p.qb == 4 && min_tiles >= 4 * p.stride;
  p.sample_tiles = p.sampled ? min_tiles / p.stride : 0;
  p.max_sample_tiles = ((p.ntiles + p.S - 1) / p.S + p.stride - 1) / p.stride;
  p.idbits = 2;
  while ((1 << p.idbits) < 4 * p.max_sample_tiles) ++p.idbits;
  p.counting = p.sampled && counting_sample_for(k) && p.idbits <= REC_ID_BITS_MAX;
  p.SX = p.counting ? XLISTS : 0;
  if (p.counting) {
    p.rec_keep = ~((1u << p.idbits) - 1u);
    p.skip_magic = (uint32_t)((1ull << 32) / (uint64_t)(p.stride - 1) + 1);
  }

  p.M = std::min<int>(k + 32, p.S * p.KL);
  p.Mp = (int)next_pow2(std::max(p.M, 2));
  // K8 key selection: the best M + 1 keys (the M candidates and the first one left out) by
  // the register top-64P fold when they fit, else the full bitonic sort (40.6 -> 36.5 us per
  // 1000-query search for the fold); the fold parks four waves' top-64P in keys[], so R is at
  // least that wide
  p.sel = p.M + 1 <= 64 ? 1 : (p.M + 1 <= 128 ? 2 : 0);
  p.R = (int)next_pow2((int64_t)(p.S + p.SX) * p.KL);
  if (p.sel) p.R = std::max(p.R, 4 * 64 * p.sel);
  p.merge_lds = (size_t)p.R * 8 + (size_t)p.Mp * 12 + (size_t)DP * 4 + 64;
  return p;
}

// The collect stage (K7c + K10), planned once K8 has counted the uncertified queries.
struct CollectPlan {
  int cgroups;  // groups of QPG failing queries
  int Sc;       // K7c's splits
  int ccap;     // collected rows per query slot
};

inline CollectPlan plan_collect(int64_t uncertified, const SearchPlan& p) {
  CollectPlan c{};
  // per-slot collect capacity: at most 4096 rows and 64M slots in all; a query that collects
  // more (a run of more than ccap near-duplicates within eps of its k-th score) sends the batch
  // to K7g, whose per-query storage is sized from a histogram — nothing grows across searches
  c.ccap = (int)std::max<int64_t>(256, std::min<int64_t>(4096, ((int64_t)64 << 20) / p.Qp));
  // K7c's grid is sized to the failing queries alone: QPG of them per workgroup, about 1024
  // workgroups in all, so more splits than the main scan (one failing query over the main
  // scan's 64 splits is one 8-wave workgroup per split, latency-bound on its own LDS-DMA round
  // trips: 0.3 ms over 512k rows, notes/knn_scan_experiments.md)
  c.cgroups = (int)((uncertified + QPG - 1) / QPG);
  c.Sc = std::max(p.S, 1024 / c.cgroups);
  c.Sc = std::min(c.Sc, p.ntiles);
  if (c.Sc >= 8) c.Sc &= ~7;
  return c;
}

}  // namespace mrag_knn
