// embed_roc.h -- match-threshold calibration behind tf2_emb_roc_* (include/tf2_amd.h): the constants the two kernels (embed_roc.hip)
// share with the host checks and with tf2_amd/embed.py, and the two enqueue calls.  They belong to no handle.
#pragma once
#include "tf2_net.h"
#include "embed_match.h"

namespace tf2 {

constexpr int kRocMaxThr = 4096;     // thresholds of a grid: the block-local histogram is 2 x (n_thr + 1) words of LDS
constexpr int kRocMaxFolds = 16;     // folds of a listed-pairs protocol
constexpr int kRocSub = 64;          // rows of a sub-tile: one A row a lane, 4 waves x 16 B rows
constexpr int kRocTile = 256;        // rows of a block's tile on either side: kRocTile / kRocSub squared sub-tile pairs a block

tf2_status emb_roc_hist(const float* rows_a, const int32_t* ids_a, int n_a, const float* rows_b, const int32_t* ids_b, int n_b, int d,
                        int n_thr, float step, int64_t* hist, void* stream);
tf2_status emb_roc_pairs(const float* rows, int n_rows, int d, const int32_t* pairs, int n_pairs, int n_folds, int n_thr, float step,
                         float* dist, int64_t* hist, int64_t* invalid, void* stream);

}  // namespace tf2
