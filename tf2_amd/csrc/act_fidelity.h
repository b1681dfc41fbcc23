// act_fidelity.h -- layer fidelity behind tf2_fid_* (include/tf2_amd.h): the handle (host) and the argument blocks of its kernels
// (act_fidelity.hip).  tf2_amd/fidelity.py states the comparison (reference_compare); the device store equals it as integers.
//
// The budget of a record (fixed point, 8 fractional bits of an int8 LSB): |256 v| <= 2^15, |e| <= 2^16, so |d| = |256 v - e| < 2^17 and
// d^2 < 2^34: sum_d2 holds 2^63 / 2^34 = 2^29 values a channel even if every value were wrong by the full range (e^2 <= 2^32 and
// (256 v)^2 <= 2^30 hold more).  Inside a block a thread sees at most kFidSlab / 4 = 256 values (kFidImgSlab / 256 = 64 in the input
// kernel), a block kFidSlab a channel: every partial sum but sum_d2 and sum_e2 fits 32 bits (sum_abs_d < 2^10 * 2^17), and the seven
// 9-bit fields of a thread's packed histogram hold 511 each.
#pragma once
#include <cstddef>
#include "act_rows.h"

namespace tf2 {

constexpr int kFidSlots = 18;            // int64 words of a channel's record (tf2_amd.h: n, nonfinite, ref_clamped, max_abs_d, sum_d, sum_abs_d, sum_d2, sum_abs_e, sum_e2, sum_q2, hist[8])
constexpr int kFidFrac = 8;              // fractional bits of the fixed point: e = rint(f * 2^(Q + 8)), d = 256 v - e
constexpr int kFidSlab = 1024;           // pixels of an NHWC tensor one block walks
constexpr int kFidChans = 64;            // channels of a block: one a lane
constexpr int kFidTile = 64;             // pixels of the float tile a block transposes through LDS at a time
constexpr int kFidImgSlab = 16384;       // values of one image plane a block of the input kernel walks
constexpr int kFidRowsPerLaunch = 64;    // table rows one launch takes (its row table travels in the kernel arguments)

// One table row of a launch: the NHWC int8 slice [npix][cp] from `base` (the slice's first channel) against the dense NCHW float32
// reference `ref` [npix / hw][c][hw].
struct FidRow {
  const int8_t* base;
  const uint8_t* dbl;        // [c] in the packed image: 1 = the channel holds 2y - 128 (null: no such channel)
  const float* ref;
  int32_t npix, c, cp, hw;
  int32_t block0;            // first block of the row in the launch's grid
  int32_t rec0;              // the row's first record (store and scale table)
};
struct FidRowsArgs {
  FidRow rows[kFidRowsPerLaunch];
  long long* store;
  const float* scales;       // [records]: 2^(Q + 8) of every channel
  int32_t n_rows;
};
static_assert(sizeof(FidRow) == 48 && offsetof(FidRowsArgs, store) == 3072 && offsetof(FidRowsArgs, scales) == 3080 &&
              offsetof(FidRowsArgs, n_rows) == 3088 && sizeof(FidRowsArgs) == 3096, "the kernel's argument layout");

// The input record: dense NCHW float32 images against their own quantisation (quant_input with trans = 2^Q0).
struct FidImgArgs {
  const float* images;
  long long* store;          // record 0
  float trans, scale;        // 2^Q0, 2^(Q0 + 8)
  int32_t c, hw, planes;     // planes = batch * c
  int32_t slabs;             // blocks a plane
};
static_assert(offsetof(FidImgArgs, store) == 8 && offsetof(FidImgArgs, slabs) == 36 && sizeof(FidImgArgs) == 40, "the kernel's argument layout");

struct Comparator {
  ActRows g;                 // the rows and their records (act_rows.h)
  std::vector<float> scale;  // [records]: 2^(Q + 8); a pooling row's Q is its source's (the runtime table already says so)

  tf2_status create(Net* n);
  size_t store_size() const { return g.store_size(kFidSlots); }
  size_t workspace_size(int batch) { return g.workspace_size(batch); }
  tf2_status store_init(void* store, size_t store_bytes, void* stream) const;
  tf2_status run(const void* images, bool images_are_q, int batch, void* ws, size_t ws_bytes, int8_t* logits, void* store,
                 size_t store_bytes, const float* const* refs, const float* scales_dev, void* stream, bool with_step = true);
};

}  // namespace tf2
