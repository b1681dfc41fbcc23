// act_caq.h -- CAQ calibration behind tf2_caq_* (include/tf2_amd.h): the records and the argument block of the two kernels
// (act_caq.hip).  tf2_amd/caq.py states both passes (reference_range / reference_error); the device stores equal it as integers.
//
// The budget of the ERROR record (fixed point, 7 fractional bits of an int8 LSB at the base exponent Qb): |e| <= 2^18, and for every
// candidate the clamped reconstruction |v << s| <= 128 * 2^7 = 2^14, so |d| < 2^18 + 2^14 and d^2 < 2^37: a sum_d2 slot holds
// 2^63 / 2^37 = 2^26 values a channel even if every value were wrong by the full range (e^2 <= 2^36 holds more).  Inside a block a lane
// sees at most 2^10 values (a 64th of kCaqSlab / 4 where every lane has four values a pass, a few times that where planes are short):
// its 64-bit sums stay below 2^47, its 32-bit counts below 2^10.
// Denormals: the kernels read the maps as 32-bit patterns.  The RANGE pass counts a denormal as the value it is (non-zero, its bin
// clamps to fit = 31) whatever the flush mode.  In the ERROR pass, with |Qb| <= 64 the scale is at most 2^71: a denormal input
// (< 2^-126) or a denormal product gives |t| < 0.5 and e = 0 whether the multiplication flushes or not.
#pragma once
#include <cstddef>
#include "act_rows.h"

namespace tf2 {

constexpr int kCaqRangeSlots = 70;       // int64 words of a channel's RANGE record (tf2_amd.h: n, nonfinite, zeros, negatives, peak_pos, peak_neg, hist[64])
constexpr int kCaqErrorSlots = 12;       // int64 words of a channel's ERROR record (n, nonfinite, ref_clamped, sum_e2, clipped[4], sum_d2[4])
constexpr int kCaqBins = 64;             // hist[b], b = clamp(fit, -32, 31) + 32
constexpr int kCaqFrac = 7;              // fractional bits of the ERROR pass: e = rint(f * 2^(Qb + 7))
constexpr int kCaqCands = 4;             // candidates Q = Qb + j, j = 0 .. 3
constexpr int kCaqELimit = 1 << 18;      // |e| <= 2^18
constexpr int kCaqSlab = 32768;          // values of one channel (over all images, in (b, i) order) one block walks, a quarter a wave
constexpr int kCaqGroup = 4;             // values of one 16-byte load
constexpr int kCaqRowsPerLaunch = 64;    // rows one launch takes (their table travels in the kernel arguments)

// One row of a launch: dense float32 [batch][c][hw] from `map`, read as 32-bit patterns.
struct CaqRow {
  const uint32_t* map;
  int32_t c, hw;
  int32_t total;             // batch * hw: the values of one channel
  int32_t n_slabs;           // ceil(total / kCaqSlab): blocks a channel
  int32_t block0;            // first block of the row in the launch's grid
  int32_t rec0;              // the row's first record (store and scale table)
};
struct CaqArgs {
  CaqRow rows[kCaqRowsPerLaunch];
  long long* store;
  const float* scales;       // ERROR pass: [records] 2^(Qb + 7); null in the RANGE pass
  int32_t n_rows;
};
static_assert(sizeof(CaqRow) == 32 && offsetof(CaqArgs, store) == 2048 && offsetof(CaqArgs, scales) == 2056 && offsetof(CaqArgs, n_rows) == 2064 &&
              sizeof(CaqArgs) == 2072, "the kernel's argument layout");

inline size_t caq_range_store_size(long long n_records) { return (size_t)n_records * kCaqRangeSlots * sizeof(long long); }
inline size_t caq_error_store_size(long long n_records) { return (size_t)n_records * kCaqErrorSlots * sizeof(long long); }

tf2_status caq_store_init(void* store, size_t store_bytes, void* stream);
// error: the ERROR pass (scales_dev required); otherwise the RANGE pass
tf2_status caq_run(bool error, const tf2_caq_row* rows, const void* const* maps, int n_rows, int batch, const float* scales_dev,
                   void* store, size_t store_bytes, void* stream);

}  // namespace tf2
