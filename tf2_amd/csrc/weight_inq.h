// weight_inq.h -- INQ weight quantisation behind tf2_inq_* (include/tf2_amd.h): the record, the scratch layout and the argument blocks of
// the kernels (weight_inq.hip).  tf2_amd/inq.py states the rule (reference_range / reference_step); the device equals it as bits.
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kInqWords = 32;            // int64 words of a segment's record (tf2_amd.h "INQ weight quantisation")
constexpr int kInqChunk = 4096;          // elements of the flat buffer one block walks: 256 threads x four 16-byte groups
constexpr int kInqSegsPerLaunch = 96;    // segments one launch takes (their table travels in the kernel arguments)
constexpr int kInqPasses = 4;            // radix-select passes over the 31-bit magnitude pattern: bits 30..23, 22..15, 14..7, 6..0
constexpr int kInqBins = 256;

// words of the record
enum : int {
  kInqN1 = 0, kInqN0, kInqMax1, kInqMax0, kInqNonfinite, kInqMaxExp, kInqMinExp, kInqNKeep, kInqNUpdate, kInqThr, kInqStatus,
  kInqFlushedMin, kInqFlushedFloor, kInqOverOne, kInqHist /* 14 .. 29 */, kInqReserved = 30
};

// The select's words of a segment, behind the histograms in the scratch buffer.
struct InqSel {
  unsigned long long rank;   // rank still to find among the values that match `prefix`
  uint32_t prefix;           // the bits of the threshold pattern found so far
  uint32_t active;           // 1: the segment is updated in this step (status 0 and n_update > 0)
};

// scratch: uint32 hist[n_segs][kInqPasses][kInqBins], then InqSel sel[n_segs]
inline size_t inq_scratch_size(long long n_segs) { return (size_t)n_segs * (kInqPasses * kInqBins * sizeof(uint32_t) + sizeof(InqSel)); }
inline size_t inq_state_size(long long n_segs) { return (size_t)n_segs * kInqWords * sizeof(long long); }

// One launch's share of the segment table; a block owns elements [first + blockIdx.x * kInqChunk, + kInqChunk) of the flat buffer.
struct InqArgs {
  long long off[kInqSegsPerLaunch];
  long long end[kInqSegsPerLaunch];      // off + count
  float* w;
  uint8_t* mask;
  uint8_t* codes;                        // null: no codes
  long long* state;                      // record of the launch's first segment
  uint32_t* hist;                        // histograms of the launch's first segment
  InqSel* sel;
  long long first;                       // first element of block 0 (a multiple of kInqChunk)
  int32_t n_segs;
  int32_t vec;                           // 16-byte accesses allowed: w 16-byte, mask and codes 4-byte aligned
  int32_t pass, shift, hi_shift;         // select passes: the digit is (mag >> shift) & ((1 << (hi_shift - shift)) - 1)
  int32_t exp_floor;
};

struct InqPlanArgs {
  long long* state;
  InqSel* sel;
  int32_t n_segs, n_values;
  double prev, cur;
};

tf2_status inq_step(float* w, uint8_t* mask, long long n_total, const tf2_inq_seg* segs, int n_segs, double prev, double cur, int n_values,
                    int exp_floor, uint8_t* codes, void* state, void* scratch, size_t scratch_bytes, void* stream);

}  // namespace tf2
