// act_audit.h -- the activation audit behind tf2_audit_* (include/tf2_amd.h): the handle (host) and the argument blocks of its kernels
// (act_audit.hip).  tf2_amd/audit.py states the statistics (reference_audit); the device store equals it as integers.
#pragma once
#include <cstddef>
#include "act_rows.h"

namespace tf2 {

constexpr int kAuditSlots = 16;          // int64 words of a channel's record (tf2_amd.h: n, neg, lo_rail, hi_rail, min, max, sum, sumsq, hist[8])
constexpr int kAuditSlab = 1024;         // pixels of an NHWC tensor one block walks: at most 2^10 * 2^14 = 2^24 in a block's sumsq counter
constexpr int kAuditChans = 256;         // channels of a block: four a lane, one wave's width of dword loads
constexpr int kAuditImgSlab = 16384;     // values of one image plane (one channel of one image) a block of the input kernel walks
constexpr int kAuditRowsPerLaunch = 64;  // table rows one launch takes (its row table travels in the kernel arguments)

// One table row of a launch: an NHWC int8 tensor slice [npix][cp] from `base` (the slice's first channel), c channels.
struct AuditRow {
  const int8_t* base;
  const uint8_t* dbl;        // [c] in the packed image: 1 = the channel holds 2y - 128 (null: no such channel)
  long long* store;          // the row's first record
  int32_t npix, c, cp;
  int32_t block0;            // first block of the row in the launch's grid
  int32_t n_cpass;           // ceil(c / kAuditChans): blocks a slab
  int32_t lp_shift;          // log2 of the lanes of a wave that run along channels (the other 64 >> lp_shift run along pixels)
  int32_t vec;               // dword loads allowed: the slice starts on a 4-byte boundary and cp % 4 == 0
  int32_t pad;
};
struct AuditRowsArgs {
  AuditRow rows[kAuditRowsPerLaunch];
  int32_t n_rows;
};
static_assert(sizeof(AuditRow) == 56 && offsetof(AuditRowsArgs, n_rows) == 3584 && sizeof(AuditRowsArgs) == 3592, "the kernel's argument layout");

// The input record: dense NCHW images, float32 (quantised with trans = 2^Q0 by quant_input) or int8.
struct AuditImgArgs {
  const void* images;
  long long* store;          // record 0
  float trans;
  int32_t is_q, c, hw, planes;       // planes = batch * c
  int32_t slabs;             // blocks a plane
  int32_t vec;               // hw % 4 == 0 and an aligned base: a lane's four values are one 16-byte (float) or 4-byte (int8) load
};
static_assert(offsetof(AuditImgArgs, store) == 8 && offsetof(AuditImgArgs, vec) == 40 && sizeof(AuditImgArgs) == 48, "the kernel's argument layout");

struct Auditor {
  ActRows g;                 // the rows and their records (act_rows.h)

  tf2_status create(Net* n) { return g.create(n); }
  size_t store_size() const { return g.store_size(kAuditSlots); }
  size_t workspace_size(int batch) { return g.workspace_size(batch); }
  tf2_status store_init(void* store, size_t store_bytes, void* stream) const;
  tf2_status run(const void* images, bool images_are_q, int batch, void* ws, size_t ws_bytes, int8_t* logits, void* store,
                 size_t store_bytes, void* stream, bool with_step = true);
};

}  // namespace tf2
