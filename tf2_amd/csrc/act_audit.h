// act_audit.h -- the activation audit behind tf2_audit_* (include/tf2_amd.h): the handle (host) and the argument blocks of its kernels
// (act_audit.hip).  tf2_amd/audit.py states the statistics (reference_audit); the device store equals it as integers.
#pragma once
#include "tf2_net.h"

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

// The input record: dense NCHW images, float32 (quantised with trans = 2^Q0 by quant_input) or int8.
struct AuditImgArgs {
  const void* images;
  long long* store;          // record 0
  float trans;
  int32_t is_q, c, hw, planes;       // planes = batch * c
  int32_t slabs;             // blocks a plane
  int32_t vec;               // hw % 4 == 0 and an aligned base: a lane's four values are one 16-byte (float) or 4-byte (int8) load
};

int launch_audit_rows(const AuditRowsArgs& a, int blocks, void* stream);
int launch_audit_image(const AuditImgArgs& a, void* stream);
int launch_audit_init(long long* store, long long n_records, void* stream);

struct Auditor {
  struct Row { int layer, C, H, W; long long rec0; int n_doubled; };
  Net* net = nullptr;
  std::vector<Row> rows;     // row -1 first
  long long n_records = 0;

  tf2_status create(Net* n);
  size_t store_size() const { return (size_t)n_records * kAuditSlots * sizeof(long long); }
  size_t workspace_size(int batch);
  tf2_status store_init(void* store, size_t store_bytes, void* stream) const;
  tf2_status run(const void* images, bool images_are_q, int batch, void* ws, size_t ws_bytes, int8_t* logits, void* store,
                 size_t store_bytes, void* stream, bool with_step = true);
};

}  // namespace tf2
