// ssd_detect.h -- on-device SSD detection behind tf2_ssd_* (include/tf2_amd.h): the detector handle (host) and the
// argument blocks of its two kernels (ssd_detect.hip).
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kSsdMaxSources = 8;
constexpr int kSsdMaxClasses = 256;
constexpr int kSsdMaxTopK = 256;
constexpr int kSsdMaxPriors = 32768;     // the select kernel keeps one class's scores of an image in LDS (4 bytes a prior)

// Stage 1 (ssd_heads_kernel): one thread per (image, prior).  Head tensors are NHWC int8 with pitch *_cp; channel `ch` of a
// head is value * 2^-Q after undoing the doubled form (2y - 128) where dbl[ch] says so; scale[ch] = 2^-Q.
struct SsdHeadArgs {
  const int8_t* loc[kSsdMaxSources];
  const int8_t* conf[kSsdMaxSources];
  int32_t loc_cp[kSsdMaxSources], conf_cp[kSsdMaxSources];
  int32_t hw[kSsdMaxSources], nb[kSsdMaxSources];
  int32_t start[kSsdMaxSources];               // first prior of each source (prefix of H * W * nb)
  int32_t loc_ch0[kSsdMaxSources], conf_ch0[kSsdMaxSources];   // first entry of each head in scale / dbl
  int32_t n_src, P, C, batch;
  float v0, v1;
  const float* priors;                          // [P][4] centre form
  const float* scale;
  const uint8_t* dbl;
  float* boxes;                                 // [batch][P][4] corner form
  float* probs;                                 // [batch][C][P] (class-major: what stage 2 reads)
  float* scores_out;                            // [batch][P][C] or null
};

// Stage 2 (ssd_select_kernel): one block per (image, class); class 0 only writes zeros.
struct SsdSelectArgs {
  const float* boxes;                           // [batch][P][4]
  const float* probs;                           // [batch][C][P]
  float* det;                                   // [batch][C][top_k][5]
  int32_t* counts;                              // [batch][C]
  int32_t P, C, top_k, batch;
  float conf_thresh, nms_thresh;
};

int launch_ssd_heads(const SsdHeadArgs& a, void* stream);
int launch_ssd_transpose(const float* src, float* dst, int batch, int P, int C, void* stream);   // [B][P][C] -> [B][C][P]
int launch_ssd_select(const SsdSelectArgs& a, void* stream);

struct SsdDetector {
  Net* net = nullptr;
  int C = 0, top_k = 0, n_src = 0, P = 0;
  float conf_thresh = 0.f, nms_thresh = 0.f, v0 = 0.f, v1 = 0.f;
  int loc_row[kSsdMaxSources] = {}, conf_row[kSsdMaxSources] = {};
  int nb[kSsdMaxSources] = {}, hw[kSsdMaxSources] = {}, start[kSsdMaxSources] = {};
  int loc_ch0[kSsdMaxSources] = {}, conf_ch0[kSsdMaxSources] = {};
  // read-only device constants, uploaded once by create: priors [P][4] | scale [n_ch] | dbl [n_ch]
  void* consts = nullptr;
  const float* priors_dev = nullptr;
  const float* scale_dev = nullptr;
  const uint8_t* dbl_dev = nullptr;

  ~SsdDetector();
  tf2_status create(Net* n, const tf2_ssd_desc* d);
  size_t workspace_size(int batch);
  size_t detect_scratch_size(int batch) const;
  tf2_status run(const void* images, bool images_are_q, int batch, void* ws, size_t ws_bytes, float* det, int32_t* counts,
                 float* boxes_out, float* scores_out, int8_t* logits, void* mark_event, void* stream);
  tf2_status detect(const float* boxes, const float* scores, int batch, void* scratch, size_t scratch_bytes, float* det,
                    int32_t* counts, void* stream);
};

}  // namespace tf2
