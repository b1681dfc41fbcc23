// classify.h -- on-device classification behind tf2_cls_* (include/tf2_amd.h): the classifier handle (host) and the argument
// block of its kernel (classify.hip).
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kClsMaxN = 4096;       // one wave keeps an image's n orderable features in LDS: 4 waves x 4096 x 4 bytes = 64 KiB a block
constexpr int kClsMaxTopK = 64;      // winner r of an image lives in lane r of its wave

struct ClassifyArgs {
  const int8_t* logits;              // [batch][n]
  const float* scale;                // [n], 2^-sh
  int32_t* labels;                   // [batch][top_k]
  float* features;                   // [batch][top_k] or null
  float* probs;                      // [batch][top_k] or null
  float* all_probs;                  // [batch][n] or null
  const int32_t* truth;              // [batch] or null
  int32_t* rank;                     // [batch] or null
  unsigned long long* tally;         // [4] or null, accumulated
  int32_t n, top_k, batch;
};

struct Classifier {
  int n = 0, top_k = 0;
  void* consts = nullptr;            // read-only device constants, uploaded once by create: scale [n]

  ~Classifier();
  tf2_status create(const Net* net, const tf2_cls_desc* d);
  tf2_status run(const int8_t* logits, int batch, int32_t* labels, float* features, float* probs, float* all_probs,
                 const int32_t* truth, int32_t* rank, uint64_t* tally, void* stream);
};

}  // namespace tf2
