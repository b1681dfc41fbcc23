// embed_match.h -- on-device face matching behind tf2_emb_* (include/tf2_amd.h): the matcher handle (host) and the constants its
// three kernels (embed_match.hip) share with the host checks and with tf2_amd/embed.py.
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kEmbMaxD = 512;        // one wave keeps an image's D features in LDS; a lane holds at most 512 / 64 of them
constexpr int kEmbMaxTopK = 16;      // winner r of a query lives in lane r of its wave
constexpr int kEmbSlab = 64;         // gallery rows a stage-1 block owns: one row a lane
constexpr int kEmbGroup = 32;        // queries a stage-1 block owns: four waves x eight accumulators a lane

struct Matcher {
  int d = 0, top_k = 0;
  void* consts = nullptr;            // read-only device constants, uploaded once by create: scale [d] = 2^-sh

  ~Matcher();
  tf2_status create(const Net* net, const tf2_emb_desc* desc);
  size_t scratch_size(int batch, long long n_rows) const;
  tf2_status embed(const int8_t* out_i8, int batch, float* rows, void* stream);
  tf2_status match(const int8_t* out_i8, int batch, const float* gallery, const int32_t* gallery_ids, long long n_rows, float threshold,
                   void* scratch, size_t scratch_bytes, int32_t* idx, float* dist, int32_t* ids_out, float* emb_out,
                   const int32_t* truth, uint64_t* tally, void* stream);
};

}  // namespace tf2
