// ycc_convert.h -- tf2_ycc_to_rgb's implementation (ycc_convert.hip): host checks, then one kernel on the caller's stream.
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kYccThreads = 256;
constexpr int kYccTileW = TF2_YCC_TILE_W;        // output pixels of a tile: 32 threads x 4 pixels a row, 8 threads x 2 rows
constexpr int kYccTileH = TF2_YCC_TILE_H;
constexpr int kYccMaxBlocksPerImage = 64;

// blocks_per_image = 0: about 2048 blocks a launch, between 1 and 64 an image -- a function of batch alone
inline int ycc_default_blocks_per_image(int batch) {
  const int n = 2048 / (batch < 1 ? 1 : batch);
  return n < 1 ? 1 : (n > kYccMaxBlocksPerImage ? kYccMaxBlocksPerImage : n);
}

tf2_status ycc_to_rgb(const tf2_ycc_desc* d, const uint8_t* src, size_t src_bytes, const tf2_ycc_src* ycc, uint8_t* pixels,
                      size_t pixels_bytes, const tf2_image_src* srcs, int batch, int32_t* status, void* stream);

}  // namespace tf2
