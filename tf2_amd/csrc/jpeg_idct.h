// jpeg_idct.h -- tf2_jpeg_idct's implementation (jpeg_idct.hip): host checks, then one kernel on the caller's stream.
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kJpegThreads = 256;
constexpr int kJpegTileBW = TF2_JPEG_TILE_BW;    // coefficient blocks of a tile: a wave takes one row of 8 blocks, 8 lanes a block
constexpr int kJpegTileBH = TF2_JPEG_TILE_BH;
constexpr int kJpegMaxBlocksPerImage = 64;

// blocks_per_image = 0: about 2048 blocks a launch, between 1 and 64 an image -- a function of batch alone
inline int jpeg_default_blocks_per_image(int batch) {
  const int n = 2048 / (batch < 1 ? 1 : batch);
  return n < 1 ? 1 : (n > kJpegMaxBlocksPerImage ? kJpegMaxBlocksPerImage : n);
}

tf2_status jpeg_idct(const tf2_jpeg_desc* d, const int16_t* coef, size_t coef_blocks, const tf2_jpeg_src* jpeg, const uint16_t* quant,
                     uint8_t* planes, size_t planes_bytes, const tf2_ycc_src* ycc, const tf2_image_src* srcs, int batch,
                     int32_t* status, void* stream);

}  // namespace tf2
