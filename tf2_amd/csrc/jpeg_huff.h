// jpeg_huff.h -- tf2_jpeg_huff's implementation (jpeg_huff.hip): host checks, then one kernel on the caller's stream.
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kHuffThreads = TF2_JPEG_HUFF_LANES;        // threads of a workgroup: the most subsequences of a chunk
constexpr int kHuffChunkBytes = 65536;                   // the most data of a chunk (it is staged in LDS)
// subsequences of a chunk: as many as the workgroup has threads and the LDS window takes, and at most 16 * subseq_bytes -- short
// subsequences are for tests, where the bound lets a file of a few KB span several chunks
inline int jpeg_huff_chunk_lanes(int subseq_bytes) {
  int n = kHuffChunkBytes / subseq_bytes;
  if (n > 16 * subseq_bytes) n = 16 * subseq_bytes;
  return n > kHuffThreads ? kHuffThreads : n;
}
constexpr int kHuffWorkHeader = 16;              // bytes in front of an image's 8 bytes a subsequence

size_t jpeg_huff_work_bytes(const tf2_jpeg_huff_desc* d, int batch, size_t max_scan_bytes);
tf2_status jpeg_huff(const tf2_jpeg_huff_desc* d, const uint8_t* bytes, size_t bytes_len, const tf2_jpeg_scan* scan,
                     const tf2_jpeg_src* jpeg, int16_t* coef, size_t coef_blocks, uint8_t* work, size_t work_bytes, int batch,
                     int32_t* status, void* stream);

}  // namespace tf2
