// image_input.h -- what the five image-input kernels state once (preprocess.hip, preprocess_aa.hip, roi_crop.hip, roi_crop_aa.hip,
// roi_warp.hip): the argument block and the host function that fills it, the rule that takes a slot of a table to its source record,
// the launch of a gather kernel (<OUT_Q, VEC>, four pixels a thread) and of a tile kernel (<OUT_Q>), and the antialiased tile kernel
// itself, a template over the geometry of its two users.  Include after <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "tf2_net.h"
#include "resample.h"
#include "resample_aa.h"
#include "preprocess.h"

namespace tf2 {

// Everything the five kernels share.  Scalars only: the argument block is not indexed (an indexed one goes through scratch).  A
// kernel's own arguments -- its table, its blocks or tiles per image -- follow the block in its parameter list.
struct ImageArgs {
  const uint8_t* pixels;
  unsigned long long pixels_bytes;
  const tf2_image_src* srcs;
  void* out;
  int32_t* status;
  int OH, OW, plane, batch;
  int pb, ch0, ch1, ch2, round_resized;
  float mean0, mean1, mean2, scale0, scale1, scale2, trans;
};

// the block of a call that passed preprocess_refusal
inline ImageArgs image_args(const Net& net, const tf2_preprocess_desc* d, int out_q, const uint8_t* pixels, size_t pixels_bytes,
                            const tf2_image_src* srcs, int batch, void* out, int32_t* status) {
  ImageArgs a{};
  a.pixels = pixels; a.pixels_bytes = pixels_bytes; a.srcs = srcs; a.out = out; a.status = status;
  a.batch = batch; a.OH = net.nd.image_h; a.OW = net.nd.image_w; a.plane = a.OH * a.OW;
  a.pb = d->pixel_bytes; a.ch0 = d->src_channel[0]; a.ch1 = d->src_channel[1]; a.ch2 = d->src_channel[2];
  a.round_resized = d->round_resized;
  a.mean0 = d->mean[0]; a.mean1 = d->mean[1]; a.mean2 = d->mean[2];
  a.scale0 = d->scale[0]; a.scale1 = d->scale[1]; a.scale2 = d->scale[2];
  // 2^-Q0, read now from where prep_input reads it (q[0]); the same value as its 1 / (1 << q0) | (1 << -q0) for every |q0| <= 30
  a.trans = out_q ? std::ldexp(1.0f, -(int)net.q[0]) : 1.0f;
  return a;
}

// The source of one slot of a ROI or transform table: TF2_ROI_EMPTY for image == -1, TF2_ROI_BAD_IMAGE for an image outside the
// batch, else r receives the source record and TF2_ROI_BAD_SRC says that it fails src_status.  A kernel ORs its own rule (the box,
// the matrix) to the result of a slot that is not EMPTY.
__device__ __forceinline__ int slot_source(const ImageArgs& a, int image, int own, tf2_image_src& r) {
  if (image == -1) return TF2_ROI_EMPTY;
  int st = 0;
  if (image < 0 || image >= a.batch) st |= TF2_ROI_BAD_IMAGE;
  else {
    r = a.srcs[image];
    if (src_status(r, a.pb, a.pixels_bytes) != 0) st |= TF2_ROI_BAD_SRC;
  }
  return st | own;
}

// ---- gather kernels: blocks_per_image blocks of kPrepThreads threads an output image, kPrepPix consecutive pixels a thread ---------

// the output image of a block, the first pixel of a thread, and whether the thread writes the image's status word
__device__ __forceinline__ void gather_thread(int blocks_per_image, int& img, int& p0, bool& first) {
  img = blockIdx.x / blocks_per_image;
  p0 = (blockIdx.x - img * blocks_per_image) * kPrepBlockPix + threadIdx.x * kPrepPix;
  first = blockIdx.x == img * blocks_per_image && threadIdx.x == 0;
}

__device__ __forceinline__ void zero_px(float (&v)[3][kPrepPix]) {
  for (int c = 0; c < 3; c++)
    for (int j = 0; j < kPrepPix; j++) v[c][j] = 0.0f;
}

// the four instantiations of a gather kernel, [OUT_Q][VEC]
#define TF2_GATHER_KERNELS(kernel) {{kernel<false, false>, kernel<false, true>}, {kernel<true, false>, kernel<true, true>}}

// Launches the instantiation that out_q and the output's alignment pick, n_images x ceil(plane / 1024) blocks.  "" or the refusal;
// the launch's own result is left for launch_result.
template <typename... Own>
std::string launch_gather(void (*const (&kernels)[2][2])(ImageArgs, int, Own...), const ImageArgs& a, int out_q, int n_images,
                          const char* n_images_name, void* stream, Own... own) {
  const int blocks_per_image = (a.plane + kPrepBlockPix - 1) / kPrepBlockPix;
  const bool vec = (a.plane % kPrepPix == 0) && ((uintptr_t)a.out % (out_q ? 4 : 16) == 0);   // whole aligned 4-pixel runs
  const long long blocks = (long long)n_images * blocks_per_image;
  if (blocks > 0x7fffffffLL) return std::string(n_images_name) + " too large for one launch";
  hipLaunchKernelGGL(kernels[out_q][vec], dim3((unsigned)blocks), dim3(kPrepThreads), 0, (hipStream_t)stream, a, blocks_per_image, own...);
  return "";
}

// ---- the antialiased tile kernel ------------------------------------------------------------------------------------------------------
// A block of 256 threads owns a tile of 8 rows x 32 columns of one output image:
//   setup    the bounds (lo, n), center and weight sum of the tile's 32 columns and 8 rows, one thread each, then the 40 x n
//            coefficients spread over the block (the double divisions are the cost) -> LDS, 40 x 65 int32
//   stream   the source rows lo(first row) .. hi(last row) of the tile in chunks of 16: thread (j, x) reduces source rows j and j + 8 of
//            the chunk over column x's taps to three bytes each, packed into one dword of LDS (a chunk is 16 x 32 dwords; two of
//            them, so one barrier a chunk); then thread (y, x) adds the chunk's rows that lie in row y's window, times the row
//            coefficient, to its three int32 accumulators.  A horizontal sum is made once per tile and source row, not once per
//            output pixel.  The kernel waits on memory latency, not bandwidth: the taps are loaded four at a time for both rows (24
//            byte loads in flight a thread), and at 1x .. 3x a tile is one or two chunks.
//   output   clip8, mean, scale, quantise; 32 consecutive elements a row.
// LDS is 15 KB whatever the scale; a tile at 32x on both axes walks 21 chunks of 65 taps (TF2_PREP_AA_MAX_SCALE bounds it).
// Bank behaviour (a half-wave, the lane group of ds_read_b32 / ds_write_b32, is one row of the tile: 32 columns, one oy): s_coef rows
// are 65 dwords apart, so the horizontal pass's 32 columns read tap k from banks (ox + k) mod 32, all different, and the vertical
// pass's row coefficient is one address for the half-wave, a broadcast; s_t holds one packed pixel a dword and 32 dwords a source
// row, so the store of a reduced row and the load of a window row touch each bank once (byte-wide rows would put four columns on a
// bank).
//
// The geometry G is what the two users differ in (preprocess_aa.hip: AaResizeCrop, roi_crop_aa.hip: AaBox), an object in registers:
//   int load(a, img, r, own...)        the record(s) of output image img -> status bits (0: r is the source record to read)
//   AaAxis axis(a, r, col)             the column (col) or row axis
//   void bounds(ax, r, col, o, center, lo, n)   aa_bounds of output index o on it
//   kSupportInLds, int taps(r)         how the tap count of the coefficient sweep is bounded: from ceil(support) of the two axes, left
//                                      in LDS by their first threads, or from the record alone
// The kernel is a __global__ template and not a device function under two kernels: hipcc folds expressions once before it inlines, and
// behind a call the stream loop was allocated 78 VGPRs instead of 76 (profiles/image_input_isa.txt).

constexpr int kAaThreads = 256;
constexpr int kAaTileH = 8, kAaTileW = 32;              // output tile
constexpr int kAaRowsPerThread = 2;                     // source rows a thread reduces per chunk
constexpr int kAaChunk = kAaTileH * kAaRowsPerThread;   // source rows of a chunk
constexpr int kAaTapGroup = 4;                          // taps whose loads are in flight together
constexpr int kAaAxes = kAaTileW + kAaTileH;            // coefficient rows of a tile: its columns, then its rows
static_assert(kAaTileH * kAaTileW == kAaThreads, "a thread per tile pixel");

template <typename G, bool OUT_Q, typename... Own>
__global__ __launch_bounds__(kAaThreads) void aa_tile_kernel(ImageArgs a, int tiles_x, int tiles_per_image, Own... own) {
  __shared__ int s_coef[kAaAxes][kAaMaxTaps];
  __shared__ double s_center[kAaAxes], s_ww[kAaAxes], s_ss[kAaAxes];
  __shared__ int s_lo[kAaAxes], s_n[kAaAxes];
  __shared__ int s_kc[2];                                          // kSupportInLds: ceil(support) along x, along y
  __shared__ uint32_t s_t[2][kAaChunk][kAaTileW];

  const int tid = threadIdx.x;
  const int b = blockIdx.x / tiles_per_image;
  const int tile = blockIdx.x - b * tiles_per_image;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int oy = tid / kAaTileW, ox = tid - oy * kAaTileW;
  G geo;
  tf2_image_src r{};
  const int st = geo.load(a, b, r, own...);
  if (tile == 0 && tid == 0) a.status[b] = st;

  int acc0 = kAaHalf, acc1 = kAaHalf, acc2 = kAaHalf;
  if (st == 0) {                                                   // (the same for the whole block)
    if (tid < kAaAxes) {                                           // bounds and weight sum of one column / one row
      const bool col = tid < kAaTileW;
      const int o = col ? tx * kAaTileW + tid : ty * kAaTileH + (tid - kAaTileW);
      const AaAxis ax = geo.axis(a, r, col);
      double center = 0.0, ww = 0.0;
      int lo = 0, n = 0;
      if (o < (col ? a.OW : a.OH)) {                               // past the image: no taps, nothing read
        geo.bounds(ax, r, col, o, center, lo, n);
        ww = aa_weight_sum(ax, center, lo, n);
      }
      s_center[tid] = center; s_ww[tid] = ww; s_ss[tid] = ax.ss; s_lo[tid] = lo; s_n[tid] = n;
      if (G::kSupportInLds && (tid == 0 || tid == kAaTileW)) s_kc[col ? 0 : 1] = (int)ceil(ax.support);   // 1 .. 32 for a slot that passed
    }
    __syncthreads();
    // the coefficients, (axis entry, tap) pairs spread over the block tap-major: n <= 2 * ceil(support) + 1 on an axis, so at 1x .. 2x
    // one sweep of the block covers the tile's 40 x 5 pairs
    const int kc = G::kSupportInLds ? (s_kc[0] > s_kc[1] ? s_kc[0] : s_kc[1]) : geo.taps(r);
    const int kmax = 2 * kc + 1 < kAaMaxTaps ? 2 * kc + 1 : kAaMaxTaps;
    for (int i = tid; i < kAaAxes * kmax; i += kAaThreads) {
      const int k = i / kAaAxes, e = i - k * kAaAxes;
      if (k < s_n[e]) {
        const AaAxis ax{0.0, 0.0, s_ss[e]};                         // (a weight reads ss alone)
        s_coef[e][k] = aa_coef(aa_weight(ax, s_center[e], s_lo[e], k), s_ww[e]);
      }
    }
    __syncthreads();

    // the source rows the tile reads: lo and hi do not decrease from one row to the next, so they are the first row's lo and the
    // last row's hi (the last row inside the output)
    const int last = a.OH - 1 - ty * kAaTileH < kAaTileH - 1 ? a.OH - 1 - ty * kAaTileH : kAaTileH - 1;
    const int row_begin = s_lo[kAaTileW], row_end = s_lo[kAaTileW + last] + s_n[kAaTileW + last];
    const int xlo = s_lo[ox], xn = s_n[ox];
    const int ylo = s_lo[kAaTileW + oy], yn = s_n[kAaTileW + oy];
    const uint8_t* const base = a.pixels + r.offset + (long long)xlo * a.pb;
    int buf = 0;
    for (int y0 = row_begin; y0 < row_end; y0 += kAaChunk, buf ^= 1) {
      // horizontal: source rows y0 + oy and y0 + oy + 8 at column ox -> three bytes each.  Rows past the tile's last one read its last
      // one instead (no lane leaves the image, nobody reads their result); the taps go four at a time, with every load of a group
      // issued before the first product (a tap past n re-reads tap n - 1 with coefficient 0)
      int h[kAaRowsPerThread][3];
      const uint8_t* p[kAaRowsPerThread];
#pragma unroll
      for (int i = 0; i < kAaRowsPerThread; i++) {
        const int sy = y0 + oy + i * kAaTileH;
        p[i] = base + (long long)(sy < row_end ? sy : row_end - 1) * r.row_pitch;
        h[i][0] = h[i][1] = h[i][2] = kAaHalf;
      }
      for (int k0 = 0; k0 < xn; k0 += kAaTapGroup) {
        int cf[kAaTapGroup];
        int v[kAaRowsPerThread][kAaTapGroup][3];
#pragma unroll
        for (int t = 0; t < kAaTapGroup; t++) {
          const int k = k0 + t;
          const int off = (k < xn ? k : xn - 1) * a.pb;
#pragma unroll
          for (int i = 0; i < kAaRowsPerThread; i++) {
            v[i][t][0] = p[i][off + a.ch0];
            v[i][t][1] = p[i][off + a.ch1];
            v[i][t][2] = p[i][off + a.ch2];
          }
        }
#pragma unroll
        for (int t = 0; t < kAaTapGroup; t++) cf[t] = k0 + t < xn ? s_coef[ox][k0 + t] : 0;
#pragma unroll
        for (int t = 0; t < kAaTapGroup; t++)
#pragma unroll
          for (int i = 0; i < kAaRowsPerThread; i++)
#pragma unroll
            for (int c = 0; c < 3; c++) h[i][c] += v[i][t][c] * cf[t];
      }
#pragma unroll
      for (int i = 0; i < kAaRowsPerThread; i++)
        s_t[buf][oy + i * kAaTileH][ox] = (uint32_t)aa_clip8(h[i][0]) | (uint32_t)aa_clip8(h[i][1]) << 8 | (uint32_t)aa_clip8(h[i][2]) << 16;
      __syncthreads();                                             // (the other buffer is written next: one barrier a chunk)
      // vertical: the chunk's rows inside this output row's window
      const int kb = y0 - ylo > 0 ? y0 - ylo : 0, ke = y0 + kAaChunk - ylo < yn ? y0 + kAaChunk - ylo : yn;
      for (int k = kb; k < ke; k++) {
        const uint32_t t = s_t[buf][ylo + k - y0][ox];
        const int cf = s_coef[kAaTileW + oy][k];
        acc0 += (int)(t & 255u) * cf;
        acc1 += (int)(t >> 8 & 255u) * cf;
        acc2 += (int)(t >> 16 & 255u) * cf;
      }
    }
  }

  const int y = ty * kAaTileH + oy, x = tx * kAaTileW + ox;
  if (y < a.OH && x < a.OW) {
    const float v0 = st != 0 ? 0.0f : ((float)aa_clip8(acc0) - a.mean0) * a.scale0;
    const float v1 = st != 0 ? 0.0f : ((float)aa_clip8(acc1) - a.mean1) * a.scale1;
    const float v2 = st != 0 ? 0.0f : ((float)aa_clip8(acc2) - a.mean2) * a.scale2;
    const long long at = (long long)b * 3 * a.plane + y * a.OW + x;
    if (OUT_Q) {
      int8_t* const o = reinterpret_cast<int8_t*>(a.out) + at;
      o[0] = st != 0 ? (int8_t)0 : (int8_t)quant_input(v0, a.trans);
      o[a.plane] = st != 0 ? (int8_t)0 : (int8_t)quant_input(v1, a.trans);
      o[2 * (long long)a.plane] = st != 0 ? (int8_t)0 : (int8_t)quant_input(v2, a.trans);
    } else {
      float* const o = reinterpret_cast<float*>(a.out) + at;
      o[0] = v0;
      o[a.plane] = v1;
      o[2 * (long long)a.plane] = v2;
    }
  }
}

// Launches aa_tile_kernel<G, out_q>, n_images x ceil(OH / 8) x ceil(OW / 32) blocks; "" or the refusal, as launch_gather.
template <typename G, typename... Own>
std::string launch_aa_tiles(const ImageArgs& a, int out_q, int n_images, const char* n_images_name, void* stream, Own... own) {
  const int tiles_x = (a.OW + kAaTileW - 1) / kAaTileW;
  const int tiles_per_image = tiles_x * ((a.OH + kAaTileH - 1) / kAaTileH);
  const long long blocks = (long long)n_images * tiles_per_image;
  if (blocks > 0x7fffffffLL) return std::string(n_images_name) + " too large for one launch";
  const dim3 grid((unsigned)blocks), block(kAaThreads);
  if (out_q) hipLaunchKernelGGL((aa_tile_kernel<G, true, Own...>), grid, block, 0, (hipStream_t)stream, a, tiles_x, tiles_per_image, own...);
  else hipLaunchKernelGGL((aa_tile_kernel<G, false, Own...>), grid, block, 0, (hipStream_t)stream, a, tiles_x, tiles_per_image, own...);
  return "";
}

}  // namespace tf2
