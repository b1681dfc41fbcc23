// preprocess_aa.hip -- raw uint8 images -> the net's input with Pillow's antialiased bilinear resize (tf2_preprocess_aa,
// include/tf2_amd.h): channel pick, Image.resize(size, BILINEAR) of the 8-bit image restated bit for bit (resample_aa.h: 22-bit integer
// coefficients, a horizontal pass to bytes, a vertical pass on those bytes), crop, per-channel mean and scale, and optionally the input
// quantisation of runner.cpp:158-164.  torchvision's Resize + CenterCrop on PIL images (data_loader.py:83-90) is this arithmetic;
// tf2_amd/preprocess.py restates it (reference_aa) and the device output is bit-identical to it.
//
// A block of 256 threads owns a tile of 8 rows x 32 columns of one image's output; the grid is batch x ceil(image_h / 8) x
// ceil(image_w / 32) blocks whatever the source sizes and scales (a captured graph stays valid when new images are copied into the
// same buffers).  The record is device data: the block validates it before it reads a pixel, and a malformed record leaves zeros and
// a status code.  A valid one:
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
// Bank behaviour: the coefficient rows are 65 dwords apart, so the 32 columns of a half-wave read 32 banks; the packed pixel makes the
// byte tile a dword tile (one conflict-free ds_read_b32 gives the three channels; byte-wide rows would put four columns on a bank).
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "resample_aa.h"
#include "preprocess.h"

namespace tf2 {

namespace {

constexpr int kAaThreads = 256;
constexpr int kAaTileH = 8, kAaTileW = 32;              // output tile
constexpr int kAaRowsPerThread = 2;                     // source rows a thread reduces per chunk
constexpr int kAaChunk = kAaTileH * kAaRowsPerThread;   // source rows of a chunk
constexpr int kAaTapGroup = 4;                          // taps whose loads are in flight together
constexpr int kAaAxes = kAaTileW + kAaTileH;            // coefficient rows of a tile: its columns, then its rows
static_assert(kAaTileH * kAaTileW == kAaThreads, "a thread per tile pixel");

struct PreprocessAaArgs {
  const uint8_t* pixels;
  unsigned long long pixels_bytes;
  const tf2_image_src* srcs;
  void* out;
  int32_t* status;
  int OH, OW, plane, tiles_x, tiles_per_image;
  int pb, ch0, ch1, ch2;
  float mean0, mean1, mean2, scale0, scale1, scale2, trans;
};

template <bool OUT_Q>
__global__ __launch_bounds__(kAaThreads) void preprocess_aa_kernel(PreprocessAaArgs a) {
  __shared__ int s_coef[kAaAxes][kAaMaxTaps];
  __shared__ double s_center[kAaAxes], s_ww[kAaAxes], s_ss[kAaAxes];
  __shared__ int s_lo[kAaAxes], s_n[kAaAxes];
  __shared__ uint32_t s_t[2][kAaChunk][kAaTileW];

  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.tiles_per_image;
  const int tile = blockIdx.x - b * a.tiles_per_image;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int oy = tid / kAaTileW, ox = tid - oy * kAaTileW;
  const tf2_image_src r = a.srcs[b];
  const int st = record_status_aa(r, a.pb, a.pixels_bytes, a.OH, a.OW);
  if (tile == 0 && tid == 0) a.status[b] = st;

  int acc0 = kAaHalf, acc1 = kAaHalf, acc2 = kAaHalf;
  if (st == 0) {                                                   // (the same for the whole block)
    if (tid < kAaAxes) {                                           // bounds and weight sum of one column / one row
      const bool col = tid < kAaTileW;
      const int o = col ? tx * kAaTileW + tid : ty * kAaTileH + (tid - kAaTileW);
      const int n_in = col ? r.w : r.h;
      const AaAxis ax = aa_axis(n_in, col ? r.resize_w : r.resize_h);
      double center = 0.0, ww = 0.0;
      int lo = 0, n = 0;
      if (o < (col ? a.OW : a.OH)) {                               // past the image: no taps, nothing read
        aa_bounds(ax, o + (col ? r.crop_x : r.crop_y), n_in, center, lo, n);
        ww = aa_weight_sum(ax, center, lo, n);
      }
      s_center[tid] = center; s_ww[tid] = ww; s_ss[tid] = ax.ss; s_lo[tid] = lo; s_n[tid] = n;
    }
    __syncthreads();
    // the coefficients, (axis entry, tap) pairs spread over the block tap-major: n <= 2 * ceil(scale) + 1 on an axis, so at 1x .. 2x
    // one sweep of the block covers the tile's 40 x 5 pairs
    const int cx = (r.w + r.resize_w - 1) / r.resize_w, cy = (r.h + r.resize_h - 1) / r.resize_h;
    const int kmax = 2 * (cx > cy ? cx : cy) + 1 < kAaMaxTaps ? 2 * (cx > cy ? cx : cy) + 1 : kAaMaxTaps;
    for (int i = tid; i < kAaAxes * kmax; i += kAaThreads) {
      const int k = i / kAaAxes, e = i - k * kAaAxes;
      if (k < s_n[e]) {
        const AaAxis ax{0.0, 0.0, s_ss[e]};                         // (a weight reads ss alone)
        s_coef[e][k] = aa_coef(aa_weight(ax, s_center[e], s_lo[e], k), s_ww[e]);
      }
    }
    __syncthreads();

    // the source rows the tile reads: lo and hi do not decrease from one row to the next, so they are the first row's lo and the
    // last row's hi (the last row inside the image)
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

}  // namespace

tf2_status preprocess_aa(const Net& net, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes,
                         const tf2_image_src* srcs, int batch, int out_q, void* out, int32_t* status, void* stream) {
  auto refuse = [](const std::string& m) { set_error("tf2_preprocess_aa: " + m); return TF2_ERR_ARG; };
  const std::string why = preprocess_refusal(net, d, batch, out_q, pixels && srcs && out && status);
  if (!why.empty()) return refuse(why);

  PreprocessAaArgs a{};
  a.pixels = pixels; a.pixels_bytes = pixels_bytes; a.srcs = srcs; a.out = out; a.status = status;
  a.OH = net.nd.image_h; a.OW = net.nd.image_w; a.plane = a.OH * a.OW;
  a.tiles_x = (a.OW + kAaTileW - 1) / kAaTileW;
  a.tiles_per_image = a.tiles_x * ((a.OH + kAaTileH - 1) / kAaTileH);
  a.pb = d->pixel_bytes; a.ch0 = d->src_channel[0]; a.ch1 = d->src_channel[1]; a.ch2 = d->src_channel[2];
  a.mean0 = d->mean[0]; a.mean1 = d->mean[1]; a.mean2 = d->mean[2];
  a.scale0 = d->scale[0]; a.scale1 = d->scale[1]; a.scale2 = d->scale[2];
  a.trans = out_q ? std::ldexp(1.0f, -(int)net.q[0]) : 1.0f;       // 2^-Q0, as tf2_preprocess reads it
  const long long blocks = (long long)batch * a.tiles_per_image;
  if (blocks > 0x7fffffffLL) return refuse("batch too large for one launch");
  const dim3 grid((unsigned)blocks), block(kAaThreads);
  hipStream_t s = (hipStream_t)stream;
  if (out_q) hipLaunchKernelGGL((preprocess_aa_kernel<true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((preprocess_aa_kernel<false>), grid, block, 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string("tf2_preprocess_aa: launch failed: ") + hipGetErrorString(e)); return TF2_ERR_HIP; }
  return TF2_OK;
}

}  // namespace tf2
