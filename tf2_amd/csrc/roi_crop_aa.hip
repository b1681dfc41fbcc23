// roi_crop_aa.hip -- detections -> a second network's input with Pillow's antialiased bilinear resize (tf2_roi_crop_aa,
// include/tf2_amd.h): each slot of a ROI table is Image.resize((OW, OH), BILINEAR, box=(x0, y0, x1, y1)) of its 8-bit source image,
// restated bit for bit (resample_aa.h, the box form: 22-bit integer coefficients, a horizontal pass to bytes, a vertical pass on
// those bytes), then channel pick, per-channel mean and scale, and optionally the input quantisation of runner.cpp:158-164.  The
// filter is centred on the box and as wide as the box's scale asks: it reads source pixels outside the box and inside the image, so
// the result is not "crop, then resize".  tf2_amd/roi.py restates it (reference_crop_aa) and the device output is bit-identical to it.
//
// The tile scheme is preprocess_aa.hip's.  A block of 256 threads owns a tile of 8 rows x 32 columns of one slot's output; the grid
// is n_slots x ceil(image_h / 8) x ceil(image_w / 32) blocks whatever the table holds (a captured graph stays valid when a new table,
// new records and new pixels are written into the same buffers).  The slot's record and its source record are device data: every
// block validates both before it reads a pixel; a slot with a status -- most slots of a real table are EMPTY -- stores zeros and
// leaves without a barrier.  A valid one:
//   setup    the bounds (lo, n), center and weight sum of the tile's 32 columns and 8 rows from the slot's float box, one thread each;
//            the first column's and the first row's thread also leave ceil(support) of their axis, which bounds the taps of the whole
//            axis (n <= 2 * ceil(support) + 1); then the 40 x n coefficients spread over the block (the double divisions are the
//            cost) -> LDS, 40 x 65 int32
//   stream   the source rows lo(first row) .. hi(last row) of the tile in chunks of 16: thread (j, x) reduces source rows j and j + 8 of
//            the chunk over column x's taps to three bytes each, packed into one dword of LDS (a chunk is 16 x 32 dwords; two of
//            them, so one barrier a chunk); then thread (y, x) adds the chunk's rows that lie in row y's window, times the row
//            coefficient, to its three int32 accumulators.  The taps are loaded four at a time for both rows.
//   output   clip8, mean, scale, quantise; 32 consecutive elements a row.
// LDS is 15 KB whatever the scale; a tile at 32x on both axes walks 21 chunks of 65 taps (TF2_PREP_AA_MAX_SCALE bounds it).
// Bank behaviour (a half-wave, the lane group of ds_read_b32 / ds_write_b32, is one row of the tile: 32 columns, one oy): s_coef rows
// are 65 dwords apart, so the horizontal pass's 32 columns read tap k from banks (ox + k) mod 32, all different, and the vertical
// pass's row coefficient is one address for the half-wave, a broadcast; s_t holds one packed pixel a dword and 32 dwords a source
// row, so the store of a reduced row and the load of a window row touch each bank once (byte-wide rows would put four columns on a
// bank).
// The stream and output code repeats preprocess_aa_kernel's: moved into a shared device function it changed that kernel's register
// allocation (78 VGPRs for 76), so the two bodies stay apart and only resample_aa.h is shared.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "resample_aa.h"
#include "preprocess.h"
#include "roi_crop.h"

namespace tf2 {

namespace {

constexpr int kAaThreads = 256;
constexpr int kAaTileH = 8, kAaTileW = 32;              // output tile
constexpr int kAaRowsPerThread = 2;                     // source rows a thread reduces per chunk
constexpr int kAaChunk = kAaTileH * kAaRowsPerThread;   // source rows of a chunk
constexpr int kAaTapGroup = 4;                          // taps whose loads are in flight together
constexpr int kAaAxes = kAaTileW + kAaTileH;            // coefficient rows of a tile: its columns, then its rows
static_assert(kAaTileH * kAaTileW == kAaThreads, "a thread per tile pixel");

struct RoiCropAaArgs {
  const uint8_t* pixels;
  unsigned long long pixels_bytes;
  const tf2_image_src* srcs;
  const tf2_roi* rois;
  void* out;
  int32_t* status;
  int batch, OH, OW, plane, tiles_x, tiles_per_image;
  int pb, ch0, ch1, ch2;
  float mean0, mean1, mean2, scale0, scale1, scale2, trans;
};

// TF2_ROI_* bits of one slot (0: cropped); r receives the source record of an image inside the batch.  tf2_roi_crop's rule, then --
// only for a slot that rule passes -- the box inside the image (double on the float32 values; -0.0 is inside) and the scale bound on
// the float32 side the filter is built from
__device__ __forceinline__ int slot_status_aa(const RoiCropAaArgs& a, const tf2_roi& R, tf2_image_src& r) {
  if (R.image == -1) return TF2_ROI_EMPTY;
  int st = 0;
  if (R.image < 0 || R.image >= a.batch) st |= TF2_ROI_BAD_IMAGE;
  else {
    r = a.srcs[R.image];
    if (src_status(r, a.pb, a.pixels_bytes) != 0) st |= TF2_ROI_BAD_SRC;
  }
  if (!box_ok(R.x0, R.y0, R.x1, R.y1)) st |= TF2_ROI_BAD_BOX;
  if (st == 0) {
    if (!((double)R.x0 >= 0.0 && (double)R.x1 <= (double)r.w && (double)R.y0 >= 0.0 && (double)R.y1 <= (double)r.h))
      st |= TF2_ROI_BOX_OUTSIDE;
    if ((double)(R.x1 - R.x0) > (double)(kAaMaxScale * a.OW) || (double)(R.y1 - R.y0) > (double)(kAaMaxScale * a.OH))
      st |= TF2_ROI_BAD_SCALE;
  }
  return st;
}

template <bool OUT_Q>
__global__ __launch_bounds__(kAaThreads) void roi_crop_aa_kernel(RoiCropAaArgs a) {
  __shared__ int s_coef[kAaAxes][kAaMaxTaps];
  __shared__ double s_center[kAaAxes], s_ww[kAaAxes], s_ss[kAaAxes];
  __shared__ int s_lo[kAaAxes], s_n[kAaAxes];
  __shared__ int s_kc[2];                                          // ceil(support) along x, along y
  __shared__ uint32_t s_t[2][kAaChunk][kAaTileW];

  const int tid = threadIdx.x;
  const int s = blockIdx.x / a.tiles_per_image;
  const int tile = blockIdx.x - s * a.tiles_per_image;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int oy = tid / kAaTileW, ox = tid - oy * kAaTileW;
  const tf2_roi R = a.rois[s];
  tf2_image_src r{};
  const int st = slot_status_aa(a, R, r);
  if (tile == 0 && tid == 0) a.status[s] = st;

  int acc0 = kAaHalf, acc1 = kAaHalf, acc2 = kAaHalf;
  if (st == 0) {                                                   // (the same for the whole block)
    if (tid < kAaAxes) {                                           // bounds and weight sum of one column / one row
      const bool col = tid < kAaTileW;
      const int o = col ? tx * kAaTileW + tid : ty * kAaTileH + (tid - kAaTileW);
      const int n_in = col ? r.w : r.h;
      const float a0 = col ? R.x0 : R.y0;
      const AaAxis ax = aa_axis_box(a0, col ? R.x1 : R.y1, col ? a.OW : a.OH);
      double center = 0.0, ww = 0.0;
      int lo = 0, n = 0;
      if (o < (col ? a.OW : a.OH)) {                               // past the image: no taps, nothing read
        aa_bounds_box(ax, a0, o, n_in, center, lo, n);
        ww = aa_weight_sum(ax, center, lo, n);
      }
      s_center[tid] = center; s_ww[tid] = ww; s_ss[tid] = ax.ss; s_lo[tid] = lo; s_n[tid] = n;
      if (tid == 0 || tid == kAaTileW) s_kc[col ? 0 : 1] = (int)ceil(ax.support);   // 1 .. 32 for a slot that passed
    }
    __syncthreads();
    // the coefficients, (axis entry, tap) pairs spread over the block tap-major: n <= 2 * ceil(support) + 1 on an axis, so at 1x .. 2x
    // one sweep of the block covers the tile's 40 x 5 pairs
    const int kc = s_kc[0] > s_kc[1] ? s_kc[0] : s_kc[1];
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
    const long long at = (long long)s * 3 * a.plane + y * a.OW + x;
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

tf2_status roi_crop_aa(const Net& net2, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes,
                       const tf2_image_src* srcs, int batch, const tf2_roi* rois, int n_slots, int out_q, void* out, int32_t* status,
                       void* stream) {
  auto refuse = [](const std::string& m) { set_error("tf2_roi_crop_aa: " + m); return TF2_ERR_ARG; };
  const std::string why = preprocess_refusal(net2, d, batch, out_q, pixels && srcs && out && status && rois);
  if (!why.empty()) return refuse(why);
  if (n_slots < 1) return refuse("n_slots must be >= 1");

  RoiCropAaArgs a{};
  a.pixels = pixels; a.pixels_bytes = pixels_bytes; a.srcs = srcs; a.rois = rois; a.out = out; a.status = status;
  a.batch = batch; a.OH = net2.nd.image_h; a.OW = net2.nd.image_w; a.plane = a.OH * a.OW;
  a.tiles_x = (a.OW + kAaTileW - 1) / kAaTileW;
  a.tiles_per_image = a.tiles_x * ((a.OH + kAaTileH - 1) / kAaTileH);
  a.pb = d->pixel_bytes; a.ch0 = d->src_channel[0]; a.ch1 = d->src_channel[1]; a.ch2 = d->src_channel[2];
  a.mean0 = d->mean[0]; a.mean1 = d->mean[1]; a.mean2 = d->mean[2];
  a.scale0 = d->scale[0]; a.scale1 = d->scale[1]; a.scale2 = d->scale[2];
  a.trans = out_q ? std::ldexp(1.0f, -(int)net2.q[0]) : 1.0f;        // 2^-Q0, read now, as tf2_roi_crop does
  const long long blocks = (long long)n_slots * a.tiles_per_image;
  if (blocks > 0x7fffffffLL) return refuse("n_slots too large for one launch");
  const dim3 grid((unsigned)blocks), block(kAaThreads);
  hipStream_t s = (hipStream_t)stream;
  if (out_q) hipLaunchKernelGGL((roi_crop_aa_kernel<true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((roi_crop_aa_kernel<false>), grid, block, 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string("tf2_roi_crop_aa: launch failed: ") + hipGetErrorString(e)); return TF2_ERR_HIP; }
  return TF2_OK;
}

}  // namespace tf2
