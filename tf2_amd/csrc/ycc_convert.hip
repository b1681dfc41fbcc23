// ycc_convert.hip -- decoder planes -> interleaved pixels on the device (tf2_ycc_to_rgb, include/tf2_amd.h): chroma upsampling
// (libjpeg's "fancy" triangle filter or replication) and the YCbCr -> RGB conversion (libjpeg's jdcolor fixed point, or limited-range
// BT.601 / BT.709 in the same fixed point) of a batch of planar / semi-planar 8-bit frames, written where the tf2_image_src records of
// the gather kernels (preprocess.hip, preprocess_aa.hip, roi_crop.hip) point.  tf2_amd/ycc.py restates the arithmetic (ycc.reference)
// and the device output is bit-identical to it.
//
// Streaming work: 1.5 to 3 bytes read and 3 or 4 written a pixel.  The grid is batch x blocks_per_image blocks of 256 threads whatever
// the records hold (a captured graph stays valid for new frames of new sizes); a block validates its image's records, then walks the
// image's kYccTileH x kYccTileW tiles with a stride of blocks_per_image.  Per tile the block stages the chroma rows the tile needs
// (one row and four columns of halo around it, clamped to the plane, so the filter's edge cases are the general formula on repeated
// samples) into LDS once, as dwords where the plane's offset and pitch allow and as bytes otherwise; then a thread makes 4 pixels
// of two rows: 4 Y bytes (one dword where aligned), the staged chroma through two LDS dwords, 12 or 16 bytes out (dwords where the
// destination's offset and pitch allow and the run is whole, bytes otherwise).  LDS is double-buffered by tile parity: one barrier
// a tile.  No scratch, no atomics; every output byte is written once.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "ycc_convert.h"

namespace tf2 {

namespace {

enum { kModeGray = 0, kModePoint = 1, kModeH2V1 = 2, kModeH2V2 = 3 };   // how a pixel's chroma comes out of the staged rows

constexpr int kTX = kYccTileW / 4;               // 32 threads along a row, 4 pixels each
constexpr int kTY = kYccThreads / kTX;           // 8 thread rows, 2 output rows each
static_assert(kTY * 2 == kYccTileH && (kTX & (kTX - 1)) == 0, "tile shape");
constexpr int kHalo = 4;                         // staged columns in front of the tile's first chroma column (a whole dword)
constexpr int kLdsSlots = kYccTileW / 4 + 2;     // dwords of a staged row: halo, up to kYccTileW columns, halo
constexpr int kLdsRows = kYccTileH + 2;          // staged rows: one above, up to kYccTileH, one below
constexpr int kYccMaxSide = 32767;

struct YccArgs {
  const uint8_t* src;
  unsigned long long src_bytes;
  const tf2_ycc_src* ycc;
  uint8_t* pixels;
  unsigned long long pixels_bytes;
  const tf2_image_src* srcs;
  int32_t* status;
  int blocks_per_image;
  int layout, sx, sy;                            // sx, sy: log2 of sub_x, sub_y (GRAY: 0)
  int ky, yoff, r_cr, g_cb, g_cr, b_cb;          // channel = (ky * (Y - yoff) + c_cb * cb + c_cr * cr + 32768) >> 16
  int sh_r, sh_g, sh_b;                          // bit positions of R, G, B in a packed pixel
  unsigned alpha_bits;                           // alpha at its position (pixel_bytes == 4)
};

__device__ __forceinline__ bool leaves(long long off, long long rows, long long pitch, long long row_bytes, unsigned long long bytes) {
  const unsigned long long span = (unsigned long long)((rows - 1) * pitch + row_bytes), o = (unsigned long long)off;
  return o > bytes || span > bytes - o;
}

// TF2_YCC_* bits of image b's two records (0: its planes may be read and its pixels written)
__device__ __forceinline__ int ycc_status(const tf2_image_src& r, const tf2_ycc_src& p, const YccArgs& a, int pb) {
  const bool chroma = a.layout != TF2_YCC_GRAY, planar = a.layout == TF2_YCC_PLANAR;
  const long long cw = ((long long)r.w + (1 << a.sx) - 1) >> a.sx, ch = ((long long)r.h + (1 << a.sy) - 1) >> a.sy;
  const long long crow = planar ? cw : 2 * cw;
  int st = 0;
  if (r.h < 1 || r.h > kYccMaxSide || r.w < 1 || r.w > kYccMaxSide) st |= TF2_YCC_BAD_SIZE;
  if ((long long)r.row_pitch < (long long)r.w * pb || p.pitch_y < r.w || (chroma && p.pitch_c < crow)) st |= TF2_YCC_BAD_PITCH;
  if (r.offset < 0 || p.off_y < 0 || (chroma && p.off_cb < 0) || (planar && p.off_cr < 0)) st |= TF2_YCC_BAD_OFFSET;
  if (st == 0) {
    if (leaves(p.off_y, r.h, p.pitch_y, r.w, a.src_bytes) || (chroma && leaves(p.off_cb, ch, p.pitch_c, crow, a.src_bytes)) ||
        (planar && leaves(p.off_cr, ch, p.pitch_c, crow, a.src_bytes)))
      st |= TF2_YCC_OUT_OF_SRC;
    if (leaves(r.offset, r.h, r.row_pitch, (long long)r.w * pb, a.pixels_bytes)) st |= TF2_YCC_OUT_OF_DST;
  }
  return st;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int byte_of(uint32_t q, int t) { return (int)((q >> (8 * t)) & 0xffu); }

// chroma columns j .. j + 3 (j a multiple of 4, possibly outside 0..cw-1: clamped) of chroma row `row` (inside the plane), both
// planes, four bytes each; vec: offsets and pitch are multiples of 4, so a run inside the row is read as dwords
__device__ __forceinline__ void load_chroma4(const uint8_t* src, const tf2_ycc_src& p, int layout, int row, int j, int cw, bool vec,
                                             uint32_t& cb, uint32_t& cr) {
  const bool whole = vec && j >= 0 && j + 3 < cw;
  if (layout == TF2_YCC_PLANAR) {
    const uint8_t* const b0 = src + p.off_cb + (long long)row * p.pitch_c;
    const uint8_t* const b1 = src + p.off_cr + (long long)row * p.pitch_c;
    if (whole) {
      cb = *reinterpret_cast<const uint32_t*>(b0 + j);
      cr = *reinterpret_cast<const uint32_t*>(b1 + j);
    } else {
      cb = cr = 0;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int jj = clampi(j + t, 0, cw - 1);
        cb |= (uint32_t)b0[jj] << (8 * t);
        cr |= (uint32_t)b1[jj] << (8 * t);
      }
    }
  } else {
    const uint8_t* const b0 = src + p.off_cb + (long long)row * p.pitch_c;
    uint32_t first, second;                       // the first and the second byte of the four pairs
    if (whole) {
      const uint32_t d0 = *reinterpret_cast<const uint32_t*>(b0 + 2 * j), d1 = *reinterpret_cast<const uint32_t*>(b0 + 2 * j + 4);
      first = (d0 & 0xffu) | ((d0 >> 16) & 0xffu) << 8 | (d1 & 0xffu) << 16 | ((d1 >> 16) & 0xffu) << 24;
      second = ((d0 >> 8) & 0xffu) | (d0 >> 24) << 8 | ((d1 >> 8) & 0xffu) << 16 | (d1 >> 24) << 24;
    } else {
      first = second = 0;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int jj = clampi(j + t, 0, cw - 1);
        first |= (uint32_t)b0[2 * jj] << (8 * t);
        second |= (uint32_t)b0[2 * jj + 1] << (8 * t);
      }
    }
    cb = layout == TF2_YCC_SEMI_CBCR ? first : second;
    cr = layout == TF2_YCC_SEMI_CBCR ? second : first;
  }
}

// four staged bytes of a row from byte b on
__device__ __forceinline__ uint32_t lds4(const uint32_t* row, int b) {
  const uint32_t lo = row[b >> 2], hi = row[(b >> 2) + 1];
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> ((b & 3) * 8));
}

struct __attribute__((aligned(4))) Px12 { uint32_t a, b, c; };
struct __attribute__((aligned(4))) Px16 { uint32_t a, b, c, d; };

template <int PB, int MODE>
__global__ __launch_bounds__(kYccThreads) void ycc_to_rgb_kernel(YccArgs a) {
  __shared__ uint32_t lds[2][2][kLdsRows][kLdsSlots];
  const int b = blockIdx.x / a.blocks_per_image, first = blockIdx.x - b * a.blocks_per_image;
  const tf2_image_src r = a.srcs[b];
  const tf2_ycc_src p = a.ycc[b];
  const int st = ycc_status(r, p, a, PB);
  if (first == 0 && threadIdx.x == 0) a.status[b] = st;
  if (st != 0) return;                            // (the whole block: nothing of the image is read or written)

  const int h = r.h, w = r.w;
  const int cw = (w + (1 << a.sx) - 1) >> a.sx, ch = (h + (1 << a.sy) - 1) >> a.sy;
  const int tiles_x = (w + kYccTileW - 1) / kYccTileW, tiles = tiles_x * ((h + kYccTileH - 1) / kYccTileH);
  const uint8_t* const ybase = a.src + p.off_y;
  uint8_t* const dbase = a.pixels + r.offset;
  const bool yvec = (((uintptr_t)ybase | (uintptr_t)(unsigned)p.pitch_y) & 3) == 0;
  const bool dvec = (((uintptr_t)dbase | (uintptr_t)(unsigned)r.row_pitch) & 3) == 0;
  const bool cvec = MODE != kModeGray &&
                    (((uintptr_t)(a.src + p.off_cb) | (uintptr_t)(unsigned)p.pitch_c |
                      (a.layout == TF2_YCC_PLANAR ? (uintptr_t)(a.src + p.off_cr) : (uintptr_t)0)) & 3) == 0;
  const int tx = threadIdx.x & (kTX - 1), ty = threadIdx.x / kTX;
  const int nslots = ((kYccTileW >> a.sx) >> 2) + 2, nrows = (kYccTileH >> a.sy) + 2;

  int buf = 0;
  for (int tile = first; tile < tiles; tile += a.blocks_per_image, buf ^= 1) {
    const int tyi = tile / tiles_x, x0 = (tile - tyi * tiles_x) * kYccTileW, y0 = tyi * kYccTileH;
    if (MODE != kModeGray) {
      const int c0 = x0 >> a.sx, r0 = y0 >> a.sy;
      for (int it = threadIdx.x; it < nrows * nslots; it += kYccThreads) {
        const int i = it / nslots, jd = it - i * nslots;
        uint32_t cb, cr;
        load_chroma4(a.src, p, a.layout, clampi(r0 - 1 + i, 0, ch - 1), c0 - kHalo + 4 * jd, cw, cvec, cb, cr);
        lds[buf][0][i][jd] = cb;
        lds[buf][1][i][jd] = cr;
      }
      __syncthreads();                            // (tiles is the same for every thread of the block)
    }
    const int x = x0 + 4 * tx;
    if (x >= w) continue;
    const bool whole = x + 3 < w;
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
      const int yl = 2 * ty + dy, y = y0 + yl;
      if (y >= h) continue;
      // -- luma
      const uint8_t* const yp = ybase + (long long)y * p.pitch_y + x;
      uint32_t yq;
      if (yvec && whole) {
        yq = *reinterpret_cast<const uint32_t*>(yp);
      } else {
        yq = 0;
#pragma unroll
        for (int t = 0; t < 4; t++)
          if (x + t < w) yq |= (uint32_t)yp[t] << (8 * t);
      }
      // -- chroma of the four pixels
      int c[2][4];
#pragma unroll
      for (int pl = 0; pl < 2; pl++) {
        if (MODE == kModeGray) {
#pragma unroll
          for (int t = 0; t < 4; t++) c[pl][t] = 128;
        } else if (MODE == kModePoint) {
          const uint32_t q = lds4(lds[buf][pl][1 + (yl >> a.sy)], kHalo + ((4 * tx) >> a.sx));
#pragma unroll
          for (int t = 0; t < 4; t++) c[pl][t] = byte_of(q, a.sx ? t >> 1 : t);
        } else if (MODE == kModeH2V1) {
          const uint32_t q = lds4(lds[buf][pl][1 + yl], kHalo - 1 + 2 * tx);
          const int pm = byte_of(q, 0), p0 = byte_of(q, 1), p1 = byte_of(q, 2), p2 = byte_of(q, 3);
          c[pl][0] = (3 * p0 + pm + 1) >> 2;
          c[pl][1] = (3 * p0 + p1 + 2) >> 2;
          c[pl][2] = (3 * p1 + p0 + 1) >> 2;
          c[pl][3] = (3 * p1 + p2 + 2) >> 2;
        } else {
          const uint32_t qa = lds4(lds[buf][pl][1 + ty], kHalo - 1 + 2 * tx);
          const uint32_t qo = lds4(lds[buf][pl][dy == 0 ? ty : 2 + ty], kHalo - 1 + 2 * tx);
          int s[4];
#pragma unroll
          for (int t = 0; t < 4; t++) s[t] = 3 * byte_of(qa, t) + byte_of(qo, t);
          c[pl][0] = (3 * s[1] + s[0] + 8) >> 4;
          c[pl][1] = (3 * s[1] + s[2] + 7) >> 4;
          c[pl][2] = (3 * s[2] + s[1] + 8) >> 4;
          c[pl][3] = (3 * s[2] + s[3] + 7) >> 4;
        }
      }
      // -- colour, packed pixels
      uint32_t px[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int base = a.ky * (byte_of(yq, t) - a.yoff) + 32768, cb = c[0][t] - 128, cr = c[1][t] - 128;
        const int R = clampi((base + a.r_cr * cr) >> 16, 0, 255);
        const int G = clampi((base + a.g_cb * cb + a.g_cr * cr) >> 16, 0, 255);
        const int B = clampi((base + a.b_cb * cb) >> 16, 0, 255);
        px[t] = (uint32_t)R << a.sh_r | (uint32_t)G << a.sh_g | (uint32_t)B << a.sh_b | a.alpha_bits;
      }
      // -- out: PB * 4 bytes as dwords, or the bytes of the pixels inside the row
      uint8_t* const dp = dbase + (long long)y * r.row_pitch + (long long)x * PB;
      if (dvec && whole) {
        if (PB == 4) *reinterpret_cast<Px16*>(dp) = Px16{px[0], px[1], px[2], px[3]};
        else *reinterpret_cast<Px12*>(dp) = Px12{px[0] | px[1] << 24, px[1] >> 8 | px[2] << 16, px[2] >> 16 | px[3] << 8};
      } else {
#pragma unroll
        for (int t = 0; t < 4; t++)
          if (x + t < w) {
#pragma unroll
            for (int k = 0; k < PB; k++) dp[t * PB + k] = (uint8_t)(px[t] >> (8 * k));
          }
      }
    }
  }
}

constexpr int fix16(double v) { return (int)(v * 65536.0 + 0.5); }

template <int PB>
void launch(int mode, dim3 grid, hipStream_t s, const YccArgs& a) {
  const dim3 block(kYccThreads);
  switch (mode) {
    case kModeGray: hipLaunchKernelGGL((ycc_to_rgb_kernel<PB, kModeGray>), grid, block, 0, s, a); break;
    case kModePoint: hipLaunchKernelGGL((ycc_to_rgb_kernel<PB, kModePoint>), grid, block, 0, s, a); break;
    case kModeH2V1: hipLaunchKernelGGL((ycc_to_rgb_kernel<PB, kModeH2V1>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((ycc_to_rgb_kernel<PB, kModeH2V2>), grid, block, 0, s, a); break;
  }
}

}  // namespace

tf2_status ycc_to_rgb(const tf2_ycc_desc* d, const uint8_t* src, size_t src_bytes, const tf2_ycc_src* ycc, uint8_t* pixels,
                      size_t pixels_bytes, const tf2_image_src* srcs, int batch, int32_t* status, void* stream) {
  auto refuse = [](const std::string& m) { return arg_refusal("tf2_ycc_to_rgb", m); };
  if (!d) return refuse("null desc");
  if (d->size != sizeof(tf2_ycc_desc)) return refuse("desc size " + std::to_string(d->size) + ", expected sizeof(tf2_ycc_desc)");
  if (d->layout < TF2_YCC_PLANAR || d->layout > TF2_YCC_GRAY) return refuse("layout must be TF2_YCC_PLANAR, _SEMI_CBCR, _SEMI_CRCB or _GRAY");
  const bool gray = d->layout == TF2_YCC_GRAY;
  if (!gray && !((d->sub_x == 1 && d->sub_y == 1) || (d->sub_x == 2 && d->sub_y == 1) || (d->sub_x == 2 && d->sub_y == 2)))
    return refuse("(sub_x, sub_y) must be (1,1), (2,1) or (2,2)");
  if (d->upsample != TF2_YCC_FANCY && d->upsample != TF2_YCC_REPLICATE) return refuse("upsample must be TF2_YCC_FANCY or TF2_YCC_REPLICATE");
  if (d->matrix < TF2_YCC_JFIF || d->matrix > TF2_YCC_BT709) return refuse("matrix must be TF2_YCC_JFIF, TF2_YCC_BT601 or TF2_YCC_BT709");
  if (d->pixel_bytes != 3 && d->pixel_bytes != 4) return refuse("pixel_bytes must be 3 or 4");
  for (int c = 0; c < 3; c++)
    if (d->dst_channel[c] < 0 || d->dst_channel[c] >= d->pixel_bytes) return refuse("dst_channel[" + std::to_string(c) + "] outside 0..pixel_bytes-1");
  if (d->dst_channel[0] == d->dst_channel[1] || d->dst_channel[0] == d->dst_channel[2] || d->dst_channel[1] == d->dst_channel[2])
    return refuse("dst_channel values must be distinct");
  if (d->alpha < 0 || d->alpha > 255) return refuse("alpha must be 0..255");
  if (d->blocks_per_image < 0) return refuse("blocks_per_image must be >= 0");
  if (batch < 1) return refuse("batch must be >= 1");
  if (!src || !ycc || !pixels || !srcs || !status) return refuse("null device pointer");
  {
    const uintptr_t s0 = (uintptr_t)src, p0 = (uintptr_t)pixels;
    if (src_bytes > UINTPTR_MAX - s0 || pixels_bytes > UINTPTR_MAX - p0) return refuse("a buffer wraps the address space");
    if (s0 < p0 + pixels_bytes && p0 < s0 + src_bytes) return refuse("the source and the pixel buffer overlap");
  }

  YccArgs a{};
  a.src = src; a.src_bytes = src_bytes; a.ycc = ycc; a.pixels = pixels; a.pixels_bytes = pixels_bytes; a.srcs = srcs; a.status = status;
  a.blocks_per_image = d->blocks_per_image ? d->blocks_per_image : ycc_default_blocks_per_image(batch);
  a.layout = d->layout;
  a.sx = gray ? 0 : d->sub_x - 1;
  a.sy = gray ? 0 : d->sub_y - 1;
  switch (d->matrix) {
    case TF2_YCC_JFIF:
      a.ky = 65536; a.yoff = 0;                   // Y + (t >> 16) == (65536 * Y + t) >> 16
      a.r_cr = fix16(1.40200); a.g_cb = -fix16(0.34414); a.g_cr = -fix16(0.71414); a.b_cb = fix16(1.77200);
      break;
    case TF2_YCC_BT601:
      a.ky = fix16(1.164383); a.yoff = 16;
      a.r_cr = fix16(1.596027); a.g_cb = -fix16(0.391762); a.g_cr = -fix16(0.812968); a.b_cb = fix16(2.017232);
      break;
    default:
      a.ky = fix16(1.164384); a.yoff = 16;
      a.r_cr = fix16(1.792741); a.g_cb = -fix16(0.213249); a.g_cr = -fix16(0.532909); a.b_cb = fix16(2.112402);
      break;
  }
  a.sh_r = 8 * d->dst_channel[0]; a.sh_g = 8 * d->dst_channel[1]; a.sh_b = 8 * d->dst_channel[2];
  a.alpha_bits = d->pixel_bytes == 4 ? (unsigned)d->alpha << (8 * (6 - d->dst_channel[0] - d->dst_channel[1] - d->dst_channel[2])) : 0u;
  const int mode = gray ? kModeGray
                        : (d->upsample == TF2_YCC_REPLICATE || d->sub_x == 1) ? kModePoint : (d->sub_y == 1 ? kModeH2V1 : kModeH2V2);
  const long long blocks = (long long)batch * a.blocks_per_image;
  if (blocks > 0x7fffffffLL) return refuse("batch * blocks_per_image too large for one launch");
  const dim3 grid((unsigned)blocks);
  if (d->pixel_bytes == 4) launch<4>(mode, grid, (hipStream_t)stream, a);
  else launch<3>(mode, grid, (hipStream_t)stream, a);
  return launch_result("tf2_ycc_to_rgb");
}

}  // namespace tf2
