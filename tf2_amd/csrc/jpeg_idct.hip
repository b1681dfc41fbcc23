// jpeg_idct.hip -- entropy-decoded JPEG coefficients -> the decoder's planes on the device (tf2_jpeg_idct, include/tf2_amd.h):
// dequantisation and libjpeg's integer "islow" inverse DCT of a batch of images, written where the tf2_ycc_src records of
// tf2_ycc_to_rgb (ycc_convert.hip) point.  tf2_amd/jpeg.py restates the arithmetic (jpeg.reference) and the device output is
// bit-identical to it.
//
// Streaming work: 128 bytes read and up to 64 written a block.  The grid is batch x blocks_per_image blocks of 256 threads whatever
// the records hold (a captured graph stays valid for new files of new sizes); a block validates its image's records, stages the
// image's quantisers in LDS, then walks the image's tiles of kJpegTileBH x kJpegTileBW coefficient blocks -- the tiles of the Y plane,
// then those of Cb and of Cr, over the blocks that hold samples of the plane -- with a stride of blocks_per_image.  Eight lanes share
// a coefficient block, a wave has the eight blocks of one tile row.  Pass 1: lane = column u, eight int16 loads (a wave reads the
// 1 KiB its blocks occupy), times the quantiser, the 1-D kernel down the column, the column into LDS (block pitch 72 dwords: lane l
// of block blk writes dword 72 * blk + 8 * k + l, so the 64 lanes of a wave land on the 64 different banks 8 * blk + l + 8 * k mod
// 64).  Pass 2: lane = row k, the row back as two 16-byte LDS reads, the 1-D kernel along it, eight clamped bytes out: a wave
// writes 64 contiguous bytes of eight plane rows, as two dwords a lane where the plane's offset and pitch allow and the run is
// whole, as bytes inside the plane otherwise.  The eight lanes that write a block's workspace are the eight lanes that read it, in
// one wave, so the block barrier between the passes and the two workspaces by tile parity are conservative: a wavefront-scope
// fence and one workspace would do (9.4 KB of LDS instead of 18.8).  No scratch, no atomics; every output byte is written once.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "jpeg_idct.h"

namespace tf2 {

namespace {

constexpr int kTileBlocks = kJpegTileBW * kJpegTileBH;
static_assert(kJpegTileBW == 8 && kTileBlocks * 8 == kJpegThreads, "a wave is one tile row of 8 blocks, 8 lanes a block");
constexpr int kWsPitch = 72;                     // dwords between the workspaces of two blocks (64 + 8)
constexpr int kJpegMaxSide = 32767;

struct JpegArgs {
  const int16_t* coef;
  unsigned long long coef_blocks;
  const tf2_jpeg_src* jpeg;
  const uint16_t* quant;
  uint8_t* planes;
  unsigned long long planes_bytes;
  const tf2_ycc_src* ycc;
  const tf2_image_src* srcs;
  int32_t* status;
  int blocks_per_image;
  int sx, sy;                                    // log2 of sub_x, sub_y (GRAY: 0)
};

__device__ __forceinline__ bool leaves(long long off, long long rows, long long pitch, long long row_bytes, unsigned long long bytes) {
  const unsigned long long span = (unsigned long long)((rows - 1) * pitch + row_bytes), o = (unsigned long long)off;
  return o > bytes || span > bytes - o;
}

template <typename T>
__device__ __forceinline__ T pick(int c, T v0, T v1, T v2) { return c == 0 ? v0 : (c == 1 ? v1 : v2); }

// TF2_JPEG_REC_* bits of image b's three records (0: its coefficients may be read and its planes written)
template <int NC>
__device__ __forceinline__ int jpeg_status(const tf2_image_src& r, const tf2_ycc_src& p, const tf2_jpeg_src& j, const JpegArgs& a) {
  const long long cw = ((long long)r.w + (1 << a.sx) - 1) >> a.sx, ch = ((long long)r.h + (1 << a.sy) - 1) >> a.sy;
  int st = 0;
  if (r.h < 1 || r.h > kJpegMaxSide || r.w < 1 || r.w > kJpegMaxSide) st |= TF2_JPEG_REC_BAD_SIZE;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const long long pw = c ? cw : r.w, ph = c ? ch : r.h;
    if (j.bw[c] < 1 || j.bh[c] < 1 || 8LL * j.bw[c] < pw || 8LL * j.bh[c] < ph) st |= TF2_JPEG_REC_BAD_GRID;
    if (j.block_off[c] < 0) st |= TF2_JPEG_REC_BAD_OFFSET;
  }
  if (p.pitch_y < r.w || (NC == 3 && p.pitch_c < cw)) st |= TF2_JPEG_REC_BAD_PITCH;
  if (p.off_y < 0 || (NC == 3 && (p.off_cb < 0 || p.off_cr < 0))) st |= TF2_JPEG_REC_BAD_OFFSET;
  if (st == 0) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const unsigned long long off = (unsigned long long)j.block_off[c], n = (unsigned long long)((long long)j.bw[c] * j.bh[c]);
      if (off > a.coef_blocks || n > a.coef_blocks - off) st |= TF2_JPEG_REC_OUT_OF_COEF;
    }
    if (leaves(p.off_y, r.h, p.pitch_y, r.w, a.planes_bytes) ||
        (NC == 3 && (leaves(p.off_cb, ch, p.pitch_c, cw, a.planes_bytes) || leaves(p.off_cr, ch, p.pitch_c, cw, a.planes_bytes))))
      st |= TF2_JPEG_REC_OUT_OF_PLANES;
  }
  return st;
}

// the 1-D kernel K(x0..x7; S) of include/tf2_amd.h, in place; unsigned: sums, products and shifts wrap modulo 2^32
template <int S>
__device__ __forceinline__ void idct8(uint32_t (&x)[8]) {
  uint32_t z1 = (x[2] + x[6]) * 4433u;
  const uint32_t t2 = z1 - x[6] * 15137u, t3 = z1 + x[2] * 6270u;
  const uint32_t t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
  const uint32_t a0 = t0 + t3, a3 = t0 - t3, a1 = t1 + t2, a2 = t1 - t2;
  uint32_t b0 = x[7], b1 = x[5], b2 = x[3], b3 = x[1];
  z1 = b0 + b3;
  uint32_t z2 = b1 + b2, z3 = b0 + b2, z4 = b1 + b3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  b0 *= 2446u; b1 *= 16819u; b2 *= 25172u; b3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5;
  z4 = z4 * (uint32_t)-3196 + z5;
  b0 += z1 + z3; b1 += z2 + z4; b2 += z2 + z3; b3 += z1 + z4;
  constexpr uint32_t half = 1u << (S - 1);
  x[0] = (uint32_t)((int32_t)(a0 + b3 + half) >> S);
  x[1] = (uint32_t)((int32_t)(a1 + b2 + half) >> S);
  x[2] = (uint32_t)((int32_t)(a2 + b1 + half) >> S);
  x[3] = (uint32_t)((int32_t)(a3 + b0 + half) >> S);
  x[4] = (uint32_t)((int32_t)(a3 - b0 + half) >> S);
  x[5] = (uint32_t)((int32_t)(a2 - b1 + half) >> S);
  x[6] = (uint32_t)((int32_t)(a1 - b2 + half) >> S);
  x[7] = (uint32_t)((int32_t)(a0 - b3 + half) >> S);
}

__device__ __forceinline__ uint32_t sample(uint32_t v) {
  const int s = (int32_t)v + 128;
  return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

struct __attribute__((aligned(4))) Row8 { uint32_t lo, hi; };

template <int NC>
__global__ __launch_bounds__(kJpegThreads) void jpeg_idct_kernel(JpegArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t ws[2][kTileBlocks][kWsPitch];
  __shared__ uint16_t qs[3 * 64];
  const int b = blockIdx.x / a.blocks_per_image, first = blockIdx.x - b * a.blocks_per_image;
  const tf2_image_src r = a.srcs[b];
  const tf2_ycc_src p = a.ycc[b];
  const tf2_jpeg_src j = a.jpeg[b];
  const int st = jpeg_status<NC>(r, p, j, a);
  if (first == 0 && threadIdx.x == 0) a.status[b] = st;
  if (st != 0) return;                            // (the whole block: nothing of the image is read or written)

  if (threadIdx.x < NC * 64) qs[threadIdx.x] = a.quant[(long long)b * 192 + threadIdx.x];
  __syncthreads();

  const int cw = (r.w + (1 << a.sx) - 1) >> a.sx, ch = (r.h + (1 << a.sy) - 1) >> a.sy;
  // blocks that hold samples of a plane, and the tiles over them
  const int nbx0 = (r.w + 7) >> 3, nby0 = (r.h + 7) >> 3, nbxc = (cw + 7) >> 3, nbyc = (ch + 7) >> 3;
  const int tx0 = (nbx0 + kJpegTileBW - 1) / kJpegTileBW, txc = (nbxc + kJpegTileBW - 1) / kJpegTileBW;
  const int tiles0 = tx0 * ((nby0 + kJpegTileBH - 1) / kJpegTileBH), tilesc = txc * ((nbyc + kJpegTileBH - 1) / kJpegTileBH);
  const int tiles = NC == 3 ? tiles0 + 2 * tilesc : tiles0;
  const int l = threadIdx.x & 7, blk = threadIdx.x >> 3;
  const int bxl = blk & (kJpegTileBW - 1), byl = blk / kJpegTileBW;

  int buf = 0;
  for (int tile = first; tile < tiles; tile += a.blocks_per_image, buf ^= 1) {
    int c = 0, t = tile;
    if (NC == 3 && t >= tiles0) {
      t -= tiles0;
      c = 1;
      if (t >= tilesc) { t -= tilesc; c = 2; }
    }
    const int pw = c ? cw : r.w, ph = c ? ch : r.h, nbx = c ? nbxc : nbx0, nby = c ? nbyc : nby0, tx = c ? txc : tx0;
    const int tyi = t / tx, bx = (t - tyi * tx) * kJpegTileBW + bxl, by = tyi * kJpegTileBH + byl;
    const bool active = bx < nbx && by < nby;     // (nbx <= bw and nby <= bh: the grid test of jpeg_status)
    uint32_t x[8];
    if (active) {
      const long long at = pick(c, j.block_off[0], j.block_off[1], j.block_off[2]) + (long long)by * pick(c, j.bw[0], j.bw[1], j.bw[2]) + bx;
      const int16_t* const cp = a.coef + at * 64 + l;
      const uint16_t* const qp = qs + c * 64 + l;
#pragma unroll
      for (int k = 0; k < 8; k++) x[k] = (uint32_t)(int32_t)cp[8 * k] * (uint32_t)qp[8 * k];
      idct8<11>(x);
#pragma unroll
      for (int k = 0; k < 8; k++) ws[buf][blk][8 * k + l] = x[k];
    }
    __syncthreads();                              // (tiles is the same for every thread of the block)
    if (!active) continue;
    const uint4 lo = *reinterpret_cast<const uint4*>(&ws[buf][blk][8 * l]), hi = *reinterpret_cast<const uint4*>(&ws[buf][blk][8 * l + 4]);
    x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
    idct8<18>(x);
    const int y = by * 8 + l, x0 = bx * 8;
    if (y >= ph) continue;
    uint8_t* const base = a.planes + pick(c, p.off_y, p.off_cb, p.off_cr);
    const int pitch = c ? p.pitch_c : p.pitch_y;
    uint8_t* const dp = base + (long long)y * pitch + x0;
    const bool vec = (((uintptr_t)base | (uintptr_t)(unsigned)pitch) & 3) == 0;
    if (vec && x0 + 7 < pw) {
      *reinterpret_cast<Row8*>(dp) = Row8{sample(x[0]) | sample(x[1]) << 8 | sample(x[2]) << 16 | sample(x[3]) << 24,
                                          sample(x[4]) | sample(x[5]) << 8 | sample(x[6]) << 16 | sample(x[7]) << 24};
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++)
        if (x0 + k < pw) dp[k] = (uint8_t)sample(x[k]);
    }
  }
}

}  // namespace

tf2_status jpeg_idct(const tf2_jpeg_desc* d, const int16_t* coef, size_t coef_blocks, const tf2_jpeg_src* jpeg, const uint16_t* quant,
                     uint8_t* planes, size_t planes_bytes, const tf2_ycc_src* ycc, const tf2_image_src* srcs, int batch,
                     int32_t* status, void* stream) {
  auto refuse = [](const std::string& m) { return arg_refusal("tf2_jpeg_idct", m); };
  if (!d) return refuse("null desc");
  if (d->size != sizeof(tf2_jpeg_desc)) return refuse("desc size " + std::to_string(d->size) + ", expected sizeof(tf2_jpeg_desc)");
  if (d->layout != TF2_YCC_PLANAR && d->layout != TF2_YCC_GRAY) return refuse("layout must be TF2_YCC_PLANAR or TF2_YCC_GRAY");
  const bool gray = d->layout == TF2_YCC_GRAY;
  if (!gray && !((d->sub_x == 1 && d->sub_y == 1) || (d->sub_x == 2 && d->sub_y == 1) || (d->sub_x == 2 && d->sub_y == 2)))
    return refuse("(sub_x, sub_y) must be (1,1), (2,1) or (2,2)");
  if (d->blocks_per_image < 0) return refuse("blocks_per_image must be >= 0");
  if (batch < 1) return refuse("batch must be >= 1");
  if (!coef || !jpeg || !quant || !planes || !ycc || !srcs || !status) return refuse("null device pointer");
  {
    if (coef_blocks > (SIZE_MAX >> 7)) return refuse("coef_blocks * 128 wraps");
    const uintptr_t c0 = (uintptr_t)coef, p0 = (uintptr_t)planes;
    const size_t coef_bytes = coef_blocks * 128;
    if (coef_bytes > UINTPTR_MAX - c0 || planes_bytes > UINTPTR_MAX - p0) return refuse("a buffer wraps the address space");
    if (c0 < p0 + planes_bytes && p0 < c0 + coef_bytes) return refuse("the coefficient and the plane buffer overlap");
  }

  JpegArgs a{};
  a.coef = coef; a.coef_blocks = coef_blocks; a.jpeg = jpeg; a.quant = quant; a.planes = planes; a.planes_bytes = planes_bytes;
  a.ycc = ycc; a.srcs = srcs; a.status = status;
  a.blocks_per_image = d->blocks_per_image ? d->blocks_per_image : jpeg_default_blocks_per_image(batch);
  a.sx = gray ? 0 : d->sub_x - 1;
  a.sy = gray ? 0 : d->sub_y - 1;
  const long long blocks = (long long)batch * a.blocks_per_image;
  if (blocks > 0x7fffffffLL) return refuse("batch * blocks_per_image too large for one launch");
  const dim3 grid((unsigned)blocks), block(kJpegThreads);
  if (gray) hipLaunchKernelGGL((jpeg_idct_kernel<1>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((jpeg_idct_kernel<3>), grid, block, 0, (hipStream_t)stream, a);
  return launch_result("tf2_jpeg_idct");
}

}  // namespace tf2
