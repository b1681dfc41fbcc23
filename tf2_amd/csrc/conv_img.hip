// conv_img.hip -- a k x k / stride 1 / pad (k - 1) / 2 row on a SMALL square map (ResNet-50's 7 x 7 x 512 3x3 rows), whole images per
// block: the input stays in LDS, the weights go straight into registers, the block's eight waves split K (gfx950).
//
// Why not conv_mfma_sk for these rows: its four waves each run an LDS-DMA ring for BOTH operands, so every pixel's 512 bytes are
// gathered from L2 once per tap (nine times) and the weights make an LDS round trip as well -- a 64 x 64 output tile moves
// (64 + 64) x 4608 bytes through the ring for ~2 us of MFMA.  Why not conv_c3: it has no split over K; on a map of 49 pixels its
// grid is a few dozen blocks that each walk all 72 slabs in sequence.  Here:
//
//   * a block owns one 64-row m-tile of the packed image and G = 2 whole images (98 pixels = four 32-pixel column tiles, the last one
//     ragged; the last block of an odd batch holds one image);
//   * prologue: the m-tile's header rows and the block's input -- per image the zero-padded (H + 2) x (W + 2) map, border positions
//     filled from the row's stored zero (ConvArgs::zero: the pad row of a doubled tensor, else the zero page) -- go global -> LDS by
//     LDS-DMA, once.  Layout: lds_tile.h's, as conv_bneck's halo tile (per 64-channel slab 64 bytes per pixel, the four 16-byte chunks XOR-swizzled by
//     pixel so that a tap's shifted reads spread over the banks): one DMA instruction then covers 16 pixels x 64 contiguous bytes --
//     16 half cache lines.  (Four 16-byte planes per slab, conv_bband's mid1 layout, would make a tap an immediate offset, but a DMA
//     instruction fills 1 KiB of ONE plane: 64 lanes on 64 different cache lines for 16 bytes each, four times the line requests of
//     the prologue -- and the prologue is the serial part of a block that lives a few microseconds.)
//   * K loop: the (window, tap, slab) list is split over the eight waves, window-major (two-window rows: waves 0-3 the high window,
//     4-7 the low one).  Each wave accumulates the WHOLE 64-channel x 128-pixel tile for its part: 2 x 4 MFMA tiles, 128 accumulator
//     registers; a B fragment (one ds_read_b128) feeds two MFMAs.  Weight fragments come from the packed tiles two steps ahead
//     (conv_bneck's scheme, same tiles: nothing is repacked).  No barrier, no DMA inside the loop;
//   * combining: behind one barrier the partial int32 tiles are summed through LDS over the input tile's space, in two hand-overs
//     (eight 32 KiB partial tiles do not fit at once): waves 4-7 store theirs, wave w < 4 adds wave (w + 4)'s to its own -- two-window
//     rows: (hi << dshift) + lo per K part, which sums to ((sum hi) << dshift) + (sum lo) in Z/2^32, conv_mfma_sk's combination and
//     exactness argument -- and stores the sum in the same slot (only wave w reads slot w, so it may overwrite it); then every wave
//     adds up ONE of the eight 32 x 32 tiles from the four slots, requantises it (requant_epilogue.h as it stands) and stores 16-byte
//     NHWC groups.
//
// Nothing a block reads is written by another block of the launch, and nothing is exchanged between blocks: the launch has none of the
// group launches' preconditions and may share the chip with anything.  Plain vector stores only.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "tf2_internal.h"
#include "tf2_device.h"
#include "requant_epilogue.h"
#include "lds_tile.h"

namespace tf2 {

constexpr int kImgG = 2;                 // images per block
constexpr int kImgWaves = 8;

// the geometry of one instantiation, shared by the kernel, the launcher and conv_img_lds_bytes
template <int HW, int C, int KS>
struct ImgShape {
  static constexpr int PAD = (KS - 1) / 2, HP = HW + 2 * PAD;
  static constexpr int NPIX = HW * HW, NHALO = HP * HP;
  static constexpr int NSL = C / 64, NE = KS * KS * NSL;                // 64-byte slabs of a pixel, (tap, slab) entries of an m-tile
  static constexpr int NT = (kImgG * NPIX + 31) / 32;                   // 32-pixel column tiles of a block
  static constexpr int HGRP = (kImgG * NHALO + 15) / 16;                // 16-pixel DMA groups of a slab of the input tile
  static constexpr int SLABB = HGRP * 1024;                             // bytes of one slab of the input tile
  static constexpr int TILE_BYTES = NSL * SLABB;
  static constexpr int PART_BYTES = 64 * NT * 32 * 4;                   // one wave's partial tile
  static constexpr int PRM_OFF = TILE_BYTES > 4 * PART_BYTES ? TILE_BYTES : 4 * PART_BYTES;      // the header rows: behind both uses of the space in front
  static_assert(C % 64 == 0 && (KS == 1 || KS == 3), "instantiated forms");
  static_assert(NE % kImgWaves == 0, "the entry list splits evenly over the waves (both window forms)");
  static_assert(NT == 4, "eight waves finish eight 32 x 32 tiles: two row tiles x four column tiles");
};

template <int HW, int C, int KS, bool DUAL>
__global__ __launch_bounds__(512) void conv_img_kernel(ImgArgs a) {
  using S = ImgShape<HW, C, KS>;
  constexpr int PAD = S::PAD, HP = S::HP, NPIX = S::NPIX, NHALO = S::NHALO, NSL = S::NSL, NE = S::NE, NT = S::NT, HGRP = S::HGRP, SLABB = S::SLABB;
  constexpr int NW = DUAL ? 2 : 1;
  constexpr int NI = NW * NE / kImgWaves;                // list items of a wave, all of ONE window (NE % NI == 0)
  static_assert(NE % NI == 0, "a wave's items lie in one window");
  constexpr int A_BYTES = NW * 64 * 64;                  // one entry of the weight storage: (hi | lo) x 64 rows x 64 bytes
  extern __shared__ __attribute__((aligned(16))) int8_t lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  int8_t* const tile = lds;
  int* const prm = reinterpret_cast<int*>(lds + S::PRM_OFF);

  // block -> (image group, m-tile); the m-tile is the fast index: with the blocks dealt round-robin over the eight XCDs the blocks of
  // one XCD share their weight tiles (one L2 fetches 1 / 8 of the row's weights when the row has a multiple of eight m-tiles)
  const int bid = blockIdx.x;
  const int grp = bid / a.n_mtiles, mt = bid - grp * a.n_mtiles;
  const int img0 = grp * kImgG;
  const int n_img = (a.B - img0) < kImgG ? (a.B - img0) : kImgG;
  const int n_px = n_img * NPIX;

  // ---- prologue: header rows and the padded input maps by LDS-DMA ----
  {
    const int8_t* h = reinterpret_cast<const int8_t*>(a.hdr) + (size_t)mt * a.hdr_bytes + lane * 16;
    for (int i = wave; i * 1024 < a.hdr_used; i += kImgWaves)
      lds_dma16(h + i * 1024, reinterpret_cast<int8_t*>(prm) + i * 1024);
    // what this lane fetches of a 16-pixel group of the swizzled tile: lds_tile.h.  Positions of the border, of an image the batch
    // does not have and of the group's padding take the stored zero.
    const int chunk = dma_lane_chunk(lane);
    for (int gi = wave; gi < HGRP * NSL; gi += kImgWaves) {
      const int s = gi / HGRP, g = gi - s * HGRP;
      const int hh = g * 16 + dma_lane_row(lane);
      const int hi = hh / NHALO, hq = hh - hi * NHALO;
      const int hr = hq / HP, hc = hq - hr * HP;
      const int row = hr - PAD, col = hc - PAD;
      const bool ok = hi < n_img && (unsigned)row < (unsigned)HW && (unsigned)col < (unsigned)HW;
      const int8_t* src = ok ? a.x + ((size_t)(img0 + hi) * NPIX + row * HW + col) * C + s * 64 + chunk * 16
                             : a.zero + s * 64 + chunk * 16;
      lds_dma16(src, tile + s * SLABB + g * 1024);
    }
  }
  // per-lane B addresses: pixel p = (image, r, c) -> position h0 + dh * HP + dw of the padded maps for tap (dh, dw), byte address
  // swz_off(h, half); the second K half is the same address ^ 32 (lds_tile.h)
  int h0[NT];
#pragma unroll
  for (int j = 0; j < NT; j++) {
    int p = j * 32 + (lane & 31);
    if (p >= n_px) p = 0;                                // lanes beyond the block's pixels compute on pixel 0 and are never stored
    const int pi = p / NPIX, q = p - pi * NPIX;
    const int r = q / HW;
    h0[j] = pi * NHALO + r * HP + (q - r * HW);
  }

  // this wave's part of the (window, tap, slab) list: items v0 .. v0 + NI - 1 = entries e0 .. of window win
  const int v0 = wave * NI;
  const int win = v0 / NE, e0 = v0 - win * NE;
  struct Afr { i32x4 k[2][2]; };                         // [row tile][K half] of one window of one weight tile
  const int8_t* const wbase = a.w + ((size_t)mt * NE + e0) * A_BYTES + win * (64 * 64) + (lane & 31) * 64 + half * 16;
  auto load_a = [&](Afr& f, int i) __attribute__((always_inline)) {
    const int8_t* p = wbase + (size_t)i * A_BYTES;
#pragma unroll
    for (int rt = 0; rt < 2; rt++) {
      f.k[rt][0] = *reinterpret_cast<const i32x4*>(p + rt * 2048);
      f.k[rt][1] = *reinterpret_cast<const i32x4*>(p + rt * 2048 + 32);
    }
  };
  Afr f0, f1, f2;                                        // weight fragments: two steps ahead of the MFMAs
  load_a(f0, 0);
  if (NI > 1) load_a(f1, 1);

  i32x16 acc[2][NT];
#pragma unroll
  for (int rt = 0; rt < 2; rt++)
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[rt][j][r] = 0;

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // header rows + input maps complete in every wave
  asm volatile("" ::: "memory");

  // ---- K loop: item i = entry e0 + i = (tap, slab) ----
  auto step = [&](auto i_c) __attribute__((always_inline)) {
    constexpr int i = decltype(i_c)::value;
    Afr& cur = i % 3 == 0 ? f0 : i % 3 == 1 ? f1 : f2;
    Afr& nxt = (i + 2) % 3 == 0 ? f0 : (i + 2) % 3 == 1 ? f1 : f2;
    if (i + 2 < NI) load_a(nxt, i + 2);
    const int e = e0 + i;                                // wave-uniform
    const int t = e / NSL, s = e - t * NSL;
    const int th = t / KS, toff = th * HP + (t - th * KS);
    const int8_t* B = tile + s * SLABB;
    int ba[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) {
      const int hh = h0[j] + toff;
      ba[j] = swz_off(hh, half);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      i32x4 bf[NT];
#pragma unroll
      for (int j = 0; j < NT; j++) bf[j] = *reinterpret_cast<const i32x4*>(B + (ba[j] ^ (ks << 5)));
#pragma unroll
      for (int j = 0; j < NT; j++) {
        acc[0][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.k[0][ks], bf[j], acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.k[1][ks], bf[j], acc[1][j], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                   // steps stay in order: the unrolled loop must not pile up loads
  };
  static_for<0, NI>(step);

  // ---- combining the eight partial tiles through LDS, over the input tile's space ----
  // slot s (32 KiB) holds a partial tile in the accumulators' own lane layout: 16-byte group q of tile (rt, j) at
  // ((rt * NT + j) * 4 + q) * 1024 + lane * 16 -- every access is 64 lanes x 16 contiguous bytes
  auto part = [&](int slot, int rt, int j, int q) __attribute__((always_inline)) {
    return reinterpret_cast<i32x4*>(lds + slot * S::PART_BYTES + ((rt * NT + j) * 4 + q) * 1024 + lane * 16);
  };
  auto store_acc = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
      for (int j = 0; j < NT; j++)
#pragma unroll
        for (int q = 0; q < 4; q++)
          *part(slot, rt, j, q) = i32x4{acc[rt][j][4 * q], acc[rt][j][4 * q + 1], acc[rt][j][4 * q + 2], acc[rt][j][4 * q + 3]};
  };
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // every wave has read its last B fragment: the input tile's space is free
  asm volatile("" ::: "memory");
  if (wave >= 4) store_acc(wave - 4);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (wave < 4) {
    // two-window rows: this wave holds a part of the HIGH window, its partner the same part of the low one: (hi << dshift[1][row]) + lo
    // (weight_pack.cpp: high window first; accumulator register G * 4 + r of row tile rt = row rt * 32 + 4 * half + 8 * G + r)
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        i32x4 d = {0, 0, 0, 0};
        if (DUAL) d = *reinterpret_cast<const i32x4*>(prm + (kPrmWordsPerRow + 1) * 64 + rt * 32 + 4 * half + 8 * q);
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const i32x4 o = *part(wave, rt, j, q);
#pragma unroll
          for (int r = 0; r < 4; r++)
            acc[rt][j][4 * q + r] = (int)(((unsigned)acc[rt][j][4 * q + r] << (d[r] & 31)) + (unsigned)o[r]);
        }
      }
    store_acc(wave);                                     // (slot `wave` is read by this wave alone: no barrier between its reads and these writes)
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // ---- every wave finishes one 32 x 32 tile: row tile wave / 4, column tile wave % 4 ----
  const int rt = wave >> 2, ct = wave & 3;
  if (ct * 32 >= n_px) return;                           // (the one-image block of an odd batch: two column tiles hold no pixel)
  int a16[16];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    i32x4 sum = *part(0, rt, ct, q);
#pragma unroll
    for (int sl = 1; sl < 4; sl++) {
      const i32x4 o = *part(sl, rt, ct, q);
#pragma unroll
      for (int r = 0; r < 4; r++) sum[r] = (int)((unsigned)sum[r] + (unsigned)o[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) a16[4 * q + r] = sum[r];
  }
  const int lo_bound = a.relu ? 0 : -128;
  const i32x4 nores = {0, 0, 0, 0};
  const i32x4 out = a.fast == 1 ? requant_tile16<false, 0, true>(a16, prm, 64, rt * 32 + 4 * half, lo_bound, -128, nores, a.dbl != 0)
                                : requant_tile16<false, 0, false>(a16, prm, 64, rt * 32 + 4 * half, lo_bound, -128, nores, a.dbl != 0, a.fast == 2);
  const int p = ct * 32 + (lane & 31);
  const int ch = mt * 64 + rt * 32 + 16 * half;           // this lane's 16 output channels
  if (p < n_px && ch + 16 <= a.y_nvalid)
    *reinterpret_cast<i32x4*>(a.y + ((size_t)img0 * NPIX + p) * a.y_cp + a.y_off + ch) = out;
}

// the instantiated shapes: map side, input channels (= bytes per input pixel), filter size
bool conv_img_shape_ok(int HW, int C, int k) { return HW == 7 && C == 512 && k == 3; }

size_t conv_img_lds_bytes(int HW, int C, int k, size_t hdr_used) {
  if (!conv_img_shape_ok(HW, C, k)) return 0;
  return (size_t)ImgShape<7, 512, 3>::PRM_OFF + hdr_used;
}

long conv_img_blocks(int batch, int n_mtiles) { return (long)((batch + kImgG - 1) / kImgG) * n_mtiles; }

// 1: shape not instantiated / does not fit
int launch_conv_img(const ImgArgs& a, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!conv_img_shape_ok(a.HW, a.C, a.k) || a.hdr_used > a.hdr_bytes) return 1;
  const size_t lds = conv_img_lds_bytes(a.HW, a.C, a.k, (size_t)a.hdr_used);
  if (lds > 160 * 1024) return 1;
  const long grid = conv_img_blocks(a.B, a.n_mtiles);
#define TF2_IMG(D) do { auto fn = conv_img_kernel<7, 512, 3, D>; if (!lds_attr_once(reinterpret_cast<const void*>(fn))) return -1; \
                        TF2_LAUNCH_NAME("conv_img_kernel<%dx%d,C%d,k%d,%s,%d images>", a.HW, a.HW, a.C, a.k, D ? "two-window" : "one-window", kImgG); \
                        TF2_LAUNCH(fn, dim3((unsigned)grid), dim3(512), lds, s, a); } while (0)
  if (a.dual) TF2_IMG(true); else TF2_IMG(false);
#undef TF2_IMG
  return launch_ok() ? 0 : -1;
}

}  // namespace tf2
