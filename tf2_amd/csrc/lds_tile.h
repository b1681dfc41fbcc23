// lds_tile.h -- what every conv kernel shares on the device side, stated once (gfx950): the vector types and address-space casts, the
// compile-time loop, the XCD block remap, the block stamp, the plain LDS-DMA -- and the LAYOUT of the swizzled [pixel][64] LDS tile
// together with the lane mapping of the DMA that fills it, with the contract between the two checked by the compiler.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "vm_track.h"

namespace tf2 {

using i32x4 = int __attribute__((ext_vector_type(4)));
using i32x16 = int __attribute__((ext_vector_type(16)));

#define TF2_GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define TF2_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// fn(std::integral_constant<int, T>{}) for T, T + 1, .. N - 1: a loop whose index is a constant expression inside the body
template <int T, int N, class F>
__device__ __forceinline__ void static_for(F& fn) {
  if constexpr (T < N) { fn(std::integral_constant<int, T>{}); static_for<T + 1, N>(fn); }
}

// XCD-aware block remap.  The hardware deals consecutive block ids round-robin to the chip's 8 XCDs (id & 7), each with an L2 of its
// own; the remap hands every XCD one CONTIGUOUS range of the nblk logical tiles instead (the first nblk & 7 XCDs one tile more), so
// that neighbouring tiles -- the channel tiles of one pixel tile, the row bands of one image -- share what they read in one L2.
// A bijection on [0, nblk) for every nblk.
__host__ __device__ constexpr int xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, within = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
}

// thread 0 of the block writes the chip-wide 100 MHz wall clock into slot i of the block's stamp row (tools/*_timeline.py); dbg is
// null in production.  Reads the kernel's `tid`.
#define TF2_BLOCK_STAMP(dbg, i) do { if ((dbg) && tid == 0) (dbg)[i] = (long long)wall_clock64(); } while (0)

// one LDS-DMA wave instruction (global_load_lds_dwordx4): lane l's 16 bytes at src (a per-lane address) land at dst + 16 * l (dst
// wave-uniform) -- 1 KiB, no VGPR staging.  The compiler knows this load and drains the queue in front of the next LDS read; the
// form it does not see is dma16_hidden (vm_track.h).  lds_dma16_aux: with the instruction's cache-policy bits (1 = sc0, 16 = sc1;
// conv_bgroup.hip).  (Macros: the casts stay where the operands are computed, which is the order the scheduler was tuned with.)
#define lds_dma16_aux(src, lds_dst, aux) __builtin_amdgcn_global_load_lds(TF2_GLOBAL_PTR(src), TF2_LDS_PTR(lds_dst), 16, 0, aux)
#define lds_dma16(src, lds_dst) lds_dma16_aux(src, lds_dst, 0)

// ---- the swizzled [row][64] tile ---------------------------------------------------------------------------------------------------
// Operand tiles sit in LDS as 64-byte rows (a row = one pixel of a B tile / one output channel of an A tile, 64 K bytes) of four
// 16-byte chunks; chunk c of row r is kept in slot c ^ ((r >> 2) & 3).  A lane's MFMA fragment is one chunk of its row, read with
// ds_read_b128, and with the XOR any 16 consecutive rows of one chunk hit 16 distinct 16-byte bank groups -- whatever row the run
// starts at, so a 3x3 tap (the same tile at a shifted row) reads without bank conflict too.  The second K half of a fragment
// (chunk c ^ 2, i.e. chunk 2 + half for half = lane >> 5) is the same address ^ 32.
//
// Such a tile is filled 16 rows (1 KiB) at a time by one LDS-DMA wave instruction, whose LDS destination is lane-linear: lane l
// writes bytes 16 l .. 16 l + 15, which is slot l & 3 of row l >> 2.  The swizzle therefore goes on the per-lane SOURCE address:
// lane l fetches the chunk that belongs into its slot, (l & 3) ^ ((row >> 2) & 3) -- and row >> 2 == l >> 4 inside a group that
// starts at a multiple of 16 rows, so a lane fetches the same chunk index for every group.  swz_off and dma_lane_* must agree; the
// static assertions below are that contract.
// byte offset of chunk `chunk` of row `row` inside a [row][64] tile
__host__ __device__ constexpr int swz_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }
// ... added to a base (a pointer, or a byte offset) in the order base + row * 64 + slot, the sum the kernels were tuned with: the
// compiler folds a constant part of the row into the instruction's offset field only from this association
template <class B, class R>
__host__ __device__ constexpr B swz_at(B base, R row, int chunk) { return base + row * 64 + ((chunk ^ (((int)row >> 2) & 3)) << 4); }
// what lane `lane` of one 1 KiB DMA instruction fetches: chunk dma_lane_chunk of row dma_lane_row of the 16-row group
// (dma_lane_chunk reads bits 0-1 and 4-5 of its argument only: the thread id of a block of whole waves gives the same value)
__host__ __device__ constexpr int dma_lane_chunk(int lane) { return (lane & 3) ^ ((lane >> 4) & 3); }
__host__ __device__ constexpr int dma_lane_row(int lane) { return lane >> 2; }
// ... and where that chunk sits in a PLAIN [row][64] group (a weight tile in memory): row * 64 + chunk * 16, i.e. the lane's own
// 16-byte position with its slot replaced by the chunk the slot holds
__host__ __device__ constexpr int dma_lane_src_off(int lane) { return ((lane & ~3) | dma_lane_chunk(lane)) << 4; }

// The same four as macros, for conv_bgroup.hip (and one line of conv_bband.hip): hipcc folds a written-out expression together with its surroundings one pass before
// it inlines a call, and the group kernels' schedule (and one batch at a time, 1 % of the step) depends on which it sees.  Asserted equal below.
#define TF2_SWZ_OFF(row, chunk) ((row) * 64 + (((chunk) ^ (((row) >> 2) & 3)) << 4))
#define TF2_SWZ_AT(base, row, chunk) ((base) + (row) * 64 + (((chunk) ^ (((row) >> 2) & 3)) << 4))
#define TF2_DMA_LANE_CHUNK(lane) (((lane) & 3) ^ (((lane) >> 4) & 3))
#define TF2_DMA_LANE_ROW(lane) ((lane) >> 2)

namespace lds_tile_contract {
// a lane-linear DMA of a 16-row group produces exactly the layout the fragment reads assume
constexpr bool dma_fills_layout() {
  for (int l = 0; l < 64; l++)
    if (swz_off(dma_lane_row(l), dma_lane_chunk(l)) != 16 * l || dma_lane_src_off(l) != dma_lane_row(l) * 64 + dma_lane_chunk(l) * 16) return false;
  for (int tid = 0; tid < 1024; tid++)
    if (dma_lane_chunk(tid) != dma_lane_chunk(tid & 63)) return false;
  for (int l = 0; l < 64; l++)
    if (TF2_DMA_LANE_CHUNK(l) != dma_lane_chunk(l) || TF2_DMA_LANE_ROW(l) != dma_lane_row(l)) return false;
  for (int row = 0; row < 64; row++)
    for (int c = 0; c < 4; c++)
      if (TF2_SWZ_OFF(row, c) != swz_off(row, c) || TF2_SWZ_AT(128, row, c) != swz_at(128, row, c)) return false;
  return true;
}
// the second K half is the same address ^ 32
constexpr bool k_half_is_xor32() {
  for (int row = 0; row < 64; row++)
    for (int c = 0; c < 4; c++)
      if (swz_off(row, c ^ 2) != (swz_off(row, c) ^ 32) || swz_at(0, row, c) != swz_off(row, c)) return false;
  return true;
}
// sixteen consecutive rows of one chunk, from any start row, hit sixteen distinct 16-byte bank groups
constexpr bool rows_spread_over_banks() {
  for (int c = 0; c < 4; c++)
    for (int r0 = 0; r0 < 16; r0++) {
      unsigned seen = 0;
      for (int r = r0; r < r0 + 16; r++) seen |= 1u << ((swz_off(r, c) >> 4) & 15);
      if (seen != 0xffffu) return false;
    }
  return true;
}
static_assert(dma_fills_layout(), "swz_off(dma_lane_row(l), dma_lane_chunk(l)) == 16 * l for every lane");
static_assert(k_half_is_xor32(), "swz_off(row, c ^ 2) == swz_off(row, c) ^ 32");
static_assert(rows_spread_over_banks(), "16 consecutive rows of a chunk in 16 distinct bank groups");
}  // namespace lds_tile_contract

}  // namespace tf2
