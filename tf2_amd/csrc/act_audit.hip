// act_audit.hip -- the activation audit (tf2_audit_*, include/tf2_amd.h): every kept map of a keep_all step reduced to exact per-channel
// integer statistics in a caller-owned device store, with no host copy and no synchronisation.  tf2_amd/audit.py states the record
// (reference_audit); the store equals it as integers, whatever the grid and the order of the blocks: every counter is an integer added
// (or minimised / maximised) with a 64-bit atomic.  act_rows.h holds what this file shares with act_fidelity and act_caq: the rows of
// a net (ActRows), the refusals and kept maps in front of Auditor::run (KeptMaps), the rows dealt to launches (LaunchBatch), the
// block-to-row search, add64 and the wave reductions.
//
// The arithmetic is on four values of ONE channel packed in a dword (acc_dword): sum and sum of squares are one sdot4 each, the counts
// are byte-parallel bit tricks closed by a population count -- negative = the sign bits; |v| per byte is (v ^ s) + sign with s = 0xff on
// negative bytes (no carry leaves a byte); |v| = 128 is bit 7 of that, v = 127 is |v| + 1 reaching bit 7 on a non-negative byte; the
// top bit of |v| & 0x7f smeared downwards makes bit k of a byte say "bit length > k", which gives the histogram as differences of
// seven counts.  No floating point but quant_input's on float images, no division in a loop, no scratch.
//
// audit_rows_kernel   NHWC tensors with pitch: up to kAuditRowsPerLaunch table rows a launch, their descriptions in the kernel arguments
//                     (no device table to keep alive or to miss in a graph replay).  A block owns kAuditSlab pixels x kAuditChans
//                     channels of one row.  Lanes run along channels with dword loads, four channels a lane; where a row has fewer than
//                     256 channels the other lanes of the wave run along pixels.  A lane loads its four channels of four consecutive
//                     pixels, transposes the 4 x 4 bytes and feeds four one-channel dwords to acc_dword; pixels past the slab's end
//                     repeat the group's last real pixel for min / max and are zero for everything else.  "Doubled" channels
//                     (PackLayer::off_dbl: 2y - 128) are undone on the packed dword, ((t ^ 0x80808080) >> 1) & 0x7f7f7f7f.  Waves and
//                     pixel lanes combine through LDS atomics (14 x 256 words), then one thread a channel issues the 64-bit atomics
//                     for the non-zero counters.
// audit_image_kernel  the input record from the caller's dense NCHW images: a block owns kAuditImgSlab values of one plane, a lane four
//                     consecutive ones (float: through quant_input with trans = 2^Q0); lanes reduce with shuffles, waves through LDS,
//                     one thread a block issues the atomics (all blocks of a channel meet on the same words of the store).
// audit_init_kernel   the empty store: zeros, min = 127, max = -128.
//
//   kernel              VGPRs  scratch  static LDS
//   audit_rows_kernel   86     0        14 336
//   audit_image_kernel  51     0        256
//   audit_init_kernel   6      0        0
// Measured on an MI355X, ResNet-50 at batch 32 (tools/act_audit_time.py, profiles/act_audit_time_b32.json): the audit alone 0.297 ms for
// 0.353 GB behind a keep_all step of 0.707 ms; rows kernel 261 us, input kernel 32 us in a kernel trace.  Two pixel groups an
// iteration (eight loads in flight) cost 125 VGPRs and were slower; the loop keeps one.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "input_quant.h"
#include "act_audit.h"

namespace tf2 {

namespace {

constexpr int kThreads = 256;
constexpr int kRedSlots = 14;          // neg, lo, hi, min, max, sum, sumsq, ge[7]
static_assert(kAuditChans == kThreads && kAuditChans == 4 * 64, "a wave's dword loads span the block's channels; one flushing thread a channel");
static_assert((long long)kAuditSlab * 16384 < (1ll << 31) && (long long)kAuditImgSlab * 16384 < (1ll << 31), "a block's sumsq fits 32 bits");

struct Acc {                           // one channel
  uint32_t neg, lo, hi, ge[7];         // ge[k]: values with |v| & 0x7f >= 2^k
  int32_t mn, mx, sum, sq;
};

__device__ __forceinline__ void acc_init(Acc& a) {
  a.neg = a.lo = a.hi = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) a.ge[k] = 0;
  a.mn = 127; a.mx = -128; a.sum = 0; a.sq = 0;
}

// t: four values of one channel, every byte a real value (min / max); m: the same with the bytes that do not count set to zero
__device__ __forceinline__ void acc_dword(Acc& a, uint32_t t, uint32_t m) {
  const int b0 = (int)(t << 24) >> 24, b1 = (int)(t << 16) >> 24, b2 = (int)(t << 8) >> 24, b3 = (int)t >> 24;
  a.mn = min(a.mn, min(min(b0, b1), min(b2, b3)));
  a.mx = max(a.mx, max(max(b0, b1), max(b2, b3)));
  a.sum = __builtin_amdgcn_sdot4((int)m, 0x01010101, a.sum, false);
  a.sq = __builtin_amdgcn_sdot4((int)m, (int)m, a.sq, false);
  const uint32_t sgn = m & 0x80808080u;
  a.neg += __popc(sgn);
  const uint32_t s = (sgn << 1) - (sgn >> 7);                       // 0xff on the negative bytes
  const uint32_t ab = (m ^ s) + (sgn >> 7);                         // |v| per byte, 0 .. 128
  a.lo += __popc(ab & 0x80808080u);
  const uint32_t a7 = ab & 0x7f7f7f7fu;                             // (the low rail's byte is 0 from here on: it is in no hist bin)
  a.hi += __popc((a7 + 0x01010101u) & ~sgn & 0x80808080u);
  uint32_t sm = a7 | ((a7 >> 1) & 0x7f7f7f7fu);
  sm |= (sm >> 2) & 0x3f3f3f3fu;
  sm |= (sm >> 4) & 0x0f0f0f0fu;
#pragma unroll
  for (int k = 0; k < 7; k++) a.ge[k] += __popc(sm & (0x01010101u << k));
}

// a channel's record from a block's (or a wave's) counters over n values
__device__ __forceinline__ void flush_record(long long* rec, int n, int neg, int lo, int hi, int mn, int mx, int sum, int sq, const int (&ge)[7]) {
  unsigned long long* const u = reinterpret_cast<unsigned long long*>(rec);
  add64(u + 0, n); add64(u + 1, neg); add64(u + 2, lo); add64(u + 3, hi);
  if (mn < 127) atomicMin(rec + 4, (long long)mn);
  if (mx > -128) atomicMax(rec + 5, (long long)mx);
  add64(u + 6, sum); add64(u + 7, sq);
  add64(u + 8, n - lo - ge[0]);
#pragma unroll
  for (int b = 1; b < 7; b++) add64(u + 8 + b, ge[b - 1] - ge[b]);
  add64(u + 15, ge[6]);
}

// A lane's four channels (from `col`) of pixel group g of a slab: four pixels, one past the slab's end repeats the last real one.
template <bool VEC>
__device__ __forceinline__ void load_group(uint32_t (&d)[4], const int8_t* col, int pix0, int g, int nv, int cp, int nch) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const long long pj = pix0 + 4 * g + min(j, nv - 1);
    const int8_t* const q = col + pj * cp;
    if (VEC) {
      d[j] = *reinterpret_cast<const uint32_t*>(q);
    } else {
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (k < nch) v |= (uint32_t)(uint8_t)q[k] << (8 * k);
      d[j] = v;
    }
  }
}

// the group's 4 x 4 bytes transposed to one dword a channel, doubled channels undone, counted; vm: the bytes of the real pixels
__device__ __forceinline__ void count_group(Acc (&a)[4], const uint32_t (&d)[4], const bool (&dbl)[4], uint32_t vm) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint32_t t = ((d[0] >> (8 * k)) & 0xffu) | (((d[1] >> (8 * k)) & 0xffu) << 8) | (((d[2] >> (8 * k)) & 0xffu) << 16) |
                 (((d[3] >> (8 * k)) & 0xffu) << 24);
    if (dbl[k]) t = ((t ^ 0x80808080u) >> 1) & 0x7f7f7f7fu;         // 2y - 128 -> y = (v + 128) >> 1
    acc_dword(a[k], t, t & vm);
  }
}

__device__ __forceinline__ uint32_t real_bytes(int nv) { return nv == 4 ? 0xffffffffu : (1u << (8 * nv)) - 1u; }

// the lane's groups first, first + stride, ... of the slab
template <bool VEC>
__device__ __forceinline__ void walk_slab(Acc (&a)[4], const bool (&dbl)[4], const int8_t* col, int pix0, int spix, int cp, int nch, int first,
                                          int stride, int ng) {
  for (int g = first; g < ng; g += stride) {
    const int nv = min(4, spix - 4 * g);                            // >= 1
    uint32_t d[4];
    load_group<VEC>(d, col, pix0, g, nv, cp, nch);
    count_group(a, d, dbl, real_bytes(nv));
  }
}

__global__ __launch_bounds__(kThreads) void audit_rows_kernel(AuditRowsArgs p) {
  __shared__ int red[kRedSlots][kAuditChans];
  int r;
  TF2_ROW_OF_BLOCK(r, p);
  const AuditRow& R = p.rows[r];
  const int local = (int)blockIdx.x - R.block0;
  const int slab = local / R.n_cpass, cpass = local - slab * R.n_cpass;
  const int pix0 = slab * kAuditSlab;
  const int spix = min(kAuditSlab, R.npix - pix0);
  const int C = R.c, cp = R.cp;

  for (int i = threadIdx.x; i < kRedSlots * kAuditChans; i += kThreads) {
    const int slot = i / kAuditChans;
    (&red[0][0])[i] = slot == 3 ? 127 : slot == 4 ? -128 : 0;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cg = lane & ((1 << R.lp_shift) - 1), pl = lane >> R.lp_shift, npl = 64 >> R.lp_shift;
  const int c0 = cpass * kAuditChans + 4 * cg;
  if (c0 < C) {
    Acc a[4];
    bool dbl[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      acc_init(a[k]);
      dbl[k] = R.dbl != nullptr && c0 + k < C && R.dbl[c0 + k] != 0;
    }
    const int ng = (spix + 3) >> 2;
    if (R.vec) walk_slab<true>(a, dbl, R.base + c0, pix0, spix, cp, min(4, C - c0), wave * npl + pl, 4 * npl, ng);
    else walk_slab<false>(a, dbl, R.base + c0, pix0, spix, cp, min(4, C - c0), wave * npl + pl, 4 * npl, ng);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int ch = 4 * cg + k;
      if (c0 + k < C) {
        if (a[k].neg) atomicAdd(&red[0][ch], (int)a[k].neg);
        if (a[k].lo) atomicAdd(&red[1][ch], (int)a[k].lo);
        if (a[k].hi) atomicAdd(&red[2][ch], (int)a[k].hi);
        atomicMin(&red[3][ch], a[k].mn);
        atomicMax(&red[4][ch], a[k].mx);
        if (a[k].sum) atomicAdd(&red[5][ch], a[k].sum);
        if (a[k].sq) atomicAdd(&red[6][ch], a[k].sq);
#pragma unroll
        for (int b = 0; b < 7; b++)
          if (a[k].ge[b]) atomicAdd(&red[7 + b][ch], (int)a[k].ge[b]);
      }
    }
  }
  __syncthreads();

  const int t = threadIdx.x, c = cpass * kAuditChans + t;
  if (c < C) {
    int ge[7];
#pragma unroll
    for (int b = 0; b < 7; b++) ge[b] = red[7 + b][t];
    flush_record(R.store + (long long)c * kAuditSlots, spix, red[0][t], red[1][t], red[2][t], red[3][t], red[4][t], red[5][t], red[6][t], ge);
  }
}

__global__ __launch_bounds__(kThreads) void audit_image_kernel(AuditImgArgs p) {
  const int plane = (int)blockIdx.x / p.slabs, slab = (int)blockIdx.x - plane * p.slabs;
  const int ch = plane % p.c;
  const int v0 = slab * kAuditImgSlab;
  const int sv = min(kAuditImgSlab, p.hw - v0);
  const long long at0 = (long long)plane * p.hw + v0;
  const int8_t* const q8 = static_cast<const int8_t*>(p.images);
  const float* const f32 = static_cast<const float*>(p.images);
  Acc a;
  acc_init(a);
  int n = 0;
  for (int i = 4 * (int)threadIdx.x; i < sv; i += 4 * kThreads) {
    const int nv = min(4, sv - i);
    uint32_t t = 0;
    if (p.is_q) {
      if (p.vec && nv == 4) {
        t = *reinterpret_cast<const uint32_t*>(q8 + at0 + i);
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) t |= (uint32_t)(uint8_t)q8[at0 + i + min(k, nv - 1)] << (8 * k);
      }
    } else {
      float f[4];
      if (p.vec && nv == 4) {
        const float4 x = *reinterpret_cast<const float4*>(f32 + at0 + i);
        f[0] = x.x; f[1] = x.y; f[2] = x.z; f[3] = x.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) f[k] = f32[at0 + i + min(k, nv - 1)];
      }
#pragma unroll
      for (int k = 0; k < 4; k++) t |= ((uint32_t)quant_input(f[k], p.trans) & 0xffu) << (8 * k);
    }
    const uint32_t vm = nv == 4 ? 0xffffffffu : (1u << (8 * nv)) - 1u;
    acc_dword(a, t, t & vm);
    n += nv;
  }
  n = wave_sum(n);
  const int neg = wave_sum((int)a.neg), lo = wave_sum((int)a.lo), hi = wave_sum((int)a.hi), sum = wave_sum(a.sum), sq = wave_sum(a.sq);
  int ge[7];
#pragma unroll
  for (int b = 0; b < 7; b++) ge[b] = wave_sum((int)a.ge[b]);
  const int mn = wave_min(a.mn), mx = wave_max(a.mx);
  // the block's waves meet in LDS: every block of a channel adds to the same few words of the store, so one thread a block does
  __shared__ int part[kThreads / 64][16];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    int* const w = part[wave];
    w[0] = n; w[1] = neg; w[2] = lo; w[3] = hi; w[4] = mn; w[5] = mx; w[6] = sum; w[7] = sq;
#pragma unroll
    for (int b = 0; b < 7; b++) w[8 + b] = ge[b];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t[15];
#pragma unroll
    for (int i = 0; i < 15; i++) {
      t[i] = part[0][i];
#pragma unroll
      for (int v = 1; v < kThreads / 64; v++) t[i] = i == 4 ? min(t[i], part[v][i]) : i == 5 ? max(t[i], part[v][i]) : t[i] + part[v][i];
    }
    const int g7[7] = {t[8], t[9], t[10], t[11], t[12], t[13], t[14]};
    if (t[0] > 0) flush_record(p.store + (long long)ch * kAuditSlots, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], g7);
  }
}

__global__ __launch_bounds__(kThreads) void audit_init_kernel(long long* store, long long words) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < words) {
    const int slot = (int)(i & (kAuditSlots - 1));
    store[i] = slot == 4 ? 127 : slot == 5 ? -128 : 0;
  }
}

}  // namespace

// ---- the handle --------------------------------------------------------------------------------------------------------
tf2_status Auditor::store_init(void* store, size_t store_bytes, void* stream) const {
  if (!store) return arg_refusal("tf2_audit_store_init", "null store_dev");
  if (store_bytes < store_size()) { set_error("tf2_audit_store_init: store too small (tf2_audit_store_size: " + std::to_string(store_size()) + ")"); return TF2_ERR_SIZE; }
  const long long words = g.n_records * kAuditSlots;
  hipLaunchKernelGGL(audit_init_kernel, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (long long*)store, words);
  return launch_result("tf2_audit_store_init");
}

// with_step: the keep_all step first (tf2_audit_run); without, the audit alone of a workspace that holds one (tf2_audit_kept)
tf2_status Auditor::run(const void* images, bool images_are_q, int batch, void* ws, size_t ws_bytes, int8_t* logits, void* store,
                        size_t store_bytes, void* stream, bool with_step) {
  Net* const net = g.net;
  KeptMaps kept;
  if (tf2_status st = kept.open(g, "tf2_audit", !images || !ws || (with_step && !logits) || !store, "null device pointer", batch, ws, ws_bytes,
                                store_bytes, store_size(), 0))
    return st;
  // every row and the grids, before anything is enqueued
  LaunchBatch<AuditRowsArgs, AuditRow, kAuditRowsPerLaunch> rows("tf2_audit_run", AuditRowsArgs{});
  for (int l = 0; l < net->nd.n_layers; l++) {
    KeptMap m;
    if (tf2_status st = kept.map(l, m)) return st;
    const int n_cpass = (m.C + kAuditChans - 1) / kAuditChans;
    AuditRow* const R = rows.add((m.npix + kAuditSlab - 1) / kAuditSlab * n_cpass);
    if (!R) return TF2_ERR_UNSUPPORTED;
    R->base = m.base; R->dbl = m.dbl;
    R->store = (long long*)store + m.rec0 * kAuditSlots;
    R->npix = (int32_t)m.npix; R->c = m.C; R->cp = m.Cp;
    R->n_cpass = n_cpass;
    const int groups = (std::min(m.C, kAuditChans) + 3) / 4;
    R->lp_shift = 0;
    while ((1 << R->lp_shift) < groups) R->lp_shift++;
    R->vec = (((uintptr_t)m.base & 3) == 0 && m.Cp % 4 == 0 && m.off + round_up(m.C, 4) <= m.Cp) ? 1 : 0;
    R->pad = 0;
  }
  AuditImgArgs I{};
  I.images = images; I.store = (long long*)store; I.trans = std::ldexp(1.0f, -(int)net->q[0]); I.is_q = images_are_q ? 1 : 0;
  I.c = net->nd.image_c; I.hw = net->nd.image_h * net->nd.image_w; I.planes = batch * I.c;
  I.slabs = (I.hw + kAuditImgSlab - 1) / kAuditImgSlab;
  I.vec = (I.hw % 4 == 0 && ((uintptr_t)images & (images_are_q ? 3 : 15)) == 0) ? 1 : 0;

  if (with_step)
    if (tf2_status st = net->run(images, images_are_q, batch, ws, ws_bytes, logits, stream)) return st;
  hipLaunchKernelGGL(audit_image_kernel, dim3((unsigned)((long long)I.planes * I.slabs)), dim3(kThreads), 0, (hipStream_t)stream, I);
  if (tf2_status st = launch_result("tf2_audit_run", "image audit launch failed")) return st;
  for (size_t i = 0; i < rows.launches.size(); i++) {
    hipLaunchKernelGGL(audit_rows_kernel, dim3((unsigned)rows.blocks[i]), dim3(kThreads), 0, (hipStream_t)stream, rows.launches[i]);
    if (tf2_status st = launch_result("tf2_audit_run", "audit launch failed")) return st;
  }
  return TF2_OK;
}

}  // namespace tf2
