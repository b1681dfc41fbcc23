// act_fidelity.hip -- layer fidelity (tf2_fid_*, include/tf2_amd.h): every kept int8 map of a keep_all step set against the float32 map of
// a float forward, per channel, in a caller-owned device store, with no host copy and no synchronisation.  tf2_amd/fidelity.py states
// the record (reference_compare); the store equals it as integers, whatever the grid and the order of the blocks: every counter is an
// integer added (or maximised) with a 64-bit atomic.  act_rows.h holds what this file shares with act_audit and act_caq: the rows of a
// net (ActRows), the refusals and kept maps in front of Comparator::run (KeptMaps), the rows dealt to launches (LaunchBatch), the
// block-to-row search, add64 and the wave reductions.
//
// Per value (fid_count): f not finite -> nonfinite, nothing else.  t = f * 2^(Q + 8), one float32 multiplication; |t| >= 65536 (an
// overflow to inf included) -> e = +-65536 and ref_clamped; else e = rint(t), half to even.  d = 256 v - e, |d| < 2^17;
// k = min(7, bit_length((|d| + 128) >> 8)).  A value that does not count is turned into v = 0, e = 0, which adds nothing anywhere:
// hist[0] is not counted but taken as n minus the other bins, so the loop has no branch.
//
// fid_rows_kernel    the meeting of the two layouts.  Up to kFidRowsPerLaunch table rows a launch, their descriptions in the kernel
//                    arguments (a row with a NULL reference is not in the table and costs no block).  A block owns kFidSlab pixels x
//                    kFidChans channels of one row and walks them in tiles of kFidTile pixels.  The float side is read with lanes
//                    along pixels -- a lane takes four consecutive pixels of one channel, one 16-byte load where they lie in one image
//                    and the address is aligned, else four loads with the address formed per pixel, ((b C + c) HW + i): a tile
//                    straddles images whenever HW is no multiple of four (49, 1) -- and written to an LDS tile [channel][pixel] of
//                    pitch 65 words.  The int8 side is read as it lies, lanes along channels (64 consecutive bytes a wave), and each
//                    lane counts ITS channel, taking the float from the LDS tile (pitch 65: the 32 lanes of a half-wave on 32 banks).
//                    The four waves split a tile's pixels.  The next tile's float and int8 loads are issued before the current tile
//                    is counted; two LDS tiles, one barrier a tile.  A lane keeps its channel's counters in registers over the whole
//                    slab (at most 256 values: 32-bit sums, nonfinite and ref_clamped as the halves of one word, n as the
//                    real values minus nonfinite, the histogram as seven 9-bit fields of one 64-bit word, sum_d2 and
//                    sum_e2 through 64-bit multiply-adds); the waves meet in LDS atomics, then one thread a channel issues the
//                    64-bit atomics for the non-zero counters.
// fid_image_kernel   row -1 from the caller's dense NCHW float images: v = quant_input(f, 2^Q0), e from the same f.  A block owns
//                    kFidImgSlab values of one plane; the same counters, reduced over the block's lanes, one thread issues the atomics.
//
//   kernel             VGPRs  scratch  static LDS
//   fid_rows_kernel    135    0        38 144
//   fid_image_kernel   51     0        4 864
// Measured on an MI355X, ResNet-50 at batch 32 (tools/fidelity_time.py, profiles/fidelity_time_b32.json): the comparison alone 0.649 ms
// for 1.686 GB (0.333 GB of int8 maps, 1.352 GB of float32) = 2.60 TB/s, beside 1.20 TB/s of tf2_audit_kept in the same job; rows kernel
// 590 us (5,368 blocks, one launch), input kernel 51 us in a kernel trace.  The loop is bound by instruction issue, so what shortened it
// were instructions: a first version that guarded every int8 load with its own branch (a lane past C, a pixel past the end) and kept
// n, nonfinite and ref_clamped as three counters took 0.790 ms (rows kernel 727 us); loads from clamped addresses without a branch, the
// two rare counts as the halves of one word and n derived from the number of real values gave the figures above.  A launch bound of
// four blocks a CU (128 VGPRs, the LDS's limit) spilled three registers to scratch and was not kept.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "input_quant.h"
#include "act_fidelity.h"

namespace tf2 {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPitch = kFidTile + 1;                     // words of a channel's line in the LDS tile
constexpr int kPixPerWave = kFidTile / kWaves;           // pixels of a tile one wave counts
constexpr int kRed32 = 15;                               // n, nonfinite, clamped, max, sum_d, sum_abs_d, sum_abs_e, sum_v2, hist[1..7]
static_assert(kFidChans == 64 && kFidTile == 64 && kFidTile * kFidChans == 16 * kThreads, "a lane a channel; four float4 a thread and tile");
static_assert(kFidSlab / kWaves < 512 && kFidImgSlab / kThreads < 512, "a thread's histogram fields are 9 bits wide");
static_assert((long long)kFidSlab << 17 < (1ll << 31) && (long long)kFidImgSlab * 98304 < (1ll << 31), "a block's sum_abs_d (|d| <= 2^15 + 2^16) fits 32 bits");

struct Acc {                                             // one channel, one thread
  uint32_t flags, maxd, sad, sae, sv2;                  // flags: nonfinite in the low half, ref_clamped in the high half (n = the real values - nonfinite)
  int32_t sd;
  unsigned long long d2, e2, hist;                       // hist: bins 1..7 in 9-bit fields
};

__device__ __forceinline__ void acc_init(Acc& a) {
  a.flags = a.maxd = a.sad = a.sae = a.sv2 = 0;
  a.sd = 0;
  a.d2 = a.e2 = a.hist = 0;
}

// ok: the value exists (a real pixel of a real channel)
__device__ __forceinline__ void fid_count(Acc& a, int v, float f, float scale, bool ok) {
  const bool fin = ok && __builtin_fabsf(f) < __builtin_inff();            // (NaN compares false)
  const float t = f * scale;
  const bool big = __builtin_fabsf(t) >= 65536.0f;
  const int r = (int)__builtin_rintf((fin && !big) ? t : 0.0f);
  const int e = !fin ? 0 : big ? (t < 0.0f ? -65536 : 65536) : r;
  v = fin ? v : 0;
  a.flags += fin ? (big ? 0x10000u : 0u) : (ok ? 1u : 0u);
  const int d = 256 * v - e;
  const uint32_t ad = (uint32_t)(d < 0 ? -d : d), ae = (uint32_t)(e < 0 ? -e : e);
  a.maxd = max(a.maxd, ad);
  a.sd += d;
  a.sad += ad;
  a.d2 += (unsigned long long)ad * ad;
  a.sae += ae;
  a.e2 += (unsigned long long)ae * ae;
  a.sv2 += (uint32_t)(v * v);
  const uint32_t m = (ad + 128u) >> 8;                                       // <= 384
  const int k = min(7, 32 - __clz((int)m));                                  // bit length; __clz(0) = 32
  a.hist += (1ull << (9 * k)) >> 9;                                          // k = 0 adds nothing
}

struct Red {
  int w[kRed32][kFidChans];
  unsigned long long q[2][kFidChans];
};

__device__ __forceinline__ void red_clear(Red& R) {
  for (int i = threadIdx.x; i < kRed32 * kFidChans; i += kThreads) (&R.w[0][0])[i] = 0;
  for (int i = threadIdx.x; i < 2 * kFidChans; i += kThreads) (&R.q[0][0])[i] = 0;
}

// valid: the real values the thread counted (finite or not)
__device__ __forceinline__ void red_add(Red& R, int ch, const Acc& a, int valid) {
  const int nonfin = (int)(a.flags & 0xffffu), clamp = (int)(a.flags >> 16);
  if (valid - nonfin) atomicAdd(&R.w[0][ch], valid - nonfin);
  if (nonfin) atomicAdd(&R.w[1][ch], nonfin);
  if (clamp) atomicAdd(&R.w[2][ch], clamp);
  if (a.maxd) atomicMax(&R.w[3][ch], (int)a.maxd);
  if (a.sd) atomicAdd(&R.w[4][ch], a.sd);
  if (a.sad) atomicAdd(&R.w[5][ch], (int)a.sad);
  if (a.sae) atomicAdd(&R.w[6][ch], (int)a.sae);
  if (a.sv2) atomicAdd(&R.w[7][ch], (int)a.sv2);
#pragma unroll
  for (int k = 1; k < 8; k++) {
    const int h = (int)((a.hist >> (9 * (k - 1))) & 511u);
    if (h) atomicAdd(&R.w[7 + k][ch], h);
  }
  if (a.d2) atomicAdd(&R.q[0][ch], a.d2);
  if (a.e2) atomicAdd(&R.q[1][ch], a.e2);
}

// a channel's record from a block's counters
__device__ __forceinline__ void flush_record(long long* rec, long long n, long long nonfin, long long clamp, long long maxd, long long sd,
                                             long long sad, unsigned long long d2, long long sae, unsigned long long e2, long long sv2,
                                             const long long (&h)[7]) {
  unsigned long long* const u = reinterpret_cast<unsigned long long*>(rec);
  add64(u + 0, n); add64(u + 1, nonfin); add64(u + 2, clamp);
  if (maxd) atomicMax(rec + 3, maxd);
  add64(u + 4, sd); add64(u + 5, sad); add64(u + 6, (long long)d2); add64(u + 7, sae); add64(u + 8, (long long)e2);
  add64(u + 9, sv2 << (2 * kFidFrac));
  long long h0 = n;
#pragma unroll
  for (int k = 0; k < 7; k++) { h0 -= h[k]; add64(u + 11 + k, h[k]); }
  add64(u + 10, h0);
}

// Four consecutive pixels (from P, all < end) of channel c of the reference: ((b C + c) HW + i) per pixel
__device__ __forceinline__ float4 load_ref4(const float* ref, bool aligned, uint32_t P, uint32_t end, int c, int C, uint32_t hw) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (P >= end) return x;
  const uint32_t b = P / hw, i = P - b * hw;
  const long long at = ((long long)b * C + c) * hw + i;
  if (aligned && i + 3 < hw && P + 3 < end && (at & 3) == 0) return *reinterpret_cast<const float4*>(ref + at);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t Pj = P + j;
    if (Pj < end) {
      const uint32_t bj = Pj / hw, ij = Pj - bj * hw;
      const float v = ref[((long long)bj * C + c) * hw + ij];
      if (j == 0) x.x = v; else if (j == 1) x.y = v; else if (j == 2) x.z = v; else x.w = v;
    }
  }
  return x;
}

__global__ __launch_bounds__(kThreads) void fid_rows_kernel(FidRowsArgs p) {
  __shared__ float tile[2][kFidChans * kPitch];
  __shared__ Red red;
  int r;
  TF2_ROW_OF_BLOCK(r, p);
  const FidRow& R = p.rows[r];
  const int C = R.c, cp = R.cp;
  const uint32_t hw = (uint32_t)R.hw;
  const int n_cpass = (C + kFidChans - 1) / kFidChans;
  const int local = (int)blockIdx.x - R.block0;
  const int slab = local / n_cpass, cpass = local - slab * n_cpass;
  const uint32_t pix0 = (uint32_t)slab * kFidSlab;
  const uint32_t end = min(pix0 + (uint32_t)kFidSlab, (uint32_t)R.npix);
  const int tiles = (int)((end - pix0 + kFidTile - 1) / kFidTile);
  const int c0 = cpass * kFidChans;
  const bool aligned = ((uintptr_t)R.ref & 15) == 0;

  red_clear(red);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the float side: this thread's four pixels of channels lc, lc + 16, lc + 32, lc + 48 of the block
  const int lc = threadIdx.x >> 4, lp = (threadIdx.x & 15) * 4;
  // the int8 side: this thread's channel, the wave's pixels of a tile
  const int c = c0 + lane;
  const bool c_ok = c < C;
  const bool dbl = c_ok && R.dbl != nullptr && R.dbl[c] != 0;
  const int dadd = dbl ? 128 : 0, dsh = dbl ? 1 : 0;                // 2y - 128 -> y = (v + 128) >> 1
  const float scale = c_ok ? p.scales[R.rec0 + c] : 0.0f;
  const int8_t* const col = R.base + min(c, C - 1);                 // (a lane past the row's channels, a pixel past the slab's end: loads
                                                                    //  without a branch from the last real one, never counted)

  float4 nf[4];
  int nv[kPixPerWave];
  auto load_tile = [&](int t) {
    const uint32_t P = pix0 + (uint32_t)t * kFidTile;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      nf[i] = load_ref4(R.ref, aligned, P + lp, end, min(c0 + lc + 16 * i, C - 1), C, hw);
    }
#pragma unroll
    for (int j = 0; j < kPixPerWave; j++) {
      const uint32_t Pj = min(P + wave * kPixPerWave + j, end - 1);
      nv[j] = (int)col[(long long)Pj * cp];
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      float* const d = &tile[buf][(lc + 16 * i) * kPitch + lp];
      d[0] = nf[i].x; d[1] = nf[i].y; d[2] = nf[i].z; d[3] = nf[i].w;
    }
  };

  Acc a;
  acc_init(a);
  int valid = 0;
  load_tile(0);
  store_tile(0);
  int cv[kPixPerWave];
#pragma unroll
  for (int j = 0; j < kPixPerWave; j++) cv[j] = nv[j];
  __syncthreads();
  for (int t = 0; t < tiles; t++) {
    const int buf = t & 1;
    if (t + 1 < tiles) load_tile(t + 1);
    const uint32_t P = pix0 + (uint32_t)t * kFidTile + wave * kPixPerWave;
    const float* const line = &tile[buf][lane * kPitch + wave * kPixPerWave];
    valid += P < end ? (int)min((uint32_t)kPixPerWave, end - P) : 0;
#pragma unroll
    for (int j = 0; j < kPixPerWave; j++) fid_count(a, (cv[j] + dadd) >> dsh, line[j], scale, c_ok && P + j < end);
    if (t + 1 < tiles) {
      store_tile(buf ^ 1);
#pragma unroll
      for (int j = 0; j < kPixPerWave; j++) cv[j] = nv[j];
    }
    __syncthreads();
  }
  if (c_ok) red_add(red, lane, a, valid);
  __syncthreads();

  const int tch = threadIdx.x, oc = c0 + tch;
  if (tch < kFidChans && oc < C) {
    long long h[7];
#pragma unroll
    for (int k = 0; k < 7; k++) h[k] = red.w[8 + k][tch];
    flush_record(p.store + (long long)(R.rec0 + oc) * kFidSlots, red.w[0][tch], red.w[1][tch], red.w[2][tch], red.w[3][tch], red.w[4][tch],
                 (uint32_t)red.w[5][tch], red.q[0][tch], (uint32_t)red.w[6][tch], red.q[1][tch], (uint32_t)red.w[7][tch], h);
  }
}

__global__ __launch_bounds__(kThreads) void fid_image_kernel(FidImgArgs p) {
  __shared__ Red red;
  const int plane = (int)blockIdx.x / p.slabs, slab = (int)blockIdx.x - plane * p.slabs;
  const int ch = plane % p.c;
  const int v0 = slab * kFidImgSlab;
  const int sv = min(kFidImgSlab, p.hw - v0);
  const float* const src = p.images + (long long)plane * p.hw + v0;
  red_clear(red);
  __syncthreads();
  Acc a;
  acc_init(a);
  for (int i = (int)threadIdx.x; i < sv; i += kThreads) {
    const float f = src[i];
    fid_count(a, quant_input(f, p.trans), f, p.scale, true);
  }
  const int lane = threadIdx.x & 63;
  red_add(red, lane, a, (int)threadIdx.x < sv ? (sv - (int)threadIdx.x + kThreads - 1) / kThreads : 0);   // the block's waves meet lane by lane ...
  __syncthreads();
  if (threadIdx.x < 64) {                                           // ... and wave 0 folds the 64 lanes
    long long w[kRed32];
#pragma unroll
    for (int s = 0; s < kRed32; s++) {
      const int v = s == 3 ? wave_max(red.w[s][lane]) : wave_sum(red.w[s][lane]);
      w[s] = s == 5 || s == 6 || s == 7 ? (long long)(uint32_t)v : (long long)v;
    }
    const unsigned long long d2 = wave_sum(red.q[0][lane]), e2 = wave_sum(red.q[1][lane]);
    if (lane == 0) {
      const long long h[7] = {w[8], w[9], w[10], w[11], w[12], w[13], w[14]};
      flush_record(p.store + (long long)ch * kFidSlots, w[0], w[1], w[2], w[3], w[4], w[5], d2, w[6], e2, w[7], h);
    }
  }
}

}  // namespace

// ---- the handle --------------------------------------------------------------------------------------------------------
tf2_status Comparator::create(Net* n) {
  if (tf2_status st = g.create(n)) return st;
  if (n->q.size() < (size_t)(n->nd.n_layers + 1) * n->nd.max_out_channel) { set_error("tf2_fid_create: q table not set (tf2_net_set_q first)"); return TF2_ERR_STATE; }
  scale.assign((size_t)g.n_records, 0.0f);
  const int M = n->nd.max_out_channel;
  for (const ActRows::Row& row : g.rows)
    for (int c = 0; c < row.C; c++) {
      const int Q = -(int)(row.layer < 0 ? n->q[0] : n->q[(size_t)(row.layer + 1) * M + c]);     // Verify: 1 << -q[l + 1][c]; the input: q[0][0]
      if (Q + kFidFrac > 127 || Q + kFidFrac < -126) { set_error("tf2_fid_create: row " + std::to_string(row.layer) + ": 2^(Q + 8) is no normal float32"); return TF2_ERR_UNSUPPORTED; }
      scale[(size_t)row.rec0 + c] = std::ldexp(1.0f, Q + kFidFrac);
    }
  return TF2_OK;
}

tf2_status Comparator::store_init(void* store, size_t store_bytes, void* stream) const {
  if (!store) return arg_refusal("tf2_fid_store_init", "null store_dev");
  if (store_bytes < store_size()) { set_error("tf2_fid_store_init: store too small (tf2_fid_store_size: " + std::to_string(store_size()) + ")"); return TF2_ERR_SIZE; }
  if (hipMemsetAsync(store, 0, store_size(), (hipStream_t)stream) != hipSuccess) { set_error(std::string("tf2_fid_store_init: memset failed: ") + hipGetErrorString(hipGetLastError())); return TF2_ERR_HIP; }
  return TF2_OK;
}

// with_step: the keep_all step first (tf2_fid_run); without, the comparison alone of a workspace that holds one (tf2_fid_kept)
tf2_status Comparator::run(const void* images, bool images_are_q, int batch, void* ws, size_t ws_bytes, int8_t* logits, void* store,
                           size_t store_bytes, const float* const* refs, const float* scales_dev, void* stream, bool with_step) {
  Net* const net = g.net;
  KeptMaps kept;
  if (tf2_status st = kept.open(g, "tf2_fid", !images || !ws || (with_step && !logits) || !store || !refs || !scales_dev, "null pointer", batch, ws,
                                ws_bytes, store_bytes, store_size(), kFidSlab))
    return st;
  // every row and the grids, before anything is enqueued
  FidRowsArgs first{};
  first.store = (long long*)store; first.scales = scales_dev;
  LaunchBatch<FidRowsArgs, FidRow, kFidRowsPerLaunch> rows("tf2_fid_run", first);
  for (int l = 0; l < net->nd.n_layers; l++) {
    KeptMap m;
    if (tf2_status st = kept.map(l, m)) return st;
    if (!refs[l]) continue;
    FidRow* const R = rows.add((m.npix + kFidSlab - 1) / kFidSlab * ((m.C + kFidChans - 1) / kFidChans));
    if (!R) return TF2_ERR_UNSUPPORTED;
    R->base = m.base; R->dbl = m.dbl;
    R->ref = refs[l];
    R->npix = (int32_t)m.npix; R->c = m.C; R->cp = m.Cp; R->hw = m.HW;
    R->rec0 = (int32_t)m.rec0;
  }
  FidImgArgs I{};
  I.images = (const float*)images; I.store = (long long*)store; I.trans = std::ldexp(1.0f, -(int)net->q[0]); I.scale = scale[0];
  I.c = net->nd.image_c; I.hw = net->nd.image_h * net->nd.image_w; I.planes = batch * I.c;
  I.slabs = (I.hw + kFidImgSlab - 1) / kFidImgSlab;

  if (with_step)
    if (tf2_status st = net->run(images, images_are_q, batch, ws, ws_bytes, logits, stream)) return st;
  if (!images_are_q) {
    hipLaunchKernelGGL(fid_image_kernel, dim3((unsigned)((long long)I.planes * I.slabs)), dim3(kThreads), 0, (hipStream_t)stream, I);
    if (tf2_status st = launch_result("tf2_fid_run", "input launch failed")) return st;
  }
  for (size_t i = 0; i < rows.launches.size(); i++) {
    hipLaunchKernelGGL(fid_rows_kernel, dim3((unsigned)rows.blocks[i]), dim3(kThreads), 0, (hipStream_t)stream, rows.launches[i]);
    if (tf2_status st = launch_result("tf2_fid_run")) return st;
  }
  return TF2_OK;
}

}  // namespace tf2
