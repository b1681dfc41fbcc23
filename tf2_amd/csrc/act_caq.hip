// act_caq.hip -- CAQ calibration (tf2_caq_*, include/tf2_amd.h): the float32 maps of a float forward, read once, into exact per-channel
// integer records in a caller-owned device store, with no host copy and no synchronisation.  tf2_amd/caq.py states both records
// (reference_range / reference_error); the stores equal it as integers, whatever the grid and the order of the blocks: every counter
// is an integer added (or maximised) with a 64-bit atomic.  act_rows.h holds what this file shares with act_audit and act_fidelity: the
// rows dealt to launches (LaunchBatch), the block-to-row search, add64 and the wave reductions.
//
// caq_range_kernel   pass 1.  Per value, on the bit pattern (mag = bits & 0x7fffffff): mag >= 0x7f800000 -> nonfinite, nothing else;
//                    mag == 0 -> zeros; otherwise the sign picks negatives and the peak it may raise, and the value falls into
//                    hist[clamp(fit, -32, 31) + 32] with fit = 133 - ((mag + 0x1ffff) >> 23): 133 - E of the biased exponent E, one less
//                    where the significand exceeds 0xFE0000 (the carry).  A denormal gives 132 or 133 there, its true fit is >= 132:
//                    both clamp to 31.
// caq_error_kernel   pass 2.  t = f * 2^(Qb + 7) from the scale table, e = rint(t) or +-2^18, then the four candidates in registers:
//                    u = (e + (1 << (s - 1))) >> s, v = clamp(u, -128, 127), d = e - (v << s), s = 7 - j.
//
// Both kernels walk the maps the same way (walk_channel).  A block owns kCaqSlab values of ONE channel of one row, taken over all
// images in (b, i) order, so a 7 x 7 plane is walked by one block through all its images; its waves share them evenly.  The data
// are NCHW: plane (b, c) is a contiguous run of hw floats whose start is only 4-byte aligned, so a wave reads ALIGNED groups of four
// values -- one 16-byte load where the whole group belongs to the wave's share of the plane, guarded single loads at the head and the
// tail -- and nothing outside its share is ever read.  Where a plane has fewer than 64 groups the wave's lanes are dealt over
// 64 / groups planes at once (hw = 49: four planes a pass, 52 lanes; hw = 1: a plane a lane).  All loops are wave-uniform; a value
// that does not exist is counted as "not ok" and adds nothing.
// The histogram of pass 1 costs no LDS traffic in the loop: lane L of a wave keeps the count of bin L, and the wave counts the
// distinct bins present (three to six in a channel) by ballot and population count.  The waves meet in LDS once a slab, then the block
// issues 64-bit atomics for the non-zero counters only.
//
//   kernel             VGPRs  scratch  static LDS
//   caq_range_kernel   26     0        276
//   caq_error_kernel   45     0        72
// Measured on an MI355X, ResNet-50 at batch 32 (tools/caq_time.py, profiles/caq_time_b32.json; 1.352 GB of float32 maps, 55 rows, one
// launch a pass): pass 1 0.643 ms = 2.10 TB/s, pass 2 0.876 ms = 1.54 TB/s, beside 0.661 ms of tf2_fid_kept for the same floats in the
// same job.  A first version -- 8192 values a block, a fixed 2048 a wave, 64-bit index compares for every value -- took 0.942 and
// 1.444 ms: a channel of 7 x 7 planes (1568 values at batch 32) kept three of a block's four waves idle, and the block's end (wave
// reductions, LDS, atomics) was a quarter of the error kernel's block.  An even share for every wave, 32768 values a block and 32-bit
// indices relative to the wave's share gave the figures above.  Not tried: the next group's load issued before the current one is
// counted; lanes along channels for the hw = 1 rows (one block a channel as it stands: 3 of ResNet-50's 55 rows, 0.4 MB).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>
#include "tf2_device.h"
#include "act_caq.h"

namespace tf2 {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kCaqSlab % (kWaves * kCaqGroup) == 0 && kCaqGroup == 4, "a wave's share of a whole slab is whole groups of four");
static_assert(kCaqSlab / kWaves / 64 * 8 <= 1024, "a lane sees at most 2^10 values: a 64th of its wave's share, a few times that where planes are short");
static_assert(kCaqBins == 64, "a lane a bin");

// The values [wv0, wv1) of channel c of row R (a channel's values in (b, i) order: v = b * hw + i), every one handed to acc.count(bits,
// true) exactly once; the calls are made by all 64 lanes together (acc.count may use wave-wide operations), a lane without a value
// passes ok = false.  wv0 < wv1 and both are the same in every lane.
template <class Acc>
__device__ __forceinline__ void walk_channel(const CaqRow& R, int c, int wv0, int wv1, int lane, Acc& acc) {
  const int hw = R.hw;
  const int mis = (int)(((uintptr_t)R.map >> 2) & 3);    // floats from the 16-byte boundary below the map to its first value
  const uint32_t* const base = R.map - mis;               // 16-byte aligned; never read below the wave's share
  const int G = (hw + 6) / 4;                             // aligned groups n <= hw consecutive values can touch: at most (n + 2) / 4 + 1
  const int lpp = G < 64 ? G : 64;                        // lanes a plane
  const int ppp = 64 / lpp;                               // planes a pass
  const int iters = (G + lpp - 1) / lpp;
  const int slot = lane / lpp, gi = lane - slot * lpp;
  const int b0 = wv0 / hw, b1 = (wv1 - 1) / hw;
  for (int pb = b0; pb <= b1; pb += ppp) {
    const int b = pb + slot;
    const bool live = slot < ppp && b <= b1;
    const long long first = (long long)b * hw;            // the plane's first value in the channel's order
    const int i_lo = (int)max((long long)wv0 - first, 0ll), i_hi = (int)min((long long)wv1 - first, (long long)hw);
    const long long E = ((long long)b * R.c + c) * hw + mis;       // the plane's first value, in floats from `base`
    const long long A_lo = E + i_lo;                      // the share's first value, in floats from `base`
    const uint32_t n = live ? (uint32_t)(i_hi - i_lo) : 0u;
    const uint32_t off = (uint32_t)(A_lo & 3);
    const uint32_t* const pg = base + (A_lo - off);       // the aligned group that holds it
    uint32_t r = 4u * (uint32_t)gi - off;                 // the lane's group from the share's first value: element k is real where r + k < n
    for (int it = 0; it < iters; it++, r += 4u * (uint32_t)lpp) {
      const bool k0 = r < n, k1 = r + 1u < n, k2 = r + 2u < n, k3 = r + 3u < n;      // (unsigned: a value in front of the share wraps)
      const uint32_t* const q = pg + (int)(r + off);
      uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
      if (k0 && k3) {
        const uint4 x = *reinterpret_cast<const uint4*>(q);
        x0 = x.x; x1 = x.y; x2 = x.z; x3 = x.w;
      } else {
        if (k0) x0 = q[0];
        if (k1) x1 = q[1];
        if (k2) x2 = q[2];
        if (k3) x3 = q[3];
      }
      acc.count(x0, k0); acc.count(x1, k1); acc.count(x2, k2); acc.count(x3, k3);
    }
  }
}

// The block's row and channel and the wave's share of its values (wv0 == wv1: the wave has nothing to walk)
struct Share {
  int r, c, wv0, wv1, valid;          // valid: the values of the whole block
};
__device__ __forceinline__ Share share_of(const CaqArgs& p, int wave) {
  Share s;
  TF2_ROW_OF_BLOCK(s.r, p);
  const CaqRow& R = p.rows[s.r];
  const int local = (int)blockIdx.x - R.block0;
  const int slab = local / R.c;
  s.c = local - slab * R.c;
  const int v0 = slab * kCaqSlab, v1 = min(v0 + kCaqSlab, R.total);
  s.valid = v1 - v0;
  const int span = (((s.valid + kWaves - 1) / kWaves) + kCaqGroup - 1) & ~(kCaqGroup - 1);     // the waves share what there is
  s.wv0 = min(v0 + wave * span, v1);
  s.wv1 = min(s.wv0 + span, v1);
  return s;
}

struct RangeAcc {
  uint32_t nonfin, zeros, negs, ppos, pneg, hist;                   // hist: lane L holds the wave's count of bin L
  int lane;
  __device__ __forceinline__ void count(uint32_t bits, bool ok) {
    const uint32_t mag = bits & 0x7fffffffu;
    const bool fin = ok && mag < 0x7f800000u;
    const bool nz = fin && mag != 0u;
    const bool neg = nz && (bits >> 31) != 0u;
    nonfin += (ok && !fin) ? 1u : 0u;
    zeros += (fin && !nz) ? 1u : 0u;
    negs += neg ? 1u : 0u;
    ppos = max(ppos, (nz && !neg) ? mag : 0u);
    pneg = max(pneg, neg ? mag : 0u);
    const int fit = 133 - (int)((mag + 0x1ffffu) >> 23);
    const int bin = nz ? min(max(fit, -32), 31) + 32 : -1;
    unsigned long long rem = __ballot(nz);
    while (rem) {                                                   // the distinct bins present, one a turn
      const int b = __builtin_amdgcn_readlane(bin, __builtin_ctzll(rem));
      const unsigned long long m = __ballot(bin == b);
      hist += lane == b ? (uint32_t)__popcll(m) : 0u;
      rem &= ~m;
    }
  }
};

struct ErrorAcc {
  float scale;
  uint32_t nonfin, clamped, clip[kCaqCands];
  unsigned long long e2, d2[kCaqCands];
  __device__ __forceinline__ void count(uint32_t bits, bool ok) {
    const bool fin = ok && (bits & 0x7fffffffu) < 0x7f800000u;
    nonfin += (ok && !fin) ? 1u : 0u;
    const float t = __uint_as_float(bits) * scale;
    const bool big = fin && __builtin_fabsf(t) >= (float)kCaqELimit;             // (an overflow to inf included)
    const int r = (int)__builtin_rintf((fin && !big) ? t : 0.0f);
    const int e = big ? (t < 0.0f ? -kCaqELimit : kCaqELimit) : r;
    clamped += big ? 1u : 0u;
    const uint32_t ae = (uint32_t)(e < 0 ? -e : e);
    e2 += (unsigned long long)ae * ae;
#pragma unroll
    for (int j = 0; j < kCaqCands; j++) {
      const int s = kCaqFrac - j;
      const int u = (e + (1 << (s - 1))) >> s;
      const int v = min(max(u, -128), 127);
      clip[j] += u != v ? 1u : 0u;
      const int d = e - v * (1 << s);
      const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
      d2[j] += (unsigned long long)ad * ad;
    }
  }
};

__global__ __launch_bounds__(kThreads) void caq_range_kernel(CaqArgs p) {
  __shared__ uint32_t sh_hist[kCaqBins];
  __shared__ uint32_t sh_s[5];                                      // nonfinite, zeros, negatives, peak_pos, peak_neg
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const Share s = share_of(p, wave);
  if (threadIdx.x < kCaqBins) sh_hist[threadIdx.x] = 0;
  if (threadIdx.x < 5) sh_s[threadIdx.x] = 0;
  __syncthreads();
  if (s.wv0 < s.wv1) {
    RangeAcc a;
    a.nonfin = a.zeros = a.negs = a.ppos = a.pneg = a.hist = 0;
    a.lane = lane;
    walk_channel(p.rows[s.r], s.c, s.wv0, s.wv1, lane, a);
    if (a.hist) atomicAdd(&sh_hist[lane], a.hist);
    const uint32_t nonfin = wave_sum(a.nonfin), zeros = wave_sum(a.zeros), negs = wave_sum(a.negs);
    const uint32_t ppos = wave_max(a.ppos), pneg = wave_max(a.pneg);
    if (lane == 0) {
      if (nonfin) atomicAdd(&sh_s[0], nonfin);
      if (zeros) atomicAdd(&sh_s[1], zeros);
      if (negs) atomicAdd(&sh_s[2], negs);
      if (ppos) atomicMax(&sh_s[3], ppos);
      if (pneg) atomicMax(&sh_s[4], pneg);
    }
  }
  __syncthreads();
  long long* const rec = p.store + (long long)(p.rows[s.r].rec0 + s.c) * kCaqRangeSlots;
  const int t = threadIdx.x;
  if (t < kCaqBins) add64(rec + 6 + t, sh_hist[t]);
  else if (t == 64) add64(rec + 0, (unsigned long long)(s.valid - (int)sh_s[0]));
  else if (t <= 67) add64(rec + (t - 64), sh_s[t - 65]);            // 65 nonfinite, 66 zeros, 67 negatives
  else if (t <= 69) { if (sh_s[t - 65]) atomicMax(rec + (t - 64), (long long)sh_s[t - 65]); }     // 68 peak_pos, 69 peak_neg
}

__global__ __launch_bounds__(kThreads) void caq_error_kernel(CaqArgs p) {
  __shared__ unsigned long long sh_q[1 + kCaqCands];                // sum_e2, sum_d2[4]
  __shared__ uint32_t sh_w[2 + kCaqCands];                          // nonfinite, ref_clamped, clipped[4]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const Share s = share_of(p, wave);
  if (threadIdx.x < 1 + kCaqCands) sh_q[threadIdx.x] = 0;
  if (threadIdx.x < 2 + kCaqCands) sh_w[threadIdx.x] = 0;
  __syncthreads();
  const int record = p.rows[s.r].rec0 + s.c;
  if (s.wv0 < s.wv1) {
    ErrorAcc a;
    a.scale = p.scales[record];
    a.nonfin = a.clamped = 0;
    a.e2 = 0;
#pragma unroll
    for (int j = 0; j < kCaqCands; j++) { a.clip[j] = 0; a.d2[j] = 0; }
    walk_channel(p.rows[s.r], s.c, s.wv0, s.wv1, lane, a);
    const uint32_t nonfin = wave_sum(a.nonfin), clamped = wave_sum(a.clamped);
    const unsigned long long e2 = wave_sum(a.e2);
    uint32_t clip[kCaqCands];
    unsigned long long d2[kCaqCands];
#pragma unroll
    for (int j = 0; j < kCaqCands; j++) { clip[j] = wave_sum(a.clip[j]); d2[j] = wave_sum(a.d2[j]); }
    if (lane == 0) {
      if (nonfin) atomicAdd(&sh_w[0], nonfin);
      if (clamped) atomicAdd(&sh_w[1], clamped);
      if (e2) atomicAdd(&sh_q[0], e2);
#pragma unroll
      for (int j = 0; j < kCaqCands; j++) {
        if (clip[j]) atomicAdd(&sh_w[2 + j], clip[j]);
        if (d2[j]) atomicAdd(&sh_q[1 + j], d2[j]);
      }
    }
  }
  __syncthreads();
  long long* const rec = p.store + (long long)record * kCaqErrorSlots;
  const int t = threadIdx.x;
  if (t == 0) add64(rec + 0, (unsigned long long)(s.valid - (int)sh_w[0]));
  else if (t <= 2) add64(rec + t, sh_w[t - 1]);                     // 1 nonfinite, 2 ref_clamped
  else if (t == 3) add64(rec + 3, sh_q[0]);
  else if (t <= 7) add64(rec + t, sh_w[t - 2]);                     // 4..7 clipped[j]
  else if (t <= 11) add64(rec + t, sh_q[t - 7]);                    // 8..11 sum_d2[j]
}

}  // namespace

tf2_status caq_store_init(void* store, size_t store_bytes, void* stream) {
  if (!store) return arg_refusal("tf2_caq_store_init", "null store_dev");
  if (store_bytes == 0 || store_bytes % 8 != 0 || ((uintptr_t)store & 7) != 0) return arg_refusal("tf2_caq_store_init", "the store is whole, 8-byte aligned int64 words");
  if (hipMemsetAsync(store, 0, store_bytes, (hipStream_t)stream) != hipSuccess) { set_error(std::string("tf2_caq_store_init: memset failed: ") + hipGetErrorString(hipGetLastError())); return TF2_ERR_HIP; }
  return TF2_OK;
}

tf2_status caq_run(bool error, const tf2_caq_row* rows, const void* const* maps, int n_rows, int batch, const float* scales_dev,
                   void* store, size_t store_bytes, void* stream) {
  const std::string who = error ? "tf2_caq_error: " : "tf2_caq_range: ";
  if (!rows || !maps || !store || (error && !scales_dev)) { set_error(who + "null pointer"); return TF2_ERR_ARG; }
  if (n_rows < 1) { set_error(who + "n_rows must be positive"); return TF2_ERR_ARG; }
  if (batch <= 0) { set_error(who + "batch must be positive"); return TF2_ERR_ARG; }
  if (((uintptr_t)store & 7) != 0) { set_error(who + "store_dev is not 8-byte aligned"); return TF2_ERR_ARG; }
  const long long slots = error ? kCaqErrorSlots : kCaqRangeSlots;
  const long long capacity = (long long)(store_bytes / (size_t)(slots * 8));
  // every row and the grids, before anything is enqueued
  std::vector<std::pair<long long, long long>> spans;
  long long last = 0;
  for (int i = 0; i < n_rows; i++) {
    const tf2_caq_row& r = rows[i];
    if (r.C <= 0 || r.HW <= 0 || r.first_record < 0) { set_error(who + "row " + std::to_string(i) + ": C, HW must be positive, first_record not negative"); return TF2_ERR_ARG; }
    if (r.first_record + r.C > 0x7fffffffll) { set_error(who + "row " + std::to_string(i) + ": record index beyond 2^31"); return TF2_ERR_UNSUPPORTED; }
    if ((long long)batch * r.HW + kCaqSlab > 0x7fffffffll) { set_error(who + "row " + std::to_string(i) + ": batch * HW beyond 2^31"); return TF2_ERR_UNSUPPORTED; }
    if (((uintptr_t)maps[i] & 3) != 0) { set_error(who + "row " + std::to_string(i) + ": map is not 4-byte aligned"); return TF2_ERR_ARG; }
    spans.emplace_back((long long)r.first_record, (long long)(r.first_record + r.C));
    last = std::max(last, (long long)(r.first_record + r.C));
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); i++)
    if (spans[i].first < spans[i - 1].second) { set_error(who + "the rows' record ranges overlap"); return TF2_ERR_ARG; }
  if (last > capacity) {
    set_error(who + "store too small: the rows reach record " + std::to_string(last) + ", store_bytes holds " + std::to_string(capacity));
    return TF2_ERR_SIZE;
  }
  CaqArgs first{};
  first.store = (long long*)store; first.scales = error ? scales_dev : nullptr;
  LaunchBatch<CaqArgs, CaqRow, kCaqRowsPerLaunch> batches(error ? "tf2_caq_error" : "tf2_caq_range", first);
  for (int i = 0; i < n_rows; i++) {
    if (!maps[i]) continue;                                          // not observed: no block, its records stay
    const int total = batch * rows[i].HW, n_slabs = (total + kCaqSlab - 1) / kCaqSlab;
    CaqRow* const R = batches.add((long long)n_slabs * rows[i].C);
    if (!R) return TF2_ERR_UNSUPPORTED;
    R->map = (const uint32_t*)maps[i];
    R->c = rows[i].C; R->hw = rows[i].HW; R->total = total;
    R->n_slabs = n_slabs;
    R->rec0 = (int32_t)rows[i].first_record;
  }
  for (size_t i = 0; i < batches.launches.size(); i++) {
    if (error) hipLaunchKernelGGL(caq_error_kernel, dim3((unsigned)batches.blocks[i]), dim3(kThreads), 0, (hipStream_t)stream, batches.launches[i]);
    else hipLaunchKernelGGL(caq_range_kernel, dim3((unsigned)batches.blocks[i]), dim3(kThreads), 0, (hipStream_t)stream, batches.launches[i]);
    if (tf2_status st = launch_result(batches.fn.c_str())) return st;
  }
  return TF2_OK;
}

}  // namespace tf2
