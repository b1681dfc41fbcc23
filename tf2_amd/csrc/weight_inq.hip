// weight_inq.hip -- INQ weight quantisation on the device (tf2_inq_*, include/tf2_amd.h): float32 weights to 0 / +-2^e, many tensors
// ("segments") of one flat buffer a call, in place, with a parallel uint8 mask (1: still float, 0: quantised).  The rule is the
// reference's ComputeQuantumRange + ShapeIntoTwoPower (TransForm_Kit/Compression/compress_net/core/compress_core.py) stated on float
// bit patterns; tf2_amd/inq.py (reference_range / reference_step) is that statement in numpy, and weights, masks, codes and every word
// of the record equal it as bits, whatever the grid and the order of the blocks: integer adds, maxima and plain stores only.
//
// A block owns kInqChunk consecutive elements of the flat buffer and walks the segments that meet its chunk one after the other, so an
// element is always counted for its own segment and elements in no segment are never touched.  A lane takes groups of four elements
// on 16-byte boundaries: one 16-byte load (and one dword of mask) where the whole group lies inside the segment, element by element at
// a segment's unaligned head and tail.  The segment table travels in the kernel arguments, kInqSegsPerLaunch segments a launch.
//
// inq_init_kernel     zeroes the records and the select's scratch, so that a replay on refilled weights equals a fresh call.
// inq_range_kernel    per segment n1, n0, the largest magnitude pattern over mask 1 and over mask 0, the non-finite count: lanes reduce
//                     with shuffles, waves through LDS atomics, one thread a block issues the 64-bit atomics.
// inq_plan_kernel     one thread a segment: max_exp, min_exp, n_keep = rint(rint(n1 / (1 - prev)) * (1 - cur)) in double, n_update, status.
// inq_hist_kernel     one radix-select pass: the digit (8, 8, 8, 7 bits from the top of the 31-bit magnitude) of every mask-1 value whose
//                     higher bits equal the prefix found so far, counted in a block-local LDS histogram; the non-zero bins go to the
//                     segment's histogram of that pass with integer atomics.
// inq_resolve_kernel  one block a segment between passes: the digit whose bin holds rank n_keep, the rank inside that bin.  After the
//                     last pass the prefix is the threshold pattern: the element of index n_keep in the ascending order of |w| over mask 1.
// inq_shape_kernel    the elementwise map: a mask-1 weight with |w| >= thr becomes copysign(2^e, w) or +0.0, its mask 0; codes, the
//                     16-bin code histogram and the three counters (wave ballots, LDS, 64-bit atomics for the non-zero ones).
//
//   kernel              VGPRs  scratch  static LDS
//   inq_init_kernel     4      0        0
//   inq_range_kernel    27     0        20
//   inq_plan_kernel     22     0        0
//   inq_hist_kernel     25     0        1 024
//   inq_resolve_kernel  24     0        1 024
//   inq_shape_kernel    38     0        76
// Measured on an MI355X, ResNet-50's stream (25.5 M weights in 55 segments; tools/inq_time.py, profiles/inq_time.json): a step at
// portion 1 takes 0.477 ms, a 0.5 -> 0.75 step 0.504 ms (DESIGN.md "INQ on the device: the select").
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include <vector>
#include "act_rows.h"      // add64
#include "weight_inq.h"

namespace tf2 {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kMag = 0x7fffffffu;
constexpr int kNoExp = -1000;            // "exponent" of zero
static_assert(kInqChunk == kThreads * 16 && kInqBins == kThreads, "four 16-byte groups a lane; one thread a bin");

// exponent of the leading bit: floor(log2 a) (denormals from the leading-bit position)
__device__ __forceinline__ int exp2_of(uint32_t mag) {
  if (mag == 0) return kNoExp;
  const int E = (int)(mag >> 23);
  return E ? E - 127 : (31 - __clz(mag)) - 149;
}

// exp_of: e with 0.75 * 2^e <= a < 1.5 * 2^e, the reference's floor(log(4a/3) / log 2)
__device__ __forceinline__ int exp_of(uint32_t mag) {
  if (mag == 0) return kNoExp;
  const int E = (int)(mag >> 23);
  uint32_t m = mag & 0x7fffffu;
  int e = E - 127;
  if (!E) {
    const int p = 31 - __clz(m);
    e = p - 149;
    m = (m << (23 - p)) & 0x7fffffu;
  }
  return e + (m >= 0x400000u ? 1 : 0);
}

__device__ __forceinline__ uint32_t pow2_bits(int e) { return e >= -126 ? (uint32_t)(e + 127) << 23 : 1u << (e + 149); }   // e in -149 .. 127

struct Grp {
  uint32_t w[4];
  uint32_t m;        // the four mask bytes
  uint32_t valid;    // bit k: element k lies inside [a, b)
  bool full;
};

// the group of four elements from gb (a multiple of 4) of the segment part [a, b)
__device__ __forceinline__ void load_grp(Grp& g, const float* w, const uint8_t* mask, long long gb, long long a, long long b, bool vec) {
  g.full = vec && gb >= a && gb + 4 <= b;
  if (g.full) {
    const uint4 x = *reinterpret_cast<const uint4*>(w + gb);
    g.w[0] = x.x; g.w[1] = x.y; g.w[2] = x.z; g.w[3] = x.w;
    g.m = *reinterpret_cast<const uint32_t*>(mask + gb);
    g.valid = 0xfu;
  } else {
    g.m = 0; g.valid = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const long long i = gb + k;
      g.w[k] = 0;
      if (i >= a && i < b) {
        g.w[k] = __float_as_uint(w[i]);
        g.m |= (uint32_t)mask[i] << (8 * k);
        g.valid |= 1u << k;
      }
    }
  }
}

__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

__device__ __forceinline__ void max64(long long* p, unsigned long long v) {
  if (v) atomicMax(reinterpret_cast<unsigned long long*>(p), v);
}

__global__ __launch_bounds__(kThreads) void inq_init_kernel(unsigned long long* state, long long state_words, unsigned long long* scratch,
                                                            long long scratch_words) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < state_words) state[i] = 0;
  else if (i - state_words < scratch_words) scratch[i - state_words] = 0;
}

__global__ __launch_bounds__(kThreads) void inq_range_kernel(InqArgs p) {
  __shared__ unsigned int red[5];                                    // n1, n0, max1, max0, non-finite
  const long long c0 = p.first + (long long)blockIdx.x * kInqChunk, c1 = c0 + kInqChunk;
  for (int s = 0; s < p.n_segs; s++) {
    const long long a = max(c0, p.off[s]), b = min(c1, p.end[s]);    // (block-uniform)
    if (a >= b) continue;
    if (threadIdx.x < 5) red[threadIdx.x] = 0;
    __syncthreads();
    uint32_t n1 = 0, n0 = 0, mx1 = 0, mx0 = 0, nf = 0;
    const long long g0 = a & ~3ll;
    const int ng = (int)((b - g0 + 3) >> 2);
    for (int g = threadIdx.x; g < ng; g += kThreads) {
      Grp G;
      load_grp(G, p.w, p.mask, g0 + 4ll * g, a, b, p.vec != 0);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if ((G.valid >> k) & 1u) {
          const uint32_t mag = G.w[k] & kMag;
          const bool one = ((G.m >> (8 * k)) & 0xffu) != 0;
          n1 += one ? 1u : 0u;
          n0 += one ? 0u : 1u;
          mx1 = one ? max(mx1, mag) : mx1;
          mx0 = one ? mx0 : max(mx0, mag);
          nf += mag >= 0x7f800000u ? 1u : 0u;
        }
      }
    }
    n1 = wave_add(n1); n0 = wave_add(n0); nf = wave_add(nf);
    mx1 = wave_max(mx1); mx0 = wave_max(mx0);
    if ((threadIdx.x & 63) == 0) {
      if (n1) atomicAdd(&red[0], n1);
      if (n0) atomicAdd(&red[1], n0);
      if (mx1) atomicMax(&red[2], mx1);
      if (mx0) atomicMax(&red[3], mx0);
      if (nf) atomicAdd(&red[4], nf);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long long* const R = p.state + (long long)s * kInqWords;
      add64(R + kInqN1, red[0]); add64(R + kInqN0, red[1]);
      max64(R + kInqMax1, red[2]); max64(R + kInqMax0, red[3]);
      add64(R + kInqNonfinite, red[4]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void inq_plan_kernel(InqPlanArgs p) {
  const int s = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (s >= p.n_segs) return;
  long long* const R = p.state + (long long)s * kInqWords;
  const long long n1 = R[kInqN1];
  const uint32_t max1 = (uint32_t)R[kInqMax1], max0 = (uint32_t)R[kInqMax0];
  long long status = 0;
  int max_exp = -100;
  if (R[kInqNonfinite]) {
    status = TF2_INQ_NONFINITE;                                      // the patterns say nothing about a range
  } else if (n1 == 0) {
    // every weight is quantised: nothing to do
  } else if (max0 == 0) {                                            // nothing but zeros fixed so far: the range is the float weights'
    if (max1 == 0) status |= TF2_INQ_ALL_ZERO;
    else max_exp = exp_of(max1);
  } else {
    max_exp = exp2_of(max0);
    if (max1 != 0 && exp_of(max1) > max_exp) status |= TF2_INQ_RANGE_GREW;
  }
  long long n_keep = n1, n_update = 0;
  if (!status) {
    const double n_init = rint((double)n1 / (1.0 - p.prev));
    n_keep = (long long)rint(n_init * (1.0 - p.cur));
    n_update = n1 - n_keep;
  }
  R[kInqMaxExp] = max_exp;
  R[kInqMinExp] = max_exp - p.n_values + 1;
  R[kInqNKeep] = n_keep;
  R[kInqNUpdate] = n_update;
  R[kInqStatus] = status;
  InqSel S;
  S.rank = (unsigned long long)n_keep; S.prefix = 0; S.active = (!status && n_update > 0) ? 1u : 0u;
  p.sel[s] = S;
}

__global__ __launch_bounds__(kThreads) void inq_hist_kernel(InqArgs p) {
  __shared__ unsigned int h[kInqBins];
  const long long c0 = p.first + (long long)blockIdx.x * kInqChunk, c1 = c0 + kInqChunk;
  const uint32_t dmask = (1u << (p.hi_shift - p.shift)) - 1u;
  for (int s = 0; s < p.n_segs; s++) {
    const long long a = max(c0, p.off[s]), b = min(c1, p.end[s]);
    if (a >= b) continue;
    const InqSel S = p.sel[s];
    if (!S.active) continue;
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t want = S.prefix >> p.hi_shift;
    const long long g0 = a & ~3ll;
    const int ng = (int)((b - g0 + 3) >> 2);
    for (int g = threadIdx.x; g < ng; g += kThreads) {
      Grp G;
      load_grp(G, p.w, p.mask, g0 + 4ll * g, a, b, p.vec != 0);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t mag = G.w[k] & kMag;
        if (((G.valid >> k) & 1u) && ((G.m >> (8 * k)) & 0xffu) && (mag >> p.hi_shift) == want) atomicAdd(&h[(mag >> p.shift) & dmask], 1u);
      }
    }
    __syncthreads();
    const unsigned int c = h[threadIdx.x];
    if (c) atomicAdd(p.hist + ((long long)s * kInqPasses + p.pass) * kInqBins + threadIdx.x, c);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kInqBins) void inq_resolve_kernel(const uint32_t* hist, InqSel* sel, long long* state, int pass, int shift) {
  __shared__ unsigned int h[kInqBins];
  const int s = (int)blockIdx.x, t = (int)threadIdx.x;
  const InqSel S = sel[s];
  if (!S.active) return;
  const unsigned int c = hist[((long long)s * kInqPasses + pass) * kInqBins + t];
  h[t] = c;
  __syncthreads();                                                   // (every thread has read S before one of them writes it)
  unsigned long long below = 0;
  for (int i = 0; i < kInqBins; i++) below += i < t ? h[i] : 0u;
  if (below <= S.rank && S.rank < below + c) {                       // exactly one thread: the bins sum to more than the rank
    const uint32_t prefix = S.prefix | ((uint32_t)t << shift);
    sel[s].rank = S.rank - below;
    sel[s].prefix = prefix;
    if (pass == kInqPasses - 1) state[(long long)s * kInqWords + kInqThr] = prefix;
  }
}

__global__ __launch_bounds__(kThreads) void inq_shape_kernel(InqArgs p) {
  __shared__ unsigned int cnt[19];                                   // 16 codes, flushed under min_exp, under exp_floor, emitted with e > 0
  const long long c0 = p.first + (long long)blockIdx.x * kInqChunk, c1 = c0 + kInqChunk;
  for (int s = 0; s < p.n_segs; s++) {
    const long long a = max(c0, p.off[s]), b = min(c1, p.end[s]);
    if (a >= b) continue;
    long long* const R = p.state + (long long)s * kInqWords;
    const int min_exp = (int)R[kInqMinExp];
    const bool active = R[kInqStatus] == 0 && R[kInqNUpdate] > 0;
    const uint32_t thr = (uint32_t)R[kInqThr];
    if (threadIdx.x < 19) cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t acc[19];                                                // wave-uniform
#pragma unroll
    for (int i = 0; i < 19; i++) acc[i] = 0;
    const long long g0 = a & ~3ll;
    const int ng = (int)((b - g0 + 3) >> 2);
    const int ngr = (ng + 63) & ~63;                                 // whole waves stay together for the ballots
    for (int g = threadIdx.x; g < ngr; g += kThreads) {
      Grp G;
      const long long gb = g0 + 4ll * g;
      if (g < ng) load_grp(G, p.w, p.mask, gb, a, b, p.vec != 0);
      else { G.full = false; G.valid = 0; G.m = 0; G.w[0] = G.w[1] = G.w[2] = G.w[3] = 0; }
      uint32_t nb[4], code[4], keep = 0xffffffffu, any = 0, codes = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t w = G.w[k], mag = w & kMag;
        const bool valid = (G.valid >> k) & 1u;
        const bool one = ((G.m >> (8 * k)) & 0xffu) != 0;
        const bool sel = valid && active && one && mag >= thr;
        bool fmin = false, ffloor = false, over = false;
        nb[k] = w;
        if (sel) {
          nb[k] = 0;
          if (mag) {
            const int e = min(exp_of(mag), 127);
            if (e < min_exp) fmin = true;
            else if (e < p.exp_floor) ffloor = true;
            else { nb[k] = (w & 0x80000000u) | pow2_bits(e); over = e > 0; }
          }
          keep &= ~(0xffu << (8 * k));
          any = 1;
        }
        uint32_t c = 15;
        if (!one || sel) {
          const uint32_t m2 = nb[k] & kMag;
          const int kk = exp2_of(m2) - min_exp;
          c = m2 == 0 ? 7u : (kk >= 0 && kk <= 6) ? (uint32_t)kk + ((nb[k] >> 31) ? 0u : 8u) : 15u;
        }
        code[k] = valid ? c : 0xffu;
        codes |= c << (8 * k);
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] += (uint32_t)__popcll(__ballot(code[k] == (uint32_t)i));
        acc[16] += (uint32_t)__popcll(__ballot(fmin));
        acc[17] += (uint32_t)__popcll(__ballot(ffloor));
        acc[18] += (uint32_t)__popcll(__ballot(over));
      }
      if (G.full) {
        if (any) {
          *reinterpret_cast<uint4*>(p.w + gb) = make_uint4(nb[0], nb[1], nb[2], nb[3]);
          *reinterpret_cast<uint32_t*>(p.mask + gb) = G.m & keep;
        }
        if (p.codes) *reinterpret_cast<uint32_t*>(p.codes + gb) = codes;
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if ((G.valid >> k) & 1u) {
            if (!((keep >> (8 * k)) & 0xffu)) { p.w[gb + k] = __uint_as_float(nb[k]); p.mask[gb + k] = 0; }
            if (p.codes) p.codes[gb + k] = (uint8_t)code[k];
          }
        }
      }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int i = 0; i < 19; i++)
        if (acc[i]) atomicAdd(&cnt[i], acc[i]);
    }
    __syncthreads();
    if (threadIdx.x < 19) {
      const int t = threadIdx.x;
      add64(R + (t < 16 ? kInqHist + t : kInqFlushedMin + (t - 16)), cnt[t]);
    }
    __syncthreads();
  }
}

bool launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return true;
  set_error(std::string("tf2_inq_step: ") + what + " launch failed: " + hipGetErrorString(e));
  return false;
}

}  // namespace

tf2_status inq_step(float* w, uint8_t* mask, long long n_total, const tf2_inq_seg* segs, int n_segs, double prev, double cur, int n_values,
                    int exp_floor, uint8_t* codes, void* state, void* scratch, size_t scratch_bytes, void* stream) {
  if (!w || !mask || !segs || !state || !scratch) return arg_refusal("tf2_inq_step", "null pointer");
  if (n_segs < 1) return arg_refusal("tf2_inq_step", "n_segs must be >= 1");
  if (n_total < 1 || n_total > (1ll << 42)) return arg_refusal("tf2_inq_step", "n_total outside 1 .. 2^42");
  long long at = 0;
  for (int i = 0; i < n_segs; i++) {
    const long long o = segs[i].offset, c = segs[i].count;
    if (c < 1 || c > 0x7fffffffll || o < at || o > n_total - c) {
      set_error("tf2_inq_step: segment " + std::to_string(i) + " (offset " + std::to_string(o) + ", count " + std::to_string(c) +
                "): the table must ascend without overlap inside n_total, counts in 1 .. 2^31 - 1");
      return TF2_ERR_ARG;
    }
    at = o + c;
  }
  if (!(prev >= 0.0 && prev < 1.0)) return arg_refusal("tf2_inq_step", "prev must be in [0, 1)");
  if (!(cur >= prev && cur <= 1.0)) return arg_refusal("tf2_inq_step", "cur must be in [prev, 1]");
  if (n_values < 1 || n_values > 15) return arg_refusal("tf2_inq_step", "n_values must be in 1 .. 15");
  if (exp_floor < -150 || exp_floor > 127) return arg_refusal("tf2_inq_step", "exp_floor must be in -150 .. 127");
  if (((uintptr_t)state & 7) || ((uintptr_t)scratch & 7)) return arg_refusal("tf2_inq_step", "state and scratch must be 8-byte aligned");
  if (scratch_bytes < inq_scratch_size(n_segs)) {
    set_error("tf2_inq_step: scratch too small (tf2_inq_scratch_size: " + std::to_string(inq_scratch_size(n_segs)) + ")");
    return TF2_ERR_SIZE;
  }
  // every launch's table and grid, before anything is enqueued
  uint32_t* const hist = (uint32_t*)scratch;
  InqSel* const sel = (InqSel*)((char*)scratch + (size_t)n_segs * kInqPasses * kInqBins * sizeof(uint32_t));
  const int vec = (((uintptr_t)w & 15) == 0 && ((uintptr_t)mask & 3) == 0 && (!codes || ((uintptr_t)codes & 3) == 0)) ? 1 : 0;
  std::vector<InqArgs> launches;
  std::vector<unsigned> blocks;
  for (int s0 = 0; s0 < n_segs; s0 += kInqSegsPerLaunch) {
    InqArgs A{};
    A.n_segs = std::min(kInqSegsPerLaunch, n_segs - s0);
    for (int i = 0; i < A.n_segs; i++) { A.off[i] = segs[s0 + i].offset; A.end[i] = segs[s0 + i].offset + segs[s0 + i].count; }
    A.w = w; A.mask = mask; A.codes = codes;
    A.state = (long long*)state + (long long)s0 * kInqWords;
    A.hist = hist + (long long)s0 * kInqPasses * kInqBins;
    A.sel = sel + s0;
    A.first = A.off[0] / kInqChunk * kInqChunk;
    A.vec = vec; A.exp_floor = exp_floor;
    launches.push_back(A);
    blocks.push_back((unsigned)((A.end[A.n_segs - 1] - A.first + kInqChunk - 1) / kInqChunk));   // (n_total <= 2^42: under 2^30 blocks)
  }
  hipStream_t st = (hipStream_t)stream;
  const long long state_words = (long long)n_segs * kInqWords, scratch_words = (long long)(inq_scratch_size(n_segs) / 8);
  hipLaunchKernelGGL(inq_init_kernel, dim3((unsigned)((state_words + scratch_words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     (unsigned long long*)state, state_words, (unsigned long long*)scratch, scratch_words);
  if (!launched("init")) return TF2_ERR_HIP;
  for (size_t i = 0; i < launches.size(); i++) {
    hipLaunchKernelGGL(inq_range_kernel, dim3(blocks[i]), dim3(kThreads), 0, st, launches[i]);
    if (!launched("range")) return TF2_ERR_HIP;
  }
  InqPlanArgs P{};
  P.state = (long long*)state; P.sel = sel; P.n_segs = n_segs; P.n_values = n_values; P.prev = prev; P.cur = cur;
  hipLaunchKernelGGL(inq_plan_kernel, dim3((unsigned)((n_segs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, P);
  if (!launched("plan")) return TF2_ERR_HIP;
  static const int kShift[kInqPasses + 1] = {31, 23, 15, 7, 0};
  for (int pass = 0; pass < kInqPasses; pass++) {
    for (size_t i = 0; i < launches.size(); i++) {
      InqArgs A = launches[i];
      A.pass = pass; A.hi_shift = kShift[pass]; A.shift = kShift[pass + 1];
      hipLaunchKernelGGL(inq_hist_kernel, dim3(blocks[i]), dim3(kThreads), 0, st, A);
      if (!launched("select")) return TF2_ERR_HIP;
    }
    hipLaunchKernelGGL(inq_resolve_kernel, dim3((unsigned)n_segs), dim3(kInqBins), 0, st, (const uint32_t*)hist, sel, (long long*)state, pass,
                       kShift[pass + 1]);
    if (!launched("resolve")) return TF2_ERR_HIP;
  }
  for (size_t i = 0; i < launches.size(); i++) {
    hipLaunchKernelGGL(inq_shape_kernel, dim3(blocks[i]), dim3(kThreads), 0, st, launches[i]);
    if (!launched("shape")) return TF2_ERR_HIP;
  }
  return TF2_OK;
}

}  // namespace tf2
