// weight_dnscp.hip -- DNS channel pruning on the device (tf2_dnscp_*, include/tf2_amd.h): per INPUT channel of every conv [N][C][k][k]
// of one flat float32 buffer a keep byte, decided by the reference's rule (TransForm_Kit/DnsChannelpruning/dnscp_core.py: cal_mean_std,
// maskChannelCalc) stated on float bit patterns with exact integer sums; tf2_amd/dnscp.py (reference_stats / reference_step) is that
// statement in numpy, and keep bytes, the masked stream, the channel sums S1 and every word of the record equal it as bits, whatever
// the grid and the order of the blocks: integer adds, maxima and plain stores only.
//
// A block owns kDnsChunk consecutive elements of the flat buffer and walks the convs that meet its chunk one after the other (as
// weight_inq.hip does with its segments), so elements in no conv are never touched.  A lane takes groups of four elements on 16-byte
// boundaries: one 16-byte load where the whole group lies inside the conv, element by element at an unaligned head and tail.  The
// channel of an element is ((i - offset) / kk) % C: one 32-bit division a group, then counted on.
//
// dns_init_kernel, dns_zero_sums_kernel   zero the records and the convs' S1 words, so that a replay on refilled weights equals a fresh call.
// dns_max_kernel      per conv the largest FINITE magnitude pattern and the non-finite count (shuffles, LDS atomics, one 64-bit atomic
//                     a block).  Its leading-bit exponent E fixes the conv's fixed point: m(a) = floor(a * 2^(31 - E)) < 2^32.
// dns_sum_kernel      reads every filter once: S1[c] += m in an LDS slot per channel (64-bit LDS adds, a lane first joins its own
//                     elements of one channel), one 64-bit atomic per touched channel and block; over the kept channels A1 = sum m,
//                     A2 = sum m^2 as (hi, lo) halves and nz in registers, reduced by shuffles, one atomic each a block.
// dns_decide_kernel   one block a conv, a thread 16 channels: B_lo / B_hi from the thresholds in double, the hysteresis compare on S1,
//                     a scan of the kept counts, the multiple-of-16 fix-up in ascending channel order, the keep bytes, the record.
// dns_apply_kernel    out = dense where the channel is kept, else +0.0; one read and one write of the stream.
// dns_compact_kernel  the export: dst[n'][c'][j] = src[n_idx[n']][c_idx[c']][j] for every tensor of the pruned stream.
//
//   kernel                VGPRs  scratch  static LDS
//   dns_init_kernel       4      0        0
//   dns_zero_sums_kernel  8      0        0
//   dns_max_kernel        22     0        8
//   dns_sum_kernel        54     0        36 896
//   dns_decide_kernel     28     0        1 036
//   dns_apply_kernel      63     0        4 096
//   dns_compact_kernel    14     0        0
// Measured on an MI355X, ResNet-50's 32 prunable convs (16.3 M weights, 7 552 channels; tools/dnscp_time.py, profiles/dnscp_time.json):
// a step with every conv updated takes 0.204 ms.
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <string>
#include <vector>
#include "act_rows.h"      // add64
#include "weight_dnscp.h"

namespace tf2 {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kMag = 0x7fffffffu;
constexpr uint32_t kInf = 0x7f800000u;
constexpr int kNoExp = -1000;            // "exponent" of zero
static_assert(kDnsChunk == kThreads * 16, "four 16-byte groups a lane");
static_assert(kDnsMaxC == kThreads * 16, "the decision: 16 channels a thread");

// exponent of the leading bit: floor(log2 a) (denormals from the leading-bit position)
__device__ __forceinline__ int exp2_of(uint32_t mag) {
  if (mag == 0) return kNoExp;
  const int E = (int)(mag >> 23);
  return E ? E - 127 : (31 - __clz(mag)) - 149;
}

// m(a) = floor(a * 2^(31 - E)) of a magnitude pattern under the conv's E (>= the pattern's own leading-bit exponent); 0 for zero and
// for a non-finite pattern
__device__ __forceinline__ uint32_t fixed_of(uint32_t mag, int E) {
  if (mag == 0 || mag >= kInf) return 0;
  const int e = (int)(mag >> 23);
  const uint32_t sig = e ? (mag & 0x7fffffu) | 0x800000u : mag;
  const int sh = (e ? e - 127 : -126) + 8 - E;                       // <= 8 for a normal, <= 31 - leading bit for a denormal
  return sh >= 0 ? sig << sh : (sh > -32 ? sig >> -sh : 0u);
}

struct Grp {
  uint32_t w[4];
  uint32_t valid;    // bit k: element k lies inside [a, b)
  bool full;
};

__device__ __forceinline__ void load_grp(Grp& g, const float* w, long long gb, long long a, long long b, bool vec) {
  g.full = vec && gb >= a && gb + 4 <= b;
  if (g.full) {
    const uint4 x = *reinterpret_cast<const uint4*>(w + gb);
    g.w[0] = x.x; g.w[1] = x.y; g.w[2] = x.z; g.w[3] = x.w;
    g.valid = 0xfu;
  } else {
    g.valid = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const long long i = gb + k;
      g.w[k] = 0;
      if (i >= a && i < b) { g.w[k] = __float_as_uint(w[i]); g.valid |= 1u << k; }
    }
  }
}

// channel and position inside the channel's kk run of element `rel` of a conv (rel < 2^28); next() steps one element on
struct Chan {
  uint32_t c, r, C, kk;
  __device__ __forceinline__ Chan(long long rel, int C_, int kk_) : C((uint32_t)C_), kk((uint32_t)kk_) {
    const uint32_t u = rel < 0 ? 0u : (uint32_t)rel;                 // (a group's elements before the conv are never valid)
    const uint32_t q = u / kk;
    r = u - q * kk;
    c = q % C;
  }
  __device__ __forceinline__ void next() {
    if (++r == kk) { r = 0; if (++c == C) c = 0; }
  }
};

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
__device__ __forceinline__ unsigned long long wave_add64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

__device__ __forceinline__ void max64(long long* p, unsigned long long v) {
  if (v) atomicMax(reinterpret_cast<unsigned long long*>(p), v);
}

__global__ __launch_bounds__(kThreads) void dns_init_kernel(unsigned long long* state, long long state_words) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < state_words) state[i] = 0;
}

__global__ __launch_bounds__(kThreads) void dns_zero_sums_kernel(DnsArgs p) {
  for (int s = 0; s < p.n_convs; s++)
    for (int c = (int)blockIdx.x * kThreads + (int)threadIdx.x; c < p.C[s]; c += (int)gridDim.x * kThreads) p.sums[p.keep_off[s] + c] = 0;
}

__global__ __launch_bounds__(kThreads) void dns_max_kernel(DnsArgs p) {
  __shared__ unsigned int red[2];                                    // max finite pattern, non-finite count
  const long long c0 = p.first + (long long)blockIdx.x * kDnsChunk, c1 = c0 + kDnsChunk;
  for (int s = 0; s < p.n_convs; s++) {
    const long long a = max(c0, p.off[s]), b = min(c1, p.end[s]);    // (block-uniform)
    if (a >= b) continue;
    if (threadIdx.x < 2) red[threadIdx.x] = 0;
    __syncthreads();
    uint32_t mx = 0, nf = 0;
    const long long g0 = a & ~3ll;
    const int ng = (int)((b - g0 + 3) >> 2);
    for (int g = threadIdx.x; g < ng; g += kThreads) {
      Grp G;
      load_grp(G, p.w, g0 + 4ll * g, a, b, p.vec != 0);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t mag = G.w[k] & kMag;                          // (an element outside [a, b) reads as 0)
        if (mag >= kInf) nf++;
        else mx = max(mx, mag);
      }
    }
    mx = wave_max(mx); nf = wave_add(nf);
    if ((threadIdx.x & 63) == 0) {
      if (mx) atomicMax(&red[0], mx);
      if (nf) atomicAdd(&red[1], nf);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long long* const R = p.state + (long long)s * kDnsWords;
      max64(R + kDnsMax, red[0]);
      add64(R + kDnsNonfinite, red[1]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void dns_sum_kernel(DnsArgs p) {
  __shared__ unsigned long long s1[kDnsMaxC];                        // the chunk's share of S1, a slot a channel
  __shared__ uint8_t kp[kDnsMaxC];
  __shared__ unsigned long long red[4];                              // A1, A2 hi, A2 lo, nz
  const long long c0 = p.first + (long long)blockIdx.x * kDnsChunk, c1 = c0 + kDnsChunk;
  for (int s = 0; s < p.n_convs; s++) {
    const long long a = max(c0, p.off[s]), b = min(c1, p.end[s]);
    if (a >= b) continue;
    long long* const R = p.state + (long long)s * kDnsWords;
    const int C = p.C[s], kk = p.kk[s];
    const int E = exp2_of((uint32_t)R[kDnsMax]);
    for (int c = threadIdx.x; c < C; c += kThreads) {
      s1[c] = 0;
      kp[c] = p.keep ? p.keep[p.keep_off[s] + c] : (uint8_t)1;
    }
    if (threadIdx.x < 4) red[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long a1 = 0, a2h = 0, a2l = 0;
    uint32_t nz = 0;
    const long long g0 = a & ~3ll;
    const int ng = (int)((b - g0 + 3) >> 2);
    for (int g = threadIdx.x; g < ng; g += kThreads) {
      Grp G;
      const long long gb = g0 + 4ll * g;
      load_grp(G, p.w, gb, a, b, p.vec != 0);
      Chan ch(gb - p.off[s], C, kk);
      uint32_t run_c = ch.c;                                         // the lane joins its elements of one channel before the LDS add
      unsigned long long run = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool valid = (G.valid >> k) & 1u;
        const uint32_t mag = G.w[k] & kMag;
        if (valid) {
          if (ch.c != run_c) {
            if (run) atomicAdd(&s1[run_c], run);
            run = 0; run_c = ch.c;
          }
          const unsigned long long m = fixed_of(mag, E);
          run += m;
          if (kp[ch.c]) {
            const unsigned long long sq = m * m;
            a1 += m; a2h += sq >> 32; a2l += sq & 0xffffffffull;
            nz += mag != 0 ? 1u : 0u;
          }
        }
        if (valid || gb + k >= p.off[s]) ch.next();                   // (elements before the conv's first do not count on)
      }
      if (run) atomicAdd(&s1[run_c], run);
    }
    a1 = wave_add64(a1); a2h = wave_add64(a2h); a2l = wave_add64(a2l); nz = wave_add(nz);
    if ((threadIdx.x & 63) == 0) {
      if (a1) atomicAdd(&red[0], a1);
      if (a2h) atomicAdd(&red[1], a2h);
      if (a2l) atomicAdd(&red[2], a2l);
      if (nz) atomicAdd(&red[3], (unsigned long long)nz);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kThreads) add64(p.sums + p.keep_off[s] + c, s1[c]);
    if (threadIdx.x == 0) {
      add64(R + kDnsA1, red[0]); add64(R + kDnsA2Hi, red[1]); add64(R + kDnsA2Lo, red[2]); add64(R + kDnsNz, red[3]);
    }
    __syncthreads();
  }
}

// floor(t * nkk * 2^k) clamped to [-1, 2^63 - 1]: one IEEE multiply, an exact scaling (k in -96 .. 180), a floor
__device__ __forceinline__ long long bound_of(double t, double nkk, int k) {
  double x = t * nkk;
  x = x * __longlong_as_double((long long)(k + 1023) << 52);
  x = floor(x);
  if (x >= 9223372036854775808.0) return LLONG_MAX;
  if (x < -1.0) return -1;
  return (long long)x;
}

__global__ __launch_bounds__(kThreads) void dns_decide_kernel(DnsDecideArgs p) {
  __shared__ int cnt[kThreads];
  __shared__ int tot[3];                                             // kept before, pruned by t_lo, revived by t_hi
  const int s = (int)blockIdx.x, t = (int)threadIdx.x;
  long long* const R = p.state + (long long)s * kDnsWords;
  const int C = p.C[s];
  uint8_t* const keep = p.keep ? p.keep + p.keep_off[s] : nullptr;
  const long long* const S1 = p.sums + p.keep_off[s];
  const bool update = (p.flags[s] & TF2_DNSCP_UPDATE) != 0;
  const uint32_t mx = (uint32_t)R[kDnsMax];
  const int E = exp2_of(mx);
  long long status = R[kDnsNonfinite] ? TF2_DNSCP_NONFINITE : (mx == 0 ? TF2_DNSCP_ALL_ZERO : 0);
  long long b_lo = 0, b_hi = 0;
  if (update) {
    const double t_lo = p.t_lo[s], t_hi = p.t_hi[s], nkk = (double)p.nkk[s];
    const int k = 31 - max(E, -149);
    b_lo = t_lo != t_lo ? -1 : bound_of(t_lo, nkk, k);
    b_hi = t_hi != t_hi ? LLONG_MAX : bound_of(t_hi, nkk, k);
    if (t_lo != t_lo || t_hi != t_hi) status |= TF2_DNSCP_NAN_THRESHOLD;
  }
  const bool decide = update && !(status & TF2_DNSCP_NONFINITE);
  uint32_t k0 = 0, k1 = 0;                                           // keep bits of channels 16 t .. 16 t + 15: before, behind the thresholds
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const int c = t * 16 + j;
    if (c < C) {
      const bool old = keep ? keep[c] != 0 : true;
      bool nw = old;
      if (decide) {
        const long long v = S1[c];
        if (old && v <= b_lo) nw = false;
        else if (!old && v > b_hi) nw = true;
      }
      k0 |= (old ? 1u : 0u) << j;
      k1 |= (nw ? 1u : 0u) << j;
    }
  }
  cnt[t] = __popc(k1);
  if (t < 3) tot[t] = 0;
  __syncthreads();
  if (k0) atomicAdd(&tot[0], __popc(k0));
  if (k0 & ~k1) atomicAdd(&tot[1], __popc(k0 & ~k1));
  if (~k0 & k1) atomicAdd(&tot[2], __popc(~k0 & k1));
  int below = 0, nzc = 0;
  for (int i = 0; i < kThreads; i++) { const int v = cnt[i]; below += i < t ? v : 0; nzc += v; }
  __syncthreads();
  uint32_t k2 = k1;
  int fix = 0;
  if (decide) {
    const int q = nzc >> 4, r = nzc & 15;
    int target = 16 * (q + (r > 8 || (r == 8 && (q & 1)) ? 1 : 0));  // round half to even
    if (target == 0) target = 16;
    if (target > nzc) {                                              // the first pruned channels by index come back
      const int need = target - nzc;
      int rank = min(t * 16, C) - below;
      fix = min(need, C - nzc);
#pragma unroll
      for (int j = 0; j < 16; j++)
        if (t * 16 + j < C && !((k1 >> j) & 1u)) { if (rank < need) k2 |= 1u << j; rank++; }
    } else if (target < nzc) {                                       // the first kept channels by index go
      const int need = nzc - target;
      int rank = below;
      fix = -need;
#pragma unroll
      for (int j = 0; j < 16; j++)
        if ((k1 >> j) & 1u) { if (rank < need) k2 &= ~(1u << j); rank++; }
    }
    if (keep) {
#pragma unroll
      for (int j = 0; j < 16; j++)
        if (t * 16 + j < C) keep[t * 16 + j] = (uint8_t)((k2 >> j) & 1u);
    }
  }
  if (t == 0) {
    R[kDnsN] = (long long)p.nkk[s] * C;
    R[kDnsE] = E;
    R[kDnsKeptBefore] = tot[0];
    R[kDnsPruned] = tot[1];
    R[kDnsRevived] = tot[2];
    R[kDnsFixup] = fix;
    R[kDnsKeptAfter] = decide ? nzc + fix : tot[0];
    R[kDnsStatus] = status;
    R[kDnsBLo] = b_lo;
    R[kDnsBHi] = b_hi;
  }
}

__global__ __launch_bounds__(kThreads) void dns_apply_kernel(DnsArgs p) {
  __shared__ uint8_t kp[kDnsMaxC];
  const long long c0 = p.first + (long long)blockIdx.x * kDnsChunk, c1 = c0 + kDnsChunk;
  for (int s = 0; s < p.n_convs; s++) {
    const long long a = max(c0, p.off[s]), b = min(c1, p.end[s]);
    if (a >= b) continue;
    if (p.state[(long long)s * kDnsWords + kDnsStatus] & TF2_DNSCP_NONFINITE) continue;   // (block-uniform) left as it was
    const int C = p.C[s], kk = p.kk[s];
    for (int c = threadIdx.x; c < C; c += kThreads) kp[c] = p.keep[p.keep_off[s] + c];
    __syncthreads();
    const long long g0 = a & ~3ll;
    const int ng = (int)((b - g0 + 3) >> 2);
    for (int g = threadIdx.x; g < ng; g += kThreads) {
      Grp G;
      const long long gb = g0 + 4ll * g;
      load_grp(G, p.w, gb, a, b, p.vec != 0);
      Chan ch(gb - p.off[s], C, kk);
      uint32_t cut = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool valid = (G.valid >> k) & 1u;
        if (valid && !kp[ch.c]) { G.w[k] = 0; cut |= 1u << k; }
        if (valid || gb + k >= p.off[s]) ch.next();
      }
      if (G.full) {
        if (cut || !p.inplace) *reinterpret_cast<uint4*>(p.out + gb) = make_uint4(G.w[0], G.w[1], G.w[2], G.w[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (((G.valid >> k) & 1u) && (((cut >> k) & 1u) || !p.inplace)) p.out[gb + k] = __uint_as_float(G.w[k]);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void dns_compact_kernel(DnsCompactArgs p) {
  int s = 0;
  while (s + 1 < p.n_segs && blockIdx.x >= p.block0[s + 1]) s++;     // (block-uniform; at most kDnsSegsPerLaunch steps)
  const uint32_t c_out = (uint32_t)p.c_out[s], kk = (uint32_t)p.kk[s], c_src = (uint32_t)p.c_src[s];
  const long long count = (long long)p.n_out[s] * c_out * kk;
  const long long base = (long long)(blockIdx.x - p.block0[s]) * kDnsCompactBlock;
#pragma unroll
  for (int u = 0; u < kDnsCompactBlock / kThreads; u++) {
    const long long i = base + u * kThreads + threadIdx.x;
    if (i >= count) break;
    const uint32_t row = (uint32_t)i / kk, j = (uint32_t)i - row * kk;                 // (count < 2^31)
    const uint32_t n1 = row / c_out, c1 = row - n1 * c_out;
    const int n = p.n_idx[s] < 0 ? (int)n1 : p.idx[p.n_idx[s] + n1];
    const int c = p.c_idx[s] < 0 ? (int)c1 : p.idx[p.c_idx[s] + c1];
    uint32_t v = 0x7fc00000u;                                        // an index outside the source tensor: NaN, never a read
    if (n >= 0 && n < p.n_src[s] && c >= 0 && (uint32_t)c < c_src)
      v = __float_as_uint(p.src[p.src_off[s] + ((long long)n * c_src + c) * kk + j]);
    p.dst[p.dst_off[s] + i] = __uint_as_float(v);
  }
}

bool launched(const char* fn, const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return true;
  set_error(std::string(fn) + ": " + what + " launch failed: " + hipGetErrorString(e));
  return false;
}

}  // namespace

tf2_status dnscp_run(const float* dense, float* out, long long n_total, const tf2_dnscp_conv* convs, int n_convs, uint8_t* keep,
                     long long n_channels, long long* sums, void* state, void* scratch, size_t scratch_bytes, void* stream, bool step) {
  const std::string fn = step ? "tf2_dnscp_step" : "tf2_dnscp_stats";
  (void)scratch; (void)scratch_bytes;                                // tf2_dnscp_scratch_size is 0: every intermediate lives in state and sums
  if (!dense || !convs || !sums || !state || (step && (!out || !keep))) { set_error(fn + ": null pointer"); return TF2_ERR_ARG; }
  if (n_convs < 1) { set_error(fn + ": n_convs must be >= 1"); return TF2_ERR_ARG; }
  if (n_total < 1 || n_total > (1ll << 42)) { set_error(fn + ": n_total outside 1 .. 2^42"); return TF2_ERR_ARG; }
  if (n_channels < 1) { set_error(fn + ": n_channels must be >= 1"); return TF2_ERR_ARG; }
  long long at = 0, kat = 0;
  for (int i = 0; i < n_convs; i++) {
    const tf2_dnscp_conv& c = convs[i];
    const std::string who = fn + ": conv " + std::to_string(i);
    if (c.N < 1 || c.C < 1 || c.kk < 1) { set_error(who + ": N, C and kk must be >= 1"); return TF2_ERR_ARG; }
    if (c.C > kDnsMaxC) { set_error(who + ": C = " + std::to_string(c.C) + " is above 4096"); return TF2_ERR_UNSUPPORTED; }
    if ((long long)c.N * c.kk >= (1ll << 22)) { set_error(who + ": N * kk must be under 2^22 (exact sums)"); return TF2_ERR_UNSUPPORTED; }
    const long long n = (long long)c.N * c.kk * c.C;
    if (n >= (1ll << 28)) { set_error(who + ": N * C * kk must be under 2^28 (exact sums)"); return TF2_ERR_UNSUPPORTED; }
    if (c.offset < at || c.offset > n_total - n) {
      set_error(who + " (offset " + std::to_string(c.offset) + ", " + std::to_string(n) + " elements): the table must ascend without overlap inside n_total");
      return TF2_ERR_ARG;
    }
    if (c.keep_offset < kat || c.keep_offset > n_channels - c.C) {
      set_error(who + " (keep_offset " + std::to_string(c.keep_offset) + "): keep ranges must ascend without overlap inside n_channels");
      return TF2_ERR_ARG;
    }
    if (c.flags & ~TF2_DNSCP_UPDATE) { set_error(who + ": unknown flags"); return TF2_ERR_ARG; }
    if (!step && (c.flags & TF2_DNSCP_UPDATE)) { set_error(who + ": TF2_DNSCP_UPDATE belongs to tf2_dnscp_step"); return TF2_ERR_ARG; }
    if ((c.flags & TF2_DNSCP_UPDATE) && (c.t_lo < 0.0 || c.t_hi < 0.0)) { set_error(who + ": thresholds must be >= 0 or NaN"); return TF2_ERR_ARG; }
    at = c.offset + n;
    kat = c.keep_offset + c.C;
  }
  if (((uintptr_t)state & 7) || ((uintptr_t)sums & 7)) { set_error(fn + ": state and sums must be 8-byte aligned"); return TF2_ERR_ARG; }
  if (step && out != dense && out < dense + n_total && dense < out + n_total) { set_error(fn + ": out_dev overlaps dense_dev without being equal to it"); return TF2_ERR_ARG; }
  // every launch's table and grid, before anything is enqueued
  const int vec = (((uintptr_t)dense & 15) == 0 && (!step || ((uintptr_t)out & 15) == 0)) ? 1 : 0;
  std::vector<DnsArgs> launches;
  std::vector<DnsDecideArgs> decides;
  std::vector<unsigned> blocks;
  for (int s0 = 0; s0 < n_convs; s0 += kDnsConvsPerLaunch) {
    DnsArgs A{};
    DnsDecideArgs D{};
    A.n_convs = std::min(kDnsConvsPerLaunch, n_convs - s0);
    for (int i = 0; i < A.n_convs; i++) {
      const tf2_dnscp_conv& c = convs[s0 + i];
      A.off[i] = c.offset; A.end[i] = c.offset + (long long)c.N * c.kk * c.C; A.keep_off[i] = c.keep_offset; A.C[i] = c.C; A.kk[i] = c.kk;
      D.keep_off[i] = c.keep_offset; D.t_lo[i] = c.t_lo; D.t_hi[i] = c.t_hi; D.C[i] = c.C; D.nkk[i] = c.N * c.kk; D.flags[i] = c.flags;
    }
    A.w = dense; A.out = out; A.keep = keep; A.sums = sums; A.vec = vec; A.inplace = out == dense ? 1 : 0;
    A.state = (long long*)state + (long long)s0 * kDnsWords;
    A.first = A.off[0] / kDnsChunk * kDnsChunk;
    D.keep = keep; D.sums = sums; D.state = A.state;
    launches.push_back(A);
    decides.push_back(D);
    blocks.push_back((unsigned)((A.end[A.n_convs - 1] - A.first + kDnsChunk - 1) / kDnsChunk));   // (n_total <= 2^42: under 2^30 blocks)
  }
  hipStream_t st = (hipStream_t)stream;
  const char* const f = fn.c_str();
  const long long state_words = (long long)n_convs * kDnsWords;
  hipLaunchKernelGGL(dns_init_kernel, dim3((unsigned)((state_words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (unsigned long long*)state,
                     state_words);
  if (!launched(f, "init")) return TF2_ERR_HIP;
  for (size_t i = 0; i < launches.size(); i++) {
    hipLaunchKernelGGL(dns_zero_sums_kernel, dim3(16), dim3(kThreads), 0, st, launches[i]);
    if (!launched(f, "init")) return TF2_ERR_HIP;
    hipLaunchKernelGGL(dns_max_kernel, dim3(blocks[i]), dim3(kThreads), 0, st, launches[i]);
    if (!launched(f, "max")) return TF2_ERR_HIP;
  }
  for (size_t i = 0; i < launches.size(); i++) {
    hipLaunchKernelGGL(dns_sum_kernel, dim3(blocks[i]), dim3(kThreads), 0, st, launches[i]);
    if (!launched(f, "sum")) return TF2_ERR_HIP;
    hipLaunchKernelGGL(dns_decide_kernel, dim3((unsigned)launches[i].n_convs), dim3(kThreads), 0, st, decides[i]);
    if (!launched(f, "decide")) return TF2_ERR_HIP;
  }
  if (step) {
    for (size_t i = 0; i < launches.size(); i++) {
      hipLaunchKernelGGL(dns_apply_kernel, dim3(blocks[i]), dim3(kThreads), 0, st, launches[i]);
      if (!launched(f, "apply")) return TF2_ERR_HIP;
    }
  }
  return TF2_OK;
}

tf2_status dnscp_compact(const float* src, long long n_src, float* dst, long long n_dst, const tf2_dnscp_seg* segs, int n_segs,
                         const int32_t* idx, long long n_idx, void* stream) {
  const std::string fn = "tf2_dnscp_compact";
  if (!src || !dst || !segs) { set_error(fn + ": null pointer"); return TF2_ERR_ARG; }
  if (n_segs < 1) { set_error(fn + ": n_segs must be >= 1"); return TF2_ERR_ARG; }
  if (n_src < 1 || n_dst < 1 || n_src > (1ll << 42) || n_dst > (1ll << 42) || n_idx < 0) { set_error(fn + ": n_src / n_dst outside 1 .. 2^42, or n_idx < 0"); return TF2_ERR_ARG; }
  if (dst < src + n_src && src < dst + n_dst) { set_error(fn + ": dst_dev overlaps src_dev"); return TF2_ERR_ARG; }
  long long at = 0;
  for (int i = 0; i < n_segs; i++) {
    const tf2_dnscp_seg& g = segs[i];
    const std::string who = fn + ": segment " + std::to_string(i);
    if (g.n_src < 1 || g.c_src < 1 || g.n_out < 1 || g.c_out < 1 || g.kk < 1) { set_error(who + ": sizes must be >= 1"); return TF2_ERR_ARG; }
    const long long ns = (long long)g.n_src * g.c_src * g.kk, nd = (long long)g.n_out * g.c_out * g.kk;
    if (ns > 0x7fffffffll || nd > 0x7fffffffll) { set_error(who + ": a tensor holds at most 2^31 - 1 elements"); return TF2_ERR_UNSUPPORTED; }
    if (g.src_offset < 0 || g.src_offset > n_src - ns) { set_error(who + ": the source tensor leaves src_dev"); return TF2_ERR_ARG; }
    if (g.dst_offset < at || g.dst_offset > n_dst - nd) { set_error(who + ": destination tensors must ascend without overlap inside n_dst"); return TF2_ERR_ARG; }
    if (g.n_idx < 0 ? g.n_out != g.n_src : (!idx || g.n_idx > n_idx - g.n_out)) { set_error(who + ": n_idx"); return TF2_ERR_ARG; }
    if (g.c_idx < 0 ? g.c_out != g.c_src : (!idx || g.c_idx > n_idx - g.c_out)) { set_error(who + ": c_idx"); return TF2_ERR_ARG; }
    at = g.dst_offset + nd;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int s0 = 0; s0 < n_segs; s0 += kDnsSegsPerLaunch) {
    DnsCompactArgs A{};
    A.n_segs = std::min(kDnsSegsPerLaunch, n_segs - s0);
    unsigned nb = 0;
    for (int i = 0; i < A.n_segs; i++) {
      const tf2_dnscp_seg& g = segs[s0 + i];
      A.src_off[i] = g.src_offset; A.dst_off[i] = g.dst_offset; A.n_idx[i] = g.n_idx; A.c_idx[i] = g.c_idx;
      A.n_src[i] = g.n_src; A.c_src[i] = g.c_src; A.n_out[i] = g.n_out; A.c_out[i] = g.c_out; A.kk[i] = g.kk;
      A.block0[i] = nb;
      nb += (unsigned)(((long long)g.n_out * g.c_out * g.kk + kDnsCompactBlock - 1) / kDnsCompactBlock);
    }
    A.block0[A.n_segs] = nb;
    A.src = src; A.dst = dst; A.idx = idx;
    hipLaunchKernelGGL(dns_compact_kernel, dim3(nb), dim3(kThreads), 0, st, A);
    if (!launched("tf2_dnscp_compact", "compact")) return TF2_ERR_HIP;
  }
  return TF2_OK;
}

}  // namespace tf2
