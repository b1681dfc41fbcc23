// embed_roc.hip -- match-threshold calibration on the device (tf2_emb_roc_*, include/tf2_amd.h): the genuine and impostor distance
// histograms of all pairs of a labelled set of float32 rows [N][D] (or of two sets), and of a caller's listed pairs, over the
// threshold grid thr[t] = (float)(t + 1) * step, t < n_thr.  tf2_amd/embed.py states it (roc_thresholds, reference_roc_hist,
// reference_pairs); every count and every distance is bit-identical to it.
//
// A distance is tf2_emb_match's, bit for bit: the sum over c ascending from +0 of separately rounded (a[c] - b[c])^2 (__fsub_rn /
// __fmul_rn / __fadd_rn; the library is built with -ffp-contract=off as well), no matrix or dot instruction; a NaN distance counts as
// +inf.  bin(d) = #{t : thr[t] <= d} in 0..n_thr by binary search; thr[t] is the one float32 multiply, evaluated at every probe (two
// vector operations, against an LDS read with a different address in every lane): the table is never stored.  The distance matrix is
// never written either.  Counts are integers added with atomics: the result is exact and does not depend on the grid, the tile or
// the order of the blocks.
//
// roc_hist_kernel   A block owns one pair of tiles of kRocTile = 256 rows, (ti, tj); self mode launches the pairs ti <= tj alone
//                   (blockIdx.x is the triangular index) and counts i < j.  The block walks the tile pair's 4 x 4 sub-tile pairs of
//                   64 x 64 rows (those of a diagonal tile that hold no i < j, and those past the rows, are skipped), each in
//                   match_slab_kernel's shape: the two sub-tiles are staged through LDS in chunks of 32 columns, A as rows (stride
//                   36 words: a lane's 16-byte reads of its own row are conflict-free), B transposed (bT[c][row]: a lane stages one
//                   row, so the stores of a wave fall on consecutive words); lane l of every wave owns row l of A and wave w the
//                   rows 16 w .. 16 w + 15 of B: sixteen accumulators a lane, the B values four 16-byte LDS reads at one address
//                   for the whole wave (a broadcast).  A finished distance is binned and counted with one LDS atomic into the block's
//                   histogram of 2 x (n_thr + 1) uint32 (dynamic LDS; a block counts at most 65 536 pairs); the non-zero bins leave
//                   with one 64-bit atomicAdd each when the block is done.
//                   LDS: 9 216 (A) + 8 192 (B) static + 8 (n_thr + 1) dynamic bytes (20.6 KiB at n_thr = 400, 49.4 KiB at 4096);
//                   VGPRs and scratch: see the table at the end of this comment.
// roc_pairs_kernel  one wave a listed pair (a, b, same, fold).  The pair is validated before any row is read; the lanes write the
//                   squares (a[c] - b[c])^2 into LDS, every lane adds them in order (broadcast reads), lane 0 stores the distance
//                   (-1.0f for an invalid pair), and adds 1 to hist[fold][same][bin] or to the invalid counter: 64-bit atomics.
//
//   kernel             VGPRs  SGPRs  scratch  static LDS
//   roc_hist_kernel    116    102    0        17 408
//   roc_pairs_kernel   44     28     0        8 192
// Measured on an MI355X at D = 128, n_thr = 400 (tools/embed_roc_time.py, profiles/embed_roc_time.json): all pairs of 13 233 rows
// 1.09 ms, of 100 000 rows 43.7 ms -- 0.0125 and 0.0087 ns a distance, 0.75 and 0.53 of match_slab_kernel's 0.0166 (batch 32,
// 100 000 rows, the same process).
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "embed_roc.h"

namespace tf2 {

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kBw = kRocSub / kWaves;              // B rows a wave owns: accumulators a lane
constexpr int kChunk = 32;                         // columns staged at a time
constexpr int kStride = kChunk + 4;                // A's LDS row stride in words: 16-byte aligned rows, 9 t mod 16 is a bijection
constexpr int kSubs = kRocTile / kRocSub;          // sub-tiles a tile side
static_assert(kRocSub == 64 && kBw == 16 && kRocTile % kRocSub == 0, "one A row a lane, four float4 of B a wave");

struct HistArgs {
  const float* a;                    // [n_a][d]
  const int32_t* ida;                // [n_a]
  const float* b;                    // [n_b][d] (self mode: a)
  const int32_t* idb;                // [n_b]    (self mode: ida)
  unsigned long long* hist;          // [2][n_thr + 1], accumulated
  float step;
  int32_t n_a, n_b, d, n_thr, self, vec4, tiles_a;
};

// #{t : thr[t] <= dist}, thr[t] = (float)(t + 1) * step: non-decreasing in t (a rounded product by one positive factor is monotone)
__device__ __forceinline__ int bin_of(float dist, int n_thr, float step) {
  int lo = 0, hi = n_thr;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (__fmul_rn((float)(mid + 1), step) <= dist) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one column: the lane's A value against the wave's kBw B values (one address for the whole wave)
__device__ __forceinline__ void column(float (&acc)[kBw], const float* __restrict__ bq, float a) {
#pragma unroll
  for (int v = 0; v < kBw / 4; v++) {
    const float4 b = *reinterpret_cast<const float4*>(bq + 4 * v);
    float t;
    t = __fsub_rn(a, b.x); acc[4 * v + 0] = __fadd_rn(acc[4 * v + 0], __fmul_rn(t, t));
    t = __fsub_rn(a, b.y); acc[4 * v + 1] = __fadd_rn(acc[4 * v + 1], __fmul_rn(t, t));
    t = __fsub_rn(a, b.z); acc[4 * v + 2] = __fadd_rn(acc[4 * v + 2], __fmul_rn(t, t));
    t = __fsub_rn(a, b.w); acc[4 * v + 3] = __fadd_rn(acc[4 * v + 3], __fmul_rn(t, t));
  }
}

__global__ __launch_bounds__(kThreads) void roc_hist_kernel(HistArgs p) {
  extern __shared__ uint32_t hist[];                                // [2][n_thr + 1]
  __shared__ __attribute__((aligned(16))) float as[kRocSub * kStride];
  __shared__ __attribute__((aligned(16))) float bt[kChunk * kRocSub];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bins = p.n_thr + 1;

  long long ti, tj;
  if (p.self) {                                                     // blockIdx.x = tj (tj + 1) / 2 + ti, ti <= tj
    const long long q = blockIdx.x;
    tj = (long long)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while (tj * (tj + 1) / 2 > q) tj--;
    while ((tj + 1) * (tj + 2) / 2 <= q) tj++;
    ti = q - tj * (tj + 1) / 2;
  } else {
    tj = blockIdx.x / p.tiles_a;
    ti = blockIdx.x - tj * p.tiles_a;
  }

  for (int i = threadIdx.x; i < 2 * bins; i += kThreads) hist[i] = 0;
  __syncthreads();

  const int d = p.d;
  for (int si = 0; si < kSubs; si++) {
    const long long a0 = ti * kRocTile + si * kRocSub;
    if (a0 >= p.n_a) break;
    const int arows = p.n_a - a0 < kRocSub ? (int)(p.n_a - a0) : kRocSub;
    const long long ai = a0 + lane;                                 // the lane's A row
    const int ida = lane < arows ? p.ida[ai] : -1;
    for (int sj = 0; sj < kSubs; sj++) {
      const long long b0 = tj * kRocTile + sj * kRocSub;
      if (b0 >= p.n_b) break;
      if (p.self && b0 + kRocSub - 1 <= a0) continue;               // no i < j in this sub-tile pair (block-uniform)
      const int brows = p.n_b - b0 < kRocSub ? (int)(p.n_b - b0) : kRocSub;

      float acc[kBw];
#pragma unroll
      for (int j = 0; j < kBw; j++) acc[j] = 0.0f;

      for (int c0 = 0; c0 < d; c0 += kChunk) {
        const int ck = d - c0 < kChunk ? d - c0 : kChunk;
        __syncthreads();                                            // the previous chunk has been read
        if (p.vec4) {                                               // d % 4 == 0 and 16-byte aligned rows: ck % 4 == 0
          const int per = ck >> 2;                                  // float4 a row
          for (int i = threadIdx.x; i < kRocSub * per; i += kThreads) {
            const int r = i / per, v = i - r * per;
            float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r < arows) x = *reinterpret_cast<const float4*>(p.a + (a0 + r) * d + c0 + 4 * v);
            *reinterpret_cast<float4*>(as + r * kStride + 4 * v) = x;
            const int rb = i & (kRocSub - 1), vb = i >> 6;          // B: a lane a row
            float4 y = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (rb < brows) y = *reinterpret_cast<const float4*>(p.b + (b0 + rb) * d + c0 + 4 * vb);
            float* const o = bt + 4 * vb * kRocSub + rb;
            o[0] = y.x; o[kRocSub] = y.y; o[2 * kRocSub] = y.z; o[3 * kRocSub] = y.w;
          }
        } else {
          for (int i = threadIdx.x; i < kRocSub * ck; i += kThreads) {
            const int r = i / ck, c = i - r * ck;
            as[r * kStride + c] = r < arows ? p.a[(a0 + r) * d + c0 + c] : 0.0f;
            const int rb = i & (kRocSub - 1), cb = i >> 6;
            bt[cb * kRocSub + rb] = rb < brows ? p.b[(b0 + rb) * d + c0 + cb] : 0.0f;
          }
        }
        __syncthreads();
        const float* const mine = as + lane * kStride;
        const float* bq = bt + kBw * wave;
        int c = 0;
        for (; c + 4 <= ck; c += 4) {
          const float4 g = *reinterpret_cast<const float4*>(mine + c);
          column(acc, bq, g.x); bq += kRocSub;
          column(acc, bq, g.y); bq += kRocSub;
          column(acc, bq, g.z); bq += kRocSub;
          column(acc, bq, g.w); bq += kRocSub;
        }
        for (; c < ck; c++) {
          column(acc, bq, mine[c]); bq += kRocSub;
        }
      }

#pragma unroll
      for (int j = 0; j < kBw; j++) {
        const int jb = kBw * wave + j;                              // (wave-uniform)
        if (jb < brows) {
          const long long bj = b0 + jb;
          const int idb = p.idb[bj];
          if (ida >= 0 && idb >= 0 && (!p.self || ai < bj)) {       // (ida < 0 as well for the lanes past A's rows)
            float dist = acc[j];
            if (dist != dist) dist = __uint_as_float(0x7f800000u);
            atomicAdd(hist + (ida == idb ? bins : 0) + bin_of(dist, p.n_thr, p.step), 1u);
          }
        }
      }
    }
  }

  __syncthreads();
  for (int i = threadIdx.x; i < 2 * bins; i += kThreads) {
    const uint32_t v = hist[i];
    if (v) atomicAdd(p.hist + i, (unsigned long long)v);
  }
}

struct PairArgs {
  const float* rows;                 // [n_rows][d]
  const int32_t* pairs;              // [n_pairs][4]: a, b, same, fold
  float* dist;                       // [n_pairs]
  unsigned long long* hist;          // [n_folds][2][n_thr + 1], accumulated
  unsigned long long* invalid;       // [1], accumulated
  float step;
  int32_t n_rows, d, n_pairs, n_folds, n_thr;
};

__global__ __launch_bounds__(kThreads) void roc_pairs_kernel(PairArgs p) {
  __shared__ float sq[kWaves][kEmbMaxD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pi = blockIdx.x * kWaves + wave;
  const bool live = pi < p.n_pairs;                                 // (wave-uniform)
  int a = -1, b = -1, same = -1, fold = -1;
  if (live) {
    const int32_t* const q = p.pairs + 4ll * pi;
    a = q[0]; b = q[1]; same = q[2]; fold = q[3];
  }
  const bool valid = a >= 0 && a < p.n_rows && b >= 0 && b < p.n_rows && (same == 0 || same == 1) && fold >= 0 && fold < p.n_folds;
  float* const s = sq[wave];
  if (valid) {
    const float* const ra = p.rows + (long long)a * p.d;
    const float* const rb = p.rows + (long long)b * p.d;
    for (int c = lane; c < p.d; c += 64) {
      const float t = __fsub_rn(ra[c], rb[c]);
      s[c] = __fmul_rn(t, t);
    }
  }
  __syncthreads();
  if (!live) return;
  if (!valid) {
    if (lane == 0) {
      p.dist[pi] = -1.0f;
      atomicAdd(p.invalid, 1ull);
    }
    return;
  }
  float dist = 0.0f;
  for (int c = 0; c < p.d; c++) dist = __fadd_rn(dist, s[c]);
  if (dist != dist) dist = __uint_as_float(0x7f800000u);
  if (lane == 0) {
    p.dist[pi] = dist;
    atomicAdd(p.hist + ((long long)fold * 2 + same) * (p.n_thr + 1) + bin_of(dist, p.n_thr, p.step), 1ull);
  }
}

// the checks the two calls share; the message names the call
tf2_status check_grid(const char* who, int d, int n_thr, float step) {
  auto fail = [&](const std::string& m) { set_error(std::string(who) + ": " + m); return TF2_ERR_ARG; };
  if (d < 2 || d > kEmbMaxD) return fail("d must be in 2.." + std::to_string(kEmbMaxD));
  if (n_thr < 1 || n_thr > kRocMaxThr) return fail("n_thr must be in 1.." + std::to_string(kRocMaxThr));
  if (!std::isfinite(step) || !(step > 0.0f)) return fail("step must be finite and > 0");
  return TF2_OK;
}

}  // namespace

tf2_status emb_roc_hist(const float* rows_a, const int32_t* ids_a, int n_a, const float* rows_b, const int32_t* ids_b, int n_b, int d,
                        int n_thr, float step, int64_t* hist, void* stream) {
  auto fail = [](const std::string& m) { return arg_refusal("tf2_emb_roc_hist", m); };
  const tf2_status st = check_grid("tf2_emb_roc_hist", d, n_thr, step);
  if (st != TF2_OK) return st;
  if (n_a < 1) return fail("n_a must be >= 1");
  if (rows_b && n_b < 1) return fail("n_b must be >= 1");
  if (!rows_a || !ids_a) return fail("null rows_a_dev / ids_a_dev");
  if (rows_b && !ids_b) return fail("null ids_b_dev (rows_b_dev is given: cross mode)");
  if (!hist) return fail("null hist_dev");
  HistArgs p{};
  p.self = rows_b ? 0 : 1;
  p.a = rows_a; p.ida = ids_a; p.n_a = n_a;
  p.b = p.self ? rows_a : rows_b; p.idb = p.self ? ids_a : ids_b; p.n_b = p.self ? n_a : n_b;
  p.hist = reinterpret_cast<unsigned long long*>(hist);
  p.step = step; p.d = d; p.n_thr = n_thr;
  p.vec4 = (d % 4 == 0 && ((uintptr_t)p.a & 15) == 0 && ((uintptr_t)p.b & 15) == 0) ? 1 : 0;
  const long long ta = ((long long)p.n_a + kRocTile - 1) / kRocTile, tb = ((long long)p.n_b + kRocTile - 1) / kRocTile;
  p.tiles_a = (int32_t)ta;
  const long long blocks = p.self ? ta * (ta + 1) / 2 : ta * tb;
  if (blocks > 0x7fffffffll) { set_error("tf2_emb_roc_hist: too many tile pairs for one grid"); return TF2_ERR_UNSUPPORTED; }
  hipLaunchKernelGGL(roc_hist_kernel, dim3((unsigned)blocks), dim3(kThreads), (size_t)2 * (n_thr + 1) * sizeof(uint32_t), (hipStream_t)stream, p);
  return launch_result("tf2_emb_roc_hist");
}

tf2_status emb_roc_pairs(const float* rows, int n_rows, int d, const int32_t* pairs, int n_pairs, int n_folds, int n_thr, float step,
                         float* dist, int64_t* hist, int64_t* invalid, void* stream) {
  auto fail = [](const std::string& m) { return arg_refusal("tf2_emb_roc_pairs", m); };
  const tf2_status st = check_grid("tf2_emb_roc_pairs", d, n_thr, step);
  if (st != TF2_OK) return st;
  if (n_rows < 1) return fail("n_rows must be >= 1");
  if (n_pairs < 1) return fail("n_pairs must be >= 1");
  if (n_folds < 1 || n_folds > kRocMaxFolds) return fail("n_folds must be in 1.." + std::to_string(kRocMaxFolds));
  if (!rows || !pairs) return fail("null rows_dev / pairs_dev");
  if (!dist || !hist || !invalid) return fail("null dist_dev / hist_dev / invalid_dev");
  PairArgs p{};
  p.rows = rows; p.pairs = pairs; p.dist = dist;
  p.hist = reinterpret_cast<unsigned long long*>(hist);
  p.invalid = reinterpret_cast<unsigned long long*>(invalid);
  p.step = step; p.n_rows = n_rows; p.d = d; p.n_pairs = n_pairs; p.n_folds = n_folds; p.n_thr = n_thr;
  hipLaunchKernelGGL(roc_pairs_kernel, dim3((unsigned)(((long long)n_pairs + kWaves - 1) / kWaves)), dim3(kThreads), 0, (hipStream_t)stream, p);
  return launch_result("tf2_emb_roc_pairs");
}

}  // namespace tf2
