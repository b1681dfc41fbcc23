// classify.hip -- the classification head on the device (tf2_cls_*, include/tf2_amd.h): int8 logits [batch][n] -> top-k labels and
// features with the tie rule of Evaluation() (network_helper.cpp:143-207), max-subtracted float32 softmax probabilities, the rank of a
// ground-truth label and accumulated top-1 / top-k tallies.  tf2_amd/classify.py restates the arithmetic (classify.reference); labels,
// features, ranks and tallies are bit-identical to it, and labels and features to tf2_topk.
//
// One wave per image, four images a block.  The wave reads the image's logits once (bytes, lane-consecutive), dequantises them
// (logit * 2^-sh: exact, the same value as the reference's logit / (1 << sh)) and keeps each feature as an ORDERABLE 32-bit word in
// LDS: unsigned order of the words == float order of the features.  Entry i belongs to lane i % 64 alone, so the LDS is indexed
// private storage and the wave needs no barrier.  A 64-bit key (word << 32 | i) is unique per entry and orders by (feature
// descending, index descending) -- the closed form of the reference's k bubble passes with a strict '>'.  Round r takes the largest
// key strictly below round r-1's winner: a lane-local scan, then a 64-lane butterfly maximum; nothing is mutated, and lane r keeps
// winner r, so the results leave with one coalesced store per output.  The softmax maximum is round 0's winner; the sum is 64 strided
// partial sums (ascending i) and a 6-step butterfly, a fixed order: ceil(n / 64) + 6 additions on the longest path, and the same
// bits every run.  A block adds its (at most four) images' counts with one 64-bit atomicAdd per nonzero counter.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include <vector>
#include "tf2_device.h"
#include "tf2_net.h"
#include "classify.h"

namespace tf2 {

namespace {

constexpr int kClsWaves = 4;                       // images per block
constexpr int kClsThreads = 64 * kClsWaves;
constexpr int kClsLoads = 8;                       // logit bytes a lane has in flight

// float -> word whose unsigned order is the float order (no NaN, no -0 here: the features are int8 * 2^-sh), and back
__device__ __forceinline__ uint32_t ord_of(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float feature_of(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o > v ? o : v;
  }
  return v;
}

// the same bits in every lane: each step adds the two halves of a pair, and a + b == b + a
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(kClsThreads) void classify_kernel(ClassifyArgs a) {
  extern __shared__ uint32_t lds[];                // [kClsWaves][n]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kClsWaves + wave;
  const int n = a.n, k = a.top_k;
  uint32_t* const keys = lds + wave * n;
  uint32_t flags = 0;                              // bit 0 labelled, 1 rank == 0, 2 rank >= 0, 3 bad label

  if (b < a.batch) {                               // (wave-uniform)
    const int8_t* const lg = a.logits + (long long)b * n;
    for (int base = 0; base < n; base += 64 * kClsLoads) {
      int v[kClsLoads];
      float s[kClsLoads];
#pragma unroll
      for (int u = 0; u < kClsLoads; u++) {
        const int i = base + u * 64 + lane;
        v[u] = i < n ? (int)lg[i] : 0;
        s[u] = i < n ? a.scale[i] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kClsLoads; u++) {
        const int i = base + u * 64 + lane;
        if (i < n) keys[i] = ord_of((float)v[u] * s[u]);
      }
    }

    unsigned long long prev = ~0ull, mine = 0, first = 0;
    for (int r = 0; r < k; r++) {
      unsigned long long best = 0;                 // below every key: a key's word is never 0
      for (int i = lane; i < n; i += 64) {
        const unsigned long long key = (unsigned long long)keys[i] << 32 | (uint32_t)i;
        if (key < prev && key > best) best = key;
      }
      prev = wave_max(best);                       // exists: r < k <= n
      if (r == 0) first = prev;
      if (lane == r) mine = prev;
    }
    const int label = (int)(uint32_t)mine;
    const float feat = feature_of((uint32_t)(mine >> 32));
    const long long ok = (long long)b * k + lane;
    if (lane < k) {
      a.labels[ok] = label;
      if (a.features) a.features[ok] = feat;
    }

    if (a.probs || a.all_probs) {
      const float fmax = feature_of((uint32_t)(first >> 32));
      float sum = 0.0f;
      for (int i = lane; i < n; i += 64) {
        const float e = expf(feature_of(keys[i]) - fmax);
        sum += e;
        keys[i] = __float_as_uint(e);              // the selection is over: the entry now holds its exponential
      }
      sum = wave_sum(sum);
      if (a.probs && lane < k) a.probs[ok] = expf(feat - fmax) / sum;
      if (a.all_probs) {
        float* const ap = a.all_probs + (long long)b * n;
        for (int i = lane; i < n; i += 64) ap[i] = __uint_as_float(keys[i]) / sum;
      }
    }

    const int t = a.truth ? a.truth[b] : -1;
    int rk = -1;
    if (t >= 0 && t < n) {
      const unsigned long long hit = __ballot(lane < k && label == t);
      rk = hit ? __ffsll(hit) - 1 : -1;
    }
    if (a.rank && lane == 0) a.rank[b] = rk;
    flags = (t >= 0 ? 1u : 0u) | (rk == 0 ? 2u : 0u) | (rk >= 0 ? 4u : 0u) | (t >= n ? 8u : 0u);
  }

  if (a.tally) {                                   // (uniform over the grid)
    __syncthreads();                               // every wave is done with its entries: words 0..3 now carry the waves' flags
    if (lane == 0) lds[wave] = flags;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        unsigned long long add = 0;
#pragma unroll
        for (int w = 0; w < kClsWaves; w++) add += (lds[w] >> c) & 1u;
        if (add) atomicAdd(a.tally + c, add);
      }
    }
  }
}

}  // namespace

Classifier::~Classifier() {
  if (consts) (void)hipFree(consts);
}

tf2_status Classifier::create(const Net* net, const tf2_cls_desc* d) {
  auto fail = [](const std::string& m) { return arg_refusal("tf2_cls_create", m); };
  if (!d || d->size != sizeof(tf2_cls_desc)) return fail("desc size: missing, or not sizeof(tf2_cls_desc)");
  if (net->q.empty()) { set_error("tf2_cls_create: q table not set (tf2_net_set_q first)"); return TF2_ERR_STATE; }
  const tf2_layer_desc& LL = net->layers[net->nd.n_layers - 1];
  if (net->logits_bytes(1) != (size_t)LL.N) return fail("the net's final map is not 1 x 1: its output is not one row of logits an image");
  for (int l = 0; l + 1 < net->nd.n_layers; l++)
    if (net->is_sink(l)) return fail("row " + std::to_string(l) + " is a network output as well: the final map is not one 1 x 1 row of logits (a detection net: tf2_ssd_*)");
  if (net->nd.n_layers >= net->nd.n_q_rows || LL.N > net->nd.max_out_channel) return fail("the q table has no row for the last layer's output");
  if (LL.N < 2 || LL.N > kClsMaxN) {
    set_error("tf2_cls_create: " + std::to_string(LL.N) + " classes; the kernel takes 2.." + std::to_string(kClsMaxN));
    return TF2_ERR_UNSUPPORTED;
  }
  const int kmax = LL.N < kClsMaxTopK ? LL.N : kClsMaxTopK;
  if (d->top_k < 1 || d->top_k > kmax) return fail("top_k must be in 1.." + std::to_string(kmax) + " (min(classes, " + std::to_string(kClsMaxTopK) + "))");
  // the row tf2_topk's callers pass: q[NUM_LAYER] (main.cpp:53), runtime values = -Q
  const int8_t* const qr = net->q.data() + (size_t)net->nd.n_layers * net->nd.max_out_channel;
  std::vector<float> scale(LL.N);
  for (int i = 0; i < LL.N; i++) {
    const int sh = -(int)qr[i];
    if (sh < 0 || sh > 30) return fail("Q of the last layer must be in 0..30 (network_helper.cpp:181); channel " + std::to_string(i) + " has " + std::to_string(sh));
    scale[i] = std::ldexp(1.0f, -sh);
  }
  n = LL.N; top_k = d->top_k;
  hipError_t e = hipMalloc(&consts, (size_t)n * 4);
  if (e == hipSuccess) e = hipMemcpy(consts, scale.data(), (size_t)n * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { set_error(std::string("tf2_cls_create: ") + hipGetErrorString(e)); return TF2_ERR_HIP; }
  return TF2_OK;
}

tf2_status Classifier::run(const int8_t* logits, int batch, int32_t* labels, float* features, float* probs, float* all_probs,
                           const int32_t* truth, int32_t* rank, uint64_t* tally, void* stream) {
  // (batch >= 1 and the two required pointers: checked by tf2_cls_run before it looks at the handle)
  ClassifyArgs a{};
  a.logits = logits; a.scale = (const float*)consts; a.labels = labels; a.features = features; a.probs = probs; a.all_probs = all_probs;
  a.truth = truth; a.rank = rank; a.tally = reinterpret_cast<unsigned long long*>(tally);
  a.n = n; a.top_k = top_k; a.batch = batch;
  const dim3 grid((unsigned)((batch + kClsWaves - 1) / kClsWaves)), block(kClsThreads);
  hipLaunchKernelGGL(classify_kernel, grid, block, (size_t)kClsWaves * n * sizeof(uint32_t), (hipStream_t)stream, a);
  return launch_result("tf2_cls_run");
}

}  // namespace tf2
