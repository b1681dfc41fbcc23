// embed_match.hip -- 1:N face matching on the device (tf2_emb_*, include/tf2_amd.h): the int8 outputs [batch][D] of an embedding
// network -> unit float32 embeddings, their squared Euclidean distances to a float32 gallery [N][D], the k nearest rows by (distance
// ascending, row index ascending) and accumulated accept / identify tallies.  tf2_amd/embed.py states the arithmetic (reference_embed,
// reference_match, reference_tally); every output is bit-identical to it.
//
// The float32 order of operations is part of the contract, so every sum runs over c ascending with separately rounded operations
// (__fsub_rn / __fmul_rn / __fadd_rn; the library is built with -ffp-contract=off as well), the square root (taken in float64) and
// the division are the correctly rounded ones, and no matrix or dot instruction is used.
//
// embed_kernel      one wave an image.  The lanes dequantise the image's bytes (out * 2^-sh: exact) into LDS; every lane then adds the
//                   squares in order (broadcast reads: the same sum in every lane) and divides its own features by the root.  It
//                   writes the row to `out` (a gallery row when enrolling) and, for a match, transposed into the scratch as qT [D][Bp]
//                   (Bp = batch rounded up to kEmbGroup) so that stage 1 reads the queries of a wave with wave-uniform loads.
// match_slab_kernel stage 1.  Block (s, g) owns the gallery rows [64 s, 64 s + 64) and the queries [32 g, 32 g + 32).  The block
//                   stages the slab through LDS in chunks of 32 columns (coalesced loads; row stride 36 words: a lane's 16-byte reads
//                   of its own row are conflict-free); lane l of every wave owns row 64 s + l and wave w the queries 32 g + 8 w .. + 7:
//                   eight accumulators a lane, the query values wave-uniform operands.  A distance becomes a 32-bit word whose
//                   unsigned order is the distance order (distances are >= +0; NaN, from a caller's gallery row, becomes +inf).  Round
//                   r of a query takes the wave minimum of the live words and, by ballot, its lowest lane -- the lowest row index --
//                   and retires that lane; lane r keeps the 64-bit key (word << 32 | row).  The slab's k keys leave with one plain
//                   store each into cand [batch][slabs][k]; slots past the slab's rows hold ~0.
// match_merge_kernel stage 2, one block a query: round r takes the smallest key above round r-1's winner among the query's slabs * k
//                   candidates (a thread-local scan with four loads in flight, a butterfly minimum a wave, the four waves' minima
//                   through LDS; nothing is mutated).  Keys are unique (the row index), so the order is total and the result does
//                   not depend on the slab size or the grid.  Lane r of wave 0 writes slot r; lane c of wave 0 adds counter c with
//                   one 64-bit atomicAdd when the query counts for it.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include <vector>
#include "tf2_device.h"
#include "tf2_net.h"
#include "embed_match.h"

namespace tf2 {

namespace {

constexpr int kWaves = 4;                          // waves a block, all three kernels
constexpr int kThreads = 64 * kWaves;
constexpr int kQw = kEmbGroup / kWaves;            // queries a stage-1 wave owns
constexpr int kChunk = 32;                         // gallery columns staged at a time
constexpr int kStride = kChunk + 4;                // LDS row stride in words: 16-byte aligned rows, 9 t mod 16 is a bijection
constexpr uint32_t kDead = 0xffffffffu;            // above every distance word (+inf is 0x7f800000)
constexpr unsigned long long kNoKey = ~0ull;
static_assert(kEmbSlab == 64 && kQw * kWaves == kEmbGroup && kEmbMaxTopK <= 64, "one row a lane, one slot a lane");

__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void embed_kernel(const int8_t* __restrict__ in, const float* __restrict__ scale,
                                                         float* __restrict__ out, float* __restrict__ qT, int d, int batch, int bp) {
  __shared__ float fs[kWaves][kEmbMaxD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kWaves + wave;
  const bool live = b < batch;                     // (wave-uniform)
  float* const f = fs[wave];
  if (live)
    for (int c = lane; c < d; c += 64) f[c] = __fmul_rn((float)in[(long long)b * d + c], scale[c]);
  __syncthreads();
  if (!live) return;
  float s = 0.0f;
  for (int c = 0; c < d; c++) {
    const float v = f[c];
    s = __fadd_rn(s, __fmul_rn(v, v));
  }
  // the correctly rounded float32 root: the float32 square root instruction is good to one unit in the last place only, while a
  // float64 root within one of ITS units, rounded to float32, is the correctly rounded one (the root of a 24-bit number is never
  // within 2^-50 of a float32 rounding boundary)
  const float norm = (float)sqrt((double)s);
  for (int c = lane; c < d; c += 64) {
    const float e = s == 0.0f ? 0.0f : __fdiv_rn(f[c], norm);
    if (out) out[(long long)b * d + c] = e;
    if (qT) qT[(long long)c * bp + b] = e;
  }
}

// one column of the slab against the wave's kQw queries
__device__ __forceinline__ void column(float (&acc)[kQw], const float* __restrict__ q, float g) {
#pragma unroll
  for (int j = 0; j < kQw; j++) {
    const float df = __fsub_rn(q[j], g);
    acc[j] = __fadd_rn(acc[j], __fmul_rn(df, df));
  }
}

__global__ __launch_bounds__(kThreads) void match_slab_kernel(const float* __restrict__ gallery, const float* __restrict__ qT,
                                                              unsigned long long* __restrict__ cand, int d, int n_rows, int batch,
                                                              int bp, int top_k, int vec4) {
  __shared__ __attribute__((aligned(16))) float slab[kEmbSlab * kStride];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long row0 = (long long)blockIdx.x * kEmbSlab;
  const int q0 = blockIdx.y * kEmbGroup + wave * kQw;              // the wave's first query (q0 + kQw <= bp)
  const bool work = q0 < batch;                                     // (wave-uniform)
  const int rows = n_rows - row0 < kEmbSlab ? (int)(n_rows - row0) : kEmbSlab;

  float acc[kQw];
#pragma unroll
  for (int j = 0; j < kQw; j++) acc[j] = 0.0f;

  for (int c0 = 0; c0 < d; c0 += kChunk) {
    const int ck = d - c0 < kChunk ? d - c0 : kChunk;
    if (c0) __syncthreads();                                        // the previous chunk has been read
    if (vec4) {                                                     // d % 4 == 0 and a 16-byte aligned gallery: ck % 4 == 0
      const int per = ck >> 2;                                      // float4 a row
      for (int i = threadIdx.x; i < kEmbSlab * per; i += kThreads) {
        const int r = i / per, v = i - r * per;
        float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r < rows) x = *reinterpret_cast<const float4*>(gallery + (row0 + r) * d + c0 + 4 * v);
        *reinterpret_cast<float4*>(slab + r * kStride + 4 * v) = x;
      }
    } else {
      for (int i = threadIdx.x; i < kEmbSlab * ck; i += kThreads) {
        const int r = i / ck, c = i - r * ck;
        slab[r * kStride + c] = r < rows ? gallery[(row0 + r) * d + c0 + c] : 0.0f;
      }
    }
    __syncthreads();
    if (work) {
      const float* const mine = slab + lane * kStride;
      // wave-uniform loads of the wave's kQw query values.  embed_kernel writes the columns b < batch of qT only: the columns
      // batch .. bp - 1 are whatever the scratch held (NaN perhaps), their accumulators are garbage and the selection below
      // stops at b >= batch before it looks at one
      const float* q = qT + (long long)c0 * bp + q0;
      int c = 0;
      for (; c + 4 <= ck; c += 4) {
        const float4 g = *reinterpret_cast<const float4*>(mine + c);
        column(acc, q, g.x); q += bp;
        column(acc, q, g.y); q += bp;
        column(acc, q, g.z); q += bp;
        column(acc, q, g.w); q += bp;
      }
      for (; c < ck; c++) {
        column(acc, q, mine[c]); q += bp;
      }
    }
  }
  if (!work) return;

  const int nslabs = gridDim.x;
#pragma unroll
  for (int j = 0; j < kQw; j++) {
    const int b = q0 + j;
    if (b >= batch) break;                                          // (wave-uniform)
    const float dist = acc[j];
    uint32_t cur = lane < rows ? (dist != dist ? 0x7f800000u : __float_as_uint(dist)) : kDead;
    unsigned long long keep = kNoKey;
    for (int r = 0; r < top_k; r++) {
      const uint32_t m = wave_min32(cur);
      unsigned long long key = kNoKey;
      if (m != kDead) {                                             // (wave-uniform)
        const int win = __ffsll((unsigned long long)__ballot(cur == m)) - 1;
        key = (unsigned long long)m << 32 | (uint32_t)(row0 + win);
        if (lane == win) cur = kDead;
      }
      if (lane == r) keep = key;
    }
    if (lane < top_k) cand[((long long)b * nslabs + blockIdx.x) * top_k + lane] = keep;
  }
}

struct MergeArgs {
  const unsigned long long* cand;    // [batch][slabs][top_k]
  const int32_t* gallery_ids;        // [n_rows] or null
  int32_t* idx;                      // [batch][top_k]
  float* dist;                       // [batch][top_k]
  int32_t* ids_out;                  // [batch][top_k] or null
  const int32_t* truth;              // [batch] or null
  unsigned long long* tally;         // [5] or null, accumulated
  float threshold;
  int32_t nslabs, top_k, batch;
};

__global__ __launch_bounds__(kThreads) void match_merge_kernel(MergeArgs a) {
  __shared__ unsigned long long wave_best[2][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;                        // the grid is the batch: every branch on b is uniform over the block
  const int k = a.top_k;
  const long long n = (long long)a.nslabs * k;
  const unsigned long long* const cq = a.cand + (long long)b * n;
  unsigned long long prev = 0, mine = kNoKey;
  for (int r = 0; r < k; r++) {
    unsigned long long best = kNoKey;              // an empty slot: never taken, and it ends the query's list
    auto take = [&](unsigned long long key) {
      if ((r == 0 || key > prev) && key < best) best = key;
    };
    long long i = threadIdx.x;
    for (; i + 3 * kThreads < n; i += 4 * kThreads) {             // four loads in flight a thread: the scan is load latency
      const unsigned long long k0 = cq[i], k1 = cq[i + kThreads], k2 = cq[i + 2 * kThreads], k3 = cq[i + 3 * kThreads];
      take(k0); take(k1); take(k2); take(k3);
    }
    for (; i < n; i += kThreads) take(cq[i]);
    best = wave_min64(best);
    if (lane == 0) wave_best[r & 1][wave] = best;
    __syncthreads();                               // (round r + 1 writes the other half; r + 2 comes after r + 1's barrier)
    prev = wave_best[r & 1][0];
#pragma unroll
    for (int w = 1; w < kWaves; w++) {
      const unsigned long long o = wave_best[r & 1][w];
      prev = o < prev ? o : prev;
    }
    if ((int)threadIdx.x == r) mine = prev;
  }
  if (wave) return;                                // wave 0: lane r holds slot r

  const bool have = mine != kNoKey;
  const int row = have ? (int)(uint32_t)mine : -1;
  const float dist = have ? __uint_as_float((uint32_t)(mine >> 32)) : __uint_as_float(0x7f800000u);
  int id = row;
  if (have && a.gallery_ids) id = a.gallery_ids[row];
  const long long o = (long long)b * k + lane;
  if (lane < k) {
    a.idx[o] = row;
    a.dist[o] = dist;
    if (a.ids_out) a.ids_out[o] = id;
  }
  const int t = a.truth ? a.truth[b] : -1;
  if (t < 0 || !a.tally) return;                   // (wave-uniform) unlabelled: nothing is counted
  const bool among = __ballot(lane < k && have && id == t) != 0;
  const int id0 = __shfl(id, 0, 64);
  const bool accept = __shfl(dist, 0, 64) < a.threshold;
  // bit 0 labelled, 1 identified, 2 among the k, 3 true accept, 4 false accept: lane c adds counter c
  const uint32_t flags = 1u | (id0 == t ? 2u : 0u) | (among ? 4u : 0u) | (accept && id0 == t ? 8u : 0u) | (accept && id0 != t ? 16u : 0u);
  if (lane < 5 && (flags >> lane & 1u)) atomicAdd(a.tally + lane, 1ull);
}

int padded_batch(int batch) { return (batch + kEmbGroup - 1) / kEmbGroup * kEmbGroup; }
long long slabs_of(long long n_rows) { return (n_rows + kEmbSlab - 1) / kEmbSlab; }

}  // namespace

Matcher::~Matcher() {
  if (consts) (void)hipFree(consts);
}

tf2_status Matcher::create(const Net* net, const tf2_emb_desc* desc) {
  auto fail = [](const std::string& m) { return arg_refusal("tf2_emb_create", m); };
  if (!desc || desc->size != sizeof(tf2_emb_desc)) return fail("desc size: missing, or not sizeof(tf2_emb_desc)");
  if (net->q.empty()) { set_error("tf2_emb_create: q table not set (tf2_net_set_q first)"); return TF2_ERR_STATE; }
  const tf2_layer_desc& LL = net->layers[net->nd.n_layers - 1];
  if (net->logits_bytes(1) != (size_t)LL.N) return fail("the net's final map is not 1 x 1: its output is not one embedding row an image");
  for (int l = 0; l + 1 < net->nd.n_layers; l++)
    if (net->is_sink(l)) return fail("row " + std::to_string(l) + " is a network output as well: the final map is not one 1 x 1 embedding row (a detection net: tf2_ssd_*)");
  if (net->nd.n_layers >= net->nd.n_q_rows || LL.N > net->nd.max_out_channel) return fail("the q table has no row for the last layer's output");
  if (LL.N < 2 || LL.N > kEmbMaxD) {
    set_error("tf2_emb_create: an embedding of " + std::to_string(LL.N) + " values; the kernels take 2.." + std::to_string(kEmbMaxD));
    return TF2_ERR_UNSUPPORTED;
  }
  const int8_t* const qr = net->q.data() + (size_t)net->nd.n_layers * net->nd.max_out_channel;
  std::vector<float> scale(LL.N);
  for (int i = 0; i < LL.N; i++) {
    const int sh = -(int)qr[i];
    if (sh < 0 || sh > 30) return fail("Q of the last layer must be in 0..30; channel " + std::to_string(i) + " has " + std::to_string(sh));
    scale[i] = std::ldexp(1.0f, -sh);
  }
  if (desc->top_k < 1 || desc->top_k > kEmbMaxTopK) return fail("top_k must be in 1.." + std::to_string(kEmbMaxTopK));
  d = LL.N; top_k = desc->top_k;
  hipError_t e = hipMalloc(&consts, (size_t)d * 4);
  if (e == hipSuccess) e = hipMemcpy(consts, scale.data(), (size_t)d * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { set_error(std::string("tf2_emb_create: ") + hipGetErrorString(e)); return TF2_ERR_HIP; }
  return TF2_OK;
}

// qT float32 [d][Bp], then cand uint64 [batch][slabs][top_k] (d * Bp * 4 is a multiple of 128: the keys are 8-byte aligned)
size_t Matcher::scratch_size(int batch, long long n_rows) const {
  if (batch < 1 || n_rows < 1) return 0;
  return (size_t)d * padded_batch(batch) * 4 + (size_t)batch * slabs_of(n_rows) * top_k * 8;
}

tf2_status Matcher::embed(const int8_t* out_i8, int batch, float* rows, void* stream) {
  const dim3 grid((unsigned)((batch + kWaves - 1) / kWaves)), block(kThreads);
  hipLaunchKernelGGL(embed_kernel, grid, block, 0, (hipStream_t)stream, out_i8, (const float*)consts, rows, (float*)nullptr, d, batch, 0);
  return launch_result("tf2_emb_embed");
}

tf2_status Matcher::match(const int8_t* out_i8, int batch, const float* gallery, const int32_t* gallery_ids, long long n_rows,
                          float threshold, void* scratch, size_t scratch_bytes, int32_t* idx, float* dist, int32_t* ids_out,
                          float* emb_out, const int32_t* truth, uint64_t* tally, void* stream) {
  // (batch, n_rows, the required pointers and the threshold: checked by tf2_emb_match before it looks at the handle)
  const size_t need = scratch_size(batch, n_rows);
  if (scratch_bytes < need) {
    set_error("tf2_emb_match: scratch_bytes " + std::to_string(scratch_bytes) + " < tf2_emb_scratch_size " + std::to_string(need));
    return TF2_ERR_SIZE;
  }
  if (((uintptr_t)scratch & 7) != 0) return arg_refusal("tf2_emb_match", "scratch_dev must be 8-byte aligned");
  const int bp = padded_batch(batch);
  const long long slabs = slabs_of(n_rows);
  if (slabs > 0x7fffffffll || (long long)bp / kEmbGroup > 65535) { set_error("tf2_emb_match: too many slabs or query groups for one grid"); return TF2_ERR_UNSUPPORTED; }
  float* const qT = (float*)scratch;
  unsigned long long* const cand = (unsigned long long*)((char*)scratch + (size_t)d * bp * 4);
  const dim3 block(kThreads);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(embed_kernel, dim3((unsigned)((batch + kWaves - 1) / kWaves)), block, 0, st, out_i8, (const float*)consts, emb_out, qT, d, batch, bp);
  const int vec4 = (d % 4 == 0 && ((uintptr_t)gallery & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(match_slab_kernel, dim3((unsigned)slabs, (unsigned)(bp / kEmbGroup)), block, 0, st, gallery, (const float*)qT, cand, d,
                     (int)n_rows, batch, bp, top_k, vec4);
  MergeArgs a{};
  a.cand = cand; a.gallery_ids = gallery_ids; a.idx = idx; a.dist = dist; a.ids_out = ids_out; a.truth = truth;
  a.tally = reinterpret_cast<unsigned long long*>(tally);
  a.threshold = threshold; a.nslabs = (int)slabs; a.top_k = top_k; a.batch = batch;
  hipLaunchKernelGGL(match_merge_kernel, dim3((unsigned)batch), block, 0, st, a);
  return launch_result("tf2_emb_match");
}

}  // namespace tf2
