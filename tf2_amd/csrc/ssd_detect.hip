// ssd_detect.hip -- SSD detection on the device (gfx950): the multibox heads of a step -> boxes, class probabilities, and per
// (image, class) the best top_k candidates after greedy NMS.  The stage of Detect (detection.py:27-62, box_utils.py:140-158
// decode, :175-239 nms) with its tie order pinned (INTEGRATION.md "SSD detection"):
//   ssd_heads_kernel      one thread per (image, prior): dequantise 4 loc + C conf int8 values (exact, 2^-Q), float32 softmax
//                         (max-subtracted), decode in the operation order of ssd.decode
//   ssd_select_kernel     one block per (image, class): candidates p > conf_thresh, radix select of the best top_k under
//                         (score descending, prior index ascending), IoU bitmask of the survivors, one wave walks it greedily
//   ssd_transpose_kernel  [B][P][C] -> [B][C][P] for tf2_ssd_detect's caller-layout scores
// Everything compares and divides in IEEE float32 (-ffp-contract=off, no fast-math intrinsics): the host statement
// ssd.detect_ordered gives bit-identical rows.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <mutex>
#include "tf2_device.h"
#include "ssd_detect.h"

namespace tf2 {

#define SSD_HIP_OK(expr)                                                              \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                   \
      return TF2_ERR_HIP;                                                             \
    }                                                                                 \
  } while (0)

// ---- stage 1 ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ssd_deq(int8_t v, int ch, const float* scale, const uint8_t* dbl) {
  int x = v;
  if (dbl[ch]) x = (x + 128) >> 1;           // doubled channels hold 2y - 128 (weight_pack.cpp; Net::read_layer)
  return (float)x * scale[ch];               // scale = 2^-Q: exact
}

__global__ void __launch_bounds__(256) ssd_heads_kernel(SsdHeadArgs a) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long)a.batch * a.P) return;
  const int b = (int)(gid / a.P), p = (int)(gid - (long)b * a.P);
  // the source of this prior: unrolled over the (uniform) tables so that no argument array is indexed by a lane value
  const int8_t* lsrc = a.loc[0]; const int8_t* csrc = a.conf[0];
  int lcp = a.loc_cp[0], ccp = a.conf_cp[0], hw = a.hw[0], nb = a.nb[0], st = a.start[0], lch = a.loc_ch0[0], cch = a.conf_ch0[0];
#pragma unroll
  for (int s = 1; s < kSsdMaxSources; s++)
    if (s < a.n_src && p >= a.start[s]) {
      lsrc = a.loc[s]; csrc = a.conf[s]; lcp = a.loc_cp[s]; ccp = a.conf_cp[s]; hw = a.hw[s]; nb = a.nb[s]; st = a.start[s];
      lch = a.loc_ch0[s]; cch = a.conf_ch0[s];
    }
  const int rem = p - st, cell = rem / nb, box = rem - cell * nb;
  const size_t pix = (size_t)b * hw + cell;
  const int8_t* lp = lsrc + pix * lcp + box * 4;
  const int8_t* cp = csrc + pix * ccp + (size_t)box * a.C;
  lch += box * 4; cch += box * a.C;
  const int C = a.C;
  // softmax over the classes (float32, max-subtracted); exp is recomputed instead of kept (C <= 256 values a lane)
  float m = -INFINITY;
  for (int c = 0; c < C; c++) m = fmaxf(m, ssd_deq(cp[c], cch + c, a.scale, a.dbl));
  float sum = 0.f;
  for (int c = 0; c < C; c++) sum += expf(ssd_deq(cp[c], cch + c, a.scale, a.dbl) - m);
  float* pr = a.probs + (size_t)b * C * a.P + p;
  float* so = a.scores_out ? a.scores_out + ((size_t)b * a.P + p) * C : nullptr;
  for (int c = 0; c < C; c++) {
    const float v = expf(ssd_deq(cp[c], cch + c, a.scale, a.dbl) - m) / sum;
    pr[(size_t)c * a.P] = v;
    if (so) so[c] = v;
  }
  // decode (ssd.decode, box_utils.py:140-158): centre = p_c + (t * v0) * p_wh, size = p_wh * exp(t * v1), x1 = centre - size / 2,
  // x2 = x1 + size
  const float4 q = *reinterpret_cast<const float4*>(a.priors + (size_t)p * 4);
  const float t0 = ssd_deq(lp[0], lch, a.scale, a.dbl), t1 = ssd_deq(lp[1], lch + 1, a.scale, a.dbl);
  const float t2 = ssd_deq(lp[2], lch + 2, a.scale, a.dbl), t3 = ssd_deq(lp[3], lch + 3, a.scale, a.dbl);
  const float cx = q.x + (t0 * a.v0) * q.z, cy = q.y + (t1 * a.v0) * q.w;
  const float w = q.z * expf(t2 * a.v1), h = q.w * expf(t3 * a.v1);
  const float x1 = cx - w / 2.f, y1 = cy - h / 2.f;
  *reinterpret_cast<float4*>(a.boxes + gid * 4) = make_float4(x1, y1, x1 + w, y1 + h);
}

__global__ void __launch_bounds__(256) ssd_transpose_kernel(const float* src, float* dst, int batch, int P, int C) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long n = (long)batch * P * C;
  if (gid >= n) return;
  // gid walks the DESTINATION [b][c][p] (coalesced stores)
  const int p = (int)(gid % P);
  const long bc = gid / P;
  const int c = (int)(bc % C), b = (int)(bc / C);
  dst[gid] = src[((size_t)b * P + p) * C + c];
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------
constexpr int kSelThreads = 512;
constexpr int kSelWaves = kSelThreads / 64;
// LDS: a fixed part, then one region that holds the class's score keys during the selection and the survivors' boxes, areas and
// IoU bitmask afterwards
constexpr int kSelFixed = 256 * 4 /*hist*/ + 16 * 4 /*misc*/ + kSelWaves * 4 /*wave sums*/ + 256 * 8 /*keys*/ + 256 * 4 /*sel_idx*/ +
                          256 * 4 /*sel_key*/ + 256 * 4 /*keep*/;
constexpr int kSelPost = 256 * 16 /*boxes*/ + 256 * 4 /*areas*/ + 256 * 4 * 8 /*mask*/;

static size_t select_lds_bytes(int P) { return (size_t)kSelFixed + (size_t)std::max(P * 4, kSelPost); }

// Exclusive prefix sum of one value per thread over the block (wave64 shuffles, then the wave totals); returns the total too.
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* wave_sums, unsigned* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wave_sums[wave] = x;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kSelWaves; w++) {
    const unsigned s = wave_sums[w];
    if (w < wave) before += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

// Wave 0: the histogram bin (searched from the top) in which the `need`-th best key lies.  misc[0] = bin, misc[1] = keys in the bins
// above it, misc[2] = keys in the bin, misc[3] = keys in all bins.
__device__ __forceinline__ void find_bin(const unsigned* hist, unsigned need, unsigned* misc) {
  const int lane = threadIdx.x;
  const unsigned h0 = hist[255 - 4 * lane], h1 = hist[254 - 4 * lane], h2 = hist[253 - 4 * lane], h3 = hist[252 - 4 * lane];
  const unsigned s = h0 + h1 + h2 + h3;
  unsigned incl = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned y = __shfl_up(incl, d, 64);
    if (lane >= d) incl += y;
  }
  const unsigned long long hit = __ballot(incl >= need);
  const int first = hit ? __ffsll((long long)hit) - 1 : 63;
  if (lane == first) {
    unsigned cum = incl - s, hj = h3;
    int j = 3;
    if (cum + h0 >= need) { j = 0; hj = h0; }
    else if (cum + h0 + h1 >= need) { j = 1; hj = h1; cum += h0; }
    else if (cum + h0 + h1 + h2 >= need) { j = 2; hj = h2; cum += h0 + h1; }
    else cum += h0 + h1 + h2;
    misc[0] = 255 - 4 * lane - j; misc[1] = cum; misc[2] = hj;
  }
  if (lane == 63) misc[3] = incl;
}

// IoU of `kept` with `other` exactly as ssd._iou_one_to_many evaluates it, one float32 operation at a time
__device__ __forceinline__ float ssd_iou(float4 kept, float area_kept, float4 other, float area_other) {
  const float lx = fmaxf(other.x, kept.x), ly = fmaxf(other.y, kept.y);
  const float hx = fminf(other.z, kept.z), hy = fminf(other.w, kept.w);
  const float wx = fmaxf(hx - lx, 0.f), wy = fmaxf(hy - ly, 0.f);
  const float inter = wx * wy;
  return inter / ((area_other - inter) + area_kept);
}

__global__ void __launch_bounds__(kSelThreads) ssd_select_kernel(SsdSelectArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned* const hist = reinterpret_cast<unsigned*>(smem);
  unsigned* const misc = hist + 256;
  unsigned* const wave_sums = misc + 16;
  unsigned long long* const keys = reinterpret_cast<unsigned long long*>(wave_sums + kSelWaves);
  int* const sel_idx = reinterpret_cast<int*>(keys + 256);
  unsigned* const sel_key = reinterpret_cast<unsigned*>(sel_idx + 256);
  int* const keep = reinterpret_cast<int*>(sel_key + 256);
  unsigned char* const region = smem + kSelFixed;
  unsigned* const sc = reinterpret_cast<unsigned*>(region);                 // selection: key of prior i (0 = no candidate)
  float4* const bx = reinterpret_cast<float4*>(region);                    // afterwards: survivors' boxes, areas, IoU bitmask
  float* const area = reinterpret_cast<float*>(bx + 256);
  unsigned long long* const mask = reinterpret_cast<unsigned long long*>(area + 256);

  const int tid = threadIdx.x;
  const int P = a.P, C = a.C, K = a.top_k;
  const int c = blockIdx.x % C, b = blockIdx.x / C;
  float* const det = a.det + ((size_t)b * C + c) * K * 5;
  if (c == 0) {                                   // background: no rows
    for (int i = tid; i < K * 5; i += kSelThreads) det[i] = 0.f;
    if (tid == 0) a.counts[(size_t)b * C] = 0;
    return;
  }
  // candidates: p > conf_thresh (>= 0, so a candidate is a positive float and its bit pattern orders it); histogram of the top byte
  for (int i = tid; i < 256; i += kSelThreads) hist[i] = 0;
  if (tid < 16) misc[tid] = 0;
  __syncthreads();
  const float* const pr = a.probs + ((size_t)b * C + c) * P;
  for (int i = tid; i < P; i += kSelThreads) {
    const float v = pr[i];
    const unsigned u = v > a.conf_thresh ? __float_as_uint(v) : 0u;
    sc[i] = u;
    if (u) atomicAdd(&hist[u >> 24], 1u);
  }
  __syncthreads();
  // radix select of the K-th best score: the keys above `thr_hi` (at digit level `sh`) are taken, of those equal to it the `need`
  // with the lowest prior indices
  unsigned need = (unsigned)K, prefix = 0;
  int sh = 0;
  bool all_taken = false;
  for (int level = 24; level >= 0; level -= 8) {
    if (level < 24) {
      for (int i = tid; i < 256; i += kSelThreads) hist[i] = 0;
      __syncthreads();
      const unsigned hi_sh = (unsigned)(level + 8);
      for (int i = tid; i < P; i += kSelThreads) {
        const unsigned u = sc[i];
        if (u && (u >> hi_sh) == (prefix >> hi_sh)) atomicAdd(&hist[(u >> level) & 255u], 1u);
      }
      __syncthreads();
    }
    if (tid < 64) find_bin(hist, need, misc);
    __syncthreads();
    if (level == 24 && misc[3] <= need) {       // no more candidates than top_k: every one is taken
      all_taken = true; sh = 31; prefix = 0; need = 0;
      __syncthreads();
      break;
    }
    const unsigned bin = misc[0], above = misc[1], inbin = misc[2];
    prefix |= bin << level;
    need -= above;
    sh = level;
    __syncthreads();                             // (misc is rewritten by the next level)
    if (inbin == need) { all_taken = true; break; }   // the whole bin is taken: no finer digit matters
  }
  // the cut: key >> sh above thr_hi, or equal to it and among the first `need` such priors in index order (ties by index ascending).
  // Thread t owns priors [t * per, (t + 1) * per): its tie count, a block scan, then its rank among the ties.
  const unsigned thr_hi = all_taken && sh == 31 ? 0u : (prefix >> sh);
  const int per = (P + kSelThreads - 1) / kSelThreads;
  const int i0 = min(P, tid * per), i1 = min(P, i0 + per);
  unsigned ties = 0;
  if (!all_taken)
    for (int i = i0; i < i1; i++) {
      const unsigned u = sc[i];
      ties += (u && (u >> sh) == thr_hi) ? 1u : 0u;
    }
  unsigned n_ties = 0;
  unsigned rank = block_exclusive_scan(ties, wave_sums, &n_ties);
  for (int i = i0; i < i1; i++) {
    const unsigned u = sc[i];
    if (!u) continue;
    const unsigned hi = sh == 31 ? 0u : (u >> sh);
    bool take;
    if (all_taken) take = hi >= thr_hi;
    else if (hi != thr_hi) take = hi > thr_hi;
    else take = rank++ < need;
    if (take) {
      const unsigned slot = atomicAdd(&misc[4], 1u);
      if (slot < (unsigned)K) keys[slot] = ((unsigned long long)u << 32) | (0xffffffffu - (unsigned)i);   // larger = better: score, then the LOWER index
    }
  }
  __syncthreads();
  const int n = min((int)misc[4], K);            // == min(top_k, candidates)
  // order the survivors best first: rank = number of better keys (keys are distinct)
  if (tid < n) {
    const unsigned long long k = keys[tid];
    int r = 0;
    for (int j = 0; j < n; j++) r += keys[j] > k ? 1 : 0;
    sel_idx[r] = (int)(0xffffffffu - (unsigned)k);
    sel_key[r] = (unsigned)(k >> 32);
  }
  __syncthreads();
  // the region now holds the survivors' boxes and areas, then the IoU bitmask: bit j of row i (j > i) = !(IoU(kept i, other j) <= nms_thresh)
  const float* const boxes = a.boxes + (size_t)b * P * 4;
  if (tid < n) {
    const float4 q = *reinterpret_cast<const float4*>(boxes + (size_t)sel_idx[tid] * 4);
    bx[tid] = q;
    area[tid] = (q.z - q.x) * (q.w - q.y);
  }
  __syncthreads();
  const int nw = (n + 63) >> 6;
  for (int it = tid; it < n * nw; it += kSelThreads) {
    const int i = it / nw, w = it - i * nw;
    const float4 ki = bx[i];
    const float ai = area[i];
    unsigned long long bits = 0;
    const int j0 = max(w * 64, i + 1), j1 = min(n, w * 64 + 64);
    for (int j = j0; j < j1; j++)
      if (!(ssd_iou(ki, ai, bx[j], area[j]) <= a.nms_thresh)) bits |= 1ull << (j - w * 64);   // (a NaN IoU suppresses, as IoU.le does)
    mask[i * 4 + w] = bits;
  }
  __syncthreads();
  // greedy walk (wave 0; every lane keeps the same removed-set): keep i unless a kept box suppressed it
  if (tid < 64) {
    unsigned long long r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    int nk = 0;
    for (int i = 0; i < n; i++) {
      const int w = i >> 6;
      const unsigned long long rw = w == 0 ? r0 : w == 1 ? r1 : w == 2 ? r2 : r3;
      if ((rw >> (i & 63)) & 1ull) continue;
      if (tid == 0) keep[nk] = i;
      nk++;
      const unsigned long long* m = mask + i * 4;
      if (nw > 0) r0 |= m[0];
      if (nw > 1) r1 |= m[1];
      if (nw > 2) r2 |= m[2];
      if (nw > 3) r3 |= m[3];
    }
    if (tid == 0) misc[5] = (unsigned)nk;
  }
  __syncthreads();
  const int nk = (int)misc[5];
  for (int r = tid; r < K; r += kSelThreads) {
    float* row = det + (size_t)r * 5;
    if (r < nk) {
      const int i = keep[r];
      const float4 q = bx[i];
      row[0] = __uint_as_float(sel_key[i]); row[1] = q.x; row[2] = q.y; row[3] = q.z; row[4] = q.w;
    } else {
      row[0] = 0.f; row[1] = 0.f; row[2] = 0.f; row[3] = 0.f; row[4] = 0.f;
    }
  }
  if (tid == 0) a.counts[(size_t)b * C + c] = nk;
}

int launch_ssd_heads(const SsdHeadArgs& a, void* stream) {
  const long n = (long)a.batch * a.P;
  hipLaunchKernelGGL(ssd_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_ssd_transpose(const float* src, float* dst, int batch, int P, int C, void* stream) {
  const long n = (long)batch * P * C;
  hipLaunchKernelGGL(ssd_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, batch, P, C);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_ssd_select(const SsdSelectArgs& a, void* stream) {
  const size_t lds = select_lds_bytes(a.P);
  if (lds > 64 * 1024 && !lds_attr_once(reinterpret_cast<const void*>(&ssd_select_kernel))) return -1;
  hipLaunchKernelGGL(ssd_select_kernel, dim3((unsigned)(a.batch * a.C)), dim3(kSelThreads), lds, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the detector handle -----------------------------------------------------------------------------------------------
static size_t align256(size_t x) { return (x + 255) / 256 * 256; }

SsdDetector::~SsdDetector() {
  if (consts) (void)hipFree(consts);
}

tf2_status SsdDetector::create(Net* n, const tf2_ssd_desc* d) {
  auto fail = [](const std::string& m) { return arg_refusal("tf2_ssd_create", m); };
  if (!d || d->size < sizeof(tf2_ssd_desc)) return fail("desc missing or older than this library's tf2_ssd_desc");
  if (!n->packed_valid) { set_error("tf2_ssd_create: no packed image (tf2_net_pack / tf2_net_packed_adopt first)"); return TF2_ERR_STATE; }
  if (n->q.empty()) { set_error("tf2_ssd_create: q table not set"); return TF2_ERR_STATE; }
  if (d->num_classes < 2 || d->num_classes > kSsdMaxClasses) return fail("num_classes must be in 2.." + std::to_string(kSsdMaxClasses));
  if (d->top_k < 1 || d->top_k > kSsdMaxTopK) return fail("top_k must be in 1.." + std::to_string(kSsdMaxTopK));
  if (!(d->nms_thresh > 0.f) || !std::isfinite(d->nms_thresh)) return fail("nms_thresh must be positive and finite");
  if (!(d->conf_thresh >= 0.f) || !std::isfinite(d->conf_thresh)) return fail("conf_thresh must be >= 0 and finite");
  if (!std::isfinite(d->variance[0]) || !std::isfinite(d->variance[1])) return fail("variance must be finite");
  if (d->n_sources < 1 || d->n_sources > kSsdMaxSources) return fail("n_sources must be in 1.." + std::to_string(kSsdMaxSources));
  if (!d->priors || d->n_priors < 1 || d->n_priors > kSsdMaxPriors) return fail("priors missing or n_priors outside 1.." + std::to_string(kSsdMaxPriors));
  const int nl = n->nd.n_layers, C = d->num_classes;
  std::vector<char> used(nl, 0);
  int total = 0, n_ch = 0;
  for (int s = 0; s < d->n_sources; s++) {
    const int lr = d->loc_row[s], cr = d->conf_row[s];
    const std::string src = "source " + std::to_string(s) + ": ";
    if (lr < 0 || lr >= nl || cr < 0 || cr >= nl) return fail(src + "head row outside the table");
    if (lr == cr || used[lr] || used[cr]) return fail(src + "a head row is named twice");
    used[lr] = used[cr] = 1;
    const tf2_layer_desc& Ll = n->layers[lr];
    const tf2_layer_desc& Lc = n->layers[cr];
    for (int r : {lr, cr}) {
      if (n->layers[r].concat >= 0) return fail(src + "row " + std::to_string(r) + " is a concat member");
      if (!n->is_sink(r)) return fail(src + "row " + std::to_string(r) + " is read by another row (not a network output)");
    }
    if (Ll.N % 4) return fail(src + "loc row " + std::to_string(lr) + " has N = " + std::to_string(Ll.N) + ", not 4 * boxes");
    const int nbx = Ll.N / 4;
    if (Lc.N != nbx * C)
      return fail(src + "conf row " + std::to_string(cr) + " has N = " + std::to_string(Lc.N) + ", expected boxes * num_classes = " +
                  std::to_string(nbx * C));
    const int lh = Ll.endpool ? 1 : Ll.PH, lw = Ll.endpool ? 1 : Ll.PW, ch = Lc.endpool ? 1 : Lc.PH, cw = Lc.endpool ? 1 : Lc.PW;
    if (lh != ch || lw != cw) return fail(src + "loc and conf rows have different maps");
    loc_row[s] = lr; conf_row[s] = cr; nb[s] = nbx; hw[s] = lh * lw; start[s] = total;
    loc_ch0[s] = n_ch; n_ch += Ll.N;
    conf_ch0[s] = n_ch; n_ch += Lc.N;
    total += lh * lw * nbx;
  }
  if (total != d->n_priors)
    return fail("the heads hold " + std::to_string(total) + " boxes per image, n_priors is " + std::to_string(d->n_priors));
  net = n;
  this->C = C; top_k = d->top_k; n_src = d->n_sources; P = d->n_priors;
  conf_thresh = d->conf_thresh; nms_thresh = d->nms_thresh; v0 = d->variance[0]; v1 = d->variance[1];
  // per head channel: 2^-Q from the runtime q table (row l + 1 is the Q the row requantised to) and the doubled-form flag
  std::vector<float> scale(n_ch);
  std::vector<uint8_t> dbl(n_ch, 0);
  const int M = n->nd.max_out_channel;
  for (int s = 0; s < n_src; s++)
    for (int k = 0; k < 2; k++) {
      const int row = k ? conf_row[s] : loc_row[s], ch0 = k ? conf_ch0[s] : loc_ch0[s];
      const int8_t* qr = n->q.data() + (size_t)(row + 1) * M;
      const PackLayer* pl = n->pack_layer(row);
      const uint8_t* f = (pl && pl->off_dbl) ? n->packed.data() + pl->off_dbl : nullptr;
      for (int c = 0; c < n->layers[row].N; c++) {
        scale[ch0 + c] = std::ldexp(1.0f, qr[c]);      // runtime q = -Q
        dbl[ch0 + c] = f && f[c] ? 1 : 0;
      }
    }
  const size_t pri_bytes = (size_t)P * 16, sc_bytes = align256((size_t)n_ch * 4);
  SSD_HIP_OK(hipMalloc(&consts, align256(pri_bytes) + sc_bytes + align256(n_ch)));
  uint8_t* base = (uint8_t*)consts;
  priors_dev = (const float*)base;
  scale_dev = (const float*)(base + align256(pri_bytes));
  dbl_dev = base + align256(pri_bytes) + sc_bytes;
  SSD_HIP_OK(hipMemcpy((void*)priors_dev, d->priors, pri_bytes, hipMemcpyHostToDevice));
  SSD_HIP_OK(hipMemcpy((void*)scale_dev, scale.data(), (size_t)n_ch * 4, hipMemcpyHostToDevice));
  SSD_HIP_OK(hipMemcpy((void*)dbl_dev, dbl.data(), (size_t)n_ch, hipMemcpyHostToDevice));
  return TF2_OK;
}

// workspace of tf2_ssd_run: the outputs-kept plan, then boxes [B][P][4] and class-major probabilities [B][C][P]
size_t SsdDetector::workspace_size(int batch) {
  if (batch <= 0) return 0;
  size_t plan_bytes;
  { std::lock_guard<std::mutex> lock(net->run_mutex); plan_bytes = net->plan(batch, PLAN_OUTPUTS)->total_bytes; }
  return align256(plan_bytes) + align256((size_t)batch * P * 16) + detect_scratch_size(batch);
}

size_t SsdDetector::detect_scratch_size(int batch) const { return batch <= 0 ? 0 : align256((size_t)batch * C * P * 4); }

tf2_status SsdDetector::run(const void* images, bool images_are_q, int batch, void* ws, size_t ws_bytes, float* det, int32_t* counts,
                            float* boxes_out, float* scores_out, int8_t* logits, void* mark_event, void* stream) {
  if (batch <= 0) return arg_refusal("tf2_ssd_run", "batch must be positive");
  if (!images || !ws || !det || !counts) return arg_refusal("tf2_ssd_run", "null device pointer");
  const size_t need = workspace_size(batch);
  if (ws_bytes < need) { set_error("tf2_ssd_run: workspace too small (tf2_ssd_workspace_size: " + std::to_string(need) + ")"); return TF2_ERR_SIZE; }
  if (tf2_status st = net->run(images, images_are_q, batch, ws, ws_bytes, logits, stream, -1, nullptr, -1, true)) return st;
  if (mark_event) SSD_HIP_OK(hipEventRecord((hipEvent_t)mark_event, (hipStream_t)stream));
  const WorkPlan* wp;
  { std::lock_guard<std::mutex> lock(net->run_mutex); wp = net->plan(batch, PLAN_OUTPUTS); }   // (map nodes are stable)
  uint8_t* const base = (uint8_t*)ws;
  SsdHeadArgs h{};
  for (int s = 0; s < n_src; s++) {
    const LayerExec& El = wp->exec[loc_row[s]];
    const LayerExec& Ec = wp->exec[conf_row[s]];
    const TensorPlan& tl = wp->tensors[El.out_tensor];
    const TensorPlan& tc = wp->tensors[Ec.out_tensor];
    h.loc[s] = (const int8_t*)(base + tl.offset + El.out_off); h.loc_cp[s] = tl.Cp;
    h.conf[s] = (const int8_t*)(base + tc.offset + Ec.out_off); h.conf_cp[s] = tc.Cp;
    h.hw[s] = hw[s]; h.nb[s] = nb[s]; h.start[s] = start[s]; h.loc_ch0[s] = loc_ch0[s]; h.conf_ch0[s] = conf_ch0[s];
  }
  h.n_src = n_src; h.P = P; h.C = C; h.batch = batch; h.v0 = v0; h.v1 = v1;
  h.priors = priors_dev; h.scale = scale_dev; h.dbl = dbl_dev;
  const size_t off_boxes = align256(wp->total_bytes), off_probs = off_boxes + align256((size_t)batch * P * 16);
  h.boxes = boxes_out ? boxes_out : (float*)(base + off_boxes);
  h.probs = (float*)(base + off_probs);
  h.scores_out = scores_out;
  if (launch_ssd_heads(h, stream)) { set_error(std::string("tf2_ssd_run: head decode launch failed: ") + hipGetErrorString(hipGetLastError())); return TF2_ERR_HIP; }
  SsdSelectArgs sa{h.boxes, h.probs, det, counts, P, C, top_k, batch, conf_thresh, nms_thresh};
  if (launch_ssd_select(sa, stream)) { set_error(std::string("tf2_ssd_run: select launch failed: ") + hipGetErrorString(hipGetLastError())); return TF2_ERR_HIP; }
  return TF2_OK;
}

tf2_status SsdDetector::detect(const float* boxes, const float* scores, int batch, void* scratch, size_t scratch_bytes, float* det,
                               int32_t* counts, void* stream) {
  if (batch <= 0) return arg_refusal("tf2_ssd_detect", "batch must be positive");
  if (!boxes || !scores || !scratch || !det || !counts) return arg_refusal("tf2_ssd_detect", "null device pointer");
  if (scratch_bytes < detect_scratch_size(batch)) { set_error("tf2_ssd_detect: scratch too small (tf2_ssd_detect_scratch_size)"); return TF2_ERR_SIZE; }
  float* probs = (float*)scratch;
  if (launch_ssd_transpose(scores, probs, batch, P, C, stream)) { set_error("tf2_ssd_detect: transpose launch failed"); return TF2_ERR_HIP; }
  SsdSelectArgs sa{boxes, probs, det, counts, P, C, top_k, batch, conf_thresh, nms_thresh};
  if (launch_ssd_select(sa, stream)) { set_error("tf2_ssd_detect: select launch failed"); return TF2_ERR_HIP; }
  return TF2_OK;
}

}  // namespace tf2
