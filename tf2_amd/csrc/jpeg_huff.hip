// jpeg_huff.hip -- the entropy-coded bytes of a batch of baseline JPEG files -> the dense coefficient blocks tf2_jpeg_idct reads
// (tf2_jpeg_huff, include/tf2_amd.h, which states the whole rule): self-synchronising parallel Huffman decoding.  tf2_amd/jpeg.py
// restates the algorithm (jpeg.reference_huff) and the device output is bit-identical to it; for files the host decoder
// (jpeg_entropy.cpp) takes, to that decoder's buffer.
//
// One workgroup of kHuffThreads threads an image, whatever the records hold.  It validates the records, builds the 2 * components
// lookup tables in LDS (a 9-bit first-level table and the maxcode walk, as the host has), zeroes the image's coefficient extent, and
// then walks the data in chunks of jpeg_huff_chunk_lanes(subseq_bytes) subsequences, one lane each:
//   rounds   every lane decodes tolerantly from its entry state to the end of its subsequence; a lane whose entry (the left
//            neighbour's exit of the round before) changed decodes again, until no entry changes (at most lanes-of-the-chunk rounds);
//   count    two segmented scans turn the lanes' (markers passed, blocks completed, DC sums) into exclusive prefixes: each lane's
//            first block in scan order, the restart markers before it, the DC predictors it starts with;
//   strict   every lane decodes once more with the host decoder's rules and writes DC values and nonzero AC coefficients.
// The chunk's converged exit and totals carry into the next chunk.  The first error ends the walk; the extent is then zeroed again.
// The bit reader is the host's (64-bit accumulator, the same fill policy), so that its fill pointer -- which the host's restart
// rule looks at -- is part of the state where a restart interval is set.  A chunk's bytes (and 16 in front, 112 behind) are copied
// into LDS first: the reader's byte loads are a dependent chain, and from global memory one lane's fill stalls its whole wave.
// LDS holds that window (64.1 KB), the tables (8.5 KB), the zigzag order and per lane the exit state and the eight counts (40 KB);
// registers hold the reader and the lane's state.  No scratch, no global atomics, no spinning: block barriers only.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "jpeg_huff.h"

namespace tf2 {

namespace {

constexpr int kLookBits = 9;
constexpr uint32_t kNoErr = 0xFFFFFFFFu;
constexpr uint32_t kWinBack = 16, kWinAhead = 112;               // bytes of the window in front of and behind a chunk's subsequences
constexpr uint32_t kWinBytes = kHuffChunkBytes + kWinBack + kWinAhead;

struct HuffArgs {
  const uint8_t* bytes;
  unsigned long long bytes_len;
  const tf2_jpeg_scan* scan;
  const tf2_jpeg_src* jpeg;
  int16_t* coef;
  unsigned long long coef_blocks;
  uint8_t* work;
  unsigned long long slice;                      // bytes of an image's workspace slice (a multiple of 8)
  int32_t* status;
  int slog;                                      // log2 of subseq_bytes
  int lanes;                                     // subsequences of a chunk: jpeg_huff_chunk_lanes
  int nc, mx, my;                                // components, luma blocks of an MCU across and down
};

struct Tab {                                     // one Huffman table, as jpeg_entropy.cpp's Huff
  uint16_t look[1 << kLookBits];                 // (length << 8) | symbol for codes of at most kLookBits bits, 0: longer
  int32_t maxcode[17];                           // the largest code of length l, -1: none
  int32_t valoff[17];                            // valptr[l] - mincode[l]
  uint8_t vals[256];
};

struct Ctx {                                     // what a lane needs of its image (uniform over the workgroup)
  const uint8_t* d;                              // the entropy-coded data
  uint32_t len;
  const Tab* tabs;                               // [2 * comp + (AC ? 1 : 0)]
  const uint8_t* zz;
  int mcub, ylum, mx, my;                        // blocks of an MCU, luma blocks of an MCU
  bool same;                                     // every component has the same tables: the rounds leave the MCU phase out of the state
  uint32_t ri, rim;                              // restart interval in MCUs and in blocks
  uint32_t mcus_x, total;
  int16_t* coef;
  long long off0, off1, off2;
  int bw0;
  uint32_t cap;                                  // steps a lane can take at most
  const uint8_t* win;                            // LDS copy of d[w0 .. w0 + wn): the chunk's bytes and what its lanes look at beyond them
  uint32_t w0, wn;
};
// a byte of the data (i < len): out of the window where it is there
__device__ __forceinline__ uint32_t byte_at(const Ctx& c, uint32_t i) {
  const uint32_t r = i - c.w0;
  return r < c.wn ? c.win[r] : c.d[i];
}

// markers passed; blocks completed since the last one (or the entry); DC sums since then -- of the rounds: per block slot, counted
// from the entry's (after a marker: the MCU's) first block, a0..a5; of the strict pass: per component, a0..a2
struct Sum { uint32_t m, bs, a0, a1, a2, a3, a4, a5; };
__device__ __forceinline__ void add_at(Sum& s, int i, uint32_t v) {
  s.a0 += i == 0 ? v : 0u; s.a1 += i == 1 ? v : 0u; s.a2 += i == 2 ? v : 0u;
  s.a3 += i == 3 ? v : 0u; s.a4 += i == 4 ? v : 0u; s.a5 += i == 5 ? v : 0u;
}
__device__ __forceinline__ uint32_t get_at(const Sum& s, int i) {
  return i == 0 ? s.a0 : (i == 1 ? s.a1 : (i == 2 ? s.a2 : (i == 3 ? s.a3 : (i == 4 ? s.a4 : s.a5))));
}
__device__ __forceinline__ void clear(Sum& s) { s.a0 = s.a1 = s.a2 = s.a3 = s.a4 = s.a5 = 0; }

// The host's bit reader (jpeg_entropy.cpp's Bits) on the image's bytes.  `ff` remembers which of the last loaded bytes were stuffed
// pairs, so that the raw position of the next unread bit follows from p and have.
struct Bits {
  uint32_t p;
  uint64_t acc;
  int have;
  bool stop;
  uint32_t ff;
};

__device__ __forceinline__ void load1(const Ctx& c, Bits& b) {
  if (b.p >= c.len) { b.stop = true; return; }
  const uint32_t v = byte_at(c, b.p);
  if (v == 0xFF) {
    if (c.len - b.p < 2 || byte_at(c, b.p + 1) != 0) { b.stop = true; return; }
    b.p += 2;
    b.ff = (b.ff << 1) | 1u;
  } else {
    b.p++;
    b.ff <<= 1;
  }
  b.acc |= (uint64_t)v << (56 - b.have);
  b.have += 8;
}
__device__ __forceinline__ void fill(const Ctx& c, Bits& b) {
  // the common case at once: the n bytes the loop below would load lie in the window and none of them is FF
  const uint32_t r = b.p - c.w0;
  if (b.have <= 56 && !b.stop && r < c.wn && r + 12 <= kWinBytes) {
    const uint32_t n = (uint32_t)(64 - b.have) >> 3;              // 1..8
    if (c.wn - r >= n) {
      const uint32_t* const w = reinterpret_cast<const uint32_t*>(c.win + (r & ~3u));
      const uint32_t sh = (r & 3u) * 8u;
      const uint64_t lo = (uint64_t)w[0] | (uint64_t)w[1] << 32;
      const uint64_t le = sh ? (lo >> sh) | ((uint64_t)w[2] << (64u - sh)) : lo;   // bytes p .. p + 7, the first one lowest
      const uint64_t keep = n == 8 ? ~0ULL : (1ULL << (8 * n)) - 1ULL;
      const uint64_t y = ~le | ~keep;                             // a zero byte of y: one of the n bytes is FF
      if (((y - 0x0101010101010101ULL) & ~y & 0x8080808080808080ULL) == 0) {
        const uint64_t be = __builtin_bswap64(le & keep);         // the first byte highest, zeros behind the n-th
        b.acc |= be >> b.have;
        b.have += (int)(8 * n);
        b.p += n;
        b.ff <<= n;
        return;
      }
    }
  }
  while (b.have <= 56 && !b.stop) load1(c, b);
}
__device__ __forceinline__ uint32_t peek(const Bits& b, int n) { return (uint32_t)(b.acc >> (64 - n)); }   // 1 <= n <= 32
__device__ __forceinline__ bool take(Bits& b, int n) {
  if (n > b.have) return false;
  b.acc <<= n;
  b.have -= n;
  return true;
}
__device__ __forceinline__ void reset(Bits& b) { b.acc = 0; b.have = 0; b.stop = false; b.ff = 0; }

// state words: w0 = pc, the raw index behind the byte the next unread bit lies in (of that byte itself where none of it is read);
// w1 = rem | lead << 3 | blk << 7 | k << 10 | stopped << 16, rem the unread bits of that byte (0..7), lead the whole bytes loaded
// beyond it (0..8; kept only where a restart interval is set)
constexpr uint32_t kStopped = 1u << 16;
__device__ __forceinline__ void position(const Bits& b, bool track, uint32_t& pc, uint32_t& rem, uint32_t& lead) {
  const uint32_t whole = (uint32_t)b.have >> 3;
  rem = (uint32_t)b.have & 7u;
  pc = b.p - whole - (uint32_t)__popc(b.ff & ((1u << whole) - 1u));
  lead = track ? whole : 0u;
}
__device__ __forceinline__ void enter(const Ctx& c, Bits& b, uint32_t w0, uint32_t w1) {
  const uint32_t rem = w1 & 7u, lead = (w1 >> 3) & 15u;
  uint32_t start = w0;
  if (rem && start >= 1) start = (start >= 2 && byte_at(c, start - 1) == 0 && byte_at(c, start - 2) == 0xFF) ? start - 2 : start - 1;
  b.p = start;
  reset(b);
  const uint32_t n = lead + (rem ? 1u : 0u);
  for (uint32_t i = 0; i < n && !b.stop; i++) load1(c, b);
  if (rem && b.have >= 8) { b.acc <<= (8 - rem); b.have -= (int)(8 - rem); }
}

// one Huffman symbol: >= 0, -1: the bits ran out, -2: no code of the table
__device__ __forceinline__ int symbol(const Ctx& c, Bits& b, const Tab& t) {
  if (b.have < 16) fill(c, b);
  const uint32_t e = t.look[peek(b, kLookBits)];
  if (e) return take(b, (int)(e >> 8)) ? (int)(e & 0xFF) : -1;
  int l = kLookBits + 1;
  int32_t code = 0;
  for (; l <= 16; l++) {
    code = (int32_t)peek(b, l);
    if (code <= t.maxcode[l]) break;
  }
  if (l > 16) return -2;
  if (!take(b, l)) return -1;
  return t.vals[(t.valoff[l] + code) & 255];
}
__device__ __forceinline__ bool extend(const Ctx& c, Bits& b, int s, int32_t& v) {
  if (b.have < s) fill(c, b);
  const int32_t r = (int32_t)peek(b, s);
  if (!take(b, s)) return false;
  v = r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
  return true;
}

// the host decoder's block index of the g-th block of the scan (g < total)
__device__ __forceinline__ long long block_of(const Ctx& c, uint32_t g) {
  const uint32_t mcu = g / (uint32_t)c.mcub, bi = g - mcu * (uint32_t)c.mcub;
  const uint32_t r = mcu / c.mcus_x, q = mcu - r * c.mcus_x;
  if ((int)bi < c.ylum) {
    const uint32_t y = bi / (uint32_t)c.mx, x = bi - y * (uint32_t)c.mx;
    return c.off0 + (long long)(r * (uint32_t)c.my + y) * c.bw0 + (q * (uint32_t)c.mx + x);
  }
  return ((int)bi == c.ylum ? c.off1 : c.off2) + (long long)r * c.mcus_x + q;
}

// A lane: the steps that begin in front of raw byte `endkey` (last: all of them), from state (in0, in1).
// strict false: the tolerant rule; s receives the lane's counts, (out0, out1) its exit state.
// strict true: the host decoder's rule from the prefix s (markers, blocks and DC predictors before the lane), coefficients written;
// returns 0 or the status bit of the lane's first error.
__device__ __forceinline__ int lane(const Ctx& c, uint32_t in0, uint32_t in1, uint32_t endkey, bool last, bool strict, Sum& s, uint32_t& out0,
                    uint32_t& out1) {
  const bool track = c.ri != 0;
  if (!strict) s = Sum{0, 0, 0, 0, 0, 0, 0, 0};
  out0 = in0;
  out1 = in1;
  if (in1 & kStopped) return 0;
  Bits b;
  enter(c, b, in0, in1);
  int blk = (int)((in1 >> 7) & 7u), k = (int)((in1 >> 10) & 63u), slot = 0;
  const bool freeze = c.same && !strict;
  Sum w = s;
  uint32_t& m = w.m;
  uint32_t& bs = w.bs;
  if (strict) blk = (int)(bs % (uint32_t)c.mcub);                 // (the state's own where the phase is part of it)
  bool tol = !strict, stopped = false;
  int16_t* cur = nullptr;
  int err = 0;
  if (strict) {
    const unsigned long long g = (unsigned long long)m * c.rim + bs;
    if (g >= c.total) return 0;
    if (track && (bs > c.rim || (bs == c.rim && k != 0))) tol = true;   // behind an interval's end: as the rounds, to the marker
    else cur = c.coef + block_of(c, (uint32_t)g) * 64;
  }
  for (uint32_t it = 0; it < c.cap; it++) {
    uint32_t pc, rem, lead;
    position(b, track, pc, rem, lead);
    if (!last && pc - (rem ? 1u : 0u) >= endkey) break;
    if (!tol && k == 0) {
      const unsigned long long g = (unsigned long long)m * c.rim + bs;
      if (g >= c.total) break;
      if (track && bs == c.rim) {                                 // the host's restart rule: FF (fill FFs) D0 + n at the fill pointer
        uint32_t q = b.p;
        if (q >= c.len) { err = TF2_JPEG_TRUNCATED; break; }
        if (byte_at(c, q) != 0xFF) { err = TF2_JPEG_BAD_CODE; break; }
        while (q < c.len && byte_at(c, q) == 0xFF) q++;
        if (q >= c.len) { err = TF2_JPEG_TRUNCATED; break; }
        if (byte_at(c, q) != 0xD0 + (m & 7u)) { err = TF2_JPEG_BAD_CODE; break; }
        b.p = q + 1;
        reset(b);
        m++; bs = 0; clear(w); blk = 0;
        continue;
      }
      cur = c.coef + block_of(c, (uint32_t)g) * 64;
    }
    const int comp = blk < c.ylum ? 0 : blk - c.ylum + 1;
    bool nobits = false, endblock = false;
    const int sym = symbol(c, b, c.tabs[2 * comp + (k ? 1 : 0)]);
    if (sym == -1) {
      nobits = true;
    } else if (sym == -2) {
      if (!tol) { err = b.have < 16 ? TF2_JPEG_TRUNCATED : TF2_JPEG_BAD_CODE; break; }
      if (!take(b, 1)) nobits = true;                             // an unknown code skips one bit
    } else if (k == 0) {                                          // DC
      int sz = sym;
      if (sz > 15) {
        if (!tol) { err = TF2_JPEG_BAD_CODE; break; }
        sz = 15;
      }
      int32_t v = 0;
      if (sz && !extend(c, b, sz, v)) {
        nobits = true;
      } else {
        add_at(w, strict ? comp : slot, (uint32_t)v);
        if (!tol) cur[0] = (int16_t)(uint16_t)get_at(w, comp);
        k = 1;
      }
    } else {                                                      // AC
      const int r = sym >> 4, sz = sym & 15;
      if (sz == 0) {
        if (r == 15) {
          k += 16;
          if (k > 64 && !tol) { err = TF2_JPEG_BAD_CODE; break; }
          if (k >= 64) endblock = true;
        } else {
          endblock = true;
        }
      } else {
        k += r;
        if (k > 63) {
          if (!tol) { err = TF2_JPEG_BAD_CODE; break; }
          endblock = true;                                        // an overrun ends the block
        } else {
          int32_t v;
          if (!extend(c, b, sz, v)) {
            nobits = true;
          } else {
            if (!tol) cur[c.zz[k]] = (int16_t)(uint16_t)(uint32_t)v;
            if (++k >= 64) endblock = true;
          }
        }
      }
    }
    if (nobits) {
      if (!tol) { err = TF2_JPEG_TRUNCATED; break; }
      uint32_t q = b.p;                                           // (the reader stopped: a marker or the end stands at p)
      while (q < c.len && byte_at(c, q) == 0xFF) q++;
      if (q > b.p && q < c.len && (byte_at(c, q) & 0xF8) == 0xD0) {      // RSTn: step over it
        b.p = q + 1;
        reset(b);
        m++; bs = 0; clear(w); blk = 0; k = 0; slot = 0;
        if (strict) tol = false;
        continue;
      }
      stopped = true;
      break;
    }
    if (endblock) {
      k = 0;
      blk = freeze || blk + 1 == c.mcub ? 0 : blk + 1;
      slot = slot + 1 == c.mcub ? 0 : slot + 1;
      bs++;
    }
  }
  if (!strict) {
    uint32_t pc, rem, lead;
    position(b, track, pc, rem, lead);
    out0 = pc;
    out1 = rem | lead << 3 | (uint32_t)blk << 7 | (uint32_t)k << 10 | (stopped ? kStopped : 0u);
    s = w;
  }
  return err;
}

__device__ __forceinline__ void zero_extent(int16_t* coef, long long off, long long blocks) {
  uint4* const p = reinterpret_cast<uint4*>(coef + off * 64);
  for (long long i = threadIdx.x; i < blocks * 8; i += kHuffThreads) p[i] = uint4{0, 0, 0, 0};
}

__global__ __launch_bounds__(kHuffThreads) void jpeg_huff_kernel(HuffArgs a) {
  __shared__ Tab tabs[6];
  __shared__ uint8_t zz[64];
  __shared__ uint32_t ex0[kHuffThreads], ex1[kHuffThreads];
  __shared__ uint32_t sm[kHuffThreads], sb[kHuffThreads], sa[6][kHuffThreads];
  __shared__ __attribute__((aligned(16))) uint8_t win[kWinBytes];
  __shared__ uint32_t carry[8];                                   // the chain's state and totals in front of the chunk, rounds
  __shared__ uint32_t s_err;
  __shared__ int s_bad_table, s_differ;
  const int b = blockIdx.x, t = threadIdx.x;
  const tf2_jpeg_scan& sc = a.scan[b];
  const tf2_jpeg_src& j = a.jpeg[b];
  const long long off = sc.byte_off, len = sc.byte_len;
  const int ri = sc.restart_interval;

  // -- the tables (from the record alone) and their validity
  if (t == 0) { s_bad_table = 0; s_differ = 0; s_err = kNoErr; }
  __syncthreads();
  if (t < 2 * a.nc) {
    const uint8_t* const counts = (t & 1) ? sc.tab[t >> 1].ac_counts : sc.tab[t >> 1].dc_counts;
    const uint8_t* const vals = (t & 1) ? sc.tab[t >> 1].ac_vals : sc.tab[t >> 1].dc_vals;
    Tab& T = tabs[t];
    int n = 0;
    for (int l = 0; l < 16; l++) n += counts[l];
    bool ok = n <= 256;
    for (int i = 0; i < (1 << kLookBits); i++) T.look[i] = 0;
    int code = 0, k = 0;
    for (int l = 1; l <= 16 && ok; l++) {
      T.valoff[l] = k - code;
      const int cnt = counts[l - 1];
      for (int i = 0; i < cnt; i++, k++, code++) {
        if (code >= (1 << l)) { ok = false; break; }
        if (l <= kLookBits) {
          const int first = code << (kLookBits - l);
          const uint16_t e = (uint16_t)((l << 8) | vals[k]);
          for (int q = 0; q < (1 << (kLookBits - l)); q++) T.look[first + q] = e;
        }
      }
      T.maxcode[l] = cnt ? code - 1 : -1;
      code <<= 1;
    }
    for (int i = 0; i < 256; i++) T.vals[i] = vals[i];
    if (!ok) s_bad_table = 1;
  }
  if (a.nc == 3) {                                                // do the components share their tables?
    const uint8_t* const t0 = sc.tab[0].dc_counts;
    for (int i = t; i < (int)sizeof(sc.tab[0]); i += kHuffThreads)
      if (t0[i] != sc.tab[1].dc_counts[i] || t0[i] != sc.tab[2].dc_counts[i]) s_differ = 1;
  }
  if (t < 64) {
    // the natural index of the t-th coefficient of the zigzag sequence, from its closed form (no table in constant memory)
    int x = 0, y = 0;
    for (int i = 0; i < t; i++) {
      if (((x + y) & 1) == 0) { if (x == 7) y++; else if (y == 0) x++; else { x++; y--; } }
      else { if (y == 7) x++; else if (x == 0) y++; else { x--; y++; } }
    }
    zz[t] = (uint8_t)(8 * y + x);
  }
  __syncthreads();

  // -- the records
  int st = 0;
  const int mcub = a.nc == 1 ? 1 : a.mx * a.my + 2;
  if (off < 0 || len < 0 || len > TF2_JPEG_HUFF_MAX_BYTES || (unsigned long long)off > a.bytes_len ||
      (unsigned long long)len > a.bytes_len - (unsigned long long)off)
    st |= TF2_JPEG_REC_BAD_RANGE;
  if (sc.components != a.nc || sc.sub_x != a.mx || sc.sub_y != a.my || ri < 0 || ri > 65535) st |= TF2_JPEG_REC_BAD_SCAN;
  if (s_bad_table) st |= TF2_JPEG_REC_BAD_TABLE;
  uint32_t N = 1;
  if (!(st & TF2_JPEG_REC_BAD_RANGE)) {
    N = (uint32_t)((len + (1LL << a.slog) - 1) >> a.slog);
    if (N < 1) N = 1;
    if ((unsigned long long)kHuffWorkHeader + 8ULL * N > a.slice) st |= TF2_JPEG_REC_WORK_TOO_SMALL;
  }
  for (int c = 0; c < a.nc; c++) {
    if (j.bw[c] < 1 || j.bh[c] < 1 || j.bw[c] > 8192 || j.bh[c] > 8192) st |= TF2_JPEG_REC_BAD_GRID;
    if (j.block_off[c] < 0) st |= TF2_JPEG_REC_BAD_OFFSET;
  }
  if (!(st & TF2_JPEG_REC_BAD_GRID)) {
    if (j.bw[0] % a.mx || j.bh[0] % a.my) st |= TF2_JPEG_REC_BAD_GRID;
    else if (a.nc == 3 && (j.bw[1] != j.bw[0] / a.mx || j.bw[2] != j.bw[1] || j.bh[1] != j.bh[0] / a.my || j.bh[2] != j.bh[1]))
      st |= TF2_JPEG_REC_BAD_GRID;
  }
  if (!(st & (TF2_JPEG_REC_BAD_GRID | TF2_JPEG_REC_BAD_OFFSET))) {
    for (int c = 0; c < a.nc; c++) {
      const unsigned long long o = (unsigned long long)j.block_off[c], n = (unsigned long long)((long long)j.bw[c] * j.bh[c]);
      if (o > a.coef_blocks || n > a.coef_blocks - o) st |= TF2_JPEG_REC_OUT_OF_COEF;
    }
  }
  if (st != 0) {                                                  // (the whole workgroup: nothing of the image is read or written)
    if (t == 0) a.status[b] = st;
    return;
  }

  Ctx c;
  c.d = a.bytes + off;
  c.len = (uint32_t)len;
  c.tabs = tabs;
  c.zz = zz;
  c.mcub = mcub;
  c.ylum = a.nc == 1 ? 1 : a.mx * a.my;
  c.same = a.nc == 3 && !s_differ;
  c.mx = a.nc == 1 ? 1 : a.mx;
  c.my = a.nc == 1 ? 1 : a.my;
  c.ri = (uint32_t)ri;
  c.rim = (uint32_t)ri * (uint32_t)mcub;
  c.mcus_x = (uint32_t)(j.bw[0] / c.mx);
  c.total = c.mcus_x * (uint32_t)(j.bh[0] / c.my) * (uint32_t)mcub;
  c.coef = a.coef;
  c.off0 = j.block_off[0];
  c.off1 = a.nc == 3 ? j.block_off[1] : 0;
  c.off2 = a.nc == 3 ? j.block_off[2] : 0;
  c.bw0 = j.bw[0];
  c.cap = 9u * c.len + 64u;
  c.win = win;
  c.w0 = 0;
  c.wn = 0;

  for (int k = 0; k < a.nc; k++) zero_extent(a.coef, j.block_off[k], (long long)j.bw[k] * j.bh[k]);
  if (t < 8) carry[t] = 0;
  __syncthreads();

  uint32_t* const wk = reinterpret_cast<uint32_t*>(a.work + (unsigned long long)b * a.slice);
  const uint32_t S = 1u << a.slog, L = (uint32_t)a.lanes, chunks = (N + L - 1) / L;
  for (uint32_t chunk = 0; chunk < chunks; chunk++) {
    const uint32_t first = chunk * L, nl = N - first < L ? N - first : L;
    const uint32_t s = first + t;
    const bool active = (uint32_t)t < nl, last = s == N - 1;
    const uint32_t endkey = (s + 1) * S;
    {                                                             // the chunk's bytes into LDS (the barrier behind the last chunk's strict pass is in front)
      const uint32_t lo = first * S > kWinBack ? first * S - kWinBack : 0u;
      const uint32_t hi = (first + nl) * S + kWinAhead < c.len ? (first + nl) * S + kWinAhead : c.len;
      c.wn = 0;                                                   // (while it is filled, and for the reads below)
      for (uint32_t i = t; lo + i < hi; i += 8 * kHuffThreads) {
        uint8_t v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = lo + i + q * kHuffThreads < hi ? c.d[lo + i + q * kHuffThreads] : (uint8_t)0;
#pragma unroll
        for (int q = 0; q < 8; q++)
          if (lo + i + q * kHuffThreads < hi) win[i + q * kHuffThreads] = v[q];
      }
      __syncthreads();
      c.w0 = lo;
      c.wn = hi - lo;
    }
    uint32_t in0 = 0, in1 = 0;
    Sum sum{0, 0, 0, 0, 0, 0, 0, 0};
    if (active) {
      if (t == 0) {
        in0 = carry[0];
        in1 = carry[1];
      } else {                                                    // the subsequence's first bit, behind the 00 of a stuffed pair
        in0 = s * S;
        if (byte_at(c, in0) == 0 && byte_at(c, in0 - 1) == 0xFF) in0++;
      }
      lane(c, in0, in1, endkey, last, false, sum, ex0[t], ex1[t]);
      sm[t] = sum.m; sb[t] = sum.bs;
      sa[0][t] = sum.a0; sa[1][t] = sum.a1; sa[2][t] = sum.a2; sa[3][t] = sum.a3; sa[4][t] = sum.a4; sa[5][t] = sum.a5;
    }
    __syncthreads();
    uint32_t rounds = 1;
    for (uint32_t r = 1; r < nl; r++) {
      uint32_t n0 = in0, n1 = in1;
      if (active && t > 0) { n0 = ex0[t - 1]; n1 = ex1[t - 1]; }
      const bool changed = n0 != in0 || n1 != in1;
      if (!__syncthreads_or(changed ? 1 : 0)) break;
      rounds++;
      if (changed) {
        in0 = n0;
        in1 = n1;
        lane(c, in0, in1, endkey, last, false, sum, ex0[t], ex1[t]);
        sm[t] = sum.m; sb[t] = sum.bs;
        sa[0][t] = sum.a0; sa[1][t] = sum.a1; sa[2][t] = sum.a2; sa[3][t] = sum.a3; sa[4][t] = sum.a4; sa[5][t] = sum.a5;
      }
      __syncthreads();
    }
    // exclusive prefixes of the counts (two segmented scans over the lanes, Hillis-Steele in LDS) and the chunk's carry.
    // (m, bs): markers add; blocks add up to a lane that passed a marker, which starts them again.
    uint32_t im = sum.m, ib = sum.bs;                             // inclusive, in sm / sb
    for (uint32_t off = 1; off < nl; off <<= 1) {
      const bool has = active && (uint32_t)t >= off;
      uint32_t pm = 0, pb = 0;
      if (has) { pm = sm[t - off]; pb = sb[t - off]; }
      __syncthreads();
      if (has) {
        ib = im ? ib : pb + ib;
        im += pm;
        sm[t] = im; sb[t] = ib;
      }
      __syncthreads();
    }
    uint32_t em = carry[2], eb = carry[3];                        // exclusive, the carry in front
    if (active && t > 0) {
      const uint32_t pm = sm[t - 1], pb = sb[t - 1];
      eb = pm ? pb : eb + pb;
      em += pm;
    }
    // the DC sums per component: the lane's slots start at block eb of the MCU (at its first block behind a marker)
    uint32_t f = sum.m ? 1u : 0u, l0 = 0, l1 = 0, l2 = 0;
    {
      uint32_t phase = f ? 0u : eb % (uint32_t)mcub;
#pragma unroll
      for (int q = 0; q < 6; q++) {
        const uint32_t v = q < mcub ? get_at(sum, q) : 0u;
        if ((int)phase < c.ylum) l0 += v; else if ((int)phase == c.ylum) l1 += v; else l2 += v;
        phase = (int)phase + 1 == mcub ? 0u : phase + 1;
      }
    }
    __syncthreads();                                              // (sm, sb read above)
    if (active) { sa[0][t] = f; sa[1][t] = l0; sa[2][t] = l1; sa[3][t] = l2; }
    __syncthreads();
    for (uint32_t off = 1; off < nl; off <<= 1) {
      const bool has = active && (uint32_t)t >= off;
      uint32_t pf = 0, p0 = 0, p1 = 0, p2 = 0;
      if (has) { pf = sa[0][t - off]; p0 = sa[1][t - off]; p1 = sa[2][t - off]; p2 = sa[3][t - off]; }
      __syncthreads();
      if (has) {
        if (!f) { l0 += p0; l1 += p1; l2 += p2; }
        f |= pf;
        sa[0][t] = f; sa[1][t] = l0; sa[2][t] = l1; sa[3][t] = l2;
      }
      __syncthreads();
    }
    uint32_t e0 = carry[4], e1 = carry[5], e2 = carry[6];
    if (active && t > 0) {
      const uint32_t pf = sa[0][t - 1], p0 = sa[1][t - 1], p1 = sa[2][t - 1], p2 = sa[3][t - 1];
      e0 = pf ? p0 : e0 + p0;
      e1 = pf ? p1 : e1 + p1;
      e2 = pf ? p2 : e2 + p2;
    }
    __syncthreads();                                              // (carry read above)
    if ((uint32_t)t == nl - 1) {                                  // the chunk's totals, the carry in front
      carry[0] = ex0[t]; carry[1] = ex1[t];
      carry[2] = carry[2] + im; carry[3] = im ? ib : carry[3] + ib;
      carry[4] = f ? l0 : carry[4] + l0; carry[5] = f ? l1 : carry[5] + l1; carry[6] = f ? l2 : carry[6] + l2;
      carry[7] += rounds;
    }
    __syncthreads();
    if (active) {
      sum = Sum{em, eb, e0, e1, e2, 0, 0, 0};
      uint32_t o0, o1;
      const int err = lane(c, in0, in1, endkey, last, true, sum, o0, o1);
      if (err) atomicMin(&s_err, (uint32_t)t << 10 | (uint32_t)err);
      wk[4 + 2 * s] = ex0[t];
      wk[5 + 2 * s] = ex1[t];
    }
    __syncthreads();
    if (s_err != kNoErr) break;
  }
  const int err = s_err == kNoErr ? 0 : (int)(s_err & 1023u);
  if (err)
    for (int k = 0; k < a.nc; k++) zero_extent(a.coef, j.block_off[k], (long long)j.bw[k] * j.bh[k]);
  if (t == 0) {
    a.status[b] = err;
    wk[0] = carry[7]; wk[1] = N; wk[2] = 0; wk[3] = 0;
  }
}

int huff_slog(const tf2_jpeg_huff_desc* d) {
  const int s = d->subseq_bytes ? d->subseq_bytes : TF2_JPEG_HUFF_DEFAULT_SUBSEQ;
  for (int l = 4; l <= 8; l++)
    if (s == (1 << l)) return l;
  return -1;
}

}  // namespace

size_t jpeg_huff_work_bytes(const tf2_jpeg_huff_desc* d, int batch, size_t max_scan_bytes) {
  if (!d || d->size != sizeof(tf2_jpeg_huff_desc) || batch < 1 || huff_slog(d) < 0) return 0;
  const int l = huff_slog(d);
  size_t n = (max_scan_bytes >> l) + ((max_scan_bytes & (((size_t)1 << l) - 1)) ? 1 : 0);
  if (n < 1) n = 1;
  return (size_t)batch * (kHuffWorkHeader + 8 * n);
}

tf2_status jpeg_huff(const tf2_jpeg_huff_desc* d, const uint8_t* bytes, size_t bytes_len, const tf2_jpeg_scan* scan,
                     const tf2_jpeg_src* jpeg, int16_t* coef, size_t coef_blocks, uint8_t* work, size_t work_bytes, int batch,
                     int32_t* status, void* stream) {
  auto refuse = [](const std::string& m) { return arg_refusal("tf2_jpeg_huff", m); };
  if (!d) return refuse("null desc");
  if (d->size != sizeof(tf2_jpeg_huff_desc)) return refuse("desc size " + std::to_string(d->size) + ", expected sizeof(tf2_jpeg_huff_desc)");
  if (d->layout != TF2_YCC_PLANAR && d->layout != TF2_YCC_GRAY) return refuse("layout must be TF2_YCC_PLANAR or TF2_YCC_GRAY");
  const bool gray = d->layout == TF2_YCC_GRAY;
  if (!gray && !((d->sub_x == 1 && d->sub_y == 1) || (d->sub_x == 2 && d->sub_y == 1) || (d->sub_x == 2 && d->sub_y == 2)))
    return refuse("(sub_x, sub_y) must be (1,1), (2,1) or (2,2)");
  if (huff_slog(d) < 0) return refuse("subseq_bytes must be 0, 16, 32, 64, 128 or 256");
  if (batch < 1) return refuse("batch must be >= 1");
  if (!bytes || !scan || !jpeg || !coef || !work || !status) return refuse("null device pointer");
  if ((uintptr_t)coef & 15) return refuse("coef_dev must be 16-byte aligned");
  if ((uintptr_t)work & 7) return refuse("work_dev must be 8-byte aligned");
  if (coef_blocks > (SIZE_MAX >> 7)) return refuse("coef_blocks * 128 wraps");
  if (work_bytes < jpeg_huff_work_bytes(d, batch, 0)) return refuse("work_bytes below tf2_jpeg_huff_work_bytes(d, batch, 0)");
  {
    const uintptr_t at[4] = {(uintptr_t)bytes, (uintptr_t)coef, (uintptr_t)work, (uintptr_t)status};
    const size_t n[4] = {bytes_len, coef_blocks * 128, work_bytes, (size_t)batch * sizeof(int32_t)};
    const char* const name[4] = {"byte", "coefficient", "workspace", "status"};
    for (int i = 0; i < 4; i++)
      if (n[i] > UINTPTR_MAX - at[i]) return refuse("a buffer wraps the address space");
    for (int i = 0; i < 4; i++)
      for (int k = i + 1; k < 4; k++)
        if (at[i] < at[k] + n[k] && at[k] < at[i] + n[i])
          return refuse(std::string("the ") + name[i] + " and the " + name[k] + " buffer overlap");
  }

  HuffArgs a{};
  a.bytes = bytes; a.bytes_len = bytes_len; a.scan = scan; a.jpeg = jpeg; a.coef = coef; a.coef_blocks = coef_blocks;
  a.work = work; a.slice = (work_bytes / (size_t)batch) & ~(size_t)7; a.status = status;
  a.slog = huff_slog(d);
  a.nc = gray ? 1 : 3;
  a.mx = gray ? 1 : d->sub_x;
  a.my = gray ? 1 : d->sub_y;
  a.lanes = jpeg_huff_chunk_lanes(1 << a.slog);
  hipLaunchKernelGGL(jpeg_huff_kernel, dim3((unsigned)batch), dim3(kHuffThreads), 0, (hipStream_t)stream, a);
  return launch_result("tf2_jpeg_huff");
}

}  // namespace tf2
