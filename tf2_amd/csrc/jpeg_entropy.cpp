// jpeg_entropy.cpp -- the serial part of a baseline JPEG decoder, on the host (tf2_jpeg_parse, tf2_jpeg_entropy, tf2_jpeg_scan_fill, include/tf2_amd.h):
// the headers, and the Huffman-coded scan into dense blocks of 64 int16 coefficients in natural order that tf2_jpeg_idct
// (jpeg_idct.hip) dequantises and transforms on the device.  Host only: no device call, no global state, no tf2_last_error -- both
// entry points may run on many threads at once.  The file needs nothing but the public header, so that it also builds alone
// (tests/native/jpeg_fuzz_main.cpp runs it under the host sanitizers).
//
// Every read of the file goes through a bounds test against `bytes`; every write of a coefficient goes to a block index below
// info->total_blocks, which the caller's capacity was tested against.  Huffman decoding is table driven: kLookBits bits index a table
// of (length, symbol) for the codes that short, and the longer codes (rare: an encoder gives them to rare symbols) walk the canonical
// maxcode list from kLookBits + 1 on.
#include <cstdint>
#include <cstring>
#include "../../include/tf2_amd.h"

namespace {

constexpr int kLookBits = 9;

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool defined = false;
  uint8_t counts[16];               // as the DHT segment gives them (tf2_jpeg_scan_fill copies them out)
  uint8_t vals[256];
  int32_t maxcode[17];              // the largest code of length l, -1: none
  int32_t valptr[17], mincode[17];
  uint16_t look[1 << kLookBits];    // (length << 8) | symbol for codes of at most kLookBits bits, 0: longer
};

struct Comp { int id, hs, vs, tq, td, ta; };

struct Header {
  tf2_jpeg_info info;
  Comp comp[4];
  Huff dc[4], ac[4];
};

// counts[1..16], the symbols in code order -> the tables; false: more than 256 symbols or codes that do not fit their lengths
bool build_huff(Huff& t, const uint8_t* counts, const uint8_t* vals, int n) {
  int code = 0, k = 0;
  std::memset(t.look, 0, sizeof t.look);
  for (int l = 1; l <= 16; l++) {
    t.valptr[l] = k;
    t.mincode[l] = code;
    for (int i = 0; i < counts[l - 1]; i++, k++, code++) {
      if (code >= (1 << l)) return false;
      if (l <= kLookBits) {
        const int first = code << (kLookBits - l);
        for (int j = 0; j < (1 << (kLookBits - l)); j++) t.look[first + j] = (uint16_t)((l << 8) | vals[k]);
      }
    }
    t.maxcode[l] = counts[l - 1] ? code - 1 : -1;
    code <<= 1;
  }
  std::memset(t.vals, 0, sizeof t.vals);
  std::memcpy(t.vals, vals, (size_t)n);
  std::memcpy(t.counts, counts, 16);
  t.defined = true;
  return k == n;
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// the headers up to and including SOS; fills H.info whole (status included)
void parse_headers(const uint8_t* f, size_t n, Header& H) {
  tf2_jpeg_info& I = H.info;
  std::memset(&I, 0, sizeof I);
  uint16_t qt[4][64];
  bool qdef[4] = {false, false, false, false};
  bool jfif = false, adobe = false, sof = false;
  int adobe_transform = 0, ncomp = 0;
  int st = 0;
  auto fail = [&](int bits) { I.status = st | bits; };
  if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return fail(TF2_JPEG_BAD_HEADER);
  size_t p = 2;
  for (;;) {
    if (p >= n) return fail(TF2_JPEG_BAD_HEADER);
    if (f[p] != 0xFF) return fail(TF2_JPEG_BAD_HEADER);
    while (p < n && f[p] == 0xFF) p++;                            // fill bytes
    if (p >= n) return fail(TF2_JPEG_BAD_HEADER);
    const int m = f[p++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;          // TEM, RSTn: no segment
    if (m == 0xD8 || m == 0xD9 || m == 0x00) return fail(TF2_JPEG_BAD_HEADER);
    if (n - p < 2) return fail(TF2_JPEG_BAD_HEADER);
    const int len = be16(f + p);
    if (len < 2 || (size_t)len > n - p) return fail(TF2_JPEG_BAD_HEADER);
    const uint8_t* s = f + p + 2;
    const int sl = len - 2;
    p += (size_t)len;
    if (m == 0xDB) {                                              // DQT
      int at = 0;
      while (at < sl) {
        const int pq = s[at] >> 4, tq = s[at] & 15;
        at++;
        if (pq > 1 || tq > 3 || sl - at < 64 * (pq + 1)) return fail(TF2_JPEG_BAD_HEADER);
        for (int k = 0; k < 64; k++) qt[tq][kZigzag[k]] = (uint16_t)(pq ? be16(s + at + 2 * k) : s[at + k]);
        at += 64 * (pq + 1);
        qdef[tq] = true;
      }
    } else if (m == 0xC4) {                                       // DHT
      int at = 0;
      while (at < sl) {
        const int tc = s[at] >> 4, th = s[at] & 15;
        at++;
        if (tc > 1 || th > 3 || sl - at < 16) return fail(TF2_JPEG_BAD_HEADER);
        int cnt = 0;
        for (int i = 0; i < 16; i++) cnt += s[at + i];
        if (cnt > 256 || sl - at - 16 < cnt) return fail(TF2_JPEG_BAD_HEADER);
        if (!build_huff(tc ? H.ac[th] : H.dc[th], s + at, s + at + 16, cnt)) return fail(TF2_JPEG_BAD_HEADER);
        at += 16 + cnt;
      }
    } else if (m == 0xCC) {                                       // DAC
      st |= TF2_JPEG_UNSUPPORTED_ARITHMETIC;
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8) {             // SOFn (0xC4 and 0xCC are taken above; 0xC8 is JPG, skipped)
      if (sof) return fail(TF2_JPEG_BAD_HEADER);
      sof = true;
      if (m >= 0xC9) st |= TF2_JPEG_UNSUPPORTED_ARITHMETIC;
      else if (m >= 0xC2) st |= TF2_JPEG_UNSUPPORTED_PROGRESSIVE;
      if (sl < 6) return fail(TF2_JPEG_BAD_HEADER);
      if (s[0] != 8) st |= TF2_JPEG_UNSUPPORTED_PRECISION;
      I.h = be16(s + 1);
      I.w = be16(s + 3);
      ncomp = s[5];
      if (I.h < 1 || I.w < 1 || ncomp < 1 || sl != 6 + 3 * ncomp) return fail(TF2_JPEG_BAD_HEADER);
      if (ncomp != 1 && ncomp != 3) { st |= TF2_JPEG_UNSUPPORTED_COMPONENTS; if (ncomp > 4) return fail(0); }
      for (int c = 0; c < ncomp; c++) {
        Comp& k = H.comp[c];
        k.id = s[6 + 3 * c];
        k.hs = s[7 + 3 * c] >> 4;
        k.vs = s[7 + 3 * c] & 15;
        k.tq = s[8 + 3 * c];
        if (k.hs < 1 || k.hs > 4 || k.vs < 1 || k.vs > 4 || k.tq > 3) return fail(TF2_JPEG_BAD_HEADER);
      }
    } else if (m == 0xDD) {                                       // DRI
      if (sl != 2) return fail(TF2_JPEG_BAD_HEADER);
      I.restart_interval = be16(s);
    } else if (m == 0xE0) {
      if (sl >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
    } else if (m == 0xDA) {                                       // SOS: the header ends here
      if (!sof) return fail(TF2_JPEG_BAD_HEADER);
      if (sl < 1) return fail(TF2_JPEG_BAD_HEADER);
      const int ns = s[0];
      if (ns < 1 || ns > 4 || sl != 4 + 2 * ns) return fail(TF2_JPEG_BAD_HEADER);
      if (ns != ncomp) st |= TF2_JPEG_UNSUPPORTED_SCANS;
      if (st) break;                                              // (a file that is refused anyway: its scan header is not judged)
      for (int c = 0; c < ncomp; c++) {                           // the components in the frame's order
        Comp& k = H.comp[c];
        if (s[1 + 2 * c] != k.id) return fail(TF2_JPEG_BAD_HEADER);
        k.td = s[2 + 2 * c] >> 4;
        k.ta = s[2 + 2 * c] & 15;
        if (k.td > 3 || k.ta > 3 || !H.dc[k.td].defined || !H.ac[k.ta].defined || !qdef[k.tq]) return fail(TF2_JPEG_BAD_HEADER);
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return fail(TF2_JPEG_BAD_HEADER);
      break;
    }                                                             // every other segment (APPn, COM, ...) is skipped
  }
  // -- what the frame is
  if (st && ncomp != 3) return fail(0);
  if (ncomp == 3) {
    const Comp *y = &H.comp[0], *cb = &H.comp[1], *cr = &H.comp[2];
    const bool rgb = jfif ? false : (adobe ? adobe_transform == 0 : (y->id == 'R' && cb->id == 'G' && cr->id == 'B'));
    if (rgb) st |= TF2_JPEG_UNSUPPORTED_COLORSPACE;
    const bool luma_ok = (y->hs == 1 && y->vs == 1) || (y->hs == 2 && y->vs == 1) || (y->hs == 2 && y->vs == 2);
    if (!luma_ok || cb->hs != 1 || cb->vs != 1 || cr->hs != 1 || cr->vs != 1) st |= TF2_JPEG_UNSUPPORTED_SAMPLING;
    if (st) return fail(0);
    I.sub_x = y->hs;
    I.sub_y = y->vs;
    const int mw = (I.w + 8 * I.sub_x - 1) / (8 * I.sub_x), mh = (I.h + 8 * I.sub_y - 1) / (8 * I.sub_y);
    for (int c = 0; c < 3; c++) {
      I.bw[c] = mw * H.comp[c].hs;
      I.bh[c] = mh * H.comp[c].vs;
      I.ph[c] = c ? (I.h + I.sub_y - 1) / I.sub_y : I.h;
      I.pw[c] = c ? (I.w + I.sub_x - 1) / I.sub_x : I.w;
    }
  } else {
    I.sub_x = I.sub_y = 1;
    I.bw[0] = (I.w + 7) / 8;
    I.bh[0] = (I.h + 7) / 8;
    I.ph[0] = I.h;
    I.pw[0] = I.w;
  }
  I.components = ncomp;
  I.total_blocks = 0;
  for (int c = 0; c < ncomp; c++) {
    I.total_blocks += (int64_t)I.bw[c] * I.bh[c];
    std::memcpy(I.quant[c], qt[H.comp[c].tq], sizeof qt[0]);
  }
  I.upsample = (ncomp == 3 && I.sub_x > 1 && I.pw[1] <= 2) ? TF2_YCC_REPLICATE : TF2_YCC_FANCY;
  I.scan_offset = (int64_t)p;
  I.status = 0;
}

// The bits of the scan.  `acc` holds `have` valid bits at its top; fill() appends whole bytes until a marker or the end of the file
// stands in the way (a stuffed FF 00 is the byte FF).  peek() reads past the valid bits as zeros; take() is refused beyond them.
struct Bits {
  const uint8_t *p, *end;
  uint64_t acc = 0;
  int have = 0;
  bool stop = false;                // a marker or the end reached: no more bytes
  void fill() {
    while (have <= 56 && !stop) {
      if (p >= end) { stop = true; break; }
      uint32_t b = *p;
      if (b == 0xFF) {
        if (end - p < 2) { stop = true; break; }
        if (p[1] != 0) { stop = true; break; }
        p += 2;
      } else {
        p++;
      }
      acc |= (uint64_t)b << (56 - have);
      have += 8;
    }
  }
  uint32_t peek(int n) const { return (uint32_t)(acc >> (64 - n)); }          // 1 <= n <= 32
  bool take(int n) {
    if (n > have) return false;
    acc <<= n;
    have -= n;
    return true;
  }
  void reset() { acc = 0; have = 0; stop = false; }
};

// one Huffman symbol: >= 0, or -TF2_JPEG_TRUNCATED / -TF2_JPEG_BAD_CODE
inline int symbol(Bits& b, const Huff& t) {
  if (b.have < 16) b.fill();
  const uint32_t e = t.look[b.peek(kLookBits)];
  if (e) {
    if (!b.take((int)(e >> 8))) return -TF2_JPEG_TRUNCATED;
    return (int)(e & 0xFF);
  }
  int l = kLookBits + 1;
  int32_t code = 0;
  for (; l <= 16; l++) {
    code = (int32_t)b.peek(l);
    if (code <= t.maxcode[l]) break;
  }
  if (l > 16) return b.have < 16 ? -TF2_JPEG_TRUNCATED : -TF2_JPEG_BAD_CODE;
  if (!b.take(l)) return -TF2_JPEG_TRUNCATED;
  return t.vals[t.valptr[l] + (code - t.mincode[l])];
}

// s extra bits as the signed value of category s (1 <= s <= 15); false: truncated
inline bool receive_extend(Bits& b, int s, int32_t& v) {
  if (b.have < s) b.fill();
  const int32_t r = (int32_t)b.peek(s);
  if (!b.take(s)) return false;
  v = r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
  return true;
}

// one block into out[64] (zeroed by the caller); 0 or a status bit
inline int decode_block(Bits& b, const Huff& dc, const Huff& ac, int32_t& pred, int16_t* out) {
  int s = symbol(b, dc);
  if (s < 0) return -s;
  if (s > 15) return TF2_JPEG_BAD_CODE;
  if (s) {
    int32_t v;
    if (!receive_extend(b, s, v)) return TF2_JPEG_TRUNCATED;
    pred = (int32_t)((uint32_t)pred + (uint32_t)v);
  }
  out[0] = (int16_t)(uint16_t)(uint32_t)pred;
  for (int k = 1; k < 64;) {
    const int rs = symbol(b, ac);
    if (rs < 0) return -rs;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r == 15) { k += 16; if (k > 64) return TF2_JPEG_BAD_CODE; continue; }
      break;                                                      // EOB (a run length below 15 with size 0 ends the block too)
    }
    k += r;
    if (k > 63) return TF2_JPEG_BAD_CODE;
    int32_t v;
    if (!receive_extend(b, s, v)) return TF2_JPEG_TRUNCATED;
    out[kZigzag[k]] = (int16_t)(uint16_t)(uint32_t)v;
    k++;
  }
  return 0;
}

}  // namespace

extern "C" {

tf2_status tf2_jpeg_parse(const uint8_t* file, size_t bytes, tf2_jpeg_info* info) {
  if (!file || !info) return TF2_ERR_ARG;
  Header H;
  parse_headers(file, bytes, H);
  *info = H.info;
  return TF2_OK;
}

tf2_status tf2_jpeg_entropy(const uint8_t* file, size_t bytes, const tf2_jpeg_info* info, int16_t* coef, size_t capacity_blocks,
                            int32_t* status) {
  if (!file || !info || !coef || !status) return TF2_ERR_ARG;
  if (info->status != 0 || info->total_blocks < 1) return TF2_ERR_ARG;
  if (capacity_blocks < (uint64_t)info->total_blocks) return TF2_ERR_SIZE;
  std::memset(coef, 0, (size_t)info->total_blocks * 64 * sizeof(int16_t));
  Header H;
  parse_headers(file, bytes, H);
  const tf2_jpeg_info& I = H.info;
  if (I.status != 0) { *status = I.status; return TF2_OK; }
  bool same = I.h == info->h && I.w == info->w && I.components == info->components && I.total_blocks == info->total_blocks;
  for (int c = 0; c < 3; c++) same = same && I.bw[c] == info->bw[c] && I.bh[c] == info->bh[c];
  if (!same) { *status = TF2_JPEG_BAD_HEADER; return TF2_OK; }

  Bits b;
  b.p = file + (size_t)I.scan_offset;
  b.end = file + bytes;
  const int nc = I.components;
  const int mx = nc == 1 ? 1 : I.sub_x, my = nc == 1 ? 1 : I.sub_y;   // luma blocks of an MCU; chroma has one
  const int mcus_x = I.bw[0] / mx, mcus_y = I.bh[0] / my;
  int64_t base[3] = {0, (int64_t)I.bw[0] * I.bh[0], (int64_t)I.bw[0] * I.bh[0] + (int64_t)I.bw[1] * I.bh[1]};
  int32_t pred[3] = {0, 0, 0};
  int left = I.restart_interval, next_rst = 0;
  int st = 0;
  for (int r = 0; r < mcus_y && !st; r++) {
    for (int q = 0; q < mcus_x && !st; q++) {
      if (I.restart_interval && left == 0) {                      // a restart marker stands here: FF (fill FFs) D0 + n
        const uint8_t* p = b.p;                                   // (fill() never steps over a marker, so it is at or behind b.p)
        if (p >= b.end) { st = TF2_JPEG_TRUNCATED; break; }
        if (*p != 0xFF) { st = TF2_JPEG_BAD_CODE; break; }
        while (p < b.end && *p == 0xFF) p++;
        if (p >= b.end) { st = TF2_JPEG_TRUNCATED; break; }
        if (*p != 0xD0 + next_rst) { st = TF2_JPEG_BAD_CODE; break; }
        b.p = p + 1;
        b.reset();
        next_rst = (next_rst + 1) & 7;
        left = I.restart_interval;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < nc && !st; c++) {
        const int nx = c ? 1 : mx, ny = c ? 1 : my;
        const Huff &dc = H.dc[H.comp[c].td], &ac = H.ac[H.comp[c].ta];
        for (int y = 0; y < ny && !st; y++)
          for (int x = 0; x < nx && !st; x++) {
            const int64_t blk = base[c] + (int64_t)(r * ny + y) * I.bw[c] + (q * nx + x);
            st = decode_block(b, dc, ac, pred[c], coef + blk * 64);
          }
      }
      left--;
    }
  }
  *status = st;
  return TF2_OK;
}

tf2_status tf2_jpeg_scan_fill(const uint8_t* file, size_t bytes, const tf2_jpeg_info* info, int64_t byte_off, tf2_jpeg_scan* out) {
  if (!file || !info || !out) return TF2_ERR_ARG;
  if (info->status != 0 || info->total_blocks < 1) return TF2_ERR_ARG;
  Header H;
  parse_headers(file, bytes, H);
  const tf2_jpeg_info& I = H.info;
  bool same = I.status == 0 && I.h == info->h && I.w == info->w && I.components == info->components &&
              I.total_blocks == info->total_blocks && I.scan_offset == info->scan_offset;
  if (!same || I.scan_offset < 0 || (uint64_t)I.scan_offset > bytes) return TF2_ERR_ARG;
  std::memset(out, 0, sizeof *out);
  out->byte_off = byte_off;
  out->byte_len = (int64_t)(bytes - (size_t)I.scan_offset);
  out->components = I.components;
  out->sub_x = I.sub_x;
  out->sub_y = I.sub_y;
  out->restart_interval = I.restart_interval;
  for (int c = 0; c < I.components; c++) {
    const Huff &dc = H.dc[H.comp[c].td], &ac = H.ac[H.comp[c].ta];
    std::memcpy(out->tab[c].dc_counts, dc.counts, 16);
    std::memcpy(out->tab[c].dc_vals, dc.vals, 256);
    std::memcpy(out->tab[c].ac_counts, ac.counts, 16);
    std::memcpy(out->tab[c].ac_vals, ac.vals, 256);
  }
  return TF2_OK;
}

}  // extern "C"
