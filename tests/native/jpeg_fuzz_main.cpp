// jpeg_fuzz_main.cpp -- a stand-alone program around tf2_amd/csrc/jpeg_entropy.cpp for the host sanitizers (tests/test_jpeg.py builds
// it with -fsanitize=address,undefined and expects exit status 0).  argv[1] is a file of JPEG files: uint32 count, then per file
// uint32 length, uint32 supported (1: the file itself must decode with status 0) and the bytes; argv[2] the number of mutations a file.  Every file is parsed and decoded as it is, then as seeded
// truncations and bit flips.  Each input lives in a heap block of exactly its size and the coefficients in one of exactly
// total_blocks blocks, so a read or a write one byte outside either is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/tf2_amd.h"

namespace {

constexpr int64_t kMaxBlocks = 1 << 15;          // a flipped size field can ask for gigabytes: beyond this the call must refuse

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

long long decoded = 0, refused = 0, flagged = 0;

// 0: fine (whatever the statuses say); 1: the library broke a promise
int run_one(const uint8_t* data, size_t n, bool must_decode) {
  uint8_t* file = (uint8_t*)std::malloc(n ? n : 1);
  std::memcpy(file, data, n);
  tf2_jpeg_info info;
  int bad = 0;
  if (tf2_jpeg_parse(file, n, &info) != TF2_OK) bad = 1;
  if (!bad && info.status == 0) {
    const int64_t total = info.total_blocks;
    if (total < 1) bad = 1;
    const int64_t cap = total > kMaxBlocks ? kMaxBlocks : total;
    int16_t* coef = (int16_t*)std::malloc((size_t)cap * 128);
    int32_t st = -1;
    const tf2_status r = tf2_jpeg_entropy(file, n, &info, coef, (size_t)cap, &st);
    if (total > cap) {
      if (r != TF2_ERR_SIZE) bad = 1;
      refused++;
    } else {
      if (r != TF2_OK || st < 0) bad = 1;
      if (st == 0) decoded++; else flagged++;
      if (must_decode && st != 0) bad = 1;
    }
    std::free(coef);
  } else {
    refused++;
  }
  std::free(file);
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s files.bin mutations\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  const int mutations = std::atoi(argv[2]);
  uint32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t n = 0, supported = 0;
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&supported, 4, 1, f) != 1) return 2;
    std::vector<uint8_t> data(n);
    if (n && std::fread(data.data(), 1, n, f) != n) return 2;
    if (run_one(data.data(), n, supported != 0)) { std::fprintf(stderr, "file %u: a promise broken on the file itself\n", i); return 1; }
    for (int m = 0; m < mutations; m++) {
      std::vector<uint8_t> v(data);
      if (m % 3 == 0) {
        v.resize(rnd() % (n + 1));                                 // a truncation anywhere, the empty file included
      } else {
        const int flips = 1 + (int)(rnd() % 4);
        for (int k = 0; k < flips && n; k++) v[rnd() % n] ^= (uint8_t)(1u << (rnd() % 8));
        if (m % 3 == 2 && n) v.resize(1 + rnd() % n);
      }
      if (run_one(v.data(), v.size(), false)) { std::fprintf(stderr, "file %u mutation %d: a promise broken\n", i, m); return 1; }
    }
  }
  std::fclose(f);
  std::printf("decoded %lld, flagged %lld, refused %lld\n", decoded, flagged, refused);
  return 0;
}
