// weight_dnscp.h -- DNS channel pruning behind tf2_dnscp_* (include/tf2_amd.h): the record and the argument blocks of the kernels
// (weight_dnscp.hip).  tf2_amd/dnscp.py states the rule (reference_stats / reference_step / reference_compact); the device equals it as bits.
#pragma once
#include "tf2_net.h"

namespace tf2 {

constexpr int kDnsWords = 16;             // int64 words of a conv's record (tf2_amd.h "Channel pruning")
constexpr int kDnsChunk = 4096;           // elements of the flat buffer one block walks: 256 threads x four 16-byte groups
constexpr int kDnsConvsPerLaunch = 48;    // convs one launch takes (their table travels in the kernel arguments)
constexpr int kDnsMaxC = 4096;            // input channels of a conv: one LDS slot each in the sum pass, one decision block
constexpr int kDnsSegsPerLaunch = 48;     // tensors one compact launch takes
constexpr int kDnsCompactBlock = 1024;    // elements of the pruned stream one compact block writes

// words of the record
enum : int {
  kDnsN = 0, kDnsNz, kDnsNonfinite, kDnsMax, kDnsE, kDnsA1, kDnsA2Hi, kDnsA2Lo, kDnsKeptBefore, kDnsPruned, kDnsRevived, kDnsFixup,
  kDnsKeptAfter, kDnsStatus, kDnsBLo, kDnsBHi
};

inline size_t dnscp_state_size(long long n_convs) { return (size_t)n_convs * kDnsWords * sizeof(long long); }

// One launch's share of the conv table; a block owns elements [first + blockIdx.x * kDnsChunk, + kDnsChunk) of the flat buffer.
struct DnsArgs {
  long long off[kDnsConvsPerLaunch];
  long long end[kDnsConvsPerLaunch];      // off + N * C * kk
  long long keep_off[kDnsConvsPerLaunch]; // the conv's first keep byte / S1 word
  int32_t C[kDnsConvsPerLaunch];
  int32_t kk[kDnsConvsPerLaunch];
  const float* w;
  float* out;                             // apply pass
  const uint8_t* keep;                    // null: every channel kept
  long long* sums;
  long long* state;                       // record of the launch's first conv
  long long first;                        // first element of block 0 (a multiple of kDnsChunk)
  int32_t n_convs;
  int32_t vec;                            // 16-byte accesses allowed
  int32_t inplace;                        // out == w: groups without a pruned element are not written
};

// The decision: one block a conv.
struct DnsDecideArgs {
  long long keep_off[kDnsConvsPerLaunch];
  double t_lo[kDnsConvsPerLaunch];
  double t_hi[kDnsConvsPerLaunch];
  int32_t C[kDnsConvsPerLaunch];
  int32_t nkk[kDnsConvsPerLaunch];        // N * kk
  int32_t flags[kDnsConvsPerLaunch];
  uint8_t* keep;                          // null: every channel kept, nothing written (tf2_dnscp_stats)
  const long long* sums;
  long long* state;
};

struct DnsCompactArgs {
  long long src_off[kDnsSegsPerLaunch];
  long long dst_off[kDnsSegsPerLaunch];
  long long n_idx[kDnsSegsPerLaunch];     // offset of the segment's n' -> n list in idx, -1: identity
  long long c_idx[kDnsSegsPerLaunch];
  int32_t n_src[kDnsSegsPerLaunch];
  int32_t c_src[kDnsSegsPerLaunch];
  int32_t n_out[kDnsSegsPerLaunch];
  int32_t c_out[kDnsSegsPerLaunch];
  int32_t kk[kDnsSegsPerLaunch];
  uint32_t block0[kDnsSegsPerLaunch + 1]; // first block of each segment
  const float* src;
  float* dst;
  const int32_t* idx;
  int32_t n_segs;
};

tf2_status dnscp_run(const float* dense, float* out, long long n_total, const tf2_dnscp_conv* convs, int n_convs, uint8_t* keep,
                     long long n_channels, long long* sums, void* state, void* scratch, size_t scratch_bytes, void* stream, bool step);
tf2_status dnscp_compact(const float* src, long long n_src, float* dst, long long n_dst, const tf2_dnscp_seg* segs, int n_segs,
                         const int32_t* idx, long long n_idx, void* stream);

}  // namespace tf2
