// act_rows.h -- what the activation observers share: the activation audit (act_audit), layer fidelity (act_fidelity) and CAQ calibration
// (act_caq) each reduce a network's per-row maps to per-channel int64 records in a caller-owned store; their counting differs, what
// stands around it is stated here once.
//   host    ActRows      the rows of a net and their records (row -1, the input, first), what tf2_*_describe reports of them
//           KeptMaps     what tf2_audit_run / tf2_fid_run refuse before they count, in their order, and the kept map of a layer
//           LaunchBatch  table rows dealt to launches of at most kRowsPerLaunch, each row's first block in its launch's grid
//   device  TF2_ROW_OF_BLOCK, add64, wave_sum / wave_min / wave_max
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "tf2_net.h"

namespace tf2 {

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct ActRows {
  struct Row { int layer, C, H, W; long long rec0; int n_doubled; };
  Net* net = nullptr;
  std::vector<Row> rows;     // row -1 first
  long long n_records = 0;

  tf2_status create(Net* n) {
    if (!n->packed_valid) { set_error("tf2_audit_create: no packed image (tf2_net_pack / tf2_net_packed_adopt first)"); return TF2_ERR_STATE; }
    net = n;
    rows.clear();
    rows.push_back(Row{-1, n->nd.image_c, n->nd.image_h, n->nd.image_w, 0, 0});
    long long rec = n->nd.image_c;
    for (int l = 0; l < n->nd.n_layers; l++) {
      const tf2_layer_desc& L = n->layers[l];
      const PackLayer* pl = n->pack_layer(l);
      const uint8_t* f = (pl && pl->off_dbl) ? n->packed.data() + pl->off_dbl : nullptr;
      int nd = 0;
      for (int c = 0; f && c < L.N; c++) nd += f[c] ? 1 : 0;
      rows.push_back(Row{l, L.N, L.endpool ? 1 : L.PH, L.endpool ? 1 : L.PW, rec, nd});
      rec += L.N;
    }
    n_records = rec;
    return TF2_OK;
  }
  size_t store_size(int slots) const { return (size_t)n_records * slots * sizeof(long long); }
  size_t workspace_size(int batch) const { return batch <= 0 ? 0 : net->workspace_size(batch, true); }
  // fn: "tf2_x_describe"; slots: int64 words of a record of that store
  tf2_status describe(const char* fn, int slots, tf2_audit_row* out, int capacity, int* n) const {
    if (!n || (capacity > 0 && !out)) return arg_refusal(fn, "null argument");
    *n = (int)rows.size();
    if ((int)rows.size() > capacity) { set_error(std::string(fn) + ": " + std::to_string(rows.size()) + " rows, capacity " + std::to_string(capacity)); return TF2_ERR_SIZE; }
    for (size_t i = 0; i < rows.size(); i++) {
      out[i].layer = rows[i].layer; out[i].C = rows[i].C; out[i].H = rows[i].H; out[i].W = rows[i].W;
      out[i].store_offset = (int64_t)(rows[i].rec0 * slots * 8);
      out[i].n_doubled = rows[i].n_doubled; out[i].reserved = 0;
    }
    return TF2_OK;
  }
};

// The kept map of a layer after a keep_all step: the NHWC int8 slice [npix][Cp] from `base` (the slice's first channel), C channels.
struct KeptMap {
  const int8_t* base;
  const uint8_t* dbl;        // [C] in the packed image on the device: 1 = the channel holds 2y - 128 (null: no such channel)
  long long npix;
  int C, Cp, HW;
  int off;                   // the slice's first channel in its tensor
  long long rec0;            // the row's first record
};
struct KeptMaps {
  std::string fn;            // "tf2_audit_run"
  const ActRows* g = nullptr;
  const WorkPlan* wp = nullptr;
  const void* ws = nullptr;
  int batch = 0;
  long long pix_slack = 0;

  // pre: "tf2_audit" / "tf2_fid"; any_null, null_text: the entry point's own null-pointer refusal; store_need: its store_size();
  // pix_slack: what the kernel adds to a pixel index beyond the row's pixels (npix + pix_slack fits 31 bits)
  tf2_status open(const ActRows& rows, const std::string& pre, bool any_null, const char* null_text, int batch_, const void* ws_, size_t ws_bytes,
                  size_t store_bytes, size_t store_need, long long pix_slack_) {
    fn = pre + "_run"; g = &rows; ws = ws_; batch = batch_; pix_slack = pix_slack_;
    Net* net = rows.net;
    if (batch <= 0) return arg_refusal(fn.c_str(), "batch must be positive");
    if (any_null) return arg_refusal(fn.c_str(), null_text);
    if (!net->packed_valid) { set_error(fn + ": no packed image (tf2_net_pack / tf2_net_packed_adopt)"); return TF2_ERR_STATE; }
    if (!net->packed_dev) { set_error(fn + ": packed image not bound to the device (tf2_net_bind_device)"); return TF2_ERR_STATE; }
    if ((int)rows.rows.size() != net->nd.n_layers + 1) { set_error(fn + ": the handle does not fit the net"); return TF2_ERR_STATE; }
    if (store_bytes < store_need) { set_error(fn + ": store too small (" + pre + "_store_size: " + std::to_string(store_need) + ")"); return TF2_ERR_SIZE; }
    { std::lock_guard<std::mutex> lock(net->run_mutex); wp = net->plan(batch, true); }      // (map nodes are stable)
    if (ws_bytes < wp->total_bytes) { set_error(fn + ": workspace too small (" + pre + "_workspace_size: " + std::to_string(wp->total_bytes) + ")"); return TF2_ERR_SIZE; }
    return TF2_OK;
  }
  // layer l's kept map, or the refusal: the kept tensor has the row's shape
  tf2_status map(int l, KeptMap& m) const {
    const LayerExec& E = wp->exec[l];
    const TensorPlan& t = wp->tensors[E.out_tensor];
    const ActRows::Row& row = g->rows[l + 1];
    const long long npix = (long long)batch * t.H * t.W;
    if (t.H * t.W != row.H * row.W || E.out_off + row.C > t.Cp || npix + pix_slack > 0x7fffffffll) {
      set_error(fn + ": row " + std::to_string(l) + ": the kept tensor does not have the row's shape"); return TF2_ERR_UNSUPPORTED;
    }
    const PackLayer* pl = g->net->pack_layer(l);
    m.base = (const int8_t*)ws + t.offset + E.out_off;
    m.dbl = (pl && pl->off_dbl) ? g->net->packed_dev + pl->off_dbl : nullptr;
    m.npix = npix; m.C = row.C; m.Cp = t.Cp; m.HW = row.H * row.W; m.off = E.out_off; m.rec0 = row.rec0;
    return TF2_OK;
  }
};

// Args: a kernel's argument block with `Row rows[kRowsPerLaunch]` and `n_rows`; Row has `block0`.  Every launch starts as a copy of
// `first` (n_rows = 0 and what all launches share: the store, the scale table).
template <class Args, class Row, int kRowsPerLaunch>
struct LaunchBatch {
  std::string fn;            // "tf2_x"
  Args first;
  std::vector<Args> launches;
  std::vector<long long> blocks;             // the grid of each launch

  LaunchBatch(const std::string& fn_, const Args& first_) : fn(fn_), first(first_) { first.n_rows = 0; }
  // the next row, n_blocks of its launch's grid from block0 on; null (and the error set) where the grid no longer fits 31 bits
  Row* add(long long n_blocks) {
    if (launches.empty() || launches.back().n_rows == kRowsPerLaunch) { launches.push_back(first); blocks.push_back(0); }
    Args& A = launches.back();
    Row* R = &A.rows[A.n_rows++];
    R->block0 = (int32_t)blocks.back();
    blocks.back() += n_blocks;
    if (blocks.back() > 0x7fffffffll) { set_error(fn + ": too many blocks for one grid"); return nullptr; }
    return R;
  }
};

// ---- device ----------------------------------------------------------------------------------------------------------------------
// r = the table row of argument block p this block belongs to (block0 ascends; block-uniform).  A macro, not a function: an inlined
// function is simplified before it meets the kernel's argument block and hipcc then allocates registers differently -- over the row
// array with its count, over the block by reference and by value, audit_rows_kernel took 94 VGPRs for 86 or other instructions, and
// both CAQ kernels changed; this form compiles to the code the three kernels had with the loop written out.
#define TF2_ROW_OF_BLOCK(r, p)               \
  r = 0;                                     \
  for (int i = 1; i < (p).n_rows; i++)       \
    if ((int)blockIdx.x >= (p).rows[i].block0) r = i

// a counter of a record: the 64-bit atomic only where there is something to add
__device__ __forceinline__ void add64(unsigned long long* p, long long v) {
  if (v) atomicAdd(p, (unsigned long long)v);
}
__device__ __forceinline__ void add64(long long* p, unsigned long long v) {
  if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), v);
}

// over the 64 lanes of a wave, the result in every lane (T: int, uint32_t, unsigned long long)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (T)__shfl_xor(v, o));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (T)__shfl_xor(v, o));
  return v;
}

}  // namespace tf2
