// tf2_net.h -- the network handle behind the C ABI (host side).
#pragma once
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "tf2_internal.h"

namespace tf2 {

struct LaunchRecord;

struct TensorPlan {
  int H = 0, W = 0, C = 0, Cp = 0;
  size_t bytes = 0;        // for the planned batch
  size_t offset = 0;
  int last_use = -1;       // last layer index reading it (n_layers = network output)
  int first_use = -1;      // the row from which the tensor holds memory (-1: the input); earlier than its producer when rows share a launch
};

struct LayerExec {
  int in_tensor = -1;      // tensor ids into WorkPlan::tensors
  int out_tensor = -1;     // final output of the layer (own tensor or concat tensor)
  int conv_tensor = -1;    // where the conv kernel writes (== out_tensor unless pool/endpool)
  int pool_tensor = -1;    // a row that pools AND averages: the PH x PW pooled map the average reads (full_size_pool.cl:71-92)
  int res_tensor = -1;
  int res_off = 0;
  int out_off = 0;         // channel offset inside out_tensor (concat slice)
};

enum PlanMode { PLAN_ORDINARY = 0, PLAN_KEEP_ALL = 1, PLAN_OUTPUTS = 2 };   // Net::plan

struct WorkPlan {
  int batch = 0;
  bool keep_all = false;
  bool outputs_kept = false;   // PLAN_OUTPUTS: sink rows live to the end of the step, no direct logits store
  std::vector<TensorPlan> tensors;
  std::vector<LayerExec> exec;
  int input_tensor = -1;
  int final_tensor = -1;
  size_t scratch_off = 0, scratch_bytes = 0;   // partial sums of conv_fc launches (behind the control area; never zeroed)
  size_t ctrl_off = 0, ctrl_bytes = 0;   // group counters of conv_bgroup launches (two words per image and launch)
  size_t ks_ctr_off = 0, ks_ctr_bytes = 0;       // ticket words of the split-K-over-blocks launches (the tail of the control area: cleared by the step's first kernel)
  size_t ks_part_off = 0, ks_part_bytes = 0;     // their partial tiles (part of the scratch area, one launch at a time)
  size_t total_bytes = 0;
};

// One prepared kernel launch of a step (net_plan.hip Net::launch_plan): argument block + kernel selection.
struct Launch {
  enum Kind { PREP, CONV, POOL, AVG, L2N } kind = CONV;
  enum Sel { SEL_MFMA2, SEL_SK, SEL_PW, SEL_PWK, SEL_PWKPAIR, SEL_SHIFT, SEL_BNECK, SEL_STEM, SEL_PAIR, SEL_SKPAIR, SEL_BGROUP, SEL_BGROUPF, SEL_BFIRST, SEL_BBAND, SEL_C3, SEL_FC, SEL_FIRST, SEL_FIRE, SEL_IMG } sel = SEL_MFMA2;
  int layer = -1;
  int TM = 0, signed_in = 0, mul24 = 0, shape = 0;
  int TM2 = 0;               // SEL_PWKPAIR: the second layer's tile height
  int pwk_slots = 0, pwk_pipe = 0;   // SEL_PWK / SEL_PWKPAIR: RunOpts::pwk_slots / pwk_pipe of the options the plan was built under
  int avg_fused = 0;         // the conv launch computes the layer's global average itself (no AVG step follows)
  ConvArgs conv{};
  ConvArgs conv2{};          // SEL_PAIR: the second (independent) layer of the launch, table row layer + 1
  ConvArgs conv_direct{};    // the last layer writing the dense logits itself (y patched per call)
  BneckArgs bneck{};
  FcArgs fc{};               // SEL_FC: a whole-window layer at batch <= 32 as a weight stream over the whole chip (conv_fc.hip)
  C3Args c3{};               // SEL_C3: a 3x3 / 1 / pad 1 layer from an LDS-resident halo tile (conv_c3.hip)
  ImgArgs img{};             // SEL_IMG: a 3x3 / 1 / pad 1 row of a small map, whole images per block (conv_img.hip)
  BBandArgs bband{};         // SEL_BBAND: rows layer .. layer + 2 (an identity bottleneck) in one launch, no exchange between blocks
  BGroupArgs bgroup{};       // SEL_BGROUP: rows layer .. layer + 2 (an identity bottleneck) in one launch
  int bg_hw = 0, bg_c = 0, bg_m = 0;
  const BGroupArgs& bg_chain_last() const { return bg_chain.empty() ? bgroup : bg_chain.back(); }
  std::vector<BGroupArgs> bg_chain;   // SEL_BGROUP of the 14 x 14 maps: this and the following identity bottlenecks in ONE launch (bgroup first)
  StemArgs stem{};
  PoolArgs pool{};
  AvgArgs avg{};
  PrepArgs prep{};
  FireArgs fire{};           // SEL_FIRE: rows layer (squeeze), layer + 1 and layer + 2 (the merged expands) in one launch (conv_fire.hip)
  FirstArgs first{};         // kind PREP, SEL_FIRST: input preparation + table row 0 in one launch (conv_first_kernel); prep = its input side
  L2NormArgs l2n{};
};

struct LaunchPlan {
  int batch = 0;
  const WorkPlan* wp = nullptr;
  void* ws = nullptr;
  const uint8_t* packed_dev = nullptr;
  int concurrent = 0;               // built for several batches in flight (wide-tile alternatives from a smaller grid on)
  int groups = 0;                   // group launches (conv_bgroup.hip) allowed: one batch at a time on a stream of >= 64 CUs
  std::vector<Launch> steps;
  int logits_direct = -1;           // index of the conv step that writes the dense logits itself (its y is patched per call), else -1
  int n_groups = 0;                 // group launches (conv_bgroup.hip) in the plan
  // Net::run walks a plan OUTSIDE the handle's mutex (several host threads, one stream and workspace each, enqueue at the same
  // time): `enqueue` serialises walks of this plan (one workspace = one step at a time anyway), `walkers` (under the handle's
  // mutex) keeps the plan from being evicted while somebody walks it
  std::shared_ptr<std::mutex> enqueue = std::make_shared<std::mutex>();
  int walkers = 0;
};

struct RunOpts {           // run-time switches of a handle, taken from the TF2_AMD_OPTS snapshot (opts.h) by Net::load_options (tf2_net_reload_options)
#define TF2_OPT(name, scope, test_only, type, member, dflt) type member = dflt;      // (one member per TF2_OPT line of opt_table.h, documented there)
#define TF2_OPT_RAW(name, scope, test_only, dflt)
#include "opt_table.h"
  int flags = 0;           // ConvGeom::flags (exp)
  long long* dbg = nullptr; long long* dbg2 = nullptr;     // dbgptr, dbgptr2
};

struct Net {
  tf2_net_desc nd{};
  std::vector<tf2_layer_desc> layers;
  std::vector<int8_t> q;                 // [n_q_rows][max_out_channel], runtime (negated)
  std::vector<LayerModel> models;
  bool model_loaded = false;

  // packed image (host copy) and its device binding
  std::vector<uint8_t> packed;
  bool packed_valid = false;
  int pack_mode = 0;
  const uint8_t* packed_dev = nullptr;
  size_t packed_dev_bytes = 0;

  // physical input layout of every layer (decided once from the graph)
  struct InLayout { int Cp_in = 0; int half = 0; int signed_in = 0; };
  // layer 0 executed as a pointwise layer over the im2col image (init(); PrepArgs::rewrite == 2)
  bool im2col0 = false; int im_stride = 1, im_pad_h = 0, im_pad_w = 0;
  std::vector<InLayout> in_layout;
  std::vector<int> out_Cp;               // channel padding of each layer's own output tensor
  std::vector<int> concat_C;             // channels of each concat tensor

  std::map<std::pair<int, int>, WorkPlan> plans;   // (batch, PlanMode) -> plan
  std::map<const void*, int> outputs_ws;           // workspace -> batch of its last step, where that step ran the outputs-kept plan
  std::list<LaunchPlan> launch_plans;              // prepared steps, keyed by (batch, plan, workspace, packed image); a list: growth and
                                                   // eviction never move a plan another thread is walking (oldest evicted at 64, under run_mutex)
  std::mutex run_mutex;                            // serialises run(): plan lookup / build, stream history, enqueue (tf2_amd.h threading note)
  RunOpts opts;

  // profiling
  bool profiling = false;
  std::vector<float> prof_ms;
  std::vector<int32_t> prof_launches;
  std::vector<std::pair<void*, void*>> prof_events;   // pending (start, stop) hipEvents
  bool profiling_loop = false; // tf2_net_profile(net, 2): ONE event pair around the whole layer loop
  float prof_loop_ms = 0.f;    // its accumulated time and count: the per-layer pairs of mode 1 each add their own record
  int prof_loop_n = 0;         // handling, so bench.py rescales their sum to this
  std::vector<int> prof_event_layer;

  tf2_status init(const tf2_net_desc* nd, const tf2_layer_desc* layers);
  tf2_status quantization(const char* text, size_t len, int8_t* q, size_t cap, int32_t* n_read) const;
  tf2_status load_model(const float* model, size_t n_floats);
  tf2_status load_model_4bit(const uint8_t* bytes, size_t n_bytes);    // straight from the 4-bit codes, no float32 copy of the weights
  tf2_status finish_model();
  tf2_status pack(int mode);
  bool stem_selected(int batch) const;     // layer 0 runs on conv_stem.hip (x-only image tensor)
  const PackLayer* pack_layer(int l) const;
  const PackLayer* pack_layer_alt(int l) const;
  bool pair_candidate(int l) const;        // rows l and l + 1 are independent plain conv rows (one launch may compute both)
  uint64_t tables_hash() const;
  const WorkPlan* plan(int batch, int mode);       // mode: PlanMode (a bool keep_all reads as ORDINARY / KEEP_ALL)
  bool is_sink(int l) const;
  const LaunchPlan* launch_plan(int batch, const WorkPlan* wp, void* ws, bool concurrent, bool allow_groups);
  size_t workspace_size(int batch, bool keep_all);      // plan(...)->total_bytes under the handle's mutex
  tf2_status describe_workspace(int batch, bool keep_all, std::vector<TensorPlan>* tensors, std::vector<LayerExec>* rows);
  bool bgroup_first_at(int l) const;       // rows l .. l + 3 = projection shortcut | reduce, 3x3, expand of the 56 x 56 stage (conv_bgroup56f_kernel)
  bool bband_at(int l, int rows) const;
    // rows l, l + 1, l + 2 are an identity bottleneck conv_bband.hip can take with `rows` output rows per block
  tf2_layer_desc exec_desc(int l) const;   // row l as executed (merged rows: the 3x3 layer of both rows' channels)
  bool out_nonneg(int l) const;            // the tensor layer l writes holds no negative value
  bool res_nonneg_single_clamp(int l) const;     // row l's residual epilogue may take the one-clamp form (requant_epilogue.h RNN)
  bool fire_at(int l) const;    // rows l (squeeze), l + 1, l + 2 (merged expands) are a fire module conv_fire.hip can take
  bool c3_at(int l) const;      // layer l can run on conv_c3.hip
  bool fc_at(int l, int batch) const;   // ... on conv_fc.hip
  bool img_at(int l) const;     // ... on conv_img.hip
  bool bgroup_at(int l) const;             // rows l, l + 1, l + 2 are an identity bottleneck conv_bgroup.hip can take (tables + packed image)
  long long stat_steps = 0, stat_group_steps = 0, stat_inflight_steps = 0, stat_small_mask_steps = 0;   // tf2_net_run_stats
  void* recent_streams[8] = {};  // streams of the last calls to run(): several distinct ones = batches in flight
  int recent_pos = 0;
  void load_options();
  size_t logits_bytes(int batch) const;
  tf2_status poll_error(int batch, void* ws, size_t ws_bytes, void* stream);
  tf2_status run(const void* images, bool images_are_q, int batch, void* ws, size_t ws_bytes,
                 int8_t* logits, void* stream, int concurrency = -1, void* mark_event = nullptr, int mark_after_layer = -1,
                 bool outputs_kept = false);
  int issue(const Launch& st, const LaunchPlan* lp, const void* images, bool images_are_q, int8_t* logits, void* stream);
  tf2_status describe_launches(int batch, bool concurrent, std::vector<std::pair<int, struct LaunchRecord>>* out);
  tf2_status read_layer(int layer, int batch, const void* ws, int8_t* dst, size_t cap, void* stream);
  void drain_profile();
};

const std::string& last_error();

// model4bit.cpp: one tensor of the 4-bit packed model file, in place
struct M4Tensor {
  int min_exp = 0, dtype = 0;
  size_t N = 0, C = 0, H = 0, W = 0, cnt = 0, words_per_row = 0;
  const uint8_t* payload = nullptr;
  // 4-bit code of weight `i` of the flattened [N][C][H][W] order (dtype 0)
  int code(size_t i) const {
    size_t word, j;
    if (W == 1) { word = i / 4; j = i % 4; }
    else { const size_t r = i / W, x = i % W; word = r * words_per_row + x / 3; j = x % 3; }
    return (int)((((unsigned)payload[2 * word] | ((unsigned)payload[2 * word + 1] << 8)) >> (4 * j)) & 15u);
  }
  float f32(size_t i) const { float v; std::memcpy(&v, payload + 4 * i, 4); return v; }      // dtype 1
};
struct M4Cursor {
  const uint8_t* p; size_t n; size_t pos = 0; int index = 0;
  M4Cursor(const uint8_t* bytes, size_t len) : p(bytes), n(len) {}
  bool done() const { return pos >= n; }
  std::string next(M4Tensor* t);          // error text, empty = ok
};
float m4_code_value(int code, int min_exp);
// decoder of the whole file into a float stream; returns an error text (empty = ok)
std::string model4bit_decode(const uint8_t* bytes, size_t n, std::vector<float>* out, size_t* n_floats);

}  // namespace tf2
