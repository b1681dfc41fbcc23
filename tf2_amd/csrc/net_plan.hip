// net_plan.hip -- launch planning (host code): which kernel runs each table row and with which argument block.
//
// Net::launch_plan builds the prepared launches of one step (LaunchPlan, tf2_net.h) once per (batch, workspace, packed image,
// in-flight flag); Net::run (net.hip) only walks them.  Here: the selection predicates of the kernels that take several rows or a
// special shape (Net::*_at; Net::plan extends tensor lifetimes by the same predicates), and the planner.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "tf2_net.h"
#include "tf2_device.h"

namespace tf2 {

// ---- selection predicates: what the tables and the packed image allow, whatever the batch and the plan ----
// Rows l and l + 1 may share a launch (conv_mfma2_pair_kernel): plain convolution rows (no pool / average / concat slice /
// L2Norm), neither reads what the other writes, neither is part of a fused bottleneck pair.  In ResNet-50: a stage's shortcut
// convolution and the first 1x1 of its first bottleneck (both read the previous stage's output).
bool Net::pair_candidate(int l) const {
  if (l < 1 || l + 1 >= nd.n_layers) return false;
  const tf2_layer_desc& A = layers[l]; const tf2_layer_desc& B = layers[l + 1];
  for (const tf2_layer_desc* L : {&A, &B})
    if (L->ipool || L->pool_en || L->endpool || L->concat >= 0 || L->src < 0) return false;
  if (B.src == l || B.add_src == l) return false;
  if (A.add_src >= 0 || B.add_src >= 0) return false;          // (a residual source may be the partner's input chain; keep it simple)
  const PackLayer* pa = pack_layer(l); const PackLayer* pb = pack_layer(l + 1);
  if (!pa || !pb || pa->kind != KIND_MFMA || pb->kind != KIND_MFMA) return false;
  if (pa->fuse_next > 0 || pa->fused_into >= 0 || pb->fuse_next > 0 || pb->fused_into >= 0) return false;
  return true;
}

// Rows l .. l + 3 = projection shortcut (1x1, 64 -> 256) and reduce (1x1, 64 -> 64) of the same 56 x 56 input, 3x3, expand +
// residual from the shortcut: conv_bgroup56f_kernel.  Shortcut, reduce and expand all two-window (packed dual) or all one-window.
bool Net::bgroup_first_at(int l) const {
  if (l < 1 || l + 3 >= nd.n_layers) return false;
  const tf2_layer_desc& S = layers[l]; const tf2_layer_desc& A = layers[l + 1]; const tf2_layer_desc& B = layers[l + 2]; const tf2_layer_desc& E = layers[l + 3];
  for (const tf2_layer_desc* L : {&S, &A, &B, &E})
    if (L->ipool || L->pool_en || L->endpool || L->concat >= 0 || L->stride != 1 || L->dil != 1 || L->H != 56 || L->W != 56) return false;
  if (S.src < 0 || S.src != A.src || layers[S.src].concat >= 0 || S.k != 1 || A.k != 1 || S.pad_h || A.pad_h || S.add_src >= 0 || A.add_src >= 0) return false;
  if (S.C != 64 || S.N != 256 || A.C != 64 || A.N != 64) return false;
  if (B.src != l + 1 || B.k != 3 || B.pad_h != 1 || B.pad_w != 1 || B.add_src >= 0 || B.C != 64 || B.N != 64) return false;
  if (E.src != l + 2 || E.k != 1 || E.pad_h || E.add_src != l || E.C != 64 || E.N != 256) return false;
  int n_dual = 0;
  for (int k = l; k <= l + 3; k++) {
    const PackLayer* pl = pack_layer(k);
    if (!pl || pl->kind != KIND_MFMA || pl->Cp_in != 64 || (long)pl->n_entries != (long)pl->n_mtiles * pl->nslab) return false;
    if (k == l ? (pl->TM != 64 && pl->TM != 128) : pl->TM != 64) return false;
    const bool one_window = pl->n_phases == 1 && !pl->dual, dual = pl->n_phases == 2 && pl->dual;
    if (!one_window && !dual) return false;
    if (k == l + 2) { if (!one_window) return false; } else n_dual += dual ? 1 : 0;
    if (k == l && pl->off_dbl) return false;            // (the shortcut's output is only ever a residual)
  }
  return n_dual == 0 || n_dual == 3;
}

// Row l as it is EXECUTED: the table row, or -- merged rows (PackLayer::merge_next, weight_pack.cpp: a 1x1 row and the 3x3 / pad 1 row
// behind it, same input, adjacent concat slices) -- the 3x3 layer of both rows' output channels
tf2_layer_desc Net::exec_desc(int l) const {
  tf2_layer_desc L = layers[l];
  const PackLayer* pl = pack_layer(l);
  if (pl && pl->merge_next > 0) { L.N += layers[pl->merge_next].N; L.k = 3; L.pad_h = L.pad_w = 1; }
  return L;
}

// The tensor layer l writes holds no negative value (its last operation is a ReLU)
bool Net::out_nonneg(int l) const {
  if (l < 0) return false;                                  // the image
  const tf2_layer_desc& L = layers[l];
  if (L.ipool == 2) return false;                           // L2Norm: sign(w) * sign(x)
  if (L.ipool) return out_nonneg(L.src);                    // a pool row keeps its input's range
  return L.add_src >= 0 ? L.add_relu != 0 : L.relu != 0;
}

// Row l adds a residual under the conditions of requant_epilogue.h's RNN form: no ReLU of its own, a post-ReLU residual tensor, the sum
// clamped to [0, 127] -- clamp(clamp(y, -128, 127) + r, 0, 127) == clamp(y + r, 0, 127), the first clamp is left out
bool Net::res_nonneg_single_clamp(int l) const {
  const tf2_layer_desc& L = layers[l];
  return L.add_src >= 0 && !L.relu && L.add_relu && layers[L.add_src].concat < 0 && out_nonneg(L.add_src);
}

// Rows l, l + 1, l + 2 = 1x1 reduce, 3x3 / 1 / pad 1, 1x1 expand + residual from the reduce's input, of a shape conv_bgroup.hip
// is instantiated for, every row single-window in 64- or 128-row dense tiles.
bool Net::bgroup_at(int l) const {
  if (l < 1 || l + 2 >= nd.n_layers) return false;
  const tf2_layer_desc& A = layers[l]; const tf2_layer_desc& B = layers[l + 1]; const tf2_layer_desc& E = layers[l + 2];
  for (const tf2_layer_desc* L : {&A, &B, &E})
    if (L->ipool || L->pool_en || L->concat >= 0 || L->stride != 1 || L->dil != 1) return false;
  // a global average may end the bottleneck where the split-K kernel could fuse it as well (7 x 7 shape only)
  if (A.endpool || B.endpool || (E.endpool && !(opts.avg_fuse && A.H == 7))) return false;
  if (A.src < 0 || A.k != 1 || A.pad_h || A.pad_w || A.add_src >= 0) return false;
  if (B.src != l || B.k != 3 || B.pad_h != 1 || B.pad_w != 1 || B.add_src >= 0 || B.C != A.N || B.N != A.N) return false;
  if (E.src != l + 1 || E.k != 1 || E.pad_h || E.pad_w || E.add_src != A.src || E.N != A.C) return false;
  if (layers[A.src].concat >= 0 || A.H != A.W || !conv_bgroup_shape_ok(A.H, A.C, A.N)) return false;
  if (!res_nonneg_single_clamp(l + 2)) return false;        // (the group kernels' expands use the single-clamp form)
  for (int k = l; k <= l + 2; k++) {
    const PackLayer* pl = pack_layer(k);
    if (!pl || pl->kind != KIND_MFMA) return false;
    if (pl->Cp_in % 64 != 0 || (long)pl->n_entries != (long)pl->n_mtiles * pl->nslab) return false;      // dense tiles
    const bool one_window = pl->n_phases == 1 && !pl->dual, dual = pl->n_phases == 2 && pl->dual;
    if (A.H == 28) {
      // the 28 x 28 kernel: 64- or 128-row tiles (its header slots hold a 128-row m-tile), the expand in 128-row tiles; the reduce
      // may be a two-window layer; rows packed for a conv_bneck pair qualify (the pair's own entries are one dense m-tile)
      if ((pl->TM != 64 && pl->TM != 128) || (k == l + 2 && pl->TM != 128)) return false;
      if (!(one_window || (k <= l + 1 && dual))) return false;
    } else {
      if (pl->fuse_next > 0 || pl->fused_into >= 0 || pl->TM != 64) return false;      // (2 KiB header slots: 64-row m-tiles)
      if (!(one_window || (k == l && A.H == 7 && dual))) return false;                 // the 7 x 7 kernel's reduce may be two-window
    }
  }
  return true;
}

// Rows l, l + 1, l + 2 = an identity bottleneck (as bgroup_at) of a shape conv_bband.hip is instantiated for, every row a dense
// single-window layer.
bool Net::bband_at(int l, int rows) const {
  if (l < 1 || l + 2 >= nd.n_layers) return false;
  const tf2_layer_desc& A = layers[l]; const tf2_layer_desc& B = layers[l + 1]; const tf2_layer_desc& E = layers[l + 2];
  for (const tf2_layer_desc* L : {&A, &B, &E})
    if (L->ipool || L->pool_en || L->endpool || L->concat >= 0 || L->stride != 1 || L->dil != 1) return false;
  if (A.src < 0 || A.k != 1 || A.pad_h || A.pad_w || A.add_src >= 0) return false;
  if (B.src != l || B.k != 3 || B.pad_h != 1 || B.pad_w != 1 || B.add_src >= 0 || B.C != A.N || B.N != A.N) return false;
  if (E.src != l + 1 || E.k != 1 || E.pad_h || E.pad_w || E.add_src != A.src || E.N != A.C) return false;
  if (layers[A.src].concat >= 0) return false;
  if (!res_nonneg_single_clamp(l + 2)) return false;        // (conv_bband's expand uses the single-clamp form)
  {
    const PackLayer* p0 = pack_layer(l); const PackLayer* p1 = pack_layer(l + 1);
    if (!p0 || !p1) return false;
    if (!conv_bband_shape_ok(A.H, A.W, A.C, A.N, std::min(conv_bband_pick_rows(A.W, A.N, p0->dual, p1->dual, rows, opts.bband_rows_dd), A.H))) return false;
  }
  if (out_Cp[A.src] != A.C) return false;                  // the input tensor holds exactly C bytes per pixel
  for (int k = l; k <= l + 2; k++) {
    const PackLayer* pl = pack_layer(k);
    if (!pl || pl->kind != KIND_MFMA || (pl->TM != 64 && pl->TM != 128)) return false;
    if (pl->Cp_in % 64 != 0 || (long)pl->n_entries != (long)pl->n_mtiles * pl->nslab) return false;      // dense tiles
    if (pl->w_share) return false;
    const bool one_window = pl->n_phases == 1 && !pl->dual, dual = pl->n_phases == 2 && pl->dual;
    if (!one_window && !(dual && k < l + 2)) return false;                                                // (the expand: single-window only)
  }
  return conv_bband_windows_ok(A.N, pack_layer(l)->dual, pack_layer(l + 1)->dual);
}

// Rows l (1x1 squeeze, ReLU), l + 1 and l + 2 (the merged expand1x1 | expand3x3 pair, PackLayer::merge_next) of a fire module whose
// squeeze output nothing else reads: conv_fire.hip takes them as one launch (a pool behind the expands follows as its own launch)
bool Net::fire_at(int l) const {
  if (l < 0 || l + 2 >= nd.n_layers) return false;
  const tf2_layer_desc& A = layers[l]; const tf2_layer_desc& B = layers[l + 1];
  if (A.ipool || A.pool_en || A.endpool || A.concat >= 0 || A.add_src >= 0 || !A.relu || A.k != 1 || A.stride != 1 || (A.pad_h | A.pad_w) || A.src == -1) return false;
  if (in_layout[l].Cp_in != A.C || A.C % 64 != 0 || in_layout[l].signed_in) return false;
  const PackLayer* p0 = pack_layer(l); const PackLayer* p1 = pack_layer(l + 1); const PackLayer* p2 = pack_layer(l + 2);
  if (!p0 || !p1 || !p2 || p0->kind != KIND_MFMA || p1->kind != KIND_MFMA || p1->merge_next != l + 2 || p2->merged_into != l + 1) return false;
  if (B.src != l || B.endpool || B.add_src >= 0 || !B.relu) return false;      // (a pool behind the expands: its own launch after the fire launch)
  for (int j = 0; j < nd.n_layers; j++)
    if (j != l + 1 && j != l + 2 && (layers[j].src == l || layers[j].add_src == l)) return false;      // the squeeze's tensor is not written
  if (p0->TM != 64 || p0->n_mtiles != 1 || (long)p0->n_entries != p0->nslab || !(p0->n_phases == 1 || p0->dual) || p0->w_share || p0->fuse_next > 0 || p0->fused_into >= 0) return false;
  if (p1->n_phases != 1 || p1->dual || p1->w_share || (p1->TM != 64 && p1->TM != 128) || p1->Cp_in != round_up(A.N, 16) || p1->off_dbl) return false;
  return conv_fire_geometry(A.H, A.W, A.C, round_up(A.N, 16), p1->Np, p0->TM, p1->TM, p0->dual, 0, nullptr, nullptr) && p1->Np == layers[l + 1].N + layers[l + 2].N;
}

// a 3x3 / stride 1 / pad 1 layer on an unsigned tensor that holds exactly C (a multiple of 64) bytes per pixel, dense one- or two-window
// tiles of its own: conv_c3.hip takes it (the halo tile of the input streamed through LDS once instead of nine gathers)
bool Net::c3_at(int l) const {
  const tf2_layer_desc& L = layers[l];
  if (L.ipool || L.k != 3 || L.stride != 1 || L.dil != 1 || L.pad_h != 1 || L.pad_w != 1 || L.src < 0 || L.add_src >= 0 || L.endpool) return false;
  if (layers[L.src].concat >= 0 || out_Cp[L.src] != L.C || L.OH != L.H || L.OW != L.W) return false;
  const PackLayer* pl = pack_layer(l);
  if (!pl || pl->kind != KIND_MFMA || (pl->TM != 64 && pl->TM != 128) || pl->w_share || pl->signed_in) return false;
  if (pl->Cp_in != L.C || pl->Cp_in % 64 != 0 || pl->nslab != 9 * (pl->Cp_in / 64) || (long)pl->n_entries != (long)pl->n_mtiles * pl->nslab) return false;
  if (pl->fuse_next > 0 || pl->fused_into >= 0) return false;
  const bool one_window = pl->n_phases == 1 && !pl->dual, dual = pl->n_phases == 2 && pl->dual;
  if (!one_window && !dual) return false;
  return conv_c3_shape_ok(L.H, L.W, L.C, pl->Np, opts.c3_min_hw);
}

// a layer whose input is ONE filter window per image (k x k / pad 0 on a k x k map), K long, at batch <= 32, not the network's last
// (that one stores the dense logits itself): conv_fc.hip streams its weights over the whole chip
bool Net::fc_at(int l, int batch) const {
  const tf2_layer_desc& L = layers[l];
  if (l == nd.n_layers - 1) return false;
  { const PackLayer* p4 = pack_layer(l); if (batch > 32 && !(p4 && p4->fc4)) return false; }      // (4-bit code layers: any batch, in chunks of 32 -- they have no int8 tiles)
  if (L.ipool || L.k != L.H || L.k != L.W || L.stride != 1 || L.dil != 1 || L.pad_h || L.pad_w || L.OH != 1 || L.OW != 1) return false;
  if (L.src < 0 || L.add_src >= 0 || L.endpool || L.pool_en || L.concat >= 0 || layers[L.src].concat >= 0 || out_Cp[L.src] != L.C) return false;
  const PackLayer* pl = pack_layer(l);
  if (!pl || pl->kind != KIND_MFMA || (pl->TM != 64 && pl->TM != 128) || pl->w_share || pl->signed_in || pl->Np % 128 != 0) return false;
  if (pl->Cp_in != L.C || pl->Cp_in % 64 != 0 || pl->nslab != L.k * L.k * (pl->Cp_in / 64) || (long)pl->n_entries != (long)pl->n_mtiles * pl->nslab) return false;
  if ((pl->nslab < opts.fc_min_slabs && !pl->fc4) || pl->fuse_next > 0 || pl->fused_into >= 0) return false;
  const bool one_window = pl->n_phases == 1 && !pl->dual, dual = pl->n_phases == 2 && pl->dual;
  return one_window || dual;
}

// a k x k (k = 1, 3) / stride 1 / pad (k - 1) / 2 row on a square map of a shape conv_img.hip is instantiated for: a post-ReLU input
// tensor of its own with exactly C bytes per pixel, dense one- or two-window 64-row tiles of its own, nothing behind the convolution
// but the requantisation (no pool, average, concat slice, residual), not the network's last row (that one stores the dense logits)
bool Net::img_at(int l) const {
  if (l < 0 || l >= nd.n_layers - 1) return false;
  const tf2_layer_desc& L = layers[l];
  if (L.ipool || L.pool_en || L.endpool || L.concat >= 0 || L.add_src >= 0 || L.src < 0) return false;
  if ((L.k != 1 && L.k != 3) || L.stride != 1 || L.dil != 1 || L.pad_h != (L.k - 1) / 2 || L.pad_w != (L.k - 1) / 2) return false;
  if (L.H != L.W || L.OH != L.H || L.OW != L.W) return false;
  if (layers[L.src].concat >= 0 || out_Cp[L.src] != L.C || !out_nonneg(L.src)) return false;
  const PackLayer* pl = pack_layer(l);
  if (!pl || pl->kind != KIND_MFMA || pl->TM != 64 || pl->w_share || pl->signed_in) return false;
  if (pl->Cp_in != L.C || pl->Cp_in % 64 != 0 || pl->nslab != L.k * L.k * (pl->Cp_in / 64) || (long)pl->n_entries != (long)pl->n_mtiles * pl->nslab) return false;
  if (pl->fuse_next > 0 || pl->fused_into >= 0 || pl->merge_next > 0 || pl->merged_into >= 0 || pl->fc4) return false;
  const bool one_window = pl->n_phases == 1 && !pl->dual, dual = pl->n_phases == 2 && pl->dual;
  if (!one_window && !dual) return false;
  return conv_img_shape_ok(L.H, L.C, L.k);
}

// conv_stem.hip takes layer 0 when the packed image holds its x-only weight tiles (weight_pack.cpp) and the fast
// space-to-depth prep applies; the input tensor then carries 32 bytes per pixel in the same allocation.
bool Net::stem_selected(int batch) const {
  const tf2_layer_desc& L0 = layers[0];
  const PackLayer* p0 = pack_layer(0);
  const long long pixels = (long long)batch * L0.H * L0.W;
  return opts.stem_mode != 0 && p0 && p0->kind == KIND_MFMA && p0->off_w2 != 0 && nd.conv1_rewrite && nd.image_c == 3 &&
         in_layout[0].Cp_in == 64 && in_layout[0].half == 32 && L0.OH == L0.H - 2 && L0.OW == L0.W - 2 &&
         pixels * 64 < (1ll << 31) && (long long)batch * 3 * nd.image_h * nd.image_w < (1ll << 31);
}

// Group launches (conv_bgroup.hip) keep eight blocks per image resident together, one block per CU: they need a device of at
// least 64 CUs -- and a STREAM that may use at least 64 of them (stream_cu_count, net.hip: Net::run asks per call).  No device
// (describing a plan on the CPU): assume the full chip.
static bool device_fits_group_launches() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return true;
  static std::mutex mu;
  static std::map<int, int> n_cu;
  std::lock_guard<std::mutex> lock(mu);
  auto it = n_cu.find(dev);
  if (it == n_cu.end()) {
    hipDeviceProp_t prop;
    const int n = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
    it = n_cu.emplace(dev, n).first;
  }
  return it->second >= 64;
}

// ---- launch plan: every kernel argument block of one step, resolved once per (batch, workspace, packed image) ----
// Net::run used to rebuild ~60 argument structs, scan the packed directory and read a dozen environment variables
// per call; at batch 1 (57 launches of a few microseconds) that host work was the step.  Now a step is a loop over
// prepared launches; only the image and logits pointers change between calls.
namespace {

// Builds the steps of one LaunchPlan.  One member function per thing planned; a function that is asked about table row l answers
// whether it TOOK the row (and the rows behind it that share its launch).  A function that has to give the whole plan up (the error text
// is set) sets `failed` and answers "took": rows() stops there.
struct Planner {
  Net& n; LaunchPlan& lp; const WorkPlan* const wp;
  int8_t* const base; const uint8_t* const pk; const uint64_t zero_off;      // the workspace; the packed image as the kernels address it, its zero page
  const int batch; const bool concurrent; const RunOpts& opts; const int nl; const bool groups_fit;
  // the global average inside the last expand's split-K launch (conv_mfma_sk AVG: 1024 blocks of 64 x 64 tiles, one image per pixel
  // tile) pays one batch at a time (a launch and the 7 x 7 map's round trip less); with batches in flight that launch costs 13 us of the
  // step against 2.6 us for the same row on 208 blocks of 128 x 128 tiles + a 512-block average (round 6, profiles/r06_experiments.txt
  // items 1-2: 94.8 -> 96.5 k img/s) -- avg_fuse = 2 (default): one batch at a time only
  const bool avg_fuse_now, stem;
  std::vector<char> fused_done, pair_done;     // rows computed by the launch of an earlier row
  int bg_used = 0;                             // group launches so far (each has its own counters)
  bool stem_pool_fused = false, failed = false;

  Planner(Net& net, LaunchPlan& plan, const WorkPlan* w, void* ws, int b, bool conc, bool allow_groups)
      : n(net), lp(plan), wp(w), base((int8_t*)ws), pk(net.packed_dev), zero_off(reinterpret_cast<const PackHeader*>(net.packed.data())->zero_off),
        batch(b), concurrent(conc), opts(net.opts), nl(net.nd.n_layers), groups_fit(allow_groups && device_fits_group_launches()),
        avg_fuse_now(net.opts.avg_fuse == 1 || (net.opts.avg_fuse == 2 && !conc)), stem(net.stem_selected(b)), fused_done(nl, 0), pair_done(nl, 0) {}

  const TensorPlan& T(int id) const { return wp->tensors[id]; }
  bool give_up() { failed = true; return true; }
  bool give_up(const std::string& m) { set_error(m); return give_up(); }
  long long* dbg_ptr(int l) const { return (opts.dbg2 && opts.dbg_layer == l) ? opts.dbg2 : nullptr; }
  void mark_done(int first, int last) { for (int k = first; k <= last; k++) pair_done[k] = 1; }

  // input: quantise + (space-to-depth) + [x | xneg]
  bool input_step() {
    const tf2_layer_desc& L0 = n.layers[0];
    Launch st; st.kind = Launch::PREP; st.layer = -1;
    PrepArgs& pa = st.prep;
    pa.img = nullptr; pa.y = base + T(wp->input_tensor).offset;
    pa.B = batch; pa.C = n.nd.image_c; pa.H = n.nd.image_h; pa.W = n.nd.image_w;
    pa.OH = L0.H; pa.OW = L0.W; pa.y_cp = n.in_layout[0].Cp_in; pa.half = n.in_layout[0].half;
    pa.rewrite = n.im2col0 ? 2 : n.nd.conv1_rewrite; pa.q0 = n.q[0]; pa.src_is_q = 0; pa.xonly = stem ? 1 : 0;
    pa.im_stride = n.im_stride; pa.im_pad_h = n.im_pad_h; pa.im_pad_w = n.im_pad_w;
    if (!n.nd.conv1_rewrite && !n.im2col0 && (L0.H != n.nd.image_h || L0.W != n.nd.image_w || L0.C != n.nd.image_c)) {
      set_error("layer 0 input does not match the image"); return false;
    }
    lp.steps.push_back(st);
    return true;
  }

  void pool_step(int l, const TensorPlan& ti, const int8_t* x, int H, int W) {
    const tf2_layer_desc L = n.exec_desc(l);
    const LayerExec& E = wp->exec[l];
    Launch st; st.kind = Launch::POOL; st.layer = l;
    PoolArgs& pa = st.pool;
    const TensorPlan& to = T(E.pool_tensor >= 0 ? E.pool_tensor : E.out_tensor);
    pa.x = x; pa.y = base + to.offset;
    pa.B = batch; pa.H = H; pa.W = W; pa.x_cp = ti.Cp; pa.x_off = 0;
    pa.PH = L.PH; pa.PW = L.PW; pa.y_cp = to.Cp; pa.y_off = E.pool_tensor >= 0 ? 0 : E.out_off;
    pa.S = L.pool_S; pa.st = L.pool_st; pa.pad = L.pool_pad; pa.C16 = round_up(L.N, 16) / 16;
    lp.steps.push_back(st);
  }

  // a row's global average as its own launch (a row that pools as well averages its pooled map: full_size_pool.cl:71-92 reads pool_tail's PH x PW output)
  void avg_step(int l, const tf2_layer_desc& L) {
    const LayerExec& E = wp->exec[l];
    Launch sa; sa.kind = Launch::AVG; sa.layer = l;
    AvgArgs& aa = sa.avg;
    const TensorPlan& to = T(E.out_tensor);
    const TensorPlan& ta = T(L.pool_en ? E.pool_tensor : E.conv_tensor);
    aa.x = base + ta.offset; aa.y = base + to.offset;
    aa.B = batch; aa.HW = L.PH * L.PW; aa.x_cp = ta.Cp; aa.x_off = 0;
    aa.y_cp = to.Cp; aa.y_off = E.out_off; aa.C = round_up(L.N, 16); aa.mult = L.endpool_mult;
    lp.steps.push_back(sa);
  }

  void l2norm_step(int l) {
    const LayerExec& E = wp->exec[l];
    const PackLayer* pl2 = n.pack_layer(l);
    const TensorPlan& ti = T(E.in_tensor); const TensorPlan& to = T(E.out_tensor);
    Launch st; st.kind = Launch::L2N; st.layer = l;
    L2NormArgs& a = st.l2n;
    a.x = base + ti.offset; a.y = base + to.offset + E.out_off;
    a.a = (const double*)(pk + pl2->off_w); a.b = (const double*)(pk + pl2->off_w2); a.e = (const int32_t*)(pk + pl2->off_bias);
    a.n_pix = batch * ti.H * ti.W; a.C = round_up(n.exec_desc(l).N, 16); a.x_cp = ti.Cp; a.y_cp = to.Cp; a.qs = pl2->max_shift;
    lp.steps.push_back(st);
  }

  // ---- one conv row: the packed entry it runs on (its own, or its alternative of the other tile height), its argument block, its kernel ----
  // The wide-tile alternative (128-row tiles, weight_pack.cpp) where its grid still fills the chip: fewer operand bytes and
  // instructions per MAC; small batches keep the 64-row tiles (more blocks, split-K).  With several batches in flight the
  // other batches' kernels fill the chip, so the wide form pays from a much smaller grid on.
  // The reverse on the 28x28 maps: their 128-row layers have a 64-row alternative (more blocks, split-K) for grids of a few
  // blocks (batch 1-2).
  const PackLayer* conv_entry(int l, const tf2_layer_desc& L, bool allow_alt) const {
    const PackLayer* pl = n.pack_layer(l);
    const PackLayer* pa = (allow_alt && !(L.endpool && avg_fuse_now && pl->TM == 64)) ? n.pack_layer_alt(l) : nullptr;   // (the fused global average runs on the 64-row tiles)
    if (pa) {
      const long blocks128 = ((long)batch * L.OH * L.OW + 127) / 128 * (pa->Np / 128);
      if (pa->TM == 128) { if (blocks128 >= (concurrent ? opts.alt_min_blocks_conc : opts.alt_min_blocks)) pl = pa; }
      else if (blocks128 < opts.alt_narrow_blocks) pl = pa;
      // (test-only, per-row A/B of the in-flight plan: rows forced onto / kept off their alternative tile height)
      if (l < 64 && ((opts.alt_rows >> l) & 1)) pl = pa;
      if (l < 64 && ((opts.noalt_rows >> l) & 1)) pl = n.pack_layer(l);
    }
    return pl;
  }

  // The argument block of row l on the entry pl; answers whether every m-tile's entry list is slabs 0 .. nslab-1 (dense weights).
  bool conv_args(int l, const tf2_layer_desc& L, const PackLayer* pl, Launch& st) {
    const LayerExec& E = wp->exec[l];
    st.kind = Launch::CONV; st.layer = l;
    ConvArgs& ca = st.conv;
    const TensorPlan& ti = T(E.in_tensor); const TensorPlan& tc = T(E.conv_tensor);
    ca.x = base + ti.offset; ca.y = base + tc.offset;
    ca.w = (const int8_t*)(pk + pl->off_w); ca.w2 = (const int8_t*)(pk + pl->off_w2);
    ca.bias = (const int32_t*)(pk + pl->off_bias); ca.alpha = (const int32_t*)(pk + pl->off_alpha);
    ca.beta = (const int32_t*)(pk + pl->off_beta);
    ca.zero = (const int8_t*)(pk + (pl->off_pad ? pl->off_pad : zero_off)); ca.max_ent = pl->max_ent;
    ca.dual = pl->dual;
    set_fast_div((uint32_t)pl->n_mtiles, &ca.mt_m, &ca.mt_s);
    // weight-tile addressing (tf2_internal.h ConvArgs): own storage, or the main entry's tiles of the other height
    {
      const int wins = pl->dual ? 2 : 1;
      const int sTM = pl->w_share ? pl->w_main_TM : pl->TM;            // rows of a storage tile
      ca.w_ent_bytes = wins * sTM * 64; ca.w_win_stride = sTM * 64; ca.w_half_stride = 4096; ca.w_sub_step = 0; ca.e_mt_shl = 0; ca.e_mt_shr = 0;
      if (pl->w_share && sTM == 2 * pl->TM) { ca.w_sub_step = 4096; ca.e_mt_shr = 1; }                       // halves of 128-row tiles
      if (pl->w_share && 2 * sTM == pl->TM) {                                                               // pairs of 64-row tiles
        const int32_t* hd0 = reinterpret_cast<const int32_t*>(n.packed.data() + pl->off_dir);
        const int nent = hd0[pl->n_phases] - hd0[0];
        ca.w_half_stride = nent * ca.w_ent_bytes; ca.e_mt_shl = 1;
      }
    }
    bool dense = false;
    if (pl->kind == KIND_MFMA) {
      ca.hdr = (const int32_t*)(pk + pl->off_hdr); ca.hdr_bytes = (int32_t)pl->hdr_bytes;
      // every m-tile's entry list is slabs 0..nslab-1 (dense weights)?  From the host copy of the image.
      const int32_t* hd = reinterpret_cast<const int32_t*>(n.packed.data() + pl->off_dir);
      dense = true;
      for (int mt = 0; mt < pl->n_mtiles && dense; mt++)
        dense = hd[(size_t)mt * (pl->n_phases + 1) + pl->n_phases] - hd[(size_t)mt * (pl->n_phases + 1)] == pl->nslab;
      ca.ent0 = hd[pl->n_phases] - hd[0];
      // arithmetic gather (tf2_internal.h ConvArgs::dense): no header read in front of the first activation DMAs
      const int taps_l = L.k * L.k;
      ca.cslabs = pl->Cp_in / 64;
      // (long slab lists on large maps pay more for the per-step arithmetic than the shorter prologue saves: VGG16 -7 % with every
      //  layer dense; layers of more than dense_max_slabs slabs whose grid runs in several rounds keep the header tables)
      const long blocks_d = ((long)batch * L.OH * L.OW + 127) / 128 * std::max(1, pl->Np / 128);
      const bool dense_pays = pl->nslab <= opts.dense_max_slabs || blocks_d <= 512;
      if (opts.dense_mode && dense && dense_pays && (pl->n_phases == 1 || pl->dual) && pl->Cp_in % 64 == 0 && pl->nslab == taps_l * ca.cslabs && L.k <= 15) {
        ca.dense = 1;
        set_fast_div((uint32_t)ca.cslabs, &ca.cs_m, &ca.cs_s); set_fast_div((uint32_t)L.k, &ca.kk_m, &ca.kk_s);
      }
    }
    ca.dbg2 = dbg_ptr(l);
    if (opts.dbg) ca.dbg = opts.dbg + (size_t)l * 16;
    ca.n_phases = pl->n_phases; ca.n_mtiles = pl->n_mtiles; ca.Np = pl->Np; ca.nslab = pl->nslab;
    ca.k = L.k; ca.dil = L.dil; ca.n_cchunk = pl->n_cchunk; ca.Cp_half = n.in_layout[l].half;
    ConvGeom& g = ca.g;
    g.H = L.H; g.W = L.W; g.Cp_in = ti.Cp;
    g.OH = L.OH; g.OW = L.OW; g.OHW = L.OH * L.OW;
    set_fast_div((uint32_t)g.OHW, &g.ohw_m, &g.ohw_s); set_fast_div((uint32_t)g.OW, &g.ow_m, &g.ow_s);
    g.stride = L.stride; g.pad_h = L.pad_h; g.pad_w = L.pad_w;
    g.n_pix = batch * L.OH * L.OW;
    const bool direct = E.conv_tensor == E.out_tensor;
    g.y_cp = tc.Cp; g.y_off = direct ? E.out_off : 0;
    g.y_nvalid = round_up(L.N, 16);
    g.relu = L.relu; g.add_relu = L.add_relu; g.has_res = L.add_src >= 0;
    g.fast = pl->fast;
    g.dbl_out = pl->off_dbl != 0;
    if (g.has_res) {
      const TensorPlan& tr = T(E.res_tensor);
      ca.res = base + tr.offset; g.res_cp = tr.Cp; g.res_off = E.res_off;
    }
    g.flags = opts.flags;
    st.TM = pl->TM; st.signed_in = pl->signed_in; st.mul24 = pl->max_shift <= 22;
    return dense;
  }

  // The kernel of an MFMA row whose argument block is filled: ring kernel, in-block split-K (with the layer's global average), conv_pw, conv_pwk
  void conv_select(int l, const tf2_layer_desc& L, const PackLayer* pl, bool dense, Launch& st) {
    const LayerExec& E = wp->exec[l];
    ConvArgs& ca = st.conv; ConvGeom& g = ca.g;
    // small grid + long slab list: the four (or eight) waves of a block split K (conv_mfma_sk.hip)
    const long blocks64 = (long)((g.n_pix + 63) / 64) * pl->n_mtiles;
    const bool sk = pl->TM == 64 && opts.sk_mode != 2 &&
                    (opts.sk_mode == 1 || (blocks64 <= 512 && (long)pl->n_entries * (pl->dual ? 2 : 1) >= 16L * pl->n_mtiles));
    st.sel = sk ? Launch::SEL_SK : Launch::SEL_MFMA2;
    if (pl->TM == 64 && l < 64 && ((opts.sk_rows >> l) & 1)) st.sel = Launch::SEL_SK;              // (test-only per-row switches)
    if (l < 64 && ((opts.nosk_rows >> l) & 1)) st.sel = Launch::SEL_MFMA2;
    st.shape = (int)(concurrent ? opts.sk_s3_blocks_conc : opts.sk_s3_blocks);      // SEL_SK: largest grid on three ring stages
    // the layer's global average inside the launch (conv_mfma_sk AVG): 64-row tiles, one image per pixel tile
    if (avg_fuse_now && L.endpool && !L.pool_en && pl->TM == 64 && g.OHW <= 64 && (g.pad_h | g.pad_w) == 0 && L.concat < 0 &&
        E.conv_tensor != E.out_tensor && !g.dbl_out && g.n_pix == batch * g.OHW) {
      const TensorPlan& to = T(E.out_tensor);
      ca.y = base + to.offset; g.y_cp = to.Cp; g.y_off = E.out_off; g.avg_mult = L.endpool_mult;
      st.sel = Launch::SEL_SK; st.avg_fused = 1;
    } else
    // register-resident pointwise kernel (conv_pw.hip) where the layer qualifies and no other kernel is forced
    if (opts.pw_mode && L.k == 1 && opts.sk_mode != 1 && !pl->w_share && conv_pw_eligible(ca, pl->TM, pl->nslab, L.k, dense ? 1 : 0, opts.pw_slabs, opts.pw_minpix)) st.sel = Launch::SEL_PW;
    // short-K pointwise rows on persistent four-wave blocks (conv_pwk.hip, round 6)
    if (pwk_now(L, st) && !pl->w_share && L.concat < 0 && !(l < 64 && ((opts.nopwk_rows >> l) & 1))) {
      const bool forced = l < 64 && ((opts.pwk_rows >> l) & 1);
      if ((forced || pl->nslab <= opts.pwk_max_slabs) && conv_pwk_eligible(ca, pl->TM, L.k, dense ? 1 : 0, opts.pwk_minpix, opts.pwk_min_units, forced)) { st.sel = Launch::SEL_PWK; st.pwk_slots = opts.pwk_slots; st.pwk_pipe = opts.pwk_pipe; }
    }
  }
  // a 1x1 row on the ring kernel (or, with pwk_sk, the split-K kernel) is one conv_pwk may take in this plan
  bool pwk_now(const tf2_layer_desc& L, const Launch& st) const {
    return opts.pwk_mode && (concurrent || opts.pwk_mode == 2) && !st.avg_fused && (st.sel == Launch::SEL_MFMA2 || (st.sel == Launch::SEL_SK && opts.pwk_sk)) && L.k == 1;
  }

  bool conv_step_on(int l, Launch& st, bool allow_alt) {
    const tf2_layer_desc L = n.exec_desc(l);
    const PackLayer* pl = conv_entry(l, L, allow_alt);
    const bool dense = conv_args(l, L, pl, st);
    if (pl->kind == KIND_MFMA) conv_select(l, L, pl, dense, st);
    else if (pl->kind == KIND_SHIFT) { st.sel = Launch::SEL_SHIFT; st.shape = pl->fast; }      // fast on a shift layer: packed 4-bit filters
    else { set_error("layer " + std::to_string(l) + " has no packed kernel"); return false; }
    return true;
  }
  // argument block + kernel selection of one conv layer; false: the plan fails (the error text is set)
  // (conv_pwk reads a layer's OWN weight tiles: a 1x1 row whose wide-tile alternative shares the main entry's tiles is tried again on
  //  the main entry)
  bool conv_step(int l, Launch& st, bool allow_alt) {
    if (!conv_step_on(l, st, allow_alt)) return false;
    if (allow_alt && pwk_now(n.exec_desc(l), st)) {
      Launch s2;
      if (conv_step_on(l, s2, false) && s2.sel == Launch::SEL_PWK) st = s2;
    }
    return true;
  }
  // the conv_steps of rows l .. l + count - 1 on their own entries (the rows of a shared launch); false: the plan fails
  bool conv_steps(int l, Launch* s, int count) {
    for (int k = 0; k < count; k++)
      if (!conv_step(l + k, s[k], false)) return false;
    return true;
  }

  // ---- three rows (reduce, 3x3, expand) in one launch: what BGroupArgs and BBandArgs share, as an identity bottleneck has it ----
  template <class Args>
  void three_row_args(Args& f, int l, const Launch& s0, const Launch& s1, const Launch& s2) const {
    const ConvArgs& c0 = s0.conv; const ConvArgs& c1 = s1.conv; const ConvArgs& c2 = s2.conv;
    f.x = c0.x; f.mid1 = c0.y; f.mid2 = c1.y; f.y = c2.y;
    f.w1 = c0.w; f.w2 = c1.w; f.w3 = c2.w; f.hdr1 = c0.hdr; f.hdr2 = c1.hdr; f.hdr3 = c2.hdr;
    f.hdr1_bytes = c0.hdr_bytes; f.hdr2_bytes = c1.hdr_bytes; f.hdr3_bytes = c2.hdr_bytes;
    f.tm1 = s0.TM; f.tm2 = s1.TM; f.tm3 = s2.TM;
    f.zero = (const int8_t*)(pk + zero_off); f.zero2 = c1.zero;
    f.dbg = dbg_ptr(l);
    f.B = batch;
    f.relu1 = c0.g.relu; f.relu2 = c1.g.relu; f.relu3 = c2.g.relu; f.add_relu = c2.g.add_relu;
    f.fast1 = c0.g.fast; f.fast2 = c1.g.fast; f.fast3 = c2.g.fast;
    f.dbl1 = c0.g.dbl_out; f.dbl2 = c1.g.dbl_out; f.dbl3 = c2.g.dbl_out;
    f.dual1 = c0.dual; f.dual2 = c1.dual;
    f.res = c2.res; f.has_res = c2.g.has_res; f.res_cp = c2.g.res_cp; f.res_off = c2.g.res_off;      // (the first bottleneck's launches: set by the caller)
    f.y_cp = c2.g.y_cp; f.y_off = c2.g.y_off;
  }

  // ---- the counters of the group launches (conv_bgroup.hip) in the workspace's control area ----
  // the step's first kernel (input preparation) advances the step counter and clears the flag words behind it
  void claim_step_counter() {
    lp.steps[0].prep.epoch_ptr = reinterpret_cast<unsigned*>(base + wp->ctrl_off);
    lp.steps[0].prep.n_flag_words = (int32_t)((wp->ctrl_bytes - 256) / 4);
  }
  // group launches are possible in this plan (one batch at a time: two such kernels sharing CUs could hold each other's slots while
  // their groups wait) and the control area has room for one more launch's flag words
  bool group_slot_free() const {
    return opts.bgroup_mode && !concurrent && wp->ctrl_bytes && groups_fit && 256 + (size_t)(bg_used + 1) * ((batch + 7) / 8 * 8) * 128 <= wp->ctrl_bytes;
  }
  void claim_group_slot(BGroupArgs& f) {
    f.epoch = reinterpret_cast<const unsigned*>(base + wp->ctrl_off);
    f.ctr = reinterpret_cast<unsigned*>(base + wp->ctrl_off + 256) + (size_t)bg_used * ((batch + 7) / 8 * 8) * 32;
    claim_step_counter();
    lp.steps[0].prep.bg_poll_limit = (int32_t)opts.bg_poll_limit; lp.steps[0].prep.bg_withhold = (int32_t)opts.bg_withhold;
    bg_used++; lp.n_groups++;
  }

  // ---- the candidates of a row, in the order rows() asks them ----
  // the first bottleneck of the 56 x 56 stage (shortcut | reduce, 3x3, expand) as ONE launch of independent row bands at two blocks per
  // CU (conv_bfirst.hip, round 6): the form for batches in flight (bfirst=2: one batch at a time as well, instead of the group launch)
  bool try_bfirst(int l) {
    return opts.bfirst_mode && (concurrent || opts.bfirst_mode == 2) && batch >= opts.bfirst_min && first_bottleneck(l, Launch::SEL_BFIRST);
  }
  // ... the same rows as a group launch (conv_bgroup56f_kernel), one batch at a time
  bool try_group_first(int l) { return group_slot_free() && batch >= opts.bgroup_min56f && first_bottleneck(l, Launch::SEL_BGROUPF); }
  bool first_bottleneck(int l, Launch::Sel sel) {
    if (!n.bgroup_first_at(l)) return false;
    Launch s[4];                                               // s[0]: the projection shortcut, computed inside the launch (the residual never leaves it)
    if (!conv_steps(l, s, 4)) return give_up();
    if (!(s[0].conv.dense && s[1].conv.dense && s[2].conv.dense && s[3].conv.dense)) return false;
    if (sel == Launch::SEL_BFIRST && !(s[1].TM == 64 && s[2].TM == 64 && s[3].TM == 64 && !s[2].conv.dual && s[1].conv.dual == s[3].conv.dual && s[0].conv.dual == s[1].conv.dual)) return false;
    Launch st; st.kind = Launch::CONV; st.sel = sel; st.layer = l;
    BGroupArgs& f = st.bgroup;
    three_row_args(f, l, s[1], s[2], s[3]);
    const ConvArgs& cs = s[0].conv;
    f.res = nullptr; f.has_res = 1; f.res_cp = 0; f.res_off = 0;
    f.dbl3 = 0; f.dual2 = 0; f.dual3 = s[3].conv.dual; f.avg_mult = 0;
    f.ws = cs.w; f.hdrs = cs.hdr; f.hdrs_bytes = cs.hdr_bytes; f.tms = s[0].TM; f.relu_s = cs.g.relu; f.fast_s = cs.g.fast;
    f.ys = cs.y; f.ys_cp = cs.g.y_cp; f.keep_s = wp->keep_all ? 1 : 0;
    if (sel == Launch::SEL_BGROUPF) claim_group_slot(f);
    mark_done(l + 1, l + 3);
    lp.steps.push_back(st);
    return true;
  }

  // a fire module (squeeze + the merged expands) as ONE launch of independent row bands (conv_fire.hip)
  bool try_fire(int l) {
    const tf2_layer_desc L = n.exec_desc(l);
    if (!(opts.fire_mode && n.fire_at(l) && (opts.fire_mode == 1 || L.W >= 28) &&
          (!n.layers[l + 1].pool_en || opts.fire_pool >= 2 || (opts.fire_pool == 1 && L.W >= 56)))) return false;
    Launch s[2];
    if (!conv_steps(l, s, 2)) return give_up();
    const PackLayer* p1 = n.pack_layer(l + 1);
    if (!(s[0].conv.dense && s[0].TM == 64 && s[1].TM == p1->TM)) return false;
    Launch st; st.kind = Launch::CONV; st.sel = Launch::SEL_FIRE; st.layer = l;
    FireArgs& f = st.fire;
    const ConvArgs& c0 = s[0].conv; const ConvArgs& c1 = s[1].conv;
    f.x = c0.x; f.mid = c0.y; f.y = c1.y; f.w1 = c0.w; f.w2 = c1.w; f.hdr1 = c0.hdr; f.hdr2 = c1.hdr; f.hdr2_bytes = c1.hdr_bytes;
    f.ent2 = reinterpret_cast<const int32_t*>(pk + p1->off_entries); f.dir2 = reinterpret_cast<const int32_t*>(pk + p1->off_dir); f.n_ent2 = (int32_t)p1->n_entries;
    f.zero = (const int8_t*)(pk + zero_off); f.zero2 = c1.zero;
    f.tm1 = s[0].TM; f.tm2 = s[1].TM; f.B = batch; f.H = L.H; f.W = L.W; f.Cin = L.C; f.Sp = round_up(L.N, 16); f.N2 = p1->Np;
    f.relu1 = c0.g.relu; f.relu2 = c1.g.relu; f.fast1 = c0.g.fast; f.fast2 = c1.g.fast; f.dbl1 = c0.g.dbl_out; f.dual1 = c0.dual;
    f.keep_mid = wp->keep_all ? 1 : 0; f.mid_cp = c0.g.y_cp; f.y_cp = c1.g.y_cp; f.y_off = c1.g.y_off; f.y_nvalid = c1.g.y_nvalid;
    f.dbg = dbg_ptr(l);
    // the pool behind the expands inside the launch where its form fits (3x3 / 2 / pad 0 in ceil mode behind a ReLU) -- one batch at a
    // time (fire_pool=3, the default; 4: always): its blocks hold 100-108 KB of LDS, one per CU, and with batches in flight that costs
    // more (317 k against 334-345 k img/s) than the pool launch it saves; alone it is 25.3 us against 19 + 9.2 (fire3), 12.6 against
    // 16.2 + 6.7 (fire5): profiles/r05_experiments.txt item 22
    const tf2_layer_desc L1 = n.exec_desc(l + 1);
    f.pool = 0;
    if (L1.pool_en && (opts.fire_pool == 4 || (opts.fire_pool == 3 && !concurrent)) && L1.pool_S == 3 && L1.pool_st == 2 && L1.pool_pad == 0 && c1.g.relu && !c1.g.dbl_out &&
        L1.PH == (L.H - 2) / 2 + 1 && L1.PW == L1.PH && c1.g.y_nvalid == f.N2 &&
        conv_fire_geometry(f.H, f.W, f.Cin, f.Sp, f.N2, f.tm1, f.tm2, f.dual1, 1, nullptr, nullptr)) {
      const TensorPlan& to1 = T(wp->exec[l + 1].out_tensor);
      f.pool = 1; f.PH = L1.PH; f.PW = L1.PW; f.yp = base + to1.offset; f.yp_cp = to1.Cp; f.yp_off = wp->exec[l + 1].out_off;
    }
    if (!conv_fire_geometry(f.H, f.W, f.Cin, f.Sp, f.N2, f.tm1, f.tm2, f.dual1, f.pool, &f, nullptr)) return false;
    pair_done[l + 1] = 1;
    lp.steps.push_back(st);
    if (L1.pool_en && !f.pool) { const TensorPlan& tc1 = T(wp->exec[l + 1].conv_tensor); pool_step(l + 1, tc1, base + tc1.offset, L1.OH, L1.OW); }
    return true;
  }

  // an identity bottleneck as ONE launch of independent row bands (conv_bband.hip): no exchange between blocks, so it may share
  // the chip with anything -- the form for batches in flight (TF2_AMD_BBAND=2: one batch at a time as well, instead of the groups)
  bool try_bband(int l) {
    const tf2_layer_desc L = n.exec_desc(l);
    const int band_rows = concurrent ? opts.bband_rows : opts.bband_rows_alone;
    if (!(opts.bband_mode && (concurrent || (opts.bband_alone_maps & (L.H >= 28 ? 2 : 4))) && batch >= opts.bband_min && n.bband_at(l, band_rows))) return false;
    Launch s[3];
    if (!conv_steps(l, s, 3)) return give_up();
    if (!(s[0].conv.dense && s[1].conv.dense && s[2].conv.dense)) return false;
    Launch st; st.kind = Launch::CONV; st.sel = Launch::SEL_BBAND; st.layer = l;
    BBandArgs& f = st.bband;
    three_row_args(f, l, s[0], s[1], s[2]);
    f.H = L.H; f.W = L.W; f.R = std::min(conv_bband_pick_rows(L.W, L.N, f.dual1, f.dual2, band_rows, opts.bband_rows_dd), L.H);
    f.tiles_per_img = (L.H + f.R - 1) / f.R;
    f.keep_mid = wp->keep_all ? 1 : 0;
#ifdef TF2_PROBES
    if (opts.flags & 16384) f.probe = 1;              // (probe, conv_bband.hip: one column tile fewer in phases 1-2)
#endif
    st.bg_c = L.C; st.bg_m = L.N;
    mark_done(l + 1, l + 2);
    lp.steps.push_back(st);
    return true;
  }

  // an identity bottleneck of a small map as ONE launch, eight blocks per image (conv_bgroup.hip)
  bool try_bgroup(int l) {
    const tf2_layer_desc L = n.exec_desc(l);
    if (!(group_slot_free() && n.bgroup_at(l) && batch >= (L.H == 7 ? opts.bgroup_min7 : L.H == 28 ? opts.bgroup_min28 : opts.bgroup_min14))) return false;
    Launch s[3];
    if (!conv_steps(l, s, 3)) return give_up();
    if (!(s[0].conv.dense && s[1].conv.dense && s[2].conv.dense && (!n.layers[l + 2].endpool || s[2].avg_fused))) return false;
    Launch st; st.kind = Launch::CONV; st.sel = Launch::SEL_BGROUP; st.layer = l;
    BGroupArgs& f = st.bgroup;
    three_row_args(f, l, s[0], s[1], s[2]);
    f.dual3 = s[2].conv.dual; f.avg_mult = s[2].conv.g.avg_mult;
    st.bg_hw = L.H; st.bg_c = L.C; st.bg_m = L.N;
    claim_group_slot(f);
    mark_done(l + 1, l + 2);
    // the 14 x 14 stage's identity bottlenecks follow one another: the groups of the previous launch carry on with this one
    // (its roll-call row doubles as the meeting "input complete")
    if (opts.bgroup_chain > 1 && !lp.steps.empty() && !f.dbg) {
      Launch& pv = lp.steps.back();
      const int pn = pv.bg_chain.empty() ? 1 : (int)pv.bg_chain.size();
      if (pv.kind == Launch::CONV && pv.sel == Launch::SEL_BGROUP && pv.bg_hw == L.H && pv.layer + 3 * pn == l && f.dual1 == pv.bgroup.dual1 && f.dual2 == pv.bgroup.dual2 && !pv.bg_chain_last().avg_mult && pn < std::min(kBgMaxChain, opts.bgroup_chain) &&
          !pv.bgroup.dbg && f.x == pv.bg_chain_last().y && f.has_res && f.res == f.x && f.res_off == 0 && pv.bg_chain_last().y_off == 0 &&
          f.res_cp == pv.bg_chain_last().y_cp) {
        if (pv.bg_chain.empty()) pv.bg_chain.push_back(pv.bgroup);
        pv.bg_chain.push_back(f);
        return true;
      }
    }
    lp.steps.push_back(st);
    return true;
  }

  // ---- the plain row: one conv launch of its own kernel, or of a kernel that takes the row over ----
  // A row and its only consumer (a 3x3 and the 1x1 expand, PackLayer::fuse_next) run as ONE conv_bneck launch in this plan?
  // A fused launch needs enough row bands to fill the chip (one block per band): small batches run the two layers on their own
  // (128-channel pairs: 42.6 against 46.8 us at batch 64 one batch at a time, but 0.62 against 0.51 us per further image --
  //  with batches in flight the two separate launches win)
  // conv_bneck.hip's phase 2 addresses the expand's output (the tensor its conv writes) and its residual as kernel-argument base + ONE
  // 32-bit byte offset (pixel * Cp + channel offset; the input and the intermediate map use 64-bit addresses): a pair whose expand
  // tensors reach 2^32 bytes runs as the two separate launches (conv_pwk_eligible has the same guard)
  bool bneck_fuses_now(const tf2_layer_desc& L, const PackLayer* pl) const {
    if (pl->fuse_next <= 0) return false;
    const int bn_TN = pl->TM == 64 ? 256 : 128;
    const int bn_R = std::min(bn_TN / L.W, L.H);
    auto below_4g = [&](int tid) { return tid < 0 || (unsigned long long)T(tid).bytes < (1ull << 32); };
    const bool bneck_fits = below_4g(wp->exec[pl->fuse_next].conv_tensor) && below_4g(wp->exec[pl->fuse_next].res_tensor);
    return bneck_fits && (long)batch * ((L.H + bn_R - 1) / bn_R) >= opts.bneck_min_blocks && !(concurrent && pl->TM == 128 && opts.bneck_min_blocks > 1);
  }

  // conv_fc.hip takes the row over (Net::fc_at) where the workspace has the room for its partial sums
  void fc_takeover(int l, Launch& st) {
    const PackLayer* pm = n.pack_layer(l);
    if (!((opts.fc_mode || pm->fc4) && n.fc_at(l, batch) && wp->scratch_bytes)) return;
    Launch sc;
    if (!(conv_step(l, sc, false) && pm->TM == sc.TM && conv_fc_scratch_bytes(pm->Np, pm->nslab, pm->dual, batch) <= wp->scratch_bytes)) return;
    const ConvArgs& c = sc.conv;
    FcArgs& f = sc.fc;
    f.x = c.x; f.y = c.y; f.w = c.w; f.hdr = c.hdr; f.hdr_bytes = c.hdr_bytes; f.tm = sc.TM;
    f.part = reinterpret_cast<int32_t*>(base + wp->scratch_off);
    f.B = batch; f.nslab = pm->nslab; f.K = pm->nslab * 64; f.Np = pm->Np;
    f.ksplit = conv_fc_pick_ksplit(pm->Np, pm->nslab); f.slabs_per_split = (pm->nslab + f.ksplit - 1) / f.ksplit;
    f.dual = c.dual; f.relu = c.g.relu; f.fast = c.g.fast; f.dbl = c.g.dbl_out;
    f.fc4 = pm->fc4; f.n_cls = pm->n_cls; f.chunks = (batch + 31) / 32;
    f.lut = pk + pm->off_lut; f.cls = pk + pm->off_cls;
    f.y_cp = c.g.y_cp; f.y_off = c.g.y_off; f.y_nvalid = c.g.y_nvalid;
    sc.sel = Launch::SEL_FC; sc.avg_fused = 0;
    st = sc;
  }

  // conv_c3.hip takes the row over (Net::c3_at) where its grid is large enough; answers whether the launch pools as well
  bool c3_takeover(int l, const tf2_layer_desc& L, Launch& st) {
    if (!(opts.c3_mode && n.c3_at(l))) return false;
    const LayerExec& E = wp->exec[l];
    const PackLayer* pm = n.pack_layer(l);
    int th = 0, tw = 0;
    conv_c3_pick_tile(L.H, L.W, &th, &tw);
    // the layer's 2x2 / stride 2 / pad 0 max pool inside the launch (conv_c3.hip POOL: tiles of TH x 32 pixels): ReLU layers whose
    // map the 32-column tiling fits; the conv map is then neither written nor read back, and the pool launch is gone
    const bool pool_in = opts.c3_pool && L.pool_en && L.relu && L.pool_S == 2 && L.pool_st == 2 && L.pool_pad == 0 && E.conv_tensor != E.out_tensor &&
                         L.PH == (L.OH + 1) / 2 && L.PW == (L.OW + 1) / 2 && conv_c3_pick_tile_pool(L.H, L.W, &th, &tw);
    const int tiles_x = (L.W + tw - 1) / tw, tiles = tiles_x * ((L.H + th - 1) / th);
    // 128 output channels per block (two waves per SIMD, the accumulators of four column tiles per wave) unless the layer has
    // 64-row tiles only, or is a one-window layer whose 128-channel grid would leave half the chip idle (VGG16's 14 x 14 maps at
    // batch 32: 29 / 33 us against 33 / 37; two-window rows spill at the 128 registers of the 64-channel form)
    int tmk = pm->Np % 128 == 0 ? 128 : 64;
    // one-window layers of 256+ channels whose 256-channel grid still covers the chip: two row tiles per wave (a B fragment feeds
    // two MFMAs: half the LDS reads per MFMA, half the blocks' prologues)
    if (tmk == 128 && !pm->dual && pm->Np % 256 == 0 && (long)batch * tiles * (pm->Np / 256) >= opts.c3_min256) tmk = 256;
    else if (tmk == 128 && !pm->dual && (long)batch * tiles * (pm->Np / 128) < 256) tmk = 64;
    if (opts.c3_mode == 2) tmk = 64; else if (opts.c3_mode == 3 && pm->Np % 128 == 0) tmk = 128;       // (experiments)
    Launch sc;
    if (!((long)batch * tiles * (pm->Np / tmk) >= opts.c3_min_blocks && conv_step(l, sc, false) && pm->TM == sc.TM)) return false;
    const ConvArgs& c = sc.conv;
    C3Args& f = sc.c3;
    f.x = c.x; f.y = c.y; f.w = c.w; f.hdr = c.hdr; f.hdr_bytes = c.hdr_bytes; f.zero2 = c.zero; f.tm = sc.TM; f.tmk = tmk;
    f.dbg = dbg_ptr(l);
    f.B = batch; f.H = L.H; f.W = L.W; f.C = L.C; f.M = pm->Np; f.x_cp = c.g.Cp_in;
    f.TH = th; f.TW = tw; f.tiles_x = tiles_x; f.tiles_per_img = tiles;
    set_fast_div((uint32_t)tw, &f.tw_m, &f.tw_s); set_fast_div((uint32_t)(tw + 2), &f.hc_m, &f.hc_s);
    set_fast_div((uint32_t)tiles_x, &f.tx_m, &f.tx_s); set_fast_div((uint32_t)tiles, &f.tpi_m, &f.tpi_s);
    f.relu = c.g.relu; f.fast = c.g.fast; f.dbl = c.g.dbl_out; f.dual = c.dual;
    f.y_cp = c.g.y_cp; f.y_off = c.g.y_off; f.y_nvalid = c.g.y_nvalid;
    if (pool_in) {
      const TensorPlan& to = T(E.out_tensor);
      f.pool = 1; f.PH = L.PH; f.PW = L.PW; f.y = base + to.offset; f.y_cp = to.Cp; f.y_off = E.out_off;
    }
    f.w9 = conv_c3_takes_w9(f, opts.c3_w9) ? 1 : 0;
    sc.sel = Launch::SEL_C3;
    st = sc;
    return pool_in;
  }

  // conv_img.hip takes the row over (Net::img_at): with batches in flight (img=2: one batch at a time as well -- rows() asks the group
  // launches first, so they keep their rows) from batch img_min on; img_rows / noimg_rows (test-only) decide a row whatever img / img_min say.
  // The kernel forms every tensor address in 64 bits; the 2^32 guard keeps its launches inside what its tests cover.
  void img_takeover(int l, const tf2_layer_desc& L, Launch& st) {
    if (l < 64 && ((opts.noimg_rows >> l) & 1)) return;
    const bool forced = l < 64 && ((opts.img_rows >> l) & 1);
    if (!(forced || (opts.img_mode && (concurrent || opts.img_mode == 2) && batch >= opts.img_min))) return;
    if (!n.img_at(l)) return;
    const PackLayer* pm = n.pack_layer(l);
    Launch sc;
    if (!(conv_step(l, sc, false) && sc.TM == 64 && pm->TM == 64)) return;
    const ConvArgs& c = sc.conv;
    if ((long long)batch * L.H * L.W * std::max(c.g.Cp_in, c.g.y_cp) >= (1ll << 32) || c.g.Cp_in != L.C || c.g.has_res || c.g.avg_mult) return;
    ImgArgs& f = sc.img;
    f.x = c.x; f.y = c.y; f.w = c.w; f.hdr = c.hdr; f.hdr_bytes = c.hdr_bytes; f.zero = c.zero;
    f.hdr_used = round_up((5 + pm->n_phases) * 64 * 4, 1024);
    f.B = batch; f.HW = L.H; f.C = L.C; f.k = L.k; f.n_mtiles = pm->n_mtiles;
    f.dual = c.dual; f.relu = c.g.relu; f.fast = c.g.fast; f.dbl = c.g.dbl_out;
    f.y_cp = c.g.y_cp; f.y_off = c.g.y_off; f.y_nvalid = c.g.y_nvalid;
    if (f.hdr_used > f.hdr_bytes || conv_img_lds_bytes(f.HW, f.C, f.k, (size_t)f.hdr_used) > 160 * 1024) return;
    sc.sel = Launch::SEL_IMG; sc.avg_fused = 0;
    st = sc;
  }

  // this 3x3 + its only consumer (the 1x1 expand) in one launch (conv_bneck.hip); the expand's argument block supplies the second half
  bool bneck_fuse(int l, const tf2_layer_desc& L, const PackLayer* pl, Launch& st) {
    fused_done[pl->fuse_next] = 1;
    Launch sb;
    if (!conv_step(pl->fuse_next, sb, false)) return false;
    const PackLayer* pb = n.pack_layer(pl->fuse_next);
    BneckArgs& f = st.bneck;
    const ConvArgs& ca = st.conv; const ConvArgs& cb = sb.conv;
    f.x = ca.x; f.y_mid = ca.y; f.ymid_cp = ca.g.y_cp;
    f.w1 = ca.w; f.hdr1 = ca.hdr; f.hdr1_used = round_up((5 + pl->n_phases) * pl->TM * 4, 1024);
    f.dual1 = pl->dual; f.fast1 = pl->fast; f.relu1 = ca.g.relu;
    f.w2 = cb.w; f.hdr2 = cb.hdr; f.hdr2_bytes = cb.hdr_bytes; f.hdr2_used = round_up((5 + pb->n_phases) * pb->TM * 4, 1024);
    f.dual2 = pb->dual; f.fast2 = pb->fast; f.relu2 = cb.g.relu;
    f.y = cb.y; f.y_cp = cb.g.y_cp; f.y_off = cb.g.y_off; f.y_nvalid = cb.g.y_nvalid;
    f.res = cb.res; f.res_cp = cb.g.res_cp; f.res_off = cb.g.res_off; f.add_relu = cb.g.add_relu; f.has_res = cb.g.has_res;
    f.zero = ca.zero; f.keep_mid = wp->keep_all ? 1 : 0; f.dbl_mid = pl->off_dbl != 0; f.dbl_out = pb->off_dbl != 0;
    f.rnn = n.res_nonneg_single_clamp(pl->fuse_next) ? 1 : 0;
    f.B = batch; f.H = L.H; f.W = L.W; f.probe = opts.flags;
    f.dbg = dbg_ptr(l);
    set_fast_div((uint32_t)L.W, &f.w_m, &f.w_s); set_fast_div((uint32_t)(L.W + 2), &f.wp_m, &f.wp_s);
    const int TN = pl->TM == 64 ? 256 : 128;      // pixel capacity of a block (wave tile 32 x 64)
    f.R = std::min(TN / L.W, L.H);
    f.tiles_per_img = (L.H + f.R - 1) / f.R;
    st.sel = Launch::SEL_BNECK; st.shape = TN;
    return true;
  }

  // this row (on the kernel `from`) and the next in one launch `to`, where both select `from` and the kernel's own eligibility function
  // accepts them.  false: the plan fails
  template <class Eligible>
  bool pair_with_next(int l, Launch& st, Launch::Sel from, Launch::Sel to, Eligible eligible) {
    if (st.sel != from) return true;
    Launch sb;
    if (!conv_step(l + 1, sb, true)) return false;
    if (sb.sel == from && eligible(sb)) {
      st.conv2 = sb.conv; st.sel = to;
      if (to == Launch::SEL_PWKPAIR) st.TM2 = sb.TM;
      fused_done[l + 1] = 1; pair_done[l + 1] = 1;
    }
    return true;
  }
  // independent neighbouring rows (Net::pair_candidate; pairs do not chain) in one launch.  false: the plan fails
  bool pair_forms(int l, Launch& st) {
    if (!n.pair_candidate(l) || (l >= 2 && n.pair_candidate(l - 1))) return true;
    // two rows of one ring-kernel instantiation
    if (!pair_with_next(l, st, Launch::SEL_MFMA2, Launch::SEL_PAIR, [&](const Launch& sb) { return conv_mfma2_pair_eligible(st.conv, st.TM, sb.conv, sb.TM); })) return false;
    // ... two conv_pwk rows of one instantiation (rows 11 | 12 with pwk=1)
    if (!pair_with_next(l, st, Launch::SEL_PWK, Launch::SEL_PWKPAIR, [&](const Launch& sb) { return conv_pwk_pair_eligible(st.conv, sb.conv); })) return false;
    // ... the same for two split-K rows (small batches: a stage's shortcut convolution and the first 1x1 of its first bottleneck on the
    // 14 x 14 / 7 x 7 maps are both split-K launches of a few dozen blocks; round 6: batch-1 latency, two launches less)
    if (st.avg_fused || l + 1 >= nl - 1) return true;
    return pair_with_next(l, st, Launch::SEL_SK, Launch::SEL_SKPAIR, [&](const Launch& sb) {
      return !sb.avg_fused && sb.shape == st.shape && conv_mfma_sk_pair_eligible(st.conv, sb.conv, opts.sk8_blocks, st.shape); });
  }

  // conv_stem.hip takes layer 0 (Net::stem_selected), with the layer's max pool where its form fits.  false: the plan fails
  bool stem_step(const tf2_layer_desc& L, const PackLayer* pl, Launch& st) {
    const LayerExec& E = wp->exec[0];
    const ConvArgs& ca = st.conv;
    StemArgs& f = st.stem;
    f.x = ca.x; f.y = ca.y; f.w = (const int8_t*)(pk + pl->off_w2); f.hdr = ca.hdr; f.zero = ca.zero;
    f.unit = pl->off_unit ? (const int8_t*)(pk + pl->off_unit) : nullptr;
    f.hdr_used = round_up((5 + pl->n_phases) * 64 * 4, 1024);
    f.B = batch; f.H = L.H; f.W = L.W; f.OH = L.OH; f.OW = L.OW;
    set_fast_div((uint32_t)L.OW, &f.ow_m, &f.ow_s); set_fast_div((uint32_t)std::max(1, L.PW), &f.pw_m, &f.pw_s);
    f.relu = ca.g.relu; f.fast = ca.g.fast; f.y_cp = ca.g.y_cp; f.y_off = ca.g.y_off; f.y_nvalid = ca.g.y_nvalid; f.dbl_out = ca.g.dbl_out; f.probe = opts.flags; f.dbg2 = dbg_ptr(0);
    // rows per block: the fewest rounds of (two blocks per CU) x rows; two blocks must share a CU's 160 KiB
    long best = -1;
    for (int R = 2; R <= 8; R++) {
      if (2 * conv_stem_lds_bytes(pl->off_unit ? 1 : pl->n_phases, R, L.W, (size_t)f.hdr_used) > 160 * 1024) break;
      const long blocks = (long)batch * ((L.OH + R - 1) / R);
      const long cost = ((blocks + 511) / 512) * R;
      if (best < 0 || cost < best || (cost == best && R == 7)) { best = cost; f.R = R; }
    }
    // the layer's 3x3 / stride 2 / pad 1 max pool in the same launch (conv_stem_pool_kernel): pooled rows per block = the most
    // that lets two blocks share a CU
    if (opts.stem_pool && L.pool_en && L.pool_S == 3 && L.pool_st == 2 && L.pool_pad == 1 && pl->off_unit &&
        L.PH == (L.OH + 1) / 2 && L.PW == (L.OW + 1) / 2 && L.N == 64 && E.conv_tensor != E.out_tensor) {
      int rows = 0;
      for (int k = 1; k <= 8; k++)
        if (2 * conv_stem_pool_lds_bytes(k, L.W, L.OW, (size_t)f.hdr_used) <= 160 * 1024) rows = k;
      if (rows >= 2) {
        // small batches: fewer pooled rows per block while the grid has fewer than ~192 blocks (batch 1: 19 bands x 2 channel halves = 38 blocks of 7 conv
        // rows on 256 CUs; with one pooled row per block 112 blocks of 3 -- a third more conv rows in all, a shorter chain: round 6, stem_pk_small)
        if (opts.stem_pk_small)
          while (rows > 1 && (long)batch * 2 * ((L.PH + rows - 1) / rows) < 192) rows--;
        const TensorPlan& to = T(E.out_tensor);
        f.yp = base + to.offset; f.PH = L.PH; f.PW = L.PW; f.yp_cp = to.Cp; f.yp_off = E.out_off; f.pk = rows;
        f.bands_per_img = (L.PH + rows - 1) / rows; f.R = 2 * rows + 1;
        stem_pool_fused = true;
      }
    }
    if (!stem_pool_fused) {
      if (best < 0) { set_error("conv_stem does not fit this first layer; run with TF2_AMD_STEM=0"); return false; }
      f.bands_per_img = (L.OH + f.R - 1) / f.R;
    }
    st.sel = Launch::SEL_STEM; st.shape = pl->n_phases;
    return true;
  }

  // the last layer of a classifier (1x1 map, split-K kernel) stores the dense logits [batch][N] itself: no copy kernel
  void logits_direct(int l, const tf2_layer_desc& L, Launch& st) {
    if (!(l == nl - 1 && !wp->keep_all && !wp->outputs_kept && st.sel == Launch::SEL_SK && !L.pool_en && !L.endpool && L.concat < 0 &&
          L.PH * L.PW == 1 && (L.N % 16 == 0 || L.N % 16 == 8))) return;
    st.conv_direct = st.conv;
    ConvGeom& gd = st.conv_direct.g;
    gd.y_cp = L.N; gd.y_off = 0; gd.y_nvalid = L.N / 16 * 16; gd.y_tail = L.N % 16;
    lp.logits_direct = (int)lp.steps.size();
  }

  // a 3x3 / stride 1 first layer on the 3-channel image: input preparation and the pointwise layer over the im2col tile in ONE
  // launch (conv_first_kernel: the tile stays in LDS); the step's first launch then belongs to table row 0
  bool first_fuse(const tf2_layer_desc& L, const PackLayer* pl, const Launch& st) {
    const LayerExec& E = wp->exec[0];
    if (!(n.im2col0 && opts.first_fuse && (st.sel == Launch::SEL_PW || st.sel == Launch::SEL_MFMA2 || st.sel == Launch::SEL_SK) &&
          st.TM == 64 && pl->TM == 64 && pl->n_mtiles == 1 && pl->nslab == 1 && pl->n_entries == 1 && !pl->w_share &&
          (pl->n_phases == 1 || pl->dual) && !L.endpool && L.concat < 0 && L.add_src < 0 && (L.pool_en != 0) == (E.conv_tensor != E.out_tensor))) return false;
    Launch& s0 = lp.steps[0];
    const int hdr_used = round_up((5 + pl->n_phases) * 64 * 4, 1024);
    int R = 0, WS = 0; size_t lds = 0;
    const ConvArgs& ca = st.conv;
    // ... and, with a 3x3 / stride 2 pool behind a ReLU (SqueezeNet 1.1's front: stride-2 conv1 + pool1), the pool as well
    // (conv_first_pool_kernel: the conv map stays in LDS)
    // (the kernels index with 32 bits: the launchers refuse batches beyond that, so the plan keeps the separate launches there)
    const bool idx32 = (long long)batch * L.OH * L.OW * 64 < (1ll << 31) && (long long)batch * 3 * n.nd.image_h * n.nd.image_w < (1ll << 31);
    const bool plain = idx32 && !L.pool_en && s0.kind == Launch::PREP && conv_first_fits(s0.prep, &R, &WS, &lds, hdr_used);
    const bool pooled = idx32 && L.pool_en && opts.first_pool && s0.kind == Launch::PREP && !ca.g.dbl_out && ca.g.y_nvalid == 64 &&
                        conv_first_pool_fits(s0.prep, L.pool_S, L.pool_st, L.pool_pad, L.PH, L.PW, ca.g.relu, hdr_used, &R, &WS, &lds);
    if (!plain && !pooled) return false;
    FirstArgs& f = s0.first;
    f.w = ca.w; f.hdr = ca.hdr; f.y = ca.y; f.im = s0.prep.y;
    f.hdr_used = hdr_used; f.dual = ca.dual; f.relu = ca.g.relu; f.fast = ca.g.fast; f.dbl = ca.g.dbl_out;
    f.y_cp = ca.g.y_cp; f.y_off = ca.g.y_off; f.y_nvalid = ca.g.y_nvalid; f.keep = wp->keep_all ? 1 : 0;
    f.pool = pooled ? 1 : 0;
    if (pooled) {
      const TensorPlan& to = T(E.out_tensor);
      f.yp = base + to.offset; f.PH = L.PH; f.PW = L.PW; f.ppad = L.pool_pad; f.yp_cp = to.Cp; f.yp_off = E.out_off;
    }
    s0.sel = Launch::SEL_FIRST; s0.layer = 0;
    return true;
  }

  // a conv row that no shared launch took: its own launch (+ its pool and its global average where no kernel fused them)
  void plain_row(int l) {
    const tf2_layer_desc L = n.exec_desc(l);
    const LayerExec& E = wp->exec[l];
    const PackLayer* pl = n.pack_layer(l);
    const bool fuse_now = bneck_fuses_now(L, pl);
    Launch st;
    if (!conv_step(l, st, !fuse_now)) { give_up(); return; }     // the fused launch needs the pair's own (one m-tile) entries
    if (!fuse_now) fc_takeover(l, st);
    if (pl->fc4 && st.sel != Launch::SEL_FC) { give_up("layer " + std::to_string(l) + " is packed as 4-bit codes (fc4) but conv_fc cannot take it"); return; }
    const bool c3_pool_fused = !fuse_now && st.sel != Launch::SEL_FC && c3_takeover(l, L, st);
    if (!fuse_now && st.sel != Launch::SEL_FC && st.sel != Launch::SEL_C3 && !st.avg_fused) img_takeover(l, L, st);
    if (fuse_now && !bneck_fuse(l, L, pl, st)) { give_up(); return; }
    if (opts.pair_mode && !fuse_now && !pair_forms(l, st)) { give_up(); return; }
    if (l == 0 && stem && !stem_step(L, pl, st)) { give_up(); return; }
    logits_direct(l, L, st);
    if (l == 0 && !fuse_now && first_fuse(L, pl, st)) return;
    lp.steps.push_back(st);
    const TensorPlan& tc = T(E.conv_tensor);
    if (L.pool_en && !(l == 0 && stem_pool_fused) && !(c3_pool_fused && st.sel == Launch::SEL_C3)) pool_step(l, tc, base + tc.offset, L.OH, L.OW);
    // (no fused pool takes a row that averages as well: conv_stem's image is not packed for it -- weight_pack.cpp --, c3_at, fire_at and
    //  the conv_first form refuse it, and the split-K / group averages read the conv map)
    if (L.endpool && !st.avg_fused) avg_step(l, L);
  }

  // every table row, in order
  bool rows() {
    for (int l = 0; l < nl && !failed; l++) {
      const PackLayer* pl = n.pack_layer(l);
      if (pl->merged_into >= 0) continue;                      // computed by the merged launch of the row in front of it
      if (n.layers[l].ipool == 2) { l2norm_step(l); continue; }
      if (n.layers[l].ipool) { const TensorPlan& ti = T(wp->exec[l].in_tensor); pool_step(l, ti, base + ti.offset, ti.H, ti.W); continue; }
      if (pl->fused_into >= 0 && fused_done[l]) continue;      // computed by the launch of layer pl->fused_into (conv_bneck.hip)
      if (pair_done[l]) continue;                              // computed by the pair launch of layer l - 1 (or a group launch)
      // THE ORDER OF THE CANDIDATES IS BEHAVIOUR: the first that takes the row has it.  A candidate that builds its rows' conv_steps
      // and then finds them ineligible has changed nothing, and the next is asked (the 56 x 56 stage's first bottleneck that
      // conv_bfirst refuses may still run as the group launch, or row by row).
      if (try_bfirst(l) || try_group_first(l) || try_fire(l) || try_bband(l) || try_bgroup(l)) continue;
      plain_row(l);
    }
    return !failed;
  }

  // ---- post-passes over the finished step list ----
  // The -128 flags of the input preparation (round 6): where the step starts as [prep_rewrite3_rows_kernel][conv_stem_pool_kernel][conv_bfirst_kernel],
  // the preparation reports per image whether a quantised element is -128 (words 16 .. 16 + batch of the workspace's control header), the stem's
  // blocks read their image's word instead of scanning their input tile behind a second barrier (0.9 of a block's 9.8 us), and conv_bfirst --
  // the launch behind the stem -- clears the words for the next step.  A fresh (or re-used) workspace may hold anything there: a non-zero word
  // only sends the first step's blocks down the path that is exact for every image.
  void q128_flags_pass() {
    if (!(opts.q128_flags && lp.steps.size() >= 3 && wp->ctrl_bytes >= 256 && batch <= 48 && lp.steps[0].kind == Launch::PREP && lp.steps[0].sel != Launch::SEL_FIRST &&
          prep_takes_rows_kernel(lp.steps[0].prep) && lp.steps[1].kind == Launch::CONV && lp.steps[1].sel == Launch::SEL_STEM && lp.steps[1].stem.yp &&
          lp.steps[1].layer == 0 && lp.steps[2].kind == Launch::CONV && lp.steps[2].sel == Launch::SEL_BFIRST && !lp.steps[2].bgroup.ctr)) return;
    unsigned* const q = reinterpret_cast<unsigned*>(base + wp->ctrl_off) + 16;
    lp.steps[0].prep.q128 = q; lp.steps[1].stem.q128 = q; lp.steps[2].bgroup.ctr = q;
  }

  // Split-K launches of a few blocks (batch 1-4: the 7 x 7 and 14 x 14 maps -- 8 or 16 blocks that each stream 150-300 KB of weights) split K over
  // BLOCKS as well (round 6, conv_mfma_sk.hip KSP): ks_parts blocks per output tile, partial tiles through the scratch area, the block that draws the
  // tile's last ticket finishes.  The ticket words sit behind the group flags and are cleared with them by the step's first kernel.
  void split_k_over_blocks_pass() {
    if (!(opts.sk_kb && wp->ks_ctr_bytes && !lp.steps.empty() && lp.steps[0].kind == Launch::PREP)) return;
    size_t ctr_used = 0;
    for (size_t i = 1; i < lp.steps.size(); i++) {
      Launch& st = lp.steps[i];
      if (st.kind != Launch::CONV || st.sel != Launch::SEL_SK || st.avg_fused || (int)i == lp.logits_direct) continue;
      ConvArgs& c = st.conv;
      if (!conv_mfma_sk_ksplit_eligible(c)) continue;
      const long blocks = (long)((c.g.n_pix + 63) / 64) * c.n_mtiles;
      if (blocks > opts.sk_kb_blocks) continue;
      const int n_virt = c.nslab * (c.dual ? 2 : 1);
      int kb = 1;
      while (kb * 2 <= opts.sk_kb_max && n_virt / (kb * 2) >= 8 && c.nslab / (kb * 2) >= 1) kb *= 2;
      if (kb < 2 || kb < opts.sk_kb_min || (size_t)blocks * kb * 16384 > wp->ks_part_bytes || (ctr_used + blocks) * 4 > wp->ks_ctr_bytes) continue;
      c.ks_parts = kb;
      c.ks_part = reinterpret_cast<int32_t*>(base + wp->ks_part_off);
      c.ks_ctr = reinterpret_cast<unsigned*>(base + wp->ks_ctr_off) + ctr_used;
      ctr_used += (size_t)blocks;
    }
    if (ctr_used) claim_step_counter();
  }

};

}  // namespace

const LaunchPlan* Net::launch_plan(int batch, const WorkPlan* wp, void* ws, bool concurrent, bool allow_groups) {
  if (concurrent) allow_groups = false;
  for (const LaunchPlan& lp : launch_plans)
    if (lp.batch == batch && lp.wp == wp && lp.ws == ws && lp.packed_dev == packed_dev && lp.concurrent == (concurrent ? 1 : 0) &&
        lp.groups == (allow_groups ? 1 : 0)) return &lp;
  if (launch_plans.size() >= 64)                       // evict the oldest plan nobody is walking
    for (auto it = launch_plans.begin(); it != launch_plans.end(); ++it)
      if (it->walkers == 0) { launch_plans.erase(it); break; }
  LaunchPlan lp;
  lp.batch = batch; lp.wp = wp; lp.ws = ws; lp.packed_dev = packed_dev; lp.concurrent = concurrent ? 1 : 0; lp.groups = allow_groups ? 1 : 0;
  Planner p(*this, lp, wp, ws, batch, concurrent, allow_groups);
  if (!p.input_step() || !p.rows()) return nullptr;
  p.q128_flags_pass();
  p.split_k_over_blocks_pass();
  launch_plans.push_back(std::move(lp));
  return &launch_plans.back();
}

}  // namespace tf2
