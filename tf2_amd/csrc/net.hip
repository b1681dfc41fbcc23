// net.hip -- network handle, workspace planning and the layer executor (host code,
// compiled with hipcc for the HIP runtime API).
//
// Replaces NetWork::Init/InitBuffer (host/src/network.cpp:22-150) and Runner::Run
// (host/src/runner.cpp:54-198): instead of one OpenCL queue per FPGA kernel and a
// cycle-scheduled pipeline, every layer is 1-3 kernel launches on the caller's HIP
// stream over NHWC int8 activation tensors that live in a caller-owned workspace.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include "tf2_net.h"
#include "tf2_device.h"
#include "opts.h"

namespace tf2 {

static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
const std::string& last_error() { return g_err; }
tf2_status arg_refusal(const char* fn, const std::string& what) { set_error(std::string(fn) + ": " + what); return TF2_ERR_ARG; }
tf2_status launch_result(const char* fn, const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return TF2_OK;
  set_error(std::string(fn) + ": " + what + ": " + hipGetErrorString(e));
  return TF2_ERR_HIP;
}

#define HIP_OK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                    \
      return TF2_ERR_HIP;                                                              \
    }                                                                                  \
  } while (0)

tf2_status Net::init(const tf2_net_desc* d, const tf2_layer_desc* ls) {
  nd = *d;
  if (nd.n_layers <= 0 || nd.n_q_rows < nd.n_layers + 1 || nd.max_out_channel <= 0) {
    set_error("tf2_net_create: bad net desc"); return TF2_ERR_ARG;
  }
  layers.assign(ls, ls + nd.n_layers);
  const int nl = nd.n_layers;
  // A 3x3 first layer on a 3-channel image (VGG16, SSD300, SqueezeNet 1.1) is executed as a POINTWISE layer over the im2col image:
  // the input kernel writes, per OUTPUT pixel, the 27 values x[c][oh * stride - pad + fh][ow * stride - pad + fw] in the order
  // c * 9 + fh * 3 + fw (zero outside the image: sequencer.cl:287) as [x | xneg], 64 bytes -- exactly the bytes the plain form writes
  // per INPUT pixel for 3 channels padded to 16 -- and the layer becomes C = 27, k = 1, stride 1 on an OH x OW map: one 64-byte K slab
  // per output instead of five (nine taps of 32 bytes, 6 of them real).  Same sums term for term; the filter codes [N][3][3][3] of
  // LoadModel ARE [N][27][1][1] in that channel order, so nothing else changes (the reference does the same kind of thing for its
  // 7x7 first layers: model_loader.cpp:244-257, input_loader.cpp:98-116).  im2col0=0 keeps the plain form.
  im2col0 = false;
  {
    const bool off = opt(OPT_im2col0) == 0;
    // (another row that reads the IMAGE would find the im2col bytes in the input tensor: such programs keep the plain form)
    bool only_consumer = true;
    for (int l = 1; l < nl; l++) if (layers[l].src == -1) only_consumer = false;
    tf2_layer_desc& L0 = layers[0];
    if (!off && only_consumer && !nd.conv1_rewrite && L0.src == -1 && !L0.ipool && L0.k == 3 && L0.model_k == 3 && L0.C == 3 && L0.model_C == 3 &&
        L0.dil <= 1 && nd.image_c == 3 && L0.H == nd.image_h && L0.W == nd.image_w && L0.stride >= 1 &&
        L0.OH == (L0.H + 2 * L0.pad_h - 3) / L0.stride + 1 && L0.OW == (L0.W + 2 * L0.pad_w - 3) / L0.stride + 1) {
      im2col0 = true; im_stride = L0.stride; im_pad_h = L0.pad_h; im_pad_w = L0.pad_w;
      L0.C = 27; L0.k = 1; L0.stride = 1; L0.pad_h = L0.pad_w = 0; L0.H = L0.OH; L0.W = L0.OW;
    }
  }
  // concat tensor widths
  concat_C.assign(std::max(0, nd.n_concat), 0);
  for (int l = 0; l < nl; l++) {
    const tf2_layer_desc& L = layers[l];
    if (L.concat >= 0) {
      if (L.concat >= nd.n_concat) { set_error("layer " + std::to_string(l) + ": concat id out of range"); return TF2_ERR_ARG; }
      if (L.n_start % 16) { set_error("layer " + std::to_string(l) + ": concat slice must start at a multiple of 16 channels"); return TF2_ERR_UNSUPPORTED; }
      concat_C[L.concat] = std::max(concat_C[L.concat], L.n_start + L.N);
    }
  }
  out_Cp.assign(nl, 0);
  in_layout.assign(nl, InLayout());
  for (int l = 0; l < nl; l++) {
    const tf2_layer_desc& L = layers[l];
    if (L.src >= l || L.add_src >= l) { set_error("layer " + std::to_string(l) + ": forward reference"); return TF2_ERR_ARG; }
    if (L.N <= 0 || L.N > nd.max_out_channel) { set_error("layer " + std::to_string(l) + ": bad N"); return TF2_ERR_ARG; }
    // the q table rows Quantization / LoadModel index with this row (quantization.cpp:42-49, model_loader.cpp:159-162)
    if (L.q_in_row < 0 || L.q_in_row >= nd.n_q_rows) { set_error("layer " + std::to_string(l) + ": q_in_row outside the q table"); return TF2_ERR_ARG; }
    if (L.C <= 0 || (!L.ipool && (l == 0 && im2col0 ? 3 : L.C) > nd.max_out_channel)) { set_error("layer " + std::to_string(l) + ": input channels exceed MAX_OUT_CHANNEL"); return TF2_ERR_ARG; }
    if (L.n_start < 0 || L.n_start + L.N > nd.max_out_channel) { set_error("layer " + std::to_string(l) + ": n_start + N exceeds MAX_OUT_CHANNEL"); return TF2_ERR_ARG; }
    if (L.concat >= 0 && nd.n_conv + 1 + L.concat >= nd.n_q_rows) { set_error("layer " + std::to_string(l) + ": concat Q row outside the q table"); return TF2_ERR_ARG; }
    if (L.pool_en && L.add_src >= 0) { set_error("layer " + std::to_string(l) + ": pool + residual in one layer is not supported"); return TF2_ERR_UNSUPPORTED; }
    // (a pooling row's global average: the oracle and netref define none -- tf2o_layer averages a CONV row's pooled map only)
    if (L.ipool == 1 && L.endpool) { set_error("layer " + std::to_string(l) + ": a pool-only row with a global average is not supported"); return TF2_ERR_UNSUPPORTED; }
    out_Cp[l] = round_up(L.N, 16);
    InLayout il;
    int srcC, srcH, srcW;
    if (L.src == -1) {
      il.half = round_up(L.C, 16);
      il.Cp_in = 2 * il.half;
      il.signed_in = 1;
      srcC = L.C; srcH = L.H; srcW = L.W;
    } else if (L.src >= 0) {
      const tf2_layer_desc& S = layers[L.src];
      il.Cp_in = S.concat >= 0 ? round_up(concat_C[S.concat], 16) : out_Cp[L.src];
      srcC = S.concat >= 0 ? concat_C[S.concat] : S.N;
      srcH = S.endpool ? 1 : S.PH; srcW = S.endpool ? 1 : S.PW;
    } else {
      const int cid = -(L.src + 2);
      if (cid >= nd.n_concat) { set_error("layer " + std::to_string(l) + ": concat source out of range"); return TF2_ERR_ARG; }
      il.Cp_in = round_up(concat_C[cid], 16);
      srcC = concat_C[cid];
      srcH = L.H; srcW = L.W;
      for (int j = 0; j < l; j++)
        if (layers[j].concat == cid) { srcH = layers[j].endpool ? 1 : layers[j].PH; srcW = layers[j].endpool ? 1 : layers[j].PW; }
    }
    if (L.ipool == 2 && (srcC != L.C || L.N != L.C || L.pool_en || L.endpool || L.add_src >= 0 || L.concat >= 0 || L.src < 0)) {
      set_error("layer " + std::to_string(l) + ": an L2Norm row maps C channels of a layer output onto C channels, nothing else"); return TF2_ERR_ARG;
    }
    if (!L.ipool && (srcC != L.C || srcH != L.H || srcW != L.W)) {
      set_error("layer " + std::to_string(l) + ": input " + std::to_string(L.C) + "x" + std::to_string(L.H) + "x" + std::to_string(L.W) +
                " does not match its producer's " + std::to_string(srcC) + "x" + std::to_string(srcH) + "x" + std::to_string(srcW));
      return TF2_ERR_ARG;
    }
    in_layout[l] = il;
    if (L.add_src >= 0) {
      const tf2_layer_desc& R = layers[L.add_src];
      if (R.N != L.N || R.PH != L.PH || R.PW != L.PW || R.endpool) { set_error("layer " + std::to_string(l) + ": residual shape mismatch"); return TF2_ERR_ARG; }
    }
  }
  prof_ms.assign(nl, 0.f); prof_launches.assign(nl, 0);
  return TF2_OK;
}

// ---- workspace planning: first-fit offsets with liveness-based reuse ---------------
// Row l is a sink: no row reads it as src, add_src or through a concat (a network output: SSD's multibox heads, the logits row).
bool Net::is_sink(int l) const {
  for (int j = 0; j < nd.n_layers; j++) {
    const tf2_layer_desc& J = layers[j];
    if (J.src == l || J.add_src == l) return false;
    if (J.src <= -2 && layers[l].concat == -(J.src + 2)) return false;
  }
  return true;
}

// mode: PLAN_ORDINARY (liveness reuse), PLAN_KEEP_ALL (every tensor its own memory, fused kernels store their intermediates),
// PLAN_OUTPUTS (the ordinary plan, but every sink row's output lives to the end of the step and the last row stays in the workspace:
// tf2_ssd_run reads the heads from it; never chosen by tf2_net_run*)
const WorkPlan* Net::plan(int batch, int mode) {
  const bool keep_all = mode == PLAN_KEEP_ALL;
  auto key = std::make_pair(batch, mode);
  auto it = plans.find(key);
  if (it != plans.end()) return &it->second;
  WorkPlan wp;
  wp.batch = batch; wp.keep_all = keep_all; wp.outputs_kept = mode == PLAN_OUTPUTS;
  const int nl = nd.n_layers;
  auto add_tensor = [&](int H, int W, int C, int Cp) {
    TensorPlan t; t.H = H; t.W = W; t.C = C; t.Cp = Cp;
    t.bytes = ((size_t)batch * H * W * Cp + 255) / 256 * 256;
    wp.tensors.push_back(t);
    return (int)wp.tensors.size() - 1;
  };
  const tf2_layer_desc& L0 = layers[0];
  wp.input_tensor = add_tensor(L0.H, L0.W, L0.C, in_layout[0].Cp_in);
  std::vector<int> concat_tensor(std::max(0, nd.n_concat), -1);
  std::vector<int> layer_out(nl, -1);
  wp.exec.assign(nl, LayerExec());
  // creation index of every tensor (the layer that first writes it); temps die in-layer
  std::vector<int> born;
  born.push_back(-1);
  for (int l = 0; l < nl; l++) {
    const tf2_layer_desc& L = layers[l];
    LayerExec& E = wp.exec[l];
    E.in_tensor = L.src == -1 ? wp.input_tensor : (L.src >= 0 ? layer_out[L.src] : concat_tensor[-(L.src + 2)]);
    const int oh = L.endpool ? 1 : L.PH, ow = L.endpool ? 1 : L.PW;
    if (L.concat >= 0) {
      if (concat_tensor[L.concat] < 0) {
        concat_tensor[L.concat] = add_tensor(oh, ow, concat_C[L.concat], round_up(concat_C[L.concat], 16));
        born.push_back(l);
      }
      E.out_tensor = concat_tensor[L.concat];
      E.out_off = L.n_start;
    } else {
      E.out_tensor = add_tensor(oh, ow, L.N, out_Cp[l]);
      born.push_back(l);
    }
    layer_out[l] = E.out_tensor;
    E.conv_tensor = E.out_tensor;
    const PackLayer* plm = packed_valid ? pack_layer(l) : nullptr;
    if (plm && plm->merged_into >= 0) {
      // computed by the merged launch of the row in front of it: its conv-stage tensor is that row's (channels behind that row's)
      E.conv_tensor = wp.exec[plm->merged_into].conv_tensor;
      wp.tensors[E.conv_tensor].last_use = std::max(wp.tensors[E.conv_tensor].last_use, l);
    } else if (!L.ipool && (L.pool_en || L.endpool)) {
      // conv (+residual) result before pooling / global average (merged rows: both rows' channels)
      const int th = L.pool_en ? L.OH : L.PH, tw = L.pool_en ? L.OW : L.PW;
      const int Nx = (plm && plm->merge_next > 0) ? L.N + layers[plm->merge_next].N : L.N;
      E.conv_tensor = add_tensor(th, tw, Nx, round_up(Nx, 16));
      born.push_back(l);
      wp.tensors[E.conv_tensor].last_use = l;
      // pool + global average: conv map -> pooled map (this tensor) -> 1 x 1 output (maxpool_kernel, then global_avg_kernel)
      if (L.pool_en && L.endpool) {
        E.pool_tensor = add_tensor(L.PH, L.PW, L.N, out_Cp[l]);
        born.push_back(l);
        wp.tensors[E.pool_tensor].last_use = l;
      }
    }
    if (L.add_src >= 0) {
      E.res_tensor = layer_out[L.add_src];
      E.res_off = layers[L.add_src].concat >= 0 ? layers[L.add_src].n_start : 0;
    }
    // liveness
    wp.tensors[E.in_tensor].last_use = std::max(wp.tensors[E.in_tensor].last_use, l);
    if (E.res_tensor >= 0) wp.tensors[E.res_tensor].last_use = std::max(wp.tensors[E.res_tensor].last_use, l);
    wp.tensors[E.out_tensor].last_use = std::max(wp.tensors[E.out_tensor].last_use, l);
  }
  wp.final_tensor = layer_out[nl - 1];
  wp.tensors[wp.final_tensor].last_use = nl;
  if (wp.outputs_kept)
    for (int l = 0; l < nl; l++)
      if (is_sink(l)) wp.tensors[wp.exec[l].out_tensor].last_use = nl;
  // Fused pairs (conv_bneck.hip: layer l computes layer fuse_next as well, block by block): everything the launch reads
  // stays live until the LATER layer's index, and everything it writes exists from the EARLIER one -- otherwise the
  // first-fit planner hands the expand's output the memory of the 3x3's input, which other blocks are still reading.
  if (packed_valid)
    for (int l = 0; l < nl; l++) {
      const PackLayer* pl = pack_layer(l);
      int b = pl ? pl->fuse_next : 0;
      if (b <= 0 && opts.pair_mode && pair_candidate(l) && !(l >= 2 && pair_candidate(l - 1))) b = l + 1;   // (pairs do not chain)
      if (b <= 0) continue;
      TensorPlan& tin = wp.tensors[wp.exec[l].in_tensor];
      tin.last_use = std::max(tin.last_use, b);
      if (wp.exec[l].res_tensor >= 0) wp.tensors[wp.exec[l].res_tensor].last_use = std::max(wp.tensors[wp.exec[l].res_tensor].last_use, b);
      for (size_t t = 0; t < wp.tensors.size(); t++)
        if (born[t] == b) born[t] = l;
    }
  // Group launches (conv_bgroup.hip: rows l .. l + 2 in one launch, images at different layers at the same time): what the launch
  // reads stays live to its last row, what it writes exists from its first
  if (packed_valid && (opts.bgroup_mode || opts.bband_mode || opts.bfirst_mode))
    for (int l = 0; l + 2 < nl; l++) {
      if ((opts.bgroup_mode || opts.bfirst_mode) && bgroup_first_at(l)) {          // (conv_bgroup56f_kernel or conv_bfirst_kernel: rows l .. l + 3)
        TensorPlan& tin = wp.tensors[wp.exec[l].in_tensor];
        tin.last_use = std::max(tin.last_use, l + 3);
        TensorPlan& tm1 = wp.tensors[wp.exec[l + 1].out_tensor];
        tm1.last_use = std::max(tm1.last_use, l + 3);
        for (size_t t = 0; t < wp.tensors.size(); t++)
          if (born[t] > l && born[t] <= l + 3) born[t] = l;
        if (opts.bgroup_mode) {
          if (!wp.ctrl_bytes) wp.ctrl_bytes = 256;
          wp.ctrl_bytes += (size_t)((batch + 7) / 8 * 8) * 128;
        }
        if (opts.bfirst_mode && opts.q128_flags && !wp.ctrl_bytes) wp.ctrl_bytes = 256;      // (the control header: the -128 flags of launch_plan)
        l += 3;
        continue;
      }
      const bool grp = opts.bgroup_mode && bgroup_at(l);
      // (band launches: the batch gate of launch_plan applies here too; whether batches are in flight is not known to the workspace
      //  plan -- one workspace serves both launch plans -- so a batch that COULD take band launches pays their longer lifetimes in
      //  both: INTEGRATION.md "Workspace")
      if (!grp && !(opts.bband_mode && batch >= opts.bband_min && (bband_at(l, opts.bband_rows) || bband_at(l, opts.bband_rows_alone)))) continue;
      TensorPlan& tin = wp.tensors[wp.exec[l].in_tensor];
      tin.last_use = std::max(tin.last_use, l + 2);
      TensorPlan& tm1 = wp.tensors[wp.exec[l].out_tensor];
      tm1.last_use = std::max(tm1.last_use, l + 2);
      for (size_t t = 0; t < wp.tensors.size(); t++)
        if (born[t] == l + 1 || born[t] == l + 2) born[t] = l;
      if (grp) {
        if (!wp.ctrl_bytes) wp.ctrl_bytes = 256;                       // the step counter
        wp.ctrl_bytes += (size_t)((batch + 7) / 8 * 8) * 128;          // three rows of eight flag words per image (roll call, two meetings)
      }
      l += 2;
    }
  // Fire launches (conv_fire.hip: rows l .. l + 2 in one launch): what the launch reads stays live to its last row, what it writes exists from
  // its first
  if (packed_valid && opts.fire_mode)
    for (int l = 0; l + 2 < nl; l++) {
      if (!fire_at(l)) continue;
      TensorPlan& tin = wp.tensors[wp.exec[l].in_tensor];
      tin.last_use = std::max(tin.last_use, l + 2);
      for (size_t t = 0; t < wp.tensors.size(); t++)
        if (born[t] == l + 1 || born[t] == l + 2) born[t] = l;
      l += 2;
    }
  // ... and consecutive identity bottlenecks of the 14 x 14 maps may share a launch (bgroup_chain): nothing such a run touches
  // shares memory (the exchange inside a launch is ordered by flags and cache scopes, not by kernel boundaries)
  if (packed_valid && opts.bgroup_mode && opts.bgroup_chain > 1)
    for (int l = 0; l + 2 < nl;) {
      if (!bgroup_at(l)) { l++; continue; }
      int e = l + 2;
      while (e + 3 < nl && bgroup_at(e + 1) && layers[e + 1].H == layers[l].H) e += 3;
      if (e > l + 2)
        for (size_t t = 0; t < wp.tensors.size(); t++) {
          if (born[t] > l && born[t] <= e) born[t] = l;
          if (wp.tensors[t].last_use >= l && wp.tensors[t].last_use < e && born[t] <= e) wp.tensors[t].last_use = e;
        }
      l = e + 1;
    }
  // ---- offsets ----
  struct Seg { size_t off, len; };
  std::vector<Seg> free_list;           // sorted by offset
  size_t top = 0;
  auto alloc = [&](size_t len) -> size_t {
    for (size_t i = 0; i < free_list.size(); i++)
      if (free_list[i].len >= len) {
        size_t off = free_list[i].off;
        free_list[i].off += len; free_list[i].len -= len;
        if (free_list[i].len == 0) free_list.erase(free_list.begin() + i);
        return off;
      }
    // extend a free segment that touches the top
    if (!free_list.empty() && free_list.back().off + free_list.back().len == top) {
      size_t off = free_list.back().off;
      top = off + len;
      free_list.pop_back();
      return off;
    }
    size_t off = top; top += len; return off;
  };
  auto release = [&](size_t off, size_t len) {
    Seg s{off, len};
    auto pos = std::lower_bound(free_list.begin(), free_list.end(), s, [](const Seg& a, const Seg& b) { return a.off < b.off; });
    pos = free_list.insert(pos, s);
    size_t i = pos - free_list.begin();
    if (i + 1 < free_list.size() && free_list[i].off + free_list[i].len == free_list[i + 1].off) {
      free_list[i].len += free_list[i + 1].len; free_list.erase(free_list.begin() + i + 1);
    }
    if (i > 0 && free_list[i - 1].off + free_list[i - 1].len == free_list[i].off) {
      free_list[i - 1].len += free_list[i].len; free_list.erase(free_list.begin() + i);
    }
  };
  for (size_t t = 0; t < wp.tensors.size(); t++) wp.tensors[t].first_use = born[t];
  std::vector<char> placed(wp.tensors.size(), 0), freed(wp.tensors.size(), 0);
  wp.tensors[wp.input_tensor].offset = alloc(wp.tensors[wp.input_tensor].bytes);
  placed[wp.input_tensor] = 1;
  for (int l = 0; l < nl; l++) {
    for (size_t t = 0; t < wp.tensors.size(); t++)
      if (!placed[t] && born[t] == l) { wp.tensors[t].offset = alloc(wp.tensors[t].bytes); placed[t] = 1; }
    if (!keep_all)
      for (size_t t = 0; t < wp.tensors.size(); t++)
        if (placed[t] && !freed[t] && wp.tensors[t].last_use <= l && (int)t != wp.final_tensor) {
          release(wp.tensors[t].offset, wp.tensors[t].bytes); freed[t] = 1;
        }
  }
  wp.ctrl_off = (top + 255) / 256 * 256 + 256;
  wp.ctrl_bytes = (wp.ctrl_bytes + 255) / 256 * 256;
  // split-K over blocks (launch_plan: grids of at most sk_kb_blocks blocks): 1024 ticket words behind the group flags, cleared with them
  if (packed_valid && opts.sk_kb && batch <= 8) {
    if (!wp.ctrl_bytes) wp.ctrl_bytes = 256;
    wp.ks_ctr_off = wp.ctrl_off + wp.ctrl_bytes; wp.ks_ctr_bytes = 4096; wp.ctrl_bytes += wp.ks_ctr_bytes;
  }
  // partial sums of the conv_fc launches (one at a time: the largest)
  wp.scratch_off = wp.ctrl_off + wp.ctrl_bytes;
  wp.scratch_bytes = 0;
  if (packed_valid)
    for (int l = 0; l < nl; l++) {
      const PackLayer* pl = pack_layer(l);
      if (pl && (opts.fc_mode || pl->fc4) && fc_at(l, batch)) wp.scratch_bytes = std::max(wp.scratch_bytes, conv_fc_scratch_bytes(pl->Np, pl->nslab, pl->dual, batch));
    }
  wp.scratch_bytes = (wp.scratch_bytes + 255) / 256 * 256;
  if (wp.ks_ctr_bytes) {                                   // partial tiles: sk_kb_blocks x sk_kb_max x 16 KB behind the conv_fc partial sums
    wp.ks_part_off = wp.scratch_off + wp.scratch_bytes;
    wp.ks_part_bytes = (size_t)std::max(1, opts.sk_kb_blocks) * std::max(1, opts.sk_kb_max) * 16384;
    wp.scratch_bytes += wp.ks_part_bytes;
  }
  wp.total_bytes = wp.scratch_off + wp.scratch_bytes;
  auto res = plans.emplace(key, std::move(wp));
  return &res.first->second;
}

// ---- run-time switches (A/B experiments and forced kernels for the tests), read when a launch plan is built ----
void Net::load_options() {
  RunOpts o;
  // (the snapshot of TF2_AMD_OPTS was taken by the caller: tf2_net_create / tf2_net_reload_options, opts.h)
#define TF2_OPT(name, scope, test_only, type, member, dflt) o.member = (type)opt(OPT_##name);
#define TF2_OPT_RAW(name, scope, test_only, dflt)
#include "opt_table.h"
  // ... and the options that are more than a value copied into its member:
  o.flags = (int)opt(OPT_exp) & 0x7ff8;          // the timing-probe bits only
  o.dbg = (long long*)(uintptr_t)(unsigned long long)opt(OPT_dbgptr);
  o.dbg2 = (long long*)(uintptr_t)(unsigned long long)opt(OPT_dbgptr2);
  // alt_min moves both thresholds (a negative value counts as not given); alt_min_conc, where given, has the last word
  if (o.alt_min_blocks < 0) o.alt_min_blocks = RunOpts().alt_min_blocks;
  else if (opt_given(OPT_alt_min) && !opt_given(OPT_alt_min_conc)) o.alt_min_blocks_conc = o.alt_min_blocks;
  if (o.bband_mode == 2) o.bband_alone_maps = 6;
  if (o.pwk_slots <= 0) o.pwk_slots = 256;
  opts = o;
  launch_plans.clear();
  // tensor lifetimes depend on which rows may share a launch (pair): re-plan what was planned (a caller's keep_all
  // workspace keeps being recognised by run / read_layer)
  std::vector<std::pair<int, int>> keys;
  for (const auto& kv : plans) keys.push_back(kv.first);
  plans.clear();
  for (const auto& k : keys) (void)plan(k.first, k.second);
}

// CUs the stream's launches may use (hipExtStreamCreateWithCUMask: tf2_amd/streams.py); an unmasked stream reports the device's.
static int stream_cu_count(hipStream_t s) {
  uint32_t mask[16] = {0};
  if (hipExtStreamGetCUMask(s, 16, mask) != hipSuccess) { (void)hipGetLastError(); return 1 << 20; }
  int n = 0;
  for (uint32_t w : mask) n += __builtin_popcount(w);
  return n > 0 ? n : 1 << 20;
}

// (launch planning -- Net::launch_plan, the planner and the selection predicates Net::*_at -- is net_plan.hip)

static thread_local LaunchRecorder* g_recorder = nullptr;
LaunchRecorder*& launch_recorder() { return g_recorder; }

// one prepared launch of a step -> its kernel (or, with a recorder installed, its description)
int Net::issue(const Launch& st, const LaunchPlan* lp, const void* images, bool images_are_q, int8_t* logits, void* stream) {
  switch (st.kind) {
    case Launch::PREP: {
      PrepArgs pa = st.prep; pa.img = images; pa.src_is_q = images_are_q ? 1 : 0;
      if (st.sel == Launch::SEL_FIRST) { FirstArgs f = st.first; f.p = pa; return f.pool ? launch_conv_first_pool(f, stream) : launch_conv_first(f, stream); }
      return launch_prep_input(pa, stream);
    }
    case Launch::POOL: return launch_maxpool(st.pool, stream);
    case Launch::AVG: return launch_global_avg(st.avg, stream);
    case Launch::L2N: return launch_l2norm(st.l2n, stream);
    case Launch::CONV:
      switch (st.sel) {
        case Launch::SEL_PW: return launch_conv_pw(st.conv, st.TM, stream);
        case Launch::SEL_PWK: return launch_conv_pwk(st.conv, st.TM, st.pwk_slots, st.pwk_pipe, stream);
        case Launch::SEL_PWKPAIR: return launch_conv_pwk_pair(st.conv, st.TM, st.conv2, st.TM2, st.pwk_slots, st.pwk_pipe, stream);
        case Launch::SEL_SK:
          if (logits && lp->logits_direct >= 0 && &st == &lp->steps[lp->logits_direct]) {
            ConvArgs cd = st.conv_direct; cd.y = logits;
            return launch_conv_mfma_sk(cd, opts.sk8_blocks, st.shape, stream);
          }
          return launch_conv_mfma_sk(st.conv, opts.sk8_blocks, st.shape, stream);
        case Launch::SEL_MFMA2: return launch_conv_mfma2(st.conv, st.TM, stream);
        case Launch::SEL_BNECK: return launch_conv_bneck(st.bneck, st.TM, st.shape, stream);
        case Launch::SEL_PAIR: return launch_conv_mfma2_pair(st.conv, st.conv2, st.TM, stream);
        case Launch::SEL_SKPAIR: return launch_conv_mfma_sk_pair(st.conv, st.conv2, opts.sk8_blocks, st.shape, stream);
        case Launch::SEL_BBAND: return launch_conv_bband(st.bband, st.bg_c, st.bg_m, stream);
        case Launch::SEL_C3: return launch_conv_c3(st.c3, stream);
        case Launch::SEL_IMG: return launch_conv_img(st.img, stream);
        case Launch::SEL_FIRE: return launch_conv_fire(st.fire, stream);
        case Launch::SEL_FC: return launch_conv_fc(st.fc, stream);
        case Launch::SEL_BGROUPF: return launch_conv_bgroup_first(st.bgroup, stream);
        case Launch::SEL_BFIRST: return launch_conv_bfirst(st.bgroup, stream);
        case Launch::SEL_BGROUP:
          if (!st.bg_chain.empty()) return launch_conv_bgroup(st.bg_chain.data(), (int)st.bg_chain.size(), st.bg_hw, st.bg_c, st.bg_m, stream);
          return launch_conv_bgroup(&st.bgroup, 1, st.bg_hw, st.bg_c, st.bg_m, stream);
        case Launch::SEL_STEM: return launch_conv_stem(st.stem, st.shape, stream);
        default: return launch_conv_shift(st.conv, st.signed_in, st.mul24, st.shape, stream);
      }
  }
  return -1;
}

// The launches one step of `batch` images consists of, as the library itself would issue them (kernel, grid, LDS, registers):
// tile shapes, fused pairs and split-K variants are decided in launch_plan / the launchers, nowhere else.  No device needed.
tf2_status Net::describe_launches(int batch, bool concurrent, std::vector<std::pair<int, LaunchRecord>>* out) {
  std::lock_guard<std::mutex> lock(run_mutex);
  if (!packed_valid) { set_error("tf2_net_describe_launches: no packed image"); return TF2_ERR_STATE; }
  if (batch <= 0) return arg_refusal("tf2_net_describe_launches", "batch must be positive");
  const WorkPlan* wp = plan(batch, false);
  // the description's plan is built beside the cache (never evicts or replaces a run plan) and dropped again
  const uint8_t* saved = packed_dev;
  if (!packed_dev) packed_dev = packed.data();               // addresses are only formatted into argument blocks nobody launches
  static char fake_ws[16];
  std::list<LaunchPlan> keep;
  keep.swap(launch_plans);
  const LaunchPlan* lp = launch_plan(batch, wp, fake_ws, concurrent, true);
  std::list<LaunchPlan> mine;
  mine.swap(launch_plans);
  launch_plans.swap(keep);
  packed_dev = saved;
  if (!lp) return TF2_ERR_ARG;
  LaunchRecorder rec; rec.name[0] = 0;
  g_recorder = &rec;
  int rc = 0;
  for (const Launch& st : lp->steps) {
    const size_t before = rec.rows.size();
    rc = issue(st, lp, fake_ws, false, nullptr, nullptr);
    if (rc) break;
    for (size_t i = before; i < rec.rows.size(); i++) out->emplace_back(st.layer, rec.rows[i]);
  }
  g_recorder = nullptr;
  if (rc) { set_error("tf2_net_describe_launches: " + std::string(device_last_error())); return TF2_ERR_HIP; }
  return TF2_OK;
}

// The liveness-planned workspace of `batch` images as the library lays it out: every tensor's byte range and the rows between which
// it holds memory, and per row the tensors it reads / writes.  No device needed (tests/test_host_abi.py checks with it that rows
// sharing a launch never share memory).
tf2_status Net::describe_workspace(int batch, bool keep_all, std::vector<TensorPlan>* tensors, std::vector<LayerExec>* rows) {
  std::lock_guard<std::mutex> lock(run_mutex);
  if (!packed_valid) { set_error("tf2_net_describe_workspace: no packed image"); return TF2_ERR_STATE; }
  if (batch <= 0) return arg_refusal("tf2_net_describe_workspace", "batch must be positive");
  const WorkPlan* wp = plan(batch, keep_all);
  *tensors = wp->tensors;
  *rows = wp->exec;
  return TF2_OK;
}

size_t Net::workspace_size(int batch, bool keep_all) {
  std::lock_guard<std::mutex> lock(run_mutex);
  const WorkPlan* wp = plan(batch, keep_all);
  return wp ? wp->total_bytes : 0;
}

size_t Net::logits_bytes(int batch) const {
  const tf2_layer_desc& LL = layers[nd.n_layers - 1];
  const size_t hw = LL.endpool ? 1 : (size_t)LL.PH * LL.PW;
  return (size_t)batch * hw * LL.N;
}

tf2_status Net::run(const void* images, bool images_are_q, int batch, void* ws, size_t ws_bytes,
                    int8_t* logits, void* stream, int concurrency, void* mark_event, int mark_after_layer, bool outputs_kept) {
  std::unique_lock<std::mutex> lock(run_mutex);
  if (!packed_valid) { set_error("tf2_net_run: no packed image (tf2_net_pack / tf2_net_packed_adopt)"); return TF2_ERR_STATE; }
  if (!packed_dev) { set_error("tf2_net_run: packed image not bound to the device (tf2_net_bind_device)"); return TF2_ERR_STATE; }
  if (q.empty()) { set_error("tf2_net_run: q table not set"); return TF2_ERR_STATE; }
  if (batch <= 0) return arg_refusal("tf2_net_run", "batch must be positive");
  // keep_all plans are a superset in size; pick whichever plan fits the caller's buffer
  const WorkPlan* wp = nullptr;
  if (outputs_kept) {
    wp = plan(batch, PLAN_OUTPUTS);                         // (tf2_ssd_run only)
  } else {
    const WorkPlan* a = plan(batch, false);
    auto itk = plans.find(std::make_pair(batch, 1));
    if (itk != plans.end() && ws_bytes >= itk->second.total_bytes) wp = &itk->second;
    else wp = a;
  }
  if (ws_bytes < wp->total_bytes) { set_error("tf2_net_run: workspace too small"); return TF2_ERR_SIZE; }
  // which workspaces last ran the outputs-kept plan (poll_error reads that plan's error word there)
  if (outputs_kept) {
    if (outputs_ws.size() >= 64 && !outputs_ws.count(ws)) outputs_ws.erase(outputs_ws.begin());
    outputs_ws[ws] = batch;
  } else if (!outputs_ws.empty()) {
    outputs_ws.erase(ws);
  }
  // batches in flight?  (calls on at least two different streams among the last eight)
  void* const tag = (void*)((uintptr_t)stream + 1);          // the null stream is a stream too; 0 = empty slot
  recent_streams[recent_pos] = tag; recent_pos = (recent_pos + 1) & 7;
  bool concurrent = opts.alt_conc_mode == 1;
  if (concurrency >= 0 && opts.alt_conc_mode == 2) concurrent = concurrency != 0;        // the caller's own statement (tf2_net_run_ex)
  else if (opts.alt_conc_mode == 2)
    for (int i = 0; i < 8 && !concurrent; i++) concurrent = recent_streams[i] != nullptr && recent_streams[i] != tag;
  hipStream_t s = (hipStream_t)stream;
  // group launches spin until the eight members of an image are resident together, one block per CU: never on a stream whose CU
  // mask leaves fewer than 64 CUs (asked per call: the handle does not know what the caller's next stream looks like)
  // (asked only where group launches could be selected: a runtime call per step under the handle's mutex otherwise;
  //  tf2_net_run_stats' small_mask_steps therefore counts such steps of the one-batch-at-a-time path only)
  const bool wide_stream = (concurrent || !opts.bgroup_mode) ? true : stream_cu_count(s) >= 64;
  const bool allow_groups = !concurrent && opts.bgroup_mode && wide_stream;
  const LaunchPlan* lp = launch_plan(batch, wp, ws, concurrent, allow_groups);
  if (!lp) return TF2_ERR_ARG;
  stat_steps++; stat_group_steps += lp->n_groups ? 1 : 0; stat_inflight_steps += concurrent ? 1 : 0; stat_small_mask_steps += wide_stream ? 0 : 1;
  const int nl = nd.n_layers;
  // The enqueue itself runs outside the handle's mutex, under the plan's own (tf2_amd.h threading note): host threads that
  // feed different streams issue their ~40 launches per step side by side.  (Profiling runs keep the handle's mutex: the
  // event lists are the handle's.)
  struct Walk {
    LaunchPlan* lp; std::unique_lock<std::mutex>& net_lock; std::unique_lock<std::mutex> plan_lock;
    ~Walk() {
      if (plan_lock.owns_lock()) plan_lock.unlock();
      if (!net_lock.owns_lock()) net_lock.lock();
      lp->walkers--;
    }
  } walk{const_cast<LaunchPlan*>(lp), lock, {}};
  walk.lp->walkers++;
  const std::shared_ptr<std::mutex> plan_mutex = lp->enqueue;
  if (!profiling && !profiling_loop) lock.unlock();
  walk.plan_lock = std::unique_lock<std::mutex>(*plan_mutex);

  hipEvent_t loop0 = nullptr, loop1 = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int ev_layer = -2;
  auto close_layer_event = [&]() -> tf2_status {
    if (ev_layer >= 0) {
      HIP_OK(hipEventRecord(ev1, s));
      prof_events.emplace_back((void*)ev0, (void*)ev1);
      prof_event_layer.push_back(ev_layer);
      ev_layer = -2;
    }
    return TF2_OK;
  };
  bool mark_pending = mark_event != nullptr;
#ifdef TF2_PROBES
  // tools/probe_run.py: leave out the launches of a layer range (results are then wrong; only durations are read)
  int skip_lo = 1 << 30, skip_hi = -1 << 30;
  if (const long long sk = opt(OPT_skip_layers); sk >= 0) { skip_lo = (int)(sk >> 32); skip_hi = (int)(unsigned)sk; }
#endif
  for (const Launch& st : lp->steps) {
#ifdef TF2_PROBES
    if (st.layer >= skip_lo && st.layer <= skip_hi) continue;
#endif
    if (mark_pending && st.layer > mark_after_layer) {       // every launch of layers 0..mark_after_layer is enqueued
      HIP_OK(hipEventRecord((hipEvent_t)mark_event, s));
      mark_pending = false;
    }
    if (profiling && st.layer != ev_layer) {            // one event pair per layer (conv + its pool / average)
      if (tf2_status e = close_layer_event()) return e;
      if (st.layer >= 0) {
        HIP_OK(hipEventCreate(&ev0)); HIP_OK(hipEventCreate(&ev1));
        HIP_OK(hipEventRecord(ev0, s));
        ev_layer = st.layer;
      }
    }
    if (profiling_loop && st.layer == 0 && !loop0) {
      HIP_OK(hipEventCreate(&loop0)); HIP_OK(hipEventCreate(&loop1));
      HIP_OK(hipEventRecord(loop0, s));
    }
    const int rc = issue(st, lp, images, images_are_q, logits, stream);
    if (rc) { set_error("kernel launch failed at layer " + std::to_string(st.layer) + ": " + device_last_error()); return TF2_ERR_HIP; }
  }
  if (mark_pending) HIP_OK(hipEventRecord((hipEvent_t)mark_event, s));
  if (profiling) { if (tf2_status e = close_layer_event()) return e; }
  if (profiling_loop && loop0) {
    HIP_OK(hipEventRecord(loop1, s));
    prof_events.emplace_back((void*)loop0, (void*)loop1);
    prof_event_layer.push_back(-1);
  }
  // dense logits [batch][H_last * W_last][N_last]  (H = W = 1 for the classification networks)
  if (logits && lp->logits_direct < 0) {
    const TensorPlan& tf = wp->tensors[wp->final_tensor];
    const tf2_layer_desc& LL = layers[nl - 1];
    const size_t rows = (size_t)batch * tf.H * tf.W;
    HIP_OK(hipMemcpy2DAsync(logits, (size_t)LL.N, (const int8_t*)ws + tf.offset + wp->exec[nl - 1].out_off, (size_t)tf.Cp,
                            (size_t)LL.N, rows, hipMemcpyDeviceToDevice, s));
  }
  return TF2_OK;
}

// Did a group launch of a step on this workspace give up a meeting (conv_bgroup.hip bg_report)?  Reads the workspace's error word
// (synchronises the stream), clears it, TF2_ERR_GROUP with the report decoded if it was set.  The plan's workspace layout is a
// function of the batch alone, so the caller names the batch the workspace was used for.
tf2_status Net::poll_error(int batch, void* ws, size_t ws_bytes, void* stream) {
  if (!packed_valid || !packed_dev) { set_error("tf2_net_poll_error: no packed model bound"); return TF2_ERR_STATE; }
  if (batch <= 0 || !ws) return arg_refusal("tf2_net_poll_error", "bad argument");
  const WorkPlan* wp = nullptr;
  auto ito = outputs_ws.find(ws);
  if (ito != outputs_ws.end() && ito->second == batch) {
    wp = plan(batch, PLAN_OUTPUTS);                         // the workspace's last step was a tf2_ssd_run
  } else {
    const WorkPlan* a = plan(batch, false);
    auto itk = plans.find(std::make_pair(batch, 1));
    if (itk != plans.end() && ws_bytes >= itk->second.total_bytes) wp = &itk->second;
    else wp = a;
  }
  if (ws_bytes < wp->total_bytes) { set_error("tf2_net_poll_error: workspace too small for this batch"); return TF2_ERR_SIZE; }
  if (!wp->ctrl_bytes) { HIP_OK(hipStreamSynchronize((hipStream_t)stream)); return TF2_OK; }      // no group launch can run on it
  unsigned word = 0;
  unsigned* dev = reinterpret_cast<unsigned*>((uint8_t*)ws + wp->ctrl_off) + 1;
  HIP_OK(hipMemcpyAsync(&word, dev, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  if (!bg_err_valid(word)) return TF2_OK;
  HIP_OK(hipMemsetAsync(dev, 0, 4, (hipStream_t)stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  const unsigned code = word & 0xffffu, meet = code & 0xff, kb = code >> 8;
  set_error(std::string("a group launch gave up a meeting of its eight blocks per image (") +
            (meet == 0x01 ? "roll call" : meet == 0x10 ? "input of a chained bottleneck" : meet == 0x20 ? "first meeting" : "second meeting") +
            ", bottleneck " + std::to_string(kb) + " of its launch): the members were not resident together -- the step's logits are not valid; "
            "see the group-launch preconditions in tf2_amd.h (>= 64 CUs on the stream, at most four concurrent callers) or set TF2_AMD_OPTS=bgroup=0");
  return TF2_ERR_GROUP;
}

void Net::drain_profile() {
  for (size_t i = 0; i < prof_events.size(); i++) {
    hipEvent_t e0 = (hipEvent_t)prof_events[i].first, e1 = (hipEvent_t)prof_events[i].second;
    float ms = 0.f;
    if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) {
      if (prof_event_layer[i] < 0) {
        prof_loop_ms += ms; prof_loop_n++;
      } else {
        prof_ms[prof_event_layer[i]] += ms;
        prof_launches[prof_event_layer[i]] += 1;
      }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  }
  prof_events.clear(); prof_event_layer.clear();
}

tf2_status Net::read_layer(int layer, int batch, const void* ws, int8_t* dst, size_t cap, void* stream) {
  // the keep_all plan of this batch (planning is deterministic: rebuilt if tf2_net_reload_options dropped it since the run)
  if (batch <= 0) return arg_refusal("tf2_net_read_layer", "batch must be positive");
  if (layer < -1 || layer >= nd.n_layers) return arg_refusal("tf2_net_read_layer", "bad layer");
  const WorkPlan* wpp;
  { std::lock_guard<std::mutex> lock(run_mutex); wpp = plan(batch, true); }        // (std::map nodes are stable: the plan outlives the lock)
  const WorkPlan& wp = *wpp;
  int tid, off, C;
  if (layer == -1) { tid = wp.input_tensor; off = 0; C = layers[0].C; }
  else { tid = wp.exec[layer].out_tensor; off = wp.exec[layer].out_off; C = layers[layer].N; }
  const TensorPlan& t = wp.tensors[tid];
  const size_t npix = (size_t)batch * t.H * t.W;
  if (layer == -1 && im2col0) {
    // the input tensor holds the im2col image (Net::init): hand back the quantised image [batch][3][H][W] it was gathered from --
    // pixel (r, c) of channel ch is tap (fh, fw) of output pixel (oh, ow) with r + pad_h = oh * stride + fh (a pixel no window covers,
    // possible with stride > 1, is not in the tensor: 0)
    const int IH = nd.image_h, IW = nd.image_w;
    if (cap < (size_t)batch * 3 * IH * IW) { set_error("tf2_net_read_layer: destination too small"); return TF2_ERR_SIZE; }
    std::vector<int8_t> tmp(npix * t.Cp);
    HIP_OK(hipMemcpyAsync(tmp.data(), (const int8_t*)ws + t.offset, tmp.size(), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    for (int b = 0; b < batch; b++)
      for (int ch = 0; ch < 3; ch++)
        for (int r = 0; r < IH; r++)
          for (int c = 0; c < IW; c++) {
            const int oh = std::min((r + im_pad_h) / im_stride, t.H - 1), fh = r + im_pad_h - oh * im_stride;
            const int ow = std::min((c + im_pad_w) / im_stride, t.W - 1), fw = c + im_pad_w - ow * im_stride;
            int8_t v = 0;
            if (fh <= 2 && fw <= 2) v = tmp[(((size_t)b * t.H + oh) * t.W + ow) * t.Cp + ch * 9 + fh * 3 + fw];
            dst[(((size_t)b * 3 + ch) * IH + r) * IW + c] = v;
          }
    return TF2_OK;
  }
  if (cap < npix * C) { set_error("tf2_net_read_layer: destination too small"); return TF2_ERR_SIZE; }
  const size_t Cp = (layer == -1 && packed_valid && stem_selected(batch)) ? 32 : (size_t)t.Cp;     // x-only image tensor (conv_stem.hip)
  std::vector<int8_t> tmp(npix * Cp);
  HIP_OK(hipMemcpyAsync(tmp.data(), (const int8_t*)ws + t.offset, tmp.size(), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  const size_t HW = (size_t)t.H * t.W;
  // doubled channels are stored as 2y - 128 (weight_pack.cpp): hand back y
  const PackLayer* pl = layer >= 0 ? pack_layer(layer) : nullptr;
  const uint8_t* dblf = (pl && pl->off_dbl) ? packed.data() + pl->off_dbl : nullptr;
  for (int b = 0; b < batch; b++)
    for (int c = 0; c < C; c++)
      for (size_t p = 0; p < HW; p++) {
        int8_t v = tmp[((size_t)b * HW + p) * Cp + off + c];
        if (dblf && dblf[c]) v = (int8_t)(((int)v + 128) >> 1);
        dst[((size_t)b * C + c) * HW + p] = v;
      }
  return TF2_OK;
}

}  // namespace tf2

