// capi.cpp -- the extern "C" surface declared in include/tf2_amd.h.
#include <cstring>
#include <new>
#include "tf2_net.h"
#include "tf2_device.h"
#include "opts.h"
#include "ssd_detect.h"
#include "preprocess.h"
#include "classify.h"
#include "ssd_eval.h"
#include "embed_match.h"
#include "embed_roc.h"
#include "roi_crop.h"
#include "roi_warp.h"
#include "ycc_convert.h"
#include "jpeg_idct.h"
#include "jpeg_huff.h"
#include "act_audit.h"
#include "act_fidelity.h"
#include "act_caq.h"
#include "weight_inq.h"
#include "weight_dnscp.h"

using namespace tf2;

struct tf2_net { Net impl; };
struct tf2_ssd { SsdDetector impl; };
struct tf2_cls { Classifier impl; };
struct tf2_det_eval { DetEvaluator impl; };
struct tf2_emb { Matcher impl; };
struct tf2_audit { Auditor impl; };
struct tf2_fid { Comparator impl; };

#define CHECK_NET(n)                                              \
  if (!(n)) { set_error("null tf2_net handle"); return TF2_ERR_ARG; }

// tf2_audit_create / tf2_fid_create: a handle (its impl has create(Net*)) on a net, deleted again where create refuses
template <class H>
static tf2_status create_observer(const char* fn, tf2_net* net, H** out) {
  CHECK_NET(net);
  if (!out) return arg_refusal(fn, "null argument");
  H* h = new (std::nothrow) H();
  if (!h) { set_error("out of memory"); return TF2_ERR_SIZE; }
  const tf2_status st = h->impl.create(&net->impl);
  if (st != TF2_OK) { delete h; return st; }
  *out = h;
  return TF2_OK;
}

extern "C" {

const char* tf2_last_error(void) { return last_error().c_str(); }
int tf2_abi_version(void) { return 1; }
int tf2_has_device_code(void) { return 1; }
// 0: the product; 1: the -DTF2_PROBES timing build (leaves work out: tools/probe_run.py); 2: the -DTF2_CHECK_DMA build (vm_track.h)
int tf2_build_kind(void) {
#if defined(TF2_PROBES)
  return 1;
#elif defined(TF2_CHECK_DMA)
  return 2;
#else
  return 0;
#endif
}
#ifdef TF2_CHECK_DMA
// tools/dma_stress.py only (not part of include/tf2_amd.h): {fragment reads that saw the sentinel of a DMA not landed, reads checked}
int tf2_check_dma_errors(unsigned long long out[2]) {
  unsigned long long a[2] = {0, 0}, b[2] = {0, 0};
  tf2::conv_bband_check_counts(a); tf2::conv_c3_check_counts(b);
  out[0] = a[0] + b[0]; out[1] = a[1] + b[1];
  return 0;
}
#endif

uint8_t tf2_get_real(float w, int8_t expand) { return get_real(w, expand); }

tf2_status tf2_net_create(const tf2_net_desc* nd, const tf2_layer_desc* layers, tf2_net** out) {
  if (!nd || !layers || !out) return arg_refusal("tf2_net_create", "null argument");
  // the option snapshot (TF2_AMD_OPTS, opts.h) is taken here and by tf2_net_reload_options, nowhere else
  { const std::string e = opts_reload(); if (!e.empty()) { set_error(e); return TF2_ERR_ARG; } }
  tf2_net* n = new (std::nothrow) tf2_net();
  if (!n) { set_error("out of memory"); return TF2_ERR_SIZE; }
  tf2_status st = n->impl.init(nd, layers);
  if (st != TF2_OK) { delete n; return st; }
  n->impl.load_options();
  *out = n;
  return TF2_OK;
}

void tf2_net_destroy(tf2_net* net) {
  if (!net) return;
  net->impl.drain_profile();
  delete net;
}

tf2_status tf2_quantization(const tf2_net* net, const char* q_text, size_t q_text_len, int8_t* q,
                            size_t q_capacity, int32_t* n_values_read) {
  CHECK_NET(net);
  if (!q_text || !q) return arg_refusal("tf2_quantization", "null argument");
  return net->impl.quantization(q_text, q_text_len, q, q_capacity, n_values_read);
}

tf2_status tf2_net_set_q(tf2_net* net, const int8_t* q, size_t n_bytes) {
  CHECK_NET(net);
  const size_t need = (size_t)net->impl.nd.n_q_rows * net->impl.nd.max_out_channel;
  if (!q || n_bytes != need) { set_error("tf2_net_set_q: expected " + std::to_string(need) + " bytes"); return TF2_ERR_SIZE; }
  net->impl.q.assign(q, q + n_bytes);
  net->impl.model_loaded = false;
  net->impl.packed_valid = false;
  net->impl.launch_plans.clear();
  return TF2_OK;
}

tf2_status tf2_net_load_model(tf2_net* net, const float* model, size_t n_floats) {
  CHECK_NET(net);
  if (!model) return arg_refusal("tf2_net_load_model", "null model");
  return net->impl.load_model(model, n_floats);
}

tf2_status tf2_model4bit_decode(const void* bytes, size_t n_bytes, float* floats, size_t capacity, size_t* n_floats) {
  if (!bytes) return arg_refusal("tf2_model4bit_decode", "null input");
  std::vector<float> out;
  size_t cnt = 0;
  const std::string err = tf2::model4bit_decode((const uint8_t*)bytes, n_bytes, floats ? &out : nullptr, &cnt);
  if (!err.empty()) { set_error(err); return TF2_ERR_ARG; }
  if (n_floats) *n_floats = cnt;
  if (floats) {
    if (capacity < cnt) { set_error("tf2_model4bit_decode: buffer too small"); return TF2_ERR_SIZE; }
    std::memcpy(floats, out.data(), cnt * sizeof(float));
  }
  return TF2_OK;
}

tf2_status tf2_net_load_model_4bit(tf2_net* net, const void* bytes, size_t n_bytes) {
  CHECK_NET(net);
  if (!bytes) return arg_refusal("tf2_net_load_model_4bit", "null input");
  return net->impl.load_model_4bit((const uint8_t*)bytes, n_bytes);
}

tf2_status tf2_net_get_codes(const tf2_net* net, int layer, uint8_t* codes, size_t capacity, size_t* n_bytes) {
  CHECK_NET(net);
  const Net& N = net->impl;
  if (!N.model_loaded || layer < 0 || layer >= N.nd.n_layers) { set_error("tf2_net_get_codes: no model / bad layer"); return TF2_ERR_STATE; }
  const auto& c = N.models[layer].codes;
  if (n_bytes) *n_bytes = c.size();
  if (codes) {
    if (capacity < c.size()) { set_error("tf2_net_get_codes: buffer too small"); return TF2_ERR_SIZE; }
    std::memcpy(codes, c.data(), c.size());
  }
  return TF2_OK;
}

tf2_status tf2_net_get_bias_bn(const tf2_net* net, int layer, int32_t* bias, int32_t* alpha, int32_t* beta, size_t capacity) {
  CHECK_NET(net);
  const Net& N = net->impl;
  if (!N.model_loaded || layer < 0 || layer >= N.nd.n_layers) { set_error("tf2_net_get_bias_bn: no model / bad layer"); return TF2_ERR_STATE; }
  const LayerModel& m = N.models[layer];
  if (capacity < m.bias.size()) { set_error("tf2_net_get_bias_bn: buffer too small"); return TF2_ERR_SIZE; }
  if (bias) std::memcpy(bias, m.bias.data(), m.bias.size() * 4);
  if (alpha) std::memcpy(alpha, m.alpha.data(), m.alpha.size() * 4);
  if (beta) std::memcpy(beta, m.beta.data(), m.beta.size() * 4);
  return TF2_OK;
}

tf2_status tf2_net_pack(tf2_net* net, int mode) { CHECK_NET(net); net->impl.launch_plans.clear(); net->impl.plans.clear(); return net->impl.pack(mode); }

size_t tf2_net_packed_size(const tf2_net* net) { return net && net->impl.packed_valid ? net->impl.packed.size() : 0; }

tf2_status tf2_net_packed_copy(const tf2_net* net, void* host_dst, size_t capacity) {
  CHECK_NET(net);
  if (!net->impl.packed_valid) { set_error("tf2_net_packed_copy: nothing packed"); return TF2_ERR_STATE; }
  if (!host_dst || capacity < net->impl.packed.size()) { set_error("tf2_net_packed_copy: buffer too small"); return TF2_ERR_SIZE; }
  std::memcpy(host_dst, net->impl.packed.data(), net->impl.packed.size());
  return TF2_OK;
}

tf2_status tf2_net_packed_adopt(tf2_net* net, const void* host_src, size_t n_bytes) {
  CHECK_NET(net);
  Net& N = net->impl;
  if (!host_src || n_bytes < sizeof(PackHeader)) { set_error("tf2_net_packed_adopt: image too small"); return TF2_ERR_SIZE; }
  PackHeader h;
  std::memcpy(&h, host_src, sizeof h);
  if (h.magic != kPackMagic || h.version != kPackVersion) return arg_refusal("tf2_net_packed_adopt", "not a tf2_amd packed image of this version");
  if (h.total_bytes != n_bytes || h.n_layers != (uint32_t)N.nd.n_layers) { set_error("tf2_net_packed_adopt: size / layer count mismatch"); return TF2_ERR_SIZE; }
  if (h.tables_hash != N.tables_hash()) return arg_refusal("tf2_net_packed_adopt", "image was packed for different network tables");
  N.packed.assign((const uint8_t*)host_src, (const uint8_t*)host_src + n_bytes);
  N.packed_valid = true;
  N.packed_dev = nullptr; N.packed_dev_bytes = 0;
  N.launch_plans.clear(); N.plans.clear();
  return TF2_OK;
}

tf2_status tf2_net_bind_device(tf2_net* net, const void* packed_dev, size_t n_bytes) {
  CHECK_NET(net);
  Net& N = net->impl;
  if (!N.packed_valid) { set_error("tf2_net_bind_device: nothing packed"); return TF2_ERR_STATE; }
  if (!packed_dev || n_bytes != N.packed.size()) { set_error("tf2_net_bind_device: size mismatch"); return TF2_ERR_SIZE; }
  N.packed_dev = (const uint8_t*)packed_dev;
  N.packed_dev_bytes = n_bytes;
  N.launch_plans.clear();
  return TF2_OK;
}

size_t tf2_net_workspace_size(tf2_net* net, int batch, int keep_all) {
  if (!net || batch <= 0) return 0;
  return net->impl.workspace_size(batch, keep_all != 0);
}

size_t tf2_net_logits_size(const tf2_net* net, int batch) {
  if (!net || batch <= 0) return 0;
  return net->impl.logits_bytes(batch);
}

tf2_status tf2_net_reload_options(tf2_net* net) {
  CHECK_NET(net);
  { const std::string e = opts_reload(); if (!e.empty()) { set_error(e); return TF2_ERR_ARG; } }
  net->impl.load_options();
  return TF2_OK;
}

tf2_status tf2_net_run(tf2_net* net, const float* images_dev, int batch, void* ws, size_t ws_bytes,
                       int8_t* logits_dev, void* hip_stream) {
  CHECK_NET(net);
  if (!images_dev || !ws) return arg_refusal("tf2_net_run", "null device pointer");
  return net->impl.run(images_dev, false, batch, ws, ws_bytes, logits_dev, hip_stream);
}

tf2_status tf2_net_run_q(tf2_net* net, const int8_t* images_q_dev, int batch, void* ws, size_t ws_bytes,
                         int8_t* logits_dev, void* hip_stream) {
  CHECK_NET(net);
  if (!images_q_dev || !ws) return arg_refusal("tf2_net_run_q", "null device pointer");
  return net->impl.run(images_q_dev, true, batch, ws, ws_bytes, logits_dev, hip_stream);
}

tf2_status tf2_net_run_ex(tf2_net* net, const void* images_dev, int batch, void* ws, size_t ws_bytes, int8_t* logits_dev,
                          void* hip_stream, const tf2_run_opts* o) {
  CHECK_NET(net);
  if (!images_dev || !ws) return arg_refusal("tf2_net_run_ex", "null device pointer");
  if (!o || o->size < sizeof(tf2_run_opts)) return arg_refusal("tf2_net_run_ex", "opts missing or older than this library's tf2_run_opts");
  if (o->concurrency < -1 || o->concurrency > 1) return arg_refusal("tf2_net_run_ex", "concurrency must be -1, 0 or 1");
  if (o->mark_event && (o->mark_after_layer < 0 || o->mark_after_layer >= net->impl.nd.n_layers)) {
    set_error("tf2_net_run_ex: mark_after_layer outside the layer table"); return TF2_ERR_ARG;
  }
  return net->impl.run(images_dev, o->images_are_q != 0, batch, ws, ws_bytes, logits_dev, hip_stream, o->concurrency, o->mark_event, o->mark_after_layer);
}

tf2_status tf2_net_run_stats(tf2_net* net, int64_t* out4) {
  CHECK_NET(net);
  if (!out4) return arg_refusal("tf2_net_run_stats", "null argument");
  std::lock_guard<std::mutex> lock(net->impl.run_mutex);
  out4[0] = net->impl.stat_steps; out4[1] = net->impl.stat_group_steps; out4[2] = net->impl.stat_inflight_steps; out4[3] = net->impl.stat_small_mask_steps;
  return TF2_OK;
}

tf2_status tf2_net_poll_error(tf2_net* net, int batch, void* workspace, size_t workspace_bytes, void* stream) {
  CHECK_NET(net);
  std::lock_guard<std::mutex> lock(net->impl.run_mutex);
  return net->impl.poll_error(batch, workspace, workspace_bytes, stream);
}

tf2_status tf2_net_describe_launches(tf2_net* net, int batch, int concurrency, tf2_launch_info* rows, int capacity, int* n) {
  CHECK_NET(net);
  if (!n || (capacity > 0 && !rows)) return arg_refusal("tf2_net_describe_launches", "null argument");
  std::vector<std::pair<int, LaunchRecord>> v;
  tf2_status st = net->impl.describe_launches(batch, concurrency != 0, &v);
  if (st != TF2_OK) return st;
  *n = (int)v.size();
  if ((int)v.size() > capacity) { set_error("tf2_net_describe_launches: " + std::to_string(v.size()) + " launches, capacity " + std::to_string(capacity)); return TF2_ERR_SIZE; }
  for (size_t i = 0; i < v.size(); i++) {
    tf2_launch_info& r = rows[i];
    r.layer = v[i].first; r.grid = (int32_t)v[i].second.grid; r.block = (int32_t)v[i].second.block;
    r.lds_bytes = (int32_t)v[i].second.lds; r.vgprs = v[i].second.vgprs;
    std::memcpy(r.kernel, v[i].second.kernel, sizeof r.kernel);
  }
  return TF2_OK;
}

tf2_status tf2_net_describe_workspace(tf2_net* net, int batch, int keep_all, tf2_tensor_info* tensors, int tensor_capacity, int* n_tensors,
                                      tf2_row_tensors* rows, int row_capacity) {
  CHECK_NET(net);
  if (!n_tensors || (tensor_capacity > 0 && !tensors) || (row_capacity > 0 && !rows)) return arg_refusal("tf2_net_describe_workspace", "null argument");
  std::vector<tf2::TensorPlan> t;
  std::vector<tf2::LayerExec> r;
  tf2_status st = net->impl.describe_workspace(batch, keep_all != 0, &t, &r);
  if (st != TF2_OK) return st;
  *n_tensors = (int)t.size();
  if ((int)t.size() > tensor_capacity || (int)r.size() > row_capacity) { set_error("tf2_net_describe_workspace: " + std::to_string(t.size()) + " tensors, " + std::to_string(r.size()) + " rows: capacity too small"); return TF2_ERR_SIZE; }
  for (size_t i = 0; i < t.size(); i++) {
    tensors[i].offset = (int64_t)t[i].offset; tensors[i].bytes = (int64_t)t[i].bytes;
    tensors[i].first_row = t[i].first_use; tensors[i].last_row = t[i].last_use;
  }
  for (size_t i = 0; i < r.size(); i++) {
    rows[i].in_tensor = r[i].in_tensor; rows[i].out_tensor = r[i].out_tensor; rows[i].conv_tensor = r[i].conv_tensor; rows[i].res_tensor = r[i].res_tensor;
  }
  return TF2_OK;
}

tf2_status tf2_ssd_create(tf2_net* net, const tf2_ssd_desc* d, tf2_ssd** out) {
  CHECK_NET(net);
  if (!d || !out) return arg_refusal("tf2_ssd_create", "null argument");
  tf2_ssd* s = new (std::nothrow) tf2_ssd();
  if (!s) { set_error("out of memory"); return TF2_ERR_SIZE; }
  const tf2_status st = s->impl.create(&net->impl, d);
  if (st != TF2_OK) { delete s; return st; }
  *out = s;
  return TF2_OK;
}

void tf2_ssd_destroy(tf2_ssd* s) { delete s; }

size_t tf2_ssd_workspace_size(tf2_ssd* s, int batch) { return s ? s->impl.workspace_size(batch) : 0; }

size_t tf2_ssd_detect_scratch_size(tf2_ssd* s, int batch) { return s ? s->impl.detect_scratch_size(batch) : 0; }

tf2_status tf2_ssd_run(tf2_ssd* s, const void* images_dev, int images_are_q, int batch, void* ws, size_t ws_bytes, float* det_dev,
                       int32_t* counts_dev, float* boxes_out, float* scores_out, int8_t* logits_out, void* mark_event, void* hip_stream) {
  if (!s) { set_error("null tf2_ssd handle"); return TF2_ERR_ARG; }
  return s->impl.run(images_dev, images_are_q != 0, batch, ws, ws_bytes, det_dev, counts_dev, boxes_out, scores_out, logits_out, mark_event,
                     hip_stream);
}

tf2_status tf2_ssd_detect(tf2_ssd* s, const float* boxes_dev, const float* scores_dev, int batch, void* scratch, size_t scratch_bytes,
                          float* det_dev, int32_t* counts_dev, void* hip_stream) {
  if (!s) { set_error("null tf2_ssd handle"); return TF2_ERR_ARG; }
  return s->impl.detect(boxes_dev, scores_dev, batch, scratch, scratch_bytes, det_dev, counts_dev, hip_stream);
}

tf2_status tf2_preprocess(const tf2_net* net, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                          const tf2_image_src* srcs_dev, int batch, int out_q, void* out_dev, int32_t* status_dev, void* stream) {
  CHECK_NET(net);
  return preprocess(net->impl, d, pixels_dev, pixels_bytes, srcs_dev, batch, out_q, out_dev, status_dev, stream);
}

tf2_status tf2_preprocess_aa(const tf2_net* net, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                             const tf2_image_src* srcs_dev, int batch, int out_q, void* out_dev, int32_t* status_dev, void* stream) {
  CHECK_NET(net);
  return preprocess_aa(net->impl, d, pixels_dev, pixels_bytes, srcs_dev, batch, out_q, out_dev, status_dev, stream);
}

tf2_status tf2_roi_select(const tf2_roi_desc* d, const float* det_dev, const int32_t* counts_dev, const tf2_image_src* srcs_dev, int batch,
                          tf2_roi* rois_dev, int32_t* roi_counts_dev, void* stream) {
  return roi_select(d, det_dev, counts_dev, srcs_dev, batch, rois_dev, roi_counts_dev, stream);
}

tf2_status tf2_roi_crop(const tf2_net* net2, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                        const tf2_image_src* srcs_dev, int batch, const tf2_roi* rois_dev, int n_slots, int out_q, void* out_dev,
                        int32_t* status_dev, void* stream) {
  CHECK_NET(net2);
  return roi_crop(net2->impl, d, pixels_dev, pixels_bytes, srcs_dev, batch, rois_dev, n_slots, out_q, out_dev, status_dev, stream);
}

tf2_status tf2_roi_crop_aa(const tf2_net* net2, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                           const tf2_image_src* srcs_dev, int batch, const tf2_roi* rois_dev, int n_slots, int out_q, void* out_dev,
                           int32_t* status_dev, void* stream) {
  CHECK_NET(net2);
  return roi_crop_aa(net2->impl, d, pixels_dev, pixels_bytes, srcs_dev, batch, rois_dev, n_slots, out_q, out_dev, status_dev, stream);
}

tf2_status tf2_roi_fit(const tf2_roi_fit_desc* d, const tf2_roi* rois_dev, const float* lmk_dev, int n_slots, tf2_roi_xform* xf_dev,
                       int32_t* status_dev, void* stream) {
  return roi_fit(d, rois_dev, lmk_dev, n_slots, xf_dev, status_dev, stream);
}

tf2_status tf2_roi_warp(const tf2_net* net2, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                        const tf2_image_src* srcs_dev, int batch, const tf2_roi_xform* xf_dev, int n_slots, int out_q, void* out_dev,
                        int32_t* status_dev, void* stream) {
  CHECK_NET(net2);
  return roi_warp(net2->impl, d, pixels_dev, pixels_bytes, srcs_dev, batch, xf_dev, n_slots, out_q, out_dev, status_dev, stream);
}

tf2_status tf2_ycc_to_rgb(const tf2_ycc_desc* d, const uint8_t* src_dev, size_t src_bytes, const tf2_ycc_src* ycc_dev, uint8_t* pixels_dev,
                          size_t pixels_bytes, const tf2_image_src* srcs_dev, int batch, int32_t* status_dev, void* stream) {
  return ycc_to_rgb(d, src_dev, src_bytes, ycc_dev, pixels_dev, pixels_bytes, srcs_dev, batch, status_dev, stream);
}

// (tf2_jpeg_parse and tf2_jpeg_entropy are defined in jpeg_entropy.cpp, which builds without the rest of the library)
tf2_status tf2_jpeg_idct(const tf2_jpeg_desc* d, const int16_t* coef_dev, size_t coef_blocks, const tf2_jpeg_src* jpeg_dev,
                         const uint16_t* quant_dev, uint8_t* planes_dev, size_t planes_bytes, const tf2_ycc_src* ycc_dev,
                         const tf2_image_src* srcs_dev, int batch, int32_t* status_dev, void* stream) {
  return jpeg_idct(d, coef_dev, coef_blocks, jpeg_dev, quant_dev, planes_dev, planes_bytes, ycc_dev, srcs_dev, batch, status_dev, stream);
}

// (tf2_jpeg_scan_fill is defined in jpeg_entropy.cpp too)
size_t tf2_jpeg_huff_work_bytes(const tf2_jpeg_huff_desc* d, int batch, size_t max_scan_bytes) {
  return jpeg_huff_work_bytes(d, batch, max_scan_bytes);
}

tf2_status tf2_jpeg_huff(const tf2_jpeg_huff_desc* d, const uint8_t* bytes_dev, size_t bytes_len, const tf2_jpeg_scan* scan_dev,
                         const tf2_jpeg_src* jpeg_dev, int16_t* coef_dev, size_t coef_blocks, uint8_t* work_dev, size_t work_bytes,
                         int batch, int32_t* status_dev, void* stream) {
  return jpeg_huff(d, bytes_dev, bytes_len, scan_dev, jpeg_dev, coef_dev, coef_blocks, work_dev, work_bytes, batch, status_dev, stream);
}

tf2_status tf2_cls_create(tf2_net* net, const tf2_cls_desc* d, tf2_cls** out) {
  CHECK_NET(net);
  if (!out) return arg_refusal("tf2_cls_create", "null argument");
  tf2_cls* c = new (std::nothrow) tf2_cls();
  if (!c) { set_error("out of memory"); return TF2_ERR_SIZE; }
  const tf2_status st = c->impl.create(&net->impl, d);
  if (st != TF2_OK) { delete c; return st; }
  *out = c;
  return TF2_OK;
}

void tf2_cls_destroy(tf2_cls* c) { delete c; }

tf2_status tf2_cls_run(tf2_cls* c, const int8_t* logits_dev, int batch, int32_t* labels_dev, float* features_dev, float* probs_dev,
                       float* all_probs_dev, const int32_t* truth_dev, int32_t* rank_dev, uint64_t* tally_dev, void* stream) {
  if (batch < 1) return arg_refusal("tf2_cls_run", "batch must be >= 1");
  if (!logits_dev || !labels_dev) return arg_refusal("tf2_cls_run", "null logits_dev / labels_dev");
  if (!c) { set_error("null tf2_cls handle"); return TF2_ERR_ARG; }
  return c->impl.run(logits_dev, batch, labels_dev, features_dev, probs_dev, all_probs_dev, truth_dev, rank_dev, tally_dev, stream);
}

tf2_status tf2_emb_create(tf2_net* net, const tf2_emb_desc* d, tf2_emb** out) {
  CHECK_NET(net);
  if (!out) return arg_refusal("tf2_emb_create", "null argument");
  tf2_emb* m = new (std::nothrow) tf2_emb();
  if (!m) { set_error("out of memory"); return TF2_ERR_SIZE; }
  const tf2_status st = m->impl.create(&net->impl, d);
  if (st != TF2_OK) { delete m; return st; }
  *out = m;
  return TF2_OK;
}

void tf2_emb_destroy(tf2_emb* m) { delete m; }

size_t tf2_emb_scratch_size(const tf2_emb* m, int batch, int n_rows) { return m ? m->impl.scratch_size(batch, n_rows) : 0; }

tf2_status tf2_emb_embed(tf2_emb* m, const int8_t* out_i8_dev, int batch, float* rows_dev, void* stream) {
  if (batch < 1) return arg_refusal("tf2_emb_embed", "batch must be >= 1");
  if (!out_i8_dev || !rows_dev) return arg_refusal("tf2_emb_embed", "null out_i8_dev / rows_dev");
  if (!m) { set_error("null tf2_emb handle"); return TF2_ERR_ARG; }
  return m->impl.embed(out_i8_dev, batch, rows_dev, stream);
}

tf2_status tf2_emb_match(tf2_emb* m, const int8_t* out_i8_dev, int batch, const float* gallery_dev, const int32_t* gallery_ids_dev,
                         int n_rows, float threshold, void* scratch_dev, size_t scratch_bytes, int32_t* idx_dev, float* dist_dev,
                         int32_t* ids_out_dev, float* emb_out_dev, const int32_t* truth_dev, uint64_t* tally_dev, void* stream) {
  if (batch < 1) return arg_refusal("tf2_emb_match", "batch must be >= 1");
  if (n_rows < 1) return arg_refusal("tf2_emb_match", "n_rows must be >= 1");
  if (!out_i8_dev || !gallery_dev) return arg_refusal("tf2_emb_match", "null out_i8_dev / gallery_dev");
  if (!scratch_dev) return arg_refusal("tf2_emb_match", "null scratch_dev");
  if (!idx_dev || !dist_dev) return arg_refusal("tf2_emb_match", "null idx_dev / dist_dev");
  if (threshold != threshold) return arg_refusal("tf2_emb_match", "threshold is NaN");
  if (!m) { set_error("null tf2_emb handle"); return TF2_ERR_ARG; }
  return m->impl.match(out_i8_dev, batch, gallery_dev, gallery_ids_dev, n_rows, threshold, scratch_dev, scratch_bytes, idx_dev, dist_dev,
                       ids_out_dev, emb_out_dev, truth_dev, tally_dev, stream);
}

tf2_status tf2_emb_roc_hist(const float* rows_a_dev, const int32_t* ids_a_dev, int n_a, const float* rows_b_dev, const int32_t* ids_b_dev,
                            int n_b, int d, int n_thr, float step, int64_t* hist_dev, void* stream) {
  return emb_roc_hist(rows_a_dev, ids_a_dev, n_a, rows_b_dev, ids_b_dev, n_b, d, n_thr, step, hist_dev, stream);
}

tf2_status tf2_emb_roc_pairs(const float* rows_dev, int n_rows, int d, const int32_t* pairs_dev, int n_pairs, int n_folds, int n_thr,
                             float step, float* dist_dev, int64_t* hist_dev, int64_t* invalid_dev, void* stream) {
  return emb_roc_pairs(rows_dev, n_rows, d, pairs_dev, n_pairs, n_folds, n_thr, step, dist_dev, hist_dev, invalid_dev, stream);
}

tf2_status tf2_audit_create(tf2_net* net, tf2_audit** out) { return create_observer("tf2_audit_create", net, out); }

void tf2_audit_destroy(tf2_audit* a) { delete a; }

size_t tf2_audit_store_size(const tf2_audit* a) { return a ? a->impl.store_size() : 0; }

tf2_status tf2_audit_describe(const tf2_audit* a, tf2_audit_row* rows, int capacity, int* n) {
  if (!a) { set_error("null tf2_audit handle"); return TF2_ERR_ARG; }
  return a->impl.g.describe("tf2_audit_describe", kAuditSlots, rows, capacity, n);
}

tf2_status tf2_audit_store_init(const tf2_audit* a, void* store_dev, size_t store_bytes, void* hip_stream) {
  if (!a) { set_error("null tf2_audit handle"); return TF2_ERR_ARG; }
  return a->impl.store_init(store_dev, store_bytes, hip_stream);
}

size_t tf2_audit_workspace_size(tf2_audit* a, int batch) { return a ? a->impl.workspace_size(batch) : 0; }

tf2_status tf2_audit_run(tf2_audit* a, const void* images_dev, int images_are_q, int batch, void* ws, size_t ws_bytes, int8_t* logits_dev,
                         void* store_dev, size_t store_bytes, void* hip_stream) {
  if (!a) { set_error("null tf2_audit handle"); return TF2_ERR_ARG; }
  return a->impl.run(images_dev, images_are_q != 0, batch, ws, ws_bytes, logits_dev, store_dev, store_bytes, hip_stream);
}

tf2_status tf2_audit_kept(tf2_audit* a, const void* images_dev, int images_are_q, int batch, void* ws, size_t ws_bytes, void* store_dev,
                          size_t store_bytes, void* hip_stream) {
  if (!a) { set_error("null tf2_audit handle"); return TF2_ERR_ARG; }
  return a->impl.run(images_dev, images_are_q != 0, batch, ws, ws_bytes, nullptr, store_dev, store_bytes, hip_stream, false);
}

tf2_status tf2_fid_create(tf2_net* net, tf2_fid** out) { return create_observer("tf2_fid_create", net, out); }

void tf2_fid_destroy(tf2_fid* f) { delete f; }

size_t tf2_fid_store_size(const tf2_fid* f) { return f ? f->impl.store_size() : 0; }

tf2_status tf2_fid_describe(const tf2_fid* f, tf2_audit_row* rows, int capacity, int* n) {
  if (!f) { set_error("null tf2_fid handle"); return TF2_ERR_ARG; }
  return f->impl.g.describe("tf2_fid_describe", kFidSlots, rows, capacity, n);
}

tf2_status tf2_fid_scales(const tf2_fid* f, float* scales, int capacity, int* n) {
  if (!f) { set_error("null tf2_fid handle"); return TF2_ERR_ARG; }
  if (!n || (capacity > 0 && !scales)) return arg_refusal("tf2_fid_scales", "null argument");
  const auto& v = f->impl.scale;
  *n = (int)v.size();
  if ((int)v.size() > capacity) { set_error("tf2_fid_scales: " + std::to_string(v.size()) + " records, capacity " + std::to_string(capacity)); return TF2_ERR_SIZE; }
  std::copy(v.begin(), v.end(), scales);
  return TF2_OK;
}

tf2_status tf2_fid_store_init(const tf2_fid* f, void* store_dev, size_t store_bytes, void* hip_stream) {
  if (!f) { set_error("null tf2_fid handle"); return TF2_ERR_ARG; }
  return f->impl.store_init(store_dev, store_bytes, hip_stream);
}

size_t tf2_fid_workspace_size(tf2_fid* f, int batch) { return f ? f->impl.workspace_size(batch) : 0; }

tf2_status tf2_fid_run(tf2_fid* f, const void* images_dev, int images_are_q, int batch, void* ws, size_t ws_bytes, int8_t* logits_dev,
                       const float* const* refs, const float* scales_dev, void* store_dev, size_t store_bytes, void* hip_stream) {
  if (!f) { set_error("null tf2_fid handle"); return TF2_ERR_ARG; }
  return f->impl.run(images_dev, images_are_q != 0, batch, ws, ws_bytes, logits_dev, store_dev, store_bytes, refs, scales_dev, hip_stream);
}

tf2_status tf2_fid_kept(tf2_fid* f, const void* images_dev, int images_are_q, int batch, void* ws, size_t ws_bytes,
                        const float* const* refs, const float* scales_dev, void* store_dev, size_t store_bytes, void* hip_stream) {
  if (!f) { set_error("null tf2_fid handle"); return TF2_ERR_ARG; }
  return f->impl.run(images_dev, images_are_q != 0, batch, ws, ws_bytes, nullptr, store_dev, store_bytes, refs, scales_dev, hip_stream, false);
}

size_t tf2_caq_range_store_size(int64_t n_records) { return n_records < 1 ? 0 : caq_range_store_size(n_records); }

size_t tf2_caq_error_store_size(int64_t n_records) { return n_records < 1 ? 0 : caq_error_store_size(n_records); }

tf2_status tf2_caq_store_init(void* store_dev, size_t store_bytes, void* hip_stream) { return caq_store_init(store_dev, store_bytes, hip_stream); }

tf2_status tf2_caq_range(const tf2_caq_row* rows, const void* const* maps, int n_rows, int batch, void* store_dev, size_t store_bytes,
                         void* hip_stream) {
  return caq_run(false, rows, maps, n_rows, batch, nullptr, store_dev, store_bytes, hip_stream);
}

tf2_status tf2_caq_error(const tf2_caq_row* rows, const void* const* maps, int n_rows, int batch, const float* scales_dev, void* store_dev,
                         size_t store_bytes, void* hip_stream) {
  return caq_run(true, rows, maps, n_rows, batch, scales_dev, store_dev, store_bytes, hip_stream);
}

size_t tf2_dnscp_state_size(int n_convs) { return n_convs < 1 ? 0 : dnscp_state_size(n_convs); }

size_t tf2_dnscp_scratch_size(int) { return 0; }

tf2_status tf2_dnscp_stats(const float* weights_dev, int64_t n_total, const tf2_dnscp_conv* convs, int n_convs, const uint8_t* keep_dev,
                           int64_t n_channels, int64_t* sums_dev, void* state_dev, void* scratch_dev, size_t scratch_bytes, void* hip_stream) {
  return dnscp_run(weights_dev, nullptr, n_total, convs, n_convs, const_cast<uint8_t*>(keep_dev), n_channels, (long long*)sums_dev, state_dev,
                   scratch_dev, scratch_bytes, hip_stream, false);
}

tf2_status tf2_dnscp_step(const float* dense_dev, float* out_dev, int64_t n_total, const tf2_dnscp_conv* convs, int n_convs, uint8_t* keep_dev,
                          int64_t n_channels, int64_t* sums_dev, void* state_dev, void* scratch_dev, size_t scratch_bytes, void* hip_stream) {
  return dnscp_run(dense_dev, out_dev, n_total, convs, n_convs, keep_dev, n_channels, (long long*)sums_dev, state_dev, scratch_dev,
                   scratch_bytes, hip_stream, true);
}

tf2_status tf2_dnscp_compact(const float* src_dev, int64_t n_src, float* dst_dev, int64_t n_dst, const tf2_dnscp_seg* segs, int n_segs,
                             const int32_t* idx_dev, int64_t n_idx, void* hip_stream) {
  return dnscp_compact(src_dev, n_src, dst_dev, n_dst, segs, n_segs, idx_dev, n_idx, hip_stream);
}

size_t tf2_inq_scratch_size(int n_segs) { return n_segs < 1 ? 0 : inq_scratch_size(n_segs); }

size_t tf2_inq_state_size(int n_segs) { return n_segs < 1 ? 0 : inq_state_size(n_segs); }

tf2_status tf2_inq_step(float* weights_dev, uint8_t* mask_dev, int64_t n_total, const tf2_inq_seg* segs, int n_segs, double prev, double cur,
                        int n_values, int exp_floor, uint8_t* codes_dev, void* state_dev, void* scratch_dev, size_t scratch_bytes,
                        void* hip_stream) {
  return inq_step(weights_dev, mask_dev, n_total, segs, n_segs, prev, cur, n_values, exp_floor, codes_dev, state_dev, scratch_dev,
                  scratch_bytes, hip_stream);
}

tf2_status tf2_det_eval_create(const tf2_det_eval_desc* d, tf2_det_eval** out) {
  if (!out) return arg_refusal("tf2_det_eval_create", "null argument");
  tf2_det_eval* e = new (std::nothrow) tf2_det_eval();
  if (!e) { set_error("out of memory"); return TF2_ERR_SIZE; }
  const tf2_status st = e->impl.create(d);
  if (st != TF2_OK) { delete e; return st; }
  *out = e;
  return TF2_OK;
}

void tf2_det_eval_destroy(tf2_det_eval* e) { delete e; }

size_t tf2_det_eval_store_size(const tf2_det_eval* e) { return e ? e->impl.store_size() : 0; }

tf2_status tf2_det_eval_store_init(const tf2_det_eval* e, void* store_dev, size_t store_bytes, void* hip_stream) {
  if (!e) { set_error("null tf2_det_eval handle"); return TF2_ERR_ARG; }
  return e->impl.store_init(store_dev, store_bytes, hip_stream);
}

tf2_status tf2_det_eval_run(const tf2_det_eval* e, const float* det_dev, const int32_t* counts_dev, const tf2_gt_box* gt_dev,
                            const int32_t* gt_count_dev, const int32_t* slot_dev, int batch, void* store_dev, size_t store_bytes,
                            int32_t* status_dev, int8_t* flags_out_dev, void* hip_stream) {
  if (batch < 1) return arg_refusal("tf2_det_eval_run", "batch must be >= 1");
  if (!det_dev || !counts_dev) return arg_refusal("tf2_det_eval_run", "null det_dev / counts_dev");
  if (!gt_dev || !gt_count_dev || !slot_dev) return arg_refusal("tf2_det_eval_run", "null gt_dev / gt_count_dev / slot_dev");
  if (!store_dev || !status_dev) return arg_refusal("tf2_det_eval_run", "null store_dev / status_dev");
  if (!e) { set_error("null tf2_det_eval handle"); return TF2_ERR_ARG; }
  return e->impl.run(det_dev, counts_dev, gt_dev, gt_count_dev, slot_dev, batch, store_dev, store_bytes, status_dev, flags_out_dev, hip_stream);
}

tf2_status tf2_det_eval_summarise(const tf2_det_eval* e, const void* store_host, size_t store_bytes, int use_07_metric,
                                  tf2_det_eval_class* per_class, int64_t* images, double* map) {
  if (!e) { set_error("null tf2_det_eval handle"); return TF2_ERR_ARG; }
  return e->impl.summarise(store_host, store_bytes, use_07_metric, per_class, images, map);
}

tf2_status tf2_net_read_layer(tf2_net* net, int layer, int batch, const void* ws, int8_t* host_dst,
                              size_t capacity, void* hip_stream) {
  CHECK_NET(net);
  if (!ws || !host_dst) return arg_refusal("tf2_net_read_layer", "null pointer");
  return net->impl.read_layer(layer, batch, ws, host_dst, capacity, hip_stream);
}

tf2_status tf2_net_profile(tf2_net* net, int enable) {
  CHECK_NET(net);
  Net& N = net->impl;
  N.drain_profile();
  if (enable) { std::fill(N.prof_ms.begin(), N.prof_ms.end(), 0.f); std::fill(N.prof_launches.begin(), N.prof_launches.end(), 0); N.prof_loop_ms = 0.f; N.prof_loop_n = 0; }
  N.profiling = enable == 1;
  N.profiling_loop = enable == 2;
  return TF2_OK;
}

tf2_status tf2_net_profile_read(tf2_net* net, float* ms, int32_t* launches, int32_t* kinds, int capacity) {
  CHECK_NET(net);
  Net& N = net->impl;
  if (capacity < N.nd.n_layers) { set_error("tf2_net_profile_read: capacity < n_layers"); return TF2_ERR_SIZE; }
  N.drain_profile();
  for (int l = 0; l < N.nd.n_layers; l++) {
    if (ms) ms[l] = N.prof_ms[l];
    if (launches) launches[l] = N.prof_launches[l];
    if (kinds) { const PackLayer* pl = N.pack_layer(l); kinds[l] = pl ? pl->kind : 0; }
  }
  return TF2_OK;
}

tf2_status tf2_net_profile_loop_read(tf2_net* net, float* ms_total, int32_t* runs) {
  CHECK_NET(net);
  Net& N = net->impl;
  N.drain_profile();
  if (ms_total) *ms_total = N.prof_loop_ms;
  if (runs) *runs = N.prof_loop_n;
  return TF2_OK;
}

// Evaluation(), network_helper.cpp:143-207: feature = out / (1 << Q); k bubble passes with
// '>' (ties: the larger index ends up on top).
tf2_status tf2_topk(const int8_t* logits, const int8_t* q_last_row, int n, int k, int32_t* labels, float* features) {
  if (!logits || !q_last_row || !labels || n <= 0 || k <= 0 || k > n) return arg_refusal("tf2_topk", "bad argument");
  std::vector<float> f(n);
  std::vector<int32_t> lab(n);
  for (int i = 0; i < n; i++) {
    const int sh = -(int)q_last_row[i];
    if (sh < 0 || sh > 30) return arg_refusal("tf2_topk", "Q of the last layer must be in 0..30 (network_helper.cpp:181)");
    f[i] = (float)logits[i] / (float)(1 << sh);
    lab[i] = i;
  }
  for (int pass = 0; pass < k; pass++)
    for (int j = 0; j + 1 < n - pass; j++)
      if (f[j] > f[j + 1]) { std::swap(f[j], f[j + 1]); std::swap(lab[j], lab[j + 1]); }
  for (int i = 0; i < k; i++) { labels[i] = lab[n - 1 - i]; if (features) features[i] = f[n - 1 - i]; }
  return TF2_OK;
}

}  // extern "C"
