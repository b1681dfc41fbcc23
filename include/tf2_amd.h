/*
 * tf2_amd.h -- C ABI of the MI355X-native drop-in for TF2's Runtime_Engine/cnn path.
 *
 * The reference has no plugin/FFI API for this path: it sits behind three C++ classes
 * and a handful of free functions compiled against one network header
 * (SURVEY.md section 8b).  Each entry point below names the reference interface it
 * replaces (paths relative to /root/reference/Runtime_Engine/cnn).  Plain pointers and
 * sizes only; no torch / HIP types in signatures (a stream is passed as void*).
 *
 * Conventions
 *   - every function returns 0 (TF2_OK) or a negative tf2_status; it never exits the
 *     process (the reference's checkError() -> exit(), common/src/AOCLUtils/opencl.cpp:226-250,
 *     is deliberately not reproduced); tf2_last_error() gives the message (thread-local).
 *   - "q" arrays hold the RUNTIME values of quantization.cpp:46, i.e. the NEGATED Q-file ints.
 *   - device pointers are raw HIP device addresses owned by the caller (PyTorch
 *     allocations); the library allocates no device memory in run calls.
 */
#ifndef TF2_AMD_H_
#define TF2_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int tf2_status;
enum {
  TF2_OK = 0,
  TF2_ERR_ARG = -1,        /* bad argument / inconsistent tables                      */
  TF2_ERR_STATE = -2,      /* call order (e.g. run before load_model)                 */
  TF2_ERR_SIZE = -3,       /* buffer too small / model stream length mismatch         */
  TF2_ERR_HIP = -4,        /* HIP runtime error (message carries hipGetErrorString)   */
  TF2_ERR_UNSUPPORTED = -5,/* layer shape not supported by any kernel                 */
  TF2_ERR_GROUP = -6       /* a group launch gave up a meeting (tf2_net_poll_error)   */
};

/* One row of the network program = one row of the k* tables of <net>.h
 * (host/inc/resnet50.h:119-1372), with the graph edges made explicit
 * (tf2_amd.config.build_plan).                                                        */
typedef struct tf2_layer_desc {
  int32_t src;          /* producer of the input: -1 image, >=0 layer, <=-2 concat -(id+2) (kInputLayer) */
  int32_t q_in_row;     /* Q-table row of the input channels (kInputLayer)               */
  int32_t C, H, W;      /* kInputChannels, kInputHeight, kInputWidth                     */
  int32_t N, k, stride; /* kOutputChannels, kFilterSize, kConvStride                     */
  int32_t pad_h, pad_w, dil; /* kPadHeight, kPadWidth, (dilation, 1 in the reference)    */
  int32_t OH, OW;       /* conv output (after conv stride)                               */
  int32_t bias_en, bn_en, relu, ipool; /* kBiasEnable, kBnEnable, kReluEnable, kIpoolEnable (1 = independent pooling row;
                           2 = this build's independent L2Norm row for SSD's conv4_3 branch: N float weights in
                           the model stream, its own Q row, no filter) */
  int32_t pool_en, pool_S, pool_st, pool_pad; /* kPoolEnable, kPoolWindow, kPoolStride2, kPoolPad */
  int32_t PH, PW;       /* kPoolOutputHeight/Width                                       */
  int32_t add_src, add_relu; /* kAdditionEnable (+ DDR page plan), kAdditionReluEnable   */
  int32_t endpool, endpool_mult; /* kEndPoolEnable; 669 for 7x7 (full_size_pool.cl:118)  */
  int32_t concat, n_start; /* kBranchTail/kConcatLayer, kNStart                          */
  int32_t model_C, model_k; /* filter dims in the model file (layer 0: INPUT_IMAGE_C, FIRST_FILTER_SIZE) */
} tf2_layer_desc;

typedef struct tf2_net_desc {
  int32_t n_layers;       /* NUM_LAYER                                                   */
  int32_t n_conv;         /* NUM_CONVOLUTIONS                                            */
  int32_t n_q_rows;       /* NUM_Q_LAYERS                                                */
  int32_t max_out_channel;/* MAX_OUT_CHANNEL                                             */
  int32_t image_c, image_h, image_w; /* INPUT_IMAGE_C/H/W                                */
  int32_t conv1_rewrite;  /* 1: layer 0 runs as 27-ch 3x3 on the 114x114 space-to-depth
                             image (model_loader.cpp:244-257, input_loader.cpp:98-116)   */
  int32_t n_concat;       /* number of concat tensors                                    */
} tf2_net_desc;

typedef struct tf2_net tf2_net;

/* ---- misc ------------------------------------------------------------------------ */
const char* tf2_last_error(void);
int tf2_abi_version(void);
/* 1 if the library was built with the gfx950 HIP kernels (always, for the shipped .so). */
int tf2_has_device_code(void);
/* 0 for the shipped library.  The same sources also build two TOOL libraries that must never serve a product: 1 = the timing-probe
 * build (-DTF2_PROBES: can leave work out of a step), 2 = the DMA-check build (-DTF2_CHECK_DMA: stamps and checks sentinels around every
 * LDS-DMA).  tf2_amd/_lib.py refuses to load a library whose kind is not 0 unless a tool asks for it (TF2_AMD_TOOL_LIB=1). */
int tf2_build_kind(void);

/* ---- load-time numerics (host CPU; replace model_loader.cpp / quantization.cpp) ----- */
/* Get_real(float, char): model_loader.cpp:98-126 */
uint8_t tf2_get_real(float w, int8_t expand);
/* Quantization(q, input, file): quantization.cpp:25-55.  Takes the Q-file TEXT. Fills
 * q[n_q_rows][max_out_channel] (caller zero-fills) from the net's layer table.        */
tf2_status tf2_quantization(const tf2_net* net, const char* q_text, size_t q_text_len,
                            int8_t* q, size_t q_capacity, int32_t* n_values_read);

/* ---- network handle (replaces NetWork::Init / InitNetwork / InitBuffer, network.cpp:22-150) */
tf2_status tf2_net_create(const tf2_net_desc* nd, const tf2_layer_desc* layers, tf2_net** out);
void tf2_net_destroy(tf2_net* net);
/* runtime q table [n_q_rows][max_out_channel] as produced by tf2_quantization */
tf2_status tf2_net_set_q(tf2_net* net, const int8_t* q, size_t n_bytes);
/* LoadModel(file, filter_raw, bias_bn, q): model_loader.cpp:129-258.  `model` is the
 * float32 stream of fpgamodel.bin / param.bin (already in memory).                     */
tf2_status tf2_net_load_model(tf2_net* net, const float* model, size_t n_floats);
/* The 4-bit packed model file of TransForm_Kit (Compression/compress_net/4bit_data_format.txt:1-44: per tensor
 * {int8 min_exp, int8 dtype, int16 N,C,H,W}, then 4-bit power-of-two codes in 16-bit words or float32).  The
 * reference documents the format and ships no reader; these are the canonical ones.  _decode: float32 LoadModel
 * stream into `floats` (capacity in floats; pass NULL/0 to get the count only).  _load_model_4bit walks the file in place:
 * every 4-bit code goes straight to the reference's byte code (Get_real of the code's value through a 16-entry table per
 * (tensor, expand)) -- no float32 copy of the weights is made; bit-identical to decode + LoadModel.                       */
tf2_status tf2_model4bit_decode(const void* bytes, size_t n_bytes, float* floats, size_t capacity, size_t* n_floats);
tf2_status tf2_net_load_model_4bit(tf2_net* net, const void* bytes, size_t n_bytes);
/* Introspection for per-function parity tests: byte codes [N][C][k][k] of a layer
 * (layer 0 after the conv1 rewrite: [N][27][3][3]) and its BiasBnParam (types.h:39-43). */
tf2_status tf2_net_get_codes(const tf2_net* net, int layer, uint8_t* codes, size_t capacity, size_t* n_bytes);
tf2_status tf2_net_get_bias_bn(const tf2_net* net, int layer, int32_t* bias, int32_t* alpha, int32_t* beta, size_t capacity);

/* ---- packed device image of the weights (what the one-time RCCL broadcast moves) ---- */
/* Options: conv kernel selection per layer class.  mode: 0 = auto (MFMA where the layer
 * qualifies, shift-accumulate VALU kernel otherwise), 1 = force the shift-accumulate
 * kernel for k>1 convs (MFMA for 1x1 only, the north-star split), 2 = shift kernel
 * everywhere.                                                                           */
tf2_status tf2_net_pack(tf2_net* net, int mode);
size_t tf2_net_packed_size(const tf2_net* net);
tf2_status tf2_net_packed_copy(const tf2_net* net, void* host_dst, size_t capacity);
/* Adopt a packed image received from another rank (host copy; same tables required).    */
tf2_status tf2_net_packed_adopt(tf2_net* net, const void* host_src, size_t n_bytes);
/* Tell the net where the packed image lives on the device (caller copied/broadcast it). */
tf2_status tf2_net_bind_device(tf2_net* net, const void* packed_dev, size_t n_bytes);

/* ---- running (replaces Runner::Run, runner.cpp:54-198, and the OpenCL device pipeline) */
/* keep_all != 0: every layer output gets its own buffer (per-layer parity tests).  Ask AFTER tf2_net_pack /
 * tf2_net_packed_adopt: the plan depends on which layer pairs the packed image runs as one launch (their inputs
 * stay live longer); a buffer sized before packing may be refused by tf2_net_run with TF2_ERR_SIZE.               */
size_t tf2_net_workspace_size(tf2_net* net, int batch, int keep_all);
/* Bytes of the dense int8 output of a run: [batch][H_last * W_last][N_last] (NHWC; H_last = W_last = 1 for the
 * classification networks, i.e. [batch][N_last] -- the buffer Runner::Run reads back, runner.cpp:176-186).      */
size_t tf2_net_logits_size(const tf2_net* net, int batch);
/* Options: ONE environment string, TF2_AMD_OPTS="name=value,name=value,flag" (INTEGRATION.md section 5 lists the product options:
 * alt_conc, bgroup, bband, c3, fc, fc4, share), parsed into an immutable snapshot at tf2_net_create and here -- nothing else in the
 * library reads the environment.  Unknown names, and test-only options (forced kernels, disabled proofs, thresholds: the test-suite's
 * and the A/B tools') without TF2_AMD_TEST=1, make both calls return TF2_ERR_ARG.  The snapshot is process-wide: packing (pack-time
 * options) and planning read the one taken last.  Drops the prepared launch plans.                              */
tf2_status tf2_net_reload_options(tf2_net* net);
/* images_dev: float32 [batch][image_c][image_h][image_w] on the device (the preprocessed
 * CHW floats LoadInputImage reads, input_loader.cpp:76-96).  Quantises with 2^Q0
 * (runner.cpp:158-164), runs every layer, writes the int8 output (tf2_net_logits_size bytes,
 * [batch][N_last] for a 1x1 final map) to logits_dev.  All kernel argument blocks of a step are
 * prepared once per (batch, workspace address) and reused by later calls.                       */
tf2_status tf2_net_run(tf2_net* net, const float* images_dev, int batch, void* workspace_dev,
                       size_t workspace_bytes, int8_t* logits_dev, void* hip_stream);
/* Same, from already-quantised int8 images [batch][image_c][image_h][image_w].          */
tf2_status tf2_net_run_q(tf2_net* net, const int8_t* images_q_dev, int batch, void* workspace_dev,
                         size_t workspace_bytes, int8_t* logits_dev, void* hip_stream);
/* The same step with per-call options (the reference has one frame loop on one command queue, runner.cpp:140-175; a
 * GPU server keeps several independent batches in flight on several streams):
 *  - images_are_q   1: int8 images (tf2_net_run_q), 0: float32.
 *  - concurrency    how the launch plan picks its tile shapes: 0 = this batch runs alone on the GPU, 1 = other batches are
 *                   in flight on other streams (their kernels fill the chip: wider tiles, unfused pairs), -1 = decide from
 *                   the streams of the last eight calls on this handle (what tf2_net_run does).  Results are bit-identical
 *                   whichever is chosen.
 *  - mark_event / mark_after_layer   a hipEvent_t recorded on hip_stream once every launch of layers 0..mark_after_layer
 *                   has been enqueued (ignored when mark_event is NULL).  A caller that pipelines batches lets the next
 *                   batch's stream wait for it (hipStreamWaitEvent), so that batch k+1 enters the chip-filling first
 *                   stage when batch k has left it instead of competing with it; bench.py does.
 * Threading: a handle may be used from several host threads, one stream AND one workspace per thread; the calls serialise
 * on an internal mutex only while they look up / build the launch plan, the enqueue of the step's launches runs side by side
 * (calls that share a workspace serialise for the whole enqueue; kernel execution is asynchronous as always).  Everything
 * else on a handle (create / set_q / load / pack / bind / reload_options / profile / destroy) must not run concurrently
 * with a run on the same handle; workspace_size / read_layer / describe_* / run_stats take the handle's mutex and may.  tf2_last_error
 * is per thread.                                                          */
typedef struct tf2_run_opts {
  uint32_t size;              /* sizeof(tf2_run_opts), for forward compatibility */
  int32_t images_are_q;
  int32_t concurrency;
  int32_t mark_after_layer;
  void* mark_event;
} tf2_run_opts;
tf2_status tf2_net_run_ex(tf2_net* net, const void* images_dev, int batch, void* workspace_dev, size_t workspace_bytes,
                          int8_t* logits_dev, void* hip_stream, const tf2_run_opts* opts);
/* Group launches (conv_bgroup.hip: the one-batch-at-a-time plan keeps the eight blocks of an image resident together, one block per
 * CU, and lets them meet inside the kernel) have PRECONDITIONS the library checks where it can and the caller owns where it cannot:
 *  - at least 64 CUs for the stream: checked per call of the one-batch-at-a-time path (hipExtStreamGetCUMask: the check counts MASK
 *    BITS, not granted CUs -- gfx950 ignores interleaved masks, so a stream masked to 32 interleaved bits is treated as small although
 *    it runs on the whole chip: safe, it merely loses the group launches); a stream masked to fewer runs the step without them.
 *  - one batch at a time: selected only for concurrency == 0, stated or inferred.  A caller that STATES concurrency = 0 on more than
 *    four streams of one device at once (or drives more than four handles that way) breaks the contract: each XCD has 32
 *    one-block slots, four concurrent group kernels always leave room for one complete group, a fifth need not -- a meeting
 *    that does not complete within 2^24 polls is given up and REPORTED (tf2_net_poll_error below: the step's logits are garbage, the
 *    context, the stream and every later step are intact; rounds 3-5 trapped here).  With
 *    concurrency = -1 (tf2_net_run) the library sees the several streams in its call history and never selects them there.
 *  - the workspace bytes behind the tensors (step counter, flags) are the library's; they are re-initialised by every step.
 * The batches-in-flight plan (concurrency = 1) has none of this: its fused launches (conv_bband.hip) exchange nothing between blocks.
 * tf2_net_run_stats: out4 = {steps run, steps whose plan had group launches, steps run with the in-flight plan, steps on a stream
 * of fewer than 64 CUs} since tf2_net_create -- what a test or a server asserts its deployment against.                          */
tf2_status tf2_net_run_stats(tf2_net* net, int64_t* out4);
/* Group launches that cannot complete REPORT, they never trap or hang the context (round 6): a block that has polled a meeting of its
 * image's eight members `bgroup_polls` times (1 << 24: seconds) writes a report into the workspace's error word and leaves the kernel, and
 * so do the other members of that image; every other image of the launch and every later launch run on (the affected step's logits are
 * garbage).  tf2_net_poll_error synchronises `stream`, reads and clears the error word of the workspace that was used for `batch` images and
 * returns TF2_ERR_GROUP (tf2_last_error says which meeting) or TF2_OK; the report is sticky across later steps until it is polled.  A
 * server polls where it synchronises anyway (when it reads a batch's logits).  Steps of the in-flight plan (concurrency = 1) have no group
 * launches and nothing to report.  The reference has no counterpart (its kernels are statically scheduled, sequencer.cl). */
tf2_status tf2_net_poll_error(tf2_net* net, int batch, void* workspace, size_t workspace_bytes, void* stream);
/* Introspection: the kernel launches one step of `batch` images consists of, in issue order, as the library's own launch
 * plan selects them (concurrency as in tf2_run_opts: 0 or 1).  Needs a packed image, no device.  rows[i].layer = the table
 * row the launch belongs to (-1: input preparation; a fused launch carries its first row).  Returns the number of launches
 * in *n (also when capacity is too small: TF2_ERR_SIZE).  tools/pmc_summary.py attaches rocprofv3 rows to layers with it. */
typedef struct tf2_launch_info {
  int32_t layer, grid, block, lds_bytes, vgprs;
  char kernel[96];
} tf2_launch_info;
tf2_status tf2_net_describe_launches(tf2_net* net, int batch, int concurrency, tf2_launch_info* rows, int capacity, int* n);
/* The liveness-planned workspace of `batch` images (no device needed): tensor t occupies [offset, offset + bytes) from table row
 * first_row (-1: the input) to last_row (n_layers: the network output); row_capacity >= n_layers entries of `rows` say which
 * tensors a row reads (in, res: -1 = none) and writes (conv: the convolution's own result; out: after pool / average).  Rows that
 * share a launch (fused pairs, group launches and their chains) keep everything they touch alive for the whole launch: two
 * tensors of such rows never overlap (tests/test_host_abi.py).  The reference has no counterpart (its feature maps live in
 * fixed on-chip buffers, feature_writer.cl:88-151).                                                                          */
typedef struct tf2_tensor_info { int64_t offset, bytes; int32_t first_row, last_row; } tf2_tensor_info;
typedef struct tf2_row_tensors { int32_t in_tensor, out_tensor, conv_tensor, res_tensor; } tf2_row_tensors;
tf2_status tf2_net_describe_workspace(tf2_net* net, int batch, int keep_all, tf2_tensor_info* tensors, int tensor_capacity, int* n_tensors,
                                      tf2_row_tensors* rows, int row_capacity);
/* After a keep_all run: copy layer `layer`'s output to the host as dense NCHW int8
 * [batch][N][PH][PW] (or [batch][N] after an end pool).  layer == -1: the quantised,
 * transformed network input [batch][C0][H0][W0].  Synchronises the stream.
 * This is the ONLY way to look at an intermediate map: inside the workspace a tensor may be
 * stored in an engine-private form (x alone instead of [x | xneg] for the image, the im2col
 * image of a 3x3 first layer on 3 channels, 2x - 128 on the "doubled" channels of internal
 * post-ReLU tensors); read_layer hands back the reference's int8 values.                   */
tf2_status tf2_net_read_layer(tf2_net* net, int layer, int batch, const void* workspace_dev,
                              int8_t* host_dst, size_t capacity, void* hip_stream);
/* Per-kernel timing hook for bench.py: records HIP events around every conv launch of
 * the next tf2_net_run calls on `hip_stream`; tf2_net_profile_read returns, per layer,
 * the accumulated milliseconds and launch count since profiling was enabled.  enable == 2
 * records ONE event pair around the whole layer loop instead (tf2_net_profile_loop_read): every
 * per-layer pair adds its own record handling, the loop pair does not, so callers rescale the
 * per-layer sum to the loop time.                                                         */
tf2_status tf2_net_profile(tf2_net* net, int enable);
tf2_status tf2_net_profile_loop_read(tf2_net* net, float* ms_total, int32_t* runs);
tf2_status tf2_net_profile_read(tf2_net* net, float* ms_per_layer, int32_t* launches_per_layer,
                                int32_t* kernel_kind_per_layer, int capacity);

/* ---- SSD detection on the device (detection.py:27-62, box_utils.py:140-158 decode, :175-239 nms; INTEGRATION.md "SSD detection") ----
 * A detector belongs to a network handle (after pack / adopt; it reads the handle's q table and packed image at create: a later
 * set_q / pack needs a new detector).  tf2_ssd_create checks on the host, before any device call: every loc row has N = 4 * nb, the
 * conf row of the same source N = nb * num_classes on the same map, both are sinks (no row reads them) and not concat members,
 * sum over sources of H * W * nb == n_priors, num_classes in 2..256, top_k in 1..256, nms_thresh > 0, conf_thresh >= 0, n_priors
 * <= 32768; a failure is TF2_ERR_ARG with a message.  The handle holds read-only device constants (priors, the heads' 2^-Q scales);
 * everything a step writes lives in the caller's workspace, so several streams with their own workspaces run side by side.
 * Semantics: per image and class >= 1, candidates p > conf_thresh (strict), the best top_k of them by (score descending, prior
 * index ascending), greedy NMS in that order (a candidate survives unless its IoU with a kept box is > nms_thresh), IoU in IEEE
 * float32 as ssd._iou_one_to_many evaluates it; rows best first, no cross-class cap.  ssd.detect_ordered is the host statement. */
typedef struct tf2_ssd tf2_ssd;
typedef struct tf2_ssd_desc {
  uint32_t size;                 /* sizeof(tf2_ssd_desc)                                                */
  int32_t num_classes;           /* 2..256, including background class 0                               */
  int32_t top_k;                 /* 1..256                                                             */
  float conf_thresh, nms_thresh; /* >= 0 / > 0 (the reference's test defaults: 0.01 / 0.45)            */
  float variance[2];             /* 0.1, 0.2                                                           */
  int32_t n_sources;             /* 1..8 (SSD300: 6)                                                   */
  int32_t loc_row[8], conf_row[8];
  const float* priors;           /* host, [n_priors][4] centre form (ssd.prior_boxes); copied          */
  int32_t n_priors;
} tf2_ssd_desc;
tf2_status tf2_ssd_create(tf2_net* net, const tf2_ssd_desc* d, tf2_ssd** out);
void       tf2_ssd_destroy(tf2_ssd* s);
/* workspace of tf2_ssd_run: the "outputs kept" plan of `batch` images (the ordinary plan, but every sink row's output lives to the
 * end of the step and the last row is not stored straight into the logits) + the detector's boxes and probabilities */
size_t     tf2_ssd_workspace_size(tf2_ssd* s, int batch);
/* scratch of tf2_ssd_detect: the probabilities transposed to class-major order */
size_t     tf2_ssd_detect_scratch_size(tf2_ssd* s, int batch);
/* One step: the network on the outputs-kept plan, then heads -> boxes + probabilities (dequantise, float32 softmax, decode) and
 * select + NMS, all enqueued on hip_stream (no host synchronisation, no allocation: graph-capturable).
 * det [batch][num_classes][top_k][5] float32 (score, x1, y1, x2, y2; rows past counts[b][c] and class 0 are zero), counts
 * [batch][num_classes] int32.  Optional (NULL): boxes_out [batch][n_priors][4] / scores_out [batch][n_priors][num_classes] float32,
 * the decoded corner-form boxes and class probabilities the selection worked on; logits_out, the network's int8 logits as
 * tf2_net_run writes them; mark_event, a hipEvent_t recorded on hip_stream between the network's launches and the detector's (timing:
 * tools/ssd_detect_time.py).  tf2_net_poll_error works on the workspace afterwards as after tf2_net_run. */
tf2_status tf2_ssd_run(tf2_ssd* s, const void* images_dev, int images_are_q, int batch, void* workspace_dev, size_t workspace_bytes,
                       float* det_dev, int32_t* counts_dev, float* boxes_out, float* scores_out, int8_t* logits_out, void* mark_event,
                       void* hip_stream);
/* The selection alone, on the caller's corner-form boxes [batch][n_priors][4] and class probabilities [batch][n_priors][num_classes]
 * (device, float32); det / counts as above. */
tf2_status tf2_ssd_detect(tf2_ssd* s, const float* boxes_dev, const float* scores_dev, int batch, void* scratch_dev,
                          size_t scratch_bytes, float* det_dev, int32_t* counts_dev, void* hip_stream);

/* ---- Image preprocessing on the device (TransForm_Kit/Quantization/data_loader.py:26-83; INTEGRATION.md "Image preprocessing") ----
 * uint8 pixels (HWC, 3 or 4 bytes a pixel, any row pitch) -> the net's input, float32 [batch][3][image_h][image_w] (what
 * tf2_net_run reads) or, out_q = 1, int8 quantised with 2^-Q0 as runner.cpp:158-164 does (what tf2_net_run_q / images_are_q = 1
 * read; the same bytes prep_input would make of the float output).  Per net channel c, output pixel (y, x) of image b, with
 * Y = y + crop_y, X = x + crop_x:
 *   fy = (Y + 0.5) * (h / resize_h) - 0.5 in double; y0 = floor(fy), wy = (float)(fy - y0); y0 < 0: y0 = 0, wy = 0;
 *   y0 >= h - 1: y0 = h - 1, wy = 0; y1 = min(y0 + 1, h - 1); the same for columns (half-pixel centres, edge clamp, no antialiasing);
 *   in float32, in this order: top = p00*(1-wx) + p01*wx, bot = p10*(1-wx) + p11*wx, r = top*(1-wy) + bot*wy (p: byte
 *   src_channel[c] of the pixel); round_resized: r = clamp(rint(r), 0, 255); v = (r - mean[c]) * scale[c].
 * tf2_amd.preprocess.reference is the host statement; the device output is bit-identical to it.
 * Host checks (TF2_ERR_ARG with a message, before any device call): desc size, pixel_bytes 3 or 4, src_channel in
 * 0..pixel_bytes-1, finite means and scales, round_resized 0 or 1, the net's image_c == 3, batch >= 1, non-null pointers, out_q = 1
 * only once the q table is set (Q0 is read at call time).
 * Device checks: the records are device data (refill them between graph replays), so the kernel validates each one and writes
 * status_dev[b] = 0, or an OR of TF2_PREP_* bits; a malformed image's output is all zeros and none of its pixels is read.  No read
 * leaves [pixels_dev, pixels_dev + pixels_bytes).  The grid depends only on batch and the net's image size: a captured graph
 * stays valid for new images of new sizes.  Enqueued on hip_stream; no allocation, no synchronisation. */
typedef struct tf2_image_src {      /* one per image, in DEVICE memory (refillable between graph replays) */
  int64_t offset;                   /* byte offset of pixel (0,0) in the pixel buffer */
  int32_t h, w, row_pitch;          /* source size, bytes between rows */
  int32_t resize_h, resize_w;       /* size after resize (== h, w: none) */
  int32_t crop_y, crop_x;           /* top-left of the image_h x image_w window in the resized image */
  int32_t reserved;
} tf2_image_src;
typedef struct tf2_preprocess_desc {
  uint32_t size;                    /* sizeof, as tf2_run_opts */
  int32_t pixel_bytes;              /* 3 (RGB/BGR) or 4 (RGBA...) */
  int32_t src_channel[3];           /* net channel c reads source byte src_channel[c] of a pixel */
  int32_t round_resized;
  float mean[3], scale[3];
} tf2_preprocess_desc;
enum {                              /* status_dev bits of a malformed record */
  TF2_PREP_BAD_SIZE = 1,            /* h or w outside 1..32767 */
  TF2_PREP_BAD_PITCH = 2,           /* row_pitch < w * pixel_bytes */
  TF2_PREP_BAD_OFFSET = 4,          /* offset < 0 */
  TF2_PREP_OUT_OF_BUFFER = 8,       /* offset + (h-1) * row_pitch + w * pixel_bytes > pixels_bytes (tested when bits 1, 2, 4 are clear) */
  TF2_PREP_BAD_RESIZE = 16,         /* resize_h or resize_w outside 1..32767 */
  TF2_PREP_BAD_CROP = 32            /* the image_h x image_w window at (crop_y, crop_x) leaves the resized image */
};
tf2_status tf2_preprocess(const tf2_net* net, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                          const tf2_image_src* srcs_dev, int batch, int out_q, void* out_dev, int32_t* status_dev, void* stream);

/* ---- Antialiased resize on the device (INTEGRATION.md "Antialiased resize on the device") ----
 * tf2_preprocess with the resize of Pillow's Image.resize(size, BILINEAR) on an RGB uint8 image (ImagingResample's 8-bit path,
 * default box, reducing_gap None) -- what torchvision's Resize does to a PIL image (data_loader.py:83-90 load_data('resnet50')) --
 * restated bit for bit.  The same arguments, structs and records.  For one axis with n_in source and n_out resized samples, in IEEE
 * double without contraction:
 *   scale = n_in / n_out; fs = max(scale, 1.0); support = fs; ss = 1.0 / fs
 *   resized index X (crop offset added): center = (X + 0.5) * scale
 *     lo = max((int)(center - support + 0.5), 0); hi = min((int)(center + support + 0.5), n_in); n = hi - lo
 *     w[k] = tri((((k + lo) - center) + 0.5) * ss), k = 0..n-1, tri(a) = 1 - |a| if |a| < 1 else 0
 *     ww = w[0] + w[1] + ... in that order; if ww != 0: w[k] = w[k] / ww;  coef[k] = (int)(w[k] * 4194304.0 + 0.5)
 * Horizontal pass first, on source rows: t[y][X][c] = clip((2097152 + sum_k src[y][lo+k][c] * coef[k]) >> 22, 0, 255) in int32, a
 * byte; the vertical pass is the same rule on the bytes t with the row coefficients (the byte in between is part of the result).
 * An axis whose size does not change has coefficients {2^22, 0} and returns its bytes.  Then v = (r - mean[c]) * scale[c] in
 * float32 on the final byte r, written as float32 or quantised as tf2_preprocess does.  Only the image_h x image_w window at
 * (crop_y, crop_x) is computed; it equals the crop of the whole resize.  round_resized is validated (0 or 1) and otherwise ignored:
 * the resize result is bytes already.  tf2_amd.preprocess.reference_aa is the host statement (tests/golden/pil_resize.npz holds
 * Pillow's own bytes); the device output is bit-identical to it.
 * Host checks: those of tf2_preprocess.  Device checks: those of tf2_preprocess, and TF2_PREP_BAD_SCALE when h > 32 * resize_h or
 * w > 32 * resize_w (an integer compare, evaluated when BAD_SIZE and BAD_RESIZE are clear): TF2_PREP_AA_MAX_SCALE bounds a filter at
 * 65 taps an axis and with it the time of one block, and still covers short sides up to 8192 for Resize(256).  Zeros and the status
 * bits for a malformed record, none of whose pixels is read; no read leaves the pixel buffer; no allocation, no synchronisation;
 * enqueued on the caller's stream; the grid depends only on batch and the net's image size. */
#define TF2_PREP_AA_MAX_SCALE 32
enum { TF2_PREP_BAD_SCALE = 64 };   /* h > 32 * resize_h or w > 32 * resize_w (tf2_preprocess_aa only) */
tf2_status tf2_preprocess_aa(const tf2_net* net, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                             const tf2_image_src* srcs_dev, int batch, int out_q, void* out_dev, int32_t* status_dev, void* stream);

/* ---- Second-stage crops on the device (the detect -> crop -> embed -> match cascade of faceverify/README.md; INTEGRATION.md
 * "Second-stage crops on the device") ----
 * The step between a detector's det / counts (tf2_ssd_run) and a second network's input: tf2_roi_select picks boxes into a table
 * of tf2_roi records in device memory, tf2_roi_crop resamples each record's box out of the SOURCE pixels (the uint8 buffer and
 * tf2_image_src records tf2_preprocess read; their resize_* and crop_* fields are not used) into one image of net2's input.  The
 * reference ships no program text for this step, so this statement is the canonical one (tf2_amd.roi.reference_select /
 * reference_crop are the host statement; every device output is bit-identical to them).
 * Select, per source image b: the candidates are the rows (c, r) of det[b] with bit c of class_mask set, r < min(counts[b][c],
 * top_k), score > min_score (strict float32; a NaN never passes) and a valid transformed box; the best max_rois of them by (score
 * descending, class ascending, rank ascending) -- a total order on the float32 values -- go to slots b * max_rois + 0 .. n-1, n to
 * roi_counts_dev[b], and the image's other slots get the empty record (image = -1, every other field 0).  Every slot is written by
 * every call with ordinary stores: no atomics, no dependence on replay order.  The transform, in double from the float32 det
 * values (x1, y1, x2, y2) and the source size (w, h) of srcs_dev[b], every operation rounded separately:
 *   X1 = x1 * w, X2 = x2 * w, Y1 = y1 * h, Y2 = y2 * h;  cx = (X1 + X2) / 2, cy = (Y1 + Y2) / 2;
 *   bw = (X2 - X1) * expand_w, bh = (Y2 - Y1) * expand_h;  square: bw = bh = (bh > bw ? bh : bw);
 *   x0 = cx - bw / 2, x1' = cx + bw / 2, y0 = cy - bh / 2, y1' = cy + bh / 2;
 *   clip: v = v < 0 ? 0 : (v > limit ? limit : v) with limit w for x and h for y (a NaN stays a NaN);  then one rounding to float32.
 * The box is valid iff the four float32 values are finite and x1' - x0 >= 1 and y1' - y0 >= 1, evaluated in double on the float32
 * values.  A source record whose h or w is outside 1..32767 gives its image zero ROIs (nothing else of the record is read).
 * Crop, per slot s with record R, source r = srcs_dev[R.image] and output pixel (y, x) of net2's image_h x image_w (OH x OW) input,
 * in double, every operation rounded separately:
 *   sy = ((double)R.y1 - (double)R.y0) / OH;  t = (y + 0.5) * sy;  t = (double)R.y0 + t;  fy = t - 0.5;  the same for columns;
 * then tf2_preprocess's rule from fy on: y0 = floor(fy), wy = (float)(fy - y0), the clamps at 0 and r.h - 1 with weight 0 (a box may
 * leave the image: it reads the edge pixels), the float32 interpolation, round_resized, (r - mean[c]) * scale[c], and for out_q = 1
 * the int8 quantisation with net2's 2^-Q0.  R = (0, 0, w, h) is tf2_preprocess with resize = (OH, OW) and crop (0, 0), bit for bit.
 * out_dev is float32 or int8 [n_slots][3][OH][OW].
 * Device checks: the table and the source records are device data, so each block validates its slot before it reads a pixel and
 * status_dev[s] receives 0 or TF2_ROI_* bits: EMPTY alone for image == -1; otherwise BAD_IMAGE (image outside 0..batch-1; no source
 * record is read), BAD_BOX (the validity rule above) and, for an image inside the batch, BAD_SRC (srcs_dev[image] fails the size /
 * pitch / offset / extent rule of tf2_preprocess) in any combination.  A slot with a nonzero status is all zeros and none of its
 * pixels is read; no read leaves [pixels_dev, pixels_dev + pixels_bytes).
 * Host checks (TF2_ERR_ARG with a message, before any device call): select -- desc size, num_classes 2..256, top_k 1..256, max_rois
 * 1..64, a class_mask that is empty, has bit 0 (background) set or a bit at or above num_classes, min_score finite and >= 0, expand
 * factors finite and > 0, square and clip 0 or 1, batch >= 1, non-null pointers; crop -- every check of tf2_preprocess (on net2),
 * n_slots >= 1, non-null rois_dev.  Select enqueues one kernel of `batch` blocks, crop one of n_slots * ceil(OH * OW / 1024) blocks
 * of 256 threads: grids that depend on batch, max_rois and net2's image size alone, no allocation, no synchronisation, no scratch
 * (graph-capturable: a captured detect + select + crop + embed + match replays on refilled pixels and records). */
typedef struct tf2_roi {            /* one slot of the ROI table, 32 bytes, in DEVICE memory */
  int32_t image;                    /* index into srcs_dev; -1: empty slot */
  int32_t cls, rank;                /* the det row the box came from */
  float score;
  float x0, y0, x1, y1;             /* the box in source pixels (pixel i covers [i, i + 1)) */
} tf2_roi;
typedef struct tf2_roi_desc {
  uint32_t size;                    /* sizeof(tf2_roi_desc) */
  int32_t num_classes, top_k;       /* layout of det / counts: 2..256, 1..256 */
  uint32_t class_mask[8];           /* bit c: class c is taken; bit 0 (background) clear, at least one bit set below num_classes */
  float min_score;                  /* finite, >= 0 */
  int32_t max_rois;                 /* 1..64 per source image */
  float expand_w, expand_h;         /* finite, > 0; 1 = the box itself */
  int32_t square, clip;             /* 0 / 1 */
} tf2_roi_desc;
enum {                              /* status_dev bits of a slot that was not cropped */
  TF2_ROI_EMPTY = 1,                /* image == -1 */
  TF2_ROI_BAD_IMAGE = 2,            /* image outside 0..batch-1 and not -1 */
  TF2_ROI_BAD_BOX = 4,              /* a coordinate not finite, or a side below 1 */
  TF2_ROI_BAD_SRC = 8               /* srcs_dev[image] fails the size / pitch / offset / extent rule */
};
tf2_status tf2_roi_select(const tf2_roi_desc* d, const float* det_dev, const int32_t* counts_dev, const tf2_image_src* srcs_dev,
                          int batch, tf2_roi* rois_dev, int32_t* roi_counts_dev, void* hip_stream);
tf2_status tf2_roi_crop(const tf2_net* net2, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                        const tf2_image_src* srcs_dev, int batch, const tf2_roi* rois_dev, int n_slots, int out_q, void* out_dev,
                        int32_t* status_dev, void* hip_stream);

/* ---- Antialiased crops on the device (INTEGRATION.md "Antialiased crops on the device") ----
 * tf2_roi_crop with the resize of Pillow's Image.resize((OW, OH), BILINEAR, box=(x0, y0, x1, y1)) on the 8-bit source image
 * (ImagingResample's 8-bit path with a box, reducing_gap None) restated bit for bit: what an enrolment pipeline that crops with
 * Pillow computes.  The same arguments, structs, records and output layout as tf2_roi_crop; round_resized is validated (0 or 1) and
 * otherwise ignored, as in tf2_preprocess_aa.  Slot s with record R and source r = srcs_dev[R.image]; along x with n_in = r.w,
 * n_out = OW, a0 = R.x0, a1 = R.x1 (along y: r.h, OH, R.y0, R.y1), in IEEE double without contraction:
 *   d = (double)(a1 - a0), the subtraction done in float32, rounded to nearest (Pillow's box is float[4])
 *   scale = d / n_out; fs = max(scale, 1.0); support = fs; ss = 1.0 / fs
 *   output index X: center = (double)a0 + (X + 0.5) * scale
 *     lo = max((int)(center - support + 0.5), 0); hi = min((int)(center + support + 0.5), n_in); n = hi - lo
 *     w[k], ww, coef[k]: exactly as tf2_preprocess_aa states them above
 * then tf2_preprocess_aa's two passes (a horizontal pass on source rows to bytes, a vertical pass on those bytes, each
 * clip((2097152 + sum) >> 22, 0, 255) in int32), v = (r - mean[c]) * scale[c] in float32 on the final byte, and for out_q = 1 the int8
 * quantisation with net2's 2^-Q0.  tf2_amd.roi.reference_crop_aa is the host statement (tests/golden/pil_resize_box.npz holds
 * Pillow's own bytes for boxes); the device output is bit-identical to it.  Two consequences:
 *   - R = (0, 0, w, h) is tf2_preprocess_aa with resize = (OH, OW) and crop (0, 0), bit for bit (d = w exactly, 0.0 + t = t).
 *   - The filter is centred on the box but clamped at the IMAGE (0 and n_in), not at the box: it reads source pixels outside the box
 *     and inside the image, up to `support` of them on each side.  The result is Pillow's resize(box=); it is NOT "crop, then
 *     resize", which would clamp the filter at the box's edge.
 * Device checks: tf2_roi_crop's rule unchanged (EMPTY alone for image == -1; BAD_IMAGE, BAD_BOX, BAD_SRC in any combination), and
 * for a slot that rule passes (an image inside the batch with BAD_BOX and BAD_SRC clear) two more bits:
 *   TF2_ROI_BOX_OUTSIDE unless 0 <= x0, x1 <= w, 0 <= y0 and y1 <= h, compared in double on the float32 values (-0.0 passes).  It is
 *     Pillow's own precondition, tf2_roi_select with clip = 1 always meets it, and it keeps every (int) conversion above in range.
 *   TF2_ROI_BAD_SCALE when d > 32 * n_out on either axis (TF2_PREP_AA_MAX_SCALE: at most 65 taps an axis, which bounds one block's LDS
 *     and time).
 * A slot with any bit set is all zeros and none of its pixels is read; no read leaves [pixels_dev, pixels_dev + pixels_bytes).
 * Boxes that leave the image stay with tf2_roi_crop, whose arithmetic and statuses are unchanged.
 * Host checks: those of tf2_roi_crop.  One kernel of n_slots * ceil(OH / 8) * ceil(OW / 32) blocks of 256 threads on the caller's
 * stream: a grid that depends on n_slots and net2's image size alone, no allocation, no synchronisation, no atomics, no scratch
 * (graph-capturable like tf2_roi_crop). */
enum {
  TF2_ROI_BOX_OUTSIDE = 16,         /* the box leaves the image (tf2_roi_crop_aa only) */
  TF2_ROI_BAD_SCALE = 32            /* a side above 32 * the output side (tf2_roi_crop_aa only) */
};
tf2_status tf2_roi_crop_aa(const tf2_net* net2, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                           const tf2_image_src* srcs_dev, int batch, const tf2_roi* rois_dev, int n_slots, int out_q, void* out_dev,
                           int32_t* status_dev, void* hip_stream);

/* ---- Aligned crops on the device (INTEGRATION.md "Aligned crops on the device") ----
 * The same select / crop split for windows that are not upright: tf2_roi_fit turns K landmarks a slot into a table of tf2_roi_xform
 * records in device memory, tf2_roi_warp resamples each record's affine window out of the SOURCE pixels into one image of net2's
 * input.  The face network of the cascade is calibrated and evaluated on aligned faces (a similarity warp that puts eyes, nose and
 * mouth corners on a fixed template); callers may also fill the table themselves (rotated boxes, a transform of their own).
 * tf2_amd.align.reference_fit / reference_warp are the host statement; every device output is bit-identical to them.
 * The record: m maps output pixel centres to source coordinates in Pillow's Image.AFFINE convention (pixel i covers [i, i + 1), as
 * in tf2_roi); image == -1 is the empty slot.  56 bytes; the table must be 8-byte aligned.
 * Fit, per slot s with R = rois_dev[s] and the float32 landmarks lmk_dev[s][i] = (u_i, v_i), i = 0 .. K-1 (K = n_points): space 0
 * takes them as source pixels, sx_i = u_i, sy_i = v_i; space 1 as relative to the slot's box, sx_i = x0 + u_i * (x1 - x0),
 * sy_i = y0 + v_i * (y1 - y0).  The template (tx_i, ty_i) = tpl[i] is in output pixels of net2's input.  The fit is the
 * least-squares similarity without reflection, landmarks -> template, inverted into the output -> source map; it is stated with
 * + - * / alone in IEEE double from the float32 values, every operation rounded separately (no contraction), sums taken in index
 * order from 0.0:
 *   mx = (sum sx_i) / K, my = (sum sy_i) / K, ux = (sum tx_i) / K, uy = (sum ty_i) / K
 *   px = sx_i - mx, py = sy_i - my, qx = tx_i - ux, qy = ty_i - uy
 *   var += px*px + py*py;   c += px*qx + py*qy;   s += px*qy - py*qx        (i = 0 .. K-1)
 *   A = c / var;  B = s / var;  n = A*A + B*B;  a = A / n;  b = -B / n
 *   m = { a, -b, (mx - a*ux) + b*uy,   b, a, (my - b*ux) - a*uy }
 * status_dev[s] receives 0 or TF2_ROI_* bits: EMPTY alone for R.image == -1; otherwise BAD_BOX when space == 1 and the box fails the
 * validity rule of tf2_roi_crop, and TF2_ROI_BAD_LANDMARKS when one of the 2 * K float32 coordinates is not finite; with both clear
 * the fit runs and BAD_LANDMARKS is set when var > 0 fails, when n > 0 fails or when any of the six results is not finite.  (The
 * image index is not judged here: tf2_roi_warp does.)  A slot with status 0 gets { R.image, 0, m }; any other gets the empty record:
 * image -1, reserved 0, every m equal to +0.0.  Every slot is written by every call with plain stores.
 * Host checks of fit (TF2_ERR_ARG with a message, before any device call): desc size, n_points in 2..16, space 0 or 1, the
 * 2 * n_points template values finite, a template variance sum(qx*qx + qy*qy) > 0 (double, as above), n_slots >= 1, non-null
 * pointers, xf_dev 8-byte aligned.  One kernel of ceil(n_slots / 64) blocks of 64 threads, a thread a slot.
 * Warp, per slot s with record T = xf_dev[s], m = T.m, source r = srcs_dev[T.image] and output pixel (y, x) of net2's OH x OW input:
 * Pillow's Image.transform((OW, OH), Image.AFFINE, m, resample=BILINEAR) on the 8-bit source (ImagingGenericTransform with
 * affine_transform and the 8-bit bilinear filter) restated bit for bit, in double, every operation rounded separately:
 *   xin = x + 0.5; yin = y + 0.5
 *   fx = (m0*xin + m1*yin) + m2;   fy = (m3*xin + m4*yin) + m5
 *   inside iff fx >= 0 && fx < r.w && fy >= 0 && fy < r.h     (a NaN is outside; no integer conversion happens before this test)
 *   outside: the byte is 0 in every channel (Pillow's fill)
 *   inside:  fx -= 0.5; fy -= 0.5; X = floor(fx); dx = fx - X; Y = floor(fy); dy = fy - Y          (X, Y >= -1)
 *            xa = clamp(X, 0, w-1); xb = clamp(X+1, 0, w-1); ya = clamp(Y, 0, h-1)
 *            v1 = p[ya][xa] + (p[ya][xb] - p[ya][xa]) * dx                                         (the difference in integers)
 *            v2 = (Y + 1 < h) ? p[Y+1][xa] + (p[Y+1][xb] - p[Y+1][xa]) * dx : v1
 *            byte = (uint8)(v1 + (v2 - v1) * dy)                                                   (truncation)
 * then v = ((float)byte - mean[c]) * scale[c] in float32 -- a fill byte 0 goes through the same line -- and for out_q = 1 the int8
 * quantisation with net2's 2^-Q0, as tf2_roi_crop.  There is no antialiasing (Pillow's transform has none; tf2_roi_crop_aa stays the
 * answer for upright boxes) and no scale limit: the cost per output pixel is constant.  The arguments, the desc, the source records
 * and the output layout are tf2_roi_crop's with xf_dev in place of rois_dev; round_resized is validated and otherwise ignored.
 * Device checks of warp, per slot, before a pixel is read: EMPTY alone for image == -1; otherwise BAD_IMAGE (outside 0..batch-1; no
 * source record is read), BAD_SRC (tf2_roi_crop's rule) and TF2_ROI_BAD_MATRIX unless all six m are finite, in any combination.  A
 * slot with any bit set is all zeros and none of its pixels is read; no read leaves [pixels_dev, pixels_dev + pixels_bytes).
 * Host checks of warp: those of tf2_roi_crop, and xf_dev 8-byte aligned.  One kernel of n_slots * ceil(OH * OW / 1024) blocks of 256
 * threads on the caller's stream: a grid that depends on n_slots and net2's image size alone, no allocation, no synchronisation, no
 * atomics, no scratch (graph-capturable: detect + select + fit + warp + embed + match replays on refilled buffers). */
#define TF2_ROI_FIT_MAX_POINTS 16
typedef struct tf2_roi_xform {      /* one slot of the transform table, 56 bytes, 8-byte aligned, in DEVICE memory */
  int32_t image;                    /* index into srcs_dev; -1: empty slot */
  int32_t reserved;                 /* 0 */
  double m[6];                      /* source x = m0*(x+.5) + m1*(y+.5) + m2, source y = m3*(x+.5) + m4*(y+.5) + m5 */
} tf2_roi_xform;
typedef struct tf2_roi_fit_desc {
  uint32_t size;                    /* sizeof(tf2_roi_fit_desc) */
  int32_t n_points;                 /* K, 2..16 */
  float tpl[TF2_ROI_FIT_MAX_POINTS][2];   /* (x, y) of the first K points in output pixels of net2's input; finite, not all equal */
  int32_t space;                    /* 0: landmarks in source pixels; 1: relative to the slot's box */
} tf2_roi_fit_desc;
enum {
  TF2_ROI_BAD_LANDMARKS = 64,       /* a landmark not finite, or a degenerate fit (tf2_roi_fit only) */
  TF2_ROI_BAD_MATRIX = 128          /* an entry of m not finite (tf2_roi_warp only) */
};
tf2_status tf2_roi_fit(const tf2_roi_fit_desc* d, const tf2_roi* rois_dev, const float* lmk_dev, int n_slots, tf2_roi_xform* xf_dev,
                       int32_t* status_dev, void* hip_stream);
tf2_status tf2_roi_warp(const tf2_net* net2, const tf2_preprocess_desc* d, const uint8_t* pixels_dev, size_t pixels_bytes,
                        const tf2_image_src* srcs_dev, int batch, const tf2_roi_xform* xf_dev, int n_slots, int out_q, void* out_dev,
                        int32_t* status_dev, void* hip_stream);

/* ---- YCbCr frames on the device (INTEGRATION.md "YCbCr frames on the device") ----
 * The step in front of the three gather calls above: a batch of planar or semi-planar 8-bit YCbCr frames (what a JPEG or a video
 * decoder leaves) -> the interleaved pixels those calls read, written where their tf2_image_src records point.  Needs no net handle.
 * Image b has the size h x w, the offset and the row_pitch of srcs_dev[b] (its resize_* and crop_* fields are not read); its planes
 * are described by ycc_dev[b]; chroma planes are ch = ceil(h / sub_y) rows of cw = ceil(w / sub_x) samples.  All arithmetic is
 * integer and >> is arithmetic; tf2_amd.ycc.reference is the host statement and the device is bit-identical to it.  With JFIF and
 * FANCY the result is byte for byte what libjpeg-turbo's decoder (and with it Pillow's) makes of the same planes: "fancy" upsampling
 * and the jdcolor tables (tests/golden/pil_ycc.npz holds Pillow's own bytes).
 * Upsampled chroma at output pixel (y, x), for a chroma plane P (Cb and Cr alike):
 *   REPLICATE                 P[y / sub_y][x / sub_x]
 *   FANCY, (1,1)              P[y][x]
 *   FANCY, (2,1)              p = P[y], k = x >> 1;  x even: k == 0 ? p[0] : (3*p[k] + p[k-1] + 1) >> 2
 *                                                    x odd:  k == cw-1 ? p[k] : (3*p[k] + p[k+1] + 2) >> 2
 *   FANCY, (2,2)              r = y >> 1, k = x >> 1, o = (y even) ? max(r-1, 0) : min(r+1, ch-1), s[j] = 3*P[r][j] + P[o][j];
 *                             x even: k == 0 ? (4*s[0] + 8) >> 4 : (3*s[k] + s[k-1] + 8) >> 4
 *                             x odd:  k == cw-1 ? (4*s[k] + 7) >> 4 : (3*s[k] + s[k+1] + 7) >> 4
 * Colour, with FIX(v) = (int)(v * 65536 + 0.5), cb = Cb - 128, cr = Cr - 128 and every result clamped to 0..255:
 *   JFIF (full range)         R = Y + ((FIX(1.40200)*cr + 32768) >> 16)
 *                             G = Y + ((-FIX(0.34414)*cb + 32768 - FIX(0.71414)*cr) >> 16)
 *                             B = Y + ((FIX(1.77200)*cb + 32768) >> 16)
 *   BT601, BT709 (limited)    yy = Y - 16, one sum a channel: (FIX(ky)*yy +- FIX(|a|)*cb +- FIX(|b|)*cr + 32768) >> 16
 *     BT601: ky 1.164383; R +1.596027 cr; G -0.391762 cb -0.812968 cr; B +2.017232 cb
 *     BT709: ky 1.164384; R +1.792741 cr; G -0.213249 cb -0.532909 cr; B +2.112402 cb
 *     (every sum fits in 27 bits; the result is at most 1 from floor(the double formula + 0.5), clamped)
 * R, G and B go to bytes dst_channel[0..2] of the output pixel, alpha to the remaining byte when pixel_bytes == 4.  Bytes of a
 * destination row beyond w * pixel_bytes are not touched.
 * Host checks (TF2_ERR_ARG with a message, before any device call): desc size, each enum in range, (sub_x, sub_y) one of (1,1),
 * (2,1), (2,2) unless GRAY, pixel_bytes 3 or 4, dst_channel distinct and in 0..pixel_bytes-1, alpha 0..255, blocks_per_image >= 0,
 * batch >= 1, non-null pointers, [src_dev, src_dev + src_bytes) and [pixels_dev, pixels_dev + pixels_bytes) disjoint.
 * Device checks: both record tables are device data (refill them between graph replays), so every block validates its image's
 * records before it touches a byte and status_dev[b] receives 0 or an OR of TF2_YCC_* bits.  cw in the pitch test is
 * (w + sub_x - 1) >> (sub_x - 1) whatever w holds.  The extent bits are tested in 64 bits and only when the first three are clear.
 * An image with a nonzero status is neither read nor written; no access leaves either buffer.  GRAY reads neither chroma offset
 * nor pitch_c.
 * One kernel of batch * blocks_per_image blocks of 256 threads (0: the library's default, a function of batch alone), each walking
 * its image's TF2_YCC_TILE_H x TF2_YCC_TILE_W tiles with a stride: the grid does not depend on the records, so a captured graph
 * stays valid for new frames of new sizes.  No allocation, no synchronisation, no scratch, no atomics; enqueued on hip_stream. */
#define TF2_YCC_TILE_W 128
#define TF2_YCC_TILE_H 16
typedef struct tf2_ycc_src {        /* one per image, in DEVICE memory, refillable between graph replays; 32 bytes */
  int64_t off_y, off_cb, off_cr;    /* byte offsets of sample (0,0) of each plane in the source buffer */
  int32_t pitch_y, pitch_c;         /* bytes between rows of the Y plane / of a chroma plane (of the interleaved one when semi-planar) */
} tf2_ycc_src;
enum { TF2_YCC_PLANAR = 0, TF2_YCC_SEMI_CBCR = 1, TF2_YCC_SEMI_CRCB = 2, TF2_YCC_GRAY = 3 };    /* layout */
enum { TF2_YCC_FANCY = 0, TF2_YCC_REPLICATE = 1 };                                              /* upsample */
enum { TF2_YCC_JFIF = 0, TF2_YCC_BT601 = 1, TF2_YCC_BT709 = 2 };                                /* matrix */
typedef struct tf2_ycc_desc {
  uint32_t size;                    /* sizeof(tf2_ycc_desc) */
  int32_t layout;                   /* PLANAR (3 planes), SEMI_CBCR (NV12: off_cb -> CbCr pairs, off_cr not read), SEMI_CRCB (NV21:
                                       off_cb -> CrCb pairs), GRAY (chroma not read, Cb = Cr = 128) */
  int32_t sub_x, sub_y;             /* (1,1), (2,1) or (2,2); GRAY: ignored */
  int32_t upsample;                 /* FANCY (libjpeg's triangle filter) or REPLICATE */
  int32_t matrix;                   /* JFIF (full range, libjpeg's tables), BT601, BT709 (limited range) */
  int32_t pixel_bytes;              /* 3 or 4 */
  int32_t dst_channel[3];           /* the byte of an output pixel that receives R, G, B: distinct, in 0..pixel_bytes-1 */
  int32_t alpha;                    /* 0..255, written to the fourth byte when pixel_bytes == 4 */
  int32_t blocks_per_image;         /* >= 1; 0: the library's default */
} tf2_ycc_desc;
enum {                              /* status_dev bits of an image that was not converted */
  TF2_YCC_BAD_SIZE = 1,             /* h or w outside 1..32767 */
  TF2_YCC_BAD_PITCH = 2,            /* row_pitch < w * pixel_bytes, pitch_y < w, pitch_c < cw (2 * cw when semi-planar) */
  TF2_YCC_BAD_OFFSET = 4,           /* a negative offset that is read (the destination's, off_y, off_cb, PLANAR: off_cr) */
  TF2_YCC_OUT_OF_SRC = 8,           /* a plane's extent leaves [0, src_bytes) */
  TF2_YCC_OUT_OF_DST = 16           /* offset + (h-1) * row_pitch + w * pixel_bytes > pixels_bytes */
};
tf2_status tf2_ycc_to_rgb(const tf2_ycc_desc* d, const uint8_t* src_dev, size_t src_bytes, const tf2_ycc_src* ycc_dev,
                          uint8_t* pixels_dev, size_t pixels_bytes, const tf2_image_src* srcs_dev, int batch,
                          int32_t* status_dev, void* hip_stream);

/* ---- JPEG files on the device (INTEGRATION.md "JPEG files on the device") ----
 * The step in front of tf2_ycc_to_rgb: a baseline JPEG file -> the planes libjpeg's decoder (and with it Pillow's) reconstructs,
 * byte for byte, written where the tf2_ycc_src records of tf2_ycc_to_rgb point.  The serial part runs on the host (tf2_jpeg_parse,
 * tf2_jpeg_entropy: headers and Huffman decoding, csrc/jpeg_entropy.cpp), dequantisation and the inverse DCT on the device
 * (tf2_jpeg_idct, csrc/jpeg_idct.hip).  tests/golden/pil_jpeg.npz holds Pillow's own bytes; tf2_amd.jpeg.reference is the host
 * statement of the device call and the device is bit-identical to it.
 * The arithmetic (libjpeg's "islow" integer inverse DCT, jidctint.c).  A block is 64 int16 coefficients c[v][u], v the vertical and
 * u the horizontal frequency, in natural (row-major) order, with a quantiser q[v][u] (uint16, natural order).  All sums, products and
 * left shifts wrap modulo 2^32 (computed unsigned); every >> is arithmetic on the wrapped value.  d[v][u] = c[v][u] * q[v][u].  The
 * 1-D kernel K(x0..x7; s):
 *   z1 = (x2+x6)*4433;  t2 = z1 - x6*15137;  t3 = z1 + x2*6270
 *   t0 = (x0+x4) << 13;  t1 = (x0-x4) << 13
 *   a0 = t0+t3;  a3 = t0-t3;  a1 = t1+t2;  a2 = t1-t2
 *   b0 = x7;  b1 = x5;  b2 = x3;  b3 = x1
 *   z1 = b0+b3;  z2 = b1+b2;  z3 = b0+b2;  z4 = b1+b3;  z5 = (z3+z4)*9633
 *   b0 *= 2446;  b1 *= 16819;  b2 *= 25172;  b3 *= 12299
 *   z1 *= -7373;  z2 *= -20995;  z3 = z3*(-16069) + z5;  z4 = z4*(-3196) + z5
 *   b0 += z1+z3;  b1 += z2+z4;  b2 += z2+z3;  b3 += z1+z4
 *   out = [a0+b3, a1+b2, a2+b1, a3+b0, a3-b0, a2-b1, a1-b2, a0-b3], each (o + (1 << (s-1))) >> s
 * Pass 1 runs down each column u: x_k = d[k][u], s = 11, giving ws[k][u].  Pass 2 runs along each row k: x_j = ws[k][j], s = 18.
 * The sample is clamp(out + 128, 0, 255).  (libjpeg's shortcuts for zero columns and rows give the same values.  For the streams a
 * conformant encoder writes nothing wraps; the wrap rule makes hostile input defined.)
 *
 * tf2_jpeg_parse reads the headers of `file` into *info: the size, the component count (1 or 3), (sub_x, sub_y), the restart
 * interval, per component the block grid bw x bh of the scan (padded to whole MCUs for three components, ceil(w/8) x ceil(h/8) for
 * one), the plane size ph x pw (Y: h x w; chroma: ceil(h / sub_y) x ceil(w / sub_x)) and the quantiser in natural order (from 8- or
 * 16-bit DQT entries), the total block count, and `upsample`, the rule libjpeg applies to this file's chroma: TF2_YCC_REPLICATE when
 * the file is subsampled and the chroma plane is at most 2 samples wide (jdsample.c filters only wider planes), TF2_YCC_FANCY
 * otherwise.  Accepted: SOF0, and SOF1 with 8-bit samples; Huffman coding; one scan holding all components; luma sampling 1x1, 2x1
 * or 2x2 with chroma 1x1, or a single component; DRI / RSTn; any APPn / COM.  Everything else sets TF2_JPEG_UNSUPPORTED_* bits in
 * info->status (and nothing is decoded, so a caller can fall back): progressive and the other non-sequential Huffman processes,
 * arithmetic coding, 12-bit samples, a component count other than 1 or 3, other sampling factors, a scan that does not hold every
 * component, and RGB data by libjpeg's rule (no JFIF marker and an Adobe marker with transform 0, or neither marker and the
 * component ids 'R', 'G', 'B').  A malformed header sets TF2_JPEG_BAD_HEADER.  The return value is TF2_ERR_ARG for null arguments
 * and TF2_OK otherwise: what the file is like is in info->status.
 * tf2_jpeg_entropy decodes the scan of a file whose info->status is 0 into dense blocks of 64 int16 in natural order: component
 * after component, each in raster order over its bw x bh grid (component c starts at block sum of bw * bh of the components before
 * it), with DC prediction, EOB and ZRL runs, byte stuffing and restart markers (predictors reset).  Values are stored as int16
 * with wrap.  Whatever the bytes hold it reads nothing outside [file, file + bytes) and writes nothing outside coef[0 ..
 * info->total_blocks * 64), which it zeroes first; capacity_blocks < info->total_blocks is TF2_ERR_SIZE and nothing is written.
 * *status receives 0, TF2_JPEG_TRUNCATED (the stream ends, or a marker stands, where bits or a restart marker are needed) or
 * TF2_JPEG_BAD_CODE (a code no table holds, a coefficient index beyond 63, a DC category above 15, a wrong restart marker), or
 * the parser's bits if the headers do not parse to what `info` says; blocks not reached stay zero.  Both calls are host only, touch
 * no global state and may run on many threads at once; neither sets tf2_last_error.
 *
 * tf2_jpeg_idct, image b: its coefficients are described by jpeg_dev[b] (block offsets into coef_dev, in blocks of 64 int16, and
 * the grids), its quantisers are quant_dev[b][c][64], its sizes h x w come from srcs_dev[b] (nothing else of that record is read)
 * and its planes go where ycc_dev[b] points in planes_dev: exactly ph x pw samples of each plane and no other byte (the rest of
 * an edge block is computed and dropped; blocks wholly outside the plane are not read).  d->layout is TF2_YCC_PLANAR (three
 * components, (sub_x, sub_y) one of (1,1), (2,1), (2,2)) or TF2_YCC_GRAY (one component: component 0 alone is read and off_y,
 * pitch_y alone of the ycc record).  A batch shares one desc: group files by layout and subsampling.
 * Host checks (TF2_ERR_ARG with a message, before any device call): desc size, layout PLANAR or GRAY, (sub_x, sub_y) unless GRAY,
 * blocks_per_image >= 0, batch >= 1, non-null pointers, coef_blocks * 128 representable, the coefficient and the plane buffer
 * disjoint.
 * Device checks: all four tables are device data (refill them between graph replays), so every block validates its image's
 * records before it touches a byte and status_dev[b] receives 0 or an OR of TF2_JPEG_REC_* bits; the extent bits are tested in 64
 * bits and only when the others are clear.  An image with a nonzero status is neither read nor written.
 * One kernel of batch * blocks_per_image blocks of 256 threads (0: the library's default, a function of batch alone), each walking
 * its image's tiles of TF2_JPEG_TILE_BH x TF2_JPEG_TILE_BW coefficient blocks (a tile lies in one plane) with a stride: the grid
 * does not depend on the records, so a captured graph stays valid for new files of new sizes.  No allocation, no synchronisation,
 * no scratch, no atomics; enqueued on hip_stream. */
#define TF2_JPEG_TILE_BW 8
#define TF2_JPEG_TILE_BH 4
enum {                              /* tf2_jpeg_info.status and tf2_jpeg_entropy's *status */
  TF2_JPEG_UNSUPPORTED_PROGRESSIVE = 1,   /* SOF2, and the lossless / hierarchical Huffman processes SOF3, 5, 6, 7 */
  TF2_JPEG_UNSUPPORTED_ARITHMETIC = 2,    /* SOF9 .. SOF15, or a DAC segment */
  TF2_JPEG_UNSUPPORTED_PRECISION = 4,     /* samples that are not 8 bits */
  TF2_JPEG_UNSUPPORTED_COMPONENTS = 8,    /* a component count other than 1 or 3 */
  TF2_JPEG_UNSUPPORTED_SAMPLING = 16,     /* luma not 1x1, 2x1 or 2x2, or chroma not 1x1 */
  TF2_JPEG_UNSUPPORTED_SCANS = 32,        /* a scan that does not hold every component */
  TF2_JPEG_UNSUPPORTED_COLORSPACE = 64,   /* three components that libjpeg takes as RGB */
  TF2_JPEG_BAD_HEADER = 128,              /* no SOI, a segment that leaves the file, a table or a field out of range, no SOF / SOS */
  TF2_JPEG_TRUNCATED = 256,               /* entropy decoder: the data ends before the last block */
  TF2_JPEG_BAD_CODE = 512                 /* entropy decoder: an invalid code, run or restart marker */
};
typedef struct tf2_jpeg_info {      /* 480 bytes */
  int32_t status;                   /* 0, or TF2_JPEG_* bits: the other fields are then not meaningful */
  int32_t h, w, components;         /* 1..65535; 1 or 3 */
  int32_t sub_x, sub_y;             /* (1,1), (2,1), (2,2); one component: (1,1) */
  int32_t restart_interval;         /* MCUs between restart markers, 0: none */
  int32_t upsample;                 /* TF2_YCC_FANCY or TF2_YCC_REPLICATE: what libjpeg does to this file's chroma */
  int32_t bw[3], bh[3];             /* the block grid of each component in the scan */
  int32_t ph[3], pw[3];             /* the plane of each component, in samples */
  int64_t total_blocks;             /* sum of bw * bh */
  int64_t scan_offset;              /* byte offset of the entropy-coded data in the file */
  uint16_t quant[3][64];            /* natural order */
} tf2_jpeg_info;
typedef struct tf2_jpeg_src {       /* one per image, in DEVICE memory, refillable between graph replays; 48 bytes */
  int64_t block_off[3];             /* first block of each component in coef_dev, in blocks of 64 int16 */
  int32_t bw[3], bh[3];             /* the block grid of each component: block (by, bx) is block_off + by * bw + bx */
} tf2_jpeg_src;
typedef struct tf2_jpeg_desc {
  uint32_t size;                    /* sizeof(tf2_jpeg_desc) */
  int32_t layout;                   /* TF2_YCC_PLANAR or TF2_YCC_GRAY */
  int32_t sub_x, sub_y;             /* (1,1), (2,1) or (2,2); GRAY: ignored */
  int32_t blocks_per_image;         /* >= 1; 0: the library's default */
} tf2_jpeg_desc;
enum {                              /* status_dev bits of an image that was not reconstructed */
  TF2_JPEG_REC_BAD_SIZE = 1,        /* h or w outside 1..32767 */
  TF2_JPEG_REC_BAD_GRID = 2,        /* a bw or bh below 1, or 8 * bw < pw, or 8 * bh < ph */
  TF2_JPEG_REC_BAD_PITCH = 4,       /* pitch_y < w, or pitch_c < cw */
  TF2_JPEG_REC_BAD_OFFSET = 8,      /* a negative offset that is used (block_off[c], off_y, PLANAR: off_cb, off_cr) */
  TF2_JPEG_REC_OUT_OF_COEF = 16,    /* block_off[c] + bw * bh > coef_blocks */
  TF2_JPEG_REC_OUT_OF_PLANES = 32   /* a plane's extent leaves [0, planes_bytes) */
};
tf2_status tf2_jpeg_parse(const uint8_t* file, size_t bytes, tf2_jpeg_info* info);
tf2_status tf2_jpeg_entropy(const uint8_t* file, size_t bytes, const tf2_jpeg_info* info, int16_t* coef, size_t capacity_blocks,
                            int32_t* status);
tf2_status tf2_jpeg_idct(const tf2_jpeg_desc* d, const int16_t* coef_dev, size_t coef_blocks, const tf2_jpeg_src* jpeg_dev,
                         const uint16_t* quant_dev, uint8_t* planes_dev, size_t planes_bytes, const tf2_ycc_src* ycc_dev,
                         const tf2_image_src* srcs_dev, int batch, int32_t* status_dev, void* hip_stream);

/* ---- JPEG entropy decoding on the device (INTEGRATION.md "JPEG entropy decoding on the device") ----
 * The step in front of tf2_jpeg_idct, as an alternative to tf2_jpeg_entropy: the entropy-coded bytes of a batch of files ->
 * the dense blocks of 64 int16 coefficients tf2_jpeg_idct reads (tf2_jpeg_huff, csrc/jpeg_huff.hip).  The host only parses the
 * headers (tf2_jpeg_parse) and copies the Huffman tables into a record (tf2_jpeg_scan_fill).  tf2_amd.jpeg.reference_huff is the
 * host statement of the device call -- the same parallel algorithm, not a serial decoder -- and the device is bit-identical to it.
 *
 * Records.  Image b's entropy-coded data is bytes_dev[scan_dev[b].byte_off .. + byte_len): from info.scan_offset to the end of
 * the file, trailing bytes included.  scan_dev[b] also holds the component count, (sub_x, sub_y), the restart interval and per
 * component the raw canonical tables of its DC and AC code (counts of the codes of length 1..16, symbols in code order); the device
 * builds its lookup tables in LDS.  The block grids and where the blocks go come from jpeg_dev[b], the tf2_jpeg_src record that
 * tf2_jpeg_idct reads.  tf2_jpeg_scan_fill fills a record from a file and the info tf2_jpeg_parse made of it (host only, no state,
 * thread safe, sets no tf2_last_error; TF2_ERR_ARG for null arguments, an info whose status is not 0, or headers that no longer
 * parse to what info says).
 *
 * The algorithm (self-synchronising Huffman decoding: Klein and Wiseman; Weissenberger and Schmidt for JPEG).  The data is cut into
 * N = max(1, ceil(byte_len / subseq_bytes)) subsequences, one lane each.  A decoder state is the bit reader's position (with, for
 * files with a restart interval, the count of whole bytes the host's 64-bit accumulator holds ahead of it, which tf2_jpeg_entropy's
 * restart rule depends on), the block's index inside the MCU, and the zigzag index k (0: a DC code is due).  A step is one code
 * with its extra bits; it belongs to the subsequence its first bit lies in, and a lane decodes steps from its entry state until the
 * position leaves its subsequence (the last lane: until the data ends) and records the exit state, the blocks it completed and the
 * sum of the DC differences per component, both since the last restart marker it passed, and the markers passed.
 *   Round 0: every lane starts at its first bit (behind the 00 of a stuffed pair that straddles the boundary) with block 0, k 0.
 *   Round r: a lane whose entry (its left neighbour's exit of round r - 1) changed decodes again; others keep their exit.
 *   When no entry changes the chain of states is the serial decoder's.  After round r the first r + 1 lanes are certainly right,
 *   so N rounds is the worst case -- a serial decode.  Lanes are processed in chunks of min(TF2_JPEG_HUFF_LANES, 65536 /
 *   subseq_bytes, 16 * subseq_bytes) -- 256, 512, 1024, 512, 256 for 16 .. 256 bytes; a chunk's converged exit is the next chunk's
 *   first entry.
 * The rounds decode TOLERANTLY, or wrongly started lanes never meet the right chain: a code no table holds skips one bit, a DC
 * category above 15 is 15, a zigzag index beyond 63 ends the block, and where the valid bits end (a marker, FF followed by anything
 * but 00, or the end of the data) in front of an RSTn the lane steps over the marker to (block 0, k 0) with an empty reader; any
 * other marker or the end is a terminal "stopped" state.  Every step consumes at least one bit, a marker, or stops.
 * Errors are judged afterwards, in a STRICT pass over the converged chain with tf2_jpeg_entropy's own rules: a prefix sum over the
 * lanes' counts gives every lane the scan-order index of its first block, the restart markers passed and the DC predictors, and
 * the lane decodes once more, writing DC values and nonzero AC coefficients in natural order at the host decoder's block index
 * (the extent was zeroed first).  Bits that run out are TF2_JPEG_TRUNCATED; a code no table holds (with 16 bits to look at), a DC
 * category above 15, an index beyond 63, and a restart marker that does not stand at the host reader's fill pointer with the right
 * number where an interval ends are TF2_JPEG_BAD_CODE.  Decoding stops at the image's total block count; trailing bytes are
 * ignored.  The first error in chain order is the status.
 *
 * Contract.  For a file tf2_jpeg_entropy decodes with status 0 the image's coefficient extent equals the host decoder's buffer bit
 * for bit and status_dev[b] is 0, for every subseq_bytes.  For a file it decodes with TF2_JPEG_TRUNCATED or TF2_JPEG_BAD_CODE,
 * status_dev[b] is one of those two (which of them may differ from the host's, whose bit reader looks further ahead) and -- a
 * stated difference from the host, which leaves the blocks before the error -- the image's whole extent is zero.
 * Device checks: every workgroup validates its image's records before it touches a byte; an image with a TF2_JPEG_REC_* bit is
 * neither read nor written (status_dev[b] alone), other images are unaffected.  Nothing is read outside the image's byte range
 * and nothing written outside its coefficient extent, its slice of the workspace and status_dev[b], whatever the bytes hold.
 * Termination: rounds are at most the lanes of a chunk, chunks ceil(N / lanes of a chunk), a lane's steps at most 9 * byte_len
 * + 64; no workgroup waits for another, nothing is polled.
 * Workspace: image b's slice is work_dev[b * (work_bytes / batch rounded down to 8) ...]: int32 {rounds used, N, 0, 0}
 * then 8 bytes per subsequence (its converged exit state).  tf2_jpeg_huff_work_bytes(d, batch, max_scan_bytes) is the size that
 * takes byte_len up to max_scan_bytes.
 * Host checks (TF2_ERR_ARG with a "tf2_jpeg_huff:" message, before any device call): desc size, layout PLANAR or GRAY, (sub_x,
 * sub_y) unless GRAY, subseq_bytes 0, 16, 32, 64, 128 or 256, batch >= 1, non-null pointers, coef_dev 16-byte and work_dev 8-byte
 * aligned, coef_blocks * 128 representable, work_bytes >= tf2_jpeg_huff_work_bytes(d, batch, 0), and the byte, coefficient,
 * workspace and status buffers pairwise disjoint.
 * One kernel of `batch` workgroups of TF2_JPEG_HUFF_LANES threads, whatever the records hold: a captured graph stays valid for new
 * files of new sizes.  No allocation, no synchronisation, no host copy, no scratch; enqueued on hip_stream. */
#define TF2_JPEG_HUFF_LANES 1024
#define TF2_JPEG_HUFF_DEFAULT_SUBSEQ 64
#define TF2_JPEG_HUFF_MAX_BYTES (1 << 28)
typedef struct tf2_jpeg_scan {      /* one per image, in DEVICE memory, refillable between graph replays; 1664 bytes */
  int64_t byte_off, byte_len;       /* the entropy-coded data in bytes_dev; byte_len <= TF2_JPEG_HUFF_MAX_BYTES */
  int32_t components;               /* 1 or 3: must agree with the desc */
  int32_t sub_x, sub_y;             /* must agree with the desc (one component: 1, 1) */
  int32_t restart_interval;         /* 0..65535 */
  struct {
    uint8_t dc_counts[16], dc_vals[256];   /* codes of length 1..16; the symbols in code order */
    uint8_t ac_counts[16], ac_vals[256];
  } tab[3];                         /* per component */
} tf2_jpeg_scan;
typedef struct tf2_jpeg_huff_desc {
  uint32_t size;                    /* sizeof(tf2_jpeg_huff_desc) */
  int32_t layout;                   /* TF2_YCC_PLANAR or TF2_YCC_GRAY */
  int32_t sub_x, sub_y;             /* (1,1), (2,1) or (2,2); GRAY: ignored */
  int32_t subseq_bytes;             /* 16, 32, 64, 128 or 256; 0: TF2_JPEG_HUFF_DEFAULT_SUBSEQ */
} tf2_jpeg_huff_desc;
enum {                              /* further status_dev bits of tf2_jpeg_huff (with REC_BAD_GRID, REC_BAD_OFFSET, REC_OUT_OF_COEF) */
  TF2_JPEG_REC_BAD_RANGE = 1024,    /* byte_off or byte_len negative, byte_len too large, or the range leaves [0, bytes_len) */
  TF2_JPEG_REC_BAD_SCAN = 2048,     /* components, sub_x, sub_y disagree with the desc, or restart_interval outside 0..65535 */
  TF2_JPEG_REC_BAD_TABLE = 4096,    /* counts that are no canonical code: more than 256 symbols or a code that does not fit its length */
  TF2_JPEG_REC_WORK_TOO_SMALL = 8192 /* the image's workspace slice is smaller than 16 + 8 * N */
};
tf2_status tf2_jpeg_scan_fill(const uint8_t* file, size_t bytes, const tf2_jpeg_info* info, int64_t byte_off, tf2_jpeg_scan* out);
size_t tf2_jpeg_huff_work_bytes(const tf2_jpeg_huff_desc* d, int batch, size_t max_scan_bytes);
tf2_status tf2_jpeg_huff(const tf2_jpeg_huff_desc* d, const uint8_t* bytes_dev, size_t bytes_len, const tf2_jpeg_scan* scan_dev,
                         const tf2_jpeg_src* jpeg_dev, int16_t* coef_dev, size_t coef_blocks, uint8_t* work_dev, size_t work_bytes,
                         int batch, int32_t* status_dev, void* hip_stream);

/* ---- Classification on the device (Evaluation, network_helper.cpp:143-207; INTEGRATION.md "Classification on the device") ----
 * A classifier belongs to a network handle whose final map is 1 x 1 (it reads the handle's q table at create: a later set_q needs
 * a new classifier).  Per image, from the int8 logits [batch][n] a run writes (n = N of the last row) and the runtime Q row of the
 * last layer's output -- the row Evaluation's callers pass, q[NUM_LAYER] (main.cpp:53):
 *   features   f[i] = (float)logit[i] / (float)(1 << sh[i]), sh[i] = -q[i] in 0..30 (exact in float32);
 *   top-k      the first top_k entries by (feature descending, index descending on equal features) -- the closed form of the
 *              reference's k bubble passes with a strict '>'; labels and features are bit-identical to the host function at the
 *              end of this header;
 *   probs      max-subtracted float32 softmax: d[i] = f[i] - fmax (one IEEE subtraction), p[i] = expf(d[i]) / sum_j expf(d[j]),
 *              the sum in a fixed order (64 strided partial sums, then a 6-step butterfly), so a run repeats bit for bit.  The
 *              reference's text (and network.Evaluation, which keeps it) does not subtract the maximum: its exp overflows once a
 *              feature passes ~88 and the result is inf / inf.  Mathematically the two agree; where Evaluation's result is finite
 *              the two differ by rounding only;
 *   truth      truth[b] < 0: unlabelled, rank[b] = -1, nothing counted; 0 <= truth[b] < n: rank[b] = the label's position among
 *              the top_k (0 = best) or -1; truth[b] >= n: a bad label, rank[b] = -1;
 *   tally      uint64 [4], ACCUMULATED (the caller zeroes it): {images with truth >= 0 (bad labels included: they are misses),
 *              rank == 0, rank >= 0, bad labels}.  Integer adds only: exact, order-independent, and a captured graph replayed
 *              over a validation set leaves the counts on the device with no synchronisation in between.
 * tf2_amd.classify.reference is the host statement.  Create checks on the host, before any device call (TF2_ERR_ARG with a
 * message; TF2_ERR_STATE before the q table is set): desc size, a 1 x 1 final map that is the net's only output (SSD300 has heads: refused), top_k in 1..min(n, 64), every Q of the last row
 * in 0..30; n outside 2..4096 is TF2_ERR_UNSUPPORTED.  The handle holds read-only device constants (the 2^-sh scales).  A run
 * checks batch >= 1 and non-null logits_dev / labels_dev, then enqueues one kernel on hip_stream: no allocation, no
 * synchronisation, a grid that depends on batch alone (graph-capturable; several streams run side by side on their own outputs).
 * labels_dev int32 [batch][top_k]; every later pointer is optional (NULL): features_dev, probs_dev float32 [batch][top_k],
 * all_probs_dev float32 [batch][n], truth_dev int32 [batch], rank_dev int32 [batch], tally_dev uint64 [4]. */
typedef struct tf2_cls tf2_cls;
typedef struct tf2_cls_desc {
  uint32_t size;                    /* sizeof(tf2_cls_desc) */
  int32_t top_k;                    /* 1..min(n, 64) */
} tf2_cls_desc;
tf2_status tf2_cls_create(tf2_net* net, const tf2_cls_desc* d, tf2_cls** out);
void       tf2_cls_destroy(tf2_cls* c);
tf2_status tf2_cls_run(tf2_cls* c, const int8_t* logits_dev, int batch, int32_t* labels_dev, float* features_dev, float* probs_dev,
                       float* all_probs_dev, const int32_t* truth_dev, int32_t* rank_dev, uint64_t* tally_dev, void* hip_stream);

/* ---- Face matching on the device (1:N search of a feature library, faceverify/README.md; INTEGRATION.md "Face matching on the
 * device") ----
 * A matcher belongs to a network handle whose only output is a 1 x 1 map of D = 2..512 channels, the embedding network (SqueezeNet
 * 1.1 with its 1000 -> 128 row: D = 128); it reads the handle's q table at create.  The reference ships no program text for the
 * matching, so this statement is the canonical one (tf2_amd.embed.reference_embed / reference_match / reference_tally are the host
 * statement; every device output is bit-identical to them).  All arithmetic is IEEE float32, every operation rounded separately
 * (no fused multiply-add), every sum taken for c ascending from +0:
 *   embedding  f[c] = (float)out[c] / (float)(1 << sh[c]), sh[c] = -q[c] in 0..30 of the last layer's runtime Q row (exact);
 *              s = sum_c f[c] * f[c];  e[c] = f[c] / sqrt(s), sqrt and division correctly rounded;  s == 0: e = 0, no division.
 *   distance   d(b, n) = sum_c (e[b][c] - g[n][c])^2 to row n of the gallery, float32 [n_rows][D] row-major in device memory that the
 *              caller owns (a feature library read from a file goes straight in; enrolling is the embed call with a row of the
 *              gallery as its output).  A NaN distance (from a caller's row only) counts, and is reported, as +inf.
 *   top-k      the first top_k rows by (distance ascending, row index ascending): idx_dev int32, dist_dev float32 [batch][top_k];
 *              slots past n_rows read idx -1, dist +inf, id -1.  ids_out_dev (optional) receives gallery_ids_dev[idx], or idx where
 *              gallery_ids_dev is NULL; emb_out_dev (optional) the queries' embeddings float32 [batch][D].
 *   tally      uint64 [5], ACCUMULATED (the caller zeroes it), with truth_dev int32 [batch]: truth < 0 is unlabelled, nothing
 *              counted; else {labelled, id[0] == truth, any of the top_k ids == truth, true accepts: dist[0] < threshold and
 *              id[0] == truth, false accepts: dist[0] < threshold and id[0] != truth}.  The comparison is a strict float32 '<'; a
 *              truth that no gallery row carries is an impostor.  Integer adds only: exact and order-independent.
 * A match enqueues three kernels on hip_stream (embed; stage 1: a block per slab of 64 gallery rows and 32 queries keeps the slab's
 * best top_k per query as 64-bit keys in the scratch; stage 2: a wave per query merges them): no allocation, no synchronisation,
 * grids that depend on batch, n_rows and the handle's constants alone (graph-capturable; a captured graph fixes n_rows).  The
 * scratch is caller-provided device memory, 8-byte aligned, of at least the stated size for (batch, n_rows); concurrent matches
 * need their own.  Host checks, before any device call (TF2_ERR_ARG with a message unless stated): create -- desc size, null net, q
 * table not set (TF2_ERR_STATE), a final 1 x 1 map that is the net's only output, D outside 2..512 (TF2_ERR_UNSUPPORTED), every Q of
 * the last row in 0..30, top_k in 1..16; run -- batch >= 1, n_rows >= 1, non-null required pointers, a threshold that is not NaN,
 * scratch_bytes below the stated size (TF2_ERR_SIZE). */
typedef struct tf2_emb tf2_emb;
typedef struct tf2_emb_desc {
  uint32_t size;                    /* sizeof(tf2_emb_desc) */
  int32_t top_k;                    /* 1..16 */
} tf2_emb_desc;
tf2_status tf2_emb_create(tf2_net* net, const tf2_emb_desc* d, tf2_emb** out);
void       tf2_emb_destroy(tf2_emb* m);
size_t     tf2_emb_scratch_size(const tf2_emb* m, int batch, int n_rows);
tf2_status tf2_emb_embed(tf2_emb* m, const int8_t* out_i8_dev, int batch, float* rows_dev, void* hip_stream);
tf2_status tf2_emb_match(tf2_emb* m, const int8_t* out_i8_dev, int batch, const float* gallery_dev, const int32_t* gallery_ids_dev,
                         int n_rows, float threshold, void* scratch_dev, size_t scratch_bytes, int32_t* idx_dev, float* dist_dev,
                         int32_t* ids_out_dev, float* emb_out_dev, const int32_t* truth_dev, uint64_t* tally_dev, void* hip_stream);

/* ---- Threshold calibration on the device (the verification curve of an embedding network; INTEGRATION.md "Threshold calibration
 * on the device") ----
 * Where tf2_emb_match's `threshold` comes from: the genuine and impostor distance histograms of a labelled set of float32 rows
 * (what tf2_emb_embed writes into a gallery), from which TAR at a target FAR, the EER and the LFW fold accuracies are read.  The two
 * calls need no handle.  tf2_amd.embed.roc_thresholds / reference_roc_hist / reference_pairs are the host statement; every count and
 * every distance is bit-identical to them.
 *   grid       thr[t] = (float)(t + 1) * step, t = 0 .. n_thr - 1: one float32 multiply (FaceNet's arange(0, 4, 0.01) on squared
 *              distances is n_thr = 400, step = 0.01f).  The kernels compute it from (n_thr, step).
 *   distance   tf2_emb_match's d for the same two rows, bit for bit: the sum over c ascending from +0 of separately rounded
 *              (a[c] - b[c])^2; a NaN distance counts as +inf.
 *   bin        bin(d) = #{t : thr[t] <= d} in 0..n_thr.  A pair is accepted at threshold t iff d < thr[t] iff bin(d) <= t: the
 *              strict float32 '<' of the tally, so a threshold read off the histogram means the same thing to tf2_emb_match.
 *   hist       int64 [2][n_thr + 1], ACCUMULATED (the caller zeroes it): hist[same][bin], same = (ids_a[i] == ids_b[j]).  Self mode
 *              (rows_b_dev == NULL; ids_b_dev and n_b are ignored) counts every pair i < j of one set, cross mode every (i, j).  A row
 *              whose id is < 0 takes part in no pair.  Integer adds only: exact, independent of grid, tile and order.
 *   pairs      pairs_dev int32 [n_pairs][4] = (a, b, same, fold); dist_dev[p] = d(rows[a], rows[b]) (NaN reported as +inf), and 1 is
 *              added to hist[fold][same][bin(d)], int64 [n_folds][2][n_thr + 1], ACCUMULATED.  A pair with a or b outside
 *              0..n_rows-1, same not in {0, 1} or fold outside 0..n_folds-1 is invalid: it reads no row, gets dist -1.0f, adds 1 to
 *              invalid_dev[0] (ACCUMULATED) and nothing to hist.  The check is made on the device: the host never sees the list.
 * The all-pairs call enqueues one kernel: a block a pair of tiles of 256 rows (self mode: the pairs ti <= tj alone), every
 * distance binned on the fly into a block-local histogram; the distance matrix is never written.  The listed-pairs call enqueues
 * one kernel, a wave a pair.  No allocation, no synchronisation, no scratch; grids that depend on the scalar arguments alone
 * (graph-capturable).  Host checks, before any device call (TF2_ERR_ARG with a message unless stated): d in 2..512; n_a, n_b (cross
 * mode), n_rows, n_pairs >= 1; n_thr in 1..4096; step finite and > 0; n_folds in 1..16; non-null rows, ids (ids_b_dev in cross
 * mode), pairs, dist, hist and invalid pointers; more than 2^31 - 1 tile pairs (TF2_ERR_UNSUPPORTED). */
tf2_status tf2_emb_roc_hist(const float* rows_a_dev, const int32_t* ids_a_dev, int n_a,
                            const float* rows_b_dev, const int32_t* ids_b_dev, int n_b,   /* rows_b_dev == NULL: self mode, i < j */
                            int d, int n_thr, float step, int64_t* hist_dev /* [2][n_thr+1], ACCUMULATED */, void* hip_stream);
tf2_status tf2_emb_roc_pairs(const float* rows_dev, int n_rows, int d, const int32_t* pairs_dev /* [n_pairs][4] */, int n_pairs,
                             int n_folds, int n_thr, float step, float* dist_dev /* [n_pairs] */,
                             int64_t* hist_dev /* [n_folds][2][n_thr+1], ACCUMULATED */, int64_t* invalid_dev /* [1], ACCUMULATED */,
                             void* hip_stream);

/* ---- Activation audit on the device (the integer side of Quantization/debug/CompareError.py; INTEGRATION.md "Activation audit on the
 * device") ----
 * Does a Q file fit the integer engine?  An audit handle reduces every kept map of a keep_all step to exact per-channel integer
 * statistics in a caller-owned device buffer, the STORE, accumulated over as many batches as the caller runs or replays: which channels
 * clip at 127 / -128 and how often, which use three of their eight bits, what the image row's Q0 makes of the input.
 * tf2_amd.audit.reference_audit is the host statement; the store equals it as integers.
 *   record     16 little-endian int64 a channel: 0 n (values seen), 1 neg (v < 0), 2 lo_rail (v == -128), 3 hi_rail (v == 127), 4 min
 *              (empty: 127), 5 max (empty: -128), 6 sum of v, 7 sum of v * v, 8..15 hist[b], b = bit length of |v| (0 for 0, 1 for 1,
 *              2 for 2..3, ... 7 for 64..127); |v| = 128 is counted in lo_rail alone, so the hist sums to n - lo_rail.
 *   values     of table row l: the tensor tf2_net_read_layer hands back for l -- after pool, add and global average ([B][N] for an
 *              end-pool row), in the reference's int8 values: the kernel reads the workspace's own NHWC layout (channel pitch, concat
 *              slice offset) and undoes the doubled form 2y - 128 of the channels the packed image flags, y = (v + 128) >> 1.
 *   store      record 0 .. image_c - 1: the network INPUT ("row -1"), taken from the caller's images_dev, dense [B][C][H][W] -- float
 *              values quantised by the engine's own input rule with 2^Q0, int8 values as they are (the workspace's input tensor may
 *              hold an x-only or im2col form that does not contain every pixel).  Then rows 0 .. n_layers - 1 in table order, each
 *              row's N channels contiguous (a concat member is audited on its own slice; pooling and L2Norm rows are rows like any
 *              other).  tf2_audit_store_size = 128 * (image_c + sum of N); tf2_audit_describe lists (layer, C, H, W, byte offset,
 *              channels in the doubled form) per row, row -1 first, and needs no device.
 * tf2_audit_create needs a packed net (TF2_ERR_STATE otherwise) and allocates nothing on the device; the net must outlive the handle
 * and keep its tables.  tf2_audit_store_init enqueues the empty store (zeros, min 127, max -128).  tf2_audit_run enqueues the
 * keep_all step of `batch` images -- logits_dev receives the ordinary logits, bit-identical to tf2_net_run -- and behind it, on the
 * same stream, one kernel for the input record and one for every 64 table rows (a block: 1024 pixels x 256 channels of one row;
 * 64-bit integer atomics for the non-zero counters).  Integer adds, minima and maxima only: the store is exact and independent of
 * grid, order and streams.  No allocation, no synchronisation, no host-side state: graph-capturable; the row descriptions travel in
 * the kernel arguments, the doubled-form flags are read from the bound packed image.
 * Refusals, before anything is enqueued: null handle / images / workspace / logits / store, batch <= 0 (TF2_ERR_ARG); a net not packed
 * or not bound to the device (TF2_ERR_STATE); workspace_bytes < tf2_audit_workspace_size (the keep_all plan's size) or store_bytes <
 * tf2_audit_store_size (TF2_ERR_SIZE); tf2_audit_describe with capacity < n_layers + 1 (TF2_ERR_SIZE, *n set).
 * tf2_audit_kept enqueues the audit kernels alone, on a workspace whose last step was this batch's keep_all step (tf2_audit_run's,
 * or tf2_net_run's on a workspace of the keep_all size) and on the images that step received: what the step left there is the
 * caller's statement, the library cannot check it.  It is how tools/act_audit_time.py times the audit by itself; same refusals. */
typedef struct tf2_audit tf2_audit;
typedef struct tf2_audit_row {
  int32_t layer, C, H, W;           /* layer -1: the input record */
  int64_t store_offset;             /* bytes, of the row's first record */
  int32_t n_doubled, reserved;      /* channels of the row stored as 2y - 128 */
} tf2_audit_row;
tf2_status tf2_audit_create(tf2_net* net, tf2_audit** out);
void       tf2_audit_destroy(tf2_audit* a);
size_t     tf2_audit_store_size(const tf2_audit* a);
tf2_status tf2_audit_describe(const tf2_audit* a, tf2_audit_row* rows, int capacity, int* n);
tf2_status tf2_audit_store_init(const tf2_audit* a, void* store_dev, size_t store_bytes, void* hip_stream);
size_t     tf2_audit_workspace_size(tf2_audit* a, int batch);
tf2_status tf2_audit_run(tf2_audit* a, const void* images_dev, int images_are_q, int batch, void* workspace_dev, size_t workspace_bytes,
                         int8_t* logits_dev, void* store_dev, size_t store_bytes, void* hip_stream);
tf2_status tf2_audit_kept(tf2_audit* a, const void* images_dev, int images_are_q, int batch, void* workspace_dev, size_t workspace_bytes,
                          void* store_dev, size_t store_bytes, void* hip_stream);

/* ---- Layer fidelity on the device (Quantization/debug/CompareError.py and Verify(), network_helper.cpp:18-141, for every row;
 * INTEGRATION.md "Layer fidelity on the device") ----
 * How far is each channel of each layer from the float network?  A fidelity handle sets every kept int8 map of a keep_all step
 * against the float32 map of a float forward (tf2_amd.calibrate.float_forward, or any other producer) and keeps exact per-channel
 * integer statistics in a caller-owned device buffer, the STORE, accumulated over as many batches as the caller runs or replays.
 * tf2_amd.fidelity.reference_compare is the host statement; the store equals it as integers.
 *   per value  v: the int8 value tf2_net_read_layer hands back for row l at (b, c, h, w), the doubled form 2y - 128 undone as in the
 *              audit.  f: the float32 reference at the same (b, c, h, w).  Q: the channel's scale exponent, Verify's for that row
 *              (1 << -q[l + 1][c] in the runtime table; a pooling row, ipool == 1, carries its source's), any integer in -64 .. 64.
 *              In this order:  f is NaN or +-inf: nonfinite += 1 and nothing else.  t = f * 2^(Q + 8), ONE float32 multiplication
 *              (exact unless it overflows to +-inf).  |t| >= 65536: e = +-65536 with t's sign, ref_clamped += 1.  Otherwise
 *              e = rint(t), half to even (65535.5 -> 65536, not counted as clamped).  d = 256 v - e, so |d| < 2^17.
 *              k = min(7, bit_length((|d| + 128) >> 8)): the error in whole LSBs after rounding; k = 0: v is the nearest int8.
 *   record     18 little-endian int64 a channel: 0 n (finite f), 1 nonfinite, 2 ref_clamped, 3 max_abs_d (a maximum; 0 when empty),
 *              4 sum_d (signed), 5 sum_abs_d, 6 sum_d2, 7 sum_abs_e, 8 sum_e2, 9 sum_q2 = sum of (256 v)^2, 10..17 hist[k].  Every
 *              slot but 3 is a sum; the empty store is all zeros; two stores combine by adding, slot 3 by the maximum.
 *   budget     d^2 < 2^34: sum_d2 holds 2^29 values a channel even if every value were wrong by the full range; e^2 <= 2^32 and
 *              (256 v)^2 <= 2^30 hold more.
 *   store      the audit's layout: record 0 .. image_c - 1 the network INPUT ("row -1"), then rows 0 .. n_layers - 1 in table order,
 *              each row's N channels contiguous.  tf2_fid_store_size = 144 * (image_c + sum of N); tf2_fid_describe lists the rows as
 *              tf2_audit_describe does (store_offset in bytes of THIS store) and needs no device.  Row -1 compares float images with
 *              their own quantisation: v = the engine's input rule on f with 2^Q0, e from the same f with Q0; with int8 images
 *              (images_are_q) the row is not compared and its records stay as they are.
 *   scales     the kernels read 2^(Q + 8) per record from a device table of tf2_fid_store_size / 144 float32 the CALLER keeps:
 *              tf2_fid_scales writes the table to host memory (no device needed), the caller uploads it once (the handle owns no
 *              device memory and a run allocates none).  What scales_dev holds is the caller's statement.
 *   refs       a HOST array of n_layers device pointers, refs[l] the reference of row l: dense float32 [batch][C][H][W] with the
 *              row's C, H, W of tf2_fid_describe ([batch][C] for an end-pool row) -- a concat member is its own slice.  Each buffer
 *              must hold batch * C * H * W floats: the library cannot check device sizes.  refs[l] == NULL: row l is not compared,
 *              costs no block and keeps its records.  The pointers are read at enqueue and travel in the kernel arguments: a
 *              captured graph replays on the same buffers, refilled.
 * tf2_fid_create needs a packed net with its q table set (TF2_ERR_STATE otherwise; TF2_ERR_UNSUPPORTED where 2^(Q + 8) is no normal
 * float32) and allocates nothing on the device; the net must outlive the handle and keep its tables and q.  tf2_fid_store_init
 * enqueues the empty store (zeros).  tf2_fid_run enqueues the keep_all step of `batch` images -- logits_dev receives the ordinary
 * logits, bit-identical to tf2_net_run -- and behind it, on the same stream, one kernel for the input record (float images) and one
 * for every 64 compared rows (a block: 1024 pixels x 64 channels of one row, the float side transposed through LDS; 64-bit integer
 * atomics for the non-zero counters, a 64-bit atomic maximum for slot 3).  Integer adds and maxima only: the store is exact and
 * independent of grid, order and streams.  No allocation, no synchronisation, no host state read at replay: graph-capturable.
 * tf2_fid_kept enqueues the comparison alone, on a workspace whose last step was this batch's keep_all step and on the images that
 * step received (as tf2_audit_kept; tools/fidelity_time.py times it).
 * Refusals, before anything is enqueued: null handle / images / workspace / logits / store / refs / scales, batch <= 0
 * (TF2_ERR_ARG); a net not packed or not bound to the device (TF2_ERR_STATE); workspace_bytes < tf2_fid_workspace_size (the keep_all
 * plan's size) or store_bytes < tf2_fid_store_size (TF2_ERR_SIZE); tf2_fid_describe with capacity < n_layers + 1 and tf2_fid_scales
 * with capacity < the records (TF2_ERR_SIZE, *n set). */
typedef struct tf2_fid tf2_fid;
tf2_status tf2_fid_create(tf2_net* net, tf2_fid** out);
void       tf2_fid_destroy(tf2_fid* f);
size_t     tf2_fid_store_size(const tf2_fid* f);
tf2_status tf2_fid_describe(const tf2_fid* f, tf2_audit_row* rows, int capacity, int* n);
tf2_status tf2_fid_scales(const tf2_fid* f, float* scales /* host */, int capacity, int* n);
tf2_status tf2_fid_store_init(const tf2_fid* f, void* store_dev, size_t store_bytes, void* hip_stream);
size_t     tf2_fid_workspace_size(tf2_fid* f, int batch);
tf2_status tf2_fid_run(tf2_fid* f, const void* images_dev, int images_are_q, int batch, void* workspace_dev, size_t workspace_bytes,
                       int8_t* logits_dev, const float* const* refs /* host array [n_layers] of device pointers */,
                       const float* scales_dev, void* store_dev, size_t store_bytes, void* hip_stream);
tf2_status tf2_fid_kept(tf2_fid* f, const void* images_dev, int images_are_q, int batch, void* workspace_dev, size_t workspace_bytes,
                        const float* const* refs, const float* scales_dev, void* store_dev, size_t store_bytes, void* hip_stream);

/* ---- CAQ calibration on the device (TransForm_Kit/Quantization/feature_write.py and quantization.py: QuantizeForShift,
 * QuantizeChannel; INTEGRATION.md "Calibration on the device") ----
 * The step that makes the Q file: which power-of-two scale keeps each channel of each float map inside int8?  The two passes read the
 * float32 maps of a float forward (tf2_amd.fidelity.float_refs, or any other producer) once each and keep exact per-channel integer
 * records in caller-owned device buffers, the STORES, accumulated over as many batches as the caller runs or replays.  They need no
 * net, no packed image and no Q table: they run before any exists.  tf2_amd.caq.reference_range / reference_error are the host
 * statement; the stores equal it as integers.  tf2_amd.caq turns host copies of the stores into Q rows (q_max: the reference's rule,
 * bit for bit; q_clip: a clip-share rule; q_mse: an error-minimising rule).
 *   fit        of a finite non-zero float32 f: the largest integer q with |f| * 2^q <= 127, stated on the bit pattern: with e the
 *              unbiased exponent and m the 24-bit significand (a denormal normalised first), fit = 6 - e where m <= 0xFE0000, else
 *              5 - e.  QuantizeForShift of a non-negative channel is fit of its peak.  The maps are read as 32-bit patterns, so a
 *              denormal counts as the value it is, whatever the flush mode.
 *   RANGE      tf2_caq_range, 70 little-endian int64 a channel: 0 n (finite values), 1 nonfinite (NaN, +-inf: nothing else is
 *              recorded for these), 2 zeros (+-0), 3 negatives (finite, < 0), 4 peak_pos (the magnitude bit pattern of the largest
 *              positive value, 0 when none), 5 peak_neg (of the most negative value, 0 when none), 6..69 hist[b] with
 *              b = clamp(fit(f), -32, 31) + 32 over the non-zero finite values.  Slots 4 and 5 are maxima, every other slot is a
 *              sum; the empty store is all zeros; two stores combine by adding, slots 4 and 5 by the maximum.  The sum of hist[b]
 *              over b < Q + 32 counts the values beyond the rail at exponent Q.
 *   ERROR      tf2_caq_error, 12 little-endian int64 a channel, against a base exponent Qb per record, any integer in -64 .. 64: the
 *              kernel reads 2^(Qb + 7) per record from a device table of float32 the CALLER keeps (tf2_amd.caq.scale_of); what
 *              scales_dev holds is the caller's statement.  The candidates are Q = Qb + j, j = 0 .. 3 (below Qb = fit(peak) nothing
 *              clips and the step only coarsens).  Per value, in this order:  f is NaN or +-inf: nonfinite += 1 and nothing else.
 *              t = f * 2^(Qb + 7), ONE float32 multiplication.  |t| >= 2^18 (an overflow to inf included): e = +-2^18 with t's sign,
 *              ref_clamped += 1; otherwise e = rint(t), half to even.  For each j, with s = 7 - j: u = (e + (1 << (s - 1))) >> s
 *              (arithmetic shift), v = clamp(u, -128, 127), clipped_j += (u != v), d = e - (v << s), sum_d2_j += d^2.
 *              Slots: 0 n, 1 nonfinite, 2 ref_clamped, 3 sum_e2, 4..7 clipped_j, 8..11 sum_d2_j.  Every slot is a sum.
 *   budget     |d| < 2^18 + 2^14, so d^2 < 2^37: a sum_d2 slot holds 2^26 values a channel even if every value were wrong by the full
 *              range; e^2 <= 2^36 holds more.
 *   denormals  with |Qb| <= 64 a denormal input or product gives |t| < 0.5 and e = 0 in either flush mode.
 *   rows       a HOST array of n_rows descriptors (C, HW, the row's first record) and a HOST array of n_rows device pointers,
 *              maps[i] the dense float32 [batch][C][HW] map of row i ([batch][C] where HW is 1).  Each buffer must hold
 *              batch * C * HW floats, 4-byte aligned: the library cannot check device sizes.  maps[i] == NULL: row i is not read,
 *              costs no block and keeps its records.  The pointers are read at enqueue and travel in the kernel arguments: a
 *              captured graph replays on the same buffers, refilled.  The audit's record layout is the convention: the network
 *              input's channels first ("row -1", the float images), then the table rows in order.
 * The functions are stateless.  A call enqueues one kernel for every 64 observed rows (a block: 32768 values of one channel, walked
 * through all images in 16-byte groups with a guarded head and tail, the histogram counted per wave by ballot over the distinct bins;
 * 64-bit integer atomics for the non-zero counters, 64-bit atomic maxima for the peaks).  Integer adds and maxima only: the stores are
 * exact and independent of grid, order and streams.  No allocation, no synchronisation, no host state read at replay:
 * graph-capturable.  tf2_caq_store_init enqueues the empty store (zeros) over store_bytes.
 * Refusals, before anything is enqueued (no device needed): null rows / maps / store / scales, n_rows < 1, batch <= 0, C <= 0,
 * HW <= 0, a negative first record, record ranges that overlap, a store or map that is not aligned (TF2_ERR_ARG); a row whose records
 * reach beyond store_bytes (TF2_ERR_SIZE); batch * HW or a record index beyond 2^31 (TF2_ERR_UNSUPPORTED). */
typedef struct tf2_caq_row { int32_t C, HW; int64_t first_record; } tf2_caq_row;
size_t     tf2_caq_range_store_size(int64_t n_records);     /* 560 * n_records */
size_t     tf2_caq_error_store_size(int64_t n_records);     /* 96 * n_records */
tf2_status tf2_caq_store_init(void* store_dev, size_t store_bytes, void* hip_stream);
tf2_status tf2_caq_range(const tf2_caq_row* rows /* host */, const void* const* maps /* host array [n_rows] of device pointers */,
                         int n_rows, int batch, void* store_dev, size_t store_bytes, void* hip_stream);
tf2_status tf2_caq_error(const tf2_caq_row* rows /* host */, const void* const* maps, int n_rows, int batch, const float* scales_dev,
                         void* store_dev, size_t store_bytes, void* hip_stream);

/* ---- INQ weight quantisation on the device (TransForm_Kit/Compression/compress_net/core/compress_core.py: ComputeQuantumRange,
 * ShapeIntoTwoPower; INTEGRATION.md "Weight quantisation on the device") ----
 * The engine computes on weights that are 0 or +-2^-i (tf2_get_real reads anything else as +-1 or 0, silently).  tf2_inq_step makes
 * such weights from float ones by the reference's incremental rule: of every tensor's still-float weights the largest become powers of
 * two (the caller retrains the rest and calls again with a larger portion).  One call works on many tensors -- SEGMENTS (offset, count
 * in elements) of one flat float32 device buffer -- in place, with a parallel uint8 mask buffer (non-zero: still float, 0: quantised).
 * Elements in no segment are never read or written.  tf2_amd.inq.reference_range / reference_step are the host statement; weights,
 * masks, codes and every word of the state equal it as bits.  All arithmetic is on float32 bit patterns, mag = bits & 0x7fffffff:
 *   exp_of     of mag > 0: the e with 0.75 * 2^e <= a < 1.5 * 2^e (the reference's floor(log(4a/3) / log 2)): E + 1 where the mantissa
 *              field is >= 0x400000, else E; denormals by the same inequality from the leading bit.  (The reference's double log gives
 *              E at a = 1.5 * 2^E exactly for 20 values of E, all <= -30; the integer rule gives E + 1 there as everywhere.)
 *   range      n1 / n0 = still-float / quantised weights, max1 / max0 the largest mag of each set.  n1 == 0: max_exp = -100, nothing to
 *              do.  max0 == 0 (nothing, or only zeros, fixed so far): max_exp = exp_of(max1), or -100 with TF2_INQ_ALL_ZERO where max1 is
 *              0 too.  Otherwise max_exp = the leading-bit exponent of max0 (a power of two), and exp_of(max1) > max_exp sets
 *              TF2_INQ_RANGE_GREW (the reference exits there).  A NaN or inf anywhere in the tensor: TF2_INQ_NONFINITE, max_exp -100.
 *              min_exp = max_exp - n_values + 1.  A tensor with a status bit is left untouched: n_keep = n1, n_update = 0.
 *   rank       n_keep = rint(rint(n1 / (1 - prev)) * (1 - cur)) in double, half to even; n_update = n1 - n_keep; nothing changes when
 *              n_update <= 0.  thr = the mag of index n_keep in the ascending order of mag over the still-float weights.
 *   shape      a still-float weight with mag >= thr (every tie included) gets mask 0 and, with e = min(exp_of(mag), 127): +-2^e with
 *              its sign where e >= min_exp and e >= exp_floor, else +0.0 (flushed_min counts e < min_exp, flushed_floor the others; a
 *              selected +-0 becomes +0.0 and counts in neither).  over_one counts the weights emitted with e > 0, which the engine
 *              cannot represent.  exp_floor = -127 is the reference's behaviour, -14 the engine's smallest weight.
 *   codes      optional, one byte an element of a segment (codes_dev parallel to weights_dev), the 4-bit file's code relative to THIS
 *              step's min_exp: 15 for a still-float weight, 7 for zero, k = e - min_exp for a negative and k + 8 for a positive power of
 *              two, 15 where k is outside 0..6.  hist[16] counts them over the whole segment, with or without codes_dev.
 *   state      32 little-endian int64 a segment, rewritten by every call: 0 n1, 1 n0, 2 max1, 3 max0 (patterns), 4 non-finite count,
 *              5 max_exp, 6 min_exp, 7 n_keep, 8 n_update, 9 thr (pattern; 0 when nothing is updated), 10 status, 11 flushed_min,
 *              12 flushed_floor, 13 over_one, 14..29 hist[16], 30..31 zero.  tf2_inq_state_size = 256 * n_segs.
 * A call enqueues, for every 96 segments: the range kernel, four select passes (an exact radix select of the rank-n_keep pattern:
 * block-local LDS histograms of 8, 8, 8 and 7 bits, integer atomics, the prefix resolved on the device in between) and the shape
 * kernel; before them one kernel that zeroes state and scratch.  No host copy, no synchronisation, no allocation, grids that depend
 * on the host arguments alone: graph-capturable, and a replay on refilled weights and masks equals a fresh call.  Integer adds,
 * maxima and plain stores only: the result does not depend on grid or order.
 * Refusals, before anything is enqueued (no device needed): null weights / mask / segs / state / scratch, n_segs < 1, a table that does
 * not ascend without overlap inside n_total or has a count outside 1 .. 2^31 - 1, prev outside [0, 1), cur outside [prev, 1], n_values
 * outside 1..15, exp_floor outside -150..127, state or scratch not 8-byte aligned (TF2_ERR_ARG); scratch_bytes <
 * tf2_inq_scratch_size (TF2_ERR_SIZE).  16-byte accesses are used where weights_dev is 16-byte and mask_dev / codes_dev are 4-byte
 * aligned (any alignment is correct). */
enum { TF2_INQ_RANGE_GREW = 1, TF2_INQ_ALL_ZERO = 2, TF2_INQ_NONFINITE = 4 };
typedef struct tf2_inq_seg { int64_t offset, count; } tf2_inq_seg;     /* elements of the flat buffer */
size_t     tf2_inq_scratch_size(int n_segs);
size_t     tf2_inq_state_size(int n_segs);
tf2_status tf2_inq_step(float* weights_dev, uint8_t* mask_dev, int64_t n_total, const tf2_inq_seg* segs /* host */, int n_segs,
                        double prev, double cur, int n_values, int exp_floor, uint8_t* codes_dev /* or NULL */, void* state_dev,
                        void* scratch_dev, size_t scratch_bytes, void* hip_stream);

/* ---- Channel pruning on the device (TransForm_Kit/DnsChannelpruning: dnscp_core.py cal_mean_std / maskChannelCalc, model_convert.py;
 * INTEGRATION.md "Channel pruning on the device") ----
 * DNS-CP prunes INPUT channels of a conv [N][C][k][k] whose mean magnitude falls under a threshold taken from the conv's own mean and
 * deviation, revives them above a higher one, and forces the kept count to a multiple of 16.  tf2_dnscp_step does that for many convs
 * -- descriptors (host records) over one flat float32 device buffer -- with one keep byte a channel (non-zero: kept) and writes the
 * masked weights; the dense weights stay the caller's (out_dev may equal dense_dev).  The random gate, the training loop and the
 * thresholds' arithmetic stay with the caller.  tf2_amd.dnscp.reference_stats / reference_step are the host statement; keep bytes, the
 * output, S1 and every word of the record equal it as bits.  Float sums have no defined order, so the rule is stated on bit patterns:
 *   fixed point  E = the leading-bit exponent of the conv's largest FINITE magnitude (denormals from the leading bit; -1000 for none);
 *                m(a) = floor(a * 2^(31 - E)), 0 <= m < 2^32, a shift of the significand; m = 0 for a non-finite pattern.
 *   sums         S1[c] = sum of m over input channel c (dense).  Over the channels kept at entry: A1 = sum m, A2_hi = sum (m^2 >> 32),
 *                A2_lo = sum (m^2 & 0xffffffff), nz = the patterns with mag != 0; n = N * C * kk.  Exact for N * kk < 2^22, n < 2^28.
 *   thresholds   host arithmetic (tf2_amd.dnscp.thresholds: mu = A1 / nz, var = (A2 - n mu^2) / n, T = max(mu + c_rate * sqrt(var), 0),
 *                t_lo = alpha_low * T, t_hi = alpha_high * T in the weights' units), handed in by the descriptor; >= 0 or NaN.
 *   compare      B = floor(t * double(N * kk) * 2^(31 - max(E, -149))): one IEEE multiply, an exact scaling, a floor, clamped to
 *                [-1, 2^63 - 1]; a NaN t_lo gives B_lo = -1, a NaN t_hi B_hi = 2^63 - 1 (nothing changes) and TF2_DNSCP_NAN_THRESHOLD.
 *                A kept channel with S1[c] <= B_lo is pruned, a pruned one with S1[c] > B_hi revived.
 *   fix-up       nz_c kept channels behind the compare; target = 16 * rint(nz_c / 16) (half to even), 16 where that is 0.  The first
 *                pruned channels by index are revived, or the first kept ones pruned, until the count is the target or C runs out.
 *   output       out = dense where the channel is kept, else the pattern 0x00000000 (the reference's multiply leaves -0.0 for a
 *                negative weight; tf2_get_real reads both as zero).  Convs without TF2_DNSCP_UPDATE get their keep bytes applied as
 *                they are.  A conv holding a NaN or inf: TF2_DNSCP_NONFINITE, its keep bytes and its part of out_dev left as they were.
 *   record       16 little-endian int64 a conv, rewritten by every call: 0 n, 1 nz, 2 non-finite count, 3 max pattern, 4 E, 5 A1,
 *                6 A2_hi, 7 A2_lo, 8 kept before, 9 pruned by t_lo, 10 revived by t_hi, 11 fix-up (+ revived, - pruned), 12 kept
 *                after, 13 status, 14 B_lo, 15 B_hi (9..11, 14, 15 are 0 without TF2_DNSCP_UPDATE).  tf2_dnscp_state_size = 128 * n_convs.
 * keep_dev and sums_dev (int64 S1) are indexed alike: conv i owns [keep_offset, keep_offset + C) of n_channels.  tf2_dnscp_stats writes
 * the record and S1 only (keep_dev NULL: all kept).  A step enqueues, for every 48 convs: zeroing, the max pass, the sum pass (every
 * filter read once; 64-bit LDS adds, one 64-bit atomic per channel and block), one decision block a conv, the apply pass.  No host
 * copy, no synchronisation, no allocation, grids from the host arguments alone: graph-capturable; integer adds and maxima only, so the
 * result does not depend on grid or order.  tf2_dnscp_scratch_size is 0 with these kernels (scratch_dev may be NULL).
 * tf2_dnscp_compact is the export (model_convert.py): for every segment dst[n'][c'][j] = src[n_idx[n']][c_idx[c']][j], j < kk, the
 * index lists int32 in idx_dev at element offsets n_idx / c_idx (-1: identity); an index outside the source tensor writes a NaN.
 * One launch per 48 segments.
 * Refusals, before anything is enqueued (no device needed): null dense / out / keep (step) / convs / sums / state, n_convs < 1, sizes
 * < 1, a conv table or keep ranges that do not ascend without overlap inside n_total / n_channels, unknown flags, TF2_DNSCP_UPDATE in
 * tf2_dnscp_stats, a negative threshold, out_dev overlapping dense_dev without being equal, state or sums not 8-byte aligned
 * (TF2_ERR_ARG); C > 4096, N * kk >= 2^22, n >= 2^28 (TF2_ERR_UNSUPPORTED).  tf2_dnscp_compact: null pointers, sizes < 1, a source
 * tensor outside n_src, destinations that do not ascend without overlap inside n_dst, an index list outside n_idx or an identity
 * between unequal sizes, dst_dev overlapping src_dev (TF2_ERR_ARG). */
enum { TF2_DNSCP_UPDATE = 1 };                                                      /* flags */
enum { TF2_DNSCP_ALL_ZERO = 1, TF2_DNSCP_NONFINITE = 2, TF2_DNSCP_NAN_THRESHOLD = 4 };   /* status */
typedef struct tf2_dnscp_conv { int64_t offset; int32_t N, C, kk, flags; int64_t keep_offset; double t_lo, t_hi; } tf2_dnscp_conv;
typedef struct tf2_dnscp_seg { int64_t src_offset, dst_offset; int32_t n_src, c_src, n_out, c_out, kk, reserved; int64_t n_idx, c_idx; } tf2_dnscp_seg;
size_t     tf2_dnscp_state_size(int n_convs);
size_t     tf2_dnscp_scratch_size(int n_convs);
tf2_status tf2_dnscp_stats(const float* weights_dev, int64_t n_total, const tf2_dnscp_conv* convs /* host */, int n_convs,
                           const uint8_t* keep_dev /* or NULL */, int64_t n_channels, int64_t* sums_dev, void* state_dev,
                           void* scratch_dev, size_t scratch_bytes, void* hip_stream);
tf2_status tf2_dnscp_step(const float* dense_dev, float* out_dev, int64_t n_total, const tf2_dnscp_conv* convs /* host */, int n_convs,
                          uint8_t* keep_dev, int64_t n_channels, int64_t* sums_dev, void* state_dev, void* scratch_dev,
                          size_t scratch_bytes, void* hip_stream);
tf2_status tf2_dnscp_compact(const float* src_dev, int64_t n_src, float* dst_dev, int64_t n_dst, const tf2_dnscp_seg* segs /* host */,
                             int n_segs, const int32_t* idx_dev, int64_t n_idx, void* hip_stream);

/* ---- Detection accuracy on the device (the PASCAL VOC devkit protocol behind the README's SSD mAP; INTEGRATION.md "Detection accuracy
 * on the device") ----
 * The reference ships no evaluation code (ssd.py: no weights, no dataset, no eval script), so this statement is the canonical one.
 * An evaluator belongs to no net and holds no device memory: it takes any det [batch][num_classes][top_k][5] / counts
 * [batch][num_classes] of the layout tf2_ssd_run writes, ground truth in the same normalised corner form, and keeps the dataset-level
 * record in a caller-owned device buffer, the STORE, of `capacity` image slots.
 * Matching (tf2_det_eval_run, one kernel a step): per image and class c >= 1, walk the class's rows r = 0 .. counts-1 (best first).
 * For row r go over the image's ground truths of class c in index order, difficult ones included, and keep the one with the largest
 * IoU (strict '>' starting from none: the lowest index wins a tie, a NaN IoU never wins).  Then flag[r] =
 *    0  no winner, or its IoU is not > iou_thresh (strict, float32): false positive
 *   -1  the winner is difficult: ignored
 *    1  the winner is not yet taken: true positive, and it is now taken
 *    0  the winner is already taken: duplicate (no fall-back to the second best, as in the devkit)
 *   -2  rows past counts[b][c], and every row of class 0.
 * IoU is plain IoU on the caller's coordinates in IEEE float32, ssd._iou_one_to_many's arithmetic inter / ((area_gt - inter) +
 * area_det) with the min / max of ssd_detect.hip (a NaN operand is ignored); the devkit's "+1 pixel" convention is not applied.
 * ssd.match_reference is the host statement; the device output is bit-identical to it.
 * Store layout (tf2_det_eval_store_size bytes; sections in this order, no padding, K = top_k, C = num_classes):
 *   seen   int32   [capacity]          1 once an image was evaluated into the slot
 *   npos   int32   [capacity][C]       non-difficult ground truths per class
 *   scores float32 [capacity][C][K]    the rows' scores (0 where the flag is -2)
 *   flags  int8    [capacity][C][K]
 * A step writes every byte of each slot it owns (slot_dev[b]) with ordinary stores: no atomics, no append counters.  The store is a
 * pure function of the set of (slot, image) pairs: independent of replay order and streams; evaluating an image twice overwrites;
 * slots need no clearing between epochs, only `seen` is zeroed (tf2_det_eval_store_init: a memset on the stream).  The slots of one
 * step, and of steps in flight side by side, must be distinct.  slot_dev[b] < 0: the image is skipped (padding of a last batch),
 * nothing is written to the store and status_dev[b] = 0.
 * Device checks: the records are device data (refill them between graph replays, like tf2_image_src), so the kernel validates each
 * image before it uses anything as an index and writes status_dev[b] = 0 or an OR of TF2_EVAL_* bits; a malformed image writes
 * nothing to the store and its `seen` is not set.  No read leaves the buffers described here.  Optional flags_out_dev
 * [batch][C][K] int8 receives the step's flags directly (-2 everywhere for a skipped or malformed image).
 * Host checks (TF2_ERR_ARG with a message, before any device call): create -- desc size, num_classes 2..256, top_k 1..256, max_gt
 * 1..256, capacity >= 1, iou_thresh finite and >= 0; run -- batch >= 1, non-null det / counts / gt / gt_count / slot / store / status,
 * store_bytes >= tf2_det_eval_store_size.  The grid depends on batch and the handle's constants alone; no allocation, no
 * synchronisation (graph-capturable).
 * tf2_det_eval_summarise runs on the HOST CPU on a host copy of the store, once per dataset: per class the records of seen slots with
 * flag >= 0, ordered by (score descending, slot ascending, rank ascending; a NaN score last) -- the devkit's argsort leaves ties
 * undefined -- then cumulative tp / fp (int64), recall = tp / npos, precision = tp / (tp + fp) in double, and AP by the devkit's
 * 11-point metric (use_07_metric != 0: thresholds k * 0.1, k = 0..10, the maximum precision at recall >= threshold or 0) or its
 * all-point metric (recall bracketed by 0 and 1, the monotone precision envelope from the right, sum of delta recall x precision).
 * per_class [C]; a class with npos == 0 (class 0 always) has ap = NaN and is left out of *map, the mean over the others (NaN if
 * there is none); *images = number of seen slots. */
typedef struct tf2_det_eval tf2_det_eval;
typedef struct tf2_gt_box {         /* one ground truth, in DEVICE memory, [batch][max_gt] */
  float x1, y1, x2, y2;
  int32_t label;                    /* 1..num_classes-1 */
  int32_t difficult;                /* != 0: matched detections are ignored, not counted in npos */
} tf2_gt_box;
typedef struct tf2_det_eval_desc {
  uint32_t size;                    /* sizeof(tf2_det_eval_desc) */
  int32_t num_classes;              /* 2..256, including background class 0 */
  int32_t top_k;                    /* 1..256 */
  int32_t max_gt;                   /* 1..256: ground truths an image may have */
  int32_t capacity;                 /* >= 1: image slots of the store */
  float iou_thresh;                 /* finite, >= 0 (VOC: 0.5) */
} tf2_det_eval_desc;
enum {                              /* status_dev bits of a malformed image */
  TF2_EVAL_BAD_SLOT = 1,            /* slot >= capacity */
  TF2_EVAL_BAD_COUNT = 2,           /* gt_count outside 0..max_gt (labels and boxes are then not looked at) */
  TF2_EVAL_BAD_LABEL = 4,           /* a label outside 1..num_classes-1 */
  TF2_EVAL_BAD_BOX = 8,             /* a non-finite coordinate, or x2 < x1, or y2 < y1 */
  TF2_EVAL_BAD_DET = 16             /* a counts[b][c] outside 0..top_k */
};
typedef struct tf2_det_eval_class { double ap; int64_t npos, tp, fp; } tf2_det_eval_class;
tf2_status tf2_det_eval_create(const tf2_det_eval_desc* d, tf2_det_eval** out);
void       tf2_det_eval_destroy(tf2_det_eval* e);
size_t     tf2_det_eval_store_size(const tf2_det_eval* e);
tf2_status tf2_det_eval_store_init(const tf2_det_eval* e, void* store_dev, size_t store_bytes, void* hip_stream);
tf2_status tf2_det_eval_run(const tf2_det_eval* e, const float* det_dev, const int32_t* counts_dev, const tf2_gt_box* gt_dev,
                            const int32_t* gt_count_dev, const int32_t* slot_dev, int batch, void* store_dev, size_t store_bytes,
                            int32_t* status_dev, int8_t* flags_out_dev, void* hip_stream);
tf2_status tf2_det_eval_summarise(const tf2_det_eval* e, const void* store_host, size_t store_bytes, int use_07_metric,
                                  tf2_det_eval_class* per_class, int64_t* images, double* map);

/* ---- Evaluation (network_helper.cpp:143-207): top-k with the reference's tie rule ---- */
tf2_status tf2_topk(const int8_t* logits, const int8_t* q_last_row, int n, int k,
                    int32_t* labels, float* features);

#ifdef __cplusplus
}
#endif
#endif /* TF2_AMD_H_ */
