// roi_crop_aa.hip -- detections -> a second network's input with Pillow's antialiased bilinear resize (tf2_roi_crop_aa,
// include/tf2_amd.h): each slot of a ROI table is Image.resize((OW, OH), BILINEAR, box=(x0, y0, x1, y1)) of its 8-bit source image,
// restated bit for bit (resample_aa.h, the box form: 22-bit integer coefficients, a horizontal pass to bytes, a vertical pass on
// those bytes), then channel pick, per-channel mean and scale, and optionally the input quantisation of runner.cpp:158-164.  The
// filter is centred on the box and as wide as the box's scale asks: it reads source pixels outside the box and inside the image, so
// the result is not "crop, then resize".  tf2_amd/roi.py restates it (reference_crop_aa) and the device output is bit-identical to it.
//
// The tile kernel is image_input.h's aa_tile_kernel (the scheme is described there), the one tf2_preprocess_aa runs, with the
// geometry below; the grid is n_slots x ceil(image_h / 8) x ceil(image_w / 32) blocks whatever the table holds (a captured graph stays
// valid when a new table, new records and new pixels are written into the same buffers).  The slot's record and its source record are
// device data: every block validates both before it reads a pixel; a slot with a status -- most slots of a real table are EMPTY --
// stores zeros and leaves without a barrier.  The first column's and the first row's thread leave ceil(support) of their axis in LDS,
// which bounds the taps of the whole axis (n <= 2 * ceil(support) + 1).
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "tf2_device.h"
#include "tf2_net.h"
#include "image_input.h"
#include "roi_crop.h"

namespace tf2 {

namespace {

// float boxes through tf2_roi records: Pillow's box form
struct AaBox {
  static constexpr bool kSupportInLds = true;
  tf2_roi R;
  // TF2_ROI_* bits of one slot (0: cropped).  tf2_roi_crop's rule, then -- only for a slot that rule passes -- the box inside the image
  // (double on the float32 values; -0.0 is inside) and the scale bound on the float32 side the filter is built from
  __device__ __forceinline__ int load(const ImageArgs& a, int s, tf2_image_src& r, const tf2_roi* rois) {
    R = rois[s];
    int st = slot_source(a, R.image, box_ok(R.x0, R.y0, R.x1, R.y1) ? 0 : TF2_ROI_BAD_BOX, r);
    if (st == 0) {
      if (!((double)R.x0 >= 0.0 && (double)R.x1 <= (double)r.w && (double)R.y0 >= 0.0 && (double)R.y1 <= (double)r.h))
        st |= TF2_ROI_BOX_OUTSIDE;
      if ((double)(R.x1 - R.x0) > (double)(kAaMaxScale * a.OW) || (double)(R.y1 - R.y0) > (double)(kAaMaxScale * a.OH))
        st |= TF2_ROI_BAD_SCALE;
    }
    return st;
  }
  __device__ __forceinline__ AaAxis axis(const ImageArgs& a, const tf2_image_src&, bool col) const {
    return aa_axis_box(col ? R.x0 : R.y0, col ? R.x1 : R.y1, col ? a.OW : a.OH);
  }
  __device__ __forceinline__ void bounds(const AaAxis& ax, const tf2_image_src& r, bool col, int o, double& center, int& lo, int& n) const {
    aa_bounds_box(ax, col ? R.x0 : R.y0, o, col ? r.w : r.h, center, lo, n);
  }
  __device__ __forceinline__ int taps(const tf2_image_src&) const { return 0; }   // (not used: kSupportInLds)
};

}  // namespace

tf2_status roi_crop_aa(const Net& net2, const tf2_preprocess_desc* d, const uint8_t* pixels, size_t pixels_bytes,
                       const tf2_image_src* srcs, int batch, const tf2_roi* rois, int n_slots, int out_q, void* out, int32_t* status,
                       void* stream) {
  std::string why = preprocess_refusal(net2, d, batch, out_q, pixels && srcs && out && status && rois);
  if (why.empty() && n_slots < 1) why = "n_slots must be >= 1";
  if (why.empty())
    why = launch_aa_tiles<AaBox>(image_args(net2, d, out_q, pixels, pixels_bytes, srcs, batch, out, status), out_q, n_slots, "n_slots",
                                 stream, rois);
  return why.empty() ? launch_result("tf2_roi_crop_aa") : arg_refusal("tf2_roi_crop_aa", why);
}

}  // namespace tf2
