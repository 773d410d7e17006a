// The image work of the MVS loader for gfx950 (datasets/general_eval.py:157-176, 220-232, 254, 267-268 and
// runner.py:106): read_img's code / 255, scale_mvs_input's cv2.resize(img, (W,H), interpolation=cv2.INTER_CUBIC) once or
// twice, the transpose to planes and the alpha split, for V views of one size per call.  Restated in float64 in
// tests/mvsdata_oracle.py.
//
// The resize is the shared 4x4 gather of svs_resize.h (coordinates, clamping, order of operations: there).  A source is
// either 8-bit codes or float32 (the second pass of the x2_mvsres chain reads what the first wrote).  A code's value is
// read_img's np.float32(code) / 255. -- a float32 DIVISION, where svs_scene.hip multiplies by float32(1/255).  The 256
// values come from the host as a device table (numpy's own division), so nothing here depends on how the device divides:
// the code-to-float rule is TableCode for codes and Identity for float32.
//
// svs_mvs_resize_cubic: the resize alone, channel-last, C = 3 or 4.  Equal sizes: a copy of the values.
// svs_mvs_resize_pack: the same resize with the sample's layout as its output: planes imgs (V,3,H,W) and masks
//   (V,1,H,W); C = 4: rgb times the resized alpha and the resized alpha itself -- the product AFTER the resize, as
//   imgs[:,:3]*imgs[:,3:] is -- C = 3: rgb and ones.  The channel-last result is never written.
// svs_mvs_codes: np.clip(img * 255, 0, 255).astype(np.uint8) of planes (3,H,W) to (H,W,3): a float32 multiply, the
//   clip, truncation toward zero (NaN, which numpy leaves to the platform's cast: 0).
//   One thread per destination pixel, consecutive threads along W.
#include "svs_resize.h"

namespace svs {
namespace mvsdata {

using namespace svs::image;

constexpr int kThreads = 256;

// grid: (ceil(W / kThreads), H)
__global__ __launch_bounds__(kThreads) void codes_kernel(const float* __restrict__ img, uint8_t* __restrict__ codes, int H,
                                                        int W) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const size_t plane = (size_t)H * W, at = (size_t)y * W + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s = img[c * plane + at] * 255.0f;
    // np.clip keeps NaN; the comparisons below are false for it and it becomes code 0
    codes[at * 3 + c] = s >= 255.0f ? (uint8_t)255 : (s > 0.0f ? (uint8_t)(int)s : (uint8_t)0);
  }
}

template <bool PACK>
int launch(const char* what, const void* src, int src_is_float, const float* table, int V, int Hs, int Ws, int C, int H,
           int W, const int* xofs, const float* xcoef, const int* yofs, const float* ycoef, float* out, float* masks,
           void* hip_stream) {
  if (!src || !out || (PACK && !masks)) { set_error("%s: null argument", what); return SVS_EINVAL; }
  if (src_is_float != 0 && src_is_float != 1) { set_error("%s: src_is_float must be 0 or 1", what); return SVS_EINVAL; }
  if (!src_is_float && !table) { set_error("%s: null code table for a source of codes", what); return SVS_EINVAL; }
  if (C != 3 && C != 4) { set_error("%s: C must be 3 or 4", what); return SVS_EINVAL; }
  if (V < 1) { set_error("%s: V must be >= 1", what); return SVS_EINVAL; }
  int rc = check_image(what, "H and W", H, W);
  if (rc || (rc = check_image(what, "Hs and Ws", Hs, Ws)) || (rc = check_grid_dim(what, "V", V)) ||
      (rc = check_grid_dim(what, "H", H)))
    return rc;
  auto* go = src_is_float ? (C == 3 ? launch_resize<Identity, 3, PACK> : launch_resize<Identity, 4, PACK>)
                          : (C == 3 ? launch_resize<TableCode, 3, PACK> : launch_resize<TableCode, 4, PACK>);
  return go(what, src, table, V, Hs, Ws, H, W, xofs, xcoef, yofs, ycoef, out, masks, hip_stream);
}

}  // namespace mvsdata
}  // namespace svs

using namespace svs;
using namespace svs::mvsdata;

extern "C" {

int svs_mvs_resize_cubic(const void* src, int src_is_float, const float* code_table, int V, int Hs, int Ws, int C, int H,
                         int W, const int* xofs, const float* xcoef, const int* yofs, const float* ycoef, float* out,
                         void* hip_stream) {
  return launch<false>("svs_mvs_resize_cubic", src, src_is_float, code_table, V, Hs, Ws, C, H, W, xofs, xcoef, yofs, ycoef,
                       out, nullptr, hip_stream);
}

int svs_mvs_resize_pack(const void* src, int src_is_float, const float* code_table, int V, int Hs, int Ws, int C, int H,
                        int W, const int* xofs, const float* xcoef, const int* yofs, const float* ycoef, float* imgs,
                        float* masks, void* hip_stream) {
  return launch<true>("svs_mvs_resize_pack", src, src_is_float, code_table, V, Hs, Ws, C, H, W, xofs, xcoef, yofs, ycoef,
                      imgs, masks, hip_stream);
}

int svs_mvs_codes(const float* img, int H, int W, uint8_t* codes, void* hip_stream) {
  const char* what = "svs_mvs_codes";
  if (!img || !codes) { set_error("%s: null argument", what); return SVS_EINVAL; }
  int rc = check_image(what, "H and W", H, W);
  if (rc || (rc = check_grid_dim(what, "H", H))) return rc;
  codes_kernel<<<dim3((W + kThreads - 1) / kThreads, H), kThreads, 0, (hipStream_t)hip_stream>>>(img, codes, H, W);
  return check_launch(what);
}

}  // extern "C"
