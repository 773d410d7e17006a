// What the 2-D convolution units offer each other: the float32 kernels (csrc/svs_conv2d.hip), the matrix-core kernels
// (csrc/svs_conv2d_mfma.hip) and the encoder that the "fpn" and "unet" feature extractors share (csrc/svs_conv2d.hip,
// csrc/svs_ucsnet.hip).
#pragma once
#include "svs_common.h"

namespace svs {
namespace conv2d {

// svs_conv2d behind its argument checks: weight in the packed layout, k in {1,3,5}, stride in {1,2}
int run_conv(const float* in, const float* weight, const float* bias, const float* add, int add_upsample2, float* out,
             int Cin, int Cout, int H, int W, int k, int stride, int relu, hipStream_t s);

// Where the encoder's eight layers write: conv0 = (c0a, c0) at (b,H,W), conv1 = (c1a, c1b, c1) at (2b,H/2,W/2), conv2 = (c2a,
// c2b, c2) at (4b,H/4,W/4).  The U-Net points c0 and c1 into its concatenation buffers.
struct EncoderBuffers {
  float *c0a, *c0, *c1a, *c1b, *c1, *c2a, *c2b, *c2;
};

// Layers 0-7 of both feature extractors (models/CasMVSNet.py:343-361, models/ucsnet.py:244-259): conv + folded BatchNorm +
// ReLU, enqueued in layer order.  Layer i runs on the matrix cores where wfrags (null, or at least 8 entries) holds its
// fragments and the shape is supported, else on the float32 kernels.
int run_encoder(const float* image, int H, int W, int b, const float* const* weights, const float* const* biases,
                const void* const* wfrags, const EncoderBuffers& o, hipStream_t s);

}  // namespace conv2d

namespace conv2dmfma {
bool supported(int Cin, int Cout, int k, int stride);
int run(const float* in, const void* wfrag, const float* bias, float* out, int Cin, int Cout, int H, int W, int k, int stride,
        int relu, hipStream_t s);
int run_lateral(const float* lat_in, const float* lat_w, const float* lat_b, const float* lat_add, const void* wfrag,
                const float* bias, float* out, int Cout, int H, int W, int relu, hipStream_t s);
}  // namespace conv2dmfma
}  // namespace svs
