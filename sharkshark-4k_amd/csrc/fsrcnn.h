// FSRCNN: the weight blob (fsrcnn_weights.cpp) and the whole-network forward on fp32 planes (fsrcnn.hip).
#pragma once
#include "common.h"

namespace ss4k {

struct ParamCursor;   // models.h

// The device blob fsrcnn_pack_weights produces, as pointers into it: all fp32
struct FsrcnnWeights {
  const float* w_feat;   // [25][56]   tap-major, cout-minor
  const float* b_feat;   // [56]
  const float* a_feat;   // [56] PReLU
  const float* w_shrink; // [56][12]
  const float* b_shrink; const float* a_shrink;  // [12]
  const float* w_map[4]; // [9][12][12]  tap, cin, cout
  const float* b_map[4]; const float* a_map[4];
  const float* w_expand; // [12][56]
  const float* b_expand; const float* a_expand;  // [56]
  const float* w_deconv; // [81][56]  (ky*9+kx), cin
  float b_deconv;
  bool prelu_abs = false;   // matrix-core modes: producing weights / biases scaled by (1 + s) / 2 and the slope arrays hold (1 - s) / (1 + s): PReLU is y + c |y|
};

// Takes the network's parameters from the state_dict cursor (key order of the reference's model), converts them to the layouts above, uploads
// the blob into `dev` and points W into it; returns the blob's bytes.  exact (in: the caller asks for the exact-fp32 kernels) comes back true
// as well for a checkpoint the matrix-core modes cannot take: a PReLU slope at or below -0.875, or a scaled value outside the fp16 range.
// Otherwise the blob is scaled for the one-fma PReLU (W.prelu_abs).
size_t fsrcnn_pack_weights(ParamCursor& pc, bool& exact, DevBuf& dev, FsrcnnWeights& W);

// mode: fp32 accuracy on the fp16 matrix rate (hi/lo-split operands, the default of an SS4K_F32 model), the exact-fp32 kernels, or
// plain fp16 operands with fp32 accumulation (an SS4K_F16 model: the precision the reference's TensorRT engine runs FSRCNN in)
enum { FS_MODE_SPLIT = 0, FS_MODE_EXACT = 1, FS_MODE_HALF = 2 };
void fsrcnn_forward(ss4k_ctx* ctx, const FsrcnnWeights& W, int factor, const float* in, float* out, int planes, int h,
                    int w, float* ws12a, float* ws12b, int mode, hipStream_t st, bool out_half = false,
                    bool in_u8 = false);   // out_half: fp16 mode only, HR planes as fp16; in_u8: `in` is the uint8 NHWC frame tensor (planes / 3 frames)

}  // namespace ss4k
