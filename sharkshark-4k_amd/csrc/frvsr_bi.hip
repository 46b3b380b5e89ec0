// Degradation 'BI' of the frame-recurrent generators: the reference's get_upsampling_func (utils/net_utils.py:96-108) then is
// F.interpolate(scale_factor=4, mode='bilinear', align_corners=False) where 'BD' has BicubicUpsample(4).  It is used in two places: the
// x4 of the LR flow before the warp (both generators) and TecoGAN's skip conv_out + upsample_func(lr_curr).  This file holds the bilinear
// up-sampler and the launchers that instantiate the stage kernels of frvsr_stages.h with it; the x4 exists once, as bil4_load / bil4_at,
// for the granular op and both fused kernels, so the fused tensors are bit-identical to the chain of the granular ops.
//
// ATen's definition for output index d of a size-`size` axis: src = max(0, 0.25 (d + 0.5) - 0.5), i0 = floor(src), i1 = min(i0 + 1, size - 1),
// lambda = src - i0, value = (1 - lambda) in[i0] + lambda in[i1].  With d = 4 i + s: src = i + (s - 1.5) / 4, so phase s of input pixel i reads
//   s = 0: (i - 1, i) lambda 0.625     s = 1: (i - 1, i) lambda 0.875     s = 2: (i, i + 1) lambda 0.125     s = 3: (i, i + 1) lambda 0.375
// and at i = 0 (s < 2) the max() gives in[0] itself; at i = size - 1 (s >= 2) i0 = i1.  Both borders take lambda = 0 here, so the first two and
// the last two outputs of a row or column ARE the border value, bit for bit (ATen rounds 0.875 v + 0.125 v at the far border).
// Order of operations: the WIDTH pass first on each of the two rows, r = fma(lx, right, (1 - lx) * left), then the height pass
// fma(ly, r_below, (1 - ly) * r_above) - ATen's order.  1 - lambda is exact for all five lambdas, every weight is a dyadic rational.
#include "frvsr_stages.h"

namespace ss4k {

// 3 x 3 neighbourhood of (y, x) with the indices clamped: rows clamp(y - 1 .. y + 1), columns clamp(x - 1 .. x + 1).  Always inside the plane
__device__ __forceinline__ void bil4_load(const float* __restrict__ pl, int y, int x, int h, int w, float f[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int yy = min(max(y - 1 + i, 0), h - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) f[i][j] = pl[(size_t)yy * w + min(max(x - 1 + j, 0), w - 1)];
  }
}
// lambda of phase s at input index i of a size-`size` axis: 0 where the pair of the phase is the border value twice.  Selects only, no table: the
// fused kernels unroll s, the per-value kernels take it from the output index
__device__ __forceinline__ float bil4_lambda(int s, int i, int size) {
  const bool low = s < 2;
  const float l = __fmaf_rn(0.25f, (float)s, low ? 0.625f : -0.375f);   // 0.625, 0.875, 0.125, 0.375: exact
  return (low ? i == 0 : i == size - 1) ? 0.f : l;
}
__device__ __forceinline__ float bil4_lerp(float l, float a, float b) { return __fmaf_rn(l, b, __fmul_rn(__fadd_rn(1.f, -l), a)); }
// output (4 y + sy, 4 x + sx) of input pixel (y, x) with neighbourhood f: phases 0, 1 pair rows / columns (0, 1) of f, phases 2, 3 pair (1, 2)
__device__ __forceinline__ float bil4_at(const float f[3][3], int sy, int sx, int y, int x, int h, int w) {
  const bool r = sy >= 2, c = sx >= 2;
  const float lx = bil4_lambda(sx, x, w), ly = bil4_lambda(sy, y, h);
  const float t0 = c ? f[0][1] : f[0][0], t1 = c ? f[0][2] : f[0][1];
  const float m0 = c ? f[1][1] : f[1][0], m1 = c ? f[1][2] : f[1][1];
  const float b0 = c ? f[2][1] : f[2][0], b1 = c ? f[2][2] : f[2][1];
  const float above = bil4_lerp(lx, r ? m0 : t0, r ? m1 : t1), below = bil4_lerp(lx, r ? b0 : m0, r ? b1 : m1);
  return bil4_lerp(ly, above, below);
}
// the up-sampler of frvsr_stages.h's kernels
struct UpBilinear4 {
  static constexpr int N = 3;
  __device__ __forceinline__ void load(const float* __restrict__ pl, int y, int x, int h, int w, float f[3][3]) const { bil4_load(pl, y, x, h, w, f); }
  __device__ __forceinline__ float at(const float f[3][3], int sy, int sx, int y, int x, int h, int w) const { return bil4_at(f, sy, sx, y, x, h, w); }
};

// ------------------------------------------------------------------ the launchers: frvsr.hip's, with the bilinear x4
void op_bilinear_upsample4(const float* in, float* out, int planes, int h, int w, hipStream_t st) {
  launch_up4("frvsr_bi::bilinear_upsample4", "bilinear x4", in, out, planes, h, w, UpBilinear4{}, st);
}
template <typename T>
void op_warp_s2d_bi_planes(const float* lr_flow, const float* hr_prev, T* out, int n, int h, int w, hipStream_t st) {
  launch_warp_s2d(sizeof(T) == 2 ? "frvsr_bi::warp_s2d_bi_planes<half>" : "frvsr_bi::warp_s2d_bi_planes<float>", "warp (bilinear)", lr_flow,
                  Strided<const float>{hr_prev, (size_t)48 * h * w}, out, n, h, w, UpBilinear4{}, st);
}
template void op_warp_s2d_bi_planes<float>(const float*, const float*, float*, int, int, int, hipStream_t);
template void op_warp_s2d_bi_planes<__half>(const float*, const float*, __half*, int, int, int, hipStream_t);
template <typename T>
void op_warp_s2d_bi_planes_items(const float* lr_flow, const FrvsrPtrs& hr_prev, T* out, int n, int h, int w, hipStream_t st) {
  launch_warp_s2d(sizeof(T) == 2 ? "frvsr_bi::warp_s2d_bi_planes_items<half>" : "frvsr_bi::warp_s2d_bi_planes_items<float>", "warp (bilinear, items)", lr_flow,
                  Table{hr_prev}, out, n, h, w, UpBilinear4{}, st);
}
template void op_warp_s2d_bi_planes_items<float>(const float*, const FrvsrPtrs&, float*, int, int, int, hipStream_t);
template void op_warp_s2d_bi_planes_items<__half>(const float*, const FrvsrPtrs&, __half*, int, int, int, hipStream_t);
void op_bilinear4_add(const float* conv, const float* lr, float* out, int n, int h, int w, hipStream_t st) {
  launch_x4_add("frvsr_bi::bilinear4_add", "bilinear4_add", conv, Strided<const float>{lr, (size_t)3 * h * w}, Strided<float>{out, (size_t)48 * h * w}, n, h, w,
                UpBilinear4{}, st);
}
void op_bilinear4_add_items(const float* conv, const FrvsrPtrs& lr, const FrvsrPtrs& out, int n, int h, int w, hipStream_t st) {
  launch_x4_add("frvsr_bi::bilinear4_add_items", "bilinear4_add (items)", conv, Table{lr}, Table{out}, n, h, w, UpBilinear4{}, st);
}

}  // namespace ss4k
