// Device functions that the kernels of frvsr.hip (degradation 'BD') and frvsr_bi.hip (degradation 'BI') share: the grid rule, backward_warp's
// arithmetic and the record store of the fused warp + space-to-depth kernels.  Written with explicit __fmaf_rn / __fmul_rn / __fadd_rn so that
// the compiler contracts nothing differently in any of the kernels that include them.  Included by .hip files only.
#pragma once
#include "frvsr.h"

namespace ss4k {

#define SS4K_LAUNCH_OK() SS4K_HIP(hipGetLastError())

static inline dim3 grid_for(size_t n, int block = 256) {
  size_t g = (n + block - 1) / block;
  if (g > 256 * 8 * 4) g = 256 * 8 * 4;   // grid-stride beyond a few waves per CU
  return dim3((unsigned)std::max<size_t>(g, 1));
}

// sampling position of backward_warp in pixels, in the reference's order of operations: torch.linspace(-1, 1, size)[i] (ATen's
// symmetric form) + flow / ((size - 1) / 2) (net_utils.py:62-72), then grid_sample's un-normalisation for align_corners=True,
// ((g + 1) / 2) * (size - 1), and its border clip.  fminf / fmaxf drop a NaN flow: the position is always inside [0, size - 1]
__device__ __forceinline__ float warp_pos(int i, int size, float flow) {
  const float step = 2.f / (float)(size - 1);
  const float lin = i < size / 2 ? __fmaf_rn(step, (float)i, -1.f) : __fmaf_rn(-step, (float)(size - i - 1), 1.f);   // (ATen's linspace fuses the multiply-add)
  const float g = __fadd_rn(lin, __fdiv_rn(flow, (float)(((double)size - 1.0) / 2.0)));
  const float p = __fmul_rn(__fdiv_rn(__fadd_rn(g, 1.f), 2.f), (float)(size - 1));
  return fminf((float)(size - 1), fmaxf(p, 0.f));
}
struct WarpTaps { int x0, x1, y0, y1; float nw, ne, sw, se; };
__device__ __forceinline__ WarpTaps warp_taps(int X, int Y, int W, int H, float fx, float fy) {
  const float px = warp_pos(X, W, fx), py = warp_pos(Y, H, fy);
  const float x0 = floorf(px), y0 = floorf(py);
  const float ex = __fadd_rn(__fadd_rn(x0, 1.f), -px), ey = __fadd_rn(__fadd_rn(y0, 1.f), -py);   // ix_se - ix, iy_se - iy
  const float dx = __fadd_rn(px, -x0), dy = __fadd_rn(py, -y0);
  WarpTaps t;
  t.x0 = (int)x0; t.y0 = (int)y0; t.x1 = min(t.x0 + 1, W - 1); t.y1 = min(t.y0 + 1, H - 1);   // (a tap past the border has weight 0)
  t.nw = __fmul_rn(ex, ey); t.ne = __fmul_rn(dx, ey); t.sw = __fmul_rn(ex, dy); t.se = __fmul_rn(dx, dy);
  return t;
}
__device__ __forceinline__ float warp_sample(const float* __restrict__ pl, int W, const WarpTaps& t) {
  const float a = pl[(size_t)t.y0 * W + t.x0], b = pl[(size_t)t.y0 * W + t.x1], c = pl[(size_t)t.y1 * W + t.x0], d = pl[(size_t)t.y1 * W + t.x1];
  return __fmaf_rn(d, t.se, __fmaf_rn(c, t.sw, __fmaf_rn(b, t.ne, __fmul_rn(a, t.nw))));
}

// The 48 channels (sy * 4 + sx) * 3 + c of LR pixel i as three records of 16 T, one per plane
template <typename T> union S2dRecord { T v[48]; uint4 u[3 * sizeof(T)]; };
// ... stored with 16-byte stores: plane p's record of pixel i of npix
template <typename T>
__device__ __forceinline__ void s2d_store(const S2dRecord<T>& rec, uint4* __restrict__ out, size_t i, size_t npix) {
  constexpr int RV = sizeof(T);   // 16-byte slots per record
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < RV; ++q) out[((size_t)p * npix + i) * RV + q] = rec.u[p * RV + q];
}

}  // namespace ss4k
