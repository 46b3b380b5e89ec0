// Glue kernels of the frame-recurrent generators built with degradation 'BI': the reference's get_upsampling_func (utils/net_utils.py:96-108)
// then is F.interpolate(scale_factor=4, mode='bilinear', align_corners=False) where 'BD' has BicubicUpsample(4).  It is used in two places: the
// x4 of the LR flow before the warp (both generators) and TecoGAN's skip conv_out + upsample_func(lr_curr).  The kernels here are the 'BI'
// twins of frvsr.hip's bicubic_upsample4, warp_s2d_planes[_items] and bicubic4_add[_items]; the warp and the record store are the SAME device
// functions (frvsr_warp.h), and the x4 exists once, as bil4_load / bil4_at, for the granular op and both fused kernels, so the
// fused tensors are bit-identical to the chain of the granular ops.
//
// ATen's definition for output index d of a size-`size` axis: src = max(0, 0.25 (d + 0.5) - 0.5), i0 = floor(src), i1 = min(i0 + 1, size - 1),
// lambda = src - i0, value = (1 - lambda) in[i0] + lambda in[i1].  With d = 4 i + s: src = i + (s - 1.5) / 4, so phase s of input pixel i reads
//   s = 0: (i - 1, i) lambda 0.625     s = 1: (i - 1, i) lambda 0.875     s = 2: (i, i + 1) lambda 0.125     s = 3: (i, i + 1) lambda 0.375
// and at i = 0 (s < 2) the max() gives in[0] itself; at i = size - 1 (s >= 2) i0 = i1.  Both borders take lambda = 0 here, so the first two and
// the last two outputs of a row or column ARE the border value, bit for bit (ATen rounds 0.875 v + 0.125 v at the far border).
// Order of operations: the WIDTH pass first on each of the two rows, r = fma(lx, right, (1 - lx) * left), then the height pass
// fma(ly, r_below, (1 - ly) * r_above) - ATen's order.  1 - lambda is exact for all five lambdas, every weight is a dyadic rational.
#include "frvsr_warp.h"

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

// ------------------------------------------------------------------ F.interpolate(scale_factor=4, 'bilinear', align_corners=False): the granular op
__global__ __launch_bounds__(256) void k_bilinear_upsample4(const float* __restrict__ in, float* __restrict__ out, int planes, int h, int w) {
  const int OW = 4 * w, OH = 4 * h;
  const size_t total = (size_t)planes * OH * OW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % OW), Y = (int)((i / OW) % OH);
    const size_t pl = i / ((size_t)OW * OH);
    float f[3][3];
    bil4_load(in + pl * h * w, Y >> 2, X >> 2, h, w, f);
    out[i] = bil4_at(f, Y & 3, X & 3, Y >> 2, X >> 2, h, w);
  }
}
void op_bilinear_upsample4(const float* in, float* out, int planes, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(planes > 0 && h > 0 && w > 0 && h <= (1 << 28) && w <= (1 << 28), "bilinear x4: sizes");
  SS4K_GLUE_ROUTE("frvsr_bi::bilinear_upsample4");
  hipLaunchKernelGGL(k_bilinear_upsample4, grid_for((size_t)planes * 16 * h * w), dim3(256), 0, st, in, out, planes, h, w);
  SS4K_LAUNCH_OK();
}

// ------------------------------------------------------------------ flow x4 + warp + space-to-depth -> three planes
// One thread per LR pixel, as k_warp_s2d_planes: its 3 x 3 clamped flow neighbourhood serves all 16 sub-pixels, and the 48 channels
// (sy * 4 + sx) * 3 + c it produces are the three records it stores, with 16-byte stores.  pixel i of item img: `src` is that item's hr_prev
template <typename T>
__device__ __forceinline__ void warp_s2d_bi_pixel(const float* __restrict__ lr_flow, const float* __restrict__ src, uint4* __restrict__ out, size_t i, size_t img,
                                                  size_t npix, int h, int w) {
  const int H = 4 * h, W = 4 * w;
  const size_t hw = (size_t)h * w, HW = (size_t)H * W;
  const int x = (int)(i % w), y = (int)((i / w) % h);
  S2dRecord<T> rec;
  float fu[3][3], fv[3][3];
  bil4_load(lr_flow + (img * 2) * hw, y, x, h, w, fu);
  bil4_load(lr_flow + (img * 2 + 1) * hw, y, x, h, w, fv);
#pragma unroll
  for (int sy = 0; sy < 4; ++sy)
#pragma unroll
    for (int sx = 0; sx < 4; ++sx) {
      const float u = __fmul_rn(4.f, bil4_at(fu, sy, sx, y, x, h, w)), v = __fmul_rn(4.f, bil4_at(fv, sy, sx, y, x, h, w));
      const WarpTaps t = warp_taps(4 * x + sx, 4 * y + sy, W, H, u, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) rec.v[(sy * 4 + sx) * 3 + c] = (T)warp_sample(src + c * HW, W, t);
    }
  s2d_store<T>(rec, out, i, npix);
}
template <typename T>
__global__ __launch_bounds__(256) void k_warp_s2d_bi_planes(const float* __restrict__ lr_flow, const float* __restrict__ hr_prev, uint4* __restrict__ out, int n,
                                                            int h, int w) {
  const size_t hw = (size_t)h * w, npix = (size_t)n * hw;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / hw;
    warp_s2d_bi_pixel<T>(lr_flow, hr_prev + img * 3 * (16 * hw), out, i, img, npix, h, w);
  }
}
// ... with every item's hr_prev where its stream keeps it (FrvsrPtrs by value, as k_warp_s2d_planes_items)
template <typename T>
__global__ __launch_bounds__(256) void k_warp_s2d_bi_planes_items(const float* __restrict__ lr_flow, FrvsrPtrs hr_prev, uint4* __restrict__ out, int n, int h,
                                                                  int w) {
  const size_t hw = (size_t)h * w, npix = (size_t)n * hw;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / hw;
    warp_s2d_bi_pixel<T>(lr_flow, hr_prev.p[img], out, i, img, npix, h, w);
  }
}
template <typename T>
void op_warp_s2d_bi_planes(const float* lr_flow, const float* hr_prev, T* out, int n, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull, "warp (bilinear): sizes");
  SS4K_GLUE_ROUTE(sizeof(T) == 2 ? "frvsr_bi::warp_s2d_bi_planes<half>" : "frvsr_bi::warp_s2d_bi_planes<float>");
  hipLaunchKernelGGL((k_warp_s2d_bi_planes<T>), grid_for((size_t)n * h * w), dim3(256), 0, st, lr_flow, hr_prev, reinterpret_cast<uint4*>(out), n, h, w);
  SS4K_LAUNCH_OK();
}
template void op_warp_s2d_bi_planes<float>(const float*, const float*, float*, int, int, int, hipStream_t);
template void op_warp_s2d_bi_planes<__half>(const float*, const float*, __half*, int, int, int, hipStream_t);
template <typename T>
void op_warp_s2d_bi_planes_items(const float* lr_flow, const FrvsrPtrs& hr_prev, T* out, int n, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull, "warp (bilinear, items): sizes");
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(hr_prev.p[i], "warp (bilinear, items): NULL item");
  SS4K_GLUE_ROUTE(sizeof(T) == 2 ? "frvsr_bi::warp_s2d_bi_planes_items<half>" : "frvsr_bi::warp_s2d_bi_planes_items<float>");
  hipLaunchKernelGGL((k_warp_s2d_bi_planes_items<T>), grid_for((size_t)n * h * w), dim3(256), 0, st, lr_flow, hr_prev, reinterpret_cast<uint4*>(out), n, h, w);
  SS4K_LAUNCH_OK();
}
template void op_warp_s2d_bi_planes_items<float>(const float*, const FrvsrPtrs&, float*, int, int, int, hipStream_t);
template void op_warp_s2d_bi_planes_items<__half>(const float*, const FrvsrPtrs&, __half*, int, int, int, hipStream_t);

// ------------------------------------------------------------------ conv_out + bilinear x4 (lr_curr) -> fp32 NCHW (TecoGAN's tail, 'BI')
// One thread per HR value.  The skip is bil4_load / bil4_at, as k_bilinear_upsample4 calls them: that op's value bit for bit,
// then ONE rounded add
__device__ __forceinline__ float bil4_add_value(const float* __restrict__ lr_plane, float conv, int X, int Y, int h, int w) {
  float f[3][3];
  bil4_load(lr_plane, Y >> 2, X >> 2, h, w, f);
  return __fadd_rn(conv, bil4_at(f, Y & 3, X & 3, Y >> 2, X >> 2, h, w));
}
__global__ __launch_bounds__(256) void k_bilinear4_add(const float* __restrict__ conv, const float* __restrict__ lr, float* __restrict__ out, int planes, int h,
                                                       int w) {
  const int OW = 4 * w, OH = 4 * h;
  const size_t total = (size_t)planes * OH * OW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % OW), Y = (int)((i / OW) % OH);
    const size_t pl = i / ((size_t)OW * OH);
    out[i] = bil4_add_value(lr + pl * h * w, conv[i], X, Y, h, w);
  }
}
// ... item (pl / 3) reading lr.p[item] and writing out.p[item] (FrvsrPtrs by value); conv stays one batch
__global__ __launch_bounds__(256) void k_bilinear4_add_items(const float* __restrict__ conv, FrvsrPtrs lr, FrvsrPtrs out, int planes, int h, int w) {
  const int OW = 4 * w, OH = 4 * h;
  const size_t HW = (size_t)OW * OH, total = (size_t)planes * HW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % OW), Y = (int)((i / OW) % OH);
    const size_t pl = i / HW, item = pl / 3, c = pl - item * 3;
    out.p[item][c * HW + (i - pl * HW)] = bil4_add_value(lr.p[item] + c * h * w, conv[i], X, Y, h, w);
  }
}
void op_bilinear4_add(const float* conv, const float* lr, float* out, int n, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull / 16, "bilinear4_add: sizes");
  SS4K_GLUE_ROUTE("frvsr_bi::bilinear4_add");
  hipLaunchKernelGGL(k_bilinear4_add, grid_for((size_t)n * 3 * 16 * h * w), dim3(256), 0, st, conv, lr, out, 3 * n, h, w);
  SS4K_LAUNCH_OK();
}
void op_bilinear4_add_items(const float* conv, const FrvsrPtrs& lr, const FrvsrPtrs& out, int n, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull / 16, "bilinear4_add (items): sizes");
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(lr.p[i] && out.p[i], "bilinear4_add (items): NULL item");
  SS4K_GLUE_ROUTE("frvsr_bi::bilinear4_add_items");
  hipLaunchKernelGGL(k_bilinear4_add_items, grid_for((size_t)n * 3 * 16 * h * w), dim3(256), 0, st, conv, lr, out, 3 * n, h, w);
  SS4K_LAUNCH_OK();
}

}  // namespace ss4k
