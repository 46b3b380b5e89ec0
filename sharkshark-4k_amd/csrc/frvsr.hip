// Glue kernels of the frame-recurrent upscaler (EGVSR's FRNet x4, reference src/upscale/model/egvsr/egvsr.py): everything of
// FRNet.forward that is not a 3x3 convolution.  The convolutions run on the conv kernels through Model::conv (frvsr.cpp).
// "planes" tensors: [plane][pixel (n, y, x)][16 channels of T], T = __half (32-byte records) or float (64-byte records).
// The flow, hr_prev and hr_curr are fp32 in both dtypes.
//
// The four stages that exist per (degradation, addressing) - the x4, flow x4 + warp + space-to-depth, conv_out + x4 skip, EGVSR's tail - are
// one kernel template and one launch helper each (frvsr_stages.h); this file holds the bicubic up-sampler (degradation 'BD') and the
// launchers that instantiate them with it, frvsr_bi.hip the bilinear one.  The x4 and the warp exist as granular ops
// (ss4k_op_bicubic_upsample4, ss4k_op_backward_warp) and inside the fused kernels, and every one goes through the SAME device functions, so
// the fused kernel's tensor is bit-identical to the chain of the granular ops (tests/test_gpu_frvsr.py).
#include "frvsr_stages.h"

namespace ss4k {

// one 16-byte slot of a record as E values of T
template <typename T> struct Slot {
  static constexpr int E = 16 / sizeof(T);
  union { uint4 u; T v[E]; };
  __device__ __forceinline__ Slot() : u(make_uint4(0, 0, 0, 0)) {}
};

// ------------------------------------------------------------------ MaxPool2d(2, 2) on planes
template <typename T>
__global__ void k_maxpool2_planes(const uint4* __restrict__ in, uint4* __restrict__ out, int nplanes, int n, int h, int w) {
  constexpr int RV = sizeof(T);   // 16-byte slots per record: 16 channels * sizeof(T) / 16
  const int oh = h / 2, ow = w / 2;
  const size_t ipx = (size_t)n * h * w, opx = (size_t)n * oh * ow, total = (size_t)nplanes * opx * RV;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int slot = (int)(i % RV);
    const size_t q = i / RV, pix = q % opx, plane = q / opx;
    const int ox = (int)(pix % ow), oy = (int)((pix / ow) % oh);
    const size_t img = pix / ((size_t)ow * oh);
    const size_t base = plane * ipx + (img * h + 2 * (size_t)oy) * w + 2 * (size_t)ox;
    Slot<T> a, b, c, d, r;
    a.u = in[base * RV + slot]; b.u = in[(base + 1) * RV + slot];
    c.u = in[(base + w) * RV + slot]; d.u = in[(base + w + 1) * RV + slot];
#pragma unroll
    for (int e = 0; e < Slot<T>::E; ++e)
      r.v[e] = (T)fmaxf(fmaxf((float)a.v[e], (float)b.v[e]), fmaxf((float)c.v[e], (float)d.v[e]));
    out[i] = r.u;   // i == ((plane * opx + pix) * RV + slot)
  }
}
template <typename T>
void op_maxpool2_planes(const T* in, T* out, int nplanes, int n, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(nplanes > 0 && n > 0 && h >= 2 && w >= 2, "maxpool2: needs at least 2 x 2 pixels");
  const size_t total = (size_t)nplanes * n * (h / 2) * (w / 2) * sizeof(T);
  SS4K_GLUE_ROUTE(sizeof(T) == 2 ? "frvsr::maxpool2_planes<half>" : "frvsr::maxpool2_planes<float>");
  hipLaunchKernelGGL((k_maxpool2_planes<T>), grid_for(total), dim3(256), 0, st, reinterpret_cast<const uint4*>(in), reinterpret_cast<uint4*>(out),
                     nplanes, n, h, w);
  SS4K_LAUNCH_OK();
}
template void op_maxpool2_planes<float>(const float*, float*, int, int, int, int, hipStream_t);
template void op_maxpool2_planes<__half>(const __half*, __half*, int, int, int, int, hipStream_t);

// ------------------------------------------------------------------ bilinear x2 (align_corners=False) on planes
// source index of ATen's upsample_bilinear2d for scale_factor = 2: src = max(0.5 (dst + 0.5) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, size - 1)
__device__ __forceinline__ void bil2_src(int dst, int size, int& i0, int& i1, float& l0, float& l1) {
  const float s = fmaxf(0.5f * ((float)dst + 0.5f) - 0.5f, 0.f);
  i0 = min((int)s, size - 1); i1 = min(i0 + 1, size - 1);
  l1 = s - (float)i0; l0 = 1.f - l1;
}
template <typename T>
__global__ void k_bilinear2_planes(const uint4* __restrict__ in, uint4* __restrict__ out, int nplanes, int n, int h, int w) {
  constexpr int RV = sizeof(T);
  const int oh = 2 * h, ow = 2 * w;
  const size_t ipx = (size_t)n * h * w, opx = (size_t)n * oh * ow, total = (size_t)nplanes * opx * RV;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int slot = (int)(i % RV);
    const size_t q = i / RV, pix = q % opx, plane = q / opx;
    const int ox = (int)(pix % ow), oy = (int)((pix / ow) % oh);
    const size_t img = pix / ((size_t)ow * oh);
    int y0, y1, x0, x1; float wy0, wy1, wx0, wx1;
    bil2_src(oy, h, y0, y1, wy0, wy1); bil2_src(ox, w, x0, x1, wx0, wx1);
    const size_t r0 = plane * ipx + (img * h + y0) * w, r1 = plane * ipx + (img * h + y1) * w;
    Slot<T> a, b, c, d, r;
    a.u = in[(r0 + x0) * RV + slot]; b.u = in[(r0 + x1) * RV + slot];
    c.u = in[(r1 + x0) * RV + slot]; d.u = in[(r1 + x1) * RV + slot];
#pragma unroll
    for (int e = 0; e < Slot<T>::E; ++e)
      r.v[e] = (T)(wy0 * (wx0 * (float)a.v[e] + wx1 * (float)b.v[e]) + wy1 * (wx0 * (float)c.v[e] + wx1 * (float)d.v[e]));
    out[i] = r.u;
  }
}
template <typename T>
void op_bilinear2_planes(const T* in, T* out, int nplanes, int n, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(nplanes > 0 && n > 0 && h > 0 && w > 0, "bilinear x2: empty tensor");
  const size_t total = (size_t)nplanes * n * (2 * h) * (2 * w) * sizeof(T);
  SS4K_GLUE_ROUTE(sizeof(T) == 2 ? "frvsr::bilinear2_planes<half>" : "frvsr::bilinear2_planes<float>");
  hipLaunchKernelGGL((k_bilinear2_planes<T>), grid_for(total), dim3(256), 0, st, reinterpret_cast<const uint4*>(in), reinterpret_cast<uint4*>(out),
                     nplanes, n, h, w);
  SS4K_LAUNCH_OK();
}
template void op_bilinear2_planes<float>(const float*, float*, int, int, int, int, hipStream_t);
template void op_bilinear2_planes<__half>(const __half*, __half*, int, int, int, int, hipStream_t);

// ------------------------------------------------------------------ tanh * 24, reflect pad on the right and at the bottom
__global__ void k_flow_finish(const float* __restrict__ raw, float* __restrict__ flow, int n, int h8, int w8, int h, int w) {
  const size_t total = (size_t)n * 2 * h * w;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % w), y = (int)((i / w) % h);
    const size_t pl = i / ((size_t)w * h);
    const int sx = x < w8 ? x : 2 * (w8 - 1) - x, sy = y < h8 ? y : 2 * (h8 - 1) - y;   // pad <= 7 <= size - 1: inside
    flow[i] = tanhf(raw[(pl * h8 + sy) * w8 + sx]) * 24.f;
  }
}
void op_flow_finish(const float* raw, float* flow, int n, int h8, int w8, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && h8 >= 8 && w8 >= 8 && h >= h8 && w >= w8 && h - h8 < 8 && w - w8 < 8, "flow pad: sizes");
  SS4K_GLUE_ROUTE("frvsr::flow_finish");
  hipLaunchKernelGGL(k_flow_finish, grid_for((size_t)n * 2 * h * w), dim3(256), 0, st, raw, flow, n, h8, w8, h, w);
  SS4K_LAUNCH_OK();
}

// ------------------------------------------------------------------ BicubicUpsample(4)
// kernels[d] = cubic . (1, s, s^2, s^3), s = d / 4, a = -0.75 (net_utils.py:126-140): tap i of phase d weighs input clamp(base - 1 + i)
struct Bic4 { float k[4][4]; };
static Bic4 bic4_taps() {
  Bic4 t;
  const float a = -0.75f;
  const float cubic[4][4] = {{0, a, -2 * a, a}, {1, 0, -(a + 3), a + 2}, {0, -a, (2 * a + 3), -(a + 2)}, {0, 0, a, -a}};
  for (int d = 0; d < 4; ++d) {
    const float s = 1.0f * d / 4, p[4] = {1.f, s, s * s, s * s * s};
    for (int i = 0; i < 4; ++i) {
      float acc = 0.f;
      for (int j = 0; j < 4; ++j) acc += cubic[i][j] * p[j];
      t.k[d][i] = acc;
    }
  }
  return t;
}
__device__ __forceinline__ float bic4_dot(const float k[4], float a, float b, float c, float d) {
  return __fmaf_rn(k[3], d, __fmaf_rn(k[2], c, __fmaf_rn(k[1], b, __fmul_rn(k[0], a))));
}
// 4 x 4 neighbourhood of (y, x) with replicate padding (1, 2, 1, 2): rows clamp(y - 1 .. y + 2), columns clamp(x - 1 .. x + 2)
__device__ __forceinline__ void bic4_load(const float* __restrict__ pl, int y, int x, int h, int w, float f[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int yy = min(max(y - 1 + i, 0), h - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[i][j] = pl[(size_t)yy * w + min(max(x - 1 + j, 0), w - 1)];
  }
}
// output (4 y + sy, 4 x + sx): the height pass first, then the width pass (net_utils.py:153-163)
__device__ __forceinline__ float bic4_at(const Bic4& t, const float f[4][4], int sy, int sx) {
  float col[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) col[j] = bic4_dot(t.k[sy], f[0][j], f[1][j], f[2][j], f[3][j]);
  return bic4_dot(t.k[sx], col[0], col[1], col[2], col[3]);
}
// the up-sampler of frvsr_stages.h's kernels: the taps travel by value in the kernel arguments
struct UpBicubic4 {
  static constexpr int N = 4;
  Bic4 taps;
  __device__ __forceinline__ void load(const float* __restrict__ pl, int y, int x, int h, int w, float f[4][4]) const { bic4_load(pl, y, x, h, w, f); }
  __device__ __forceinline__ float at(const float f[4][4], int sy, int sx, int, int, int, int) const { return bic4_at(taps, f, sy, sx); }
};
void op_bicubic_upsample4(const float* in, float* out, int planes, int h, int w, hipStream_t st) {
  launch_up4("frvsr::bicubic_upsample4", "bicubic x4", in, out, planes, h, w, UpBicubic4{bic4_taps()}, st);
}

// ------------------------------------------------------------------ backward_warp, the granular op (warp_pos, warp_taps, warp_sample: frvsr_stages.h)
__global__ void k_backward_warp(const float* __restrict__ x, const float* __restrict__ flow, float* __restrict__ out, int n, int c, int h, int w) {
  const size_t hw = (size_t)h * w, total = (size_t)n * hw;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % w), Y = (int)((i / w) % h);
    const size_t img = i / hw, p = i - img * hw;
    const WarpTaps t = warp_taps(X, Y, w, h, flow[(img * 2) * hw + p], flow[(img * 2 + 1) * hw + p]);
    for (int k = 0; k < c; ++k) out[(img * c + k) * hw + p] = warp_sample(x + (img * c + k) * hw, w, t);
  }
}
void op_backward_warp(const float* x, const float* flow, float* out, int n, int c, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && c > 0 && h >= 2 && w >= 2, "backward_warp: needs at least 2 x 2 pixels");
  SS4K_GLUE_ROUTE("frvsr::backward_warp");
  hipLaunchKernelGGL(k_backward_warp, grid_for((size_t)n * h * w), dim3(256), 0, st, x, flow, out, n, c, h, w);
  SS4K_LAUNCH_OK();
}

// ------------------------------------------------------------------ the stage kernels of frvsr_stages.h with the bicubic x4
template <typename T>
void op_warp_s2d_planes(const float* lr_flow, const float* hr_prev, T* out, int n, int h, int w, hipStream_t st) {
  launch_warp_s2d(sizeof(T) == 2 ? "frvsr::warp_s2d_planes<half>" : "frvsr::warp_s2d_planes<float>", "warp", lr_flow, Strided<const float>{hr_prev, (size_t)48 * h * w},
                  out, n, h, w, UpBicubic4{bic4_taps()}, st);
}
template void op_warp_s2d_planes<float>(const float*, const float*, float*, int, int, int, hipStream_t);
template void op_warp_s2d_planes<__half>(const float*, const float*, __half*, int, int, int, hipStream_t);
template <typename T>
void op_warp_s2d_planes_items(const float* lr_flow, const FrvsrPtrs& hr_prev, T* out, int n, int h, int w, hipStream_t st) {
  launch_warp_s2d(sizeof(T) == 2 ? "frvsr::warp_s2d_planes_items<half>" : "frvsr::warp_s2d_planes_items<float>", "warp (items)", lr_flow, Table{hr_prev}, out, n, h, w,
                  UpBicubic4{bic4_taps()}, st);
}
template void op_warp_s2d_planes_items<float>(const float*, const FrvsrPtrs&, float*, int, int, int, hipStream_t);
template void op_warp_s2d_planes_items<__half>(const float*, const FrvsrPtrs&, __half*, int, int, int, hipStream_t);

template <typename T>
void op_ps4_conv_tail(const T* in, const float* wb, float* out, int n, int h, int w, hipStream_t st) {
  launch_ps4_conv_tail(sizeof(T) == 2 ? "frvsr::ps4_conv_tail<half>" : "frvsr::ps4_conv_tail<float>", "tail",
                       in, wb, Strided<float>{out, (size_t)48 * h * w}, n, h, w, st);
}
template void op_ps4_conv_tail<float>(const float*, const float*, float*, int, int, int, hipStream_t);
template void op_ps4_conv_tail<__half>(const __half*, const float*, float*, int, int, int, hipStream_t);
template <typename T>
void op_ps4_conv_tail_items(const T* in, const float* wb, const FrvsrPtrs& out, int n, int h, int w, hipStream_t st) {
  launch_ps4_conv_tail(sizeof(T) == 2 ? "frvsr::ps4_conv_tail_items<half>" : "frvsr::ps4_conv_tail_items<float>", "tail (items)", in, wb, Table{out}, n, h, w, st);
}
template void op_ps4_conv_tail_items<float>(const float*, const float*, const FrvsrPtrs&, int, int, int, hipStream_t);
template void op_ps4_conv_tail_items<__half>(const __half*, const float*, const FrvsrPtrs&, int, int, int, hipStream_t);

// (the tail of the second generator: bounded by tests/test_gpu_tecogan*.py)
void op_bicubic4_add(const float* conv, const float* lr, float* out, int n, int h, int w, hipStream_t st) {
  launch_x4_add("frvsr_teco::bicubic4_add", "bicubic4_add", conv, Strided<const float>{lr, (size_t)3 * h * w}, Strided<float>{out, (size_t)48 * h * w}, n, h, w,
                UpBicubic4{bic4_taps()}, st);
}
void op_bicubic4_add_items(const float* conv, const FrvsrPtrs& lr, const FrvsrPtrs& out, int n, int h, int w, hipStream_t st) {
  launch_x4_add("frvsr_teco::bicubic4_add_items", "bicubic4_add (items)", conv, Table{lr}, Table{out}, n, h, w, UpBicubic4{bic4_taps()}, st);
}

// ------------------------------------------------------------------ planes -> fp32 NCHW (parity taps), clamp into another tensor
template <typename T>
__global__ void k_planes_to_nchw(const T* __restrict__ in, float* __restrict__ out, int n, int channels, int h, int w) {
  const size_t hw = (size_t)h * w, npix = (size_t)n * hw, total = npix * channels;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i % hw, k = (i / hw) % channels, img = i / (hw * channels);
    out[i] = (float)in[((k / 16) * npix + img * hw + p) * 16 + (k % 16)];
  }
}
template <typename T>
void op_planes_to_nchw(const T* in, float* out, int n, int channels, int h, int w, hipStream_t st) {
  SS4K_GLUE_ROUTE(sizeof(T) == 2 ? "frvsr::planes_to_nchw<half>" : "frvsr::planes_to_nchw<float>");
  hipLaunchKernelGGL((k_planes_to_nchw<T>), grid_for((size_t)n * channels * h * w), dim3(256), 0, st, in, out, n, channels, h, w);
  SS4K_LAUNCH_OK();
}
template void op_planes_to_nchw<float>(const float*, float*, int, int, int, int, hipStream_t);
template void op_planes_to_nchw<__half>(const __half*, float*, int, int, int, int, hipStream_t);

__global__ void k_clamp01_to(const float* __restrict__ in, float* __restrict__ out, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = fminf(fmaxf(in[i], 0.f), 1.f);
}
void op_clamp01_to(const float* in, float* out, size_t n, hipStream_t st) {
  SS4K_GLUE_ROUTE("frvsr::clamp01_to");
  hipLaunchKernelGGL(k_clamp01_to, grid_for(n), dim3(256), 0, st, in, out, n);
  SS4K_LAUNCH_OK();
}

// ------------------------------------------------------------------ the glue of a scattered round (FrvsrUpscaler::round_at)
// Three launches for the whole round, each item's frame read and written where it lies (pointer tables by value, as FrvsrPtrs).  They restate
// the arithmetic of the per-item chains of FrvsrUpscaler::round - k_u8nhwc_to_f32nchw, k_area / k_area_whole<4|8> / the identity copy, k_clamp01_to,
// k_f32nchw_to_u8nhwc, k_pack_input<T, 1> (glue.hip) - expression for expression: the bytes and the state are bit-identical
// (tests/test_gpu_frvsr_scattered.py).  Every area route sums its window rows outer, columns inner from 0.f and divides by the row count, then by
// the column count; a whole-number window of the float bounds below is the window k_area_whole takes, so one loop stands for all of them.
// window bounds of adaptive average pooling: glue.hip's a_start / a_end, the float formula
__device__ __forceinline__ int area_lo(int i, int in, int out) { return (int)floorf((float)(i * in) / out); }
__device__ __forceinline__ int area_hi(int i, int in, int out) { return (int)ceilf((float)((i + 1) * in) / out); }

__global__ __launch_bounds__(256) void k_frames_in_items(FrvsrFramesIn in, FrvsrPtrs lr_curr, int n, int h, int w, int lh, int lw) {
  const size_t lhw = (size_t)lh * lw, total = (size_t)n * lhw;
  const bool resize = h != lh || w != lw;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / lhw, p = i - img * lhw;
    const uint8_t* __restrict__ src = in.p[img];
    float* __restrict__ dst = lr_curr.p[img] + p;
    if (!resize) {
#pragma unroll
      for (int k = 0; k < 3; ++k) dst[k * lhw] = (float)src[p * 3 + k] / 255.0f;
      continue;
    }
    const int oy = (int)(p / lw), ox = (int)(p - (size_t)oy * lw);
    const int y0 = area_lo(oy, h, lh), y1 = area_hi(oy, h, lh), x0 = area_lo(ox, w, lw), x1 = area_hi(ox, w, lw);
    float sum[3] = {0.f, 0.f, 0.f};
    for (int y = y0; y < y1; ++y) {
      const uint8_t* row = src + ((size_t)y * w + x0) * 3;
      for (int x = 0; x < x1 - x0; ++x) {
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] += (float)row[3 * x + k] / 255.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k * lhw] = sum[k] / (float)(y1 - y0) / (float)(x1 - x0);
  }
}
void op_frames_in_items(const FrvsrFramesIn& in, const FrvsrPtrs& lr_curr, int n, int h, int w, int lh, int lw, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && h > 0 && w > 0 && lh > 0 && lw > 0, "frames in (items): sizes");
  SS4K_REQUIRE((double)h * lh < 2147483648.0 && (double)w * lw < 2147483648.0, "frames in (items): a window bound would overflow");
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(in.p[i] && lr_curr.p[i], "frames in (items): NULL item");
  SS4K_GLUE_ROUTE(h != lh || w != lw ? "frvsr::frames_in_items<area>" : "frvsr::frames_in_items");
  hipLaunchKernelGGL(k_frames_in_items, grid_for((size_t)n * lh * lw), dim3(256), 0, st, in, lr_curr, n, h, w, lh, lw);
  SS4K_LAUNCH_OK();
}

template <typename T>
__global__ __launch_bounds__(256) void k_pack_lr_items(FrvsrPtrs lr_curr, FrvsrPtrs lr_prev, uint4* __restrict__ a, uint4* __restrict__ b, int n, int h, int w) {
  constexpr int RV = sizeof(T);   // 16-byte slots per 16-channel record
  const size_t hw = (size_t)h * w, total = (size_t)n * hw;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / hw, p = i - img * hw;
    const float* __restrict__ c = lr_curr.p[img] + p;
    const float* __restrict__ q = lr_prev.p[img] + p;
    union { T v[16]; uint4 u[RV]; } ra, rb;
#pragma unroll
    for (int k = 0; k < 16; ++k) { ra.v[k] = (T)(k < 3 ? c[k * hw] : 0.f); rb.v[k] = (T)(k < 3 ? q[k * hw] : 0.f); }
#pragma unroll
    for (int s = 0; s < RV; ++s) { a[i * RV + s] = ra.u[s]; b[i * RV + s] = rb.u[s]; }
  }
}
template <typename T>
void op_pack_lr_items(const FrvsrPtrs& lr_curr, const FrvsrPtrs& lr_prev, T* a, T* b, int n, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && h > 0 && w > 0 && a && b, "pack (items): sizes");
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(lr_curr.p[i] && lr_prev.p[i], "pack (items): NULL item");
  SS4K_GLUE_ROUTE(sizeof(T) == 2 ? "frvsr::pack_lr_items<half>" : "frvsr::pack_lr_items<float>");
  hipLaunchKernelGGL((k_pack_lr_items<T>), grid_for((size_t)n * h * w), dim3(256), 0, st, lr_curr, lr_prev, reinterpret_cast<uint4*>(a), reinterpret_cast<uint4*>(b),
                     n, h, w);
  SS4K_LAUNCH_OK();
}
template void op_pack_lr_items<float>(const FrvsrPtrs&, const FrvsrPtrs&, float*, float*, int, int, int, hipStream_t);
template void op_pack_lr_items<__half>(const FrvsrPtrs&, const FrvsrPtrs&, __half*, __half*, int, int, int, hipStream_t);

// One thread per FOUR consecutive output pixels of a frame taken as a flat run of oh * ow pixels (a group may straddle two rows): twelve bytes,
// three 4-byte stores where the frame starts on a 4-byte boundary (k_tail_fused4's packing), twelve 1-byte stores otherwise and in the
// frame's last, partial group.  RESIZE: each pixel is the mean of its window of CLAMPED values (k_clamp01_to, then k_area).
__device__ __forceinline__ uint32_t u8_of(float v) { return (uint32_t)(uint8_t)(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }
template <bool RESIZE>
__global__ __launch_bounds__(256) void k_frames_out_items(FrvsrPtrs hr, FrvsrFramesOut out, int n, int H, int W, int oh, int ow) {
  const size_t HW = (size_t)H * W, opx = (size_t)oh * ow, groups = (opx + 3) / 4, total = (size_t)n * groups;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / groups, p0 = (i - img * groups) * 4;
    const float* __restrict__ src = hr.p[img];
    uint8_t* __restrict__ dst = out.p[img] + p0 * 3;
    const int cnt = (int)(opx - p0 < 4 ? opx - p0 : 4);
    uint32_t b[4][3] = {};
    if constexpr (!RESIZE) {
      if (cnt == 4 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {   // (HW = 16 lr_h lr_w: the planes lie a multiple of 16 bytes apart)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float4 v = *reinterpret_cast<const float4*>(src + k * HW + p0);
          b[0][k] = u8_of(v.x); b[1][k] = u8_of(v.y); b[2][k] = u8_of(v.z); b[3][k] = u8_of(v.w);
        }
      } else {
        for (int j = 0; j < cnt; ++j)
#pragma unroll
          for (int k = 0; k < 3; ++k) b[j][k] = u8_of(src[k * HW + p0 + j]);
      }
    } else {
      for (int j = 0; j < cnt; ++j) {
        const size_t p = p0 + j;
        const int oy = (int)(p / ow), ox = (int)(p - (size_t)oy * ow);
        const int y0 = area_lo(oy, H, oh), y1 = area_hi(oy, H, oh), x0 = area_lo(ox, W, ow), x1 = area_hi(ox, W, ow);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float* pl = src + k * HW;
          float sum = 0.f;
          for (int y = y0; y < y1; ++y)
            for (int x = x0; x < x1; ++x) sum += fminf(fmaxf(pl[(size_t)y * W + x], 0.f), 1.f);
          b[j][k] = u8_of(sum / (float)(y1 - y0) / (float)(x1 - x0));
        }
      }
    }
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
      uint32_t wds[3] = {0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) { const int byte = 3 * j + k; wds[byte >> 2] |= b[j][k] << (8 * (byte & 3)); }
      uint32_t* o = reinterpret_cast<uint32_t*>(dst);
      o[0] = wds[0]; o[1] = wds[1]; o[2] = wds[2];
    } else {
      for (int j = 0; j < cnt; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) dst[3 * j + k] = (uint8_t)b[j][k];
    }
  }
}
void op_frames_out_items(const FrvsrPtrs& hr, const FrvsrFramesOut& out, int n, int H, int W, int oh, int ow, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && H > 0 && W > 0 && oh > 0 && ow > 0, "frames out (items): sizes");
  SS4K_REQUIRE((double)H * oh < 2147483648.0 && (double)W * ow < 2147483648.0, "frames out (items): a window bound would overflow");
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(hr.p[i] && out.p[i], "frames out (items): NULL item");
  const dim3 g = grid_for((size_t)n * (((size_t)oh * ow + 3) / 4));
  if (H != oh || W != ow) {
    SS4K_GLUE_ROUTE("frvsr::frames_out_items<area>");
    hipLaunchKernelGGL(k_frames_out_items<true>, g, dim3(256), 0, st, hr, out, n, H, W, oh, ow);
  } else {
    SS4K_GLUE_ROUTE("frvsr::frames_out_items");
    hipLaunchKernelGGL(k_frames_out_items<false>, g, dim3(256), 0, st, hr, out, n, H, W, oh, ow);
  }
  SS4K_LAUNCH_OK();
}

}  // namespace ss4k
