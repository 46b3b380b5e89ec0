// The stages of a frame-recurrent step that exist for every (generator, degradation, addressing) combination, each as ONE kernel template
// and one launch helper: the x4 up-sampling (k_up4), flow x4 + warp + space-to-depth (k_warp_s2d), TecoGAN's conv_out + x4 skip (k_x4_add)
// and EGVSR's PixelShuffle(4) + ReLU + conv tail (k_ps4_conv_tail).  They are parametrised by two small families of types:
//   * where item i's tensor lies: Strided (one contiguous batch, base + i * stride) or Table (FrvsrPtrs, p[i]);
//   * the x4 up-sampler: UpBicubic4 (frvsr.hip, degradation 'BD') or UpBilinear4 (frvsr_bi.hip, degradation 'BI').
// frvsr.hip and frvsr_bi.hip hold the up-samplers and the launchers, which name an instantiation, a route and a refusal prefix each.
// The device functions are written with explicit __fmaf_rn / __fmul_rn / __fadd_rn so that the compiler contracts nothing differently in any
// of the kernels that call them: a fused kernel's tensor is bit-identical to the chain of the granular ops.  Included by .hip files only.
#pragma once
#include "frvsr.h"
#include <climits>

namespace ss4k {

#define SS4K_LAUNCH_OK() SS4K_HIP(hipGetLastError())

static inline dim3 grid_for(size_t n, int block = 256) {
  size_t g = (n + block - 1) / block;
  if (g > 256 * 8 * 4) g = 256 * 8 * 4;   // grid-stride beyond a few waves per CU
  return dim3((unsigned)std::max<size_t>(g, 1));
}

// ------------------------------------------------------------------ where item i's tensor lies
// One contiguous batch: any number of items.  F: float, or const float for a tensor the kernel only reads
template <typename F> struct Strided {
  F* base; size_t stride;
  static constexpr int MAX_ITEMS = INT_MAX;
  __host__ __device__ F* at(size_t i) const { return base + i * stride; }
  // plane pl = i * 3 + c of items of three planes of e elements (stride == 3 e): the planes of a batch follow each other
  __host__ __device__ F* plane(size_t pl, size_t e) const { return base + pl * e; }
  bool complete(int) const { return true; }
};
// Every item where its stream keeps it: the base pointers travel BY VALUE in the kernel arguments (FrvsrPtrs, frvsr.h)
struct Table {
  FrvsrPtrs t;
  static constexpr int MAX_ITEMS = SS4K_FRVSR_MAX_STREAMS;
  __host__ __device__ float* at(size_t i) const { return t.p[i]; }
  __host__ __device__ float* plane(size_t pl, size_t e) const { const size_t item = pl / 3; return t.p[item] + (pl - item * 3) * e; }
  bool complete(int n) const {
    for (int i = 0; i < n; ++i) if (!t.p[i]) return false;
    return true;
  }
};

// A launch helper below is inlined into its launcher, so that the product build, which compiles SS4K_GLUE_ROUTE away, keeps no route name
#define SS4K_STAGE_LAUNCH __attribute__((always_inline)) static inline void
// what: the launcher's prefix of its refusals ("warp (items)": "warp (items): sizes", "warp (items): NULL item")
#define SS4K_STAGE_REQUIRE(cond, what, text) SS4K_REQUIRE(cond, std::string(what) + ": " text)

// ------------------------------------------------------------------ the x4 up-sampling: (planes, h, w) -> (planes, 4 h, 4 w), fp32
// An up-sampler Up has the size N of its neighbourhood, load(plane, y, x, h, w, f) of input pixel (y, x)'s N x N neighbourhood and
// at(f, sy, sx, y, x, h, w), output (4 y + sy, 4 x + sx).  One thread per output value
template <typename Up>
__global__ __launch_bounds__(256) void k_up4(const float* __restrict__ in, float* __restrict__ out, int planes, int h, int w, Up up) {
  const int OW = 4 * w, OH = 4 * h;
  const size_t total = (size_t)planes * OH * OW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % OW), Y = (int)((i / OW) % OH);
    const size_t pl = i / ((size_t)OW * OH);
    float f[Up::N][Up::N];
    up.load(in + pl * h * w, Y >> 2, X >> 2, h, w, f);
    out[i] = up.at(f, Y & 3, X & 3, Y >> 2, X >> 2, h, w);
  }
}
template <typename Up>
SS4K_STAGE_LAUNCH launch_up4(const char* route, const char* what, const float* in, float* out, int planes, int h, int w, const Up& up, hipStream_t st) {
  SS4K_STAGE_REQUIRE(planes > 0 && h > 0 && w > 0 && h <= (1 << 28) && w <= (1 << 28), what, "sizes");
  SS4K_GLUE_ROUTE(route);
  hipLaunchKernelGGL(k_up4<Up>, grid_for((size_t)planes * 16 * h * w), dim3(256), 0, st, in, out, planes, h, w, up);
  SS4K_LAUNCH_OK();
}

// ------------------------------------------------------------------ backward_warp's arithmetic
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

// ------------------------------------------------------------------ flow x4 + warp + space-to-depth -> three planes
// 4 * Up(lr_flow), backward_warp(hr_prev, .) and the space-to-depth of egvsr.py:196-208.  One thread per LR pixel: its N x N flow neighbourhood
// serves all 16 sub-pixels (the four phases of each pass read the same inputs), and the 48 channels (sy * 4 + sx) * 3 + c it produces are
// exactly the three records it stores, with 16-byte stores.
// pixel i of item img: `src` is that item's hr_prev (3, 4 h, 4 w).  A function of its own on purpose: with this body written into the kernel's
// loop, hipcc fused warp_sample's last multiply-add with the conversion to __half (v_fma_mixlo_f16, ONE rounding) in 16 of the 48 channels,
// and the __half planes were no longer backward_warp's fp32 value rounded to fp16 (tests/test_gpu_frvsr_glue_budget.py holds them to it)
template <typename T, typename Up>
__device__ __forceinline__ void warp_s2d_pixel(const float* __restrict__ lr_flow, const float* __restrict__ src, uint4* __restrict__ out, size_t i, size_t img,
                                               size_t npix, int h, int w, const Up& up) {
  const int H = 4 * h, W = 4 * w;
  const size_t hw = (size_t)h * w, HW = (size_t)H * W;
  const int x = (int)(i % w), y = (int)((i / w) % h);
  S2dRecord<T> rec;
  float fu[Up::N][Up::N], fv[Up::N][Up::N];
  up.load(lr_flow + (img * 2) * hw, y, x, h, w, fu);
  up.load(lr_flow + (img * 2 + 1) * hw, y, x, h, w, fv);
#pragma unroll
  for (int sy = 0; sy < 4; ++sy)
#pragma unroll
    for (int sx = 0; sx < 4; ++sx) {
      const float u = __fmul_rn(4.f, up.at(fu, sy, sx, y, x, h, w)), v = __fmul_rn(4.f, up.at(fv, sy, sx, y, x, h, w));
      const WarpTaps t = warp_taps(4 * x + sx, 4 * y + sy, W, H, u, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) rec.v[(sy * 4 + sx) * 3 + c] = (T)warp_sample(src + c * HW, W, t);
    }
  s2d_store<T>(rec, out, i, npix);
}
template <typename T, typename Up, typename Src>
__global__ __launch_bounds__(256) void k_warp_s2d(const float* __restrict__ lr_flow, Src hr_prev, uint4* __restrict__ out, int n, int h, int w, Up up) {
  const size_t hw = (size_t)h * w, npix = (size_t)n * hw;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / hw;
    warp_s2d_pixel<T>(lr_flow, hr_prev.at(img), out, i, img, npix, h, w, up);
  }
}
template <typename T, typename Up, typename Src>
SS4K_STAGE_LAUNCH launch_warp_s2d(const char* route, const char* what, const float* lr_flow, const Src& hr_prev, T* out, int n, int h, int w, const Up& up,
                                  hipStream_t st) {
  SS4K_STAGE_REQUIRE(n > 0 && n <= Src::MAX_ITEMS && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull, what, "sizes");
  SS4K_STAGE_REQUIRE(hr_prev.complete(n), what, "NULL item");
  SS4K_GLUE_ROUTE(route);
  hipLaunchKernelGGL((k_warp_s2d<T, Up, Src>), grid_for((size_t)n * h * w), dim3(256), 0, st, lr_flow, hr_prev, reinterpret_cast<uint4*>(out), n, h, w, up);
  SS4K_LAUNCH_OK();
}

// ------------------------------------------------------------------ conv_out + Up(lr_curr) -> fp32 NCHW (TecoGAN's tail)
// One thread per HR value of plane pl = item * 3 + c.  The skip is Up's load / at, as k_up4 calls them: that op's value bit for bit, then ONE
// rounded add.  lr: items of (3, h, w); out: items of (3, 4 h, 4 w); conv is one contiguous batch in either addressing
template <typename Up, typename Lr, typename Out>
__global__ __launch_bounds__(256) void k_x4_add(const float* __restrict__ conv, Lr lr, Out out, int planes, int h, int w, Up up) {
  const int OW = 4 * w, OH = 4 * h;
  const size_t HW = (size_t)OW * OH, total = (size_t)planes * HW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % OW), Y = (int)((i / OW) % OH);
    const size_t pl = i / HW;
    float f[Up::N][Up::N];
    up.load(lr.plane(pl, (size_t)h * w), Y >> 2, X >> 2, h, w, f);
    out.plane(pl, HW)[i - pl * HW] = __fadd_rn(conv[i], up.at(f, Y & 3, X & 3, Y >> 2, X >> 2, h, w));
  }
}
template <typename Up, typename Lr, typename Out>
SS4K_STAGE_LAUNCH launch_x4_add(const char* route, const char* what, const float* conv, const Lr& lr, const Out& out, int n, int h, int w, const Up& up,
                                hipStream_t st) {
  SS4K_STAGE_REQUIRE(n > 0 && n <= Out::MAX_ITEMS && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull / 16, what, "sizes");
  SS4K_STAGE_REQUIRE(lr.complete(n) && out.complete(n), what, "NULL item");
  SS4K_GLUE_ROUTE(route);
  hipLaunchKernelGGL((k_x4_add<Up, Lr, Out>), grid_for((size_t)n * 3 * 16 * h * w), dim3(256), 0, st, conv, lr, out, 3 * n, h, w, up);
  SS4K_LAUNCH_OK();
}

// ------------------------------------------------------------------ PixelShuffle(4) + ReLU + Conv2d(4, 3, 3, 1, 1) -> fp32 NCHW (EGVSR's tail)
// One thread per HR pixel.  Shuffled channel c of HR pixel (Y, X) is LR channel c * 16 + (Y % 4) * 4 + X % 4 of pixel (Y / 4, X / 4): element
// (Y % 4) * 4 + X % 4 of plane c's record.  3 x 3 x 4 rectified values, 108 MACs in fp32, weights and biases in LDS; zero padding at the HR border.
// HR pixel (Y, X) of item img: the three output values, bias first, taps in (ky, kx, c) order
template <typename T>
__device__ __forceinline__ void ps4_tail_pixel(const T* __restrict__ in, const float* s_w, size_t img, size_t npix, int X, int Y, int h, int w, float acc[3]) {
  const int H = 4 * h, W = 4 * w;
  acc[0] = s_w[108]; acc[1] = s_w[109]; acc[2] = s_w[110];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = Y + ky - 1;
    if (yy < 0 || yy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = X + kx - 1;
      if (xx < 0 || xx >= W) continue;
      const size_t pix = (img * h + (yy >> 2)) * w + (xx >> 2);
      const int sub = (yy & 3) * 4 + (xx & 3);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = fmaxf((float)in[((size_t)c * npix + pix) * 16 + sub], 0.f);
#pragma unroll
        for (int o = 0; o < 3; ++o) acc[o] = fmaf(s_w[((o * 4 + c) * 3 + ky) * 3 + kx], v, acc[o]);
      }
    }
  }
}
// out.at(img): item img's (3, 4 h, 4 w)
template <typename T, typename Out>
__global__ __launch_bounds__(256) void k_ps4_conv_tail(const T* __restrict__ in, const float* __restrict__ wb, Out out, int n, int h, int w) {
  __shared__ float s_w[112];
  if (threadIdx.x < 111) s_w[threadIdx.x] = wb[threadIdx.x];
  __syncthreads();
  const int H = 4 * h, W = 4 * w;
  const size_t HW = (size_t)H * W, total = (size_t)n * HW, npix = (size_t)n * h * w;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % W), Y = (int)((i / W) % H);
    const size_t img = i / HW;
    float acc[3];
    ps4_tail_pixel<T>(in, s_w, img, npix, X, Y, h, w, acc);
    float* dst = out.at(img) + (i - img * HW);
#pragma unroll
    for (int o = 0; o < 3; ++o) dst[o * HW] = acc[o];
  }
}
template <typename T, typename Out>
SS4K_STAGE_LAUNCH launch_ps4_conv_tail(const char* route, const char* what, const T* in, const float* wb, const Out& out, int n, int h, int w, hipStream_t st) {
  SS4K_STAGE_REQUIRE(n > 0 && n <= Out::MAX_ITEMS && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull / 16, what, "sizes");
  SS4K_STAGE_REQUIRE(out.complete(n), what, "NULL item");
  SS4K_GLUE_ROUTE(route);
  hipLaunchKernelGGL((k_ps4_conv_tail<T, Out>), grid_for((size_t)n * 16 * h * w), dim3(256), 0, st, in, wb, out, n, h, w);
  SS4K_LAUNCH_OK();
}

}  // namespace ss4k
