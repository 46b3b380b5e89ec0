// The glue kernels of the frame-recurrent chain with the online denoiser in front (frvsr_temporal.cpp, FrvsrTemporal::round / flush): the one
// every wave runs, and frvt::clear_flagged_items (below), which only the waves of streams that carry scene-cut flags run in front of it.
// frvt::denoised_in_items turns a wave's denoised frames into the generator's input, each written into its own stream's lr buffer,
//   lr_curr = 0.8 * clamp01(sharpen3x3_reflect(den)) + 0.2 * lr_before            (fsrcnn_upscaler.py:279-281)
// in ONE launch whatever the wave's size.  The value is bit for bit what glue::depthwise_reflect<3> (glue.hip) gives with clamp and blend: the
// loops below are that kernel's - the same tap order, the row loop kept rolled, the same `acc += tap * px` and `acc * a + b * src` expressions,
// the taps read from the same device table and the two blend factors passed as kernel arguments - so the compiler contracts them the same way.
// Do not "improve" the arithmetic: tests/test_gpu_frvsr_temporal_kernel.py compares the bits.
#include "frvsr_temporal.h"

#ifndef SS4K_LAUNCH_OK
#define SS4K_LAUNCH_OK() SS4K_HIP(hipGetLastError())
#endif

namespace ss4k {

// torch's 'reflect': -1 -> 1, n -> n - 2 (glue.hip's reflect)
__device__ __forceinline__ int frvt_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// blockIdx.z = 3 * item + plane, blockIdx.y strides over the rows, blockIdx.x over a row's pixels.  The item is uniform over the workgroup, so
// its three table entries are scalar loads from the kernel arguments: no scratch, no device table.  Every output pixel is written by exactly one
// thread, and no workgroup waits for another.
__global__ __launch_bounds__(256) void k_frvt_denoised_in(FrvtTable tab, const float* __restrict__ taps, int n_items, int h, int w,
                                                          float blend_a, float blend_b) {
  constexpr int K = 3, r = 1;
  const int item = blockIdx.z / 3, pl = blockIdx.z % 3;
  if (item >= n_items) return;
  const float* __restrict__ src = tab.den[item] + (size_t)pl * h * w;
  const float* __restrict__ blend_src = tab.lr[item];
  float* __restrict__ out = tab.dst[item];
  for (int y = blockIdx.y; y < h; y += gridDim.y) {
    const size_t row = ((size_t)pl * h + y) * w;
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < w; x += gridDim.x * blockDim.x) {
      int xi[K];
#pragma unroll
      for (int kx = 0; kx < K; ++kx) xi[kx] = frvt_reflect(x + kx - r, w);
      float acc = 0.f;
#pragma unroll 1
      for (int ky = 0; ky < K; ++ky) {
        const float* sr = src + (size_t)frvt_reflect(y + ky - r, h) * w;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) acc += taps[ky * K + kx] * sr[xi[kx]];
      }
      acc = fminf(fmaxf(acc, 0.f), 1.f);
      acc = acc * blend_a + blend_b * blend_src[row + x];
      out[row + x] = acc;
    }
  }
}

void op_frvt_denoised_in_items(const FrvtTable& tab, int n_items, int h, int w, const float* taps_dev, float blend_a, float blend_b, hipStream_t st) {
  // every refusal before the launch
  SS4K_REQUIRE(n_items >= 1 && n_items <= FRVT_MAX_ITEMS, "frvsr denoised in: 1..64 items");
  SS4K_REQUIRE(h >= 2 && w >= 2, "frvsr denoised in: reflect padding of 1 needs a plane of at least 2 x 2, as torch requires");
  SS4K_REQUIRE((double)h * (double)w * 3.0 < 2147483648.0, "frvsr denoised in: a frame holds fewer than 2^31 values");
  SS4K_REQUIRE(taps_dev, "frvsr denoised in: NULL taps");
  const size_t frame_bytes = (size_t)3 * h * w * 4;
  for (int i = 0; i < n_items; ++i) {
    SS4K_REQUIRE(tab.den[i] && tab.lr[i] && tab.dst[i], "frvsr denoised in: NULL item pointer");
    SS4K_REQUIRE((((uintptr_t)tab.den[i] | (uintptr_t)tab.lr[i] | (uintptr_t)tab.dst[i]) & 3) == 0, "frvsr denoised in: misaligned item pointer");
    // a pixel's neighbours are read while other pixels are written: the destination may not lie inside the item's sources
    const char* d = reinterpret_cast<const char*>(tab.dst[i]);
    for (const float* src : {tab.den[i], tab.lr[i]}) {
      const char* s = reinterpret_cast<const char*>(src);
      SS4K_REQUIRE(s + frame_bytes <= d || d + frame_bytes <= s, "frvsr denoised in: a destination overlaps its item's sources");
    }
  }
  SS4K_GLUE_ROUTE("frvt::denoised_in_items");
  const dim3 grid((unsigned)std::min((w + 255) / 256, 64), (unsigned)std::min(h, 65535), (unsigned)(3 * n_items));
  hipLaunchKernelGGL(k_frvt_denoised_in, grid, dim3(256), 0, st, tab, taps_dev, n_items, h, w, blend_a, blend_b);
  SS4K_LAUNCH_OK();
}

// ---- frvt::denoised_in_crop_items: the same, with den a frame of LARGER planes of which only the top-left (h, w) count -------------------------
// The padded chain's denoiser runs at (ph, pw), (h, w) rounded up to multiples of 4; what follows it acts on the crop.  The loops, the
// expressions and the tap table are k_frvt_denoised_in's, term for term - only den's strides differ: a row is pw values, a plane ph * pw; lr and
// dst keep w and h * w.  The reflection is at the crop's borders (h, w), so the padding is never read.  The value is bit for bit what
// k_frvt_denoised_in gives on a contiguous copy of the crop (tests/test_gpu_frvsr_temporal_pad_kernel.py): the strides change addresses, not
// the order or the form of the floating-point operations.
__global__ __launch_bounds__(256) void k_frvt_denoised_in_crop(FrvtTable tab, const float* __restrict__ taps, int n_items, int h, int w, int ph,
                                                               int pw, float blend_a, float blend_b) {
  constexpr int K = 3, r = 1;
  const int item = blockIdx.z / 3, pl = blockIdx.z % 3;
  if (item >= n_items) return;
  const float* __restrict__ src = tab.den[item] + (size_t)pl * ph * pw;
  const float* __restrict__ blend_src = tab.lr[item];
  float* __restrict__ out = tab.dst[item];
  for (int y = blockIdx.y; y < h; y += gridDim.y) {
    const size_t row = ((size_t)pl * h + y) * w;
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < w; x += gridDim.x * blockDim.x) {
      int xi[K];
#pragma unroll
      for (int kx = 0; kx < K; ++kx) xi[kx] = frvt_reflect(x + kx - r, w);
      float acc = 0.f;
#pragma unroll 1
      for (int ky = 0; ky < K; ++ky) {
        const float* sr = src + (size_t)frvt_reflect(y + ky - r, h) * pw;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) acc += taps[ky * K + kx] * sr[xi[kx]];
      }
      acc = fminf(fmaxf(acc, 0.f), 1.f);
      acc = acc * blend_a + blend_b * blend_src[row + x];
      out[row + x] = acc;
    }
  }
}

void op_frvt_denoised_in_crop_items(const FrvtTable& tab, int n_items, int h, int w, int ph, int pw, const float* taps_dev, float blend_a,
                                    float blend_b, hipStream_t st) {
  // every refusal before the launch
  SS4K_REQUIRE(n_items >= 1 && n_items <= FRVT_MAX_ITEMS, "frvsr denoised in crop: 1..64 items");
  SS4K_REQUIRE(h >= 2 && w >= 2, "frvsr denoised in crop: reflect padding of 1 needs a plane of at least 2 x 2, as torch requires");
  SS4K_REQUIRE(ph >= h && pw >= w, "frvsr denoised in crop: the denoised planes hold the crop");
  SS4K_REQUIRE((double)ph * (double)pw * 3.0 < 2147483648.0, "frvsr denoised in crop: a denoised frame holds fewer than 2^31 values");
  SS4K_REQUIRE(taps_dev, "frvsr denoised in crop: NULL taps");
  const size_t frame_bytes = (size_t)3 * h * w * 4, den_bytes = (size_t)3 * ph * pw * 4;
  for (int i = 0; i < n_items; ++i) {
    SS4K_REQUIRE(tab.den[i] && tab.lr[i] && tab.dst[i], "frvsr denoised in crop: NULL item pointer");
    SS4K_REQUIRE((((uintptr_t)tab.den[i] | (uintptr_t)tab.lr[i] | (uintptr_t)tab.dst[i]) & 3) == 0, "frvsr denoised in crop: misaligned item pointer");
    // a pixel's neighbours are read while other pixels are written: the destination may not lie inside the item's sources, of which den is
    // the larger frame
    const char* d = reinterpret_cast<const char*>(tab.dst[i]);
    const char* dn = reinterpret_cast<const char*>(tab.den[i]);
    const char* l = reinterpret_cast<const char*>(tab.lr[i]);
    SS4K_REQUIRE(dn + den_bytes <= d || d + frame_bytes <= dn, "frvsr denoised in crop: a destination overlaps its item's sources");
    SS4K_REQUIRE(l + frame_bytes <= d || d + frame_bytes <= l, "frvsr denoised in crop: a destination overlaps its item's sources");
  }
  SS4K_GLUE_ROUTE("frvt::denoised_in_crop_items");
  const dim3 grid((unsigned)std::min((w + 255) / 256, 64), (unsigned)std::min(h, 65535), (unsigned)(3 * n_items));
  hipLaunchKernelGGL(k_frvt_denoised_in_crop, grid, dim3(256), 0, st, tab, taps_dev, n_items, h, w, ph, pw, blend_a, blend_b);
  SS4K_LAUNCH_OK();
}

// ---- frvt::clear_flagged_items: the late reset of a scene cut -----------------------------------------------------------------------------------
// A frame that the detector flagged when it went in leaves the denoiser 16 frames later; in that wave its stream's lr_prev / hr_prev must read
// as zero, as for a stream's first frame.  blockIdx.y is the item: its flag pointer and the flag word are uniform over the workgroup (loads from
// the kernel arguments and one load through a uniform pointer), so a workgroup whose item has no live ring or no cut returns at once, whole.
// Otherwise it zero-fills both buffers grid-stride over blockIdx.x with 16-byte stores, plus a tail of up to three dwords - cut::clear_items'
// fill (scene_cut.hip) with the flag read where the ring keeps it.  No LDS, no atomics, no workgroup waits for another, no scratch.
typedef uint32_t frvt_u32x4 __attribute__((ext_vector_type(4)));
constexpr int FRVT_CLEAR_BLOCK = 256;

__device__ __forceinline__ void frvt_zero_fill(void* p, size_t bytes) {
  const size_t chunks = bytes >> 4;
  frvt_u32x4* q = reinterpret_cast<frvt_u32x4*>(p);
  const frvt_u32x4 z = {0u, 0u, 0u, 0u};
  for (size_t c = blockIdx.x * (size_t)FRVT_CLEAR_BLOCK + threadIdx.x; c < chunks; c += (size_t)gridDim.x * FRVT_CLEAR_BLOCK) q[c] = z;
  if (blockIdx.x == 0 && threadIdx.x < ((bytes & 15) >> 2)) reinterpret_cast<uint32_t*>(p)[(chunks << 2) + threadIdx.x] = 0u;
}

__global__ __launch_bounds__(FRVT_CLEAR_BLOCK) void k_frvt_clear_flagged(FrvtClearTable tab, int n_items, size_t lr_bytes, size_t hr_bytes) {
  const int item = blockIdx.y;
  if (item >= n_items) return;
  const uint32_t* flag = tab.flag[item];
  if (!flag) return;      // a stream without a live flag ring
  if (!*flag) return;     // the leaving frame starts no scene
  frvt_zero_fill(tab.lr[item], lr_bytes);
  frvt_zero_fill(tab.hr[item], hr_bytes);
}

void op_frvt_clear_flagged_items(const FrvtClearTable& tab, int n_items, size_t lr_bytes, size_t hr_bytes, hipStream_t st) {
  // every refusal before the launch
  SS4K_REQUIRE(n_items >= 1 && n_items <= FRVT_MAX_ITEMS, "frvsr clear flagged: 1..64 items");
  SS4K_REQUIRE(lr_bytes > 0 && hr_bytes > 0 && lr_bytes % 4 == 0 && hr_bytes % 4 == 0, "frvsr clear flagged: sizes are multiples of 4");
  for (int i = 0; i < n_items; ++i) {
    SS4K_REQUIRE(tab.lr[i] && tab.hr[i], "frvsr clear flagged: NULL state pointer");
    SS4K_REQUIRE((((uintptr_t)tab.lr[i] | (uintptr_t)tab.hr[i]) & 15) == 0, "frvsr clear flagged: state pointers are 16-byte aligned");
    SS4K_REQUIRE(((uintptr_t)tab.flag[i] & 3) == 0, "frvsr clear flagged: a flag is a 32-bit word");
  }
  SS4K_GLUE_ROUTE("frvt::clear_flagged_items");
  // cut::clear_items' shape: at most max(32, 2048 / n) workgroups per item, enough to stream the larger buffer
  const size_t want = ((std::max(lr_bytes, hr_bytes) >> 4) + FRVT_CLEAR_BLOCK - 1) / FRVT_CLEAR_BLOCK, cap = (size_t)std::max(32, 2048 / n_items);
  const unsigned gx = (unsigned)std::max<size_t>(1, std::min(want, cap));
  hipLaunchKernelGGL(k_frvt_clear_flagged, dim3(gx, (unsigned)n_items), dim3(FRVT_CLEAR_BLOCK), 0, st, tab, n_items, lr_bytes, hr_bytes);
  SS4K_LAUNCH_OK();
}

}  // namespace ss4k
