// The one kernel of a round of the temporal upscaler with stream slots (upscaler_temporal.cpp, TemporalUpscaler::round):
// tround::gather_planes<3|4> collects the LR planes of the round's frames - each in a ring slot of its own stream, in its own allocation - into
// one contiguous run.  With four planes it builds the packed (K, 4, lh, lw) denoiser input, the noise plane included, each frame at its own level; with three it gathers the
// leaving frames for the tail.  It only copies 16-byte slots and writes two constants.
#include "upscaler_temporal.h"

#ifndef SS4K_LAUNCH_OK
#define SS4K_LAUNCH_OK() SS4K_HIP(hipGetLastError())
#endif

namespace ss4k {

constexpr unsigned TROUND_MAX_BLOCKS = 256 * 8 * 4;   // 2^21 threads of 256: grid-stride beyond (bsvd_online.hip's blocks_for)

// One thread per 16-byte slot of the destination; blockIdx.y is the frame (no division per slot, and the table entry and the flag word are the
// same for a whole workgroup), blockIdx.x strides over the frame's slots.  Frame j: planes 0..2 from tab.src[j] (3 * plane_slots slots,
// contiguous); plane 3 - PLANES == 4 only - is level_start where the frame starts a stream (bit j of start_bits) or a scene (*tab.flag[j] != 0, a
// NULL pointer: no flag), else tab.level[j]: every frame carries its own stream's level.  blockIdx.y is uniform over the workgroup, so the table
// entries are scalar loads from the kernel arguments: no scratch, no device table.
// The flag word is an ordinary (vector) load of a word an earlier kernel on the stream wrote.
template <int PLANES>
__global__ __launch_bounds__(256) void k_tround_gather(TroundTable tab, uint4* __restrict__ dst, int k, unsigned plane_slots,
                                                       unsigned long long start_bits, float level_start) {
  const size_t src_slots = (size_t)3 * plane_slots, frame_slots = (size_t)PLANES * plane_slots;
  const int j = blockIdx.y;
  if (j >= k) return;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(tab.src[j]);
  uint4* __restrict__ out = dst + (size_t)j * frame_slots;
  unsigned bits = 0;
  if (PLANES == 4) {
    bool start = (start_bits >> j) & 1ull;
    const uint32_t* f = tab.flag[j];
    if (!start && f) start = *f != 0;
    bits = __float_as_uint(start ? level_start : tab.level[j]);
  }
  for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r < frame_slots; r += (size_t)gridDim.x * blockDim.x)
    out[r] = PLANES == 4 && r >= src_slots ? make_uint4(bits, bits, bits, bits) : src[r];
}

void op_tround_gather(const TroundTable& tab, float* dst, int k, size_t plane_px, int planes, unsigned long long start_bits, float level_start,
                      hipStream_t st) {
  SS4K_REQUIRE(k >= 1 && k <= TROUND_MAX_FRAMES, "temporal gather: 1..64 frames");
  SS4K_REQUIRE(planes == 3 || planes == 4, "temporal gather: 3 or 4 output planes");
  SS4K_REQUIRE(plane_px > 0 && plane_px % 4 == 0 && plane_px / 4 < 4294967296ull / 4, "temporal gather: a plane is a positive multiple of 4 pixels below 2^32");
  SS4K_REQUIRE(dst && ((uintptr_t)dst & 15) == 0, "temporal gather: NULL or misaligned destination");
  for (int j = 0; j < k; ++j) {
    SS4K_REQUIRE(tab.src[j] && ((uintptr_t)tab.src[j] & 15) == 0, "temporal gather: NULL or misaligned source");
    SS4K_REQUIRE(((uintptr_t)tab.flag[j] & 3) == 0, "temporal gather: misaligned flag word");
    // a source inside the destination would be read while it is written
    const char* s = reinterpret_cast<const char*>(tab.src[j]); const char* d = reinterpret_cast<const char*>(dst);
    SS4K_REQUIRE(s + plane_px * 12 <= d || d + (size_t)k * planes * plane_px * 4 <= s, "temporal gather: a source overlaps the destination");
  }
  const unsigned plane_slots = (unsigned)(plane_px / 4);
  // at most 2^21 threads in all: a frame's blocks are capped at the launch's share and stride beyond
  const size_t frame_slots = (size_t)planes * plane_slots;
  const dim3 blocks((unsigned)std::max<size_t>(std::min<size_t>((frame_slots + 255) / 256, TROUND_MAX_BLOCKS / (unsigned)k), 1), (unsigned)k);
  if (planes == 4) {
    SS4K_GLUE_ROUTE("tround::gather_planes<4>");
    hipLaunchKernelGGL(k_tround_gather<4>, blocks, dim3(256), 0, st, tab, reinterpret_cast<uint4*>(dst), k, plane_slots, start_bits, level_start);
  } else {
    SS4K_GLUE_ROUTE("tround::gather_planes<3>");
    hipLaunchKernelGGL(k_tround_gather<3>, blocks, dim3(256), 0, st, tab, reinterpret_cast<uint4*>(dst), k, plane_slots, start_bits, level_start);
  }
  SS4K_LAUNCH_OK();
}

// ---- tround::gather_planes_pad: gather_planes<4> for a frame whose planes BSVD's two 2x poolings do not divide -------------------------------
// Frame j: planes 0..2 from a ring slot of (3, lh, lw) fp32, written as (ph, pw) planes - (lh, lw) rounded up to multiples of 4 - padded at the
// bottom and on the right by reflection without repeating the edge (torch's and numpy's 'reflect': row y >= lh is row 2 (lh - 1) - y, columns
// likewise); plane 3 is the frame's level over the whole (ph, pw), by gather_planes<4>'s rule.  One thread per 16-byte slot of the destination
// (pw is a multiple of 4: a slot never crosses a row); a source row starts at any 4-byte address (lw may be odd), so the four values are dword
// loads, each at its own reflected column.  blockIdx.y is the frame, blockIdx.x strides over the frame's slots.  Indices are 32-bit: the
// launcher refuses a frame of 2^31 values or more.  No LDS, no atomics, no workgroup waits for another, no scratch.
__device__ __forceinline__ unsigned tround_reflect_hi(unsigned i, unsigned n) { return i >= n ? 2u * (n - 1u) - i : i; }

__global__ __launch_bounds__(256) void k_tround_gather_pad(TroundTable tab, uint4* __restrict__ dst, int k, unsigned lh, unsigned lw, unsigned ph,
                                                           unsigned row_slots, unsigned long long start_bits, float level_start) {
  const unsigned plane_slots = ph * row_slots, src_slots = 3u * plane_slots, frame_slots = 4u * plane_slots;
  const int j = blockIdx.y;
  if (j >= k) return;
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(tab.src[j]);
  uint4* __restrict__ out = dst + (size_t)j * frame_slots;
  bool start = (start_bits >> j) & 1ull;
  const uint32_t* f = tab.flag[j];
  if (!start && f) start = *f != 0;
  const unsigned bits = __float_as_uint(start ? level_start : tab.level[j]);
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < frame_slots; r += gridDim.x * blockDim.x) {
    uint4 v = make_uint4(bits, bits, bits, bits);
    if (r < src_slots) {
      const unsigned pl = r / plane_slots, in_plane = r - pl * plane_slots, y = in_plane / row_slots, x = (in_plane - y * row_slots) * 4u;
      const uint32_t* __restrict__ row = src + ((size_t)pl * lh + tround_reflect_hi(y, lh)) * lw;
      v.x = row[tround_reflect_hi(x, lw)];
      v.y = row[tround_reflect_hi(x + 1u, lw)];
      v.z = row[tround_reflect_hi(x + 2u, lw)];
      v.w = row[tround_reflect_hi(x + 3u, lw)];
    }
    out[r] = v;
  }
}

void op_tround_gather_pad(const TroundTable& tab, float* dst, int k, int lh, int lw, unsigned long long start_bits, float level_start,
                          hipStream_t st) {
  SS4K_REQUIRE(k >= 1 && k <= TROUND_MAX_FRAMES, "temporal gather pad: 1..64 frames");
  // at most 3 rows or columns are padded: reflection without the edge needs more rows and columns than that
  SS4K_REQUIRE(lh >= 4 && lw >= 4, "temporal gather pad: a plane of at least 4 x 4");
  const size_t ph = ((size_t)lh + 3) & ~size_t(3), pw = ((size_t)lw + 3) & ~size_t(3);
  SS4K_REQUIRE((double)ph * (double)pw * 4.0 < 2147483648.0, "temporal gather pad: a padded frame of four planes holds fewer than 2^31 values");
  SS4K_REQUIRE(dst && ((uintptr_t)dst & 15) == 0, "temporal gather pad: NULL or misaligned destination");
  const size_t src_bytes = (size_t)3 * lh * lw * 4, dst_bytes = (size_t)k * 4 * ph * pw * 4;
  for (int j = 0; j < k; ++j) {
    SS4K_REQUIRE(tab.src[j] && ((uintptr_t)tab.src[j] & 3) == 0, "temporal gather pad: NULL or misaligned source");
    SS4K_REQUIRE(((uintptr_t)tab.flag[j] & 3) == 0, "temporal gather pad: misaligned flag word");
    // a source inside the destination would be read while it is written
    const char* s = reinterpret_cast<const char*>(tab.src[j]); const char* d = reinterpret_cast<const char*>(dst);
    SS4K_REQUIRE(s + src_bytes <= d || d + dst_bytes <= s, "temporal gather pad: a source overlaps the destination");
  }
  const unsigned row_slots = (unsigned)(pw / 4);
  const size_t frame_slots = (size_t)4 * ph * row_slots;
  // at most 2^21 threads in all: a frame's blocks are capped at the launch's share and stride beyond
  const dim3 blocks((unsigned)std::max<size_t>(std::min<size_t>((frame_slots + 255) / 256, TROUND_MAX_BLOCKS / (unsigned)k), 1), (unsigned)k);
  SS4K_GLUE_ROUTE("tround::gather_planes_pad");
  hipLaunchKernelGGL(k_tround_gather_pad, blocks, dim3(256), 0, st, tab, reinterpret_cast<uint4*>(dst), k, (unsigned)lh, (unsigned)lw, (unsigned)ph,
                     row_slots, start_bits, level_start);
  SS4K_LAUNCH_OK();
}

}  // namespace ss4k
