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

}  // namespace ss4k
