// Kernels of the online BSVD executor (bsvd_online.h): the windowed temporal shift and the carry / history update.  Both only select and
// copy 16-byte slots of the conv kernels' planes layout ([plane][frame][pixel][record]), fp16 and fp32 records alike.  The shift has a
// cut-aware build (scene cuts: neighbours across a cut are zeros), and bsvdo::noise_planes fills the noise planes of a push from the flags.
#include "bsvd_online.h"

#ifndef SS4K_LAUNCH_OK
#define SS4K_LAUNCH_OK() SS4K_HIP(hipGetLastError())
#endif

namespace ss4k {

constexpr unsigned MAX_BLOCKS_1D = 256 * 8 * 4;   // 2^21 threads of 256: grid-stride beyond (glue.hip's grid1d)

static inline unsigned blocks_for(size_t n) {
  const size_t g = (n + 255) / 256;
  return (unsigned)std::max<size_t>(std::min<size_t>(g, MAX_BLOCKS_1D), 1);
}

// CUTS: the cut-aware build.  flag[f & mask] != 0: stream frame f is the first of a new scene; f0: the stream frame of output frame 0.  A neighbour
// across a cut is zeros, as it is at either end of a stream.  The flag words are ordinary (vector) loads, read only where the group is live today.
template <bool CUTS>
__global__ void k_bsvd_online_shift(const uint4* __restrict__ in, uint4* __restrict__ out, int nplanes, int in_frames, int slot0, int frames,
                                    size_t frame_slots, int spr, int ch_per_plane, int fold, int first_has_prev, int n_next,
                                    const uint32_t* __restrict__ flag, unsigned mask, int f0) {
  const int ch_per_slot = ch_per_plane / spr;
  const size_t out_plane = (size_t)frames * frame_slots;
  const size_t in_plane = (size_t)in_frames * frame_slots;
  const size_t total = out_plane * nplanes;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int p = (int)(i / out_plane);
    const size_t r = i - (size_t)p * out_plane;
    const int t = (int)(r / frame_slots);
    const size_t q = r - (size_t)t * frame_slots;
    const int ch0 = p * ch_per_plane + (int)(q % spr) * ch_per_slot;
    int ts = t;
    bool live = true;
    if (ch0 < fold) {
      ts = t + 1; live = t < n_next;
      if (CUTS) live = live && flag[(unsigned)(f0 + t + 1) & mask] == 0;
    } else if (ch0 < 2 * fold) {
      ts = t - 1; live = t > 0 || first_has_prev;
      if (CUTS) live = live && flag[(unsigned)(f0 + t) & mask] == 0;
    }
    uint4 v = make_uint4(0, 0, 0, 0);
    if (live) v = in[(size_t)p * in_plane + (size_t)(slot0 + ts) * frame_slots + q];
    out[i] = v;
  }
}

// the checks both builds share: everything the kernel reads lies inside the input
static void check_shift(const void* in, void* out, int nplanes, int in_frames, int slot0, int frames, size_t frame_px, int slots_per_record,
                        int ch_per_plane, int fold, int first_has_prev, int n_next) {
  SS4K_REQUIRE(in && out && nplanes > 0 && frames > 0 && frame_px > 0 && in_frames > 0, "online shift: empty tensor");
  SS4K_REQUIRE(slots_per_record > 0 && ch_per_plane >= slots_per_record && fold > 0 && fold % (ch_per_plane / slots_per_record) == 0,
               "online shift: fold must be a multiple of the 16-byte channel group");
  SS4K_REQUIRE(n_next >= 0 && n_next <= frames, "online shift: n_next outside 0..frames");
  // every slot the kernel reads lies inside the input: centres slot0 .. slot0 + frames - 1, the first frame's t - 1, the last live t + 1
  SS4K_REQUIRE(slot0 - (first_has_prev ? 1 : 0) >= 0 && slot0 + std::max(frames - 1, n_next) < in_frames,
               "online shift: the window leaves the carried buffer");
}

void op_bsvd_online_shift(const void* in, void* out, int nplanes, int in_frames, int slot0, int frames, size_t frame_px, int slots_per_record,
                          int ch_per_plane, int fold, int first_has_prev, int n_next, hipStream_t st) {
  check_shift(in, out, nplanes, in_frames, slot0, frames, frame_px, slots_per_record, ch_per_plane, fold, first_has_prev, n_next);
  SS4K_GLUE_ROUTE(slots_per_record == 2 ? "bsvdo::shift_window<half>" : "bsvdo::shift_window<float>");
  const size_t total = (size_t)nplanes * frames * frame_px * slots_per_record;
  hipLaunchKernelGGL(k_bsvd_online_shift<false>, dim3(blocks_for(total)), dim3(256), 0, st, reinterpret_cast<const uint4*>(in),
                     reinterpret_cast<uint4*>(out), nplanes, in_frames, slot0, frames, frame_px * slots_per_record, slots_per_record,
                     ch_per_plane, fold, first_has_prev, n_next, (const uint32_t*)nullptr, 0u, 0);
  SS4K_LAUNCH_OK();
}

void op_bsvd_online_shift_cuts(const void* in, void* out, int nplanes, int in_frames, int slot0, int frames, size_t frame_px, int slots_per_record,
                               int ch_per_plane, int fold, int first_has_prev, int n_next, const uint32_t* flag_ring, unsigned ring_mask, int f0,
                               hipStream_t st) {
  check_shift(in, out, nplanes, in_frames, slot0, frames, frame_px, slots_per_record, ch_per_plane, fold, first_has_prev, n_next);
  SS4K_REQUIRE(flag_ring && ((uintptr_t)flag_ring & 3) == 0, "online shift (cuts): NULL or misaligned flag ring");
  SS4K_REQUIRE((ring_mask & (ring_mask + 1u)) == 0 && ring_mask != 0xffffffffu, "online shift (cuts): the ring mask must be 2^k - 1");
  SS4K_REQUIRE(f0 >= 0 && (double)f0 + frames + 1 < 2147483648.0, "online shift (cuts): frame number outside 0..2^31");
  SS4K_GLUE_ROUTE(slots_per_record == 2 ? "bsvdo::shift_window_cuts<half>" : "bsvdo::shift_window_cuts<float>");
  const size_t total = (size_t)nplanes * frames * frame_px * slots_per_record;
  hipLaunchKernelGGL(k_bsvd_online_shift<true>, dim3(blocks_for(total)), dim3(256), 0, st, reinterpret_cast<const uint4*>(in),
                     reinterpret_cast<uint4*>(out), nplanes, in_frames, slot0, frames, frame_px * slots_per_record, slots_per_record,
                     ch_per_plane, fold, first_has_prev, n_next, flag_ring, ring_mask, f0);
  SS4K_LAUNCH_OK();
}

// blockIdx.y: the frame; blockIdx.x strides over its noise plane (channel 3 of the packed (n, 4, h, w) input)
__global__ void k_bsvd_noise_planes(float* __restrict__ frames4, size_t plane_px, const uint32_t* __restrict__ flags, int stream_first,
                                    float level_start, float level) {
  const int f = blockIdx.y;
  const bool start = flags[f] != 0 || (f == 0 && stream_first);
  const float v = start ? level_start : level;
  float* dst = frames4 + ((size_t)f * 4 + 3) * plane_px;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < plane_px; i += (size_t)gridDim.x * blockDim.x) dst[i] = v;
}

void op_bsvd_noise_planes(float* frames4, int n, size_t plane_px, const uint32_t* flags, int stream_first, float level_start, float level,
                          hipStream_t st) {
  SS4K_REQUIRE(frames4 && flags && plane_px > 0, "noise planes: NULL argument or an empty plane");
  SS4K_REQUIRE(n >= 1 && n <= BSVD_ONLINE_MAX_PUSH, "noise planes: 1..64 frames");
  SS4K_REQUIRE(((uintptr_t)frames4 & 3) == 0 && ((uintptr_t)flags & 3) == 0, "noise planes: misaligned pointer");
  SS4K_GLUE_ROUTE("bsvdo::noise_planes");
  const unsigned gx = (unsigned)std::min<size_t>(blocks_for(plane_px), 1024);
  hipLaunchKernelGGL(k_bsvd_noise_planes, dim3(gx, (unsigned)n), dim3(256), 0, st, frames4, plane_px, flags, stream_first, level_start, level);
  SS4K_LAUNCH_OK();
}

// blockIdx.y: the entry; blockIdx.x strides over its nplanes * count * frame_slots slots
__global__ void k_bsvd_online_carry(const BsvdCarryTable tab) {
  const BsvdCarry e = tab.e[blockIdx.y];
  const size_t row = (size_t)e.count * e.frame_slots;
  const size_t total = row * e.nplanes;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(e.src);
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(e.dst);
  const size_t src_plane = (size_t)e.src_frames * e.frame_slots, dst_plane = (size_t)e.dst_frames * e.frame_slots;
  const size_t src_off = (size_t)e.src_first * e.frame_slots;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i / row, r = i - p * row;
    dst[p * dst_plane + r] = src[p * src_plane + src_off + r];
  }
}

void op_bsvd_online_carry(const BsvdCarryTable& tab, int entries, hipStream_t st) {
  SS4K_REQUIRE(entries > 0 && entries <= BSVD_ONLINE_MAX_CARRIES, "online carry: 1..22 entries");
  size_t most = 0;
  for (int i = 0; i < entries; ++i) {
    const BsvdCarry& e = tab.e[i];
    SS4K_REQUIRE(e.src && e.dst && e.nplanes > 0 && e.count > 0 && e.frame_slots > 0, "online carry: empty entry");
    SS4K_REQUIRE(e.src_first >= 0 && e.src_first + e.count <= e.src_frames && e.count <= e.dst_frames, "online carry: the move leaves its buffers");
    const size_t slot = 16, src_b = (size_t)e.nplanes * e.src_frames * e.frame_slots * slot, dst_b = (size_t)e.nplanes * e.dst_frames * e.frame_slots * slot;
    const char* s = static_cast<const char*>(e.src); const char* d = static_cast<const char*>(e.dst);
    SS4K_REQUIRE(s + src_b <= d || d + dst_b <= s, "online carry: source and destination overlap (the move has no safe order: use a ping-pong pair)");
    most = std::max(most, (size_t)e.nplanes * e.count * e.frame_slots);
  }
  SS4K_GLUE_ROUTE("bsvdo::carry");
  hipLaunchKernelGGL(k_bsvd_online_carry, dim3(blocks_for(most), entries), dim3(256), 0, st, tab);
  SS4K_LAUNCH_OK();
}

}  // namespace ss4k
