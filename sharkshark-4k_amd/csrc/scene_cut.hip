// Scene-cut detection kernels (scene_cut.h), gfx950.  Three launches per round whatever its size, in stream order: cut::sad_items sums
// |frame - prev| per item into a u64 and writes the frame over prev in the same pass, cut::decide applies the rule per item, cut::clear_items
// zero-fills the recurrent state of the items it flagged.  Integer sums: exact, and independent of the order the workgroups arrive in.
// cut::decide_run is the rule for the temporal BSVD service (upscaler_temporal.cpp): the n frames of a job are ONE stream's consecutive frames.
#include "scene_cut.h"
#include "glue.h"

#define SS4K_LAUNCH_OK() SS4K_HIP(hipGetLastError())

namespace ss4k {
namespace cut {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int BLOCK = 256;
constexpr int EDGE_THREADS = 30;   // at most 15 head bytes and 15 tail bytes around the 16-byte chunks

// workgroups per item: enough to stream a frame, few enough that a round of many items stays a small grid (the kernels stride)
static unsigned grid_x(size_t chunks, int n) {
  const size_t want = (chunks + BLOCK - 1) / BLOCK, cap = (size_t)std::max(32, 2048 / std::max(n, 1));
  return (unsigned)std::max<size_t>(1, std::min(want, cap));
}

// The 16-byte chunks are aligned on b (the stored frame: the side that is loaded AND stored); a's chunks then start at any byte address and
// are read as one 16-byte load all the same (the global memory path takes unaligned addresses).  The bytes in front of b's first aligned
// address and behind its last whole chunk - fewer than 16 each - go one per thread through workgroup 0.
template <bool STORE>
__global__ __launch_bounds__(BLOCK) void k_sad_items(SadItems it, unsigned long long* __restrict__ acc, size_t bytes) {
  const int item = blockIdx.y;
  const bool compare = (it.compare >> item) & 1;
  const uint8_t* a = it.a[item];
  uint8_t* b = it.b[item];
  const size_t to_aligned = (size_t)(-(uintptr_t)b & 15);
  const size_t head = to_aligned < bytes ? to_aligned : bytes;
  const size_t chunks = (bytes - head) >> 4, tail0 = head + (chunks << 4);
  uint32_t sum = 0;   // <= 4080 per chunk: the launcher bounds the chunks per thread
  for (size_t c = blockIdx.x * (size_t)BLOCK + threadIdx.x; c < chunks; c += (size_t)gridDim.x * BLOCK) {
    u32x4 va;
    __builtin_memcpy(&va, a + head + (c << 4), 16);
    u32x4* pb = reinterpret_cast<u32x4*>(b + head + (c << 4));
    if (compare) {
      const u32x4 vb = *pb;
      sum = __builtin_amdgcn_sad_u8(va.x, vb.x, sum);
      sum = __builtin_amdgcn_sad_u8(va.y, vb.y, sum);
      sum = __builtin_amdgcn_sad_u8(va.z, vb.z, sum);
      sum = __builtin_amdgcn_sad_u8(va.w, vb.w, sum);
    }
    if (STORE) *pb = va;
  }
  if (blockIdx.x == 0 && threadIdx.x < EDGE_THREADS) {
    const size_t t = threadIdx.x, ntail = bytes - tail0;
    if (t < head + ntail) {
      const size_t idx = t < head ? t : tail0 + (t - head);
      const uint8_t va = a[idx];
      if (compare) { const int d = (int)va - (int)b[idx]; sum += (uint32_t)(d < 0 ? -d : d); }
      if (STORE) b[idx] = va;
    }
  }
  if (!compare) return;   // (the whole workgroup: an item that is not compared is only copied)
  unsigned long long s = sum;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ unsigned long long part[BLOCK / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
#pragma unroll
    for (int k = 0; k < BLOCK / 64; ++k) tot += part[k];
    atomicAdd(acc + item, tot);   // ONE 64-bit integer atomic per workgroup and item
  }
}

void sad_items(const SadItems& it, unsigned long long* acc, int n, size_t bytes, bool store, hipStream_t st) {
  SS4K_REQUIRE(n >= 1 && n <= MAX_ITEMS, "scene cut (sad): 1..64 items");
  SS4K_REQUIRE(bytes >= 1 && bytes <= MAX_FRAME_BYTES, "scene cut (sad): frame size");
  SS4K_REQUIRE(acc && ((uintptr_t)acc & 7) == 0, "scene cut (sad): the sums are 8-byte aligned");
  const unsigned long long all = n == 64 ? ~0ull : (1ull << n) - 1;
  SS4K_REQUIRE(store || (it.compare & all) == all, "scene cut (sad): without a store every item is compared");
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(it.a[i] && it.b[i], "scene cut (sad): NULL item");
  const dim3 grid(grid_x(bytes >> 4, n), (unsigned)n);
  if (store) hipLaunchKernelGGL(k_sad_items<true>, grid, dim3(BLOCK), 0, st, it, acc, bytes);
  else hipLaunchKernelGGL(k_sad_items<false>, grid, dim3(BLOCK), 0, st, it, acc, bytes);
  SS4K_LAUNCH_OK();
}

__global__ __launch_bounds__(64) void k_decide(DecideItems it, unsigned long long* __restrict__ acc, SlotState* __restrict__ state,
                                               uint32_t* __restrict__ flags, int n) {
  const int i = threadIdx.x;
  if (i >= n) return;
  SlotState s = state[it.slot[i]];
  uint32_t is_cut = 0;
  if ((it.compare >> i) & 1) {
    const unsigned long long S = acc[i], d = S > s.s_prev ? S - s.s_prev : s.s_prev - S, score = S < d ? S : d;
    is_cut = score >= it.T ? 1u : 0u;
    s.s_prev = S; s.compared += 1; s.cuts += is_cut;
    s.last_sad = S; s.last_score = score;
  } else {   // no comparison: the next one starts from S_prev = 0
    s.s_prev = 0; s.last_sad = 0; s.last_score = 0;
  }
  s.last_was_cut = (int32_t)is_cut; s.reserved = 0;
  state[it.slot[i]] = s;
  flags[i] = is_cut;
  acc[i] = 0;
}

void decide(const DecideItems& it, unsigned long long* acc, SlotState* state, uint32_t* flags, int n, hipStream_t st) {
  SS4K_REQUIRE(n >= 1 && n <= MAX_ITEMS, "scene cut (decide): 1..64 items");
  SS4K_REQUIRE(acc && state && flags && it.T >= 1, "scene cut (decide): NULL argument or a threshold of 0");
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(it.slot[i] >= 0 && it.slot[i] < MAX_ITEMS, "scene cut (decide): slot");
  hipLaunchKernelGGL(k_decide, dim3(1), dim3(64), 0, st, it, acc, state, flags, n);
  SS4K_LAUNCH_OK();
}

// ONE thread: the n sums of a run of consecutive frames of one stream depend on each other through S_prev, so they are walked in order
__global__ __launch_bounds__(64) void k_decide_run(unsigned long long* __restrict__ acc, SlotState* __restrict__ state, uint32_t* __restrict__ ring,
                                                   unsigned pos, unsigned mask, int n, int compare_first, unsigned long long T) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  SlotState s = state[0];
  for (int i = 0; i < n; ++i) {
    uint32_t is_cut = 0;
    if (i > 0 || compare_first) {
      const unsigned long long S = acc[i], d = S > s.s_prev ? S - s.s_prev : s.s_prev - S, score = S < d ? S : d;
      is_cut = score >= T ? 1u : 0u;
      s.s_prev = S; s.compared += 1; s.cuts += is_cut;
      s.last_sad = S; s.last_score = score;
    } else {   // no comparison: the next one starts from S_prev = 0
      s.s_prev = 0; s.last_sad = 0; s.last_score = 0;
    }
    s.last_was_cut = (int32_t)is_cut;
    ring[(pos + (unsigned)i) & mask] = is_cut;
    acc[i] = 0;
  }
  s.reserved = 0;
  state[0] = s;
}

void decide_run(unsigned long long* acc, SlotState* state, uint32_t* ring, unsigned pos, unsigned mask, int n, bool compare_first,
                unsigned long long T, hipStream_t st) {
  SS4K_REQUIRE(n >= 1 && n <= MAX_ITEMS, "scene cut (decide_run): 1..64 frames");
  SS4K_REQUIRE(acc && state && ring && T >= 1, "scene cut (decide_run): NULL argument or a threshold of 0");
  SS4K_REQUIRE((mask & (mask + 1u)) == 0 && mask != 0xffffffffu && (unsigned)n <= mask + 1u, "scene cut (decide_run): the ring mask must be 2^k - 1 and hold the run");
  SS4K_GLUE_ROUTE("cut::decide_run");
  hipLaunchKernelGGL(k_decide_run, dim3(1), dim3(64), 0, st, acc, state, ring, pos, mask, n, compare_first ? 1 : 0, T);
  SS4K_LAUNCH_OK();
}

__device__ __forceinline__ void zero_fill(void* p, size_t bytes) {
  const size_t chunks = bytes >> 4;
  u32x4* q = reinterpret_cast<u32x4*>(p);
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (size_t c = blockIdx.x * (size_t)BLOCK + threadIdx.x; c < chunks; c += (size_t)gridDim.x * BLOCK) q[c] = z;
  if (blockIdx.x == 0 && threadIdx.x < ((bytes & 15) >> 2)) reinterpret_cast<uint32_t*>(p)[(chunks << 2) + threadIdx.x] = 0u;
}

__global__ __launch_bounds__(BLOCK) void k_clear_items(ClearItems it, const uint32_t* __restrict__ flags, size_t lr_bytes, size_t hr_bytes) {
  const int item = blockIdx.y;
  if (!flags[item]) return;   // no cut: the workgroup is done
  zero_fill(it.lr[item], lr_bytes);
  zero_fill(it.hr[item], hr_bytes);
}

void clear_items(const ClearItems& it, unsigned long long compare, const uint32_t* flags, int n, size_t lr_bytes, size_t hr_bytes, hipStream_t st) {
  SS4K_REQUIRE(n >= 1 && n <= MAX_ITEMS && flags, "scene cut (clear): 1..64 items");
  SS4K_REQUIRE(lr_bytes > 0 && hr_bytes > 0 && lr_bytes % 4 == 0 && hr_bytes % 4 == 0, "scene cut (clear): sizes are multiples of 4");
  for (int i = 0; i < n; ++i) {
    if (!((compare >> i) & 1)) continue;   // (never flagged: its pointers are not read)
    SS4K_REQUIRE(it.lr[i] && it.hr[i] && ((uintptr_t)it.lr[i] & 15) == 0 && ((uintptr_t)it.hr[i] & 15) == 0, "scene cut (clear): state pointers are 16-byte aligned");
  }
  hipLaunchKernelGGL(k_clear_items, dim3(grid_x(std::max(lr_bytes, hr_bytes) >> 4, n), (unsigned)n), dim3(BLOCK), 0, st, it, flags, lr_bytes, hr_bytes);
  SS4K_LAUNCH_OK();
}

}  // namespace cut
}  // namespace ss4k
