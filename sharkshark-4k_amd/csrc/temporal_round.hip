// The one kernel of a round of the temporal upscaler with stream slots (upscaler_temporal.cpp, TemporalUpscaler::round):
// tround::gather_planes<3|4> collects the LR planes of the round's frames - each in a ring slot of its own stream, in its own allocation - into
// one contiguous run.  With four planes it builds the packed (K, 4, lh, lw) denoiser input, the noise plane included, each frame at its own level; with three it gathers the
// leaving frames for the tail.  It only copies 16-byte slots and writes two constants.  tround::gather_planes_pad is its padded form, and
// tround::gather_planes_motion[_pad] (at the end of this file) the four-plane gathers whose noise plane is the motion-adaptive map.
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

// ---- tround::gather_planes_motion[_pad]: the four-plane gather with the motion-adaptive noise map (temporal_motion_plan.h) -------------------------
// One kernel for both forms.  Frame j (blockIdx.y) is cut into tiles of TILE_H source rows by TILE_W columns of the PADDED width; blockIdx.x
// strides over a frame's tiles.  A workgroup of 256 takes a tile; thread (r, c) = (tid / 16, tid % 16) owns the 16-byte slot of row T0 + r at
// columns X0 + 4c .. + 3 in all four output planes.  Per tile:
//   1. every thread loads its own slot of the current frame's three planes (columns beyond lw: reflected) - they are the slot's planes 0..2;
//   2. D = (|a0 - b0| + |a1 - b1| + |a2 - b2|) / 3 goes to LDS for the tile's source rows T0 - 1 .. T0 + TILE_H and source columns
//      X0 - 4 .. X0 + TILE_W + 3, where they lie inside the frame: a thread's own slot from the values of step 1, the 68 slots of the frame
//      around them by the first 68 threads.  The halo is four columns wide so that it is whole slots, and so that the source columns which the
//      padded columns of a row's last slot reflect to (down to lw - 4, neighbours to lw - 5) are in the tile that holds that slot;
//   3. after one barrier a thread reads, per pixel, the nine D of its SOURCE pixel's neighbourhood - rows and columns reflected at the frame's
//      borders, in source order - and accumulates them with the taps in one fixed chain of fused multiply-adds.  A padded column's value is so
//      computed as the pixel it reflects to is computed anywhere: the same bits;
//   4. four 16-byte stores, and four more into row 2 (lh - 1) - y where that is a padded row: a padded row is its source row, copied.
// A frame with the constant plane skips 2 and 3 (the decision is the same for a whole workgroup).  The unpadded form is the padded one with
// (ph, pw) = (lh, lw) and 16-byte loads.  LDS: 18 rows of 72 floats; column c sits at c + c / 32 of a 74-float row.  What that is for: a
// ds_read_b32 is served per 32-lane half of the wave over 32 banks, and a half holds two tile rows of sixteen threads four floats apart; the
// shift after column 31 puts the sixteen threads of a row on sixteen different banks, and the stride 74 = 2 mod 4 puts the second row on the
// other bank classes, up to two lanes per half that still share a bank where a row crosses column 32 or 64.  The two halves of a wave (rows r
// and r + 2, stride 148 = 0 mod 4) are served one after the other and do not meet.  This is reasoned from the bank rule, not measured: no
// conflict counter was read.  A pixel costs nine scalar LDS reads, 36 per thread, with no reuse between a thread's four neighbouring pixels -
// 36 KiB of LDS reads for a tile that moves 40 KiB through global memory, which is what bounds the kernel.
// No atomics, no scratch, no workgroup waits for another; indices are 32-bit, the launcher refuses 4 ph pw >= 2^31.
struct TroundTaps { float w[9]; };

constexpr int TM_TH = TROUND_MOTION_TILE_H, TM_TW = TROUND_MOTION_TILE_W, TM_HALO = 4;
constexpr int TM_ROWS = TM_TH + 2, TM_SLOT_COLS = TM_TW / 4 + 2, TM_STRIDE = 74;
constexpr int TM_HALO_SLOTS = 2 * TM_SLOT_COLS + 2 * TM_TH;   // 68
constexpr unsigned TROUND_MOTION_MAX_BLOCKS = 2048;           // 256 CUs x 8 workgroups of this size: tiles beyond are strode over
static_assert(TM_TH * (TM_TW / 4) == 256, "one thread per slot of a tile");
static_assert(TM_TW + 2 * TM_HALO + (TM_TW + 2 * TM_HALO - 1) / 32 <= TM_STRIDE, "the padded LDS row holds the tile's columns");

__device__ __forceinline__ int tm_lds(int row, int col) { return row * TM_STRIDE + col + (col >> 5); }
__device__ __forceinline__ int tm_reflect(int i, int n) { i = i < 0 ? -i : i; return i >= n ? 2 * (n - 1) - i : i; }
__device__ __forceinline__ float tm_diff(float a0, float b0, float a1, float b1, float a2, float b2) {
  return __fdiv_rn(__fadd_rn(__fadd_rn(fabsf(__fsub_rn(a0, b0)), fabsf(__fsub_rn(a1, b1))), fabsf(__fsub_rn(a2, b2))), 3.0f);
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_tround_gather_motion(TroundTable tab, TroundTaps taps, float* __restrict__ dst, int k, int lh, int lw,
                                                              int ph, int pw, unsigned long long start_bits, float level_start, int tiles_x,
                                                              int n_tiles) {
  __shared__ float D[TM_ROWS * TM_STRIDE];
  const int j = blockIdx.y;
  if (j >= k) return;
  const float* __restrict__ cur = tab.src[j];
  const float* __restrict__ prev = tab.prev[j];
  bool constant = (start_bits >> j) & 1ull;   // (a frame without the bit has a previous frame: the launcher refuses it otherwise)
  const uint32_t* f = tab.flag[j];
  if (!constant && f) constant = *f != 0;
  const float scale = tab.level[j];
  float* __restrict__ out = dst + (size_t)j * 4u * (size_t)ph * pw;
  const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;

  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int ty = tile / tiles_x, T0 = ty * TM_TH, X0 = (tile - ty * tiles_x) * TM_TW;
    const int y = T0 + r, x = X0 + 4 * c;
    const bool active = y < lh && x < pw;
    float cv[3][4] = {};
    if (active) {
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        const float* __restrict__ row = cur + (pl * lh + y) * lw;
        if (ALIGNED) {   // lw == pw: the slot lies inside the row
          const float4 v = *reinterpret_cast<const float4*>(row + x);
          cv[pl][0] = v.x; cv[pl][1] = v.y; cv[pl][2] = v.z; cv[pl][3] = v.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) cv[pl][i] = row[tround_reflect_hi((unsigned)(x + i), (unsigned)lw)];
        }
      }
    }
    if (!constant) {
      // D of one slot of the staged region: slot row sr (source row T0 - 1 + sr), slot column sc (source columns X0 - 4 + 4 sc ..)
      auto stage = [&](int sr, int sc, bool own) {
        const int gy = T0 - 1 + sr, gx = X0 - TM_HALO + 4 * sc;
        if (gy < 0 || gy >= lh || gx < 0 || gx >= lw) return;
        float a[3][4], b[3][4];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          const int at = (pl * lh + gy) * lw + gx;
          if (ALIGNED) {   // gx and lw are multiples of 4: the slot lies inside the row
            const float4 q = *reinterpret_cast<const float4*>(prev + at);
            b[pl][0] = q.x; b[pl][1] = q.y; b[pl][2] = q.z; b[pl][3] = q.w;
            if (own) {
#pragma unroll
              for (int i = 0; i < 4; ++i) a[pl][i] = cv[pl][i];
            } else {
              const float4 v = *reinterpret_cast<const float4*>(cur + at);
              a[pl][0] = v.x; a[pl][1] = v.y; a[pl][2] = v.z; a[pl][3] = v.w;
            }
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const bool in = gx + i < lw;
              b[pl][i] = in ? prev[at + i] : 0.f;
              a[pl][i] = own ? cv[pl][i] : in ? cur[at + i] : 0.f;   // (own: columns below lw are not reflected)
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (gx + i < lw) D[tm_lds(sr, 4 * sc + i)] = tm_diff(a[0][i], b[0][i], a[1][i], b[1][i], a[2][i], b[2][i]);
      };
      if (active) stage(1 + r, 1 + c, true);
      if (tid < TM_HALO_SLOTS) {
        int sr, sc;
        if (tid < 2 * TM_SLOT_COLS) { sr = tid < TM_SLOT_COLS ? 0 : TM_ROWS - 1; sc = tid < TM_SLOT_COLS ? tid : tid - TM_SLOT_COLS; }
        else { const int h = tid - 2 * TM_SLOT_COLS; sr = 1 + (h >> 1); sc = (h & 1) ? TM_SLOT_COLS - 1 : 0; }
        stage(sr, sc, false);
      }
      __syncthreads();
    }
    if (active) {
      float m[4];
      if (constant) {
        m[0] = m[1] = m[2] = m[3] = level_start;
      } else {
        const int r0 = tm_reflect(y - 1, lh) - T0 + 1, r1 = r + 1, r2 = tm_reflect(y + 1, lh) - T0 + 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gx = (int)tround_reflect_hi((unsigned)(x + i), (unsigned)lw), off = X0 - TM_HALO;
          const int c0 = tm_reflect(gx - 1, lw) - off, c1 = gx - off, c2 = tm_reflect(gx + 1, lw) - off;
          float acc = __fmul_rn(taps.w[0], D[tm_lds(r0, c0)]);
          acc = __fmaf_rn(taps.w[1], D[tm_lds(r0, c1)], acc);
          acc = __fmaf_rn(taps.w[2], D[tm_lds(r0, c2)], acc);
          acc = __fmaf_rn(taps.w[3], D[tm_lds(r1, c0)], acc);
          acc = __fmaf_rn(taps.w[4], D[tm_lds(r1, c1)], acc);
          acc = __fmaf_rn(taps.w[5], D[tm_lds(r1, c2)], acc);
          acc = __fmaf_rn(taps.w[6], D[tm_lds(r2, c0)], acc);
          acc = __fmaf_rn(taps.w[7], D[tm_lds(r2, c1)], acc);
          acc = __fmaf_rn(taps.w[8], D[tm_lds(r2, c2)], acc);
          m[i] = __fmul_rn(fminf(fmaxf(__fmul_rn(10.0f, acc), 0.0f), 0.1f), scale);
        }
      }
      const int y2 = 2 * (lh - 1) - y;   // the padded row that is this row's reflection, if there is one
      const bool twice = y2 >= lh && y2 < ph;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        const float4 v = make_float4(cv[pl][0], cv[pl][1], cv[pl][2], cv[pl][3]);
        *reinterpret_cast<float4*>(out + (pl * ph + y) * pw + x) = v;
        if (twice) *reinterpret_cast<float4*>(out + (pl * ph + y2) * pw + x) = v;
      }
      const float4 v3 = make_float4(m[0], m[1], m[2], m[3]);
      *reinterpret_cast<float4*>(out + (3 * ph + y) * pw + x) = v3;
      if (twice) *reinterpret_cast<float4*>(out + (3 * ph + y2) * pw + x) = v3;
    }
    if (!constant) __syncthreads();   // the next tile's D goes where this one's is still being read
  }
}

static void tround_gather_motion(const TroundTable& tab, float* dst, int k, int lh, int lw, bool pad, unsigned long long start_bits, float level_start,
                                 hipStream_t st) {
  SS4K_REQUIRE(k >= 1 && k <= TROUND_MAX_FRAMES, "temporal gather motion: 1..64 frames");
  // (the padded form pads at most 3 rows or columns by reflection without the edge: op_tround_gather_pad's limit)
  SS4K_REQUIRE(!pad || (lh >= 4 && lw >= 4), "temporal gather motion pad: a plane of at least 4 x 4");
  SS4K_REQUIRE(pad || (lh >= 2 && lw >= 2 && lw % 4 == 0), "temporal gather motion: a plane of at least 2 x 2 whose rows are whole 16-byte slots");
  const size_t ph = pad ? ((size_t)lh + 3) & ~size_t(3) : (size_t)lh, pw = pad ? ((size_t)lw + 3) & ~size_t(3) : (size_t)lw;
  SS4K_REQUIRE((double)ph * (double)pw * 4.0 < 2147483648.0, "temporal gather motion: a frame of four planes holds fewer than 2^31 values");
  SS4K_REQUIRE(dst && ((uintptr_t)dst & 15) == 0, "temporal gather motion: NULL or misaligned destination");
  const size_t src_bytes = (size_t)3 * lh * lw * 4, dst_bytes = (size_t)k * 4 * ph * pw * 4;
  const uintptr_t align = pad ? 3 : 15;
  const char* d = reinterpret_cast<const char*>(dst);
  for (int j = 0; j < k; ++j) {
    SS4K_REQUIRE(tab.src[j] && ((uintptr_t)tab.src[j] & align) == 0, "temporal gather motion: NULL or misaligned source");
    SS4K_REQUIRE(((uintptr_t)tab.flag[j] & 3) == 0, "temporal gather motion: misaligned flag word");
    // a source inside the destination would be read while it is written
    const char* s = reinterpret_cast<const char*>(tab.src[j]);
    SS4K_REQUIRE(s + src_bytes <= d || d + dst_bytes <= s, "temporal gather motion: a source overlaps the destination");
    if ((start_bits >> j) & 1ull) continue;   // a stream's first frame: no previous frame is read
    SS4K_REQUIRE(tab.prev[j] && ((uintptr_t)tab.prev[j] & align) == 0, "temporal gather motion: NULL or misaligned previous frame");
    const char* p = reinterpret_cast<const char*>(tab.prev[j]);
    SS4K_REQUIRE(p + src_bytes <= d || d + dst_bytes <= p, "temporal gather motion: a previous frame overlaps the destination");
  }
  TroundTaps taps;
  temporal_round::motion_taps(taps.w);
  const int tiles_x = (int)((pw + TM_TW - 1) / TM_TW), n_tiles = tiles_x * ((lh + TM_TH - 1) / TM_TH);
  const dim3 blocks(std::max(std::min((unsigned)n_tiles, TROUND_MOTION_MAX_BLOCKS / (unsigned)k), 1u), (unsigned)k);
  if (pad) {
    SS4K_GLUE_ROUTE("tround::gather_planes_motion_pad");
    hipLaunchKernelGGL(k_tround_gather_motion<false>, blocks, dim3(256), 0, st, tab, taps, dst, k, lh, lw, (int)ph, (int)pw, start_bits, level_start,
                       tiles_x, n_tiles);
  } else {
    SS4K_GLUE_ROUTE("tround::gather_planes_motion");
    hipLaunchKernelGGL(k_tround_gather_motion<true>, blocks, dim3(256), 0, st, tab, taps, dst, k, lh, lw, (int)ph, (int)pw, start_bits, level_start,
                       tiles_x, n_tiles);
  }
  SS4K_LAUNCH_OK();
}

void op_tround_gather_motion(const TroundTable& tab, float* dst, int k, int lh, int lw, unsigned long long start_bits, float level_start, hipStream_t st) {
  tround_gather_motion(tab, dst, k, lh, lw, false, start_bits, level_start, st);
}

void op_tround_gather_motion_pad(const TroundTable& tab, float* dst, int k, int lh, int lw, unsigned long long start_bits, float level_start,
                                 hipStream_t st) {
  tround_gather_motion(tab, dst, k, lh, lw, true, start_bits, level_start, st);
}

}  // namespace ss4k
