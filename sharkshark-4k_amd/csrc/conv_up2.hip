// ConvTranspose2d(64, 64, 3, stride 2, pad 1, output_padding 1) + bias + ReLU on "planes" tensors, (N, H, W) -> (N, 2 H, 2 W): the two
// up-sampling layers of TecoGAN's SRNet (tecogan_nets.py:118-122) by their four output phases.  With Wt the state_dict's (C_in, C_out, 3, 3),
// output pixel (2 y + a, 2 x + b), a, b in {0, 1}, is
//   sum over dy, dx in {0, 1} with ky = a + 1 - 2 dy, kx = b + 1 - 2 dx both in 0..2 of  x[:, y + dy, x + dx] . Wt[:, :, ky, kx]   + bias
// with x zero at row H and column W: phase (0,0) has 1 tap, (0,1) and (1,0) have 2, (1,1) has 4.  The four phases of one input pixel read one
// 2 x 2 input window and use each of the nine 64 x 64 tap matrices exactly once - the matrix work of ONE 3x3 64 -> 64 layer at the INPUT
// resolution, a quarter of what the same layer costs embedded in a pad-1 3x3 convolution 64 -> 256 + PixelShuffle(2) (frvsr_teco.cpp).
// A first kernel: correct and bounded like the conv kernels, no pipelining - every tile waits for its halo, and one workgroup per CU holds
// the LDS.  Measured at 264-276 TFLOP/s on its useful FLOPs against 285-313 for the embedded route, so SS4K_FRVSR_CONVT_PHASE selects it and
// the default stays the embedded route (profiles/NOTES_r11.md).
//
// Tile: TH x TW = 8 x 32 input pixels per workgroup of 4 waves, a wave taking rows w and w + 4 as two 16-pixel groups each.  The matrix
// core multiplies weights (operand A: 16 output channels x K) by pixels (operand B: K x 16 pixels), as conv_w16.hip orients them, so an
// accumulator lane holds 4 consecutive output channels of one pixel (row 4 (lane >> 4) + r, column lane & 15):
//   __half: v_mfma_f32_16x16x32_f16, K = 32 = two planes of one tap; lane l holds k = 8 (l >> 4) + j, j = 0..7
//   float : v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fma chain), K = 4; lane l holds k = l >> 4
// A window's B fragments are read once from LDS and feed every phase that uses the window; an A fragment is read once and feeds both
// 16-pixel groups.  Accumulators: 2 groups x 4 phases x CBL 16-channel blocks.
//
// LDS (dynamic, 16-byte carves): the weights of one PASS, then the (TH + 1) x (TW + 1) halo tile.
//   __half: one pass holds all nine tap matrices, 73 728 B, + 38 016 B of tile = 111 744 B
//   float : the nine matrices are 147 456 B, so a pass holds one 16-channel output block (CBL = 1, 36 864 B) + 76 032 B of tile, and the
//           kernel makes four passes over its tiles, each writing one output plane
// The tile is stored slot-major - [16-byte slot of the pixel's four records][pixel] - so that the 16 lanes of a B read (one pixel each,
// the same slot) touch 16 consecutive 16-byte slots.
//
// Packed weights (pack_convt3x3s2 in pack.cpp, host side, once per model), PASSES = 4 / CBL, KS = k-steps per tap (2 | 16), E = K per lane (8 | 1):
//   blob[pass][tap = ky * 3 + kx][ks][cb < CBL][lane][e] = Wt[cin = ks * 4 E + E (lane >> 4) + e][cout = 16 (pass * CBL + cb) + (lane & 15)][ky][kx]
// Every (cin, cout, ky, kx) appears exactly once: lane & 15 and (pass, cb) enumerate cout, (ks, lane >> 4, e) enumerate cin.
#include "frvsr.h"
#include <type_traits>

namespace ss4k {
namespace up2 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int NW = 4, TH = CONVT_TH, TW = CONVT_TW, XH = TH + 1, XW = TW + 1, NPIX = XH * XW;
static_assert(TH % NW == 0 && TW == 32, "a wave takes whole rows of two 16-pixel groups");

template <typename T> struct Cfg {
  static constexpr bool HALF = sizeof(T) == 2;
  static constexpr int REC = HALF ? 32 : 64;        // bytes of a pixel's record in a plane
  static constexpr int SPR = REC / 16;              // 16-byte slots per record
  static constexpr int SLOTS = 4 * SPR;             // ... per pixel (four planes)
  static constexpr int KS = HALF ? 2 : 16;          // k-steps per tap
  static constexpr int E = HALF ? 8 : 1;            // K per lane and step
  static constexpr int FRAG = E * (int)sizeof(T);   // bytes of a lane's A (or B) fragment
  static constexpr int CBL = HALF ? 4 : 1;          // 16-channel output blocks per pass
  static constexpr int PASSES = 4 / CBL;
  static constexpr int W_BYTES = 9 * KS * CBL * 64 * FRAG;
  static constexpr int X_BYTES = SLOTS * NPIX * 16;
  static constexpr size_t LDS_BYTES = W_BYTES + X_BYTES;
  static_assert(W_BYTES % 16 == 0 && LDS_BYTES <= 160 * 1024, "LDS carves");
};

template <typename T>
__global__ __launch_bounds__(64 * NW) void convt3x3s2_kernel(const ConvtArgs a) {
  using C = Cfg<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wl = smem;
  char* const xl = smem + C::W_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, p16 = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntiles = a.N * a.tiles_y * a.tiles_x;
  const int OH = 2 * a.H, OW = 2 * a.W;

  for (int pass = 0; pass < C::PASSES; ++pass) {
    __syncthreads();   // (the pass before has read its weights)
    {
      const uint4* src = reinterpret_cast<const uint4*>(a.w + (size_t)pass * C::W_BYTES);
      for (int i = tid; i < C::W_BYTES / 16; i += 64 * NW) reinterpret_cast<uint4*>(wl)[i] = src[i];
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const int tx = tile % a.tiles_x, ty = (tile / a.tiles_x) % a.tiles_y, n = tile / (a.tiles_x * a.tiles_y);
      const int x0 = tx * TW, y0 = ty * TH;
      __syncthreads();   // the tile before has been read
      // halo tile: rows y0 .. y0 + TH, columns x0 .. x0 + TW, zeros past the image; consecutive threads read consecutive 16 bytes of a plane's row
      for (int i = tid; i < NPIX * C::SLOTS; i += 64 * NW) {
        const int s = i % C::SPR;
        int r = i / C::SPR;
        const int px = r % XW; r /= XW;
        const int plane = r % 4, row = r / 4;
        const int y = y0 + row, x = x0 + px;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (y < a.H && x < a.W)
          v = *reinterpret_cast<const uint4*>(a.in + (size_t)plane * a.in_plane_bytes + (((size_t)n * a.H + y) * a.W + x) * C::REC + s * 16);
        *reinterpret_cast<uint4*>(xl + ((size_t)(plane * C::SPR + s) * NPIX + row * XW + px) * 16) = v;
      }
      __syncthreads();   // (also: this pass's weights are in place)

      for (int rr = wave; rr < TH; rr += NW) {
        f32x4 acc[2][4][C::CBL];
#pragma unroll
        for (int hn = 0; hn < 2; ++hn)
#pragma unroll
          for (int ph = 0; ph < 4; ++ph)
#pragma unroll
            for (int cb = 0; cb < C::CBL; ++cb) acc[hn][ph][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int dx = 0; dx < 2; ++dx) {
            // the window's B fragments: pixel (rr + dy, 16 hn + p16 + dx), k-step ks
            const int pix = (rr + dy) * XW + p16 + dx;
            std::conditional_t<C::HALF, uint4, float> b[C::KS][2];
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
              for (int hn = 0; hn < 2; ++hn) {
                if constexpr (C::HALF)   // k = 8 q + j of step ks: plane 2 ks + (q >> 1), record half q & 1 = slot 4 ks + q
                  b[ks][hn] = *reinterpret_cast<const uint4*>(xl + ((size_t)(4 * ks + q) * NPIX + pix + 16 * hn) * 16);
                else                     // k = q of step ks: channel 4 ks + q = plane ks >> 2, slot ks & 3 of its record, float q
                  b[ks][hn] = *reinterpret_cast<const float*>(xl + ((size_t)ks * NPIX + pix + 16 * hn) * 16 + q * 4);
              }
#pragma unroll
            for (int pa = 0; pa < 2; ++pa)
#pragma unroll
              for (int pb = 0; pb < 2; ++pb) {
                const int ky = pa + 1 - 2 * dy, kx = pb + 1 - 2 * dx;
                if (ky < 0 || kx < 0) continue;
                const int tap = ky * 3 + kx, ph = 2 * pa + pb;
#pragma unroll
                for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
                  for (int cb = 0; cb < C::CBL; ++cb) {
                    const char* wp = wl + ((size_t)((tap * C::KS + ks) * C::CBL + cb) * 64 + lane) * C::FRAG;
                    if constexpr (C::HALF) {
                      const f16x8 w = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(wp));
#pragma unroll
                      for (int hn = 0; hn < 2; ++hn)
                        acc[hn][ph][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, __builtin_bit_cast(f16x8, b[ks][hn]), acc[hn][ph][cb], 0, 0, 0);
                    } else {
                      const float w = *reinterpret_cast<const float*>(wp);
#pragma unroll
                      for (int hn = 0; hn < 2; ++hn) acc[hn][ph][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[ks][hn], acc[hn][ph][cb], 0, 0, 0);
                    }
                  }
              }
          }
        // bias, ReLU, store: the lane's 4 channels (4 q ..) of output pixel (2 y + pa, 2 x + pb), plane pass * CBL + cb
        const int y = y0 + rr;
#pragma unroll
        for (int cb = 0; cb < C::CBL; ++cb) {
          const int plane = pass * C::CBL + cb;
          const float4 bias = *reinterpret_cast<const float4*>(a.bias + plane * 16 + 4 * q);
          char* const op = a.out + (size_t)plane * a.out_plane_bytes + 4 * q * sizeof(T);
#pragma unroll
          for (int hn = 0; hn < 2; ++hn) {
            const int x = x0 + 16 * hn + p16;
            if (y >= a.H || x >= a.W) continue;
#pragma unroll
            for (int ph = 0; ph < 4; ++ph) {
              const f32x4 t = acc[hn][ph][cb];
              const float v0 = fmaxf(t[0] + bias.x, 0.f), v1 = fmaxf(t[1] + bias.y, 0.f), v2 = fmaxf(t[2] + bias.z, 0.f), v3 = fmaxf(t[3] + bias.w, 0.f);
              char* o = op + (((size_t)n * OH + 2 * y + (ph >> 1)) * OW + 2 * x + (ph & 1)) * C::REC;
              if constexpr (C::HALF) {
                union { uint2 u; __half h[4]; } pk;
                pk.h[0] = __float2half_rn(v0); pk.h[1] = __float2half_rn(v1); pk.h[2] = __float2half_rn(v2); pk.h[3] = __float2half_rn(v3);
                *reinterpret_cast<uint2*>(o) = pk.u;
              } else {
                *reinterpret_cast<float4*>(o) = make_float4(v0, v1, v2, v3);
              }
            }
          }
        }
      }
    }
  }
}

}  // namespace up2

void launch_convt3x3s2(ss4k_ctx* ctx, const ConvtArgs& a0, int dtype, int max_workgroups, hipStream_t st) {
  using namespace up2;
  ConvtArgs a = a0;
  SS4K_REQUIRE(a.N > 0 && a.H > 0 && a.W > 0 && (double)a.N * 4.0 * a.H * a.W < 2147483648.0, "convt3x3s2: sizes");
  a.tiles_x = (a.W + TW - 1) / TW; a.tiles_y = (a.H + TH - 1) / TH;
  const int ntiles = a.N * a.tiles_y * a.tiles_x;
  int gx = std::min(ntiles, std::max(1, ctx->num_cu));   // one workgroup per CU: its LDS
  if (max_workgroups > 0) gx = std::min(gx, max_workgroups);
  const double flops = 2.0 * 9.0 * 64.0 * 64.0 * (double)a.N * a.H * a.W;
  ProfScope ps(ctx, st, PROF_CONV);
  if (dtype == SS4K_F16) {
    const void* fn = reinterpret_cast<const void*>(&convt3x3s2_kernel<__half>);
    if (ctx->lds_attr_set.insert(fn).second) SS4K_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg<__half>::LDS_BYTES));
    ctx->prof_family = "up2::convt3x3s2_kernel<half> (stride-2 transposed 3x3 by output phase, 16x16x32 MFMA)";
    hipLaunchKernelGGL(convt3x3s2_kernel<__half>, dim3(gx), dim3(64 * NW), Cfg<__half>::LDS_BYTES, st, a);
  } else {
    const void* fn = reinterpret_cast<const void*>(&convt3x3s2_kernel<float>);
    if (ctx->lds_attr_set.insert(fn).second) SS4K_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg<float>::LDS_BYTES));
    ctx->prof_family = "up2::convt3x3s2_kernel<float> (stride-2 transposed 3x3 by output phase, 16x16x4 fp32 MFMA)";
    hipLaunchKernelGGL(convt3x3s2_kernel<float>, dim3(gx), dim3(64 * NW), Cfg<float>::LDS_BYTES, st, a);
  }
  SS4K_HIP(hipGetLastError());
  ps.done(flops);
}

}  // namespace ss4k
