// The tail of TecoGAN's frame-recurrent generator (reference src/upscale/model/egvsr/models/networks/tecogan_nets.py:101-149, the FRNet
// EGVSR's was cut down from): after the last residual block
//   conv_up  = ConvTranspose2d(64, 64, 3, 2, 1, output_padding=1), ReLU, the same again        (h, w) -> (2 h, 2 w) -> (4 h, 4 w)
//   conv_out = Conv2d(64, 3, 3, 1, 1)                                                           at (4 h, 4 w)
//   out     += BicubicUpsample(4)(lr_curr)                                                      degradation 'BD'
//   out     += F.interpolate(lr_curr, scale_factor=4, 'bilinear', align_corners=False)          degradation 'BI' (frvsr_bi.hip)
// Everything before it is Frvsr::run (frvsr.cpp), which branches here when the generator is SS4K_FRVSR_TECOGAN; the tail's state is Frvsr::teco.
//
// The transposed convolution.  ConvTranspose2d(k 3, s 2, p 1, output_padding 1) maps (H, W) to (2 H, 2 W); with Wt the state_dict's
// (C_in, C_out, 3, 3), output pixel (2 y + a, 2 x + b), a, b in {0, 1}, is
//   sum over dy, dx in {0, 1} with ky = a + 1 - 2 dy, kx = b + 1 - 2 dx both in 0..2 of  x[:, y + dy, x + dx] . Wt[:, :, ky, kx]   (+ bias)
// where x is zero at row H and column W.  That is a pad-1 3x3 convolution 64 -> 256 followed by PixelShuffle(2):
//   W_eq[c' * 4 + 2 a + b][c][1 + dy][1 + dx] = Wt[c][c'][a + 1 - 2 dy][b + 1 - 2 dx]     (zero elsewhere), bias repeated per phase
// (tap (1 + dy, 1 + dx) of a pad-1 correlation reads x[y + dy, x + dx]; output channel c' * 4 + 2 a + b is PixelShuffle(2)'s channel c' of
// pixel (2 y + a, 2 x + b)).  Two routes compute it:
//   embedded (the default, SS4K_FRVSR_CONVT_EMBEDDED): embed_convt() builds W_eq on the host, once per model, and the layer runs on
//            conv_mfma.hip's PixelShuffle(2) epilogue in both dtypes - four times the matrix work, on a kernel that runs near its peak;
//   phase    (SS4K_FRVSR_CONVT_PHASE): conv_up2.hip computes the sum phase by phase - nine 64 x 64 tap products per INPUT pixel.  A first
//            kernel: measured 7 to 13 % slower than the embedded route, so it stays behind its pin as the cross-check.
// tests/test_tecogan_oracle_cpu.py holds both forms against F.conv_transpose2d in float64.
#include "frvsr.h"

namespace ss4k {

// W_eq (256, 64, 3, 3) OIHW followed by its 256 biases, from Wt (64, 64, 3, 3) + 64 biases
std::vector<float> embed_convt(const float* wt_and_bias, int nf) {
  const float* wt = wt_and_bias; const float* bias = wt_and_bias + (size_t)nf * nf * 9;
  std::vector<float> eq((size_t)4 * nf * nf * 9 + 4 * nf, 0.f);
  for (int co = 0; co < nf; ++co)
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) {
        const int o = co * 4 + 2 * a + b;
        for (int dy = 0; dy < 2; ++dy)
          for (int dx = 0; dx < 2; ++dx) {
            const int ky = a + 1 - 2 * dy, kx = b + 1 - 2 * dx;
            if (ky < 0 || kx < 0) continue;
            for (int ci = 0; ci < nf; ++ci) eq[(((size_t)o * nf + ci) * 3 + 1 + dy) * 3 + 1 + dx] = wt[(((size_t)ci * nf + co) * 3 + ky) * 3 + kx];
          }
        eq[(size_t)4 * nf * nf * 9 + o] = bias[co];
      }
  return eq;
}

void Frvsr::build_teco_tail(const float* up0, const float* up2, const float* out_w) {
  const int nf = desc.num_feat;
  const float* up[2] = {up0, up2};
  teco.embedded = !(route_flags & SS4K_FRVSR_CONVT_PHASE);
  for (int k = 0; k < 2; ++k) {
    if (teco.embedded) {
      const std::vector<float> eq = embed_convt(up[k], nf);
      ParamCursor pc{eq.data(), eq.size()};
      teco.up_layer[k] = net.add_conv(pc, 4 * nf, nf, net.spec_plain(nf, 1), false);
    } else {
      SS4K_REQUIRE(nf == 64, "tecogan tail: the phase kernel is built for 64 channels");
      const std::vector<uint8_t> pk = pack_convt3x3s2(up[k], desc.dtype);
      teco.up_w[k].ensure(pk.size()); teco.up_b[k].ensure((size_t)nf * 4);
      SS4K_HIP(hipMemcpy(teco.up_w[k].ptr, pk.data(), pk.size(), hipMemcpyHostToDevice));
      SS4K_HIP(hipMemcpy(teco.up_b[k].ptr, up[k] + (size_t)nf * nf * 9, (size_t)nf * 4, hipMemcpyHostToDevice));
      net.weight_bytes += pk.size() + (size_t)nf * 4;
    }
  }
  ParamCursor pc{out_w, (size_t)3 * nf * 9 + 3};
  teco.out_layer = net.add_conv(pc, 3, nf, net.spec_plain(nf), false);   // (an fp16 model: also conv_w16n.hip's blob)
}

void Frvsr::run_teco_tail(const Tens& body_all, int slot, const float* lr_curr, float* hr_out, const Items* items, int n, int h, int w, hipStream_t st) {
  const TecoTailDev& dev = teco.dev;
  const bool plan = net.plan_only, bi = degradation == SS4K_FRVSR_BI;
  const int nf = desc.num_feat;
  SS4K_REQUIRE(dev.group_items >= 0 && dev.group_items <= SS4K_FRVSR_MAX_STREAMS, "tecogan tail: group_items must be in 0..64");
  // items of one group: no plane of the (4 h, 4 w) tensors reaches 2^32 bytes
  const int fit = (int)std::max(1.0, std::min((double)n, std::floor(4294967295.0 / (16.0 * h * w * conv_rec_bytes(desc.dtype)))));
  const int G = std::min({n, dev.group_items > 0 ? dev.group_items : fit, (int)SS4K_FRVSR_MAX_STREAMS});
  const size_t lr_px = (size_t)h * w, rec = (size_t)net.rec();
  const Tens U1G = net.act(slot++, (size_t)G * 4 * lr_px, nf), U2G = net.act(slot++, (size_t)G * 16 * lr_px, nf);
  // conv_out's fp32 NCHW result (G, 3, 4 h, 4 w): 12 bytes per HR pixel in a slot of one plane (a record is 32 or 64)
  const Tens CO = net.act_planes(slot++, (size_t)G * 16 * lr_px, 1);
  auto relu = [](const Tens& out) { ConvOpts o; o.act = ACT_LRELU; o.slope = 0.f; o.epi = EPI_NHWC_PS2; o.out = out; return o; };
  for (int i0 = 0; i0 < n; i0 += G) {
    const int g = std::min(G, n - i0);
    // the group's tensors: planes of exactly g items at the head of the buffers (a short last group packs its planes closer)
    const Tens U1{U1G.p, (size_t)g * 4 * lr_px * rec, 0}, U2{U2G.p, (size_t)g * 16 * lr_px * rec, 0};
    const Tens body{body_all.p + (plan ? 0 : (size_t)i0 * lr_px * rec), body_all.plane_bytes, body_all.plane0};   // items i0 .. i0 + g of every plane
    timed(FRV_CONVT, st, [&] {
      if (teco.embedded) {
        net.conv(teco.up_layer[0], body, nullptr, g, h, w, relu(U1), st);
        net.conv(teco.up_layer[1], U1, nullptr, g, 2 * h, 2 * w, relu(U2), st);
      } else if (!plan) {
        const ConvtArgs a1{body.p + (size_t)body.plane0 * body.plane_bytes, body.plane_bytes, U1.p, U1.plane_bytes, teco.up_w[0].as<char>(), teco.up_b[0].as<float>(), g, h, w, 0, 0};
        launch_convt3x3s2(ctx, a1, desc.dtype, dev.max_workgroups, st);
        const ConvtArgs a2{U1.p, U1.plane_bytes, U2.p, U2.plane_bytes, teco.up_w[1].as<char>(), teco.up_b[1].as<float>(), g, 2 * h, 2 * w, 0, 0};
        launch_convt3x3s2(ctx, a2, desc.dtype, dev.max_workgroups, st);
      }
    });
    if (!plan && dev.up1) {
      float* t1 = dev.up1 + (size_t)i0 * nf * 4 * lr_px; float* t2 = dev.up2 + (size_t)i0 * nf * 16 * lr_px;
      SS4K_PLANES_T(desc.dtype, op_planes_to_nchw((const T*)U1.p, t1, g, nf, 2 * h, 2 * w, st); op_planes_to_nchw((const T*)U2.p, t2, g, nf, 4 * h, 4 * w, st));
    }
    timed(FRV_CONV_OUT, st, [&] {
      ConvOpts o; o.epi = EPI_NCHW_F32; o.out = Tens{CO.p, 0, 0};
      net.conv(teco.out_layer, U2, nullptr, g, 4 * h, 4 * w, o, st);
      net.lanes_join(st, true);
    });
    timed(FRV_SKIP, st, [&] {
      if (plan) return;
      const float* co = reinterpret_cast<const float*>(CO.p);
      if (items) {
        FrvsrPtrs lr{}, out{};
        for (int i = 0; i < g; ++i) { lr.p[i] = const_cast<float*>(items->lr_curr[i0 + i]); out.p[i] = items->hr_out->p[i0 + i]; }
        (bi ? op_bilinear4_add_items : op_bicubic4_add_items)(co, lr, out, g, h, w, st);
      } else {
        (bi ? op_bilinear4_add : op_bicubic4_add)(co, lr_curr + (size_t)i0 * 3 * lr_px, hr_out + (size_t)i0 * 48 * lr_px, g, h, w, st);
      }
    });
  }
}

void Frvsr::tecogan_tail_taps(const float* body_nchw, const float* lr_curr, float* up1, float* up2, float* hr_out, int n, int h, int w, const TecoTailDev& opts,
                              hipStream_t st) {
  SS4K_REQUIRE(generator == SS4K_FRVSR_TECOGAN, "tail taps: the object is not a TecoGAN generator");
  SS4K_REQUIRE(n > 0 && h > 0 && w > 0 && (double)n * 16.0 * h * w < 2147483648.0, "tail taps: sizes");
  SS4K_REQUIRE(opts.max_workgroups >= 0 && opts.group_items >= 0 && opts.group_items <= SS4K_FRVSR_MAX_STREAMS, "tail taps: max_workgroups >= 0, group_items in 0..64");
  const Tens body = net.act(0, (size_t)n * h * w, desc.num_feat);
  net.pack_in(body_nchw, body, net.planes_for(desc.num_feat), n, desc.num_feat, h, w, 1, st);
  const TecoTailDev was = teco.dev;
  teco.dev = opts; teco.dev.up1 = up1; teco.dev.up2 = up2;
  try { run_teco_tail(body, 1, lr_curr, hr_out, nullptr, n, h, w, st); } catch (...) { teco.dev = was; throw; }
  teco.dev = was;
}

}  // namespace ss4k
