// The tail of TecoGAN's frame-recurrent generator (reference src/upscale/model/egvsr/models/networks/tecogan_nets.py:101-149, the FRNet
// EGVSR's was cut down from): after the last residual block
//   conv_up  = ConvTranspose2d(64, 64, 3, 2, 1, output_padding=1), ReLU, the same again        (h, w) -> (2 h, 2 w) -> (4 h, 4 w)
//   conv_out = Conv2d(64, 3, 3, 1, 1)                                                           at (4 h, 4 w)
//   out     += BicubicUpsample(4)(lr_curr)                                                      degradation 'BD'
//   out     += F.interpolate(lr_curr, scale_factor=4, 'bilinear', align_corners=False)          degradation 'BI' (frvsr_bi.hip)
// Everything before it is Frvsr::run (frvsr.cpp), which calls this through FrvsrTail.  The file holds the tail together with every launcher
// it names beyond Model::conv, so that frvsr.cpp links wherever it linked before.
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

namespace {

struct TecoTail final : FrvsrTail {
  bool embedded = false;
  bool bilinear = false;                        // degradation 'BI': the skip is op_bilinear4_add[_items]
  int up_layer[2] = {-1, -1}, out_layer = -1;   // embedded route: the W_eq layers of f.net
  DevBuf up_w[2], up_b[2];                      // phase route: pack_convt3x3s2's blob and the 64 biases
  TecoTailDev dev{};

  void build(Frvsr& f, const float* up0, const float* up2, const float* out_w) override {
    const int nf = f.desc.num_feat;
    const float* up[2] = {up0, up2};
    for (int k = 0; k < 2; ++k) {
      if (embedded) {
        const std::vector<float> eq = embed_convt(up[k], nf);
        ParamCursor pc{eq.data(), eq.size()};
        up_layer[k] = f.net.add_conv(pc, 4 * nf, nf, f.net.spec_plain(nf, 1), false);
      } else {
        SS4K_REQUIRE(nf == 64, "tecogan tail: the phase kernel is built for 64 channels");
        const std::vector<uint8_t> pk = pack_convt3x3s2(up[k], f.desc.dtype);
        up_w[k].ensure(pk.size()); up_b[k].ensure((size_t)nf * 4);
        SS4K_HIP(hipMemcpy(up_w[k].ptr, pk.data(), pk.size(), hipMemcpyHostToDevice));
        SS4K_HIP(hipMemcpy(up_b[k].ptr, up[k] + (size_t)nf * nf * 9, (size_t)nf * 4, hipMemcpyHostToDevice));
        f.net.weight_bytes += pk.size() + (size_t)nf * 4;
      }
    }
    ParamCursor pc{out_w, (size_t)3 * nf * 9 + 3};
    out_layer = f.net.add_conv(pc, 3, nf, f.net.spec_plain(nf), false);   // (an fp16 model: also conv_w16n.hip's blob)
  }

  // items of one group: no plane of the (4 h, 4 w) tensors reaches 2^32 bytes
  static int default_group(const Frvsr& f, int n, int h, int w) {
    const double item = 16.0 * h * w * conv_rec_bytes(f.desc.dtype);
    return (int)std::max(1.0, std::min((double)n, std::floor(4294967295.0 / item)));
  }

  void run(Frvsr& f, const Call& c, hipStream_t st) override {
    Model& net = f.net;
    const bool plan = net.plan_only, f16 = f.desc.dtype == SS4K_F16;
    const int nf = f.desc.num_feat, n = c.n, h = c.h, w = c.w;
    SS4K_REQUIRE(dev.group_items >= 0 && dev.group_items <= SS4K_FRVSR_MAX_STREAMS, "tecogan tail: group_items must be in 0..64");
    const int G = std::min({n, dev.group_items > 0 ? dev.group_items : default_group(f, n, h, w), (int)SS4K_FRVSR_MAX_STREAMS});
    const size_t lr_px = (size_t)h * w, rec = (size_t)net.rec();
    int slot = c.slot;
    const Tens U1G = net.act(slot++, (size_t)G * 4 * lr_px, nf), U2G = net.act(slot++, (size_t)G * 16 * lr_px, nf);
    // conv_out's fp32 NCHW result (G, 3, 4 h, 4 w): 12 bytes per HR pixel in a slot of one plane (a record is 32 or 64)
    const Tens CO = net.act_planes(slot++, (size_t)G * 16 * lr_px, 1);
    auto relu = [](const Tens& out) { ConvOpts o; o.act = ACT_LRELU; o.slope = 0.f; o.epi = EPI_NHWC_PS2; o.out = out; return o; };
    for (int i0 = 0; i0 < n; i0 += G) {
      const int g = std::min(G, n - i0);
      // the group's tensors: planes of exactly g items at the head of the buffers (a short last group packs its planes closer)
      const Tens U1{U1G.p, (size_t)g * 4 * lr_px * rec, 0}, U2{U2G.p, (size_t)g * 16 * lr_px * rec, 0};
      const Tens body{c.body.p + (plan ? 0 : (size_t)i0 * lr_px * rec), c.body.plane_bytes, c.body.plane0};   // items i0 .. i0 + g of every plane
      f.timed(FRV_CONVT, st, [&] {
        if (embedded) {
          net.conv(up_layer[0], body, nullptr, g, h, w, relu(U1), st);
          net.conv(up_layer[1], U1, nullptr, g, 2 * h, 2 * w, relu(U2), st);
        } else if (!plan) {
          const ConvtArgs a1{body.p + (size_t)body.plane0 * body.plane_bytes, body.plane_bytes, U1.p, U1.plane_bytes, up_w[0].as<char>(), up_b[0].as<float>(), g, h, w, 0, 0};
          launch_convt3x3s2(f.ctx, a1, f.desc.dtype, dev.max_workgroups, st);
          const ConvtArgs a2{U1.p, U1.plane_bytes, U2.p, U2.plane_bytes, up_w[1].as<char>(), up_b[1].as<float>(), g, 2 * h, 2 * w, 0, 0};
          launch_convt3x3s2(f.ctx, a2, f.desc.dtype, dev.max_workgroups, st);
        }
      });
      if (!plan && dev.up1) {
        float* t1 = dev.up1 + (size_t)i0 * nf * 4 * lr_px; float* t2 = dev.up2 + (size_t)i0 * nf * 16 * lr_px;
        if (f16) {
          op_planes_to_nchw<__half>(reinterpret_cast<const __half*>(U1.p), t1, g, nf, 2 * h, 2 * w, st);
          op_planes_to_nchw<__half>(reinterpret_cast<const __half*>(U2.p), t2, g, nf, 4 * h, 4 * w, st);
        } else {
          op_planes_to_nchw<float>(reinterpret_cast<const float*>(U1.p), t1, g, nf, 2 * h, 2 * w, st);
          op_planes_to_nchw<float>(reinterpret_cast<const float*>(U2.p), t2, g, nf, 4 * h, 4 * w, st);
        }
      }
      f.timed(FRV_CONV_OUT, st, [&] {
        ConvOpts o; o.epi = EPI_NCHW_F32; o.out = Tens{CO.p, 0, 0};
        net.conv(out_layer, U2, nullptr, g, 4 * h, 4 * w, o, st);
        net.lanes_join(st, true);
      });
      f.timed(FRV_SKIP, st, [&] {
        if (plan) return;
        const float* co = reinterpret_cast<const float*>(CO.p);
        if (c.items_lr) {
          FrvsrPtrs lr{}, out{};
          for (int i = 0; i < g; ++i) { lr.p[i] = const_cast<float*>(c.items_lr[i0 + i]); out.p[i] = c.items_out->p[i0 + i]; }
          if (bilinear) op_bilinear4_add_items(co, lr, out, g, h, w, st);
          else op_bicubic4_add_items(co, lr, out, g, h, w, st);
        } else if (bilinear) {
          op_bilinear4_add(co, c.lr_curr + (size_t)i0 * 3 * lr_px, c.hr_out + (size_t)i0 * 48 * lr_px, g, h, w, st);
        } else {
          op_bicubic4_add(co, c.lr_curr + (size_t)i0 * 3 * lr_px, c.hr_out + (size_t)i0 * 48 * lr_px, g, h, w, st);
        }
      });
    }
  }
};

}  // namespace

std::unique_ptr<FrvsrTail> make_tecogan_tail(int route_flags, int degradation) {
  SS4K_REQUIRE(degradation == SS4K_FRVSR_BD || degradation == SS4K_FRVSR_BI, "frvsr: degradation must be SS4K_FRVSR_BD or SS4K_FRVSR_BI");
  SS4K_REQUIRE((route_flags & ~(SS4K_FRVSR_CONVT_EMBEDDED | SS4K_FRVSR_CONVT_PHASE)) == 0, "frvsr: unknown route flags");
  SS4K_REQUIRE(route_flags != (SS4K_FRVSR_CONVT_EMBEDDED | SS4K_FRVSR_CONVT_PHASE), "frvsr: the transposed layers take one route");
  auto t = std::make_unique<TecoTail>();
  t->bilinear = degradation == SS4K_FRVSR_BI;
  t->embedded = !(route_flags & SS4K_FRVSR_CONVT_PHASE);   // unpinned: the embedded route, the faster one as measured
  return t;
}

void tecogan_tail_taps(Frvsr& f, const float* body_nchw, const float* lr_curr, float* up1, float* up2, float* hr_out, int n, int h, int w,
                       const TecoTailDev& opts, hipStream_t st) {
  TecoTail* t = dynamic_cast<TecoTail*>(f.tail.get());
  SS4K_REQUIRE(t, "tail taps: the object is not a TecoGAN generator");
  SS4K_REQUIRE(n > 0 && h > 0 && w > 0 && (double)n * 16.0 * h * w < 2147483648.0, "tail taps: sizes");
  SS4K_REQUIRE(opts.max_workgroups >= 0 && opts.group_items >= 0 && opts.group_items <= SS4K_FRVSR_MAX_STREAMS, "tail taps: max_workgroups >= 0, group_items in 0..64");
  const Tens body = f.net.act(0, (size_t)n * h * w, f.desc.num_feat);
  f.net.pack_in(body_nchw, body, f.net.planes_for(f.desc.num_feat), n, f.desc.num_feat, h, w, 1, st);
  const TecoTailDev was = t->dev;
  t->dev = opts; t->dev.up1 = up1; t->dev.up2 = up2;
  try { t->run(f, FrvsrTail::Call{body, 1, lr_curr, hr_out, nullptr, nullptr, n, h, w}, st); } catch (...) { t->dev = was; throw; }
  t->dev = was;
}

}  // namespace ss4k
