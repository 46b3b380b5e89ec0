// Executor of the frame-recurrent upscaler (EGVSR's FRNet x4, reference src/upscale/model/egvsr/egvsr.py:146-212) and the service path
// around it (src/upscale/egvsr_upscaler.py:172-212).  Every convolution is 3x3 / stride 1 / pad 1 and runs through Model::conv on the conv
// kernels the other networks use; the rest of the network is the glue of frvsr.hip.  Weights arrive as FRNet's state_dict flattened in key order
// (sharkshark-4k_amd/weights.py: frnet_keys).
#include "frvsr.h"

namespace ss4k {

// FNet's convolutions (cout, cin) in state_dict order (egvsr.py:19-61); every one but the last is followed by LeakyReLU(0.2)
static const int FNET_CONVS[14][2] = {{32, 6}, {32, 32}, {64, 32}, {64, 64}, {128, 64}, {128, 128}, {256, 128}, {256, 256},
                                      {128, 256}, {128, 128}, {64, 128}, {64, 64}, {32, 64}, {2, 32}};

static void validate_frvsr_desc(const ss4k_frvsr_desc& d) {
  SS4K_REQUIRE(d.dtype == SS4K_F32 || d.dtype == SS4K_F16, "frvsr desc.dtype must be SS4K_F32 or SS4K_F16");
  SS4K_REQUIRE(d.num_feat > 0 && d.num_feat <= SS4K_DESC_MAX_WIDTH && d.num_feat % 16 == 0, "frvsr: num_feat must be a multiple of 16 in 16..512");
  SS4K_REQUIRE(d.num_feat == 64, "frvsr: SRNet's tail is PixelShuffle(4) + Conv2d(4, 3) (egvsr.py:122-127): num_feat must be 64");
  SS4K_REQUIRE(d.num_block >= 0 && d.num_block <= SS4K_DESC_MAX_BLOCKS, "frvsr: num_block must be in 0..64");
  SS4K_REQUIRE(d.flags == 0, "frvsr desc.flags must be 0");
  for (int r : d.reserved) SS4K_REQUIRE(r == 0, "frvsr desc.reserved must be 0");
}

size_t frvsr_param_count(const ss4k_frvsr_desc& d, int generator, int degradation) {
  try { validate_frvsr_desc(d); } catch (const Error&) { return 0; }
  if (generator != SS4K_FRVSR_EGVSR && generator != SS4K_FRVSR_TECOGAN) return 0;
  if (degradation != SS4K_FRVSR_BD && degradation != SS4K_FRVSR_BI) return 0;
  const size_t nf = (size_t)d.num_feat;
  const size_t kernels = degradation == SS4K_FRVSR_BD ? 16 : 0;     // 'BI': the function is a functools.partial, not a module with a buffer
  size_t n = kernels;                                               // upsample_func.kernels
  for (auto& c : FNET_CONVS) n += (size_t)c[0] * c[1] * 9 + c[0];
  n += nf * 51 * 9 + nf;                                            // srnet.conv_in.0
  n += (size_t)d.num_block * 2 * (nf * nf * 9 + nf);                // srnet.resblocks.*.conv.{0,2}
  n += 2 * (nf * nf * 9 + nf);                                      // srnet.conv_up.{0,2}: in the state_dict; EGVSR's forward does not use them
  n += generator == SS4K_FRVSR_TECOGAN ? 3 * nf * 9 + 3 : 3 * 4 * 9 + 3;   // srnet.conv_out: Conv2d(nf, 3) at (4 h, 4 w) (tecogan_nets.py:128) | Conv2d(4, 3)
  n += kernels;                                                     // srnet.upsample_func.kernels
  return n;
}

void Frvsr::build(const float* w, size_t n) {
  validate_frvsr_desc(desc);
  SS4K_REQUIRE(generator == SS4K_FRVSR_EGVSR || generator == SS4K_FRVSR_TECOGAN, "frvsr: generator must be SS4K_FRVSR_EGVSR or SS4K_FRVSR_TECOGAN");
  SS4K_REQUIRE(degradation == SS4K_FRVSR_BD || degradation == SS4K_FRVSR_BI, "frvsr: degradation must be SS4K_FRVSR_BD or SS4K_FRVSR_BI");
  SS4K_REQUIRE((route_flags & ~(SS4K_FRVSR_CONVT_EMBEDDED | SS4K_FRVSR_CONVT_PHASE)) == 0, "frvsr: unknown route flags");
  SS4K_REQUIRE(route_flags != (SS4K_FRVSR_CONVT_EMBEDDED | SS4K_FRVSR_CONVT_PHASE), "frvsr: the route flags pin one route of the transposed layers, not both");
  SS4K_REQUIRE(generator == SS4K_FRVSR_TECOGAN || route_flags == 0, "frvsr: the route flags belong to the TecoGAN generator");
  SS4K_REQUIRE(n == frvsr_param_count(desc, generator, degradation), "weight blob size does not match the frvsr description");
  const size_t kernels = degradation == SS4K_FRVSR_BD ? 16 : 0;
  net.ctx = ctx;
  net.desc = ss4k_model_desc{}; net.desc.kind = SS4K_SRVGG; net.desc.dtype = desc.dtype; net.desc.scale = 4; net.desc.num_feat = desc.num_feat;
  const int nf = desc.num_feat;
  ParamCursor pc{w, n};
  (void)pc.take(kernels);
  fnet0 = 0;
  for (int i = 0; i < 14; ++i)   // torch.cat([x1, x2], 1) (egvsr.py:67): two input segments of one plane each
    net.add_conv(pc, FNET_CONVS[i][0], FNET_CONVS[i][1], i == 0 ? net.spec_concat(3, 3) : net.spec_plain(FNET_CONVS[i][1]), false);
  srnet0 = (int)net.layers.size();
  net.add_conv(pc, nf, 51, net.spec_concat(3, 48), false);   // torch.cat([lr_curr, hr_prev_tran], 1) (egvsr.py:137)
  for (int i = 0; i < 2 * desc.num_block; ++i) net.add_conv(pc, nf, nf, net.spec_plain(nf), false);
  if (generator == SS4K_FRVSR_TECOGAN) {
    const float* up0 = pc.take((size_t)nf * nf * 9 + nf);
    const float* up2 = pc.take((size_t)nf * nf * 9 + nf);
    build_teco_tail(up0, up2, pc.take((size_t)3 * nf * 9 + 3));
  } else {
    (void)pc.take(2 * ((size_t)nf * nf * 9 + nf));
    const float* tw = pc.take(108);
    std::vector<float> wb(tw, tw + 108);
    const float* b = pc.take(3);
    wb.insert(wb.end(), b, b + 3);
    tail_wb.ensure(wb.size() * 4);
    SS4K_HIP(hipMemcpy(tail_wb.ptr, wb.data(), wb.size() * 4, hipMemcpyHostToDevice));
  }
  (void)pc.take(kernels);
  SS4K_REQUIRE(pc.pos == n, "internal: weight cursor did not consume the blob");
}

Frvsr::~Frvsr() {
  for (auto& s : spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
}

void Frvsr::prof_collect() {
  for (auto& s : spans) {
    float ms = 0.f;
    if (hipEventSynchronize(s.b) == hipSuccess && hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) stage_ms[s.stage] += ms;
    else (void)hipGetLastError();
    (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b);
  }
  spans.clear();
}

size_t Frvsr::workspace_bytes(int n, int h, int w) {
  net.plan_only = true; net.plan_bytes.clear();
  try { step(nullptr, nullptr, nullptr, nullptr, n, h, w, nullptr); } catch (...) { net.plan_only = false; throw; }
  net.plan_only = false;
  size_t total = 0;
  for (size_t b : net.plan_bytes) total += (b + 255) & ~size_t(255);
  const size_t flow_b = (size_t)n * 2 * h * w * 4;
  return total + 2 * ((flow_b + 255) & ~size_t(255));   // flow_raw (sized like flow: at most as large), flow
}

void Frvsr::step(const float* lr_curr, const float* lr_prev, const float* hr_prev, float* hr_out, int n, int h, int w, hipStream_t st) {
  run(lr_curr, lr_prev, hr_prev, hr_out, nullptr, n, h, w, st);
}

void Frvsr::step_items(const Items& items, int n, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS, "frvsr step: 1..64 items that live in buffers of their own");
  SS4K_REQUIRE(items.lr_curr && items.lr_prev && items.hr_prev && items.hr_out, "frvsr step: NULL item table");
  run(nullptr, nullptr, nullptr, nullptr, &items, n, h, w, st);
}

// `items` null: the four contiguous batches; else the per-item pointers (the contiguous arguments are unused)
void Frvsr::run(const float* lr_curr, const float* lr_prev, const float* hr_prev, float* hr_out, const Items* items, int n, int h, int w, hipStream_t st) {
  SS4K_REQUIRE(n > 0, "frvsr step: empty batch");
  SS4K_REQUIRE(h >= 8 && w >= 8, "frvsr step: h and w must be at least 8 (the flow is computed at (h // 8 * 8, w // 8 * 8) and reflect-padded, egvsr.py:191-194)");
  SS4K_REQUIRE((double)n * 16.0 * h * w < 2147483648.0, "frvsr step: the output of a call holds at most 2^31 pixels per plane");
  const bool plan = net.plan_only, bi = degradation == SS4K_FRVSR_BI;
  const int dt = desc.dtype;
  const int h1 = h / 2, w1 = w / 2, h2 = h1 / 2, w2 = w1 / 2, h3 = h2 / 2, w3 = w2 / 2, h8 = 8 * h3, w8 = 8 * w3;
  const size_t px = (size_t)n * h * w, px1 = (size_t)n * h1 * w1, px2 = (size_t)n * h2 * w2, px3 = (size_t)n * h3 * w3;
  auto stage = [&](int s, auto&& body) { timed(s, st, body); };
  auto lrelu = [](const Tens& out, float slope) { ConvOpts o; o.act = ACT_LRELU; o.slope = slope; o.out = out; return o; };
  auto pool = [&](const Tens& in, const Tens& out, int channels, int H, int W) {
    if (!plan) SS4K_PLANES_T(dt, op_maxpool2_planes((const T*)in.p, (T*)out.p, channels / 16, n, H, W, st));
  };
  auto up2 = [&](const Tens& in, const Tens& out, int channels, int H, int W) {
    if (!plan) SS4K_PLANES_T(dt, op_bilinear2_planes((const T*)in.p, (T*)out.p, channels / 16, n, H, W, st));
  };
  int slot = 0;
  auto act = [&](size_t pixels, int channels) { return net.act(slot++, pixels, channels); };

  // ---- inputs: lr_curr and lr_prev as one 16-channel plane each (channels 0..2 live)
  Tens A = net.act_planes(slot++, px, 1), B = net.act_planes(slot++, px, 1);
  stage(FRV_GLUE, [&] {
    if (!items) {
      net.pack_in(lr_curr, A, 1, n, 3, h, w, 1, st);
      net.pack_in(lr_prev, B, 1, n, 3, h, w, 1, st);
    } else if (plan) {
      return;
    } else if (items->pack_batched) {
      FrvsrPtrs c{}, p{};
      for (int i = 0; i < n; ++i) { c.p[i] = const_cast<float*>(items->lr_curr[i]); p.p[i] = const_cast<float*>(items->lr_prev[i]); }
      SS4K_PLANES_T(dt, op_pack_lr_items(c, p, (T*)A.p, (T*)B.p, n, h, w, st));
    } else {   // item i's pixels are one contiguous run of the single plane
      const size_t item_b = (size_t)h * w * conv_rec_bytes(dt);
      for (int i = 0; i < n; ++i) {
        net.pack_in(items->lr_curr[i], Tens{A.p + i * item_b, A.plane_bytes, 0}, 1, 1, 3, h, w, 1, st);
        net.pack_in(items->lr_prev[i], Tens{B.p + i * item_b, B.plane_bytes, 0}, 1, 1, 3, h, w, 1, st);
      }
    }
  });

  // ---- FNet (egvsr.py:63-78)
  int li = fnet0;
  Tens e1a = act(px, 32), e1b = act(px, 32), p1 = act(px1, 32);
  Tens e2a = act(px1, 64), e2b = act(px1, 64), p2 = act(px2, 64);
  Tens e3a = act(px2, 128), e3b = act(px2, 128), p3 = act(px3, 128);
  Tens d1a = act(px3, 256), d1b = act(px3, 256), u1 = act(px3 * 4, 256);
  Tens d2a = act(px3 * 4, 128), d2b = act(px3 * 4, 128), u2 = act(px3 * 16, 128);
  Tens d3a = act(px3 * 16, 64), d3b = act(px3 * 16, 64), u3 = act(px3 * 64, 64);
  Tens f0 = act(px3 * 64, 32);
  const size_t flow_raw_b = (size_t)n * 2 * h8 * w8 * 4, flow_b = (size_t)n * 2 * h * w * 4;
  if (!plan) { flow_raw.ensure(flow_raw_b); flow.ensure(flow_b); }
  auto two = [&](const Tens& in0, const Tens* in1, const Tens& mid, const Tens& out, int H, int W) {
    stage(FRV_FNET_CONV, [&] {
      net.conv(li++, in0, in1, n, H, W, lrelu(mid, 0.2f), st);
      net.conv(li++, mid, nullptr, n, H, W, lrelu(out, 0.2f), st);
    });
  };
  two(A, &B, e1a, e1b, h, w);
  stage(FRV_POOL_UP, [&] { pool(e1b, p1, 32, h, w); });
  two(p1, nullptr, e2a, e2b, h1, w1);
  stage(FRV_POOL_UP, [&] { pool(e2b, p2, 64, h1, w1); });
  two(p2, nullptr, e3a, e3b, h2, w2);
  stage(FRV_POOL_UP, [&] { pool(e3b, p3, 128, h2, w2); });
  two(p3, nullptr, d1a, d1b, h3, w3);
  stage(FRV_POOL_UP, [&] { up2(d1b, u1, 256, h3, w3); });
  two(u1, nullptr, d2a, d2b, 2 * h3, 2 * w3);
  stage(FRV_POOL_UP, [&] { up2(d2b, u2, 128, 2 * h3, 2 * w3); });
  two(u2, nullptr, d3a, d3b, 4 * h3, 4 * w3);
  stage(FRV_POOL_UP, [&] { up2(d3b, u3, 64, 4 * h3, 4 * w3); });
  stage(FRV_FNET_CONV, [&] {
    net.conv(li++, u3, nullptr, n, h8, w8, lrelu(f0, 0.2f), st);
    ConvOpts o; o.epi = EPI_NCHW_F32; o.out = Tens{flow_raw.as<char>(), 0, 0};   // the raw flow leaves the network as fp32 NCHW (n, 2, h8, w8)
    net.conv(li++, f0, nullptr, n, h8, w8, o, st);
  });
  // tanh * 24 (egvsr.py:76), reflect pad to (h, w) (:191-194)
  stage(FRV_FLOW, [&] { if (!plan) op_flow_finish(flow_raw.as<float>(), flow.as<float>(), n, h8, w8, h, w, st); });

  // ---- hr_flow = 4 * BicubicUpsample(4)(lr_flow), backward_warp(hr_prev, hr_flow), space-to-depth (egvsr.py:196-208): one launch, three planes.
  // Degradation 'BI': the same stage with F.interpolate(scale_factor=4, 'bilinear') of the flow (utils/net_utils.py:96-108; frvsr_bi.hip)
  Tens Wp = net.act_planes(slot++, px, 3);
  stage(FRV_WARP, [&] {
    if (plan) return;
    const float* fl = flow.as<float>();
    if (items && bi) SS4K_PLANES_T(dt, op_warp_s2d_bi_planes_items(fl, *items->hr_prev, (T*)Wp.p, n, h, w, st));
    else if (items) SS4K_PLANES_T(dt, op_warp_s2d_planes_items(fl, *items->hr_prev, (T*)Wp.p, n, h, w, st));
    else if (bi) SS4K_PLANES_T(dt, op_warp_s2d_bi_planes(fl, hr_prev, (T*)Wp.p, n, h, w, st));
    else SS4K_PLANES_T(dt, op_warp_s2d_planes(fl, hr_prev, (T*)Wp.p, n, h, w, st));
  });
  if (keep_taps && !plan) {
    tap_s2d.ensure(px * 48 * 4);
    SS4K_PLANES_T(dt, op_planes_to_nchw((const T*)Wp.p, tap_s2d.as<float>(), n, 48, h, w, st));
  }

  // ---- SRNet (egvsr.py:132-143): ReLU is LeakyReLU with slope 0; a residual block's skip is res1 with alpha = 1
  const int nf = desc.num_feat;
  li = srnet0;
  Tens x0 = act(px, nf), t = act(px, nf), x1 = act(px, nf);
  Tens cur = x0, nxt = x1;
  stage(FRV_SRNET_CONV, [&] {
    net.conv(li++, A, &Wp, n, h, w, lrelu(x0, 0.f), st);
    for (int b = 0; b < desc.num_block; ++b) {
      net.conv(li++, cur, nullptr, n, h, w, lrelu(t, 0.f), st);
      ConvOpts o; o.res1 = &cur; o.out = nxt;
      net.conv(li++, t, nullptr, n, h, w, o, st);
      std::swap(cur, nxt);
    }
    net.lanes_join(st, true);   // (closes the context's conv profiling section if one is open; a step never forks)
  });
  if (generator == SS4K_FRVSR_TECOGAN) { run_teco_tail(cur, slot, lr_curr, hr_out, items, n, h, w, st); return; }   // (stages of its own: frvsr_teco.cpp)
  // PixelShuffle(4), ReLU, conv_out (egvsr.py:139-140)
  stage(FRV_TAIL, [&] {
    if (plan) return;
    if (items) SS4K_PLANES_T(dt, op_ps4_conv_tail_items((const T*)cur.p, tail_wb.as<float>(), *items->hr_out, n, h, w, st));
    else SS4K_PLANES_T(dt, op_ps4_conv_tail((const T*)cur.p, tail_wb.as<float>(), hr_out, n, h, w, st));
  });
}

// ------------------------------------------------------------------------------------------ the service path
void FrvsrUpscaler::out_shape(int* oh, int* ow) const {
  *oh = out_h > 0 ? out_h : 4 * lr_h; *ow = out_w > 0 ? out_w : 4 * lr_w;
}

size_t FrvsrUpscaler::state_bytes() const {
  size_t b = 0;
  for (const Slot& s : slots) b += s.lr[0].bytes + s.lr[1].bytes + s.hr[0].bytes + s.hr[1].bytes;
  return b;
}

void FrvsrUpscaler::check_round(const int32_t* slot_ids, int S, int h, int w, bool area_chain) const {
  SS4K_REQUIRE(S >= 1 && S <= (int)slots.size(), "frvsr round: n_streams must be in 1..max_streams");
  SS4K_REQUIRE(h > 0 && w > 0, "frvsr round: empty frames");
  bool seen[SS4K_FRVSR_MAX_STREAMS] = {};
  for (int i = 0; i < S; ++i) {
    SS4K_REQUIRE(slot_ids[i] >= 0 && slot_ids[i] < (int)slots.size(), "frvsr round: slot outside 0..max_streams-1");
    SS4K_REQUIRE(!seen[slot_ids[i]], "frvsr round: a slot is named twice (a round holds ONE frame per stream)");
    seen[slot_ids[i]] = true;
  }
  SS4K_REQUIRE((double)S * 16.0 * lr_h * lr_w < 2147483648.0, "frvsr round: the output of a round holds at most 2^31 pixels per plane");
  if (area_chain) {   // round()'s per-item chains resize with op_area, whose grid holds one block row per output row (glue.hip: "area: grid limits")
    int oh, ow; out_shape(&oh, &ow);
    SS4K_REQUIRE((h == lr_h && w == lr_w) || lr_h <= 65535, "frvsr round: frames are resized to an lr_shape of at most 65535 rows");
    SS4K_REQUIRE((oh == 4 * lr_h && ow == 4 * lr_w) || oh <= 65535, "frvsr round: the output is resized to at most 65535 rows");
  }
}

// the first change of any slot in a round: every item's state buffers exist, a stream's first frame sees zeros, and the round's tables point at them
void FrvsrUpscaler::open_slots(const int32_t* slot_ids, int S, hipStream_t st, RoundPtrs& r) {
  const size_t lr_b = (size_t)3 * lr_h * lr_w * 4, hr_b = (size_t)3 * 16 * lr_h * lr_w * 4;
  for (int i = 0; i < S; ++i) {
    Slot& s = slots[slot_ids[i]];
    for (int k = 0; k < 2; ++k) { s.lr[k].ensure(lr_b); s.hr[k].ensure(hr_b); }
    if (!s.have_state) {   // self.lr_prev = zeros_like(lr_curr), self.hr_prev = zeros (egvsr_upscaler.py:197-202)
      SS4K_HIP(hipMemsetAsync(s.lr[s.cur].ptr, 0, lr_b, st));
      SS4K_HIP(hipMemsetAsync(s.hr[s.cur].ptr, 0, hr_b, st));
      s.have_state = true;
    }
    r.lr_prev[i] = s.lr[s.cur].as<float>(); r.lr_curr[i] = r.lr_dst.p[i] = s.lr[s.cur ^ 1].as<float>();
    r.hr_prev.p[i] = s.hr[s.cur].as<float>(); r.hr_curr.p[i] = s.hr[s.cur ^ 1].as<float>();
  }
  m->keep_taps = taps_on;
}

// after the step: the state takes the UNCLAMPED output (:206-207); the taps describe the round's last item
void FrvsrUpscaler::close_slots(const int32_t* slot_ids, int S) {
  for (int i = 0; i < S; ++i) slots[slot_ids[i]].cur ^= 1;
  m->keep_taps = false;
  if (taps_on) {
    const int d[4][4] = {{1, 3, lr_h, lr_w}, {1, 2, lr_h, lr_w}, {1, 48, lr_h, lr_w}, {1, 3, 4 * lr_h, 4 * lr_w}};
    std::memcpy(tap_dims, d, sizeof(d));
    tap_slot = slot_ids[S - 1]; tap_item = S - 1;
  }
}

void FrvsrUpscaler::round(const uint8_t* in, const int32_t* slot_ids, int S, int h, int w, uint8_t* out, hipStream_t st) {
  check_round(slot_ids, S, h, w, true);   // every refusal comes before the first change of any slot
  const int H = 4 * lr_h, W = 4 * lr_w;
  int oh, ow; out_shape(&oh, &ow);
  const size_t hr_b = (size_t)3 * H * W * 4;
  const bool resize_in = h != lr_h || w != lr_w, resize_out = oh != H || ow != W;
  RoundPtrs r{};
  open_slots(slot_ids, S, st, r);
  m->timed(FRV_GLUE, st, [&] {
    for (int i = 0; i < S; ++i) {
      const uint8_t* frame = in + (size_t)i * h * w * 3;
      float* dst = r.lr_dst.p[i];
      if (resize_in) {   // img / 255.0, F.interpolate(img, size=self.lr_shape, mode='area') (egvsr_upscaler.py:195-196)
        img.ensure((size_t)3 * h * w * 4);
        op_u8nhwc_to_f32nchw(frame, img.as<float>(), 1, h, w, 3, st);
        op_area(img.as<float>(), dst, 3, h, w, lr_h, lr_w, st);
      } else {
        op_u8nhwc_to_f32nchw(frame, dst, 1, h, w, 3, st);
      }
    }
  });
  // (:204) one stream: the contiguous launchers, as before there were slots; several: the same step with every item's state where it lives
  if (S == 1) m->step(r.lr_curr[0], r.lr_prev[0], r.hr_prev.p[0], r.hr_curr.p[0], 1, lr_h, lr_w, st);
  else m->step_items(Frvsr::Items{r.lr_curr, r.lr_prev, &r.hr_prev, &r.hr_curr}, S, lr_h, lr_w, st);
  close_slots(slot_ids, S);
  m->timed(FRV_GLUE, st, [&] {
    for (int i = 0; i < S; ++i) {
      uint8_t* dst = out + (size_t)i * oh * ow * 3;
      if (resize_out) {   // clamp(hr_curr, 0, 1), F.interpolate(size=self.output_shape, mode='area') (:209-211)
        hrc.ensure(hr_b); outf.ensure((size_t)3 * oh * ow * 4);
        op_clamp01_to(r.hr_curr.p[i], hrc.as<float>(), (size_t)3 * H * W, st);
        op_area(hrc.as<float>(), outf.as<float>(), 3, H, W, oh, ow, st);
        op_f32nchw_to_u8nhwc(outf.as<float>(), dst, 1, 3, oh, ow, st);
      } else {
        op_f32nchw_to_u8nhwc(r.hr_curr.p[i], dst, 1, 3, H, W, st);   // (clamps, * 255, truncates: :209,212)
      }
    }
  });
}

void FrvsrUpscaler::round_at(const uint8_t* const* in, const int32_t* slot_ids, int S, int h, int w, uint8_t* const* out, hipStream_t st) {
  check_round(slot_ids, S, h, w, false);
  const int H = 4 * lr_h, W = 4 * lr_w;
  int oh, ow; out_shape(&oh, &ow);
  // what the two frame kernels' launchers would refuse is refused here, before the first change of any slot
  SS4K_REQUIRE((double)h * lr_h < 2147483648.0 && (double)w * lr_w < 2147483648.0 && (double)H * oh < 2147483648.0 && (double)W * ow < 2147483648.0,
               "frvsr round: frame sizes whose area window bounds overflow");
  FrvsrFramesIn fin{}; FrvsrFramesOut fout{};
  for (int i = 0; i < S; ++i) {
    SS4K_REQUIRE(in[i] && out[i], "frvsr round: NULL frame pointer");
    fin.p[i] = in[i]; fout.p[i] = out[i];
  }
  RoundPtrs r{};
  open_slots(slot_ids, S, st, r);
  m->timed(FRV_GLUE, st, [&] { op_frames_in_items(fin, r.lr_dst, S, h, w, lr_h, lr_w, st); });
  // always the item launchers, S = 1 included: they are bit-identical to the contiguous ones, and the packing is one launch for the round
  m->step_items(Frvsr::Items{r.lr_curr, r.lr_prev, &r.hr_prev, &r.hr_curr, true}, S, lr_h, lr_w, st);
  close_slots(slot_ids, S);
  m->timed(FRV_GLUE, st, [&] { op_frames_out_items(r.hr_curr, fout, S, H, W, oh, ow, st); });
}

void FrvsrUpscaler::frames(const uint8_t* in, int n, int h, int w, uint8_t* out, hipStream_t st) {
  int oh, ow; out_shape(&oh, &ow);
  const int32_t slot0 = 0;
  for (int i = 0; i < n; ++i) round(in + (size_t)i * h * w * 3, &slot0, 1, h, w, out + (size_t)i * oh * ow * 3, st);
}

}  // namespace ss4k
