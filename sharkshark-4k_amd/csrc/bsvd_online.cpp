// Executor of the online BSVD machine (bsvd_online.h): runs the plan of bsvd_online_plan.h through the held model's conv layers.
// One launch chain per push: every BiBufferConv joins the frames of its window anyway.
#include "bsvd_online.h"

namespace ss4k {

using namespace bsvd_online;

void BsvdOnline::create(ss4k_ctx* c, Model* m, int max_push_) {
  SS4K_REQUIRE(c && m, "bsvd online: NULL argument");
  SS4K_REQUIRE(m->desc.kind == SS4K_BSVD && m->desc.bsvd_stream == 1, "bsvd online: the model must be BSVD built with bsvd_stream = 1");
  SS4K_REQUIRE(max_push_ >= 1 && max_push_ <= BSVD_ONLINE_MAX_PUSH, "bsvd online: max_push must be in 1..64");
  ctx = c; net = m; max_push = max_push_;
}

int BsvdOnline::channels_of(int b, int c) const {
  const ss4k_model_desc& d = net->desc;
  switch (c) {
    case C_IN: return b == 0 ? 4 : d.bsvd_mid_ch;
    case C_X0: return d.bsvd_chns[0];
    case C_D0: case C_MA: case C_X1: case C_S1: case C_MA2: return d.bsvd_chns[1];
    default: return d.bsvd_chns[2];
  }
}
// the planes a producer writes (Model::act's rule); the packed network input is one plane
int BsvdOnline::planes_of(int b, int c) const {
  return b == 0 && c == C_IN ? net->planes_for(4) : net->planes_for(cout_pad_of(channels_of(b, c)));
}
size_t BsvdOnline::frame_bytes(int c) const {
  const int r = CARRIED[c].res;
  return (size_t)(h >> r) * (w >> r) * net->rec();
}

size_t BsvdOnline::state_bytes() const {
  size_t t = 0;
  for (auto& blk : carried) for (auto& pr : blk) for (auto& b : pr) t += b.bytes;
  return t + flag_ring.bytes;
}
size_t BsvdOnline::state_bytes_for(int hh, int ww) const {
  size_t t = 0;
  for (int b = 0; b < 2; ++b)
    for (int c = 0; c < C_COUNT; ++c) {
      const int r = CARRIED[c].res;
      const size_t need = (size_t)planes_of(b, c) * cap_frames(c) * (size_t)(hh >> r) * (ww >> r) * net->rec();
      t += 2 * ((need + 255) & ~size_t(255));
    }
  return t;
}

void BsvdOnline::ensure_state() {
  for (int b = 0; b < 2; ++b)
    for (int c = 0; c < C_COUNT; ++c)
      for (int k = 0; k < 2; ++k) carried[b][c][k].ensure((size_t)planes_of(b, c) * cap_frames(c) * frame_bytes(c));
}

// the flags of stream frames first .. first + n - 1 into the ring (NULL: zeros), in at most two pieces where the run wraps
void BsvdOnline::ring_write(const uint32_t* cuts_dev, int first, int n, hipStream_t st) {
  uint32_t* ring = flag_ring.as<uint32_t>();
  for (int done = 0; done < n;) {
    const int at = (first + done) & (BSVD_ONLINE_CUT_RING - 1), k = std::min(n - done, BSVD_ONLINE_CUT_RING - at);
    if (cuts_dev) SS4K_HIP(hipMemcpyAsync(ring + at, cuts_dev + done, (size_t)k * 4, hipMemcpyDeviceToDevice, st));
    else SS4K_HIP(hipMemsetAsync(ring + at, 0, (size_t)k * 4, st));
    done += k;
  }
}

int BsvdOnline::push(const float* in, int n, int hh, int ww, float* out, size_t out_capacity_frames, hipStream_t st, const uint32_t* cuts_dev) {
  // every refusal before the first launch and before any state or counter changes
  SS4K_REQUIRE(net, "bsvd online: not created");
  SS4K_REQUIRE(in && out, "bsvd online push: NULL argument");
  SS4K_REQUIRE(n > 0 && n <= max_push, "bsvd online push: n must be in 1..max_push");
  SS4K_REQUIRE(hh > 0 && ww > 0 && hh % 4 == 0 && ww % 4 == 0, "bsvd online push: frame size must be divisible by 4");
  SS4K_REQUIRE(h == 0 || (hh == h && ww == w), "bsvd online push: frame size differs from the stream's first push (flush or reset first)");
  SS4K_REQUIRE((double)(LAG / 2 + max_push) * hh * ww < 2147483648.0, "bsvd online push: a carried plane holds at most 2^31 pixels");
  const Plan p = make_plan(state, n, false);
  SS4K_REQUIRE(out_capacity_frames >= (size_t)p.emitted, "bsvd online push: output capacity below the frames that become ready");
  SS4K_REQUIRE(!cuts_dev || ((uintptr_t)cuts_dev & 3) == 0, "bsvd online push: the cut flags are 32-bit words");
  const bool first = h == 0, cuts_before = cuts_live;
  h = hh; w = ww;
  try {
    ensure_state();
    if (cuts_dev && !cuts_live) {   // the stream's first flags: from here on it runs the cut-aware shift
      flag_ring.ensure((size_t)BSVD_ONLINE_CUT_RING * 4);
      SS4K_HIP(hipMemsetAsync(flag_ring.ptr, 0, (size_t)BSVD_ONLINE_CUT_RING * 4, st));
      cuts_live = true;
    }
    if (cuts_live) ring_write(cuts_dev, state.pushed, n, st);   // (a push without flags still retires the slots of frames 128 back)
    run(p, in, out, st);
  } catch (...) {
    if (first) { h = w = 0; }
    cuts_live = cuts_before;
    throw;
  }
  state = p.after;
  return p.emitted;
}

int BsvdOnline::flush(float* out, size_t out_capacity_frames, hipStream_t st) {
  SS4K_REQUIRE(net, "bsvd online: not created");
  const int left = pending();
  SS4K_REQUIRE(left == 0 || out, "bsvd online flush: NULL argument");
  SS4K_REQUIRE(out_capacity_frames >= (size_t)left, "bsvd online flush: output capacity below the pending frames");
  int done = 0;
  try {
    for (int calls = flush_calls(state); calls > 0;) {
      const int k = std::min(calls, max_push);
      const Plan p = make_plan(state, k, true);
      run(p, nullptr, out + (size_t)done * 3 * h * w, st);
      state = p.after; done += p.emitted; calls -= k;
    }
  } catch (...) { reset(); throw; }   // a flush that failed half way has no stream left to continue
  reset();
  return done;
}

void BsvdOnline::run(const Plan& p, const float* in, float* out, hipStream_t st) {
  Model& m = *net;
  const ss4k_model_desc& d = m.desc;
  const int c0 = d.bsvd_chns[0], c1 = d.bsvd_chns[1], c2 = d.bsvd_chns[2];
  const int rec = m.rec();
  // one launch chain (Model::launch_lanes: no fork unless a forward set two lanes for this n)
  m.cur_lanes = 1; m.cur_n = 0; m.forked = false;
  BsvdCarryTable tab{}; int entries = 0;
  int dims[3][2] = {{h, w}, {h / 2, w / 2}, {h / 4, w / 4}};

  for (int b = 0; b < 2; ++b) {
    const int L = b * BLOCK_LAG;
    auto win = [&](int j) { return p.win[L + j]; };
    // carried tensor c of block bb (this block's, or - for block 0's output - the next block's input) at stream frame f
    auto at = [&](int bb, int c, int f) {
      const size_t fb = frame_bytes(c);
      return Tens{carried[bb][c][cur[bb][c]].as<char>() + (size_t)p.slot_of(bb, c, f) * fb, (size_t)cap_frames(c) * fb, 0};
    };
    auto relu6 = [&](Tens outT) { ConvOpts o; o.act = ACT_RELU6; o.out = outT; return o; };
    // transient tensors live in the model's activation slots, numbered as Model::forward numbers them: never larger than the clip's
    auto scratch = [&](int idx, int res, int frames, int channels) { return m.act(idx, (size_t)frames * dims[res][0] * dims[res][1], channels); };
    // layers of a DenBlock in state_dict order (models.cpp: bsvd_denblock_shapes)
    enum { INC0 = 0, INC3, DOWNC0, MEM1, MEM2, DOWNC1, MEM3, MEM4, MEM5, MEM6, UPC2, MEM7, MEM8, UPC1, OUTC0, OUTC3 };
    static const int MEM_LAYER[BLOCK_LAG] = {MEM1, MEM2, MEM3, MEM4, MEM5, MEM6, MEM7, MEM8};
    const int l0 = b * 16;
    // BiBufferConv k of the block (1..8) + ReLU6: its carried input -> outT, the frames of win(k)
    auto bibuf = [&](int k, int c, const Tens& outT) {
      const int src = BIBUF_INPUT[k - 1], res = CARRIED[src].res, H = dims[res][0], W = dims[res][1];
      const Window wo = win(k), wi = win(k - 1);
      const int N = wo.count();
      if (N == 0) return;
      const int lead = m.shifted_planes(c);
      Tens S = m.act(14, (size_t)N * H * W, lead * m.cw());
      const Tens centre = at(b, src, wo.lo);
      const int n_next = std::max(0, std::min(N, wi.hi - 1 - wo.lo));   // output frames whose t + 1 the input holds
      SS4K_REQUIRE(n_next == N || p.flushing, "internal: a BiBufferConv would run ahead of its input");
      if (cuts_live)
        op_bsvd_online_shift_cuts(carried[b][src][cur[b][src]].ptr, S.p, lead, cap_frames(src), p.slot_of(b, src, wo.lo), N, (size_t)H * W, rec / 16,
                                  m.cw(), c / 8, wo.lo > 0 ? 1 : 0, n_next, flag_ring.as<uint32_t>(), BSVD_ONLINE_CUT_RING - 1, wo.lo, st);
      else
        op_bsvd_online_shift(carried[b][src][cur[b][src]].ptr, S.p, lead, cap_frames(src), p.slot_of(b, src, wo.lo), N, (size_t)H * W, rec / 16,
                             m.cw(), c / 8, wo.lo > 0 ? 1 : 0, n_next, st);
      const Tens rest{centre.p, centre.plane_bytes, lead};
      m.conv(l0 + MEM_LAYER[k - 1], S, m.planes_for(c) > lead ? &rest : nullptr, N, H, W, relu6(outT), st);
    };
    const int N0 = win(0).count(), N2 = win(2).count(), N6 = win(6).count(), N8 = win(8).count();
    if (N0 > 0) {
      const Tens IN = at(b, C_IN, win(0).lo), X0 = at(b, C_X0, win(0).lo);
      if (b == 0) m.pack_in(in, IN, m.planes_for(4), N0, 4, h, w, 1, st);
      if (!m.conv_pair(l0 + INC0, IN, N0, h, w, relu6(X0), st)) {                            // inc.convblock.0 + .3
        Tens I0 = scratch(2, 0, N0, d.bsvd_interm_ch);
        m.conv(l0 + INC0, IN, nullptr, N0, h, w, relu6(I0), st);
        m.conv(l0 + INC3, I0, nullptr, N0, h, w, relu6(X0), st);
      }
      ConvOpts o = relu6(at(b, C_D0, win(0).lo)); o.epi = EPI_NHWC_SUB2;
      m.conv(l0 + DOWNC0, X0, nullptr, N0, h, w, o, st);                                     // downc0 stride 2
    }
    bibuf(1, c1, at(b, C_MA, win(1).lo));
    bibuf(2, c1, at(b, C_X1, win(2).lo));
    if (N2 > 0) {
      ConvOpts o = relu6(at(b, C_D1, win(2).lo)); o.epi = EPI_NHWC_SUB2;
      m.conv(l0 + DOWNC1, at(b, C_X1, win(2).lo), nullptr, N2, h / 2, w / 2, o, st);         // downc1 stride 2
    }
    bibuf(3, c2, at(b, C_MB, win(3).lo));
    bibuf(4, c2, at(b, C_X2, win(4).lo));
    bibuf(5, c2, at(b, C_MC, win(5).lo));                                                    // upc2.memconv
    if (N6 > 0) {
      Tens Mb2 = scratch(8, 2, N6, c2);
      bibuf(6, c2, Mb2);
      const Tens X1 = at(b, C_X1, win(6).lo);
      ConvOpts o; o.epi = EPI_NHWC_PS2; o.res1 = &X1; o.out = at(b, C_S1, win(6).lo);
      m.conv(l0 + UPC2, Mb2, nullptr, N6, h / 4, w / 4, o, st);                              // PixelShuffle + skip3
    }
    bibuf(7, c1, at(b, C_MA2, win(7).lo));                                                   // upc1.memconv
    if (N8 > 0) {
      Tens D02 = scratch(4, 1, N8, c1), S0 = scratch(12, 0, N8, c0);
      bibuf(8, c1, D02);
      const Tens X0 = at(b, C_X0, win(8).lo), IN = at(b, C_IN, win(8).lo);
      { ConvOpts o; o.epi = EPI_NHWC_PS2; o.res1 = &X0; o.out = S0;
        m.conv(l0 + UPC1, D02, nullptr, N8, h / 2, w / 2, o, st); }                          // PixelShuffle + skip2
      ConvOpts o; o.res1 = &IN; o.bsvd_resid = 1;
      if (b == 0) o.out = at(1, C_IN, win(8).lo);
      else { o.epi = EPI_NCHW_F32; o.out = Tens{reinterpret_cast<char*>(out), 0, 0}; }
      if (!m.conv_pair(l0 + OUTC0, S0, N8, h, w, o, st)) {                                   // outc.convblock.0 + .3 + residual
        Tens O0 = scratch(13, 0, N8, c0);
        m.conv(l0 + OUTC0, S0, nullptr, N8, h, w, relu6(O0), st);
        m.conv(l0 + OUTC3, O0, nullptr, N8, h, w, o, st);
      }
    }
    // the carry of every tensor that gained frames: its last `hist` slots to the front of the pair's other buffer
    for (int c = 0; c < C_COUNT; ++c) {
      const int cnt = p.write_count(b, c);
      if (cnt == 0) continue;
      BsvdCarry& e = tab.e[entries++];
      e.src = carried[b][c][cur[b][c]].ptr; e.dst = carried[b][c][cur[b][c] ^ 1].ptr;
      e.nplanes = planes_of(b, c); e.src_frames = e.dst_frames = cap_frames(c);
      e.src_first = cnt; e.count = CARRIED[c].hist;
      e.frame_slots = (unsigned)(frame_bytes(c) / 16);
    }
  }
  // a push never forks, so there is no second chain to wait for: only the context's conv profiling section, if launch_lanes opened one, ends here
  if (m.section_open) {
    SS4K_HIP(hipEventRecord(m.section.b, st));
    ctx->prof_sections.push_back(m.section);
    m.section_open = false;
  }
  if (entries > 0) {
    op_bsvd_online_carry(tab, entries, st);
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < C_COUNT; ++c) if (p.write_count(b, c) > 0) cur[b][c] ^= 1;
  }
}

}  // namespace ss4k
