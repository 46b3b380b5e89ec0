// The per-frame service chain with a LAGGED denoiser: Upscaler::single with BSVD as the online machine (bsvd_online.h) in the place of the
// per-frame model.  single() denoises a frame and then needs the SAME frame's undenoised LR planes twice - for 0.8 * sharpen(den) + 0.2 * lr
// and for the mean / std match (fsrcnn_upscaler.py:279-281, 304-312).  The online denoiser returns a frame 16 frames after it went in, so those
// LR planes wait in a ring of lag + max_push frames and each frame meets its own when it comes out.
// With scene cuts on (TemporalCut) a job's input bytes are summed against their predecessors first; the flags stay on the device, where the
// denoiser's shift and the noise planes read them.
// Several streams share one object: what a stream owns sits in a TemporalSlot, and a round (temporal_round_plan.h) takes frames of several slots,
// pushes each slot's denoiser in turn and runs ONE tail over everything that became ready.  The one-stream entry points are slot 0.
// The noise plane is a constant per frame, or - set_noise_map - the motion-adaptive map (temporal_motion_plan.h): the same ring that keeps a
// frame's LR planes for its tail still holds the frame before it when it arrives, and the round's gather reads both.
#include "upscaler_temporal.h"
#include "frvsr.h"
#include <cmath>

namespace ss4k {

TemporalCut::~TemporalCut() {
  if (block) (void)hipHostFree(block);
}

bool TemporalCut::zones_intact() const {
  if (!block) return true;
  for (unsigned char c : block->front) if (c != 0xFF) return false;
  for (unsigned char c : block->back) if (c != 0xFF) return false;
  return true;
}

void TemporalCut::set(double t) {
  SS4K_REQUIRE(t == t && t >= 0.0 && t <= 255.0, "scene cut: the threshold is 0 (off) or a mean absolute difference in (0, 255]");
  if (t == 0.0) {   // off: the stored frame goes, and what the counters held with it
    release_device();
  } else if (!on()) {   // on again: the next frame is not compared
    have = false;
    if (!block) {
      SS4K_HIP(hipHostMalloc((void**)&block, sizeof(Pinned), hipHostMallocDefault));
      std::memset(block, 0xFF, sizeof(Pinned));
      host = &block->s;
    }
    std::memset(host, 0, sizeof(cut::SlotState));
    fresh = true;
  }
  threshold = t;
}

const uint32_t* TemporalCut::detect(const uint8_t* in, int n, int hh, int ww, hipStream_t st) {
  const size_t bytes = (size_t)3 * hh * ww;
  SS4K_REQUIRE(n >= 1 && n <= cut::MAX_ITEMS && bytes >= 1 && bytes <= cut::MAX_FRAME_BYTES, "scene cut: a job of 1..64 frames of at most 2^36 bytes");
  const uint8_t* fr[cut::MAX_ITEMS];
  for (int i = 0; i < n; ++i) fr[i] = in + (size_t)i * bytes;
  return detect_at(fr, n, hh, ww, st);
}

void TemporalCut::reserve(size_t bytes) {
  state.ensure(sizeof(cut::SlotState)); acc.ensure(cut::MAX_ITEMS * 8); flags.ensure(cut::MAX_ITEMS * 4);
  if (prev.bytes < bytes) { have = false; prev.ensure(bytes); }   // (a larger frame than the stored one: no comparison anyway)
}

void TemporalCut::release_device() {
  have = false;
  state.release(); acc.release(); flags.release(); prev.release();   // (a free waits for the device: no copy into `host` is in flight after it)
  if (host) std::memset(host, 0, sizeof(cut::SlotState));
  fresh = true;
}

const uint32_t* TemporalCut::detect_at(const uint8_t* const* fr, int n, int hh, int ww, hipStream_t st) {
  const size_t bytes = (size_t)3 * hh * ww;
  SS4K_REQUIRE(n >= 1 && n <= cut::MAX_ITEMS && bytes >= 1 && bytes <= cut::MAX_FRAME_BYTES, "scene cut: a job of 1..64 frames of at most 2^36 bytes");
  reserve(bytes);   // allocations first: one that fails leaves the comparison that is still possible as it was
  if (fresh) {
    SS4K_HIP(hipMemsetAsync(state.ptr, 0, sizeof(cut::SlotState), st));
    SS4K_HIP(hipMemsetAsync(acc.ptr, 0, cut::MAX_ITEMS * 8, st));
    SS4K_HIP(hipMemsetAsync(flags.ptr, 0, cut::MAX_ITEMS * 4, st));
    fresh = false;
  }
  const bool compare_first = have && h == hh && w == ww;   // no comparison for a stream's first frame, or after a change of frame size
  const int i0 = compare_first ? 0 : 1;
  if (n > i0) {
    cut::SadItems it{};
    for (int i = i0; i < n; ++i) {
      it.a[i - i0] = fr[i];
      it.b[i - i0] = i == 0 ? prev.as<uint8_t>() : const_cast<uint8_t*>(fr[i - 1]);   // (the build without the store writes nothing through b)
    }
    const int k = n - i0;
    it.compare = k == 64 ? ~0ull : (1ull << k) - 1;
    cut::sad_items(it, acc.as<unsigned long long>() + i0, k, bytes, false, st);
  }
  const unsigned long long T = (unsigned long long)std::max(1.0, std::ceil(threshold * 3.0 * (double)hh * (double)ww));
  cut::decide_run(acc.as<unsigned long long>(), state.as<cut::SlotState>(), flags.as<uint32_t>(), 0u, (unsigned)cut::MAX_ITEMS - 1u, n, compare_first, T, st);
  SS4K_HIP(hipMemcpyAsync(prev.ptr, fr[n - 1], bytes, hipMemcpyDeviceToDevice, st));
  SS4K_HIP(hipMemcpyAsync(host, state.ptr, sizeof(cut::SlotState), hipMemcpyDeviceToHost, st));
  have = true; h = hh; w = ww;
  return flags.as<uint32_t>();
}

static void fill_plane(float* p, size_t n, float v, hipStream_t st) {
  uint32_t bits; std::memcpy(&bits, &v, 4);   // hipMemsetD32Async writes a 32-bit pattern
  SS4K_HIP(hipMemsetD32Async((hipDeviceptr_t)p, (int)bits, n, st));
}

void TemporalUpscaler::create(ss4k_ctx* c, const ss4k_upscale_cfg& cfg, Model* sr, Model* bsvd_stream_model, int max_push_, int max_streams_) {
  SS4K_REQUIRE(c && sr && bsvd_stream_model, "temporal upscaler: NULL argument");
  SS4K_REQUIRE(max_streams_ >= 1 && max_streams_ <= temporal_round::MAX_STREAMS, "temporal upscaler: max_streams must be in 1..64");
  SS4K_REQUIRE(cfg.lr_h > 0 && cfg.lr_w > 0, "lr_shape must be positive");
  SS4K_REQUIRE(cfg.single_mode && cfg.denoising, "temporal upscaler: cfg must have single_mode and denoising set (the batched path has no denoiser)");
  SS4K_REQUIRE(cfg.lr_h % 4 == 0 && cfg.lr_w % 4 == 0, "temporal upscaler: lr_shape must be divisible by 4 (BSVD)");
  SS4K_REQUIRE((sr->in_channels() == 3) == (cfg.sr_is_realesrgan != 0), "sr_is_realesrgan does not match the SR model kind");
  std::vector<std::unique_ptr<TemporalSlot>> made;
  for (int s = 0; s < max_streams_; ++s) {
    made.push_back(std::make_unique<TemporalSlot>());
    made.back()->on.create(c, bsvd_stream_model, max_push_);
  }
  slots = std::move(made);
  max_push = max_push_;
  up.ctx = c; up.cfg = cfg; up.sr = sr; up.dn = bsvd_stream_model;
  up.upload_taps();
#ifdef SS4K_DEV
  // guard mode (upscaler.h); a slot's ring is state: never poisoned.  A round reads nothing of these that it has not written
  up.for_each_job_buf([](DevBuf& b) { b.transient = true; });
  for (DevBuf* b : {&lr4, &den, &den_flush, &lrk, &blend}) b->transient = true;
#endif
}

TemporalSlot& TemporalUpscaler::slot(int s) {
  SS4K_REQUIRE(s >= 0 && s < max_streams(), "temporal upscaler: a slot outside 0..max_streams-1");
  return *slots[s];
}
const TemporalSlot& TemporalUpscaler::slot(int s) const {
  SS4K_REQUIRE(s >= 0 && s < max_streams(), "temporal upscaler: a slot outside 0..max_streams-1");
  return *slots[s];
}

size_t TemporalUpscaler::state_bytes() const {
  size_t t = 0;
  for (const auto& s : slots) t += s->on.state_bytes() + s->ring.bytes + (s->cut ? s->cut->prev.bytes : 0);
  return t;
}

size_t TemporalUpscaler::stream_state_bytes_for() const {
  const size_t ring = (size_t)3 * up.cfg.lr_h * up.cfg.lr_w * ring_frames() * 4;
  return slots[0]->on.state_bytes_for(up.cfg.lr_h, up.cfg.lr_w) + ((ring + 255) & ~size_t(255));
}

void TemporalUpscaler::release_idle() {
  for (auto& s : slots) {
    if (s->running()) continue;
    s->rate = -1;
    s->on.release_state(); s->ring.release();
    if (s->cut) s->cut->release_device();   // (its counters start over, as after set_scene_cut(0): they lived in the buffers that go)
  }
}

void TemporalUpscaler::reset(int si) {
  TemporalSlot& s = slot(si);
  s.on.reset(); s.first_frame = true; s.pushed = s.emitted = 0; s.rate = -1;
  if (s.cut) s.cut->forget();
}

void TemporalUpscaler::set_denoise_rate(int si, float rate) {
  TemporalSlot& s = slot(si);
  SS4K_REQUIRE(std::isfinite(rate) && rate >= 0.f, "temporal upscaler: a denoise rate is finite and not negative");
  s.rate = (double)rate;
}

void TemporalUpscaler::set_noise_map(int mode) {
  SS4K_REQUIRE(mode == temporal_round::NOISE_MAP_CONSTANT || mode == temporal_round::NOISE_MAP_MOTION, "temporal upscaler: the noise map is constant (0) or motion (1)");
  // a stream's frames all enter by one rule: what its denoiser carries was made from the planes it was given
  for (const auto& s : slots) SS4K_REQUIRE(!s->running(), "temporal upscaler: the noise map cannot change while a stream is running");
  noise_map = mode;
}

// the detector of a slot that has none yet, once a threshold is set
void TemporalUpscaler::want_cut(TemporalSlot& s) {
  if (s.cut || !(cut_threshold > 0)) return;
  auto c = std::make_unique<TemporalCut>();
  c->set(cut_threshold);
  s.cut = std::move(c);
}

void TemporalUpscaler::set_scene_cut(double threshold) {
  SS4K_REQUIRE(threshold == threshold && threshold >= 0.0 && threshold <= 255.0, "scene cut: the threshold is 0 (off) or a mean absolute difference in (0, 255]");
  cut_threshold = threshold;
  want_cut(*slots[0]);   // (the other slots make theirs with their first round: a pinned block each)
  for (auto& s : slots) if (s->cut) s->cut->set(threshold);
}

// frames [emitted, emitted + k) of the slot's ring as one contiguous run in lrk, then the factored tail
void TemporalUpscaler::emit(TemporalSlot& s, int k, const float* denoised, uint8_t* out, hipStream_t st) {
  const size_t frame = (size_t)3 * up.cfg.lr_h * up.cfg.lr_w;
  lrk.ensure(frame * k * 4); blend.ensure(frame * k * 4);
  for (int i = 0; i < k; ++i)
    SS4K_HIP(hipMemcpyAsync(lrk.as<float>() + frame * i, s.ring.as<float>() + frame * ((s.emitted + i) % ring_frames()), frame * 4, hipMemcpyDeviceToDevice, st));
  up.single_tail(lrk.as<float>(), denoised, blend.as<float>(), k, out, st);
  s.emitted += k;
}

int TemporalUpscaler::round(const uint8_t* const* fr, const int* slot_ids, int k, int h, int w, uint8_t* out, size_t out_capacity_bytes,
                            int* n_out_per_item, int* item_slots, int* n_items, hipStream_t st) {
  const int lh = up.cfg.lr_h, lw = up.cfg.lr_w;
  const size_t plane = (size_t)lh * lw, frame = 3 * plane;
  // ---- every refusal for the whole round, before the first launch and before any state changes
  SS4K_REQUIRE(fr && slot_ids && n_out_per_item && item_slots && n_items, "temporal round: NULL argument");
  SS4K_REQUIRE(h > 0 && w > 0, "temporal round: empty frames");
  int oh, ow; up.out_shape(h, w, &oh, &ow);
  bsvd_online::State states[temporal_round::MAX_STREAMS];
  for (int s = 0; s < max_streams(); ++s) states[s] = slots[s]->on.state;
  const temporal_round::Plan p = temporal_round::make_round(slot_ids, k, states, max_push, max_streams(), (long long)(out_capacity_bytes / ((size_t)oh * ow * 3)));
  SS4K_REQUIRE(!p.refusal, p.refusal ? p.refusal : "");
  for (int i = 0; i < k; ++i) SS4K_REQUIRE(fr[i], "temporal round: NULL frame");
  SS4K_REQUIRE(out || p.total == 0, "temporal round: NULL output for a round that returns frames");
  const temporal_round::Motion mo = temporal_round::make_motion(p, max_push);   // (read in motion mode alone)
  // (what the launchers and the push would refuse, restated: none of them may stop a round half way)
  SS4K_REQUIRE((double)(bsvd_online::LAG / 2 + max_push) * lh * lw < 2147483648.0, "bsvd online push: a carried plane holds at most 2^31 pixels");
  SS4K_REQUIRE((double)h * lh < 2147483648.0 && (double)w * lw < 2147483648.0, "temporal round: a window bound of the area resize would overflow");
  SS4K_REQUIRE(!(cut_threshold > 0) || (size_t)3 * h * w <= cut::MAX_FRAME_BYTES, "scene cut: a frame holds at most 2^36 bytes");
  const int biggest = p.n_chunks ? p.chunk_n[0] : 1;
  up.sr->check_input(up.cfg.sr_is_realesrgan ? biggest : 3 * biggest, lh, lw);
  // ---- allocations, still before the first launch: one that fails leaves every stream as it was (a slot that gained its ring or its detector
  // keeps it).  What a slot's denoiser allocates with its first push is BsvdOnline's own and happens inside step 4.
  lr4.ensure(plane * 4 * k * 4);
  den.ensure(frame * std::max(p.total, max_push) * 4); lrk.ensure(frame * std::max(p.total, 1) * 4); blend.ensure(frame * max_push * 4);
  for (int t = 0; t < p.n_items; ++t) {
    TemporalSlot& s = *slots[p.items[t].slot];
    s.ring.ensure(frame * ring_frames() * 4);
    want_cut(s);
    if (s.cut && s.cut->on()) s.cut->reserve((size_t)3 * h * w);
  }
  try {
    // ---- 1. frames in: one launch, every frame from where it lies into its stream's ring slot
    FrvsrFramesIn fin{}; FrvsrPtrs dst{}; TroundTable tab{};
    unsigned long long start_bits = 0;
    for (int t = 0; t < p.n_items; ++t) {
      const temporal_round::Item& it = p.items[t];
      TemporalSlot& s = *slots[it.slot];
      for (int j = 0; j < it.n; ++j) {
        const int q = it.first + j;
        fin.p[q] = fr[p.order[q]];
        dst.p[q] = s.ring.as<float>() + frame * p.ring_in[q];
        tab.src[q] = dst.p[q];
        tab.level[q] = motion() ? motion_level(s) : level(s);
        // the frame before it in its stream: a ring slot this round's frames-in launch does not write, or an earlier frame of this item
        if (motion() && mo.ring_prev[q] >= 0) tab.prev[q] = s.ring.as<float>() + frame * mo.ring_prev[q];
      }
      if (s.first_frame) start_bits |= 1ull << it.first;
      SS4K_REQUIRE(!motion() || s.first_frame == (((mo.constant_bits >> it.first) & 1ull) != 0), "internal: a slot's first frame is not its denoiser's");
    }
    op_frames_in_items(fin, dst, k, h, w, lh, lw, st);
    // ---- 2. scene cuts: each slot's own detector on its own frames, frame 0 of an item against the slot's stored frame
    const uint32_t* item_cuts[temporal_round::MAX_FRAMES] = {};
    for (int t = 0; t < p.n_items; ++t) {
      const temporal_round::Item& it = p.items[t];
      TemporalSlot& s = *slots[it.slot];
      if (!(s.cut && s.cut->on())) continue;
      item_cuts[t] = s.cut->detect_at(fin.p + it.first, it.n, h, w, st);
      for (int j = 0; j < it.n; ++j) tab.flag[it.first + j] = item_cuts[t] + j;
    }
    // ---- 3. the packed (k, 4, lh, lw) denoiser input, noise planes included: one launch
    if (motion()) op_tround_gather_motion(tab, lr4.as<float>(), k, lh, lw, start_bits, 0.05f, st);
    else op_tround_gather(tab, lr4.as<float>(), k, plane, 4, start_bits, 0.05f, st);
    // ---- 4. one push per item, one after the other: they share the model's activation slots
    for (int t = 0; t < p.n_items; ++t) {
      const temporal_round::Item& it = p.items[t];
      TemporalSlot& s = *slots[it.slot];
      s.first_frame = false;
      const int got = s.on.push(lr4.as<float>() + plane * 4 * it.first, it.n, lh, lw, den.as<float>() + frame * it.den_off, (size_t)std::max(it.emitted, 1), st,
                                item_cuts[t]);
      s.pushed += it.n;
      SS4K_REQUIRE(got == it.emitted, "internal: the online denoiser emitted another number of frames than its plan");
    }
    if (p.total > 0) {
      // ---- 5. the leaving frames' LR planes out of their rings: one launch
      TroundTable leave{};
      for (int t = 0; t < p.n_items; ++t) {
        const temporal_round::Item& it = p.items[t];
        for (int q = 0; q < it.emitted; ++q) leave.src[it.den_off + q] = slots[it.slot]->ring.as<float>() + frame * p.ring_out[it.den_off + q];
        slots[it.slot]->emitted += it.emitted;
      }
      op_tround_gather(leave, lrk.as<float>(), p.total, plane, 3, 0ull, 0.f, st);
      // ---- 6. the tail over the round's frames, whatever stream they belong to
      for (int c = 0; c < p.n_chunks; ++c) {
        const size_t off = (size_t)p.chunk_off[c];
        up.single_tail(lrk.as<float>() + frame * off, den.as<float>() + frame * off, blend.as<float>(), p.chunk_n[c], out + off * oh * ow * 3, st);
      }
    }
  } catch (...) {   // a round that failed half way: none of its streams can go on (as a failed flush)
    for (int t = 0; t < p.n_items; ++t) reset(p.items[t].slot);
    throw;
  }
  for (int t = 0; t < p.n_items; ++t) { n_out_per_item[t] = p.items[t].emitted; item_slots[t] = p.items[t].slot; }
  *n_items = p.n_items;
  return p.total;
}

int TemporalUpscaler::frames(const uint8_t* in, int n, int h, int w, uint8_t* out, size_t out_capacity_bytes, hipStream_t st) {
  TemporalSlot& s0 = *slots[0];
  BsvdOnline& on = s0.on; DevBuf& ring = s0.ring; bool& first_frame = s0.first_frame; long long& pushed = s0.pushed;
  TemporalCut* cut = s0.cut.get();
  const int lh = up.cfg.lr_h, lw = up.cfg.lr_w;
  const size_t plane = (size_t)lh * lw, frame = 3 * plane;
  // ---- every refusal before the first launch and before any state changes
  SS4K_REQUIRE(in && out, "temporal upscaler: NULL argument");
  SS4K_REQUIRE(n > 0 && n <= on.max_push && h > 0 && w > 0, "temporal upscaler: a job holds 1..max_push frames");
  const int k = bsvd_online::make_plan(on.state, n, false).emitted;
  int oh, ow; up.out_shape(h, w, &oh, &ow);
  SS4K_REQUIRE(out_capacity_bytes >= (size_t)k * oh * ow * 3, "temporal upscaler: output buffer too small for the frames that become ready");
  up.sr->check_input(up.cfg.sr_is_realesrgan ? std::max(k, 1) : 3 * std::max(k, 1), lh, lw);
  // (the push's own size refusal, restated: a job that BsvdOnline::push would refuse must not move the detector either)
  const bool with_cuts = cut && cut->on();
  SS4K_REQUIRE(!(with_cuts || motion()) || (double)(bsvd_online::LAG / 2 + on.max_push) * lh * lw < 2147483648.0,
               "bsvd online push: a carried plane holds at most 2^31 pixels");
  SS4K_REQUIRE(!motion() || first_frame == (pushed == 0), "internal: a slot's first frame is not its stream's");
  // ---- scene cuts, if on: the job's flags, all on the device; with the constant plane also the noise planes (0.05 for a scene's first frame as
  // for a stream's) - the motion gather below reads the flags itself
  const uint32_t* cuts = nullptr;
  if (with_cuts) {
    lr4.ensure(plane * 4 * n * 4);
    cuts = cut->detect(in, n, h, w, st);
    if (!motion()) {
      op_bsvd_noise_planes(lr4.as<float>(), n, plane, cuts, first_frame ? 1 : 0, 0.05f, level(s0), st);
      first_frame = false;
    }
  }
  const float* lr_before = up.planes_in(in, n, h, w, lh, lw, st);
  ring.ensure(frame * ring_frames() * 4); lr4.ensure(plane * 4 * n * 4); den.ensure(frame * on.max_push * 4);
  // ---- lr4, the packed denoiser input, and the job's planes into the ring.  Constant plane: a copy and a fill per frame.  Motion map: round()'s
  // gather on the ring slots, every frame against the slot before its own (one launch, behind the loop)
  TroundTable tab{};
  for (int i = 0; i < n; ++i) {
    float* at = ring.as<float>() + frame * ((pushed + i) % ring_frames());
    if (!motion()) {
      const float noise = first_frame ? 0.05f : level(s0);  // fsrcnn_upscaler.py:262, :269-271
      first_frame = false;
      float* dst = lr4.as<float>() + plane * 4 * i;
      SS4K_HIP(hipMemcpyAsync(dst, lr_before + frame * i, frame * 4, hipMemcpyDeviceToDevice, st));
      if (!cuts) fill_plane(dst + frame, plane, noise, st);
    }
    SS4K_HIP(hipMemcpyAsync(at, lr_before + frame * i, frame * 4, hipMemcpyDeviceToDevice, st));
    tab.src[i] = at; tab.flag[i] = cuts ? cuts + i : nullptr; tab.level[i] = motion_level(s0);
    if (pushed + i > 0) tab.prev[i] = ring.as<float>() + frame * ((pushed + i - 1) % ring_frames());
  }
  if (motion()) {
    op_tround_gather_motion(tab, lr4.as<float>(), n, lh, lw, first_frame ? 1ull : 0ull, 0.05f, st);
    first_frame = false;
  }
  const int got = on.push(lr4.as<float>(), n, lh, lw, den.as<float>(), on.max_push, st, cuts);
  pushed += n;
  SS4K_REQUIRE(got == k, "internal: the online denoiser emitted another number of frames than its plan");
  if (k > 0) emit(s0, k, den.as<float>(), out, st);
  return k;
}

int TemporalUpscaler::flush(int si, uint8_t* out, size_t out_capacity_bytes, hipStream_t st) {
  TemporalSlot& s = slot(si);
  BsvdOnline& on = s.on;
  const int left = on.pending();
  if (left == 0) { reset(si); return 0; }   // (reset() clears the detector's stream too)
  SS4K_REQUIRE(out, "temporal upscaler flush: NULL argument");
  const int lh = up.cfg.lr_h, lw = up.cfg.lr_w;
  int oh, ow; up.out_shape(lh, lw, &oh, &ow);   // (the output size does not depend on the input frames' size on the per-frame path)
  SS4K_REQUIRE(out_capacity_bytes >= (size_t)left * oh * ow * 3, "temporal upscaler flush: output buffer too small for the pending frames");
  const size_t frame = (size_t)3 * lh * lw;
  den_flush.ensure(frame * left * 4);
  const int got = on.flush(den_flush.as<float>(), left, st);
  SS4K_REQUIRE(got == left, "internal: the online denoiser drained another number of frames than were pending");
  for (int done = 0; done < left; done += on.max_push) {   // the tail in jobs of at most max_push frames, like the pushes
    const int k = std::min(on.max_push, left - done);
    emit(s, k, den_flush.as<float>() + frame * done, out + (size_t)done * oh * ow * 3, st);
  }
  s.first_frame = true; s.pushed = s.emitted = 0; s.rate = -1;
  if (s.cut) s.cut->forget();
  return left;
}

}  // namespace ss4k
