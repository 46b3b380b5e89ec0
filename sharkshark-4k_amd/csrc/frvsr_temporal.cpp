// The frame-recurrent chain with a LAGGED denoiser in front (frvsr_temporal.h): TemporalUpscaler::round's steps up to the denoiser's pushes -
// frames into each stream's LR ring, one gather of the packed denoiser input, one push per item - and then, instead of one tail over the ready
// frames, the recurrent generator in waves (frvsr_temporal_plan.h): per wave one open_slots, ONE glue launch that writes every item's
// 0.8 * clamp01(sharpen(den)) + 0.2 * lr_before into its stream's lr buffer (frvsr_temporal.hip), one batched step, close_slots and one launch
// that writes the wave's frames where they go in the output.  The generator's files are not touched: the waves are FrvsrUpscaler rounds made
// from outside, as the scene-cut detector makes its refusals.
// Scene cuts (set_scene_cut): a slot's TemporalCut flags the input frames as they arrive, the flags go into the noise planes and the denoiser's
// ring as in TemporalUpscaler::round, and a wave that holds a stream with a live ring runs one more launch, frvt::clear_flagged_items, between
// open_slots and the glue: where the leaving frame's word is set, the stream's lr_prev / hr_prev are zeroed - the reset, 16 frames late.
#include "frvsr_temporal.h"
#include "upscaler_temporal.h"   // op_tround_gather, TroundTable
#include <cmath>

namespace ss4k {

// sharpen_ker(strength), fsrcnn_upscaler.py:54-84: the taps Upscaler::upload_taps uploads as k_sharp (upscaler.cpp), the same expressions
static std::vector<float> frvt_sharpen_taps(double strength) {
  std::vector<float> t(9);
  const float s = (float)strength, one_m = (float)(1.0 - strength);
  float sum = 0.f;
  for (int i = 0; i < 9; ++i) {
    const float sharp = i == 4 ? 9.f : -1.f, ident = i == 4 ? 1.f : 0.f;
    t[i] = sharp * s + one_m * ident; sum += t[i];
  }
  for (auto& v : t) v /= sum;
  return t;
}

void FrvsrTemporal::create(ss4k_ctx* c, Frvsr* m, Model* bsvd_stream_model, int lr_h, int lr_w, int out_h, int out_w, double rate, int max_push_,
                           int max_streams_, bool allow_pad) {
  SS4K_REQUIRE(c && m && bsvd_stream_model, "frvsr temporal: NULL argument");
  SS4K_REQUIRE(max_streams_ >= 1 && max_streams_ <= temporal_round::MAX_STREAMS, "frvsr temporal: max_streams must be in 1..64");
  SS4K_REQUIRE(lr_h >= 8 && lr_w >= 8, "lr_shape must be at least 8 x 8");
  SS4K_REQUIRE(allow_pad || (lr_h % 4 == 0 && lr_w % 4 == 0), "frvsr temporal: lr_shape must be divisible by 4 (BSVD)");
  SS4K_REQUIRE((out_h == 0 && out_w == 0) || (out_h > 0 && out_w > 0), "output_shape is (0, 0) or positive");
  SS4K_REQUIRE((double)lr_h * lr_w * 16.0 < 2147483648.0, "lr_shape: the output frame must hold fewer than 2^31 pixels");
  SS4K_REQUIRE(std::isfinite(rate) && rate >= 0.0, "frvsr temporal: a denoise rate is finite and not negative");
  std::vector<std::unique_ptr<FrvtSlot>> made;
  for (int s = 0; s < max_streams_; ++s) {
    made.push_back(std::make_unique<FrvtSlot>());
    made.back()->on.create(c, bsvd_stream_model, max_push_);   // (refuses max_push outside 1..64 and a model that is not a streaming BSVD)
  }
  const std::vector<float> taps = frvt_sharpen_taps(0.00002);
  k_sharp.ensure(taps.size() * 4);
  SS4K_HIP(hipMemcpy(k_sharp.ptr, taps.data(), taps.size() * 4, hipMemcpyHostToDevice));
  slots = std::move(made);
  ctx = c; denoise_rate = rate; max_push = max_push_;
  up.ctx = c; up.m = m; up.lr_h = lr_h; up.lr_w = lr_w; up.out_h = out_h; up.out_w = out_w;
  up.slots.resize((size_t)max_streams_);
  pad_h = (lr_h + 3) & ~3; pad_w = (lr_w + 3) & ~3;   // (a divisible shape: itself, and every launch below is the unpadded one)
#ifdef SS4K_DEV
  // guard mode (upscaler.h): a round reads nothing of these that it has not written.  The rings, the denoisers' state and lr / hr are state
  for (DevBuf* b : {&lr4, &den}) b->transient = true;
#endif
}

FrvtSlot& FrvsrTemporal::slot(int s) {
  SS4K_REQUIRE(s >= 0 && s < max_streams(), "frvsr temporal: a slot outside 0..max_streams-1");
  return *slots[s];
}
const FrvtSlot& FrvsrTemporal::slot(int s) const {
  SS4K_REQUIRE(s >= 0 && s < max_streams(), "frvsr temporal: a slot outside 0..max_streams-1");
  return *slots[s];
}

static size_t recurrent_bytes(const FrvsrUpscaler::Slot& r) { return r.lr[0].bytes + r.lr[1].bytes + r.hr[0].bytes + r.hr[1].bytes; }

static size_t detector_bytes(const FrvtSlot& s) {
  return s.cut ? s.cut->prev.bytes + s.cut->state.bytes + s.cut->acc.bytes + s.cut->flags.bytes : 0;
}

size_t FrvsrTemporal::state_bytes() const {
  size_t t = 0;
  for (int s = 0; s < max_streams(); ++s)
    t += slots[s]->on.state_bytes() + slots[s]->ring.bytes + recurrent_bytes(up.slots[s]) + detector_bytes(*slots[s]);
  return t;
}

size_t FrvsrTemporal::stream_state_bytes_for() const {
  const auto r256 = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t lr_b = (size_t)3 * up.lr_h * up.lr_w * 4;
  return slots[0]->on.state_bytes_for(pad_h, pad_w) + r256(lr_b * ring_frames()) + 2 * r256(lr_b) + 2 * r256(16 * lr_b);
}

void FrvsrTemporal::release_idle() {
  for (int s = 0; s < max_streams(); ++s) {
    FrvtSlot& t = *slots[s];
    if (t.running()) continue;
    t.rate = -1;
    t.on.release_state(); t.ring.release();
    if (t.cut) t.cut->release_device();   // (its counters start over, as after set_scene_cut(0): they lived in the buffers that go)
    FrvsrUpscaler::Slot& r = up.slots[s];
    r.have_state = false;
    for (int k = 0; k < 2; ++k) { r.lr[k].release(); r.hr[k].release(); }
  }
}

void FrvsrTemporal::reset(int si) {
  FrvtSlot& s = slot(si);
  s.on.reset(); s.first_frame = true; s.pushed = s.emitted = 0; s.rate = -1;
  up.slots[si].have_state = false;   // the next frame through the generator sees zero lr_prev / hr_prev
  if (s.cut) s.cut->forget();        // ... and is not compared
}

// the detector of a slot that has none yet, once a threshold is set
void FrvsrTemporal::want_cut(FrvtSlot& s) {
  if (s.cut || !(cut_threshold > 0)) return;
  auto c = std::make_unique<TemporalCut>();
  c->set(cut_threshold);
  s.cut = std::move(c);
}

void FrvsrTemporal::set_scene_cut(double threshold) {
  SS4K_REQUIRE(threshold == threshold && threshold >= 0.0 && threshold <= 255.0, "scene cut: the threshold is 0 (off) or a mean absolute difference in (0, 255]");
  cut_threshold = threshold;
  want_cut(*slots[0]);   // (the other slots make theirs with their first round: a pinned block each)
  for (auto& s : slots) if (s->cut) s->cut->set(threshold);
}

void FrvsrTemporal::set_noise_map(int mode) {
  SS4K_REQUIRE(mode == temporal_round::NOISE_MAP_CONSTANT || mode == temporal_round::NOISE_MAP_MOTION, "frvsr temporal: the noise map is constant (0) or motion (1)");
  // a stream's frames all enter by one rule: what its denoiser carries was made from the planes it was given
  for (const auto& s : slots) SS4K_REQUIRE(!s->running(), "frvsr temporal: the noise map cannot change while a stream is running");
  noise_map = mode;
}

void FrvsrTemporal::set_denoise_rate(int si, float rate) {
  FrvtSlot& s = slot(si);
  SS4K_REQUIRE(std::isfinite(rate) && rate >= 0.f, "frvsr temporal: a denoise rate is finite and not negative");
  s.rate = (double)rate;
}

// what the launchers of a round or a flush would refuse, restated: none of them may stop either half way
void FrvsrTemporal::check_sizes(int h, int w) const {
  const int lh = up.lr_h, lw = up.lr_w, H = 4 * lh, W = 4 * lw;
  int oh, ow; up.out_shape(&oh, &ow);
  SS4K_REQUIRE((double)(bsvd_online::LAG / 2 + max_push) * pad_h * pad_w < 2147483648.0, "bsvd online push: a carried plane holds at most 2^31 pixels");
  SS4K_REQUIRE((double)pad_h * pad_w * 4.0 < 2147483648.0, "frvsr temporal: a padded denoiser frame holds fewer than 2^31 values");
  SS4K_REQUIRE((double)h * lh < 2147483648.0 && (double)w * lw < 2147483648.0 && (double)H * oh < 2147483648.0 && (double)W * ow < 2147483648.0,
               "frvsr temporal: frame sizes whose area window bounds overflow");
  SS4K_REQUIRE(lh >= 2 && lw >= 2 && (double)lh * lw * 3.0 < 2147483648.0, "frvsr denoised in: a frame of at least 2 x 2 and fewer than 2^31 values");
}

void FrvsrTemporal::run_wave(const frvsr_temporal::Wave& wv, const float* const* den_of, const float* const* ring_of, uint8_t* const* out_of,
                             const uint32_t* const* flag_of, hipStream_t st) {
  const int lh = up.lr_h, lw = up.lr_w;
  int oh, ow; up.out_shape(&oh, &ow);
  int32_t ids[FRVT_MAX_ITEMS];
  for (int i = 0; i < wv.n; ++i) ids[i] = wv.slot[i];
  FrvsrUpscaler::RoundPtrs r{};
  up.open_slots(ids, wv.n, st, r);
  if (flag_of) {
    // a frame that was flagged when it went in leaves now: its stream's lr_prev / hr_prev read as zero, as open_slots gives a stream's first
    // frame.  The flags stay on the device; the launch is the same whether a cut leaves or not
    FrvtClearTable clr{};
    for (int i = 0; i < wv.n; ++i) { clr.flag[i] = flag_of[i]; clr.lr[i] = const_cast<float*>(r.lr_prev[i]); clr.hr[i] = r.hr_prev.p[i]; }
    up.m->timed(FRV_GLUE, st, [&] { op_frvt_clear_flagged_items(clr, wv.n, (size_t)3 * lh * lw * 4, (size_t)3 * 16 * lh * lw * 4, st); });
  }
  FrvtTable tab{}; FrvsrFramesOut fout{};
  for (int i = 0; i < wv.n; ++i) { tab.den[i] = den_of[i]; tab.lr[i] = ring_of[i]; tab.dst[i] = r.lr_dst.p[i]; fout.p[i] = out_of[i]; }
  // clamp(sharpen(den)) * 0.8 + 0.2 * lr   (fsrcnn_upscaler.py:279-281; Upscaler::single_tail's constants)
  if (padded())   // den is (3, pad_h, pad_w): the top-left (lh, lw) are the frame
    up.m->timed(FRV_GLUE, st, [&] { op_frvt_denoised_in_crop_items(tab, wv.n, lh, lw, pad_h, pad_w, k_sharp.as<float>(), 0.8f, (float)(1 - 0.8), st); });
  else
    up.m->timed(FRV_GLUE, st, [&] { op_frvt_denoised_in_items(tab, wv.n, lh, lw, k_sharp.as<float>(), 0.8f, (float)(1 - 0.8), st); });
  up.m->step_items(Frvsr::Items{r.lr_curr, r.lr_prev, &r.hr_prev, &r.hr_curr, true}, wv.n, lh, lw, st);
  up.close_slots(ids, wv.n);
  up.m->timed(FRV_GLUE, st, [&] { op_frames_out_items(r.hr_curr, fout, wv.n, 4 * lh, 4 * lw, oh, ow, st); });
}

int FrvsrTemporal::round(const uint8_t* const* fr, const int* slot_ids, int k, int h, int w, uint8_t* out, size_t out_capacity_bytes,
                         int* n_out_per_item, int* item_slots, int* n_items, hipStream_t st) {
  const int lh = up.lr_h, lw = up.lr_w;
  const size_t plane = (size_t)lh * lw, frame = 3 * plane;
  const size_t pplane = (size_t)pad_h * pad_w, pframe = 3 * pplane;   // the denoiser's planes and frames: lr4 and den
  // ---- every refusal for the whole round, before the first launch and before any state changes
  SS4K_REQUIRE(fr && slot_ids && n_out_per_item && item_slots && n_items, "frvsr temporal round: NULL argument");
  SS4K_REQUIRE(h > 0 && w > 0, "frvsr temporal round: empty frames");
  int oh, ow; up.out_shape(&oh, &ow);
  const size_t out_frame = (size_t)oh * ow * 3;
  bsvd_online::State states[temporal_round::MAX_STREAMS];
  for (int s = 0; s < max_streams(); ++s) states[s] = slots[s]->on.state;
  const temporal_round::Plan p = temporal_round::make_round(slot_ids, k, states, max_push, max_streams(), (long long)(out_capacity_bytes / out_frame));
  SS4K_REQUIRE(!p.refusal, p.refusal ? p.refusal : "");
  for (int i = 0; i < k; ++i) SS4K_REQUIRE(fr[i], "frvsr temporal round: NULL frame");
  SS4K_REQUIRE(out || p.total == 0, "frvsr temporal round: NULL output for a round that returns frames");
  const frvsr_temporal::Waves waves = frvsr_temporal::make_waves(p);
  const temporal_round::Motion mo = temporal_round::make_motion(p, max_push);   // (read in motion mode alone)
  for (int r = 0; r < waves.n_waves; ++r) {
    int32_t ids[FRVT_MAX_ITEMS];
    for (int i = 0; i < waves.w[r].n; ++i) ids[i] = waves.w[r].slot[i];
    up.check_round(ids, waves.w[r].n, h, w, false);
  }
  check_sizes(h, w);
  SS4K_REQUIRE(!(cut_threshold > 0) || (size_t)3 * h * w <= cut::MAX_FRAME_BYTES, "scene cut: a frame holds at most 2^36 bytes");
  // ---- allocations, still before the first launch: one that fails leaves every stream as it was (a slot that gained buffers keeps them).  A
  // slot's recurrent state is made here, with the stream's first frame, not 16 frames later: what a running slot holds does not depend on
  // how far its stream has come.  What a slot's denoiser allocates with its first push is BsvdOnline's own and happens inside step 3.
  lr4.ensure(pplane * 4 * k * 4);
  den.ensure(pframe * std::max(p.total, max_push) * 4);
  for (int t = 0; t < p.n_items; ++t) {
    slots[p.items[t].slot]->ring.ensure(frame * ring_frames() * 4);
    FrvsrUpscaler::Slot& rs = up.slots[p.items[t].slot];
    for (int b = 0; b < 2; ++b) { rs.lr[b].ensure(frame * 4); rs.hr[b].ensure(frame * 16 * 4); }
    FrvtSlot& s = *slots[p.items[t].slot];
    want_cut(s);   // (with no threshold set: nothing, and the round launches what it launched before there was a detector)
    if (s.cut && s.cut->on()) s.cut->reserve((size_t)3 * h * w);
  }
  try {
    // ---- 1. frames in: one launch, every frame from where it lies into its stream's ring slot
    FrvsrFramesIn fin{}; FrvsrPtrs dst{}; TroundTable tab{};
    unsigned long long start_bits = 0;
    for (int t = 0; t < p.n_items; ++t) {
      const temporal_round::Item& it = p.items[t];
      FrvtSlot& s = *slots[it.slot];
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
    up.m->timed(FRV_GLUE, st, [&] { op_frames_in_items(fin, dst, k, h, w, lh, lw, st); });
    // ---- 1b. scene cuts (TemporalUpscaler::round's step 2): each slot's own detector on its own frames as they arrived, frame 0 of an item
    // against the slot's stored frame.  The flags stay on the device: the gather, the denoiser's ring and - 16 frames later - the waves read them
    const uint32_t* item_cuts[temporal_round::MAX_FRAMES] = {};
    for (int t = 0; t < p.n_items; ++t) {
      const temporal_round::Item& it = p.items[t];
      FrvtSlot& s = *slots[it.slot];
      if (!(s.cut && s.cut->on())) continue;
      item_cuts[t] = s.cut->detect_at(fin.p + it.first, it.n, h, w, st);
      for (int j = 0; j < it.n; ++j) tab.flag[it.first + j] = item_cuts[t] + j;
    }
    // ---- 2. the packed (k, 4, lh, lw) denoiser input, noise planes included: one launch
    if (motion() && padded()) op_tround_gather_motion_pad(tab, lr4.as<float>(), k, lh, lw, start_bits, 0.05f, st);
    else if (motion()) op_tround_gather_motion(tab, lr4.as<float>(), k, lh, lw, start_bits, 0.05f, st);
    else if (padded()) op_tround_gather_pad(tab, lr4.as<float>(), k, lh, lw, start_bits, 0.05f, st);
    else op_tround_gather(tab, lr4.as<float>(), k, plane, 4, start_bits, 0.05f, st);
    // ---- 3. one push per item, one after the other: they share the model's activation slots
    for (int t = 0; t < p.n_items; ++t) {
      const temporal_round::Item& it = p.items[t];
      FrvtSlot& s = *slots[it.slot];
      s.first_frame = false;
      const int got = s.on.push(lr4.as<float>() + pplane * 4 * it.first, it.n, pad_h, pad_w, den.as<float>() + pframe * it.den_off, (size_t)std::max(it.emitted, 1), st,
                                item_cuts[t]);
      s.pushed += it.n;
      SS4K_REQUIRE(got == it.emitted, "internal: the online denoiser emitted another number of frames than its plan");
    }
    // ---- 4. the generator, wave after wave: frame den_off + r of every item that has one
    for (int r = 0; r < waves.n_waves; ++r) {
      const frvsr_temporal::Wave& wv = waves.w[r];
      const float* den_of[FRVT_MAX_ITEMS]; const float* ring_of[FRVT_MAX_ITEMS]; uint8_t* out_of[FRVT_MAX_ITEMS];
      const uint32_t* flag_of[FRVT_MAX_ITEMS];
      bool any_ring = false;
      for (int i = 0; i < wv.n; ++i) {
        FrvtSlot& s = *slots[wv.slot[i]];
        den_of[i] = den.as<float>() + pframe * wv.out[i];
        ring_of[i] = s.ring.as<float>() + frame * p.ring_out[wv.out[i]];
        out_of[i] = out + out_frame * wv.out[i];
        SS4K_REQUIRE((long long)wv.frame[i] == s.emitted, "internal: a wave carries another frame than the next one of its stream");
        // the leaving frame's own word: written by the push that brought it, this round's or an earlier one (frvsr_temporal_plan.h)
        flag_of[i] = s.on.cuts_live ? s.on.flag_ring.as<uint32_t>() + frvsr_temporal::ring_word(wv.frame[i]) : nullptr;
        any_ring = any_ring || s.on.cuts_live;
      }
      run_wave(wv, den_of, ring_of, out_of, any_ring ? flag_of : nullptr, st);
      for (int i = 0; i < wv.n; ++i) slots[wv.slot[i]]->emitted += 1;
    }
  } catch (...) {   // a round that failed half way: none of its streams can go on, neither half of them
    for (int t = 0; t < p.n_items; ++t) reset(p.items[t].slot);
    throw;
  }
  for (int t = 0; t < p.n_items; ++t) { n_out_per_item[t] = p.items[t].emitted; item_slots[t] = p.items[t].slot; }
  *n_items = p.n_items;
  return p.total;
}

int FrvsrTemporal::flush(int si, uint8_t* out, size_t out_capacity_bytes, hipStream_t st) {
  FrvtSlot& s = slot(si);
  const int left = s.on.pending();
  if (left == 0) { reset(si); return 0; }
  // ---- every refusal before the first launch
  SS4K_REQUIRE(out, "frvsr temporal flush: NULL argument");
  const int lh = up.lr_h, lw = up.lr_w;
  int oh, ow; up.out_shape(&oh, &ow);
  const size_t out_frame = (size_t)oh * ow * 3, frame = (size_t)3 * lh * lw, pframe = (size_t)3 * pad_h * pad_w;
  SS4K_REQUIRE(out_capacity_bytes >= (size_t)left * out_frame, "frvsr temporal flush: output buffer too small for the pending frames");
  const frvsr_temporal::Waves waves = frvsr_temporal::make_flush(si, left, (int)s.emitted);
  SS4K_REQUIRE(waves.n_waves == left, "internal: a flush of more frames than a slot can hold");
  // BsvdOnline::flush() ends with reset(), which drops cuts_live - and leaves the ring's words as they are until the NEXT stream's first push
  // with flags zero-fills them on its stream.  The waves below run before any such push, on the same stream: they read what this stream wrote
  const uint32_t* const flag_ring = s.on.cuts_live ? s.on.flag_ring.as<uint32_t>() : nullptr;
  const int32_t id = si;
  up.check_round(&id, 1, lh, lw, false);
  check_sizes(lh, lw);
  den.ensure(pframe * left * 4);
  try {
    const int got = s.on.flush(den.as<float>(), (size_t)left, st);
    SS4K_REQUIRE(got == left, "internal: the online denoiser drained another number of frames than were pending");
    for (int r = 0; r < left; ++r) {   // the generator takes a stream's frames one at a time
      const float* den_of = den.as<float>() + pframe * r;
      const float* ring_of = s.ring.as<float>() + frame * ((s.emitted + r) % ring_frames());
      uint8_t* out_of = out + out_frame * r;
      const uint32_t* flag_of = flag_ring ? flag_ring + frvsr_temporal::ring_word(waves.w[r].frame[0]) : nullptr;
      run_wave(waves.w[r], &den_of, &ring_of, &out_of, flag_ring ? &flag_of : nullptr, st);
    }
  } catch (...) {
    reset(si);
    throw;
  }
  reset(si);   // the stream has ended: the slot is free
  return left;
}

}  // namespace ss4k
