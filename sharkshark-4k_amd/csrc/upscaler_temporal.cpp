// The per-frame service chain with a LAGGED denoiser: Upscaler::single with BSVD as the online machine (bsvd_online.h) in the place of the
// per-frame model.  single() denoises a frame and then needs the SAME frame's undenoised LR planes twice - for 0.8 * sharpen(den) + 0.2 * lr
// and for the mean / std match (fsrcnn_upscaler.py:279-281, 304-312).  The online denoiser returns a frame 16 frames after it went in, so those
// LR planes wait in a ring of lag + max_push frames and each frame meets its own when it comes out.
// With scene cuts on (TemporalCut) a job's input bytes are summed against their predecessors first; the flags stay on the device, where the
// denoiser's shift and the noise planes read them.
#include "upscaler_temporal.h"
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
    have = false;
    state.release(); acc.release(); flags.release(); prev.release();   // (a free waits for the device: no copy into `host` is in flight after it)
    if (host) std::memset(host, 0, sizeof(cut::SlotState));
    fresh = true;
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
  // ---- allocations first: one that fails leaves the comparison that is still possible as it was
  state.ensure(sizeof(cut::SlotState)); acc.ensure(cut::MAX_ITEMS * 8); flags.ensure(cut::MAX_ITEMS * 4);
  if (prev.bytes < bytes) { have = false; prev.ensure(bytes); }   // (a larger frame than the stored one: no comparison anyway)
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
      it.a[i - i0] = in + (size_t)i * bytes;
      it.b[i - i0] = i == 0 ? prev.as<uint8_t>() : const_cast<uint8_t*>(in + (size_t)(i - 1) * bytes);   // (the build without the store writes nothing through b)
    }
    const int k = n - i0;
    it.compare = k == 64 ? ~0ull : (1ull << k) - 1;
    cut::sad_items(it, acc.as<unsigned long long>() + i0, k, bytes, false, st);
  }
  const unsigned long long T = (unsigned long long)std::max(1.0, std::ceil(threshold * 3.0 * (double)hh * (double)ww));
  cut::decide_run(acc.as<unsigned long long>(), state.as<cut::SlotState>(), flags.as<uint32_t>(), 0u, (unsigned)cut::MAX_ITEMS - 1u, n, compare_first, T, st);
  SS4K_HIP(hipMemcpyAsync(prev.ptr, in + (size_t)(n - 1) * bytes, bytes, hipMemcpyDeviceToDevice, st));
  SS4K_HIP(hipMemcpyAsync(host, state.ptr, sizeof(cut::SlotState), hipMemcpyDeviceToHost, st));
  have = true; h = hh; w = ww;
  return flags.as<uint32_t>();
}

static void fill_plane(float* p, size_t n, float v, hipStream_t st) {
  uint32_t bits; std::memcpy(&bits, &v, 4);   // hipMemsetD32Async writes a 32-bit pattern
  SS4K_HIP(hipMemsetD32Async((hipDeviceptr_t)p, (int)bits, n, st));
}

void TemporalUpscaler::create(ss4k_ctx* c, const ss4k_upscale_cfg& cfg, Model* sr, Model* bsvd_stream_model, int max_push_) {
  SS4K_REQUIRE(c && sr && bsvd_stream_model, "temporal upscaler: NULL argument");
  SS4K_REQUIRE(cfg.lr_h > 0 && cfg.lr_w > 0, "lr_shape must be positive");
  SS4K_REQUIRE(cfg.single_mode && cfg.denoising, "temporal upscaler: cfg must have single_mode and denoising set (the batched path has no denoiser)");
  SS4K_REQUIRE(cfg.lr_h % 4 == 0 && cfg.lr_w % 4 == 0, "temporal upscaler: lr_shape must be divisible by 4 (BSVD)");
  SS4K_REQUIRE((sr->in_channels() == 3) == (cfg.sr_is_realesrgan != 0), "sr_is_realesrgan does not match the SR model kind");
  on.create(c, bsvd_stream_model, max_push_);
  up.ctx = c; up.cfg = cfg; up.sr = sr; up.dn = bsvd_stream_model;
  up.upload_taps();
#ifdef SS4K_DEV
  up.for_each_job_buf([](DevBuf& b) { b.transient = true; });   // guard mode (upscaler.h); ring is state: never poisoned
#endif
}

size_t TemporalUpscaler::state_bytes() const { return on.state_bytes() + ring.bytes + (cut ? cut->prev.bytes : 0); }

void TemporalUpscaler::reset() { on.reset(); first_frame = true; pushed = emitted = 0; if (cut) cut->forget(); }

void TemporalUpscaler::set_scene_cut(double threshold) {
  if (!cut) {
    SS4K_REQUIRE(threshold == threshold && threshold >= 0.0 && threshold <= 255.0, "scene cut: the threshold is 0 (off) or a mean absolute difference in (0, 255]");
    if (threshold == 0.0) return;
    cut = std::make_unique<TemporalCut>();
  }
  cut->set(threshold);
}

// frames [emitted, emitted + k) of the ring as one contiguous run in lrk, then the factored tail
void TemporalUpscaler::emit(int k, const float* denoised, uint8_t* out, hipStream_t st) {
  const size_t frame = (size_t)3 * up.cfg.lr_h * up.cfg.lr_w;
  lrk.ensure(frame * k * 4); blend.ensure(frame * k * 4);
  for (int i = 0; i < k; ++i)
    SS4K_HIP(hipMemcpyAsync(lrk.as<float>() + frame * i, ring.as<float>() + frame * ((emitted + i) % ring_frames()), frame * 4, hipMemcpyDeviceToDevice, st));
  up.single_tail(lrk.as<float>(), denoised, blend.as<float>(), k, out, st);
  emitted += k;
}

int TemporalUpscaler::frames(const uint8_t* in, int n, int h, int w, uint8_t* out, size_t out_capacity_bytes, hipStream_t st) {
  const int lh = up.cfg.lr_h, lw = up.cfg.lr_w;
  const size_t plane = (size_t)lh * lw, frame = 3 * plane;
  // ---- every refusal before the first launch and before any state changes
  SS4K_REQUIRE(in && out, "temporal upscaler: NULL argument");
  SS4K_REQUIRE(n > 0 && n <= on.max_push && h > 0 && w > 0, "temporal upscaler: a job holds 1..max_push frames");
  const int k = bsvd_online::make_plan(on.state, n, false).emitted;
  int oh, ow; up.out_shape(h, w, &oh, &ow);
  SS4K_REQUIRE(out_capacity_bytes >= (size_t)k * oh * ow * 3, "temporal upscaler: output buffer too small for the frames that become ready");
  up.sr->check_input(up.cfg.sr_is_realesrgan ? std::max(k, 1) : 3 * std::max(k, 1), lh, lw);
  // ---- scene cuts, if on: the job's flags and its noise planes (0.05 for a scene's first frame as for a stream's), all on the device
  const uint32_t* cuts = nullptr;
  if (cut && cut->on()) {
    // (the push's own size refusal, restated: a job that BsvdOnline::push would refuse must not move the detector either)
    SS4K_REQUIRE((double)(bsvd_online::LAG / 2 + on.max_push) * lh * lw < 2147483648.0, "bsvd online push: a carried plane holds at most 2^31 pixels");
    lr4.ensure(plane * 4 * n * 4);
    cuts = cut->detect(in, n, h, w, st);
    op_bsvd_noise_planes(lr4.as<float>(), n, plane, cuts, first_frame ? 1 : 0, 0.05f, (float)(0.1 * up.cfg.denoise_rate), st);
    first_frame = false;
  }
  const float* lr_before = up.planes_in(in, n, h, w, lh, lw, st);
  ring.ensure(frame * ring_frames() * 4); lr4.ensure(plane * 4 * n * 4); den.ensure(frame * on.max_push * 4);
  for (int i = 0; i < n; ++i) {
    const float noise = first_frame ? 0.05f : (float)(0.1 * up.cfg.denoise_rate);  // fsrcnn_upscaler.py:262, :269-271
    first_frame = false;
    float* dst = lr4.as<float>() + plane * 4 * i;
    SS4K_HIP(hipMemcpyAsync(dst, lr_before + frame * i, frame * 4, hipMemcpyDeviceToDevice, st));
    if (!cuts) fill_plane(dst + frame, plane, noise, st);
    SS4K_HIP(hipMemcpyAsync(ring.as<float>() + frame * ((pushed + i) % ring_frames()), lr_before + frame * i, frame * 4, hipMemcpyDeviceToDevice, st));
  }
  const int got = on.push(lr4.as<float>(), n, lh, lw, den.as<float>(), on.max_push, st, cuts);
  pushed += n;
  SS4K_REQUIRE(got == k, "internal: the online denoiser emitted another number of frames than its plan");
  if (k > 0) emit(k, den.as<float>(), out, st);
  return k;
}

int TemporalUpscaler::flush(uint8_t* out, size_t out_capacity_bytes, hipStream_t st) {
  const int left = on.pending();
  if (left == 0) { reset(); return 0; }   // (reset() clears the detector's stream too)
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
    emit(k, den_flush.as<float>() + frame * done, out + (size_t)done * oh * ow * 3, st);
  }
  first_frame = true; pushed = emitted = 0;
  if (cut) cut->forget();
  return left;
}

}  // namespace ss4k
