// The per-frame service chain with a LAGGED denoiser: Upscaler::single with BSVD as the online machine (bsvd_online.h) in the place of the
// per-frame model.  single() denoises a frame and then needs the SAME frame's undenoised LR planes twice - for 0.8 * sharpen(den) + 0.2 * lr
// and for the mean / std match (fsrcnn_upscaler.py:279-281, 304-312).  The online denoiser returns a frame 16 frames after it went in, so those
// LR planes wait in a ring of lag + max_push frames and each frame meets its own when it comes out.
#include "upscaler_temporal.h"

namespace ss4k {

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

size_t TemporalUpscaler::state_bytes() const { return on.state_bytes() + ring.bytes; }

void TemporalUpscaler::reset() { on.reset(); first_frame = true; pushed = emitted = 0; }

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
  const float* lr_before = up.planes_in(in, n, h, w, lh, lw, st);
  ring.ensure(frame * ring_frames() * 4); lr4.ensure(plane * 4 * n * 4); den.ensure(frame * on.max_push * 4);
  for (int i = 0; i < n; ++i) {
    const float noise = first_frame ? 0.05f : (float)(0.1 * up.cfg.denoise_rate);  // fsrcnn_upscaler.py:262, :269-271
    first_frame = false;
    float* dst = lr4.as<float>() + plane * 4 * i;
    SS4K_HIP(hipMemcpyAsync(dst, lr_before + frame * i, frame * 4, hipMemcpyDeviceToDevice, st));
    fill_plane(dst + frame, plane, noise, st);
    SS4K_HIP(hipMemcpyAsync(ring.as<float>() + frame * ((pushed + i) % ring_frames()), lr_before + frame * i, frame * 4, hipMemcpyDeviceToDevice, st));
  }
  const int got = on.push(lr4.as<float>(), n, lh, lw, den.as<float>(), on.max_push, st);
  pushed += n;
  SS4K_REQUIRE(got == k, "internal: the online denoiser emitted another number of frames than its plan");
  if (k > 0) emit(k, den.as<float>(), out, st);
  return k;
}

int TemporalUpscaler::flush(uint8_t* out, size_t out_capacity_bytes, hipStream_t st) {
  const int left = on.pending();
  if (left == 0) { reset(); return 0; }
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
  return left;
}

}  // namespace ss4k
