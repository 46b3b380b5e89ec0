// The two service paths of the frame-in/frame-out upscaler (reference src/upscale/fsrcnn_upscaler.py) and the steps they share.
#include "upscaler.h"
#include "host_tables.h"
#include <chrono>

namespace ss4k {

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static std::vector<float> sharpen_taps(double strength) {  // sharpen_ker, fsrcnn_upscaler.py:54-84
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

static void fill_plane(float* p, size_t n, float v, hipStream_t st) {
  uint32_t bits; std::memcpy(&bits, &v, 4);   // hipMemsetD32Async writes a 32-bit pattern
  SS4K_HIP(hipMemsetD32Async((hipDeviceptr_t)p, (int)bits, n, st));
}

// The one place the HR tensor's element type is chosen: f(p as __half*) where the network wrote fp16 (hr16), else f(p)
template <typename F> static void as_hr(bool hr16, float* p, F&& f) {
  if (hr16) f(reinterpret_cast<__half*>(p)); else f(p);
}

void Upscaler::upload_taps() {
  auto up = [](DevBuf& b, const std::vector<float>& v) {
    b.ensure(v.size() * 4);
    SS4K_HIP(hipMemcpy(b.ptr, v.data(), v.size() * 4, hipMemcpyHostToDevice));
  };
  up(k_gauss17, gaussian_taps_1d(17, 8.0f));
  up(k_sharp, sharpen_taps(0.00002));
  up(k_sharp_hr, sharpen_taps(0.00007));
}

void Upscaler::save_tap(int which, const float* src, int n, int c, int h, int w, hipStream_t st) {
  if (!taps_on) return;
  const size_t bytes = (size_t)n * c * h * w * 4;
  tap[which].ensure(bytes);
  SS4K_HIP(hipMemcpyAsync(tap[which].ptr, src, bytes, hipMemcpyDeviceToDevice, st));
  tap_dims[which][0] = n; tap_dims[which][1] = c; tap_dims[which][2] = h; tap_dims[which][3] = w;
}

// The per-frame path always works at lr_shape (:239-241), the batched path only on larger frames and with lr_hr_resize (:173-176)
void Upscaler::lr_size(int h, int w, int* lh, int* lw) const {
  const bool to_lr = cfg.single_mode || ((w > cfg.lr_w || h > cfg.lr_h) && cfg.lr_hr_resize);
  *lh = to_lr ? cfg.lr_h : h; *lw = to_lr ? cfg.lr_w : w;
}

const float* Upscaler::planes_in(const uint8_t* in, int n, int h, int w, int lh, int lw, hipStream_t st) {
  const int P = 3 * n;
  img.ensure((size_t)P * h * w * 4);
  op_u8nhwc_to_f32nchw(in, img.as<float>(), n, h, w, 3, st);
  if (h == lh && w == lw) return img.as<float>();   // at equal size adaptive average pooling is the identity: no copy
  lr.ensure((size_t)P * lh * lw * 4);
  op_area(img.as<float>(), lr.as<float>(), P, h, w, lh, lw, st);
  return lr.as<float>();
}

void Upscaler::out_shape(int h, int w, int* oh, int* ow) const {
  int lh, lw; lr_size(h, w, &lh, &lw);
  int oc, H, W; sr->out_shape(1, lh, lw, &oc, &H, &W);
  // resized() without its equal-size exception: the pass that is skipped there would return the same size
  const bool resize = cfg.out_h > 0 && (cfg.single_mode || cfg.lr_hr_resize);
  *oh = resize ? cfg.out_h : H; *ow = resize ? cfg.out_w : W;
}

// The batched path resizes only with lr_hr_resize (:223), the per-frame path whenever output_shape is set (:316).  Always bicubic (quirk,
// :224-231).  At equal size align_corners=False bicubic has taps (0,1,0,0): the identity on already clamped values, so that pass is skipped
bool Upscaler::resized(int H, int W) const {
  return cfg.out_h > 0 && (cfg.single_mode || cfg.lr_hr_resize) && !(cfg.out_h == H && cfg.out_w == W);
}

void Upscaler::ensure_stats(int P) {
  st_hr.ensure(P * 8); st_lr.ensure(P * 8);
  SS4K_REQUIRE(P <= STATS_MAX_PLANES, "too many frames in one job");
  st_acc.ensure(sizeof(double) * 2 * P * STATS_SLOTS);
}

template <typename HT>
void Upscaler::stats_pair(const HT* hrt, const float* lrp, int P, int hr_px, int lr_px, bool hr_rode_along, hipStream_t st) {
  if (hr_rode_along) op_plane_stats_finish(st_acc.as<double>(), st_hr.as<float>(), P, hr_px, st);
  else op_plane_stats(st_acc.as<double>(), hrt, st_hr.as<float>(), P, hr_px, st);
  op_plane_stats(st_acc.as<double>(), lrp, st_lr.as<float>(), P, lr_px, st);
}

void Upscaler::color_maps(const float* lrp, int P, int lh, int lw, int mh, int mw, hipStream_t st) {
  const size_t sm = (size_t)P * mh * mw * 4;
  lb.ensure(sm); hb.ensure(sm); lbb.ensure(sm); hbb.ensure(sm);
  op_area(lrp, lb.as<float>(), P, lh, lw, mh, mw, st);
}

// diff = blur(hb) - blur(lb) (fsrcnn_upscaler.py:211-213), left in hb.  The blur is linear and its reflect padding commutes with
// the subtraction, so ONE blur of hb - lb, in its separable form (two 17-tap passes instead of two 289-tap ones): the same
// value up to the order of the fp32 additions (1e-7 relative; parity tolerance 1e-3 / 1e-4, colour tap vs oracle)
void Upscaler::color_diff(int P, int mh, int mw, hipStream_t st) {
  op_sub(hb.as<float>(), lb.as<float>(), hbb.as<float>(), (size_t)P * mh * mw, st);
  op_gauss17_reflect(hbb.as<float>(), lbb.as<float>(), hb.as<float>(), k_gauss17.as<float>(), P, mh, mw, st);
}

// Every per-element expression is the unfused path's.  Not resized: one read of hr.  Resized: the same in place without the uint8 store
// (bicubic reads 16 neighbours of the finished tensor), then bicubic -> uint8
template <typename HT>
void Upscaler::finish_fused(HT* hrt, const float* diff, int n, int H, int W, int mh, int mw, uint8_t* out, hipStream_t st) {
  const bool rs = resized(H, W);
  op_tail_fused(hrt, rs ? nullptr : out, diff, n, 3, H, W, mh, mw, st_hr.as<float>(), st_lr.as<float>(), st);
  if (rs) op_bicubic_u8(hrt, out, n, 3, H, W, cfg.out_h, cfg.out_w, st);
}

void Upscaler::finish_unfused(float* hrp, int n, int H, int W, uint8_t* out, hipStream_t st) {
  const int P = 3 * n;
  op_clamp01(hrp, (size_t)P * H * W, st);
  const float* fin = hrp; int FH = H, FW = W;
  if (resized(H, W)) {
    FH = cfg.out_h; FW = cfg.out_w;
    hr2.ensure((size_t)P * FH * FW * 4);
    op_bicubic(hrp, hr2.as<float>(), P, H, W, FH, FW, 1, st);
    fin = hr2.as<float>();
  }
  save_tap(4, fin, n, 3, FH, FW, st);
  op_f32nchw_to_u8nhwc(fin, out, n, 3, FH, FW, st);
}

void Upscaler::multi(const uint8_t* in, int n, int h, int w, uint8_t* out, hipStream_t st) {
  const int P = 3 * n;
  int lh, lw; lr_size(h, w, &lh, &lw);
  int oc, H, W; sr->out_shape(n, lh, lw, &oc, &H, &W);
  const int mh = H / 8, mw = W / 8;
  const bool color = mh > 8 && H > 64 && W > 64;  // local colour match, :201-218
  // ---- every refusal of a job that its sizes decide comes before the job's first launch and allocation
  sr->check_input(n, lh, lw);
  SS4K_REQUIRE(P <= STATS_MAX_PLANES, "too many frames in one job");
  // the reference's guard looks at the height only; for HR widths of 65..71 its 17-tap reflect pad (8)
  // reaches the 8-pixel-wide map and torch raises - so does this build
  SS4K_REQUIRE(!color || mw > 8, "local colour match: HR width / 8 must exceed the 17-tap blur's reflect padding (torch raises here too)");
  const float* lrp = planes_in(in, n, h, w, lh, lw, st);
  // fp16 HR tensor where the network's tail can write one (an fp16 SRVGG): the fused path below makes four passes over it (x4 on
  // 720p: 2880 x 5120 x 3 per frame), half the bytes each.  The fp32 parity path (taps) and fp32 models keep fp32.
  const bool hr16 = !taps_on && sr->can_half_out();
  hr.ensure((size_t)P * H * W * (hr16 ? 2 : 4));
  float* hrp = hr.as<float>();
  ensure_stats(P);
  const double tm0 = now_ms();
  // statistics of hr ride along with its producer where it can
  const bool hr_rode_along = sr->forward(lrp, hrp, n, lh, lw, st, ForwardOpts{taps_on ? nullptr : st_acc.as<double>(), hr16});
  enq_model_ms = now_ms() - tm0; enq_denoise_ms = 0;
  if (!taps_on) {
    // ---- fused path: the HR tensor is read by the statistics (unless they rode along), by the area reduction and by ONE tail pass
    SS4K_REQUIRE(!hr16 || hr_rode_along, "internal: the fp16 HR tensor's statistics must ride along with its producer");
    as_hr(hr16, hrp, [&](auto* hrt) {
      stats_pair(hrt, lrp, P, H * W, lh * lw, hr_rode_along, st);               // :190-196
      if (color) {
        color_maps(lrp, P, lh, lw, mh, mw, st);
        op_area_normalized(hrt, hb.as<float>(), P, H, W, mh, mw, st_hr.as<float>(), st_lr.as<float>(), st);   // area of the normalised tensor
        color_diff(P, mh, mw, st);
      }
      finish_fused(hrt, color ? hb.as<float>() : nullptr, n, H, W, mh, mw, out, st);   // :197-198, :215-233
    });
    return;
  }
  // ---- unfused path (parity taps enabled): one kernel per torch call of the reference
  save_tap(0, lrp, n, 3, lh, lw, st); save_tap(1, hrp, n, 3, H, W, st);
  stats_pair(hrp, lrp, P, H * W, lh * lw, false, st);                           // :190-196
  op_normalize(hrp, st_hr.as<float>(), st_lr.as<float>(), P, H * W, st);        // :197-198
  save_tap(2, hrp, n, 3, H, W, st);
  if (color) {
    color_maps(lrp, P, lh, lw, mh, mw, st);
    op_area(hrp, hb.as<float>(), P, H, W, mh, mw, st);
    color_diff(P, mh, mw, st);
    op_bilinear(hb.as<float>(), hrp, P, mh, mw, H, W, /*subtract_from_out=*/1, 0, st);   // hr -= diff (:215-218)
  }
  save_tap(3, hrp, n, 3, H, W, st);
  finish_unfused(hrp, n, H, W, out, st);                                        // :220-233
}

// The reference loops frame by frame in Python (:158-161); every frame is independent (BSVD sees F = 1, only the noise-map level differs
// for the very first frame of the stream), so the n frames of a job are pushed through each stage as one batch.
void Upscaler::single(const uint8_t* in, int n, int h, int w, uint8_t* out, hipStream_t st) {
  const int lh = cfg.lr_h, lw = cfg.lr_w, P = 3 * n;
  const size_t plane = (size_t)lh * lw;
  int oc, H, W; sr->out_shape(1, lh, lw, &oc, &H, &W);
  // ---- every refusal of a job that its sizes decide comes before the job's first launch and allocation (and before first_frame changes)
  sr->check_input(cfg.sr_is_realesrgan ? n : P, lh, lw);
  if (cfg.denoising) dn->check_input(n, lh, lw);
  SS4K_REQUIRE(P <= STATS_MAX_PLANES, "too many frames in one job");
  // FSRCNN on frames that need neither the area resize nor the denoiser reads the uint8 frames ITSELF (fsrcnn.hip, U8IN: the same
  // (float)byte / 255.0f) and the low-resolution statistics come straight from the bytes: the fp32 colour planes are never written
  // (round 6: one launch and 44 MB + 44 MB of traffic per four 720p frames less).  The parity path (taps) keeps the planes.
  const bool u8_direct = !taps_on && !cfg.denoising && !cfg.sr_is_realesrgan && h == lh && w == lw && sr->can_u8_in();
  if (u8_direct) {
    SS4K_REQUIRE(2 * P <= STATS_MAX_PLANES, "too many frames in one job");   // (the frames' and the output's planes share one set of accumulators)
    const bool hr16 = sr->can_half_out();
    hr.ensure((size_t)P * H * W * 4 * 2);
    st_hr.ensure(P * 8); st_lr.ensure(P * 8);
    // one set of accumulators for both tensors' statistics - the frames' [0, P) and the network output's [P, 2 P) - finished by ONE launch
    // that also zeroes what it has read: the accumulators (their own buffer, sized once for the largest job) are memset only when they
    // are new or when a job died between its first partial sum and its finishing launch (three launches of ~ 5 us less than two
    // op_plane_stats calls, in a 0.65 ms job)
    const size_t acc2_bytes = sizeof(double) * 2 * STATS_MAX_PLANES * STATS_SLOTS;
    if (st_acc2.bytes < acc2_bytes) { st_acc2.ensure(acc2_bytes); acc2_clean = false; }
    // (a job that is being CAPTURED into a graph by the caller runs later, any number of times, in whatever state an eager job in
    // between has left: it always carries the memset, and nothing it records changes what the buffer holds now)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    const bool capturing = cap != hipStreamCaptureStatusNone, was_clean = acc2_clean;
    if (!acc2_clean || capturing) SS4K_HIP(hipMemsetAsync(st_acc2.as<double>(), 0, acc2_bytes, st));
    acc2_clean = false;
    op_plane_stats_u8nhwc_partial(st_acc2.as<double>(), in, n, lh * lw, 2 * P, 0, st);
    enq_denoise_ms = 0;
    const double tm0 = now_ms();
    sr->forward(reinterpret_cast<const float*>(in), hr.as<float>(), P, lh, lw, st, ForwardOpts{nullptr, hr16, /*u8_in=*/true});
    enq_model_ms = now_ms() - tm0;
    as_hr(hr16, hr.as<float>(), [&](auto* hrt) {
      op_plane_stats_partial(st_acc2.as<double>(), hrt, P, H * W, 2 * P, P, st);
      op_plane_stats_finish2(st_acc2.as<double>(), st_lr.as<float>(), st_hr.as<float>(), P, lh * lw, H * W, true, st);
      acc2_clean = capturing ? was_clean : true;
      finish_fused(hrt, nullptr, n, H, W, 1, 1, out, st);
    });
    return;
  }
  const float* lr_before = planes_in(in, n, h, w, lh, lw, st);
  if (cfg.denoising) {
    lr4.ensure(plane * 4 * n * 4); den.ensure(plane * P * 4 * 2);
    for (int i = 0; i < n; ++i) {
      const float noise = first_frame ? 0.05f : (float)(0.1 * cfg.denoise_rate);  // :262, :269-271
      first_frame = false;
      float* dst = lr4.as<float>() + plane * 4 * i;
      SS4K_HIP(hipMemcpyAsync(dst, lr_before + plane * 3 * i, plane * 3 * 4, hipMemcpyDeviceToDevice, st));
      fill_plane(dst + plane * 3, plane, noise, st);  // constant noise-map plane
    }
    float* den0 = den.as<float>();
    const double t0 = now_ms();
    dn->forward(lr4.as<float>(), den0, n, lh, lw, st);
    enq_denoise_ms = now_ms() - t0;
    single_tail(lr_before, den0, den0 + plane * P, n, out, st);
    return;
  }
  single_tail(lr_before, nullptr, nullptr, n, out, st);
}

// What single() does after the denoiser, for n frames at lr_shape: lr_before = the undenoised LR planes of the SAME frames; denoised (null:
// no denoiser) = the denoiser's output for them, blend = n frames of scratch for the sharpened blend.  The temporal upscaler
// (upscaler_temporal.cpp) calls it with frames whose denoised planes arrive jobs later than their LR planes.
void Upscaler::single_tail(const float* lr_before, const float* denoised, float* blend, int n, uint8_t* out, hipStream_t st) {
  const int lh = cfg.lr_h, lw = cfg.lr_w, P = 3 * n;
  int oc, H, W; sr->out_shape(1, lh, lw, &oc, &H, &W);
  const float* lr_cur = lr_before;
  if (denoised) {
    // clamp(sharpen(den)) * 0.8 + 0.2 * lr   (:279-281)
    op_depthwise_reflect(denoised, blend, k_sharp.as<float>(), P, lh, lw, 3, 1, lr_before, 0.8f, (float)(1 - 0.8), st);
    lr_cur = blend;
  }
  save_tap(0, lr_cur, n, 3, lh, lw, st);
  hr.ensure((size_t)P * H * W * 4 * 2);
  float* hrp = hr.as<float>();
  // fp16 HR tensor where the network can write one and nothing but the fused tail reads it (no HR sharpening pass, no taps)
  const bool hr16 = !taps_on && !cfg.denoising && sr->can_half_out();
  const double tm0 = now_ms();
  sr->forward(lr_cur, hrp, cfg.sr_is_realesrgan ? n : P, lh, lw, st, ForwardOpts{nullptr, hr16});  // FSRCNN: on the colour planes (:297)
  enq_model_ms = now_ms() - tm0;
  if (cfg.denoising) {
    float* hs = hrp + (size_t)P * H * W;
    op_depthwise_reflect(hrp, hs, k_sharp_hr.as<float>(), P, H, W, 3, 1, nullptr, 0, 0, st);  // :298-299
    hrp = hs;
  }
  save_tap(1, hrp, n, 3, H, W, st);
  ensure_stats(P);
  if (!taps_on) {
    // ---- fused path: normalise -> clamp -> [bicubic] -> uint8 without writing the normalised tensor (same expressions)
    as_hr(hr16, hrp, [&](auto* hrt) {
      stats_pair(hrt, lr_before, P, H * W, lh * lw, false, st);                 // :304-310
      finish_fused(hrt, nullptr, n, H, W, 1, 1, out, st);                      // :311-326
    });
    return;
  }
  // ---- unfused path (parity taps enabled)
  stats_pair(hrp, lr_before, P, H * W, lh * lw, false, st);                     // :304-310
  op_normalize(hrp, st_hr.as<float>(), st_lr.as<float>(), P, H * W, st);        // :311-312
  save_tap(2, hrp, n, 3, H, W, st);
  finish_unfused(hrp, n, H, W, out, st);                                        // :315-326
}

}  // namespace ss4k
