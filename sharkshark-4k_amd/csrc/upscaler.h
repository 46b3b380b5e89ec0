// The frame-in/frame-out upscaler behind ss4k_upscaler (include/ss4k.h): the service paths of the reference's
// src/upscale/fsrcnn_upscaler.py, uint8 NHWC frames in, uint8 NHWC frames out.
#pragma once
#include "models.h"

namespace ss4k {

struct Upscaler {
  ss4k_ctx* ctx = nullptr; ss4k_upscale_cfg cfg{}; Model* sr = nullptr; Model* dn = nullptr;
  DevBuf k_gauss17, k_sharp, k_sharp_hr;
  DevBuf img, lr, lr4, den, hr, hr2, lb, hb, lbb, hbb, st_hr, st_lr, st_acc, st_acc2;
  bool acc2_clean = false;   // st_acc2 holds zeros (its last user re-zeroed what it had summed: k_stats_final2)
  bool first_frame = true;
  bool taps_on = false;
  // host time spent enqueueing the last job's denoise / SR model stages: what the reference's
  // 'fsrcnn.denoise' / 'fsrcnn.model' profiler spans measure on an asynchronous device queue
  // (util/profiler.py:12-24 - no device sync)
  double enq_denoise_ms = 0, enq_model_ms = 0;
  DevBuf tap[5]; int tap_dims[5][4] = {};

  // The per-job buffers: every job rewrites what it reads from these, so the dev library marks them `transient` and guard mode
  // (ss4k_dev_guard_poison) refills them with 0xFF between jobs.  NOT in the list, so never poisoned: k_gauss17 and k_sharp* (uploaded once,
  // upload_taps); st_acc2 (its "clean after the finishing launch" invariant is the contract: acc2_clean, single()).
  // Elsewhere: a model's weights, bias, PReLU, w16 and fs_blob (uploaded once); the context's zero_page (zeros are its content) and
  // cv-area tables (they hold offsets: poison there would turn a stale read into a wild address, not a NaN).
  template <typename F> void for_each_job_buf(F&& f) {
    for (DevBuf* b : {&img, &lr, &lr4, &den, &hr, &hr2, &lb, &hb, &lbb, &hbb, &st_hr, &st_lr, &st_acc}) f(*b);
    for (DevBuf& t : tap) f(t);
  }

  void upload_taps();                                         // once, at creation: k_gauss17, k_sharp, k_sharp_hr
  void out_shape(int h, int w, int* oh, int* ow) const;       // the frame size a job of (h, w) frames returns
  // n frames (n, h, w, 3) -> (n, oh, ow, 3), enqueued on st: multi() without cfg.single_mode, single() with it
  void multi(const uint8_t* in, int n, int h, int w, uint8_t* out, hipStream_t st);    // fsrcnn_upscaler.py:168-233
  void single(const uint8_t* in, int n, int h, int w, uint8_t* out, hipStream_t st);   // fsrcnn_upscaler.py:235-326
  // the two halves of single() that the temporal upscaler (upscaler_temporal.cpp) runs jobs apart:
  // uint8 NHWC frames -> / 255 -> fp32 planes (img), through area to (lh, lw) where that is another size (lr): the planes' address
  const float* planes_in(const uint8_t* in, int n, int h, int w, int lh, int lw, hipStream_t st);
  // ... and everything after the denoiser (:279-326): sharpen + blend with lr_before, the SR forward, the HR sharpen, the statistics, the finish
  void single_tail(const float* lr_before, const float* denoised, float* blend, int n, uint8_t* out, hipStream_t st);

 private:
  void lr_size(int h, int w, int* lh, int* lw) const;         // the size the network sees for (h, w) frames
  bool resized(int H, int W) const;                           // the finished (H, W) tensor is resized to cfg.out_h x cfg.out_w
  void save_tap(int which, const float* src, int n, int c, int h, int w, hipStream_t st);   // a copy for the parity taps; nothing unless taps_on
  void ensure_stats(int P);                                   // st_hr, st_lr and st_acc for P planes
  // mean / std of the HR planes into st_hr and of the LR planes into st_lr, both through st_acc; hr_rode_along: the network already summed
  // the HR planes into st_acc while it wrote them (ForwardOpts::stats_acc)
  template <typename HT> void stats_pair(const HT* hrt, const float* lrp, int P, int hr_px, int lr_px, bool hr_rode_along, hipStream_t st);
  // the (mh, mw) colour maps: lb = area(lrp); hb, lbb and hbb sized.  The caller fills hb, then color_diff() leaves the difference in hb
  void color_maps(const float* lrp, int P, int lh, int lw, int mh, int mw, hipStream_t st);
  void color_diff(int P, int mh, int mw, hipStream_t st);
  // the ending without parity taps: normalise, - diff (or null), clamp, [bicubic,] * 255 -> out, in one or two passes over the HR tensor
  template <typename HT> void finish_fused(HT* hrt, const float* diff, int n, int H, int W, int mh, int mw, uint8_t* out, hipStream_t st);
  // the ending with parity taps, one kernel per torch call, from the clamp onwards: clamp, [bicubic into hr2,] tap 4, * 255 -> out
  void finish_unfused(float* hrp, int n, int H, int W, uint8_t* out, hipStream_t st);
};

}  // namespace ss4k

struct ss4k_upscaler { ss4k::Upscaler u; };
