// The per-frame service chain with the online BSVD denoiser (upscaler_temporal.cpp), behind ss4k_upscaler_temporal (include/ss4k.h).
#pragma once
#include "bsvd_online.h"
#include "scene_cut.h"
#include "upscaler.h"
#include <memory>

namespace ss4k {

// Scene cuts for the temporal stream (include/ss4k.h: ss4k_upscaler_temporal_set_scene_cut): the rule of scene_cut.h on the job's input bytes,
// frame i against frame i - 1 of the job and frame 0 against a device copy of the previous job's last frame.  The flags never leave the
// device: BsvdOnline::push copies them into its ring, and the host learns about cuts only when it asks.  Created by the first
// set_scene_cut(threshold > 0); every device buffer is a DevBuf, so guard mode sees it.
struct TemporalCut {
  double threshold = 0;        // mean absolute byte difference in 8-bit levels, (0, 255]; 0 = off
  DevBuf prev;                 // the previous job's last frame, uint8 HWC as it arrived: 3hw bytes
  int h = 0, w = 0;
  bool have = false;           // prev holds the running stream's last frame
  DevBuf state, acc, flags;    // one cut::SlotState, u64[MAX_ITEMS], u32[MAX_ITEMS]: the job's flags, frame i in word i
  // pinned copy of `state`, refreshed by an asynchronous copy after every job; it sits between two red zones of 0xFF that the dev library checks
  // whenever the stats are read (zones_intact)
  struct Pinned { unsigned char front[64]; cut::SlotState s; unsigned char back[64]; };
  Pinned* block = nullptr;
  cut::SlotState* host = nullptr;   // &block->s
  bool zones_intact() const;
  bool fresh = true;           // the device state has not been zeroed yet (done on the first job's stream)
  ~TemporalCut();
  bool on() const { return threshold > 0; }
  void set(double t);
  void forget() { have = false; }   // reset / flush: the next frame is a stream's first
  // the sums, cut::decide_run, the refresh of prev and of the pinned block; returns the job's n flag words (device)
  const uint32_t* detect(const uint8_t* in, int n, int hh, int ww, hipStream_t st);
};

struct TemporalUpscaler {
  Upscaler up;          // the chain's glue, taps and SR model; its per-frame denoiser path is not used
  BsvdOnline on;
  DevBuf ring;          // lr_before of the frames inside the denoiser: (lag + max_push) frames of (3, lr_h, lr_w) fp32, frame i in slot i % frames
  DevBuf lr4, den, den_flush, lrk, blend;
  bool first_frame = true;
  std::unique_ptr<TemporalCut> cut;   // null until the first set_scene_cut(threshold > 0)
  long long pushed = 0, emitted = 0;   // frames of the running stream

  void create(ss4k_ctx* c, const ss4k_upscale_cfg& cfg, Model* sr, Model* bsvd_stream_model, int max_push);
  int ring_frames() const { return on.lag() + on.max_push; }
  // n frames (n, h, w, 3) in -> the k frames that became ready, (k, oh, ow, 3), oldest first; returns k
  int frames(const uint8_t* in, int n, int h, int w, uint8_t* out, size_t out_capacity_bytes, hipStream_t st);
  // the frames still inside; ends the stream
  int flush(uint8_t* out, size_t out_capacity_bytes, hipStream_t st);
  void reset();
  size_t state_bytes() const;
  void set_scene_cut(double threshold);

 private:
  void emit(int k, const float* denoised, uint8_t* out, hipStream_t st);
};

}  // namespace ss4k

struct ss4k_upscaler_temporal { ss4k::TemporalUpscaler t; };
