// The per-frame service chain with the online BSVD denoiser (upscaler_temporal.cpp), behind ss4k_upscaler_temporal (include/ss4k.h).
#pragma once
#include "bsvd_online.h"
#include "upscaler.h"

namespace ss4k {

struct TemporalUpscaler {
  Upscaler up;          // the chain's glue, taps and SR model; its per-frame denoiser path is not used
  BsvdOnline on;
  DevBuf ring;          // lr_before of the frames inside the denoiser: (lag + max_push) frames of (3, lr_h, lr_w) fp32, frame i in slot i % frames
  DevBuf lr4, den, den_flush, lrk, blend;
  bool first_frame = true;
  long long pushed = 0, emitted = 0;   // frames of the running stream

  void create(ss4k_ctx* c, const ss4k_upscale_cfg& cfg, Model* sr, Model* bsvd_stream_model, int max_push);
  int ring_frames() const { return on.lag() + on.max_push; }
  // n frames (n, h, w, 3) in -> the k frames that became ready, (k, oh, ow, 3), oldest first; returns k
  int frames(const uint8_t* in, int n, int h, int w, uint8_t* out, size_t out_capacity_bytes, hipStream_t st);
  // the frames still inside; ends the stream
  int flush(uint8_t* out, size_t out_capacity_bytes, hipStream_t st);
  void reset();
  size_t state_bytes() const;

 private:
  void emit(int k, const float* denoised, uint8_t* out, hipStream_t st);
};

}  // namespace ss4k

struct ss4k_upscaler_temporal { ss4k::TemporalUpscaler t; };
