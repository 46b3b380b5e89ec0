// The frame-recurrent service chain with the online BSVD denoiser in front (frvsr_temporal.cpp), behind ss4k_frvsr_temporal (include/ss4k.h):
// what TemporalUpscaler is to the per-frame chain.  Per stream, frame t:
//   lr_before_t = area(img / 255, lr_shape)                                             (egvsr_upscaler.py:195-196)
//   den_t       = the online denoiser's output for frame t of the stream of (lr_before, noise) inputs; noise 0.05 for a stream's first frame,
//                 0.1 * rate after (fsrcnn_upscaler.py:262,269-271); it exists once frame t + 16 has entered, or at a flush
//   lr_curr_t   = 0.8 * clamp01(sharpen3x3_reflect(den_t)) + 0.2 * lr_before_t           (fsrcnn_upscaler.py:279-281)
//   hr_t        = FRNet(lr_curr_t, lr_curr_{t-1}, hr_{t-1}), zeros for a stream's first frame; clamp, area to output_shape, * 255 truncated
// Nothing of the per-frame tail follows (no HR sharpening, no mean / std match): hr_prev stays the generator's own output.
// The round is temporal_round::make_round's; its ready frames pass the generator in waves (frvsr_temporal_plan.h).
#pragma once
#include "bsvd_online.h"
#include "frvsr.h"
#include "temporal_round_plan.h"
#include "frvsr_temporal_plan.h"
#include "glue.h"
#include <memory>
#include <vector>

namespace ss4k {

// ---- the kernel of a wave (frvsr_temporal.hip) ---------------------------------------------------------------------------------------------------
// Item i: its denoised frame den[i] and its undenoised LR planes lr[i] (a slot of its stream's ring), 3 planes of (h, w) fp32 each, and dst[i],
// its stream's own lr buffer as FrvsrUpscaler::open_slots hands it out.  BY VALUE in the kernel arguments, as FrvsrPtrs / TroundTable: 1536
// bytes, no device table.
constexpr int FRVT_MAX_ITEMS = SS4K_FRVSR_MAX_STREAMS;
struct FrvtTable { const float* den[FRVT_MAX_ITEMS]; const float* lr[FRVT_MAX_ITEMS]; float* dst[FRVT_MAX_ITEMS]; };
static_assert(sizeof(FrvtTable) == 1536, "the wave's table travels in the kernel arguments: keep it far below 4 KiB");
// dst[i] = blend_a * clamp01(depthwise3x3_reflect(den[i], taps)) + blend_b * lr[i]: op_depthwise_reflect (k = 3, clamp, blend) per item, bit for
// bit, in one launch.  Refuses - before the launch - n_items outside 1..64, h < 2 or w < 2 (torch's reflect), 3 h w >= 2^31, NULL or misaligned
// pointers and a destination that overlaps its item's sources.
void op_frvt_denoised_in_items(const FrvtTable& tab, int n_items, int h, int w, const float* taps_dev, float blend_a, float blend_b, hipStream_t st);

// what one stream owns beside its recurrent state (FrvsrUpscaler::Slot): TemporalSlot without the cut detector
struct FrvtSlot {
  BsvdOnline on;
  DevBuf ring;          // lr_before of the frames inside the denoiser: (lag + max_push) frames of (3, lr_h, lr_w) fp32, frame i in slot i % frames
  bool first_frame = true;
  long long pushed = 0, emitted = 0;   // frames of the running stream
  double rate = -1;     // the stream's denoise rate (set_denoise_rate); negative: the object's.  Ends with the stream
  bool running() const { return on.state.pushed > 0; }
};

struct FrvsrTemporal {
  ss4k_ctx* ctx = nullptr;
  FrvsrUpscaler up;     // the generator's rounds, every stream's lr / hr state where it lives; its own frame entry points are not used
  std::vector<std::unique_ptr<FrvtSlot>> slots;   // max_streams of them, slot s beside up.slots[s]
  DevBuf lr4, den;      // job buffers, shared: the packed denoiser input of a round, the denoised frames of a round or a flush
  DevBuf k_sharp;       // the nine taps of sharpen_ker(strength = 0.00002), uploaded once
  double denoise_rate = 1.0;
  int max_push = 0;

  void create(ss4k_ctx* c, Frvsr* m, Model* bsvd_stream_model, int lr_h, int lr_w, int out_h, int out_w, double denoise_rate, int max_push, int max_streams);
  int max_streams() const { return (int)slots.size(); }
  int ring_frames() const { return bsvd_online::LAG + max_push; }
  FrvtSlot& slot(int s);
  const FrvtSlot& slot(int s) const;
  // A round (temporal_round_plan.h): k frames, frame i of slot slot_ids[i], each read where it lies.  The ready frames leave contiguously, item
  // after item, oldest first within an item; n_out_per_item / item_slots (k entries each) and *n_items describe them.  Returns their number.
  int round(const uint8_t* const* frames, const int* slot_ids, int k, int h, int w, uint8_t* out, size_t out_capacity_bytes, int* n_out_per_item,
            int* item_slots, int* n_items, hipStream_t st);
  // the up to 16 frames still inside a slot, through the generator in order; ends its stream
  int flush(int s, uint8_t* out, size_t out_capacity_bytes, hipStream_t st);
  void reset(int s);                       // drops the stream: denoiser state, LR ring and recurrent state count as gone
  int pending(int s) const { return slot(s).on.pending(); }
  void set_denoise_rate(int s, float rate);
  void out_shape(int* oh, int* ow) const { up.out_shape(oh, ow); }
  size_t state_bytes() const;              // the slots in use
  size_t stream_state_bytes_for() const;   // what one slot will hold, before any push
  void release_idle();                     // frees the state of slots with no running stream
  float level(const FrvtSlot& s) const { return (float)(0.1 * (s.rate < 0 ? denoise_rate : s.rate)); }   // fsrcnn_upscaler.py:269-271

 private:
  // one wave: open_slots, denoised_in_items, the step, close_slots, frames out.  den_of / ring_of / out_of: entry i's denoised frame, ring slot
  // and output frame
  void run_wave(const frvsr_temporal::Wave& wv, const float* const* den_of, const float* const* ring_of, uint8_t* const* out_of, hipStream_t st);
  void check_sizes(int h, int w) const;    // the launchers' size limits, restated
};

}  // namespace ss4k

struct ss4k_frvsr_temporal { ss4k::FrvsrTemporal t; };
