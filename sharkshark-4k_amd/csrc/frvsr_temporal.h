// The frame-recurrent service chain with the online BSVD denoiser in front (frvsr_temporal.cpp), behind ss4k_frvsr_temporal (include/ss4k.h):
// what TemporalUpscaler is to the per-frame chain.  Per stream, frame t:
//   lr_before_t = area(img / 255, lr_shape)                                             (egvsr_upscaler.py:195-196)
//   den_t       = the online denoiser's output for frame t of the stream of (lr_before, noise) inputs; noise 0.05 for a stream's first frame,
//                 0.1 * rate after (fsrcnn_upscaler.py:262,269-271); it exists once frame t + 16 has entered, or at a flush
//   lr_curr_t   = 0.8 * clamp01(sharpen3x3_reflect(den_t)) + 0.2 * lr_before_t           (fsrcnn_upscaler.py:279-281)
//   hr_t        = FRNet(lr_curr_t, lr_curr_{t-1}, hr_{t-1}), zeros for a stream's first frame; clamp, area to output_shape, * 255 truncated
// An lr_shape (lh, lw) that 4 does not divide (create with allow_pad; include/ss4k.h: ss4k_frvsr_temporal_create_padded): the denoiser alone runs
// at (ph, pw), (lh, lw) rounded up to multiples of 4.  Its input is lr_before padded at the bottom and on the right by 'reflect' (row y >= lh is
// row 2 (lh - 1) - y, columns likewise; the noise plane its constant over (ph, pw)), its output is cropped to the top-left (lh, lw) before the
// sharpening, whose own reflection is at the crop's borders.  The ring, the generator, its state, the detector and the output stay at (lh, lw).
// Nothing of the per-frame tail follows (no HR sharpening, no mean / std match): hr_prev stays the generator's own output.
// The round is temporal_round::make_round's; its ready frames pass the generator in waves (frvsr_temporal_plan.h).
#pragma once
#include "bsvd_online.h"
#include "frvsr.h"
#include "temporal_round_plan.h"
#include "frvsr_temporal_plan.h"
#include "glue.h"
#include "upscaler_temporal.h"   // TemporalCut: a slot's detector, the one TemporalSlot holds
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
// The cropped form: den[i] is 3 planes of (ph, pw) >= (h, w), of which the top-left (h, w) are the frame; lr[i] and dst[i] stay (3, h, w).  The
// reflection is at the crop's borders, the rest of den is never read; bit for bit op_frvt_denoised_in_items on a contiguous copy of the crop.
// Refuses what that one refuses, ph < h or pw < w, 3 ph pw >= 2^31; the overlap check takes den at its own, larger size.
void op_frvt_denoised_in_crop_items(const FrvtTable& tab, int n_items, int h, int w, int ph, int pw, const float* taps_dev, float blend_a,
                                    float blend_b, hipStream_t st);

// ---- the late reset of a scene cut (frvsr_temporal.hip) -------------------------------------------------------------------------------------------
// Item i: the device word that says whether the frame that leaves the denoiser in this wave starts a scene - its stream's flag ring at the
// frame's number (frvsr_temporal_plan.h: ring_word), NULL for a stream without a live ring - and the stream's lr_prev / hr_prev as
// FrvsrUpscaler::open_slots hands them out.  BY VALUE in the kernel arguments, as FrvtTable: 1536 bytes, no device table.
struct FrvtClearTable { const uint32_t* flag[FRVT_MAX_ITEMS]; void* lr[FRVT_MAX_ITEMS]; void* hr[FRVT_MAX_ITEMS]; };
static_assert(sizeof(FrvtClearTable) == 1536, "the wave's table travels in the kernel arguments: keep it far below 4 KiB");
static_assert(frvsr_temporal::CUT_RING == BSVD_ONLINE_CUT_RING, "the wave plan addresses the denoiser's flag ring: one size");
// lr[i] (lr_bytes) and hr[i] (hr_bytes) become zero for every item whose flag pointer is not NULL and whose word is not 0: what open_slots gives
// a stream's first frame (cut::clear_items with the flag read where the ring keeps it).  One launch.  Refuses - before the launch - n_items
// outside 1..64, a size that is 0 or no multiple of 4, and a NULL or not 16-byte aligned lr / hr of ANY item; a flag pointer is NULL or 4-byte
// aligned.
void op_frvt_clear_flagged_items(const FrvtClearTable& tab, int n_items, size_t lr_bytes, size_t hr_bytes, hipStream_t st);

// what one stream owns beside its recurrent state (FrvsrUpscaler::Slot): TemporalSlot
struct FrvtSlot {
  BsvdOnline on;
  DevBuf ring;          // lr_before of the frames inside the denoiser: (lag + max_push) frames of (3, lr_h, lr_w) fp32, frame i in slot i % frames
  bool first_frame = true;
  std::unique_ptr<TemporalCut> cut;   // null until a threshold > 0 reaches the slot
  long long pushed = 0, emitted = 0;   // frames of the running stream
  double rate = -1;     // the stream's denoise rate (set_denoise_rate); negative: the object's.  Ends with the stream
  bool running() const { return on.state.pushed > 0; }
};

struct FrvsrTemporal {
  ss4k_ctx* ctx = nullptr;
  FrvsrUpscaler up;     // the generator's rounds, every stream's lr / hr state where it lives; its own frame entry points are not used
  std::vector<std::unique_ptr<FrvtSlot>> slots;   // max_streams of them, slot s beside up.slots[s]
  DevBuf lr4, den;      // job buffers, shared: the packed denoiser input of a round, the denoised frames of a round or a flush - at (pad_h, pad_w)
  int pad_h = 0, pad_w = 0;   // the denoiser's shape: lr_shape rounded up to multiples of 4 - lr_shape itself unless created with allow_pad
  DevBuf k_sharp;       // the nine taps of sharpen_ker(strength = 0.00002), uploaded once
  double denoise_rate = 1.0;
  double cut_threshold = 0;   // what set_scene_cut last said; a slot's detector is made when the slot first needs it
  int max_push = 0;
  int noise_map = temporal_round::NOISE_MAP_CONSTANT;   // set_noise_map: the denoiser's fourth plane, a constant per frame or the motion map

  void create(ss4k_ctx* c, Frvsr* m, Model* bsvd_stream_model, int lr_h, int lr_w, int out_h, int out_w, double denoise_rate, int max_push, int max_streams,
              bool allow_pad = false);
  bool padded() const { return pad_h != up.lr_h || pad_w != up.lr_w; }
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
  // Scene cuts, every slot (include/ss4k.h: ss4k_frvsr_temporal_set_scene_cut).  0: detection stops, the stored frames and the counters go; flags
  // already in a ring keep acting - on the denoiser and, when their frames leave, on the generator
  void set_scene_cut(double threshold);
  void out_shape(int* oh, int* ow) const { up.out_shape(oh, ow); }
  size_t state_bytes() const;              // the slots in use
  size_t stream_state_bytes_for() const;   // what one slot will hold, before any push
  void release_idle();                     // frees the state of slots with no running stream
  float level(const FrvtSlot& s) const { return (float)(0.1 * (s.rate < 0 ? denoise_rate : s.rate)); }   // fsrcnn_upscaler.py:269-271
  // the motion map's scale for the slot's frames (temporal_motion_plan.h)
  float motion_level(const FrvtSlot& s) const { return temporal_round::motion_scale(s.rate < 0 ? denoise_rate : s.rate); }
  bool motion() const { return noise_map == temporal_round::NOISE_MAP_MOTION; }
  void set_noise_map(int mode);            // refused while any slot has a running stream

 private:
  // one wave: open_slots, the late reset if a stream of the wave carries cut flags, denoised_in_items, the step, close_slots, frames out.
  // den_of / ring_of / out_of: entry i's denoised frame, ring slot and output frame; flag_of: NULL (no entry has a live flag ring) or entry i's
  // word in its stream's flag ring, NULL for an entry without one
  void run_wave(const frvsr_temporal::Wave& wv, const float* const* den_of, const float* const* ring_of, uint8_t* const* out_of,
                const uint32_t* const* flag_of, hipStream_t st);
  void check_sizes(int h, int w) const;    // the launchers' size limits, restated
  void want_cut(FrvtSlot& s);              // the detector of a slot that has none yet, once a threshold is set
};

}  // namespace ss4k

struct ss4k_frvsr_temporal { ss4k::FrvsrTemporal t; };
