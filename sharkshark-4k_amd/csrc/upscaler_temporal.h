// The per-frame service chain with the online BSVD denoiser (upscaler_temporal.cpp), behind ss4k_upscaler_temporal (include/ss4k.h).
#pragma once
#include "bsvd_online.h"
#include "scene_cut.h"
#include "temporal_round_plan.h"
#include "temporal_motion_plan.h"
#include "upscaler.h"
#include <memory>
#include <vector>

namespace ss4k {

// Scene cuts for a temporal stream (include/ss4k.h: ss4k_upscaler_temporal_set_scene_cut): the rule of scene_cut.h on the job's input bytes,
// frame i against frame i - 1 of the job and frame 0 against a device copy of the previous job's last frame.  The flags never leave the
// device: BsvdOnline::push copies them into its ring, and the host learns about cuts only when it asks.  Created by the first
// set_scene_cut(threshold > 0); every device buffer is a DevBuf, so guard mode sees it.  One per stream slot, nothing shared.
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
  void reserve(size_t frame_bytes);   // the device buffers a job of such frames needs; detect / detect_at start with it
  void release_device();              // every device buffer goes and the counters start over (set(0), an idle slot's release); the threshold stays
  // the sums, cut::decide_run, the refresh of prev and of the pinned block; returns the job's n flag words (device)
  const uint32_t* detect(const uint8_t* in, int n, int hh, int ww, hipStream_t st);
  // ... the job's frames named one by one (a round's item: each frame lies where the caller has it, at any byte address)
  const uint32_t* detect_at(const uint8_t* const* fr, int n, int hh, int ww, hipStream_t st);
};

// ---- the kernel of a round (temporal_round.hip) -----------------------------------------------------------------------------------------------
// Frame j of a launch: its three LR planes at src[j] (3 * plane_px fp32, contiguous, 16-byte aligned - a slot of its stream's ring), and the device
// word that says whether it starts a scene (NULL: it does not), and the noise level of its stream's slot (read with four planes only).  prev[j]
// is read by the motion gathers alone: the three LR planes of the frame before it in its stream (NULL: it has none).  BY VALUE in the kernel
// arguments, as FrvsrPtrs: 1792 bytes, no device table.
constexpr int TROUND_MAX_FRAMES = temporal_round::MAX_FRAMES;
struct TroundTable {
  const float* src[TROUND_MAX_FRAMES]; const uint32_t* flag[TROUND_MAX_FRAMES]; float level[TROUND_MAX_FRAMES]; const float* prev[TROUND_MAX_FRAMES];
};
static_assert(sizeof(TroundTable) == 1792, "the round's table travels in the kernel arguments: keep it far below 4 KiB");
// dst (k, planes, plane_px) fp32: planes 0..2 of frame j from src[j]; with planes == 4, plane 3 is level_start where bit j of start_bits is set or
// *flag[j] != 0, and level[j] otherwise - the bits of bsvdo::noise_planes / the one-stream path's fill.  One launch, one thread per 16-byte slot.
void op_tround_gather(const TroundTable& tab, float* dst, int k, size_t plane_px, int planes, unsigned long long start_bits, float level_start,
                      hipStream_t st);
// The padded form of the four-plane gather, for the frame-recurrent chain at an lr_shape that 4 does not divide (frvsr_temporal.h): src[j] is
// (3, lh, lw) fp32 at any 4-byte address, dst (k, 4, ph, pw) with (ph, pw) = (lh, lw) rounded up to multiples of 4.  Planes 0..2 are padded at
// the bottom and on the right by 'reflect' (row y >= lh is row 2 (lh - 1) - y, columns likewise), plane 3 is the frame's level by the rule above,
// over the whole (ph, pw).  One launch.  Refuses - before the launch - what op_tround_gather refuses (a source need only be 4-byte aligned),
// lh < 4 or lw < 4, and 4 ph pw >= 2^31.
void op_tround_gather_pad(const TroundTable& tab, float* dst, int k, int lh, int lw, unsigned long long start_bits, float level_start,
                          hipStream_t st);

// ---- the motion-adaptive noise map (temporal_motion_plan.h has the rule) ------------------------------------------------------------------------
// op_tround_gather with four planes where plane 3 of frame j is a MAP: the constant level_start where bit j of start_bits is set, *flag[j] != 0 or
// prev[j] is NULL - the bits of op_tround_gather - and otherwise min(max(10 B, 0), 0.1f) * level[j], B the 3 x 3 Gaussian ('reflect' borders) of the
// mean over the planes of |src[j] - prev[j]|; level[j] carries temporal_round::motion_scale(rate).  fp32 throughout, in one fixed order per pixel:
// a pixel's bits depend on its own 54 inputs, the taps and level[j] alone.  One launch; a workgroup takes TROUND_MOTION_TILE_H x _W pixel tiles.
// Refuses - before the launch - what op_tround_gather refuses (with lh * lw for plane_px, and lw a multiple of 4: a row is whole 16-byte slots),
// lh < 2 or lw < 2, and a prev[j] that a frame needs (no start bit) and that is misaligned or overlaps the destination.
constexpr int TROUND_MOTION_TILE_H = 16, TROUND_MOTION_TILE_W = 64;
void op_tround_gather_motion(const TroundTable& tab, float* dst, int k, int lh, int lw, unsigned long long start_bits, float level_start, hipStream_t st);
// The padded form (op_tround_gather_pad's shapes and alignments): the map is computed on the (lh, lw) frame and padded to (ph, pw) by the same
// reflection as planes 0..2.  On a shape that 4 divides: the bits of op_tround_gather_motion.
void op_tround_gather_motion_pad(const TroundTable& tab, float* dst, int k, int lh, int lw, unsigned long long start_bits, float level_start,
                                 hipStream_t st);

// what one stream owns; allocated by its first push
struct TemporalSlot {
  BsvdOnline on;
  DevBuf ring;          // lr_before of the frames inside the denoiser: (lag + max_push) frames of (3, lr_h, lr_w) fp32, frame i in slot i % frames
  bool first_frame = true;
  std::unique_ptr<TemporalCut> cut;   // null until a threshold > 0 reaches the slot
  long long pushed = 0, emitted = 0;   // frames of the running stream
  double rate = -1;     // the stream's denoise rate (set_denoise_rate); negative: the object's cfg.denoise_rate.  Ends with the stream
  bool running() const { return on.state.pushed > 0; }
};

struct TemporalUpscaler {
  Upscaler up;          // the chain's glue, taps and SR model; its per-frame denoiser path is not used
  std::vector<std::unique_ptr<TemporalSlot>> slots;   // max_streams of them; the one-stream entry points are slot 0
  DevBuf lr4, den, den_flush, lrk, blend;             // job buffers, shared: the pushes of a round run one after the other
  double cut_threshold = 0;                           // what set_scene_cut last said; a slot's detector is made when the slot first needs it
  int max_push = 0;
  int noise_map = temporal_round::NOISE_MAP_CONSTANT; // set_noise_map: the denoiser's fourth plane, a constant per frame or the motion map

  void create(ss4k_ctx* c, const ss4k_upscale_cfg& cfg, Model* sr, Model* bsvd_stream_model, int max_push, int max_streams = 1);
  int max_streams() const { return (int)slots.size(); }
  int ring_frames() const { return bsvd_online::LAG + max_push; }
  TemporalSlot& slot(int s);
  const TemporalSlot& slot(int s) const;
  // n frames (n, h, w, 3) in -> the k frames that became ready, (k, oh, ow, 3), oldest first; returns k.  Slot 0.
  int frames(const uint8_t* in, int n, int h, int w, uint8_t* out, size_t out_capacity_bytes, hipStream_t st);
  // A round (temporal_round_plan.h): k frames, frame i of slot slot_ids[i], each read where it lies.  The ready frames leave contiguously, item
  // after item; n_out_per_item / item_slots (k entries each) and *n_items describe them.  Returns their number.
  int round(const uint8_t* const* frames, const int* slot_ids, int k, int h, int w, uint8_t* out, size_t out_capacity_bytes, int* n_out_per_item,
            int* item_slots, int* n_items, hipStream_t st);
  // the frames still inside a slot; ends its stream
  int flush(int s, uint8_t* out, size_t out_capacity_bytes, hipStream_t st);
  void reset(int s);
  size_t state_bytes() const;              // the slots in use
  size_t stream_state_bytes_for() const;   // what one slot will hold, before any push
  void release_idle();                     // frees the state of slots with no running stream
  void set_scene_cut(double threshold);    // every slot
  void set_denoise_rate(int s, float rate);   // the slot's frames from the next push or round on, until its stream ends
  float level(const TemporalSlot& s) const { return (float)(0.1 * (s.rate < 0 ? up.cfg.denoise_rate : s.rate)); }   // fsrcnn_upscaler.py:269-271
  // the motion map's scale for the slot's frames (temporal_motion_plan.h)
  float motion_level(const TemporalSlot& s) const { return temporal_round::motion_scale(s.rate < 0 ? up.cfg.denoise_rate : s.rate); }
  bool motion() const { return noise_map == temporal_round::NOISE_MAP_MOTION; }
  void set_noise_map(int mode);            // refused while any slot has a running stream

 private:
  void emit(TemporalSlot& s, int k, const float* denoised, uint8_t* out, hipStream_t st);
  void want_cut(TemporalSlot& s);
};

}  // namespace ss4k

struct ss4k_upscaler_temporal { ss4k::TemporalUpscaler t; };
