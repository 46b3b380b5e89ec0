// BSVD as the reference's online machine (bsvd/model.py:510-513 feedin_one_element): a stateful denoiser whose temporal state crosses job
// boundaries.  A BsvdOnline holds a Model built with bsvd_stream = 1 the way Frvsr holds one - a container of layers, packed weights and
// workspaces, run through Model::conv / conv_pair - plus the per-stream history the 16 BiBufferConvs and the three MemSkip queues of each
// DenBlock need between pushes.  The frames it emits are bit-identical to one clip forward over all frames of the stream.
// What runs when is decided by bsvd_online_plan.h; this file executes the plan.  Kernels: bsvd_online.hip.
#pragma once
#include "bsvd_online_plan.h"
#include "models.h"

namespace ss4k {

// ---- kernels (bsvd_online.hip); records are the conv kernels' planes layout, one thread per 16-byte slot, grid-stride -------------------
// The ShiftConv input of `frames` consecutive output frames of a BiBufferConv whose input lives in a carried buffer: `in` holds in_frames
// frames per plane, output frame i has its centre in slot slot0 + i.  Channels [0, fold) come from slot + 1, zeros for output frames
// i >= n_next (the stream ends there: flushing); [fold, 2 fold) from slot - 1, zeros for i = 0 unless first_has_prev; the rest of the
// leading planes from the centre.  out: nplanes planes of `frames` frames.
void op_bsvd_online_shift(const void* in, void* out, int nplanes, int in_frames, int slot0, int frames, size_t frame_px, int slots_per_record,
                          int ch_per_plane, int fold, int first_has_prev, int n_next, hipStream_t st);
// Scene cuts.  flag_ring[f & ring_mask] != 0: stream frame f is the first frame of a new scene.  The ring holds BSVD_ONLINE_CUT_RING frames: the
// oldest frame any window of a push still reads is pushed - LAG - 8 (the last BiBufferConv's window starts LAG frames behind the frames pushed
// before, and the deepest history - a skip partner's - lies 8 frames in front of a window), the newest is the push's last one, max_push <= 64
// frames further on.
constexpr int BSVD_ONLINE_MAX_PUSH = 64;
constexpr int BSVD_ONLINE_MAX_HIST = 8;
constexpr int BSVD_ONLINE_CUT_RING = 128;
static_assert((BSVD_ONLINE_CUT_RING & (BSVD_ONLINE_CUT_RING - 1)) == 0, "the flag ring is addressed with a mask");
static_assert(bsvd_online::LAG + BSVD_ONLINE_MAX_HIST + BSVD_ONLINE_MAX_PUSH <= BSVD_ONLINE_CUT_RING, "a push's windows reach further back than the flag ring holds");
constexpr bool bsvd_online_hist_fits() {
  for (int c = 0; c < bsvd_online::C_COUNT; ++c) if (bsvd_online::CARRIED[c].hist > BSVD_ONLINE_MAX_HIST) return false;
  return true;
}
static_assert(bsvd_online_hist_fits(), "a carried tensor's history is deeper than BSVD_ONLINE_MAX_HIST");
// The cut-aware build of the shift: the same arguments plus the ring, its mask (2^k - 1) and f0, the stream frame number of output frame 0.
// The "next" group of output frame t is live only if it is live in op_bsvd_online_shift AND flag[f0 + t + 1] is 0, the "previous" group only
// if it is live there AND flag[f0 + t] is 0; the centre group and everything else are the same.
void op_bsvd_online_shift_cuts(const void* in, void* out, int nplanes, int in_frames, int slot0, int frames, size_t frame_px, int slots_per_record,
                               int ch_per_plane, int fold, int first_has_prev, int n_next, const uint32_t* flag_ring, unsigned ring_mask, int f0,
                               hipStream_t st);
// The noise plane (channel 3) of each of the n packed (4, h, w) fp32 input frames of a push, one launch: level_start where the frame starts a
// scene - flags[i] != 0, or i == 0 and stream_first - and level otherwise.  flags: n device words.
void op_bsvd_noise_planes(float* frames4, int n, size_t plane_px, const uint32_t* flags, int stream_first, float level_start, float level,
                          hipStream_t st);
// The carry / history update, one launch for every carried tensor of a push: entry e copies, in each of its planes, `count` frames starting
// at frame src_first of src (src_frames frames per plane) to the front of dst (dst_frames frames per plane).  src and dst never overlap
// (ping-pong pairs), so a tensor that gained fewer frames than its history is deep moves correctly.  The table travels BY VALUE in the
// kernel arguments: no device table, no upload.
constexpr int BSVD_ONLINE_MAX_CARRIES = 2 * bsvd_online::C_COUNT;
struct BsvdCarry { const void* src; void* dst; int nplanes, src_frames, dst_frames, src_first, count; unsigned frame_slots; };
struct BsvdCarryTable { BsvdCarry e[BSVD_ONLINE_MAX_CARRIES]; };
void op_bsvd_online_carry(const BsvdCarryTable& tab, int entries, hipStream_t st);

struct BsvdOnline {
  ss4k_ctx* ctx = nullptr;
  Model* net = nullptr;        // BSVD, bsvd_stream = 1; not owned
  int max_push = 0;
  int h = 0, w = 0;            // the stream's frame size (0: no push yet)
  bsvd_online::State state{};
  // carried tensors: a ping-pong pair each, (hist + max_push) frames per plane; cur[] names the buffer that holds the history
  DevBuf carried[2][bsvd_online::C_COUNT][2];
  int cur[2][bsvd_online::C_COUNT] = {};
  // scene cuts: the flag ring (BSVD_ONLINE_CUT_RING words, frame f at f & mask), allocated and zeroed by the stream's first push that brings
  // flags.  From then on the stream runs the cut-aware shift - its flush rounds too - until reset() or the end of flush()
  DevBuf flag_ring;
  bool cuts_live = false;

  void create(ss4k_ctx* c, Model* m, int max_push_);
  int lag() const { return bsvd_online::LAG; }
  int pending() const { return bsvd_online::pending(state); }
  size_t state_bytes() const;
  // what the state will hold at (h, w): the plan's figure, known before the first push
  size_t state_bytes_for(int hh, int ww) const;
  // (the ring counts as zero again: the next stream's first push with flags zero-fills it on its stream before it writes into it)
  void reset() { state = bsvd_online::State{}; h = w = 0; cuts_live = false; }
  // reset() and the memory back: the next stream's first push allocates again (a temporal upscaler's idle slot)
  void release_state() {
    reset();
    for (auto& blk : carried) for (auto& pr : blk) for (auto& b : pr) b.release();
    flag_ring.release();
  }
  // in (n, 4, h, w) fp32 NCHW -> the frames that became ready, oldest first, (k, 3, h, w) fp32 NCHW; returns k.
  // cuts_dev: n device words read in stream order (an earlier kernel on st may have produced them), word i != 0: frame i of the push is the
  // first of a new scene; NULL: no cut in this push.  A flag on the stream's first frame has no effect.
  int push(const float* in, int n, int hh, int ww, float* out, size_t out_capacity_frames, hipStream_t st, const uint32_t* cuts_dev = nullptr);
  // the remaining min(lag, pushed) frames, in rounds of at most max_push feed calls; then reset()
  int flush(float* out, size_t out_capacity_frames, hipStream_t st);

 private:
  int channels_of(int b, int c) const;
  int planes_of(int b, int c) const;
  size_t frame_bytes(int c) const;
  int cap_frames(int c) const { return bsvd_online::CARRIED[c].hist + max_push; }
  void ensure_state();
  void ring_write(const uint32_t* cuts_dev, int first, int n, hipStream_t st);
  void run(const bsvd_online::Plan& p, const float* in, float* out, hipStream_t st);
};

}  // namespace ss4k

struct ss4k_bsvd_online { ss4k::BsvdOnline o; };
