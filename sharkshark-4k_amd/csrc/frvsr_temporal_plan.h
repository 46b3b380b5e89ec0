// The tail of one round of the frame-recurrent chain with the online denoiser in front (frvsr_temporal.cpp, FrvsrTemporal::round).  The round
// itself - items, ring slots, den_off, refusals - is temporal_round::make_round, unchanged.  What differs is what follows the denoiser: the
// per-frame chain runs ONE tail over everything that became ready, the recurrent generator cannot - frame t of a stream needs frame t - 1's
// output.  So the ready frames leave in WAVES: wave r holds, for every item that emitted more than r frames, that item's r-th ready frame.  A wave
// is one FrvsrUpscaler round: its slots are distinct because the items of a round are (one item per slot), and a stream's frames pass in order
// because wave r comes before wave r + 1.  The number of waves is the largest `emitted` of the round.
// A pure function of the plan: no GPU call, no allocation and no #include - bsvd_online_plan.h and temporal_round_plan.h go in front of it.
// tests/test_frvsr_temporal_plan_cpu.py replays random rounds and flushes against a naive per-stream simulation.
//
// Scene cuts.  A stream that carries cut flags keeps them in its denoiser's ring of CUT_RING words, stream frame f at f & (CUT_RING - 1)
// (bsvd_online.h).  A frame's flag acts a second time when the frame LEAVES the denoiser, LAG frames after it went in: the wave that holds it
// zeroes the stream's lr_prev / hr_prev first (frvt::clear_flagged_items).  So every wave entry names the stream frame number of its leaving
// frame, and ring_word() says where that frame's word sits.  The word is still the frame's own: a push writes the words of the frames it brings
// and of no others, a frame that leaves with a push has at most LAG + max_push - 1 newer frames behind it, and the frames a flush drains have at
// most LAG - 1 - a flush writes no word at all.  (After BsvdOnline::flush() the ring's contents stay what they were until the NEXT stream's
// first push with flags zero-fills them on its stream; the flush waves run after flush() on the same stream and before any such push, so they
// read the words the ended stream wrote.)  tests/test_frvsr_temporal_cuts_plan_cpu.py replays that against a naive ring.
#pragma once

namespace ss4k {
namespace frvsr_temporal {

constexpr int MAX_WAVES = temporal_round::MAX_FRAMES;   // an item emits at most max_push <= 64 frames
constexpr int MAX_WAVE_ITEMS = temporal_round::MAX_STREAMS;
constexpr int CUT_RING = 128;     // BSVD_ONLINE_CUT_RING (frvsr_temporal.h asserts the two are one number)
static_assert((CUT_RING & (CUT_RING - 1)) == 0, "the flag ring is addressed with a mask");
static_assert(bsvd_online::LAG + temporal_round::MAX_FRAMES <= CUT_RING,
              "a word written by a push must still be its frame's own when the frame leaves: LAG + max_push <= the ring, flushes included");

struct Wave {
  int n = 0;                       // entries: 1..max_streams
  int slot[MAX_WAVE_ITEMS] = {};   // the stream slot of entry i (distinct within the wave)
  int item[MAX_WAVE_ITEMS] = {};   // the round's item it belongs to (flush: 0)
  int out[MAX_WAVE_ITEMS] = {};    // its index in the denoised buffer and in the output, in frames: den_off + r
  int frame[MAX_WAVE_ITEMS] = {};  // the stream frame number of the leaving frame: what its slot had emitted before this wave
};

struct Waves {
  int n_waves = 0;                 // max(emitted) over the items
  Wave w[MAX_WAVES];
};

// the waves of a round that make_round accepted (a refused plan has none)
inline Waves make_waves(const temporal_round::Plan& p) {
  Waves v;
  if (p.refusal) return v;
  for (int t = 0; t < p.n_items; ++t)
    if (p.items[t].emitted > v.n_waves) v.n_waves = p.items[t].emitted;
  for (int r = 0; r < v.n_waves; ++r) {
    Wave& wv = v.w[r];
    for (int t = 0; t < p.n_items; ++t) {
      const temporal_round::Item& it = p.items[t];
      if (it.emitted <= r) continue;
      wv.slot[wv.n] = it.slot; wv.item[wv.n] = t; wv.out[wv.n] = it.den_off + r;
      wv.frame[wv.n] = bsvd_online::emitted_total(it.before) + r;
      ++wv.n;
    }
  }
  return v;
}

// a flush of the n frames still inside one slot (0..LAG): n waves of one, output frame r in wave r.  emitted: the frames the slot's stream has
// returned so far, the stream frame number of the flush's first frame
inline Waves make_flush(int slot, int n, int emitted = 0) {
  Waves v;
  if (n < 0 || n > MAX_WAVES) return v;
  v.n_waves = n;
  for (int r = 0; r < n; ++r) { v.w[r].n = 1; v.w[r].slot[0] = slot; v.w[r].item[0] = 0; v.w[r].out[0] = r; v.w[r].frame[0] = emitted + r; }
  return v;
}

// where the cut flag of stream frame f sits in its stream's flag ring
inline int ring_word(int frame) { return frame & (CUT_RING - 1); }

}  // namespace frvsr_temporal
}  // namespace ss4k
