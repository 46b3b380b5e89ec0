// The plan of one ROUND of a temporal upscaler with stream slots (upscaler_temporal.cpp, TemporalUpscaler::round): K frames of several streams,
// each frame named by its slot, become items - one per slot, in order of the slot's first appearance - and every item is one push of that slot's
// online denoiser.  A pure function of (the K slot numbers, every slot's bsvd_online::State, max_push, max_streams, the output capacity): no HIP,
// no allocation and no #include - bsvd_online_plan.h goes in front of it.  tests/test_temporal_round_plan_cpu.py replays random rounds against a
// naive per-stream simulation.
//
// Where things sit.  Frame i of a stream waits for its denoised self in slot i % (LAG + max_push) of the stream's LR ring.  An item's denoised
// frames land at den_off in the round's contiguous denoised buffer and at the same offset, in frames, in the output: the output is item after item,
// oldest first within an item.  The tail then runs over the round's E ready frames in chunks of at most max_push frames, whatever stream they
// belong to, so the SR workspace of a round never exceeds that of a one-stream object with the same max_push.
#pragma once

namespace ss4k {
namespace temporal_round {

constexpr int MAX_FRAMES = 64;    // cut::MAX_ITEMS: frames of a round
constexpr int MAX_STREAMS = 64;   // slots of an object

struct Item {
  int slot = 0;
  int first = 0, n = 0;     // its frames: Plan::order[first .. first + n), in the caller's order
  int emitted = 0;          // make_plan(state, n, false).emitted
  int den_off = 0;          // offset of its ready frames in the denoised buffer and in the output, in frames; Plan::ring_out[den_off ..]
  bsvd_online::State before, after;
};

struct Plan {
  const char* refusal = nullptr;   // non-null: the round is refused for this reason and nothing below is valid
  int k = 0, n_items = 0;
  Item items[MAX_FRAMES];
  int order[MAX_FRAMES] = {};      // the caller's frame indices, item after item
  int ring_in[MAX_FRAMES] = {};    // ring slot (of its own stream's ring) that frame order[j] enters
  int total = 0;                   // E: the frames that leave with this round
  int ring_out[MAX_FRAMES] = {};   // ring slot that output frame e leaves
  int n_chunks = 0;                // the tail: chunk c is output frames [chunk_off[c], chunk_off[c] + chunk_n[c])
  int chunk_off[MAX_FRAMES] = {}, chunk_n[MAX_FRAMES] = {};
};

inline int ring_frames(int max_push) { return bsvd_online::LAG + max_push; }

// slots[0 .. k): the slot of every frame; states[0 .. max_streams): every slot's state (a slot never pushed: State{})
inline Plan make_round(const int* slots, int k, const bsvd_online::State* states, int max_push, int max_streams, long long out_capacity_frames) {
  Plan p;
  if (max_push < 1 || max_push > MAX_FRAMES || max_streams < 1 || max_streams > MAX_STREAMS) { p.refusal = "temporal round: max_push and max_streams are 1..64"; return p; }
  if (!slots || !states) { p.refusal = "temporal round: NULL argument"; return p; }
  if (k < 1 || k > MAX_FRAMES) { p.refusal = "temporal round: a round holds 1..64 frames"; return p; }
  int item_of[MAX_STREAMS];
  for (int s = 0; s < MAX_STREAMS; ++s) item_of[s] = -1;
  for (int i = 0; i < k; ++i) {
    const int s = slots[i];
    if (s < 0 || s >= max_streams) { p.refusal = "temporal round: a slot outside 0..max_streams-1"; return p; }
    if (item_of[s] < 0) { item_of[s] = p.n_items; p.items[p.n_items].slot = s; p.items[p.n_items].n = 0; ++p.n_items; }
    if (++p.items[item_of[s]].n > max_push) { p.refusal = "temporal round: more than max_push frames for one slot"; return p; }
  }
  p.k = k;
  const int R = ring_frames(max_push);
  int first = 0, e = 0;
  for (int t = 0; t < p.n_items; ++t) {
    Item& it = p.items[t];
    const bsvd_online::Plan push = bsvd_online::make_plan(states[it.slot], it.n, false);
    it.first = first; it.emitted = push.emitted; it.den_off = e; it.before = push.before; it.after = push.after;
    int j = 0;
    for (int i = 0; i < k; ++i) {
      if (slots[i] != it.slot) continue;
      p.order[first + j] = i;
      p.ring_in[first + j] = (it.before.pushed + j) % R;
      ++j;
    }
    const int out0 = bsvd_online::emitted_total(it.before);
    for (int q = 0; q < it.emitted; ++q) p.ring_out[e + q] = (out0 + q) % R;
    first += it.n; e += it.emitted;
  }
  p.total = e;
  if (out_capacity_frames < (long long)e) { p.refusal = "temporal round: output buffer too small for the frames that become ready"; return p; }
  for (int off = 0; off < e; off += max_push) {
    p.chunk_off[p.n_chunks] = off;
    p.chunk_n[p.n_chunks] = e - off < max_push ? e - off : max_push;
    ++p.n_chunks;
  }
  return p;
}

}  // namespace temporal_round
}  // namespace ss4k
