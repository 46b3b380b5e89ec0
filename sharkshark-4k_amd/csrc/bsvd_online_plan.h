// The plan of one push (or one flush round) of the online BSVD executor (bsvd_online.cpp): which frames every tensor gains, where they sit
// in the carried buffers, and how many frames leave.  A pure function of (frames pushed so far, the feed clock, n, flushing): no HIP, no
// allocation - tests/test_bsvd_online_plan_cpu.py replays it against a frame-by-frame simulation of the reference's machine
// (bsvd/model.py:59-138 BiBufferConv, :332-350 MemSkip, :402-424 DenBlock.forward).
//
// Lags.  The 16 BiBufferConvs are numbered 1..16 in execution order, 8 per DenBlock.  A tensor behind j of them has lag j: once the feed
// clock stands at c (c calls of feedin_one_element so far, the draining None calls included) it is complete up to frame min(pushed, c - j) - 1.
// A push of n frames moves the clock by n, so a tensor of lag j gains the WINDOW [min(pushed0, clock0 - j), min(pushed1, clock1 - j)) (clamped at 0).
// BiBufferConv j emits frame t from frames t - 1, t, t + 1 of its input (lag j - 1); t + 1 lies beyond the input only while flushing (zeros).
//
// Carried tensors.  A tensor that a LATER lag reads again keeps `hist` frames in front of each window: buffer slot s holds stream frame
// (window.lo - hist + s).  After the push the last `hist` slots move to the front.  hist = 2 for a BiBufferConv's input (frames t - 1 and t of
// the next window's first output), and the lag difference for a skip partner (MemSkip): 4 for X1, 8 for X0 and for the block input.
#pragma once

namespace ss4k {
namespace bsvd_online {

constexpr int LAG = 16;         // BiBufferConvs of the network
constexpr int BLOCK_LAG = 8;    // ... of one DenBlock

// carried tensors of one DenBlock, in the order they are produced
enum Carried { C_IN = 0, C_X0, C_D0, C_MA, C_X1, C_D1, C_MB, C_X2, C_MC, C_S1, C_MA2, C_COUNT };
struct CarriedSpec { int lag, hist, res; };   // lag inside the block; res: 0 full resolution, 1 half, 2 quarter
// D0 -1-> MA -2-> X1 -> D1 -3-> MB -4-> X2 -5-> MC -6-> (Mb') -> S1 (+ X1) -7-> MA2 -8-> (D0') -> S0 (+ X0) -> out (IN - .)
constexpr CarriedSpec CARRIED[C_COUNT] = {
    {0, 8, 0},   // C_IN : the block input; its RGB meets outc's output at lag 8 (skip1)
    {0, 8, 0},   // C_X0 : inc's output; meets upc1's PixelShuffle at lag 8 (skip2); downc0 reads its window
    {0, 2, 1},   // C_D0 : input of BiBufferConv 1
    {1, 2, 1},   // C_MA : input of BiBufferConv 2
    {2, 4, 1},   // C_X1 : meets upc2's PixelShuffle at lag 6 (skip3); downc1 reads its window
    {2, 2, 2},   // C_D1 : input of BiBufferConv 3
    {3, 2, 2},   // C_MB : input of BiBufferConv 4
    {4, 2, 2},   // C_X2 : input of BiBufferConv 5
    {5, 2, 2},   // C_MC : input of BiBufferConv 6
    {6, 2, 1},   // C_S1 : input of BiBufferConv 7
    {7, 2, 1},   // C_MA2: input of BiBufferConv 8
};
// the carried input of BiBufferConv k (1..8) of a block
constexpr int BIBUF_INPUT[BLOCK_LAG] = {C_D0, C_MA, C_D1, C_MB, C_X2, C_MC, C_S1, C_MA2};

struct Window { int lo, hi; int count() const { return hi - lo; } };

struct State {
  int pushed = 0;   // real frames fed so far
  int clock = 0;    // feed calls so far: pushed + the None calls of a flush in progress
};

struct Plan {
  State before, after;
  bool flushing = false;
  Window win[LAG + 1];   // by lag
  int emitted = 0;       // win[LAG].count(): frames that leave with this push, oldest first

  // slot of stream frame f in carried tensor c of block b during this push (slot 0 may lie before frame 0 of the stream: never read)
  int slot_of(int b, int c, int f) const { return f - (win[b * BLOCK_LAG + CARRIED[c].lag].lo - CARRIED[c].hist); }
  // first slot the push writes, and how many
  int write_slot(int c) const { return CARRIED[c].hist; }
  int write_count(int b, int c) const { return win[b * BLOCK_LAG + CARRIED[c].lag].count(); }
  // frames of carried tensor c of block b that a later push still reads: the carry's extent, at most CARRIED[c].hist
  int carry_extent(int b, int c) const {
    const int a = b * BLOCK_LAG + CARRIED[c].lag;
    int oldest;   // first frame a later push reads
    if (c == C_IN || c == C_X0) oldest = win[b * BLOCK_LAG + 8].hi;
    else if (c == C_X1) oldest = win[b * BLOCK_LAG + 6].hi;
    else oldest = win[a + 1].hi > 0 ? win[a + 1].hi - 1 : 0;   // frame t - 1 of the consumer's next output
    return win[a].hi - oldest;
  }
  // BiBufferConv j (1..LAG) emitting frame t: are its neighbours zeros?
  bool prev_is_zero(int t) const { return t - 1 < 0; }
  bool next_is_zero(int j, int t) const { return t + 1 >= win[j - 1].hi; }   // (only while flushing: make_plan's windows guarantee it)
};

inline int frames_done(int pushed, int clock, int lag) {
  int v = clock - lag;
  if (v < 0) v = 0;
  return v < pushed ? v : pushed;
}

// n real frames (flushing = false) or n None calls (flushing = true)
inline Plan make_plan(const State& s, int n, bool flushing) {
  Plan p;
  p.before = s; p.flushing = flushing;
  p.after.pushed = s.pushed + (flushing ? 0 : n);
  p.after.clock = s.clock + n;
  for (int j = 0; j <= LAG; ++j) {
    p.win[j].lo = frames_done(s.pushed, s.clock, j);
    p.win[j].hi = frames_done(p.after.pushed, p.after.clock, j);
  }
  p.emitted = p.win[LAG].count();
  return p;
}

// frames emitted so far / still inside: known on the host without a synchronisation
inline int emitted_total(const State& s) { return frames_done(s.pushed, s.clock, LAG); }
inline int pending(const State& s) { return s.pushed - emitted_total(s); }
// None calls that drain a stream
inline int flush_calls(const State& s) { const int left = s.pushed + LAG - s.clock; return s.pushed == 0 || left < 0 ? 0 : left; }

}  // namespace bsvd_online
}  // namespace ss4k
