// Stand-alone check of csrc/bsvd_online_plan.h (tests/test_bsvd_online_plan_cpu.py compiles it with -fsanitize=address,undefined and runs it).
// Random push schedules are replayed against a frame-by-frame simulation of the reference's machine - sixteen one-frame BiBufferConv buffers
// and the three MemSkip queues of each DenBlock (bsvd/model.py:59-138, 332-350, 402-424), on frame NUMBERS instead of tensors.
#include "../sharkshark-4k_amd/csrc/bsvd_online_plan.h"
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

using namespace ss4k::bsvd_online;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

constexpr int NONE = -1, ZEROS = -2;

// one emission of a BiBufferConv: frame t from (left, t, right); left / right are frame numbers or ZEROS
struct Emit { int t, left, right; };

struct BiBuffer {   // BiBufferConv.forward
  int center = NONE, left = ZEROS;
  bool feed(int in, Emit* out) {
    if (center == NONE) { center = in; return false; }   // (start stage, or end stage with an empty memory)
    *out = Emit{center, left, in == NONE ? ZEROS : in};
    left = center; center = in;
    return true;
  }
};

struct Block {   // DenBlock.forward on frame numbers; log[j]: what the tensor of block lag j gained in this call (NONE: nothing)
  BiBuffer mem[BLOCK_LAG];
  std::deque<int> skip1, skip2, skip3;
  int feed(int in, int gained[BLOCK_LAG + 1], Emit emits[BLOCK_LAG + 1]) {
    for (int j = 0; j <= BLOCK_LAG; ++j) gained[j] = NONE;
    if (in != NONE) { skip1.push_front(in); skip2.push_front(in); }
    gained[0] = in;
    int x = in;
    auto stage = [&](int k) {   // BiBufferConv k (1..8); a None input still clocks it
      Emit e{};
      x = mem[k - 1].feed(x, &e) ? e.t : NONE;
      gained[k] = x; emits[k] = e;
    };
    stage(1); stage(2);
    if (x != NONE) skip3.push_front(x);
    stage(3); stage(4); stage(5); stage(6);
    if (x != NONE) { CHECK(!skip3.empty() && skip3.back() == x, "skip3 pops frame %d for frame %d", skip3.empty() ? -9 : skip3.back(), x); if (!skip3.empty()) skip3.pop_back(); }
    stage(7); stage(8);
    if (x != NONE) {
      CHECK(!skip2.empty() && skip2.back() == x, "skip2 pops the wrong frame for %d", x); if (!skip2.empty()) skip2.pop_back();
      CHECK(!skip1.empty() && skip1.back() == x, "skip1 pops the wrong frame for %d", x); if (!skip1.empty()) skip1.pop_back();
    }
    return x;
  }
};

struct Machine {
  Block blk[2];
  // one feedin_one_element: gained[j] for the global lags 0..16
  int feed(int in, int gained[LAG + 1], Emit emits[LAG + 1]) {
    int g[BLOCK_LAG + 1]; Emit e[BLOCK_LAG + 1];
    int x = blk[0].feed(in, g, e);
    for (int j = 0; j <= BLOCK_LAG; ++j) { gained[j] = g[j]; emits[j] = e[j]; }
    x = blk[1].feed(x, g, e);
    for (int j = 1; j <= BLOCK_LAG; ++j) { gained[BLOCK_LAG + j] = g[j]; emits[BLOCK_LAG + j] = e[j]; }
    return x;
  }
};

static unsigned g_rng = 2463534242u;
static int rnd(int lo, int hi) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return lo + (int)(g_rng % (unsigned)(hi - lo + 1)); }

// one push (flushing = false: n real frames first .. first + n - 1) or one flush round (n None calls) against the machine
static void step(Machine& mc, State& st, int n, bool flushing, int max_push, int* total) {
  const Plan p = make_plan(st, n, flushing);
  std::vector<int> got[LAG + 1];
  std::vector<Emit> em[LAG + 1];
  for (int i = 0; i < n; ++i) {
    int g[LAG + 1]; Emit e[LAG + 1];
    mc.feed(flushing ? NONE : st.pushed + i, g, e);
    for (int j = 0; j <= LAG; ++j) if (g[j] != NONE) { got[j].push_back(g[j]); em[j].push_back(e[j]); }
  }
  // every layer emits every frame exactly once and in order: the window IS what the machine gained
  for (int j = 0; j <= LAG; ++j) {
    CHECK(p.win[j].lo >= 0 && p.win[j].count() >= 0 && p.win[j].count() <= n, "lag %d: window [%d, %d) of a push of %d", j, p.win[j].lo, p.win[j].hi, n);
    CHECK((int)got[j].size() == p.win[j].count(), "lag %d: machine gained %d frames, plan %d (pushed %d clock %d n %d flush %d)", j, (int)got[j].size(),
          p.win[j].count(), st.pushed, st.clock, n, (int)flushing);
    for (size_t i = 0; i < got[j].size() && (int)i < p.win[j].count(); ++i) CHECK(got[j][i] == p.win[j].lo + (int)i, "lag %d: frame %d where the plan has %d", j, got[j][i], p.win[j].lo + (int)i);
  }
  CHECK(p.emitted == p.win[LAG].count(), "emitted");
  // every neighbour is what the machine used and is held where the plan says
  for (int j = 1; j <= LAG; ++j) {
    const int b = (j - 1) / BLOCK_LAG, k = j - b * BLOCK_LAG, src = BIBUF_INPUT[k - 1], cap = CARRIED[src].hist + max_push;
    for (size_t i = 0; i < em[j].size(); ++i) {
      const Emit e = em[j][i];
      CHECK(e.left == (p.prev_is_zero(e.t) ? ZEROS : e.t - 1), "BiBufferConv %d frame %d: left %d", j, e.t, e.left);
      CHECK(e.right == (p.next_is_zero(j, e.t) ? ZEROS : e.t + 1), "BiBufferConv %d frame %d: right %d (input window ends at %d)", j, e.t, e.right, p.win[j - 1].hi);
      CHECK(!p.next_is_zero(j, e.t) || (flushing && e.t + 1 >= st.pushed), "BiBufferConv %d frame %d: zeros for t + 1 inside the stream", j, e.t);
      const int lo = e.left == ZEROS ? e.t : e.t - 1, hi = e.right == ZEROS ? e.t : e.t + 1;
      CHECK(p.slot_of(b, src, lo) >= 0 && p.slot_of(b, src, hi) < cap, "BiBufferConv %d frame %d: slots %d..%d outside 0..%d", j, e.t, p.slot_of(b, src, lo), p.slot_of(b, src, hi), cap - 1);
      CHECK(hi < p.win[j - 1].hi, "BiBufferConv %d frame %d reads frame %d its input does not hold yet", j, e.t, hi);
    }
  }
  // every skip partner is held when it is read
  for (int b = 0; b < 2; ++b) {
    const int L = b * BLOCK_LAG;
    const int partner[3][2] = {{C_X1, 6}, {C_X0, 8}, {C_IN, 8}};
    for (auto& pr : partner) {
      const Window rd = p.win[L + pr[1]], have = p.win[L + CARRIED[pr[0]].lag];
      if (rd.count() == 0) continue;
      CHECK(p.slot_of(b, pr[0], rd.lo) >= 0 && p.slot_of(b, pr[0], rd.hi - 1) < CARRIED[pr[0]].hist + max_push, "block %d skip tensor %d: slots outside the buffer", b, pr[0]);
      CHECK(rd.hi <= have.hi && rd.lo >= have.lo - CARRIED[pr[0]].hist, "block %d skip tensor %d: frames [%d, %d) against held [%d, %d)", b, pr[0], rd.lo, rd.hi, have.lo - CARRIED[pr[0]].hist, have.hi);
    }
  }
  // no carry exceeds its capacity: by the plan's own figure, and by what the machine still holds (its buffers and queues)
  for (int b = 0; b < 2; ++b) {
    const int L = b * BLOCK_LAG;
    for (int c = 0; c < C_COUNT; ++c) {
      CHECK(p.carry_extent(b, c) >= 0 && p.carry_extent(b, c) <= CARRIED[c].hist, "block %d tensor %d: carry of %d frames, capacity %d", b, c, p.carry_extent(b, c), CARRIED[c].hist);
      CHECK(p.write_slot(c) + p.write_count(b, c) <= CARRIED[c].hist + max_push, "block %d tensor %d: the window overruns the buffer", b, c);
    }
    for (int k = 1; k <= BLOCK_LAG; ++k) {
      const BiBuffer& m = mc.blk[b].mem[k - 1];
      const int src = BIBUF_INPUT[k - 1], oldest_kept = p.win[L + k - 1].hi - CARRIED[src].hist;
      if (m.center >= 0) CHECK(m.center >= oldest_kept && (m.left < 0 || m.left >= oldest_kept), "block %d BiBufferConv %d holds frames %d / %d, the carry starts at %d", b, k, m.left, m.center, oldest_kept);
    }
    const std::deque<int>* q[3] = {&mc.blk[b].skip3, &mc.blk[b].skip2, &mc.blk[b].skip1};
    const int qc[3] = {C_X1, C_X0, C_IN};
    for (int i = 0; i < 3; ++i) {
      CHECK((int)q[i]->size() <= CARRIED[qc[i]].hist, "block %d: skip queue of tensor %d holds %d frames", b, qc[i], (int)q[i]->size());
      CHECK((int)q[i]->size() == p.carry_extent(b, qc[i]), "block %d: skip queue of tensor %d holds %d frames, the plan carries %d", b, qc[i], (int)q[i]->size(), p.carry_extent(b, qc[i]));
      for (int f : *q[i]) CHECK(f >= p.win[L + CARRIED[qc[i]].lag].hi - CARRIED[qc[i]].hist, "block %d: queued frame %d is older than the carry", b, f);
    }
  }
  st = p.after;
  *total += p.emitted;
  if (!flushing) CHECK(*total == (st.pushed > LAG ? st.pushed - LAG : 0), "emitted %d after %d pushed", *total, st.pushed);
  CHECK(*total == emitted_total(st) && pending(st) == st.pushed - *total, "the host-side counts: emitted %d, pending %d after %d", emitted_total(st), pending(st), *total);
}

static void stream(int max_push, int frames) {
  Machine mc; State st; int emitted = 0;
  while (st.pushed < frames) step(mc, st, std::min(rnd(1, max_push), frames - st.pushed), false, max_push, &emitted);
  // a flush emits the rest
  int calls = flush_calls(st);
  CHECK(calls == (frames > 0 ? LAG : 0), "flush of a %d-frame stream takes %d calls", frames, calls);
  while (calls > 0) { const int k = std::min(calls, max_push); step(mc, st, k, true, max_push, &emitted); calls -= k; }
  CHECK(emitted == frames && pending(st) == 0, "a %d-frame stream emitted %d frames", frames, emitted);
}

int main() {
  int streams = 0;
  for (int max_push = 1; max_push <= 8; ++max_push)
    for (int frames = 0; frames <= 40; ++frames)
      for (int rep = 0; rep < 4; ++rep) {
        // a flush at the end, or in the middle followed by a second stream (a fresh State: flush ends with reset)
        stream(max_push, frames);
        if (rep & 1) stream(max_push, rnd(0, 40));
        ++streams;
      }
  std::printf("%d streams, %d failures\n", streams, g_fail);
  return g_fail ? 1 : 0;
}
