// tests/test_temporal_motion_plan_cpu.py: where a round's frames find their stream's previous LR frame, and which of them get the constant noise
// plane (csrc/temporal_motion_plan.h), replayed against a naive per-stream simulation.  Random rounds with max_push 1, 4 and 64 (and a few
// others), streams that end by a flush or a reset and slots that are re-used.  For every frame of every accepted round:
//   - the previous ring slot is the slot its predecessor entered (the naive stream remembers where each of its frames went);
//   - it is never a slot this round's frames-in launch writes for another frame than that predecessor, and never the frame's own;
//   - whatever a ring slot held before - the predecessor - has not been overwritten since by a later frame of the stream;
//   - constant frames are exactly the stream starts.
// The taps and the scale are held to their formulas.
#include "../sharkshark-4k_amd/csrc/bsvd_online_plan.h"
#include "../sharkshark-4k_amd/csrc/temporal_round_plan.h"
#include "../sharkshark-4k_amd/csrc/temporal_motion_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

using namespace ss4k;
namespace tr = ss4k::temporal_round;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++failures;                                         \
      if (failures <= 20) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                     \
  } while (0)

// the naive machine of one stream: a ring of R slots that remembers which stream frame each slot holds, and where every frame went
struct NaiveStream {
  long long pushed = 0;
  std::vector<long long> ring;        // ring[slot] = number of the stream frame it holds, -1: none
  long long last_slot = -1;           // the slot the stream's newest frame entered
  explicit NaiveStream(int R = 0) : ring((size_t)R, -1) {}
};

int main() {
  std::mt19937 rng(20261021);
  long long rounds = 0, frames = 0, constants = 0, refused = 0;
  const int pushes[] = {1, 4, 64, 2, 7, 33};
  for (int trial = 0; trial < 360; ++trial) {
    const int max_push = pushes[trial % 6];
    const int max_streams = 1 + (int)(rng() % (max_push == 64 ? 3 : 8));
    const int R = tr::ring_frames(max_push);
    std::vector<bsvd_online::State> st((size_t)max_streams);
    std::vector<NaiveStream> naive((size_t)max_streams, NaiveStream(R));
    for (int round = 0; round < 50; ++round) {
      for (int s = 0; s < max_streams; ++s)   // a stream ends now and then (flush and reset look alike from here: the next frame is a first one)
        if (rng() % 19 == 0) { st[(size_t)s] = bsvd_online::State{}; naive[(size_t)s] = NaiveStream(R); }
      std::vector<int> slots;
      for (int s = 0; s < max_streams; ++s) {
        if (rng() % 3 == 0) continue;
        int n = (int)(rng() % (unsigned)(max_push + 1));
        if (max_push == 64 && rng() % 2) n = 64 / max_streams;   // full pushes too
        for (int i = 0; i < n; ++i) slots.push_back(s);
      }
      if (rng() % 17 == 0 && max_push < 64) for (int i = 0; i <= max_push; ++i) slots.push_back(0);   // one frame too many for slot 0: refused
      std::shuffle(slots.begin(), slots.end(), rng);
      if (slots.empty() || slots.size() > (size_t)tr::MAX_FRAMES) continue;
      const tr::Plan p = tr::make_round(slots.data(), (int)slots.size(), st.data(), max_push, max_streams, 1 << 20);
      if (p.refusal) { ++refused; continue; }
      const tr::Motion m = tr::make_motion(p, max_push);
      ++rounds;
      // what the round's frames-in launch writes: (slot of the stream, ring slot) of every frame
      for (int t = 0; t < p.n_items; ++t) {
        const tr::Item& it = p.items[t];
        NaiveStream& ns = naive[(size_t)it.slot];
        CHECK(it.before.pushed == (int)ns.pushed, "item %d: the plan starts at frame %d, the stream is at %lld", t, it.before.pushed, ns.pushed);
        for (int j = 0; j < it.n; ++j) {
          const int q = it.first + j;
          ++frames;
          const bool constant = ((m.constant_bits >> q) & 1ull) != 0;
          CHECK(constant == (ns.pushed == 0), "frame %d of item %d: constant %d for stream frame %lld", j, t, (int)constant, ns.pushed);
          CHECK(constant == (m.ring_prev[q] < 0), "frame %d of item %d: constant %d with previous slot %d", j, t, (int)constant, m.ring_prev[q]);
          if (constant) ++constants;
          if (!constant) {
            const int prev = m.ring_prev[q];
            CHECK(prev >= 0 && prev < R, "previous slot %d outside the ring of %d", prev, R);
            CHECK((long long)prev == ns.last_slot, "frame %d of item %d: previous slot %d, the predecessor entered %lld", j, t, prev, ns.last_slot);
            CHECK(prev >= 0 && prev < R && ns.ring[(size_t)prev] == ns.pushed - 1, "previous slot %d holds frame %lld, not %lld", prev,
                  prev >= 0 && prev < R ? ns.ring[(size_t)prev] : -2, ns.pushed - 1);
            CHECK(prev != p.ring_in[q], "frame %d of item %d reads the slot it is written to", j, t);
            // no frame of this round - of this item: rings are per stream - other than the predecessor itself is written there
            for (int j2 = 0; j2 < it.n; ++j2)
              CHECK(p.ring_in[it.first + j2] != prev || j2 == j - 1, "frame %d of item %d: its previous slot %d is written by frame %d of the round", j, t,
                    prev, j2);
            if (j == 0)
              for (int j2 = 0; j2 < it.n; ++j2)
                CHECK(p.ring_in[it.first + j2] != prev, "the predecessor of an item's first frame lies in slot %d, which the round writes", prev);
          }
          // the frame goes in
          CHECK(p.ring_in[q] == (int)(ns.pushed % R), "frame %d of item %d enters slot %d, not %lld", j, t, p.ring_in[q], ns.pushed % R);
          ns.ring[(size_t)p.ring_in[q]] = ns.pushed;
          ns.last_slot = p.ring_in[q];
          ++ns.pushed;
        }
        st[(size_t)it.slot] = it.after;
      }
      // bits beyond the round's frames stay clear
      if (p.k < 64) CHECK((m.constant_bits >> p.k) == 0, "constant bits beyond the round's %d frames", p.k);
    }
  }
  // the numbers of the rule
  float w[9];
  tr::motion_taps(w);
  double g[3], sum = 0;
  for (int i = 0; i < 3; ++i) { g[i] = std::exp(-(double)((i - 1) * (i - 1)) / (2.0 * 0.5 * 0.5)); sum += g[i]; }
  double total = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      CHECK(w[3 * i + j] == (float)((g[i] / sum) * (g[j] / sum)), "tap [%d][%d] = %.9g", i, j, (double)w[3 * i + j]);
      CHECK(w[3 * i + j] == w[3 * j + i] && w[3 * i + j] == w[3 * (2 - i) + (2 - j)], "tap [%d][%d] breaks the symmetry", i, j);
      total += (double)w[3 * i + j];
    }
  CHECK(std::fabs(total - 1.0) < 1e-6, "the taps sum to %.9g", total);
  CHECK(tr::motion_scale(1.0) == (float)0.35 && tr::motion_scale(0.25) == (float)(0.35 * 0.25) && tr::motion_scale(0.0) == 0.f, "the scale is (float)(0.35 rate)");
  std::printf("%lld rounds, %lld frames (%lld constant), %lld refused, %d failures\n", rounds, frames, constants, refused, failures);
  return failures ? 1 : 0;
}
