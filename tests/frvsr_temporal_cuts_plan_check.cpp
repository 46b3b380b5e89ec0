// tests/test_frvsr_temporal_cuts_plan_cpu.py: the flag-ring word that every wave of the frame-recurrent chain with the online denoiser in front
// reads for its leaving frame (csrc/frvsr_temporal_plan.h: Wave::frame, ring_word) replayed against a naive per-stream simulation.  20 000 random
// rounds and flushes over max_streams 1..64 and max_push 1..64.  The naive ring of a slot is what BsvdOnline keeps: 128 words, a push writes the
// words of the frames it brings (frame f at f & 127) and remembers WHICH frame wrote each word; a flush writes none; a stream's end leaves the
// words as they are.  For every leaving frame the word the wave names must be the one written for exactly that frame, by its own stream, and not
// yet overwritten - in rounds, and in the flush waves that run after the denoiser's own flush.
#include "../sharkshark-4k_amd/csrc/bsvd_online_plan.h"
#include "../sharkshark-4k_amd/csrc/temporal_round_plan.h"
#include "../sharkshark-4k_amd/csrc/frvsr_temporal_plan.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

using namespace ss4k;
namespace tr = ss4k::temporal_round;
namespace ft = ss4k::frvsr_temporal;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++failures;                                         \
      if (failures <= 20) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                     \
  } while (0)

// the naive machine of one slot: the stream's counters and the ring as the denoiser keeps it.  owner[w]: the stream frame whose flag word w
// holds, -1 for a word no frame of THIS stream has written; stream_id tells a word of the stream before from one of the running stream
struct NaiveSlot {
  long long pushed = 0, left = 0;        // frames of the running stream that went in / that came back
  long long stream_id = 0;
  long long owner[ft::CUT_RING];
  long long owner_stream[ft::CUT_RING];
  bool flagged[ft::CUT_RING];            // the word itself: random flags, so a stale word would also read wrong
  std::vector<bool> flag_of_frame;       // what the detector said of every frame of the running stream
  NaiveSlot() { for (int w = 0; w < ft::CUT_RING; ++w) { owner[w] = -1; owner_stream[w] = -1; flagged[w] = false; } }
  void push_one(bool flag) {
    const int w = (int)(pushed & (ft::CUT_RING - 1));
    owner[w] = pushed; owner_stream[w] = stream_id; flagged[w] = flag;
    flag_of_frame.push_back(flag);
    ++pushed;
  }
  int ready() const { return (int)std::max(0LL, pushed - 16 - left); }   // frame i leaves once frame i + 16 is in
  void end() { pushed = left = 0; ++stream_id; flag_of_frame.clear(); }   // (the ring's words stay: nobody zero-fills them here)
};

static void leave(NaiveSlot& ns, int slot, int frame, const char* where) {
  CHECK((long long)frame == ns.left, "%s, slot %d: the wave names frame %d, the stream's next leaving frame is %lld", where, slot, frame, ns.left);
  const int w = ft::ring_word(frame);
  CHECK(w >= 0 && w < ft::CUT_RING && w == (frame & 127), "%s, slot %d: frame %d reads word %d", where, slot, frame, w);
  if (w < 0 || w >= ft::CUT_RING) return;
  CHECK(ns.owner[w] == (long long)frame && ns.owner_stream[w] == ns.stream_id,
        "%s, slot %d: frame %d reads word %d, which holds frame %lld of stream %lld (running: %lld)", where, slot, frame, w, ns.owner[w],
        ns.owner_stream[w], ns.stream_id);
  if (frame >= 0 && frame < (int)ns.flag_of_frame.size())
    CHECK(ns.flagged[w] == ns.flag_of_frame[frame], "%s, slot %d: frame %d reads another frame's flag", where, slot, frame);
  ++ns.left;
}

int main() {
  std::mt19937 rng(20261021);
  long long rounds = 0, flushes = 0, waves_seen = 0, leaving = 0, wrapped = 0;
  while (rounds + flushes < 20000) {
    const int max_streams = 1 + (int)(rng() % 64), max_push = 1 + (int)(rng() % 64);
    std::vector<bsvd_online::State> st(max_streams);
    std::vector<NaiveSlot> naive(max_streams);
    const int events = 40 + (int)(rng() % 400);   // long enough that streams pass frame 128 and the ring wraps, several times
    for (int ev = 0; ev < events; ++ev) {
      // ---- a stream ends now and then: by a flush (its waves read the ring after the denoiser's flush) or by a reset
      for (int s = 0; s < max_streams; ++s) {
        if (rng() % 97 != 0) continue;
        if (rng() % 4) {
          const int left = bsvd_online::pending(st[s]);
          const ft::Waves f = ft::make_flush(s, left, bsvd_online::emitted_total(st[s]));
          ++flushes;
          CHECK(f.n_waves == left && left == (int)(naive[s].pushed - naive[s].left), "flush of slot %d: %d waves, %d pending", s, f.n_waves, left);
          for (int r = 0; r < f.n_waves; ++r) {
            CHECK(f.w[r].n == 1 && f.w[r].slot[0] == s && f.w[r].out[0] == r, "flush wave %d of slot %d", r, s);
            leave(naive[s], s, f.w[r].frame[0], "flush");
            ++waves_seen; ++leaving;
          }
        }
        st[s] = bsvd_online::State{}; naive[s].end();
      }
      std::vector<int> slots;
      for (int s = 0; s < max_streams; ++s) {
        if (rng() % 3 == 0) continue;
        const int n = (int)(rng() % (max_push + 1));
        for (int i = 0; i < n; ++i) slots.push_back(s);
      }
      std::shuffle(slots.begin(), slots.end(), rng);
      if ((int)slots.size() > tr::MAX_FRAMES) slots.resize(tr::MAX_FRAMES);
      if (slots.empty()) continue;
      const tr::Plan p = tr::make_round(slots.data(), (int)slots.size(), st.data(), max_push, max_streams, 1 << 20);
      CHECK(p.refusal == nullptr, "a legal round was refused: %s", p.refusal ? p.refusal : "");
      if (p.refusal) continue;
      ++rounds;
      // every push of the round comes before its first wave (FrvsrTemporal::round: step 3, then step 4)
      for (int t = 0; t < p.n_items; ++t) {
        NaiveSlot& ns = naive[p.items[t].slot];
        for (int j = 0; j < p.items[t].n; ++j) ns.push_one(rng() % 5 == 0);
        CHECK(ns.ready() == p.items[t].emitted, "item %d: the naive stream has %d frames ready, the plan %d", t, ns.ready(), p.items[t].emitted);
        st[p.items[t].slot] = p.items[t].after;
        if (ns.pushed > ft::CUT_RING) ++wrapped;
      }
      const ft::Waves v = ft::make_waves(p);
      for (int r = 0; r < v.n_waves; ++r) {
        const ft::Wave& w = v.w[r];
        ++waves_seen;
        for (int i = 0; i < w.n; ++i) {
          CHECK(w.slot[i] >= 0 && w.slot[i] < max_streams, "wave %d entry %d: slot %d", r, i, w.slot[i]);
          if (w.slot[i] < 0 || w.slot[i] >= max_streams) continue;
          leave(naive[w.slot[i]], w.slot[i], w.frame[i], "round");
          ++leaving;
        }
      }
      for (int t = 0; t < p.n_items; ++t) CHECK(naive[p.items[t].slot].ready() == 0, "item %d: frames were ready and left in no wave", t);
    }
  }
  // the default of make_flush: a stream that has returned nothing yet
  const ft::Waves f0 = ft::make_flush(3, 5);
  CHECK(f0.n_waves == 5 && f0.w[4].frame[0] == 4, "make_flush without a frame number starts at frame 0");
  CHECK(wrapped > 0, "no stream ever passed frame 128: the ring never wrapped");
  std::printf("%lld rounds, %lld flushes, %lld waves, %lld leaving frames, %lld pushes past the ring's size checked, %d failures\n", rounds, flushes,
              waves_seen, leaving, wrapped, failures);
  return failures ? 1 : 0;
}
