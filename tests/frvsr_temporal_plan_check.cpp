// tests/test_frvsr_temporal_plan_cpu.py: the wave plan of the frame-recurrent chain with the online denoiser in front
// (csrc/frvsr_temporal_plan.h) replayed against a naive per-stream simulation.  Random rounds over max_streams 1..8 and max_push 1..6, streams
// that end by a flush (its waves are checked too) or a reset and slots that are re-used; refused rounds in between have no waves.
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

// the naive machine of one stream: frame i leaves the denoiser when frame i + 16 has gone in, and the generator takes the frames that left one
// at a time, in order
struct NaiveStream {
  long long pushed = 0, emitted = 0, stepped = 0;   // stepped: frames that went through the recurrent step
  int push_one() { ++pushed; if (pushed - 16 > emitted) { ++emitted; return 1; } return 0; }
};

int main() {
  std::mt19937 rng(20241021);
  long long rounds = 0, refused = 0, flushes = 0, waves_seen = 0;
  for (int trial = 0; trial < 400; ++trial) {
    const int max_streams = 1 + (int)(rng() % 8), max_push = 1 + (int)(rng() % 6);
    std::vector<bsvd_online::State> st(max_streams);
    std::vector<NaiveStream> naive(max_streams);
    for (int round = 0; round < 60; ++round) {
      // ---- a stream ends now and then: by a flush (n waves of one, in order) or by a reset
      for (int s = 0; s < max_streams; ++s) {
        if (rng() % 23 != 0) continue;
        if (rng() % 2) {
          const int left = bsvd_online::pending(st[s]);
          const ft::Waves f = ft::make_flush(s, left);
          ++flushes;
          CHECK(f.n_waves == left && left == (int)(naive[s].pushed - naive[s].emitted), "flush of slot %d: %d waves for %d pending frames", s, f.n_waves, left);
          for (int r = 0; r < f.n_waves; ++r)
            CHECK(f.w[r].n == 1 && f.w[r].slot[0] == s && f.w[r].out[0] == r, "flush wave %d of slot %d: n %d slot %d out %d", r, s, f.w[r].n, f.w[r].slot[0], f.w[r].out[0]);
        }
        st[s] = bsvd_online::State{}; naive[s] = NaiveStream{};
      }
      std::vector<int> slots;
      for (int s = 0; s < max_streams; ++s) {
        if (rng() % 3 == 0) continue;
        const int n = (int)(rng() % (max_push + 1));
        for (int i = 0; i < n; ++i) slots.push_back(s);
      }
      std::shuffle(slots.begin(), slots.end(), rng);
      if ((int)slots.size() > tr::MAX_FRAMES) slots.resize(tr::MAX_FRAMES);
      // ---- refusals are make_round's, and a refused round has no waves
      {
        std::vector<int> bad = slots;
        const char* why = nullptr;
        long long cap = 1 << 20;
        const int kind = (int)(rng() % 6);
        if (kind == 0) { bad.clear(); why = "empty"; }
        else if (kind == 1) { bad.assign(tr::MAX_FRAMES + 1, 0); why = "65 frames"; }
        else if (kind == 2) { bad.push_back(rng() % 2 ? max_streams : -1); why = "slot outside"; }
        else if (kind == 3) { bad.insert(bad.end(), max_push + 1, 0); why = "more than max_push"; if ((int)bad.size() > tr::MAX_FRAMES) why = nullptr; }
        else if (kind == 4 && !slots.empty()) {
          const tr::Plan q = tr::make_round(slots.data(), (int)slots.size(), st.data(), max_push, max_streams, 1 << 20);
          if (!q.refusal && q.total > 0) { cap = q.total - 1; why = "capacity"; }
        }
        if (why) {
          const tr::Plan q = tr::make_round(bad.data(), (int)bad.size(), st.data(), max_push, max_streams, cap);
          CHECK(q.refusal != nullptr, "%s was not refused", why);
          const ft::Waves v = ft::make_waves(q);
          CHECK(v.n_waves == 0, "a refused round (%s) has %d waves", why, v.n_waves);
          ++refused;
        }
      }
      if (slots.empty()) continue;
      const int k = (int)slots.size();
      const tr::Plan p = tr::make_round(slots.data(), k, st.data(), max_push, max_streams, 1 << 20);
      CHECK(p.refusal == nullptr, "a legal round was refused: %s", p.refusal ? p.refusal : "");
      if (p.refusal) continue;
      ++rounds;
      const ft::Waves v = ft::make_waves(p);
      // ---- the naive streams: what each item emits
      std::vector<int> emitted(p.n_items, 0);
      int most = 0;
      for (int t = 0; t < p.n_items; ++t) {
        for (int j = 0; j < p.items[t].n; ++j) emitted[t] += naive[p.items[t].slot].push_one();
        CHECK(emitted[t] == p.items[t].emitted, "item %d: the naive stream emits %d, the plan %d", t, emitted[t], p.items[t].emitted);
        most = std::max(most, emitted[t]);
        st[p.items[t].slot] = p.items[t].after;
      }
      CHECK(v.n_waves == most, "%d waves, max(emitted) is %d", v.n_waves, most);
      CHECK(v.n_waves <= max_push, "%d waves with max_push %d", v.n_waves, max_push);
      // ---- every ready frame in exactly one wave, an item's frames in wave order, slots distinct within a wave
      std::vector<int> times(std::max(p.total, 1), 0);
      std::vector<int> next_of_item(p.n_items, 0);
      for (int r = 0; r < v.n_waves; ++r) {
        const ft::Wave& w = v.w[r];
        ++waves_seen;
        CHECK(w.n >= 1 && w.n <= max_streams, "wave %d holds %d entries", r, w.n);
        std::vector<int> seen(max_streams, 0);
        int last_item = -1;
        for (int i = 0; i < w.n; ++i) {
          const int t = w.item[i];
          CHECK(t >= 0 && t < p.n_items, "wave %d entry %d names item %d", r, i, t);
          if (t < 0 || t >= p.n_items) continue;
          CHECK(t > last_item, "wave %d: items out of order", r);
          last_item = t;
          CHECK(w.slot[i] == p.items[t].slot, "wave %d entry %d: slot %d, its item's is %d", r, i, w.slot[i], p.items[t].slot);
          CHECK(w.slot[i] >= 0 && w.slot[i] < max_streams && !seen[w.slot[i]], "wave %d names slot %d twice (or outside)", r, w.slot[i]);
          if (w.slot[i] >= 0 && w.slot[i] < max_streams) seen[w.slot[i]] = 1;
          CHECK(w.out[i] == p.items[t].den_off + r, "wave %d entry %d: output %d, expected den_off %d + %d", r, i, w.out[i], p.items[t].den_off, r);
          CHECK(w.out[i] >= 0 && w.out[i] < p.total, "wave %d entry %d: output %d outside 0..%d", r, i, w.out[i], p.total);
          if (w.out[i] >= 0 && w.out[i] < p.total) ++times[w.out[i]];
          // the stream's frames pass the generator in order: this is the next one of its item, and of its stream
          CHECK(next_of_item[t] == r, "item %d: wave %d carries its frame %d", t, r, next_of_item[t]);
          ++next_of_item[t];
          NaiveStream& ns = naive[p.items[t].slot];
          CHECK(ns.stepped == ns.emitted - emitted[t] + r, "slot %d: frame %lld steps when %lld was due", p.items[t].slot, ns.emitted - emitted[t] + r, ns.stepped);
          ++ns.stepped;
        }
        // an item that emitted more than r frames is in wave r
        for (int t = 0; t < p.n_items; ++t)
          if (emitted[t] > r) CHECK(std::count(w.item, w.item + w.n, t) == 1, "item %d (emitted %d) is missing from wave %d", t, emitted[t], r);
      }
      for (int e = 0; e < p.total; ++e) CHECK(times[e] == 1, "ready frame %d is in %d waves", e, times[e]);
      for (int t = 0; t < p.n_items; ++t) CHECK(next_of_item[t] == emitted[t], "item %d: %d of %d frames in waves", t, next_of_item[t], emitted[t]);
    }
  }
  // a flush outside what a slot can hold has no waves
  CHECK(ft::make_flush(0, -1).n_waves == 0 && ft::make_flush(0, ft::MAX_WAVES + 1).n_waves == 0, "flush counts outside 0..64");
  std::printf("%lld rounds, %lld waves, %lld flushes, %lld refusals checked, %d failures\n", rounds, waves_seen, flushes, refused, failures);
  return failures ? 1 : 0;
}
