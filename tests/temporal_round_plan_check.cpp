// tests/test_temporal_round_plan_cpu.py: the plan of a round (csrc/temporal_round_plan.h) replayed against a naive per-stream simulation.
// Random rounds over max_streams 1..8 and max_push 1..6: streams join, end (their slot starts a new stream) and slots are re-used; every so
// often a round that must be refused is thrown in, and a refusal must leave every state as it was.
#include "../sharkshark-4k_amd/csrc/bsvd_online_plan.h"
#include "../sharkshark-4k_amd/csrc/temporal_round_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
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

// the naive machine of one stream: frames go in one at a time, frame i leaves when frame i + 16 has gone in
struct NaiveStream {
  long long pushed = 0, emitted = 0;
  int push_one() { ++pushed; if (pushed - 16 > emitted) { ++emitted; return 1; } return 0; }
};

static bool same(const bsvd_online::State& a, const bsvd_online::State& b) { return a.pushed == b.pushed && a.clock == b.clock; }

int main() {
  std::mt19937 rng(20240917);
  long long rounds = 0, refused = 0;
  for (int trial = 0; trial < 400; ++trial) {
    const int max_streams = 1 + (int)(rng() % 8), max_push = 1 + (int)(rng() % 6);
    const int R = tr::ring_frames(max_push);
    std::vector<bsvd_online::State> st(max_streams);
    std::vector<NaiveStream> naive(max_streams);
    // what each ring slot of each stream holds: the stream frame index, -1 = free
    std::vector<std::vector<long long>> ring(max_streams, std::vector<long long>(R, -1));
    for (int round = 0; round < 60; ++round) {
      // a stream ends now and then: its slot starts over (what TemporalUpscaler::flush / reset leave behind)
      for (int s = 0; s < max_streams; ++s)
        if (rng() % 23 == 0) { st[s] = bsvd_online::State{}; naive[s] = NaiveStream{}; std::fill(ring[s].begin(), ring[s].end(), -1); }
      // the round: 0..max_push frames of each slot that takes part, interleaved at random
      std::vector<int> slots;
      for (int s = 0; s < max_streams; ++s) {
        if (rng() % 3 == 0) continue;
        const int n = (int)(rng() % (max_push + 1));
        for (int i = 0; i < n; ++i) slots.push_back(s);
      }
      std::shuffle(slots.begin(), slots.end(), rng);
      if ((int)slots.size() > tr::MAX_FRAMES) slots.resize(tr::MAX_FRAMES);
      const std::vector<bsvd_online::State> before = st;
      // ---- refusals: each leaves every state as it was
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
          for (int s = 0; s < max_streams; ++s) CHECK(same(st[s], before[s]), "a refusal (%s) changed slot %d", why, s);
          ++refused;
        }
      }
      if (slots.empty()) continue;
      const int k = (int)slots.size();
      const tr::Plan p = tr::make_round(slots.data(), k, st.data(), max_push, max_streams, 1 << 20);
      CHECK(p.refusal == nullptr, "a legal round was refused: %s", p.refusal ? p.refusal : "");
      if (p.refusal) continue;
      ++rounds;
      for (int s = 0; s < max_streams; ++s) CHECK(same(st[s], before[s]), "planning changed slot %d", s);
      CHECK(p.k == k, "k");
      // ---- items in order of first appearance, frames in the caller's order
      std::vector<int> first_seen;
      for (int s : slots) if (std::find(first_seen.begin(), first_seen.end(), s) == first_seen.end()) first_seen.push_back(s);
      CHECK(p.n_items == (int)first_seen.size(), "n_items %d against %d", p.n_items, (int)first_seen.size());
      std::vector<int> seen_frame(k, 0);
      int e = 0, first = 0;
      for (int t = 0; t < p.n_items && t < (int)first_seen.size(); ++t) {
        const tr::Item& it = p.items[t];
        CHECK(it.slot == first_seen[t], "item %d is slot %d, first appearance says %d", t, it.slot, first_seen[t]);
        CHECK(it.first == first && it.n >= 1 && it.n <= max_push, "item %d: first %d n %d", t, it.first, it.n);
        CHECK(it.n == (int)std::count(slots.begin(), slots.end(), it.slot), "item %d: frame count", t);
        for (int j = 0; j < it.n; ++j) {
          const int f = p.order[it.first + j];
          CHECK(f >= 0 && f < k && slots[f] == it.slot, "item %d frame %d names frame %d", t, j, f);
          if (f >= 0 && f < k) ++seen_frame[f];
          if (j > 0) CHECK(p.order[it.first + j - 1] < f, "item %d: frames out of the caller's order", t);
        }
        // ---- the naive stream: counts follow max(0, pushed - 16); ring slots never collide
        NaiveStream& ns = naive[it.slot];
        std::vector<long long>& rg = ring[it.slot];
        const long long emitted0 = ns.emitted;
        int got = 0;
        for (int j = 0; j < it.n; ++j) {
          const int slot_in = p.ring_in[it.first + j];
          CHECK(slot_in >= 0 && slot_in < R, "ring slot %d outside the ring", slot_in);
          CHECK(slot_in == (int)(ns.pushed % R), "frame %lld enters slot %d", ns.pushed, slot_in);
          // every frame of the round enters before any leaves (frames in, then the ring gather): the slot must be free NOW
          CHECK(rg[slot_in] == -1, "slot %d of stream slot %d still holds frame %lld when frame %lld enters", slot_in, it.slot, rg[slot_in], ns.pushed);
          rg[slot_in] = ns.pushed;
          got += ns.push_one();
        }
        CHECK(it.emitted == got, "item %d emits %d, the naive stream %d", t, it.emitted, got);
        CHECK(ns.emitted == std::max(0LL, ns.pushed - 16), "naive stream");
        CHECK(it.den_off == e, "item %d: den_off %d, expected %d (disjoint and covering)", t, it.den_off, e);
        for (int q = 0; q < it.emitted; ++q) {
          const int slot_out = p.ring_out[it.den_off + q];
          CHECK(slot_out >= 0 && slot_out < R && rg[slot_out] == emitted0 + q, "output %d of item %d leaves slot %d, which holds %lld, not %lld", q, t,
                slot_out, slot_out >= 0 && slot_out < R ? rg[slot_out] : -2, emitted0 + q);
          if (slot_out >= 0 && slot_out < R) rg[slot_out] = -1;
        }
        CHECK(same(it.before, before[it.slot]), "item %d: before", t);
        CHECK(it.after.pushed == ns.pushed && bsvd_online::emitted_total(it.after) == ns.emitted && bsvd_online::pending(it.after) == ns.pushed - ns.emitted,
              "item %d: after", t);
        st[it.slot] = it.after;
        e += it.emitted; first += it.n;
      }
      for (int f = 0; f < k; ++f) CHECK(seen_frame[f] == 1, "frame %d is in %d items", f, seen_frame[f]);
      CHECK(p.total == e, "E %d against %d", p.total, e);
      // ---- the tail: chunks of at most max_push, in order, covering [0, E)
      int at = 0;
      for (int c = 0; c < p.n_chunks; ++c) {
        CHECK(p.chunk_off[c] == at && p.chunk_n[c] >= 1 && p.chunk_n[c] <= max_push, "chunk %d: off %d n %d", c, p.chunk_off[c], p.chunk_n[c]);
        at += p.chunk_n[c];
      }
      CHECK(at == e, "the chunks cover %d of %d frames", at, e);
      CHECK(p.n_chunks == (e + max_push - 1) / max_push, "chunk count");
    }
  }
  std::printf("%lld rounds, %lld refusals checked, %d failures\n", rounds, refused, failures);
  return failures ? 1 : 0;
}
