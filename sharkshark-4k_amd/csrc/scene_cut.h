// Scene-cut detection for the frame-recurrent upscaler's rounds (include/ss4k.h: ss4k_frvsr_upscaler_set_scene_cut): the launchers of
// scene_cut.hip and the host object that api.cpp runs in front of a round (api_scene_cut.cpp).  The rule, in exact integer arithmetic
// (restated in numpy by tests/scene_cut_ref.py): a frame is compared with the stream's previous input frame, byte for byte as
// both arrived - S = sum |F - prev|, score = min(S, |S - S_prev|), a cut iff score >= T - and a cut zeroes the stream's lr_prev / hr_prev, the
// state a stream's first frame sees.  Three launches per round whatever its size, in stream order; no kernel waits for another workgroup.
#pragma once
#include "common.h"

namespace ss4k {

struct FrvsrUpscaler;

namespace cut {

constexpr int MAX_ITEMS = SS4K_FRVSR_MAX_STREAMS;
// a thread's 32-bit partial sum holds its share of a frame up to here: at least 32 workgroups of 256 threads per item, so at most 2^36 / 16 / 8192 =
// 2^19 chunks per thread, 4080 per chunk (scene_cut.hip)
constexpr size_t MAX_FRAME_BYTES = (size_t)1 << 36;

// what the device keeps per slot (one array of max_streams of them); the layout of ss4k_scene_cut_stats after s_prev
struct SlotState { unsigned long long s_prev, compared, cuts, last_sad, last_score; int32_t last_was_cut, reserved; };

// One pointer table per launch, BY VALUE in the kernel arguments (as FrvsrFramesIn: no device table, no upload).  Entries past n are not read.
// item i: frame a[i] against b[i], `bytes` bytes each at ANY byte address; bit i of `compare` clear: the item is not summed
struct SadItems { const uint8_t* a[MAX_ITEMS]; uint8_t* b[MAX_ITEMS]; unsigned long long compare; };
struct DecideItems { int32_t slot[MAX_ITEMS]; unsigned long long compare, T; };
struct ClearItems { void* lr[MAX_ITEMS]; void* hr[MAX_ITEMS]; };

// acc[i] += sum over the frame of |a[i] - b[i]| for every item whose compare bit is set (acc: n u64, zero before a round; one 64-bit atomic
// add per workgroup and item).  store: b[i] is overwritten with a[i] in the same pass, by the thread that read the bytes, for EVERY item -
// an item that is not compared is only copied.  !store: nothing but acc is written and every item must be compared.
void sad_items(const SadItems& it, unsigned long long* acc, int n, size_t bytes, bool store, hipStream_t st);
// one thread per item: the rule on acc[i] and state[slot[i]] -> flags[i] (1 = cut), the slot's S_prev / counters / last values, acc[i] = 0
void decide(const DecideItems& it, unsigned long long* acc, SlotState* state, uint32_t* flags, int n, hipStream_t st);
// The rule over a RUN of n consecutive frames of one stream (the temporal BSVD service: a job's frames), one thread walking them in order
// because frame i's score needs frame i - 1's sum: acc[i] = sum |frame i - frame i - 1| (acc[0]: against the previous job's last frame;
// not read unless compare_first).  Writes ring[(pos + i) & mask] = 1 where frame i starts a scene, else 0; updates state[0] (S_prev, the
// counters, the last values); acc[0..n) = 0.  mask = 2^k - 1 >= n - 1.
void decide_run(unsigned long long* acc, SlotState* state, uint32_t* ring, unsigned pos, unsigned mask, int n, bool compare_first,
                unsigned long long T, hipStream_t st);
// lr[i] (lr_bytes) and hr[i] (hr_bytes) become zero for every item with flags[i] != 0; an item that was not compared may hold NULLs (its flag is 0).
// Sizes are multiples of 4, pointers of compared items 16-byte aligned
void clear_items(const ClearItems& it, unsigned long long compare, const uint32_t* flags, int n, size_t lr_bytes, size_t hr_bytes, hipStream_t st);

}  // namespace cut

// The detector of one ss4k_frvsr_upscaler: it lives BESIDE FrvsrUpscaler (frvsr.h: struct ss4k_frvsr_upscaler), never inside it - frvsr.cpp and
// the executor stay what they are, and a stream with the detector off runs the code it ran before there was one.
struct SceneCut {
  double threshold = 0;      // mean absolute byte difference in 8-bit levels, (0, 255]; 0 = off
  struct Stored { DevBuf prev; int h = 0, w = 0; bool have = false; };   // a slot's last input frame, uint8 HWC as it arrived
  std::vector<Stored> stored;
  DevBuf state, acc, flags;  // SlotState[max_streams], u64[MAX_ITEMS], u32[MAX_ITEMS]
  cut::SlotState* host = nullptr;   // pinned copy of `state`, refreshed by an asynchronous copy at the end of every round's detection
  size_t host_n = 0;
  bool fresh = true;         // the device state has not been zeroed yet (done on the first round's stream)
  ~SceneCut();
  bool on() const { return threshold > 0; }
  void set(double t, size_t max_streams);
  size_t bytes() const;
  // FrvsrUpscaler::check_round from outside: every refusal of a round that its slots and sizes decide
  static void check_round(const FrvsrUpscaler& u, const int32_t* slot_ids, int S, int h, int w, bool area_chain);
  // the round's three launches in front of FrvsrUpscaler::round / round_at; the caller has made every refusal of the round before
  void detect(const FrvsrUpscaler& u, const uint8_t* const* frames, const int32_t* slot_ids, int S, int h, int w, hipStream_t st);
};

// the three entry points' bodies while the detector is on (api.cpp): every refusal of the round first, then detect(), then the unchanged round
void scene_cut_round(ss4k_frvsr_upscaler* up, const uint8_t* in, const int32_t* slot_ids, int S, int h, int w, uint8_t* out, hipStream_t st);
void scene_cut_round_at(ss4k_frvsr_upscaler* up, const uint8_t* const* in, const int32_t* slot_ids, int S, int h, int w, uint8_t* const* out, hipStream_t st);
void scene_cut_frames(ss4k_frvsr_upscaler* up, const uint8_t* in, int n, int h, int w, uint8_t* out, hipStream_t st);

}  // namespace ss4k
