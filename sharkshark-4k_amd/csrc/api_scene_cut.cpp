// Scene-cut detection in front of the frame-recurrent upscaler's rounds: the host object (scene_cut.h: SceneCut) and its part of the C ABI
// (include/ss4k.h).  The object lives beside FrvsrUpscaler in ss4k_frvsr_upscaler: it reads the slots (have_state, cur, the state buffers)
// and calls the unchanged round / round_at after its own three launches.  Every device buffer is a DevBuf, so the dev library's guard
// mode sees it.
#include "api_guard.h"
#include "frvsr.h"
#include "scene_cut.h"
#include <cmath>

namespace ss4k {

SceneCut::~SceneCut() {
  if (host) (void)hipHostFree(host);
}

void SceneCut::set(double t, size_t max_streams) {
  SS4K_REQUIRE(t == t && t >= 0.0 && t <= 255.0, "scene cut: the threshold is 0 (off) or a mean absolute difference in (0, 255]");
  if (t == 0.0) {   // off: the stored frames go, and what the counters held with them
    stored.clear();
    state.release(); acc.release(); flags.release();   // (a free waits for the device: no copy into `host` is in flight after it)
    if (host) std::memset(host, 0, host_n * sizeof(cut::SlotState));
    fresh = true;
  } else if (!on()) {   // on again: every slot starts at step 1 of the rule
    stored.clear(); stored.resize(max_streams);
    if (!host) {
      SS4K_HIP(hipHostMalloc((void**)&host, max_streams * sizeof(cut::SlotState), hipHostMallocDefault));
      host_n = max_streams;
    }
    std::memset(host, 0, host_n * sizeof(cut::SlotState));
    fresh = true;
  }
  threshold = t;
}

size_t SceneCut::bytes() const {
  size_t b = 0;
  for (const Stored& s : stored) b += s.prev.bytes;
  return b;
}

void SceneCut::check_round(const FrvsrUpscaler& u, const int32_t* slot_ids, int S, int h, int w, bool area_chain) {
  u.check_round(slot_ids, S, h, w, area_chain);
}

void SceneCut::detect(const FrvsrUpscaler& u, const uint8_t* const* frames, const int32_t* slot_ids, int S, int h, int w, hipStream_t st) {
  const size_t bytes = (size_t)3 * h * w;
  const size_t lr_b = (size_t)3 * u.lr_h * u.lr_w * 4, hr_b = lr_b * 16;
  SS4K_REQUIRE(bytes <= cut::MAX_FRAME_BYTES, "scene cut: frames of more than 2^36 bytes");
  // ---- allocations first: one that fails leaves every comparison that is still possible as it was
  state.ensure(cut::MAX_ITEMS * sizeof(cut::SlotState)); acc.ensure(cut::MAX_ITEMS * 8); flags.ensure(cut::MAX_ITEMS * 4);
  for (int i = 0; i < S; ++i) {
    Stored& sd = stored[(size_t)slot_ids[i]];
    if (sd.prev.bytes < bytes) { sd.have = false; sd.prev.ensure(bytes); }   // (a larger frame than the stored one: no comparison anyway)
  }
  if (fresh) {
    SS4K_HIP(hipMemsetAsync(state.ptr, 0, cut::MAX_ITEMS * sizeof(cut::SlotState), st));
    SS4K_HIP(hipMemsetAsync(acc.ptr, 0, cut::MAX_ITEMS * 8, st));
    SS4K_HIP(hipMemsetAsync(flags.ptr, 0, cut::MAX_ITEMS * 4, st));
    fresh = false;
  }
  cut::SadItems sad{}; cut::DecideItems dec{}; cut::ClearItems clr{};
  for (int i = 0; i < S; ++i) {
    const FrvsrUpscaler::Slot& sl = u.slots[(size_t)slot_ids[i]];
    Stored& sd = stored[(size_t)slot_ids[i]];
    const bool compare = sl.have_state && sd.have && sd.h == h && sd.w == w;   // step 1 of the rule
    sad.a[i] = frames[i]; sad.b[i] = sd.prev.as<uint8_t>();
    dec.slot[i] = slot_ids[i];
    if (compare) {
      sad.compare |= 1ull << i;
      clr.lr[i] = sl.lr[sl.cur].ptr; clr.hr[i] = sl.hr[sl.cur].ptr;   // what the step reads as lr_prev / hr_prev
    }
  }
  dec.compare = sad.compare;
  dec.T = (unsigned long long)std::max(1.0, std::ceil(threshold * 3.0 * (double)h * (double)w));
  cut::sad_items(sad, acc.as<unsigned long long>(), S, bytes, true, st);
  cut::decide(dec, acc.as<unsigned long long>(), state.as<cut::SlotState>(), flags.as<uint32_t>(), S, st);
  cut::clear_items(clr, sad.compare, flags.as<uint32_t>(), S, lr_b, hr_b, st);
  SS4K_HIP(hipMemcpyAsync(host, state.ptr, host_n * sizeof(cut::SlotState), hipMemcpyDeviceToHost, st));
  for (int i = 0; i < S; ++i) {
    Stored& sd = stored[(size_t)slot_ids[i]];
    sd.have = true; sd.h = h; sd.w = w;
  }
}

void scene_cut_round(ss4k_frvsr_upscaler* up, const uint8_t* in, const int32_t* slot_ids, int S, int h, int w, uint8_t* out, hipStream_t st) {
  SceneCut::check_round(up->u, slot_ids, S, h, w, true);
  const uint8_t* frames[SS4K_FRVSR_MAX_STREAMS];
  for (int i = 0; i < S; ++i) frames[i] = in + (size_t)i * h * w * 3;
  up->u.m->timed(FRV_GLUE, st, [&] { up->cut->detect(up->u, frames, slot_ids, S, h, w, st); });   // (the per-stage timing counts it as glue)
  up->u.round(in, slot_ids, S, h, w, out, st);
}

void scene_cut_round_at(ss4k_frvsr_upscaler* up, const uint8_t* const* in, const int32_t* slot_ids, int S, int h, int w, uint8_t* const* out, hipStream_t st) {
  SceneCut::check_round(up->u, slot_ids, S, h, w, false);
  // round_at's own refusals, which it makes after check_round (frvsr.cpp)
  int oh, ow; up->u.out_shape(&oh, &ow);
  const int H = 4 * up->u.lr_h, W = 4 * up->u.lr_w;
  SS4K_REQUIRE((double)h * up->u.lr_h < 2147483648.0 && (double)w * up->u.lr_w < 2147483648.0 && (double)H * oh < 2147483648.0 && (double)W * ow < 2147483648.0,
               "frvsr round: frame sizes whose area window bounds overflow");
  for (int i = 0; i < S; ++i) SS4K_REQUIRE(in[i] && out[i], "frvsr round: NULL frame pointer");
  up->u.m->timed(FRV_GLUE, st, [&] { up->cut->detect(up->u, in, slot_ids, S, h, w, st); });
  up->u.round_at(in, slot_ids, S, h, w, out, st);
}

void scene_cut_frames(ss4k_frvsr_upscaler* up, const uint8_t* in, int n, int h, int w, uint8_t* out, hipStream_t st) {
  int oh, ow; up->u.out_shape(&oh, &ow);
  const int32_t slot0 = 0;   // (FrvsrUpscaler::frames: n consecutive frames of slot 0, one round each)
  for (int i = 0; i < n; ++i) scene_cut_round(up, in + (size_t)i * h * w * 3, &slot0, 1, h, w, out + (size_t)i * oh * ow * 3, st);
}

}  // namespace ss4k

using namespace ss4k;

ss4k_frvsr_upscaler::~ss4k_frvsr_upscaler() { delete cut; }

extern "C" {

int ss4k_frvsr_upscaler_set_scene_cut(ss4k_frvsr_upscaler* up, double threshold) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_frvsr_upscaler_set_scene_cut: NULL argument");
    if (!up->cut) {
      SS4K_REQUIRE(threshold == threshold && threshold >= 0.0 && threshold <= 255.0, "scene cut: the threshold is 0 (off) or a mean absolute difference in (0, 255]");
      if (threshold == 0.0) return;
      up->cut = new SceneCut();
    }
    up->cut->set(threshold, up->u.slots.size());
  });
}

int ss4k_frvsr_upscaler_scene_cut(const ss4k_frvsr_upscaler* up, double* threshold) {
  return guard([&] {
    SS4K_REQUIRE(up && threshold, "ss4k_frvsr_upscaler_scene_cut: NULL argument");
    *threshold = up->cut ? up->cut->threshold : 0.0;
  });
}

int ss4k_frvsr_upscaler_scene_cut_stats(ss4k_frvsr_upscaler* up, int slot, ss4k_scene_cut_stats* out, void* hip_stream) {
  return guard([&] {
    SS4K_REQUIRE(up && out, "ss4k_frvsr_upscaler_scene_cut_stats: NULL argument");
    SS4K_REQUIRE(slot >= 0 && slot < (int)up->u.slots.size(), "ss4k_frvsr_upscaler_scene_cut_stats: slot outside 0..max_streams-1");
    cut::SlotState s{};
    if (up->cut && up->cut->on() && !up->cut->fresh) {
      SS4K_HIP(hipMemcpyAsync(&s, up->cut->state.as<cut::SlotState>() + slot, sizeof(s), hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
      SS4K_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    }
    out->compared = s.compared; out->cuts = s.cuts; out->last_sad = s.last_sad; out->last_score = s.last_score;
    out->last_was_cut = s.last_was_cut; out->reserved = 0;
  });
}

int ss4k_frvsr_upscaler_scene_cut_total(const ss4k_frvsr_upscaler* up, uint64_t* cuts) {
  return guard([&] {
    SS4K_REQUIRE(up && cuts, "ss4k_frvsr_upscaler_scene_cut_total: NULL argument");
    uint64_t n = 0;
    if (up->cut && up->cut->host) {
      const volatile cut::SlotState* h = up->cut->host;   // (written by the device's copies: read once each, no synchronisation)
      for (size_t i = 0; i < up->cut->host_n; ++i) n += h[i].cuts;
    }
    *cuts = n;
  });
}

int ss4k_op_frame_sad_u8(ss4k_ctx* ctx, const uint8_t* const* a_dev, const uint8_t* const* b_dev, int n_items, size_t bytes_per_frame,
                         uint64_t* sad_out_dev, void* hip_stream) {
  return guard([&] {
    SS4K_REQUIRE(ctx && a_dev && b_dev && sad_out_dev, "ss4k_op_frame_sad_u8: NULL argument");
    SS4K_REQUIRE(n_items >= 1 && n_items <= cut::MAX_ITEMS, "ss4k_op_frame_sad_u8: n_items must be in 1..64");
    SS4K_REQUIRE(bytes_per_frame >= 1 && bytes_per_frame <= cut::MAX_FRAME_BYTES, "ss4k_op_frame_sad_u8: bytes_per_frame must be in 1..2^36");
    SS4K_REQUIRE(((uintptr_t)sad_out_dev & 7) == 0, "ss4k_op_frame_sad_u8: sad_out_dev must be 8-byte aligned");
    cut::SadItems it{};
    for (int i = 0; i < n_items; ++i) {
      SS4K_REQUIRE(a_dev[i] && b_dev[i], "ss4k_op_frame_sad_u8: NULL frame pointer");
      it.a[i] = a_dev[i]; it.b[i] = const_cast<uint8_t*>(b_dev[i]);   // (the kernel build without the store writes nothing through b)
    }
    it.compare = n_items == 64 ? ~0ull : (1ull << n_items) - 1;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64");
    SS4K_HIP(hipMemsetAsync(sad_out_dev, 0, (size_t)n_items * 8, (hipStream_t)hip_stream));
    cut::sad_items(it, reinterpret_cast<unsigned long long*>(sad_out_dev), n_items, bytes_per_frame, false, (hipStream_t)hip_stream);
  });
}

}  // extern "C"
