// C ABI of the online BSVD machine and of the service chain around it (include/ss4k.h: ss4k_bsvd_online_*, ss4k_upscaler_temporal_*),
// scene cuts included, and - dev library only - the machine's kernels on caller buffers
// (include/ss4k_dev.h: ss4k_dev_op_bsvd_online_*).
#include "api_guard.h"
#include "bsvd_online.h"
#include "upscaler_temporal.h"
#include <memory>

using namespace ss4k;

extern "C" {

int ss4k_bsvd_online_create(ss4k_ctx* ctx, ss4k_model* model, int max_push, ss4k_bsvd_online** out) {
  return guard([&] {
    SS4K_REQUIRE(ctx && model && out, "ss4k_bsvd_online_create: NULL argument");
    auto o = std::make_unique<ss4k_bsvd_online>();
    o->o.create(ctx, &model->m, max_push);
    *out = o.release();
  });
}
void ss4k_bsvd_online_destroy(ss4k_bsvd_online* o) { delete o; }
int ss4k_bsvd_online_lag(const ss4k_bsvd_online* o) { return o ? o->o.lag() : SS4K_EINVAL; }
int ss4k_bsvd_online_push(ss4k_bsvd_online* o, const float* in, int n, int h, int w, float* out, size_t cap, int* n_out, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(o && n_out, "ss4k_bsvd_online_push: NULL argument");
    SS4K_HIP(hipSetDevice(o->o.ctx->device));
    *n_out = o->o.push(in, n, h, w, out, cap, (hipStream_t)stream);
  });
}
int ss4k_bsvd_online_push_cuts(ss4k_bsvd_online* o, const float* in, const uint32_t* cuts, int n, int h, int w, float* out, size_t cap, int* n_out,
                               void* stream) {
  return guard([&] {
    SS4K_REQUIRE(o && n_out, "ss4k_bsvd_online_push_cuts: NULL argument");
    SS4K_HIP(hipSetDevice(o->o.ctx->device));
    *n_out = o->o.push(in, n, h, w, out, cap, (hipStream_t)stream, cuts);
  });
}
int ss4k_bsvd_online_flush(ss4k_bsvd_online* o, float* out, size_t cap, int* n_out, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(o && n_out, "ss4k_bsvd_online_flush: NULL argument");
    SS4K_HIP(hipSetDevice(o->o.ctx->device));
    *n_out = o->o.flush(out, cap, (hipStream_t)stream);
  });
}
int ss4k_bsvd_online_reset(ss4k_bsvd_online* o) { if (!o) return SS4K_EINVAL; o->o.reset(); return SS4K_OK; }
int ss4k_bsvd_online_pending(const ss4k_bsvd_online* o, int* frames) {
  if (!o || !frames) return SS4K_EINVAL;
  *frames = o->o.pending();
  return SS4K_OK;
}
int ss4k_bsvd_online_state_bytes(const ss4k_bsvd_online* o, size_t* bytes) {
  if (!o || !bytes) return SS4K_EINVAL;
  *bytes = o->o.state_bytes();
  return SS4K_OK;
}

int ss4k_upscaler_temporal_create(ss4k_ctx* ctx, const ss4k_upscale_cfg* cfg, ss4k_model* sr, ss4k_model* bsvd_stream_model, int max_push,
                                  ss4k_upscaler_temporal** out) {
  return guard([&] {
    SS4K_REQUIRE(ctx && cfg && sr && bsvd_stream_model && out, "ss4k_upscaler_temporal_create: NULL argument");
    SS4K_HIP(hipSetDevice(ctx->device));
    auto u = std::make_unique<ss4k_upscaler_temporal>();
    u->t.create(ctx, *cfg, &sr->m, &bsvd_stream_model->m, max_push);
    *out = u.release();
  });
}
void ss4k_upscaler_temporal_destroy(ss4k_upscaler_temporal* up) { delete up; }
int ss4k_upscale_frames_temporal(ss4k_upscaler_temporal* up, const uint8_t* in, int n, int h, int w, uint8_t* out, size_t cap, int* n_out, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && n_out, "ss4k_upscale_frames_temporal: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.up.ctx->device));
    *n_out = up->t.frames(in, n, h, w, out, cap, (hipStream_t)stream);
  });
}
int ss4k_upscaler_temporal_flush(ss4k_upscaler_temporal* up, uint8_t* out, size_t cap, int* n_out, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && n_out, "ss4k_upscaler_temporal_flush: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.up.ctx->device));
    *n_out = up->t.flush(0, out, cap, (hipStream_t)stream);
  });
}
int ss4k_upscaler_temporal_reset(ss4k_upscaler_temporal* up) { if (!up) return SS4K_EINVAL; up->t.reset(0); return SS4K_OK; }
int ss4k_upscaler_temporal_out_shape(const ss4k_upscaler_temporal* up, int h, int w, int* oh, int* ow) {
  return guard([&] { SS4K_REQUIRE(up && oh && ow, "NULL argument"); up->t.up.out_shape(h, w, oh, ow); });
}
int ss4k_upscaler_temporal_pending(const ss4k_upscaler_temporal* up, int* frames) {
  if (!up || !frames) return SS4K_EINVAL;
  *frames = up->t.slot(0).on.pending();
  return SS4K_OK;
}
int ss4k_upscaler_temporal_state_bytes(const ss4k_upscaler_temporal* up, size_t* bytes) {
  if (!up || !bytes) return SS4K_EINVAL;
  *bytes = up->t.state_bytes();
  return SS4K_OK;
}

int ss4k_upscaler_temporal_set_scene_cut(ss4k_upscaler_temporal* up, double threshold) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_upscaler_temporal_set_scene_cut: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.up.ctx->device));
    up->t.set_scene_cut(threshold);
  });
}
int ss4k_upscaler_temporal_scene_cut(const ss4k_upscaler_temporal* up, double* threshold) {
  return guard([&] {
    SS4K_REQUIRE(up && threshold, "ss4k_upscaler_temporal_scene_cut: NULL argument");
    *threshold = up->t.cut_threshold;
  });
}
static void cut_stats_of(ss4k_upscaler_temporal* up, int slot, ss4k_scene_cut_stats* out, void* stream) {
  cut::SlotState s{};
  const TemporalCut* c = up->t.slot(slot).cut.get();
  if (c && c->on() && !c->fresh) {
    SS4K_HIP(hipSetDevice(up->t.up.ctx->device));
    SS4K_HIP(hipMemcpyAsync(&s, c->state.ptr, sizeof(s), hipMemcpyDeviceToHost, (hipStream_t)stream));
    SS4K_HIP(hipStreamSynchronize((hipStream_t)stream));
  }
#ifdef SS4K_DEV
  SS4K_REQUIRE(!c || c->zones_intact(), "ss4k_upscaler_temporal_scene_cut_stats: a red zone around the pinned stats block was written");
#endif
  out->compared = s.compared; out->cuts = s.cuts; out->last_sad = s.last_sad; out->last_score = s.last_score;
  out->last_was_cut = s.last_was_cut; out->reserved = 0;
}
int ss4k_upscaler_temporal_scene_cut_stats(ss4k_upscaler_temporal* up, ss4k_scene_cut_stats* out, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && out, "ss4k_upscaler_temporal_scene_cut_stats: NULL argument");
    cut_stats_of(up, 0, out, stream);
  });
}
int ss4k_upscaler_temporal_scene_cut_stats_stream(ss4k_upscaler_temporal* up, int slot, ss4k_scene_cut_stats* out, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && out, "ss4k_upscaler_temporal_scene_cut_stats_stream: NULL argument");
    cut_stats_of(up, slot, out, stream);
  });
}
int ss4k_upscaler_temporal_scene_cut_total(const ss4k_upscaler_temporal* up, uint64_t* cuts) {
  return guard([&] {
    SS4K_REQUIRE(up && cuts, "ss4k_upscaler_temporal_scene_cut_total: NULL argument");
    uint64_t n = 0;
    for (const auto& s : up->t.slots) {
      if (!(s->cut && s->cut->host)) continue;
      const volatile cut::SlotState* h = s->cut->host;   // (written by the device's copies: read once, no synchronisation)
      n += h->cuts;
    }
    *cuts = n;
  });
}

// ---- several streams on one object: slots and rounds (upscaler_temporal.h, temporal_round_plan.h)
int ss4k_upscaler_temporal_create_streams(ss4k_ctx* ctx, const ss4k_upscale_cfg* cfg, ss4k_model* sr, ss4k_model* bsvd_stream_model, int max_push,
                                          int max_streams, ss4k_upscaler_temporal** out) {
  return guard([&] {
    SS4K_REQUIRE(ctx && cfg && sr && bsvd_stream_model && out, "ss4k_upscaler_temporal_create_streams: NULL argument");
    SS4K_HIP(hipSetDevice(ctx->device));
    auto u = std::make_unique<ss4k_upscaler_temporal>();
    u->t.create(ctx, *cfg, &sr->m, &bsvd_stream_model->m, max_push, max_streams);
    *out = u.release();
  });
}
int ss4k_upscale_round_temporal(ss4k_upscaler_temporal* up, const uint8_t* const* frames_dev, const int* slots, int k_frames, int h, int w,
                                uint8_t* out_dev, size_t out_capacity_bytes, int* n_out_per_item, int* item_slots, int* n_items, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_upscale_round_temporal: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.up.ctx->device));
    (void)up->t.round(frames_dev, slots, k_frames, h, w, out_dev, out_capacity_bytes, n_out_per_item, item_slots, n_items, (hipStream_t)stream);
  });
}
int ss4k_upscaler_temporal_flush_stream(ss4k_upscaler_temporal* up, int slot, uint8_t* out, size_t cap, int* n_out, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && n_out, "ss4k_upscaler_temporal_flush_stream: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.up.ctx->device));
    (void)up->t.slot(slot);   // (a slot outside the object: refused before anything else)
    *n_out = up->t.flush(slot, out, cap, (hipStream_t)stream);
  });
}
int ss4k_upscaler_temporal_reset_stream(ss4k_upscaler_temporal* up, int slot) {
  return guard([&] { SS4K_REQUIRE(up, "ss4k_upscaler_temporal_reset_stream: NULL argument"); up->t.reset(slot); });
}
int ss4k_upscaler_temporal_pending_stream(const ss4k_upscaler_temporal* up, int slot, int* frames) {
  return guard([&] {
    SS4K_REQUIRE(up && frames, "ss4k_upscaler_temporal_pending_stream: NULL argument");
    *frames = up->t.slot(slot).on.pending();
  });
}
int ss4k_upscaler_temporal_stream_state_bytes_for(const ss4k_upscaler_temporal* up, size_t* bytes) {
  return guard([&] {
    SS4K_REQUIRE(up && bytes, "ss4k_upscaler_temporal_stream_state_bytes_for: NULL argument");
    *bytes = up->t.stream_state_bytes_for();
  });
}
int ss4k_upscaler_temporal_release_idle(ss4k_upscaler_temporal* up) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_upscaler_temporal_release_idle: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.up.ctx->device));
    up->t.release_idle();
  });
}
int ss4k_upscaler_temporal_set_denoise_rate_stream(ss4k_upscaler_temporal* up, int slot, float rate) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_upscaler_temporal_set_denoise_rate_stream: NULL argument");
    up->t.set_denoise_rate(slot, rate);
  });
}
int ss4k_upscaler_temporal_set_noise_map(ss4k_upscaler_temporal* up, int mode) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_upscaler_temporal_set_noise_map: NULL argument");
    up->t.set_noise_map(mode);
  });
}
int ss4k_upscaler_temporal_noise_map(const ss4k_upscaler_temporal* up, int* mode) {
  return guard([&] {
    SS4K_REQUIRE(up && mode, "ss4k_upscaler_temporal_noise_map: NULL argument");
    *mode = up->t.noise_map;
  });
}

#ifdef SS4K_DEV
static void dev_temporal_gather_motion(const float* const* src, const float* const* prev, const uint32_t* const* flags, int k, int lh, int lw,
                                       bool pad, uint64_t start_bits, float level_start, const float* scales, float* dst, void* s) {
  SS4K_REQUIRE(k >= 1 && k <= TROUND_MAX_FRAMES, "ss4k_dev_op_temporal_gather_motion: 1..64 frames");
  TroundTable tab{};
  unsigned long long bits = (unsigned long long)start_bits;
  for (int j = 0; j < k; ++j) {
    tab.src[j] = src[j]; tab.prev[j] = prev[j]; tab.flag[j] = flags ? flags[j] : nullptr; tab.level[j] = scales[j];
    if (!prev[j]) bits |= 1ull << j;   // no previous frame: the constant
  }
  if (pad) op_tround_gather_motion_pad(tab, dst, k, lh, lw, bits, level_start, (hipStream_t)s);
  else op_tround_gather_motion(tab, dst, k, lh, lw, bits, level_start, (hipStream_t)s);
}
int ss4k_dev_op_temporal_gather_motion(ss4k_ctx* c, const float* const* src, const float* const* prev, const uint32_t* const* flags, int k, int lh,
                                       int lw, uint64_t start_bits, float level_start, const float* scales, float* dst, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && src && prev && scales, "ss4k_dev_op_temporal_gather_motion: NULL argument");
    dev_temporal_gather_motion(src, prev, flags, k, lh, lw, false, start_bits, level_start, scales, dst, s);
  });
}
int ss4k_dev_op_temporal_gather_motion_pad(ss4k_ctx* c, const float* const* src, const float* const* prev, const uint32_t* const* flags, int k,
                                           int lh, int lw, uint64_t start_bits, float level_start, const float* scales, float* dst, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && src && prev && scales, "ss4k_dev_op_temporal_gather_motion_pad: NULL argument");
    dev_temporal_gather_motion(src, prev, flags, k, lh, lw, true, start_bits, level_start, scales, dst, s);
  });
}
int ss4k_dev_temporal_motion_tile(int* th, int* tw) {
  if (!th || !tw) return SS4K_EINVAL;
  *th = TROUND_MOTION_TILE_H; *tw = TROUND_MOTION_TILE_W;
  return SS4K_OK;
}
int ss4k_dev_temporal_motion_taps(float* taps9) {
  if (!taps9) return SS4K_EINVAL;
  temporal_round::motion_taps(taps9);
  return SS4K_OK;
}
#endif

#ifdef SS4K_DEV
// one launcher call behind both dev entries: levels[j] per frame, or one level for all of them
static void dev_temporal_gather(const float* const* src, const uint32_t* const* flags, int k, size_t plane_px, int planes, uint64_t start_bits,
                                float level_start, const float* levels, float level, float* dst, void* s) {
  SS4K_REQUIRE(k >= 1 && k <= TROUND_MAX_FRAMES, "ss4k_dev_op_temporal_gather: 1..64 frames");
  TroundTable tab{};
  for (int j = 0; j < k; ++j) { tab.src[j] = src[j]; tab.flag[j] = flags ? flags[j] : nullptr; tab.level[j] = levels ? levels[j] : level; }
  op_tround_gather(tab, dst, k, plane_px, planes, (unsigned long long)start_bits, level_start, (hipStream_t)s);
}
int ss4k_dev_op_temporal_gather_levels(ss4k_ctx* c, const float* const* src, const uint32_t* const* flags, int k, size_t plane_px, int planes,
                                       uint64_t start_bits, float level_start, const float* levels, float* dst, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && src && levels, "ss4k_dev_op_temporal_gather_levels: NULL argument");
    dev_temporal_gather(src, flags, k, plane_px, planes, start_bits, level_start, levels, 0.f, dst, s);
  });
}
int ss4k_dev_op_temporal_gather_pad(ss4k_ctx* c, const float* const* src, const uint32_t* const* flags, int k, int lh, int lw, uint64_t start_bits,
                                    float level_start, const float* levels, float* dst, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && src && levels, "ss4k_dev_op_temporal_gather_pad: NULL argument");
    SS4K_REQUIRE(k >= 1 && k <= TROUND_MAX_FRAMES, "ss4k_dev_op_temporal_gather_pad: 1..64 frames");
    TroundTable tab{};
    for (int j = 0; j < k; ++j) { tab.src[j] = src[j]; tab.flag[j] = flags ? flags[j] : nullptr; tab.level[j] = levels[j]; }
    op_tround_gather_pad(tab, dst, k, lh, lw, (unsigned long long)start_bits, level_start, (hipStream_t)s);
  });
}
int ss4k_dev_op_temporal_gather(ss4k_ctx* c, const float* const* src, const uint32_t* const* flags, int k, size_t plane_px, int planes,
                                uint64_t start_bits, float level_start, float level, float* dst, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && src, "ss4k_dev_op_temporal_gather: NULL argument");
    dev_temporal_gather(src, flags, k, plane_px, planes, start_bits, level_start, nullptr, level, dst, s);
  });
}
#endif

#ifdef SS4K_DEV
int ss4k_dev_op_bsvd_online_shift_cuts(ss4k_ctx* c, const void* in, void* out, int nplanes, int in_frames, int slot0, int frames, size_t frame_px,
                                       int slots_per_record, int ch_per_plane, int fold, int first_has_prev, int n_next, const uint32_t* flag_ring,
                                       unsigned ring_mask, int f0, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c, "ss4k_dev_op_bsvd_online_shift_cuts: NULL context");
    op_bsvd_online_shift_cuts(in, out, nplanes, in_frames, slot0, frames, frame_px, slots_per_record, ch_per_plane, fold, first_has_prev, n_next,
                              flag_ring, ring_mask, f0, (hipStream_t)s);
  });
}
int ss4k_dev_op_bsvd_noise_planes(ss4k_ctx* c, float* frames4, int n, size_t plane_px, const uint32_t* flags, int stream_first, float level_start,
                                  float level, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c, "ss4k_dev_op_bsvd_noise_planes: NULL context");
    op_bsvd_noise_planes(frames4, n, plane_px, flags, stream_first, level_start, level, (hipStream_t)s);
  });
}
int ss4k_dev_op_bsvd_online_shift(ss4k_ctx* c, const void* in, void* out, int nplanes, int in_frames, int slot0, int frames, size_t frame_px,
                                  int slots_per_record, int ch_per_plane, int fold, int first_has_prev, int n_next, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c, "ss4k_dev_op_bsvd_online_shift: NULL context");
    op_bsvd_online_shift(in, out, nplanes, in_frames, slot0, frames, frame_px, slots_per_record, ch_per_plane, fold, first_has_prev, n_next,
                         (hipStream_t)s);
  });
}
int ss4k_dev_op_bsvd_online_carry(ss4k_ctx* c, int entries, const void* const* src, void* const* dst, const int* nplanes, const int* src_frames,
                                  const int* dst_frames, const int* src_first, const int* count, const size_t* frame_slots, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && src && dst && nplanes && src_frames && dst_frames && src_first && count && frame_slots, "ss4k_dev_op_bsvd_online_carry: NULL argument");
    SS4K_REQUIRE(entries > 0 && entries <= BSVD_ONLINE_MAX_CARRIES, "ss4k_dev_op_bsvd_online_carry: 1..22 entries");
    BsvdCarryTable tab{};
    for (int i = 0; i < entries; ++i) {
      SS4K_REQUIRE(frame_slots[i] > 0 && frame_slots[i] < 4294967296ull, "ss4k_dev_op_bsvd_online_carry: frame_slots outside 32 bits");
      tab.e[i] = BsvdCarry{src[i], dst[i], nplanes[i], src_frames[i], dst_frames[i], src_first[i], count[i], (unsigned)frame_slots[i]};
    }
    op_bsvd_online_carry(tab, entries, (hipStream_t)s);
  });
}
#endif

}  // extern "C"
