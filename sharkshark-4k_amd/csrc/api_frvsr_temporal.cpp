// C ABI of the frame-recurrent chain with the online BSVD denoiser in front (include/ss4k.h: ss4k_frvsr_temporal_*) and - dev library only - its
// glue kernel on caller buffers and the guard-mode poison of its job buffers (include/ss4k_dev.h).
#include "api_guard.h"
#include "frvsr_temporal.h"
#include <memory>

using namespace ss4k;

extern "C" {

int ss4k_frvsr_temporal_create(ss4k_ctx* ctx, ss4k_frvsr* frvsr, ss4k_model* bsvd_stream_model, int lr_h, int lr_w, int out_h, int out_w,
                               double denoise_rate, int max_push, int max_streams, ss4k_frvsr_temporal** out) {
  return guard([&] {
    SS4K_REQUIRE(ctx && frvsr && bsvd_stream_model && out, "ss4k_frvsr_temporal_create: NULL argument");
    SS4K_HIP(hipSetDevice(ctx->device));
    auto u = std::make_unique<ss4k_frvsr_temporal>();
    u->t.create(ctx, &frvsr->f, &bsvd_stream_model->m, lr_h, lr_w, out_h, out_w, denoise_rate, max_push, max_streams);
    *out = u.release();
  });
}
int ss4k_frvsr_temporal_create_padded(ss4k_ctx* ctx, ss4k_frvsr* frvsr, ss4k_model* bsvd_stream_model, int lr_h, int lr_w, int out_h, int out_w,
                                      double denoise_rate, int max_push, int max_streams, ss4k_frvsr_temporal** out) {
  return guard([&] {
    SS4K_REQUIRE(ctx && frvsr && bsvd_stream_model && out, "ss4k_frvsr_temporal_create_padded: NULL argument");
    SS4K_HIP(hipSetDevice(ctx->device));
    auto u = std::make_unique<ss4k_frvsr_temporal>();
    u->t.create(ctx, &frvsr->f, &bsvd_stream_model->m, lr_h, lr_w, out_h, out_w, denoise_rate, max_push, max_streams, true);
    *out = u.release();
  });
}
void ss4k_frvsr_temporal_destroy(ss4k_frvsr_temporal* up) { delete up; }
int ss4k_frvsr_temporal_round(ss4k_frvsr_temporal* up, const uint8_t* const* frames_dev, const int* slots, int k_frames, int h, int w,
                              uint8_t* out_dev, size_t out_capacity_bytes, int* n_out_per_item, int* item_slots, int* n_items, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_frvsr_temporal_round: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.ctx->device));
    (void)up->t.round(frames_dev, slots, k_frames, h, w, out_dev, out_capacity_bytes, n_out_per_item, item_slots, n_items, (hipStream_t)stream);
  });
}
int ss4k_frvsr_temporal_flush_stream(ss4k_frvsr_temporal* up, int slot, uint8_t* out, size_t cap, int* n_out, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && n_out, "ss4k_frvsr_temporal_flush_stream: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.ctx->device));
    (void)up->t.slot(slot);   // (a slot outside the object: refused before anything else)
    *n_out = up->t.flush(slot, out, cap, (hipStream_t)stream);
  });
}
int ss4k_frvsr_temporal_reset_stream(ss4k_frvsr_temporal* up, int slot) {
  return guard([&] { SS4K_REQUIRE(up, "ss4k_frvsr_temporal_reset_stream: NULL argument"); up->t.reset(slot); });
}
int ss4k_frvsr_temporal_pending_stream(const ss4k_frvsr_temporal* up, int slot, int* frames) {
  return guard([&] {
    SS4K_REQUIRE(up && frames, "ss4k_frvsr_temporal_pending_stream: NULL argument");
    *frames = up->t.pending(slot);
  });
}
int ss4k_frvsr_temporal_set_denoise_rate_stream(ss4k_frvsr_temporal* up, int slot, float rate) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_frvsr_temporal_set_denoise_rate_stream: NULL argument");
    up->t.set_denoise_rate(slot, rate);
  });
}
int ss4k_frvsr_temporal_set_noise_map(ss4k_frvsr_temporal* up, int mode) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_frvsr_temporal_set_noise_map: NULL argument");
    up->t.set_noise_map(mode);
  });
}
int ss4k_frvsr_temporal_noise_map(const ss4k_frvsr_temporal* up, int* mode) {
  return guard([&] {
    SS4K_REQUIRE(up && mode, "ss4k_frvsr_temporal_noise_map: NULL argument");
    *mode = up->t.noise_map;
  });
}
int ss4k_frvsr_temporal_out_shape(const ss4k_frvsr_temporal* up, int* oh, int* ow) {
  return guard([&] { SS4K_REQUIRE(up && oh && ow, "ss4k_frvsr_temporal_out_shape: NULL argument"); up->t.out_shape(oh, ow); });
}
int ss4k_frvsr_temporal_state_bytes(const ss4k_frvsr_temporal* up, size_t* bytes) {
  return guard([&] { SS4K_REQUIRE(up && bytes, "ss4k_frvsr_temporal_state_bytes: NULL argument"); *bytes = up->t.state_bytes(); });
}
int ss4k_frvsr_temporal_stream_state_bytes_for(const ss4k_frvsr_temporal* up, size_t* bytes) {
  return guard([&] {
    SS4K_REQUIRE(up && bytes, "ss4k_frvsr_temporal_stream_state_bytes_for: NULL argument");
    *bytes = up->t.stream_state_bytes_for();
  });
}
int ss4k_frvsr_temporal_release_idle(ss4k_frvsr_temporal* up) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_frvsr_temporal_release_idle: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.ctx->device));
    up->t.release_idle();
  });
}

int ss4k_frvsr_temporal_set_scene_cut(ss4k_frvsr_temporal* up, double threshold) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_frvsr_temporal_set_scene_cut: NULL argument");
    SS4K_HIP(hipSetDevice(up->t.ctx->device));
    up->t.set_scene_cut(threshold);
  });
}
int ss4k_frvsr_temporal_scene_cut(const ss4k_frvsr_temporal* up, double* threshold) {
  return guard([&] {
    SS4K_REQUIRE(up && threshold, "ss4k_frvsr_temporal_scene_cut: NULL argument");
    *threshold = up->t.cut_threshold;
  });
}
int ss4k_frvsr_temporal_scene_cut_stats_stream(ss4k_frvsr_temporal* up, int slot, ss4k_scene_cut_stats* out, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && out, "ss4k_frvsr_temporal_scene_cut_stats_stream: NULL argument");
    cut::SlotState s{};
    const TemporalCut* c = up->t.slot(slot).cut.get();
    if (c && c->on() && !c->fresh) {
      SS4K_HIP(hipSetDevice(up->t.ctx->device));
      SS4K_HIP(hipMemcpyAsync(&s, c->state.ptr, sizeof(s), hipMemcpyDeviceToHost, (hipStream_t)stream));
      SS4K_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
#ifdef SS4K_DEV
    SS4K_REQUIRE(!c || c->zones_intact(), "ss4k_frvsr_temporal_scene_cut_stats_stream: a red zone around the pinned stats block was written");
#endif
    out->compared = s.compared; out->cuts = s.cuts; out->last_sad = s.last_sad; out->last_score = s.last_score;
    out->last_was_cut = s.last_was_cut; out->reserved = 0;
  });
}
int ss4k_frvsr_temporal_scene_cut_total(const ss4k_frvsr_temporal* up, uint64_t* cuts) {
  return guard([&] {
    SS4K_REQUIRE(up && cuts, "ss4k_frvsr_temporal_scene_cut_total: NULL argument");
    uint64_t n = 0;
    for (const auto& s : up->t.slots) {
      if (!(s->cut && s->cut->host)) continue;
      const volatile cut::SlotState* h = s->cut->host;   // (written by the device's copies: read once, no synchronisation)
      n += h->cuts;
    }
    *cuts = n;
  });
}

#ifdef SS4K_DEV
int ss4k_dev_op_frvsrt_clear_flagged(ss4k_ctx* c, const uint32_t* const* flags, void* const* lr, void* const* hr, int n_items, size_t lr_bytes,
                                     size_t hr_bytes, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && flags && lr && hr, "ss4k_dev_op_frvsrt_clear_flagged: NULL argument");
    SS4K_REQUIRE(n_items >= 1 && n_items <= FRVT_MAX_ITEMS, "ss4k_dev_op_frvsrt_clear_flagged: 1..64 items");
    FrvtClearTable tab{};
    for (int i = 0; i < n_items; ++i) { tab.flag[i] = flags[i]; tab.lr[i] = lr[i]; tab.hr[i] = hr[i]; }
    op_frvt_clear_flagged_items(tab, n_items, lr_bytes, hr_bytes, (hipStream_t)s);
    SS4K_HIP(hipGetLastError());
  });
}
int ss4k_dev_op_frvsrt_denoised_in(ss4k_ctx* c, const float* const* den, const float* const* lr, float* const* dst, int n_items, int h, int w,
                                   const float* taps_dev, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && den && lr && dst, "ss4k_dev_op_frvsrt_denoised_in: NULL argument");
    SS4K_REQUIRE(n_items >= 1 && n_items <= FRVT_MAX_ITEMS, "ss4k_dev_op_frvsrt_denoised_in: 1..64 items");
    FrvtTable tab{};
    for (int i = 0; i < n_items; ++i) { tab.den[i] = den[i]; tab.lr[i] = lr[i]; tab.dst[i] = dst[i]; }
    op_frvt_denoised_in_items(tab, n_items, h, w, taps_dev, 0.8f, (float)(1 - 0.8), (hipStream_t)s);
    SS4K_HIP(hipGetLastError());
  });
}
int ss4k_dev_op_frvsrt_denoised_in_crop(ss4k_ctx* c, const float* const* den, const float* const* lr, float* const* dst, int n_items, int h, int w,
                                        int ph, int pw, const float* taps_dev, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && den && lr && dst, "ss4k_dev_op_frvsrt_denoised_in_crop: NULL argument");
    SS4K_REQUIRE(n_items >= 1 && n_items <= FRVT_MAX_ITEMS, "ss4k_dev_op_frvsrt_denoised_in_crop: 1..64 items");
    FrvtTable tab{};
    for (int i = 0; i < n_items; ++i) { tab.den[i] = den[i]; tab.lr[i] = lr[i]; tab.dst[i] = dst[i]; }
    op_frvt_denoised_in_crop_items(tab, n_items, h, w, ph, pw, taps_dev, 0.8f, (float)(1 - 0.8), (hipStream_t)s);
    SS4K_HIP(hipGetLastError());
  });
}
int ss4k_dev_guard_poison_frvsr_temporal(ss4k_frvsr_temporal* up, int* buffers, size_t* bytes, size_t* bytes_256) {
  return guard([&] {
    SS4K_REQUIRE(up && buffers && bytes && bytes_256, "ss4k_dev_guard_poison_frvsr_temporal: NULL argument");
    *buffers = 0; *bytes = 0; *bytes_256 = 0;
    SS4K_HIP(hipDeviceSynchronize());
    for (DevBuf* b : {&up->t.lr4, &up->t.den}) {   // (a padded object's are these two as well, at the denoiser's larger shape)
      if (!b->ptr || !b->transient) continue;
      SS4K_HIP(hipMemset(b->ptr, 0xFF, b->bytes));
      *buffers += 1; *bytes += b->bytes; *bytes_256 += (b->bytes + 255) & ~size_t(255);
    }
    SS4K_HIP(hipDeviceSynchronize());
  });
}
#endif

}  // extern "C"
