// C ABI (include/ss4k.h): context, models, the frame-in/frame-out upscaler and the granular ops.
#include "api_guard.h"
#include "frvsr.h"
#include "host_tables.h"
#include "scene_cut.h"
#include "upscaler.h"
#include <cmath>
#include <cstdarg>
#include <memory>

namespace ss4k {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
void clear_error() { g_err[0] = 0; }

}  // namespace ss4k

using namespace ss4k;

extern "C" {

int ss4k_abi_version(void) { return SS4K_ABI_VERSION; }
const char* ss4k_last_error(void) { return g_err; }

int ss4k_ctx_create(int dev, ss4k_ctx** out) {
  return guard([&] {
    SS4K_REQUIRE(out, "ss4k_ctx_create: out is NULL");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
      throw Error(SS4K_ENODEV, "no HIP device available (libss4k_hip has no CPU fallback)");
    SS4K_REQUIRE(dev >= 0 && dev < count, "ss4k_ctx_create: bad device index");
    SS4K_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop; SS4K_HIP(hipGetDeviceProperties(&prop, dev));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
      throw Error(SS4K_ENODEV, std::string("libss4k_hip is built for gfx950 only; device is ") + prop.gcnArchName);
    auto c = std::make_unique<ss4k_ctx>();
    c->device = dev; c->num_cu = prop.multiProcessorCount;
    *out = c.release();
  });
}
void ss4k_ctx_destroy(ss4k_ctx* c) {
  if (!c) return;
  for (auto& kv : c->scratch) kv.second.release();
  for (auto& e : c->prof_events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto& e : c->prof_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto& e : c->prof_sections) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  if (c->lane_stream_) (void)hipStreamDestroy(c->lane_stream_);
  for (auto ls : c->lane_parked) (void)hipStreamDestroy(ls);
  for (auto& kv : c->cv_area) if (kv.second.uploaded) (void)hipEventDestroy(kv.second.uploaded);
  if (c->fork_event) (void)hipEventDestroy(c->fork_event);
  if (c->done_event) (void)hipEventDestroy(c->done_event);
  delete c;
}
int ss4k_ctx_device(const ss4k_ctx* c) { return c ? c->device : -1; }

size_t ss4k_model_param_count(const ss4k_model_desc* d) { return d ? model_param_count(*d) : 0; }

int ss4k_model_create(ss4k_ctx* ctx, const ss4k_model_desc* d, const float* w, size_t n, ss4k_model** out) {
  return guard([&] {
    SS4K_REQUIRE(ctx && d && w && out, "ss4k_model_create: NULL argument");
    SS4K_HIP(hipSetDevice(ctx->device));
    auto m = std::make_unique<ss4k_model>();
    m->m.ctx = ctx; m->m.desc = *d;
    m->m.build(w, n);
    *out = m.release();
  });
}
void ss4k_model_destroy(ss4k_model* m) { delete m; }
int ss4k_model_out_shape(const ss4k_model* m, int n, int h, int w, int* oc, int* oh, int* ow) {
  return guard([&] { SS4K_REQUIRE(m && oc && oh && ow, "NULL argument"); m->m.out_shape(n, h, w, oc, oh, ow); });
}
int ss4k_model_in_channels(const ss4k_model* m) { return m ? m->m.in_channels() : SS4K_EINVAL; }
int ss4k_model_workspace_bytes(ss4k_model* m, int n, int h, int w, size_t* bytes) {
  return guard([&] {
    SS4K_REQUIRE(m && bytes, "ss4k_model_workspace_bytes: NULL argument");
    *bytes = m->m.workspace_bytes(n, h, w);
  });
}
int ss4k_model_forward(ss4k_model* m, const float* in, float* out, int n, int h, int w, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(m && in && out, "ss4k_model_forward: NULL argument");
    m->m.forward(in, out, n, h, w, (hipStream_t)stream);
  });
}

int ss4k_model_check(ss4k_model* m, int wait) {
  return guard([&] {
    SS4K_REQUIRE(m, "ss4k_model_check: NULL argument");
    (void)wait;   // no kernel has an asynchronous failure mode (include/ss4k.h)
  });
}

int ss4k_upscaler_create(ss4k_ctx* ctx, const ss4k_upscale_cfg* cfg, ss4k_model* sr, ss4k_model* dn, ss4k_upscaler** out) {
  return guard([&] {
    SS4K_REQUIRE(ctx && cfg && sr && out, "ss4k_upscaler_create: NULL argument");
    SS4K_REQUIRE(cfg->lr_h > 0 && cfg->lr_w > 0, "lr_shape must be positive");
    SS4K_REQUIRE(!cfg->denoising || dn, "denoising requested without a BSVD model");
    SS4K_REQUIRE(!cfg->denoising || cfg->single_mode, "the reference only denoises on the per-frame path (fsrcnn_upscaler.py:109,168-233)");
    SS4K_REQUIRE(cfg->single_mode || cfg->sr_is_realesrgan, "the batched path requires a 3-channel SR model (fsrcnn_upscaler.py:180-184)");
    SS4K_REQUIRE((sr->m.in_channels() == 3) == (cfg->sr_is_realesrgan != 0), "sr_is_realesrgan does not match the SR model kind");
    auto u = std::make_unique<ss4k_upscaler>();
    u->u.ctx = ctx; u->u.cfg = *cfg; u->u.sr = &sr->m; u->u.dn = dn ? &dn->m : nullptr;
    u->u.upload_taps();
#ifdef SS4K_DEV
    u->u.for_each_job_buf([](DevBuf& b) { b.transient = true; });   // guard mode (upscaler.h)
#endif
    *out = u.release();
  });
}
void ss4k_upscaler_destroy(ss4k_upscaler* up) { delete up; }
int ss4k_upscaler_reset(ss4k_upscaler* up) { if (!up) return SS4K_EINVAL; up->u.first_frame = true; return SS4K_OK; }
int ss4k_upscaler_out_shape(const ss4k_upscaler* up, int n, int h, int w, int* oh, int* ow) {
  (void)n;
  return guard([&] { SS4K_REQUIRE(up && oh && ow, "NULL argument"); up->u.out_shape(h, w, oh, ow); });
}
int ss4k_upscale_frames(ss4k_upscaler* up, const uint8_t* in, int n, int h, int w, uint8_t* out, size_t cap, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && in && out, "ss4k_upscale_frames: NULL argument");
    SS4K_REQUIRE(n > 0 && h > 0 && w > 0, "ss4k_upscale_frames: empty batch");
    int oh, ow; up->u.out_shape(h, w, &oh, &ow);
    const size_t per = (size_t)oh * ow * 3;
    SS4K_REQUIRE(cap >= per * n, "ss4k_upscale_frames: output buffer too small");
    if (up->u.cfg.single_mode) up->u.single(in, n, h, w, out, (hipStream_t)stream);
    else up->u.multi(in, n, h, w, out, (hipStream_t)stream);
  });
}
int ss4k_upscaler_last_enqueue_ms(const ss4k_upscaler* up, double* denoise_ms, double* model_ms) {
  if (!up || !denoise_ms || !model_ms) return SS4K_EINVAL;
  *denoise_ms = up->u.enq_denoise_ms; *model_ms = up->u.enq_model_ms;
  return SS4K_OK;
}
int ss4k_upscaler_enable_taps(ss4k_upscaler* up, int en) { if (!up) return SS4K_EINVAL; up->u.taps_on = en != 0; return SS4K_OK; }
int ss4k_upscaler_read_tap(ss4k_upscaler* up, int which, float* out, size_t cap, int dims[4], void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && which >= 0 && which < 5 && dims, "bad tap request");
    const int* d = up->u.tap_dims[which];
    for (int i = 0; i < 4; ++i) dims[i] = d[i];
    const size_t nflt = (size_t)d[0] * d[1] * d[2] * d[3];
    SS4K_REQUIRE(nflt > 0, "tap not recorded (enable taps before ss4k_upscale_frames)");
    if (out) {
      SS4K_REQUIRE(cap >= nflt, "tap buffer too small");
      SS4K_HIP(hipMemcpyAsync(out, up->u.tap[which].ptr, nflt * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
  });
}

// ---- granular ops ---------------------------------------------------------------------------
int ss4k_op_u8nhwc_to_f32nchw(ss4k_ctx* c, const uint8_t* in, float* out, int n, int h, int w, int ch, void* s) {
  return guard([&] { SS4K_REQUIRE(c && in && out, "NULL argument"); op_u8nhwc_to_f32nchw(in, out, n, h, w, ch, (hipStream_t)s); SS4K_HIP(hipGetLastError()); });
}
int ss4k_op_area_resize(ss4k_ctx* c, const float* in, float* out, int p, int h, int w, int oh, int ow, void* s) {
  return guard([&] { SS4K_REQUIRE(c && in && out, "NULL argument"); op_area(in, out, p, h, w, oh, ow, (hipStream_t)s); SS4K_HIP(hipGetLastError()); });
}
int ss4k_op_bicubic_resize(ss4k_ctx* c, const float* in, float* out, int p, int h, int w, int oh, int ow, void* s) {
  return guard([&] { SS4K_REQUIRE(c && in && out, "NULL argument"); op_bicubic(in, out, p, h, w, oh, ow, 0, (hipStream_t)s); SS4K_HIP(hipGetLastError()); });
}
int ss4k_op_bilinear_resize(ss4k_ctx* c, const float* in, float* out, int p, int h, int w, int oh, int ow, void* s) {
  return guard([&] { SS4K_REQUIRE(c && in && out, "NULL argument"); op_bilinear(in, out, p, h, w, oh, ow, 0, 0, (hipStream_t)s); SS4K_HIP(hipGetLastError()); });
}
int ss4k_op_depthwise_reflect(ss4k_ctx* c, const float* in, float* out, int p, int h, int w, const float* k2d, int k, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && in && out && k2d, "NULL argument");
    SS4K_REQUIRE(k >= 1 && k <= 17 && (k & 1), "kernel size must be odd and <= 17");
    float* taps = c->buf("dw_taps", 17 * 17 * 4).as<float>();
    SS4K_HIP(hipMemcpyAsync(taps, k2d, (size_t)k * k * 4, hipMemcpyHostToDevice, (hipStream_t)s));
    op_depthwise_reflect(in, out, taps, p, h, w, k, 0, nullptr, 0, 0, (hipStream_t)s);
    SS4K_HIP(hipGetLastError());
  });
}
// ---- cv2.resize(..., INTER_AREA), shrinking by a non-integer factor (glue.hip: k_cv_area_u8; oracle/cv_area.py states the algorithm)
namespace {
int cv_round(double v) { return (int)std::nearbyint(v); }   // saturate_cast<int>(double): round half to even (default rounding mode)
void cv_check_factor(double f) {
  SS4K_REQUIRE(f > 0.0 && f < 1.0, "cv area resize: factors must shrink (0 < f < 1)");
  const double scale = 1.0 / f;
  SS4K_REQUIRE(std::fabs(scale - std::nearbyint(scale)) >= 2.220446049250313e-16, "cv area resize: 1 / f is an integer - OpenCV's fast path (other rounding) is not implemented");
}
}  // namespace
int ss4k_op_cv_area_shape(int h, int w, double fx, double fy, int* oh, int* ow) {
  return guard([&] {
    SS4K_REQUIRE(oh && ow && h > 0 && w > 0, "ss4k_op_cv_area_shape: bad argument");
    cv_check_factor(fx); cv_check_factor(fy);
    *oh = cv_round(h * fy); *ow = cv_round(w * fx);
    SS4K_REQUIRE(*oh > 0 && *ow > 0, "cv area resize: empty output");
  });
}
int ss4k_op_cv_area_resize_u8(ss4k_ctx* c, const uint8_t* in, uint8_t* out, size_t out_capacity, int n, int h, int w, int ch, double fx, double fy, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && in && out, "NULL argument");
    SS4K_REQUIRE(n > 0 && h > 0 && w > 0 && ch >= 1 && ch <= 4, "cv area resize: n, h, w > 0 and 1 <= channels <= 4");
    cv_check_factor(fx); cv_check_factor(fy);
    SS4K_HIP(hipSetDevice(c->device));
    const auto key = std::make_tuple(h, w, fx, fy);
    auto it = c->cv_area.find(key);
    if (it == c->cv_area.end()) {
      if (c->cv_area.size() >= 64) {   // an image server sees arbitrary sizes: bounded; the tables may still be read by enqueued launches
        SS4K_HIP(hipDeviceSynchronize());
        for (auto& kv : c->cv_area) if (kv.second.uploaded) (void)hipEventDestroy(kv.second.uploaded);
        c->cv_area.clear();
      }
      ss4k_ctx::CvAreaTab t;
      t.oh = cv_round(h * fy); t.ow = cv_round(w * fx);
      SS4K_REQUIRE(t.oh > 0 && t.ow > 0, "cv area resize: empty output");
      std::vector<CvEnt> xe, ye; std::vector<int> xo, yo;
      cv_area_tab(w, t.ow, 1.0 / fx, xe, xo);
      cv_area_tab(h, t.oh, 1.0 / fy, ye, yo);
      auto put = [&](const void* p, size_t bytes) { const size_t at = (t.host.size() + 15) & ~size_t(15); t.host.resize(at + bytes); std::memcpy(t.host.data() + at, p, bytes); return at; };
      t.xe = put(xe.data(), xe.size() * sizeof(CvEnt)); t.xo = put(xo.data(), xo.size() * sizeof(int));
      t.ye = put(ye.data(), ye.size() * sizeof(CvEnt)); t.yo = put(yo.data(), yo.size() * sizeof(int));
      t.dev.ensure(t.host.size());
      // upload and event on the LOCAL table; only a complete entry enters the cache (a throw here leaves no half-built entry behind whose
      // NULL event every later call for this shape would wait on).  Moving the table keeps its host buffer's address: the copy stays valid.
      SS4K_HIP(hipMemcpyAsync(t.dev.ptr, t.host.data(), t.host.size(), hipMemcpyHostToDevice, (hipStream_t)s));
      SS4K_HIP(hipEventCreateWithFlags(&t.uploaded, hipEventDisableTiming));
      const hipError_t rec = hipEventRecord(t.uploaded, (hipStream_t)s);
      if (rec != hipSuccess) {
        (void)hipStreamSynchronize((hipStream_t)s);   // the copy above reads t.host: let it finish before the table dies
        (void)hipEventDestroy(t.uploaded);
        SS4K_HIP(rec);
      }
      it = c->cv_area.emplace(key, std::move(t)).first;
    }
    auto& e = it->second;
    SS4K_REQUIRE(out_capacity >= (size_t)n * e.oh * e.ow * ch, "cv area resize: output buffer too small (ss4k_op_cv_area_shape gives the size)");
    SS4K_HIP(hipStreamWaitEvent((hipStream_t)s, e.uploaded, 0));
    const char* d = e.dev.as<char>();
    op_cv_area_u8(in, out, d + e.xe, reinterpret_cast<const int*>(d + e.xo), d + e.ye, reinterpret_cast<const int*>(d + e.yo), n, h, w, ch, e.oh, e.ow, (hipStream_t)s);
  });
}
int ss4k_op_plane_stats(ss4k_ctx* c, const float* in, float* stats, int p, int hw, void* s) {
  return guard([&] {
    SS4K_REQUIRE(c && in && stats, "NULL argument");
    op_plane_stats(c->buf("stats_acc", sizeof(double) * 2 * STATS_MAX_PLANES * STATS_SLOTS).as<double>(), in, stats, p, hw, (hipStream_t)s);
  });
}
int ss4k_op_f32nchw_to_u8nhwc(ss4k_ctx* c, const float* in, uint8_t* out, int n, int ch, int h, int w, void* s) {
  return guard([&] { SS4K_REQUIRE(c && in && out, "NULL argument"); op_f32nchw_to_u8nhwc(in, out, n, ch, h, w, (hipStream_t)s); SS4K_HIP(hipGetLastError()); });
}

// ---- the frame-recurrent upscaler (frvsr.cpp) ----------------------------------------------------
size_t ss4k_frvsr_param_count(const ss4k_frvsr_desc* d) { return d ? frvsr_param_count(*d) : 0; }
size_t ss4k_frvsr_param_count_as(const ss4k_frvsr_desc* d, int generator) { return d ? frvsr_param_count(*d, generator) : 0; }
int ss4k_frvsr_create(ss4k_ctx* ctx, const ss4k_frvsr_desc* d, const float* w, size_t n, ss4k_frvsr** out) {
  return ss4k_frvsr_create_as(ctx, d, SS4K_FRVSR_EGVSR, 0, w, n, out);
}
size_t ss4k_frvsr_param_count_ex(const ss4k_frvsr_desc* d, int generator, int degradation) { return d ? frvsr_param_count(*d, generator, degradation) : 0; }
int ss4k_frvsr_generator(const ss4k_frvsr* m) { return m ? m->f.generator : -1; }
int ss4k_frvsr_degradation(const ss4k_frvsr* m) { return m ? m->f.degradation : -1; }
int ss4k_frvsr_create_as(ss4k_ctx* ctx, const ss4k_frvsr_desc* d, int generator, int route_flags, const float* w, size_t n, ss4k_frvsr** out) {
  return ss4k_frvsr_create_ex(ctx, d, generator, SS4K_FRVSR_BD, route_flags, w, n, out);
}
int ss4k_frvsr_create_ex(ss4k_ctx* ctx, const ss4k_frvsr_desc* d, int generator, int degradation, int route_flags, const float* w, size_t n,
                         ss4k_frvsr** out) {
  return guard([&] {
    SS4K_REQUIRE(ctx && d && w && out, "ss4k_frvsr_create: NULL argument");
    SS4K_HIP(hipSetDevice(ctx->device));
    auto m = std::make_unique<ss4k_frvsr>();
    m->f.ctx = ctx; m->f.desc = *d; m->f.generator = generator; m->f.degradation = degradation; m->f.route_flags = route_flags;
    m->f.build(w, n);   // (validates the three together with the description and the blob size)
#ifdef SS4K_DEV
    for (DevBuf* b : {&m->f.flow_raw, &m->f.flow, &m->f.tap_s2d}) b->transient = true;   // guard mode: every step rewrites what it reads from these
#endif
    *out = m.release();
  });
}
void ss4k_frvsr_destroy(ss4k_frvsr* m) { delete m; }
int ss4k_frvsr_step(ss4k_frvsr* m, const float* lr_curr, const float* lr_prev, const float* hr_prev, float* hr_out, int n, int h, int w, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(m && lr_curr && lr_prev && hr_prev && hr_out, "ss4k_frvsr_step: NULL argument");
    m->f.step(lr_curr, lr_prev, hr_prev, hr_out, n, h, w, (hipStream_t)stream);
  });
}
int ss4k_frvsr_workspace_bytes(ss4k_frvsr* m, int n, int h, int w, size_t* bytes) {
  return guard([&] {
    SS4K_REQUIRE(m && bytes, "ss4k_frvsr_workspace_bytes: NULL argument");
    *bytes = m->f.workspace_bytes(n, h, w);
  });
}
int ss4k_frvsr_prof_enable(ss4k_frvsr* m, int en) {
  return guard([&] {
    SS4K_REQUIRE(m, "ss4k_frvsr_prof_enable: NULL argument");
    m->f.prof_collect();
    if (en) for (double& v : m->f.stage_ms) v = 0;
    m->f.prof = en != 0;
  });
}
int ss4k_frvsr_prof_read(ss4k_frvsr* m, int stage, double* ms) {
  return guard([&] {
    SS4K_REQUIRE(m && ms && stage >= 0 && stage < FRV_STAGES, "ss4k_frvsr_prof_read: bad argument");
    m->f.prof_collect();
    *ms = m->f.stage_ms[stage];
  });
}
int ss4k_frvsr_upscaler_create_streams(ss4k_ctx* ctx, ss4k_frvsr* m, int lr_h, int lr_w, int out_h, int out_w, int max_streams, ss4k_frvsr_upscaler** out) {
  return guard([&] {
    SS4K_REQUIRE(ctx && m && out, "ss4k_frvsr_upscaler_create[_streams]: NULL argument");
    SS4K_REQUIRE(lr_h >= 8 && lr_w >= 8, "lr_shape must be at least 8 x 8");
    SS4K_REQUIRE((out_h == 0 && out_w == 0) || (out_h > 0 && out_w > 0), "output_shape is (0, 0) or positive");
    SS4K_REQUIRE((double)lr_h * lr_w * 16.0 < 2147483648.0, "lr_shape: the output frame must hold fewer than 2^31 pixels");
    SS4K_REQUIRE(max_streams >= 1 && max_streams <= SS4K_FRVSR_MAX_STREAMS, "max_streams must be in 1..64 (SS4K_FRVSR_MAX_STREAMS)");
    auto u = std::make_unique<ss4k_frvsr_upscaler>();
    u->u.ctx = ctx; u->u.m = &m->f; u->u.lr_h = lr_h; u->u.lr_w = lr_w; u->u.out_h = out_h; u->u.out_w = out_w;
    u->u.slots.resize((size_t)max_streams);
#ifdef SS4K_DEV
    for (DevBuf* b : {&u->u.img, &u->u.hrc, &u->u.outf}) b->transient = true;   // (the slots' lr[] and hr[] carry the recurrent state across calls)
#endif
    *out = u.release();
  });
}
int ss4k_frvsr_upscaler_create(ss4k_ctx* ctx, ss4k_frvsr* m, int lr_h, int lr_w, int out_h, int out_w, ss4k_frvsr_upscaler** out) {
  return ss4k_frvsr_upscaler_create_streams(ctx, m, lr_h, lr_w, out_h, out_w, 1, out);
}
void ss4k_frvsr_upscaler_destroy(ss4k_frvsr_upscaler* up) { delete up; }
int ss4k_frvsr_upscaler_reset(ss4k_frvsr_upscaler* up) {
  if (!up) return SS4K_EINVAL;
  for (auto& s : up->u.slots) s.have_state = false;
  return SS4K_OK;
}
int ss4k_frvsr_upscaler_reset_stream(ss4k_frvsr_upscaler* up, int slot) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_frvsr_upscaler_reset_stream: NULL argument");
    SS4K_REQUIRE(slot >= 0 && slot < (int)up->u.slots.size(), "ss4k_frvsr_upscaler_reset_stream: slot outside 0..max_streams-1");
    up->u.slots[(size_t)slot].have_state = false;
  });
}
int ss4k_frvsr_upscaler_state_bytes(const ss4k_frvsr_upscaler* up, size_t* bytes) {
  return guard([&] { SS4K_REQUIRE(up && bytes, "ss4k_frvsr_upscaler_state_bytes: NULL argument"); *bytes = up->u.state_bytes() + (up->cut ? up->cut->bytes() : 0); });
}
int ss4k_frvsr_upscaler_out_shape(const ss4k_frvsr_upscaler* up, int* oh, int* ow) {
  return guard([&] { SS4K_REQUIRE(up && oh && ow, "NULL argument"); up->u.out_shape(oh, ow); });
}
int ss4k_frvsr_upscale_frames(ss4k_frvsr_upscaler* up, const uint8_t* in, int n, int h, int w, uint8_t* out, size_t cap, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && in && out, "ss4k_frvsr_upscale_frames: NULL argument");
    SS4K_REQUIRE(n > 0 && h > 0 && w > 0, "ss4k_frvsr_upscale_frames: empty batch");
    int oh, ow; up->u.out_shape(&oh, &ow);
    SS4K_REQUIRE(cap >= (size_t)oh * ow * 3 * n, "ss4k_frvsr_upscale_frames: output buffer too small");
    if (up->cut && up->cut->on()) scene_cut_frames(up, in, n, h, w, out, (hipStream_t)stream);   // (the detector's launches in front of every round)
    else up->u.frames(in, n, h, w, out, (hipStream_t)stream);
  });
}
int ss4k_frvsr_upscale_streams(ss4k_frvsr_upscaler* up, const int32_t* slots, int n_streams, const uint8_t* in, int h, int w, uint8_t* out, size_t cap,
                               void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_frvsr_upscale_streams: NULL argument");
    SS4K_REQUIRE(n_streams >= 1 && n_streams <= (int)up->u.slots.size(), "ss4k_frvsr_upscale_streams: n_streams must be in 1..max_streams");
    SS4K_REQUIRE(slots && in && out, "ss4k_frvsr_upscale_streams: NULL argument");
    SS4K_REQUIRE(h > 0 && w > 0, "ss4k_frvsr_upscale_streams: empty frames");
    int oh, ow; up->u.out_shape(&oh, &ow);
    SS4K_REQUIRE(cap >= (size_t)oh * ow * 3 * n_streams, "ss4k_frvsr_upscale_streams: output buffer too small");
    if (up->cut && up->cut->on()) scene_cut_round(up, in, slots, n_streams, h, w, out, (hipStream_t)stream);
    else up->u.round(in, slots, n_streams, h, w, out, (hipStream_t)stream);
  });
}
int ss4k_frvsr_upscale_streams_at(ss4k_frvsr_upscaler* up, const int32_t* slots, int n_streams, const uint8_t* const* in, int h, int w, uint8_t* const* out,
                                  size_t frame_cap, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up, "ss4k_frvsr_upscale_streams_at: NULL argument");
    SS4K_REQUIRE(n_streams >= 1 && n_streams <= (int)up->u.slots.size(), "ss4k_frvsr_upscale_streams_at: n_streams must be in 1..max_streams");
    SS4K_REQUIRE(slots && in && out, "ss4k_frvsr_upscale_streams_at: NULL argument");
    SS4K_REQUIRE(h > 0 && w > 0, "ss4k_frvsr_upscale_streams_at: empty frames");
    int oh, ow; up->u.out_shape(&oh, &ow);
    SS4K_REQUIRE(frame_cap >= (size_t)oh * ow * 3, "ss4k_frvsr_upscale_streams_at: output frames too small");
    if (up->cut && up->cut->on()) scene_cut_round_at(up, in, slots, n_streams, h, w, out, (hipStream_t)stream);
    else up->u.round_at(in, slots, n_streams, h, w, out, (hipStream_t)stream);
  });
}
int ss4k_frvsr_upscaler_enable_taps(ss4k_frvsr_upscaler* up, int en) {
  if (!up) return SS4K_EINVAL;
  up->u.taps_on = en != 0;
  if (!en) std::memset(up->u.tap_dims, 0, sizeof(up->u.tap_dims));
  return SS4K_OK;
}
int ss4k_frvsr_upscaler_read_tap(ss4k_frvsr_upscaler* up, int which, float* out, size_t cap, int dims[4], void* stream) {
  return guard([&] {
    SS4K_REQUIRE(up && which >= 0 && which < 4 && dims, "bad tap request");
    FrvsrUpscaler& u = up->u;
    const int* d = u.tap_dims[which];
    for (int i = 0; i < 4; ++i) dims[i] = d[i];
    const size_t nflt = (size_t)d[0] * d[1] * d[2] * d[3];
    SS4K_REQUIRE(nflt > 0, "tap not recorded (enable taps before ss4k_frvsr_upscale_frames)");
    if (out) {
      SS4K_REQUIRE(cap >= nflt, "tap buffer too small");
      const FrvsrUpscaler::Slot& sl = u.slots[(size_t)u.tap_slot];   // the last item of the last round: its slot's state, its part of the round's batches
      const void* src = which == 0 ? sl.lr[sl.cur].ptr : which == 1 ? (const void*)(u.m->flow.as<float>() + u.tap_item * nflt)
                      : which == 2 ? (const void*)(u.m->tap_s2d.as<float>() + u.tap_item * nflt) : sl.hr[sl.cur].ptr;
      SS4K_HIP(hipMemcpyAsync(out, src, nflt * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
  });
}
int ss4k_op_backward_warp(ss4k_ctx* c, const float* x, const float* flow, float* out, int n, int ch, int h, int w, void* s) {
  return guard([&] { SS4K_REQUIRE(c && x && flow && out, "NULL argument"); op_backward_warp(x, flow, out, n, ch, h, w, (hipStream_t)s); });
}
int ss4k_op_bicubic_upsample4(ss4k_ctx* c, const float* in, float* out, int p, int h, int w, void* s) {
  return guard([&] { SS4K_REQUIRE(c && in && out, "NULL argument"); op_bicubic_upsample4(in, out, p, h, w, (hipStream_t)s); });
}


// ---- profiling hooks --------------------------------------------------------------------------
static void prof_collect(ss4k_ctx* c) {
  for (auto& e : c->prof_events) {
    SS4K_HIP(hipEventSynchronize(e.b));
    float ms = 0; SS4K_HIP(hipEventElapsedTime(&ms, e.a, e.b));
    const int k = e.kind >= 0 && e.kind < PROF_KINDS ? e.kind : 0;
    c->kind_ms[k] += ms; c->kind_flops[k] += e.flops; c->kind_launches[k] += 1;
    if (k == PROF_CONV) { c->prof_ms += ms; c->prof_flops += e.flops; c->prof_launches += 1; }
    if (e.family) { auto& f = c->prof_families[e.family]; f.launches += 1; f.ms += ms; f.flops += e.flops; }
    c->prof_pool.push_back(e);
  }
  c->prof_events.clear();
  for (auto& e : c->prof_sections) {
    SS4K_HIP(hipEventSynchronize(e.b));
    float ms = 0; SS4K_HIP(hipEventElapsedTime(&ms, e.a, e.b));
    c->prof_section_ms += ms;
    c->prof_pool.push_back(e);
  }
  c->prof_sections.clear();
}
int ss4k_stream_pair_check(ss4k_ctx* c, void* a, void* b, int* side_by_side) {
  return guard([&] {
    SS4K_REQUIRE(c && side_by_side, "ss4k_stream_pair_check: NULL argument");
    SS4K_REQUIRE(a != b, "ss4k_stream_pair_check: the same stream twice");
    SS4K_HIP(hipSetDevice(c->device));
    *side_by_side = stream_pair_ok((hipStream_t)a, (hipStream_t)b) ? 1 : 0;
  });
}
int ss4k_prof_enable(ss4k_ctx* c, int en) { if (!c) return SS4K_EINVAL; c->prof = en != 0; return SS4K_OK; }
int ss4k_prof_reset(ss4k_ctx* c) {
  return guard([&] { SS4K_REQUIRE(c, "NULL ctx"); prof_collect(c); c->prof_ms = 0; c->prof_section_ms = 0; c->prof_flops = 0; c->prof_launches = 0;
    c->prof_families.clear();
    for (int k = 0; k < PROF_KINDS; ++k) { c->kind_ms[k] = 0; c->kind_flops[k] = 0; c->kind_launches[k] = 0; } });
}
int ss4k_prof_read_family(ss4k_ctx* c, int index, char* name, size_t name_capacity, int64_t* launches, double* ms, double* flops) {
  return guard([&] {
    SS4K_REQUIRE(c && index >= 0 && name && name_capacity > 0, "ss4k_prof_read_family: bad argument");
    prof_collect(c);
    SS4K_REQUIRE((size_t)index < c->prof_families.size(), "ss4k_prof_read_family: index past the last family");
    auto it = c->prof_families.begin();
    std::advance(it, index);
    std::snprintf(name, name_capacity, "%s", it->first.c_str());
    if (launches) *launches = it->second.launches;
    if (ms) *ms = it->second.ms;
    if (flops) *flops = it->second.flops;
  });
}
int ss4k_prof_read(ss4k_ctx* c, int64_t* launches, double* ms, double* flops) {
  return guard([&] {
    SS4K_REQUIRE(c, "NULL ctx");
    prof_collect(c);
    if (launches) *launches = c->prof_launches;
    if (ms) *ms = c->prof_ms;
    if (flops) *flops = c->prof_flops;
  });
}
int ss4k_prof_read_kind(ss4k_ctx* c, int kind, int64_t* launches, double* ms, double* flops) {
  return guard([&] {
    SS4K_REQUIRE(c && kind >= 0 && kind < PROF_KINDS, "ss4k_prof_read_kind: bad argument");
    prof_collect(c);
    if (launches) *launches = c->kind_launches[kind];
    if (ms) *ms = c->kind_ms[kind];
    if (flops) *flops = c->kind_flops[kind];
  });
}
int ss4k_prof_read_section_ms(ss4k_ctx* c, double* section_ms) {
  return guard([&] {
    SS4K_REQUIRE(c && section_ms, "NULL argument");
    prof_collect(c);
    *section_ms = c->prof_section_ms;
  });
}

}  // extern "C"
