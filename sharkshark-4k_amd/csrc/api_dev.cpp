// libss4k_hip_dev.so only (include/ss4k_dev.h): the conv bench, thin wrappers of the glue launchers the public ss4k_op_* set does not
// reach, the route report, and guard mode.  The product build compiles this file to an empty object.
#ifdef SS4K_DEV
#include "api_guard.h"
#include "frvsr.h"
#include "host_tables.h"
#include "upscaler.h"
#include "upscaler_temporal.h"
#include <mutex>
#include <type_traits>

// ---- guard mode (include/ss4k_dev.h; DevBuf in common.h) -----------------------------------------
namespace ss4k { namespace guardmode {
namespace {
struct Live { size_t need, total; };
struct Damage { bool back, freed; size_t need; long long first, last; };   // offsets relative to the payload
std::mutex g_mu;
bool g_on = false;
std::map<char*, Live> g_live;          // by base pointer
std::set<void*> g_unguarded;
std::vector<Damage> g_sticky;          // damage found when a buffer was freed or re-grown

// bytes != 0xFF in [dev, dev + n): (first, last) index or (-1, -1)
bool scan_bytes(const char* dev, size_t n, long long* first, long long* last) {
  std::vector<unsigned char> h(n);
  if (hipMemcpy(h.data(), dev, n, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); *first = 0; *last = (long long)n - 1; return true; }
  *first = *last = -1;
  for (size_t i = 0; i < n; ++i) if (h[i] != 0xFF) { if (*first < 0) *first = (long long)i; *last = (long long)i; }
  return *first >= 0;
}
void scan(char* base, const Live& e, bool freed, std::vector<Damage>& out) {
  long long a, b;
  if (scan_bytes(base, RZ, &a, &b)) out.push_back({false, freed, e.need, a - (long long)RZ, b - (long long)RZ});
  const size_t back = e.total - RZ - e.need;
  if (scan_bytes(base + RZ + e.need, back, &a, &b)) out.push_back({true, freed, e.need, (long long)e.need + a, (long long)e.need + b});
}
std::string describe(const Damage& d) {
  char t[256];
  std::snprintf(t, sizeof(t), "%s red zone of a %zu-byte buffer%s: first damaged byte at payload offset %lld, last at %lld",
                d.back ? "back" : "front", d.need, d.freed ? " (since freed)" : "", d.first, d.last);
  return t;
}
}  // namespace

bool on() { std::lock_guard<std::mutex> l(g_mu); return g_on; }
void note_unguarded(void* p, bool live) {
  std::lock_guard<std::mutex> l(g_mu);
  if (live) g_unguarded.insert(p); else g_unguarded.erase(p);
}
void* alloc(size_t need) {
  const size_t total = (RZ + need + RZ + 255) & ~size_t(255);
  void* base = nullptr;
  SS4K_HIP(hipMalloc(&base, total));
  hipError_t e = hipMemset(base, 0xFF, total);
  if (e == hipSuccess) e = hipDeviceSynchronize();   // the fill is complete before any stream (the non-blocking lane stream too) can use the buffer
  if (e != hipSuccess) { (void)hipFree(base); throw Error(SS4K_EHIP, std::string("guard fill: ") + hipGetErrorString(e)); }
  std::lock_guard<std::mutex> l(g_mu);
  g_live[static_cast<char*>(base)] = Live{need, total};
  return static_cast<char*>(base) + RZ;
}
void free_guarded(void* payload) {
  char* base = static_cast<char*>(payload) - RZ;
  (void)hipDeviceSynchronize();
  std::lock_guard<std::mutex> l(g_mu);
  auto it = g_live.find(base);
  if (it != g_live.end()) { scan(base, it->second, true, g_sticky); g_live.erase(it); }
  (void)hipFree(base);
}
}  // namespace guardmode

static void poison_one(DevBuf& b, int* n, size_t* bytes, size_t* bytes256) {
  if (!b.ptr || !b.transient) return;
  SS4K_HIP(hipMemset(b.ptr, 0xFF, b.bytes));
  *n += 1; *bytes += b.bytes; *bytes256 += (b.bytes + 255) & ~size_t(255);
}
}  // namespace ss4k

using namespace ss4k;

// a by-value pointer table (frvsr.h) filled from a HOST array of n device pointers
template <typename Tab, typename P> static Tab dev_items(P* const* host, int n) {
  Tab t{};
  for (int i = 0; i < n; ++i) t.p[i] = const_cast<std::remove_reference_t<decltype(t.p[0])>>(host[i]);
  return t;
}

extern "C" {
int ss4k_bench_conv(ss4k_ctx* c, int dtype, int cin0, int cin1, int cout, int n, int h, int w, int flags, int iters,
                    double* avg_us, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(c && avg_us && iters > 0, "bad argument");
    *avg_us = bench_conv_layer(c, dtype, cin0, cin1, cout, n, h, w, flags, iters, (hipStream_t)stream);
  });
}

// ---- the glue launchers the public ss4k_op_* set does not reach, or reaches with fixed arguments (include/ss4k_dev.h).  Thin: every
// pointer is the caller's device memory, *_half selects the __half instantiation
#define SS4K_DEV_OP(cond, ...) return guard([&] { SS4K_REQUIRE(cond, "NULL or out-of-range argument"); __VA_ARGS__; SS4K_HIP(hipGetLastError()); })
// ... the launch written once for T = __half (`half` set) and T = float
#define SS4K_DEV_HALF(half, ...) if (half) { using T = __half; __VA_ARGS__; } else { using T = float; __VA_ARGS__; }
int ss4k_dev_op_area_normalized(ss4k_ctx* c, const void* in, int in_half, float* out, int p, int h, int w, int oh, int ow, const float* st_hr,
                                const float* st_lr, void* s) {
  SS4K_DEV_OP(c && in && out && st_hr && st_lr, SS4K_DEV_HALF(in_half, op_area_normalized((const T*)in, out, p, h, w, oh, ow, st_hr, st_lr, (hipStream_t)s)));
}
int ss4k_dev_op_tail_fused(ss4k_ctx* c, void* hr, int hr_half, uint8_t* out_u8, const float* diff, int n, int ch, int h, int w, int dh, int dw,
                           const float* st_hr, const float* st_lr, void* s) {
  SS4K_DEV_OP(c && hr && (st_hr == nullptr) == (st_lr == nullptr),
              SS4K_DEV_HALF(hr_half, op_tail_fused((T*)hr, out_u8, diff, n, ch, h, w, dh, dw, st_hr, st_lr, (hipStream_t)s)));
}
int ss4k_dev_op_bicubic_u8(ss4k_ctx* c, const void* in, int in_half, uint8_t* out, int n, int ch, int h, int w, int oh, int ow, void* s) {
  SS4K_DEV_OP(c && in && out, SS4K_DEV_HALF(in_half, op_bicubic_u8((const T*)in, out, n, ch, h, w, oh, ow, (hipStream_t)s)));
}
int ss4k_dev_op_bicubic(ss4k_ctx* c, const float* in, float* out, int p, int h, int w, int oh, int ow, int clamp01, void* s) {
  SS4K_DEV_OP(c && in && out, op_bicubic(in, out, p, h, w, oh, ow, clamp01, (hipStream_t)s));
}
int ss4k_dev_op_bilinear(ss4k_ctx* c, const float* in, float* out, int p, int h, int w, int oh, int ow, int subtract_from_out, int clamp01, void* s) {
  SS4K_DEV_OP(c && in && out, op_bilinear(in, out, p, h, w, oh, ow, subtract_from_out, clamp01, (hipStream_t)s));
}
int ss4k_dev_gauss17_taps(float* taps17) {
  return guard([&] { SS4K_REQUIRE(taps17, "NULL argument"); const auto g = gaussian_taps_1d(17, 8.0f); std::memcpy(taps17, g.data(), 17 * 4); });
}
int ss4k_dev_op_gauss17_reflect(ss4k_ctx* c, const float* in, float* tmp, float* out, const float* taps17_dev, int p, int h, int w, void* s) {
  SS4K_DEV_OP(c && in && tmp && out && taps17_dev, op_gauss17_reflect(in, tmp, out, taps17_dev, p, h, w, (hipStream_t)s));
}
int ss4k_dev_op_depthwise_reflect(ss4k_ctx* c, const float* in, float* out, const float* taps_dev, int p, int h, int w, int k, int clamp01,
                                  const float* blend_src, float blend_a, float blend_b, void* s) {
  SS4K_DEV_OP(c && in && out && taps_dev, op_depthwise_reflect(in, out, taps_dev, p, h, w, k, clamp01, blend_src, blend_a, blend_b, (hipStream_t)s));
}
int ss4k_dev_op_normalize(ss4k_ctx* c, float* x, const float* st_hr, const float* st_lr, int p, int hw, void* s) {
  SS4K_DEV_OP(c && x && st_hr && st_lr, op_normalize(x, st_hr, st_lr, p, hw, (hipStream_t)s));
}
int ss4k_dev_op_sub(ss4k_ctx* c, const float* a, const float* b, float* out, size_t n, void* s) {
  SS4K_DEV_OP(c && a && b && out, op_sub(a, b, out, n, (hipStream_t)s));
}
int ss4k_dev_op_clamp01(ss4k_ctx* c, float* x, size_t n, void* s) { SS4K_DEV_OP(c && x, op_clamp01(x, n, (hipStream_t)s)); }
int ss4k_dev_op_plane_stats(ss4k_ctx* c, double* acc, const void* in, int in_half, float* stats, int p, int hw, void* s) {
  SS4K_DEV_OP(c && acc && in && stats, SS4K_DEV_HALF(in_half, op_plane_stats(acc, (const T*)in, stats, p, hw, (hipStream_t)s)));
}
int ss4k_dev_op_plane_stats_u8nhwc(ss4k_ctx* c, double* acc, const uint8_t* in, float* stats, int n, int hw, void* s) {
  SS4K_DEV_OP(c && acc && in && stats, op_plane_stats_u8nhwc(acc, in, stats, n, hw, (hipStream_t)s));
}
int ss4k_dev_op_plane_stats_partial(ss4k_ctx* c, double* acc, const void* in, int in_half, int p, int hw, int acc_planes, int plane0, void* s) {
  SS4K_DEV_OP(c && acc && in && plane0 >= 0 && p > 0 && plane0 + p <= acc_planes,
              SS4K_DEV_HALF(in_half, op_plane_stats_partial(acc, (const T*)in, p, hw, acc_planes, plane0, (hipStream_t)s)));
}
int ss4k_dev_op_plane_stats_u8nhwc_partial(ss4k_ctx* c, double* acc, const uint8_t* in, int n, int hw, int acc_planes, int plane0, void* s) {
  SS4K_DEV_OP(c && acc && in && plane0 >= 0 && n > 0 && plane0 + 3 * n <= acc_planes,
              op_plane_stats_u8nhwc_partial(acc, in, n, hw, acc_planes, plane0, (hipStream_t)s));
}
int ss4k_dev_op_plane_stats_finish(ss4k_ctx* c, const double* acc, float* stats, int p, int hw, void* s) {
  SS4K_DEV_OP(c && acc && stats, op_plane_stats_finish(acc, stats, p, hw, (hipStream_t)s));
}
int ss4k_dev_op_plane_stats_finish2(ss4k_ctx* c, double* acc, float* stats_a, float* stats_b, int p, int hw_a, int hw_b, int rezero, void* s) {
  SS4K_DEV_OP(c && acc && stats_a && stats_b, op_plane_stats_finish2(acc, stats_a, stats_b, p, hw_a, hw_b, rezero != 0, (hipStream_t)s));
}
int ss4k_dev_op_ps_nchw_addbase(ss4k_ctx* c, const void* src, int src_half, void* out, int out_half, const float* base, int n, int h, int w, int r,
                                int cq, double* stats_acc, void* s) {
  SS4K_DEV_OP(c && src && out && base,
              SS4K_REQUIRE(src_half || !out_half, "pixel shuffle tail: an fp16 output needs fp16 planes");
              if (!src_half) op_ps_nchw_addbase((const float*)src, (float*)out, base, n, h, w, r, cq, stats_acc, (hipStream_t)s);
              else if (!out_half) op_ps_nchw_addbase((const __half*)src, (float*)out, base, n, h, w, r, cq, stats_acc, (hipStream_t)s);
              else op_ps_nchw_addbase((const __half*)src, (__half*)out, base, n, h, w, r, cq, stats_acc, (hipStream_t)s));
}
int ss4k_dev_op_pack_input(ss4k_ctx* c, const float* in, void* out, int out_half, int n, int ch, int h, int w, int r, int nplanes, void* s) {
  SS4K_DEV_OP(c && in && out, SS4K_DEV_HALF(out_half, op_pack_input(in, (T*)out, n, ch, h, w, r, nplanes, (hipStream_t)s)));
}
int ss4k_dev_op_temporal_shift(ss4k_ctx* c, const void* in, void* out, int nplanes, int frames, size_t frame_px, int slots_per_record,
                               int ch_per_plane, int fold, void* s) {
  SS4K_DEV_OP(c && in && out && slots_per_record > 0 && ch_per_plane >= slots_per_record, op_temporal_shift(in, out, nplanes, frames, frame_px, slots_per_record, ch_per_plane, fold, (hipStream_t)s));
}
// ---- the launchers of csrc/frvsr.hip that the public API reaches only through a whole step or round (tests/test_gpu_frvsr_glue_budget.py).
// The _items forms take HOST arrays of n device pointers and fill the by-value tables the kernels receive
#define SS4K_DEV_ITEMS(n) ((n) > 0 && (n) <= SS4K_FRVSR_MAX_STREAMS)
int ss4k_dev_op_frvsr_maxpool2_planes(ss4k_ctx* c, const void* in, void* out, int half, int nplanes, int n, int h, int w, void* s) {
  SS4K_DEV_OP(c && in && out, SS4K_DEV_HALF(half, op_maxpool2_planes((const T*)in, (T*)out, nplanes, n, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsr_bilinear2_planes(ss4k_ctx* c, const void* in, void* out, int half, int nplanes, int n, int h, int w, void* s) {
  SS4K_DEV_OP(c && in && out, SS4K_DEV_HALF(half, op_bilinear2_planes((const T*)in, (T*)out, nplanes, n, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsr_flow_finish(ss4k_ctx* c, const float* raw, float* flow, int n, int h8, int w8, int h, int w, void* s) {
  SS4K_DEV_OP(c && raw && flow, op_flow_finish(raw, flow, n, h8, w8, h, w, (hipStream_t)s));
}
int ss4k_dev_op_frvsr_warp_s2d_planes(ss4k_ctx* c, const float* lr_flow, const float* hr_prev, void* out, int half, int n, int h, int w, void* s) {
  SS4K_DEV_OP(c && lr_flow && hr_prev && out, SS4K_DEV_HALF(half, op_warp_s2d_planes(lr_flow, hr_prev, (T*)out, n, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsr_warp_s2d_planes_items(ss4k_ctx* c, const float* lr_flow, const float* const* hr_prev, void* out, int half, int n, int h, int w,
                                            void* s) {
  SS4K_DEV_OP(c && lr_flow && hr_prev && out && SS4K_DEV_ITEMS(n),
              const FrvsrPtrs t = dev_items<FrvsrPtrs>(hr_prev, n);
              SS4K_DEV_HALF(half, op_warp_s2d_planes_items(lr_flow, t, (T*)out, n, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsr_ps4_conv_tail(ss4k_ctx* c, const void* in, int half, const float* wb, float* out, int n, int h, int w, void* s) {
  SS4K_DEV_OP(c && in && wb && out, SS4K_DEV_HALF(half, op_ps4_conv_tail((const T*)in, wb, out, n, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsr_ps4_conv_tail_items(ss4k_ctx* c, const void* in, int half, const float* wb, float* const* out, int n, int h, int w, void* s) {
  SS4K_DEV_OP(c && in && wb && out && SS4K_DEV_ITEMS(n),
              const FrvsrPtrs t = dev_items<FrvsrPtrs>(out, n);
              SS4K_DEV_HALF(half, op_ps4_conv_tail_items((const T*)in, wb, t, n, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsr_planes_to_nchw(ss4k_ctx* c, const void* in, int half, float* out, int n, int channels, int h, int w, void* s) {
  SS4K_DEV_OP(c && in && out && n > 0 && channels > 0 && h > 0 && w > 0, SS4K_DEV_HALF(half, op_planes_to_nchw((const T*)in, out, n, channels, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsr_clamp01_to(ss4k_ctx* c, const float* in, float* out, size_t n, void* s) {
  SS4K_DEV_OP(c && in && out && n > 0, op_clamp01_to(in, out, n, (hipStream_t)s));
}
int ss4k_dev_op_frvsr_frames_in_items(ss4k_ctx* c, const uint8_t* const* in, float* const* lr_curr, int n, int h, int w, int lh, int lw, void* s) {
  SS4K_DEV_OP(c && in && lr_curr && SS4K_DEV_ITEMS(n),
              op_frames_in_items(dev_items<FrvsrFramesIn>(in, n), dev_items<FrvsrPtrs>(lr_curr, n), n, h, w, lh, lw, (hipStream_t)s));
}
int ss4k_dev_op_frvsr_pack_lr_items(ss4k_ctx* c, const float* const* lr_curr, const float* const* lr_prev, void* a, void* b, int half, int n, int h, int w,
                                    void* s) {
  SS4K_DEV_OP(c && lr_curr && lr_prev && a && b && SS4K_DEV_ITEMS(n),
              const FrvsrPtrs tc = dev_items<FrvsrPtrs>(lr_curr, n); const FrvsrPtrs tp = dev_items<FrvsrPtrs>(lr_prev, n);
              SS4K_DEV_HALF(half, op_pack_lr_items(tc, tp, (T*)a, (T*)b, n, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsr_frames_out_items(ss4k_ctx* c, const float* const* hr, uint8_t* const* out, int n, int H, int W, int oh, int ow, void* s) {
  SS4K_DEV_OP(c && hr && out && SS4K_DEV_ITEMS(n),
              op_frames_out_items(dev_items<FrvsrPtrs>(hr, n), dev_items<FrvsrFramesOut>(out, n), n, H, W, oh, ow, (hipStream_t)s));
}
// ---- the launchers of csrc/frvsr_bi.hip (degradation 'BI'; tests/test_gpu_frvsr_bi_glue_budget.py)
int ss4k_dev_op_frvsrbi_bilinear_upsample4(ss4k_ctx* c, const float* in, float* out, int p, int h, int w, void* s) {
  SS4K_DEV_OP(c && in && out, op_bilinear_upsample4(in, out, p, h, w, (hipStream_t)s));
}
int ss4k_dev_op_frvsrbi_warp_s2d_planes(ss4k_ctx* c, const float* lr_flow, const float* hr_prev, void* out, int half, int n, int h, int w, void* s) {
  SS4K_DEV_OP(c && lr_flow && hr_prev && out, SS4K_DEV_HALF(half, op_warp_s2d_bi_planes(lr_flow, hr_prev, (T*)out, n, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsrbi_warp_s2d_planes_items(ss4k_ctx* c, const float* lr_flow, const float* const* hr_prev, void* out, int half, int n, int h, int w,
                                               void* s) {
  SS4K_DEV_OP(c && lr_flow && hr_prev && out && SS4K_DEV_ITEMS(n),
              const FrvsrPtrs t = dev_items<FrvsrPtrs>(hr_prev, n);
              SS4K_DEV_HALF(half, op_warp_s2d_bi_planes_items(lr_flow, t, (T*)out, n, h, w, (hipStream_t)s)));
}
int ss4k_dev_op_frvsrbi_bilinear4_add(ss4k_ctx* c, const float* conv, const float* lr, float* out, int n, int h, int w, void* s) {
  SS4K_DEV_OP(c && conv && lr && out, op_bilinear4_add(conv, lr, out, n, h, w, (hipStream_t)s));
}
int ss4k_dev_op_frvsrbi_bilinear4_add_items(ss4k_ctx* c, const float* conv, const float* const* lr, float* const* out, int n, int h, int w, void* s) {
  SS4K_DEV_OP(c && conv && lr && out && SS4K_DEV_ITEMS(n),
              op_bilinear4_add_items(conv, dev_items<FrvsrPtrs>(lr, n), dev_items<FrvsrPtrs>(out, n), n, h, w, (hipStream_t)s));
}
#undef SS4K_DEV_ITEMS
#undef SS4K_DEV_HALF
#undef SS4K_DEV_OP
// Frvsr::step on a contiguous batch with keep_taps set, and EVERY item's padded flow and warped space-to-depth tensor copied out next to hr_out
// (the public taps describe only the last item of a round): what tests/test_gpu_frvsr_budget.py holds FNet and SRNet to, each on its own
int ss4k_dev_frvsr_step_taps(ss4k_frvsr* m, const float* lr_curr, const float* lr_prev, const float* hr_prev, float* hr_out, float* flow_out,
                             float* s2d_out, int n, int h, int w, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(m && lr_curr && lr_prev && hr_prev && hr_out && flow_out && s2d_out, "ss4k_dev_frvsr_step_taps: NULL argument");
    Frvsr& f = m->f;
    const bool was = f.keep_taps;
    f.keep_taps = true;
    try { f.step(lr_curr, lr_prev, hr_prev, hr_out, n, h, w, (hipStream_t)stream); } catch (...) { f.keep_taps = was; throw; }
    f.keep_taps = was;
    const size_t px = (size_t)n * h * w;
    SS4K_HIP(hipMemcpyAsync(flow_out, f.flow.ptr, px * 2 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    SS4K_HIP(hipMemcpyAsync(s2d_out, f.tap_s2d.ptr, px * 48 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  });
}
// TecoGAN's tail alone (frvsr_teco.cpp) on a chosen body tensor, both transposed layers' outputs copied out (tests/test_gpu_tecogan_tail.py)
int ss4k_dev_frvsr_tail_taps(ss4k_frvsr* m, const float* body_nchw, const float* lr_curr, float* up1_out, float* up2_out, float* hr_out, int n, int h,
                             int w, int max_workgroups, int group_items, void* stream) {
  return guard([&] {
    SS4K_REQUIRE(m && body_nchw && lr_curr && up1_out && up2_out && hr_out, "ss4k_dev_frvsr_tail_taps: NULL argument");
    TecoTailDev o; o.max_workgroups = max_workgroups; o.group_items = group_items;
    m->f.tecogan_tail_taps(body_nchw, lr_curr, up1_out, up2_out, hr_out, n, h, w, o, (hipStream_t)stream);
  });
}
// host only: W_eq + biases of embed_convt for one transposed layer (nf * nf * 9 + nf floats in, 4 nf * nf * 9 + 4 nf out)
int ss4k_dev_frvsr_embed_convt(const float* wt_and_bias, int nf, float* out, size_t capacity_floats) {
  return guard([&] {
    SS4K_REQUIRE(wt_and_bias && out && nf > 0 && nf <= SS4K_DESC_MAX_WIDTH, "ss4k_dev_frvsr_embed_convt: bad argument");
    const std::vector<float> eq = embed_convt(wt_and_bias, nf);
    SS4K_REQUIRE(capacity_floats >= eq.size(), "ss4k_dev_frvsr_embed_convt: output too small");
    std::copy(eq.begin(), eq.end(), out);
  });
}
// host only: pack_convt3x3s2's blob for one transposed layer's Wt (64, 64, 3, 3) in dtype SS4K_F32 | SS4K_F16 (73 728 | 147 456 bytes)
int ss4k_dev_frvsr_pack_convt(const float* wt, int dtype, void* out, size_t capacity_bytes) {
  return guard([&] {
    SS4K_REQUIRE(wt && out && (dtype == SS4K_F32 || dtype == SS4K_F16), "ss4k_dev_frvsr_pack_convt: bad argument");
    const std::vector<uint8_t> pk = pack_convt3x3s2(wt, dtype);
    SS4K_REQUIRE(capacity_bytes >= pk.size(), "ss4k_dev_frvsr_pack_convt: output too small");
    std::copy(pk.begin(), pk.end(), static_cast<uint8_t*>(out));
  });
}
// ---- stream ordering (tests/test_gpu_lane_order.py, tests/test_gpu_host_io_order.py): a bounded delay on any stream, and the frame lanes'
// handicap, counters and positive control (the state lives in ss4k_ctx and Model; Model::launch_lanes / lanes_begin / lanes_join read it)
int ss4k_dev_op_spin(ss4k_ctx* c, unsigned ticks, void* s) {
  return guard([&] { SS4K_REQUIRE(c, "ss4k_dev_op_spin: NULL ctx"); op_lane_spin(ticks, (hipStream_t)s); SS4K_HIP(hipGetLastError()); });
}
int ss4k_dev_lane_handicap(ss4k_ctx* c, int lane, unsigned ticks) {
  return guard([&] {
    SS4K_REQUIRE(c && (lane == 0 || lane == 1), "ss4k_dev_lane_handicap: lane is 0 (the caller's stream) or 1 (the lane stream)");
    c->dev_handicap_lane = lane; c->dev_handicap_ticks = ticks;
  });
}
int ss4k_dev_lane_counts(ss4k_ctx* c, int64_t* forks, int64_t* joins, int64_t* spins) {
  return guard([&] {
    SS4K_REQUIRE(c && forks && joins && spins, "ss4k_dev_lane_counts: NULL argument");
    *forks = c->dev_lane_forks; *joins = c->dev_lane_joins; *spins = c->dev_lane_spins;
  });
}
int ss4k_dev_lane_counts_reset(ss4k_ctx* c) {
  return guard([&] { SS4K_REQUIRE(c, "ss4k_dev_lane_counts_reset: NULL ctx"); c->dev_lane_forks = c->dev_lane_joins = c->dev_lane_spins = 0; });
}
int ss4k_dev_lane_drop_join(ss4k_ctx* c, int k) {
  return guard([&] { SS4K_REQUIRE(c && k >= 0, "ss4k_dev_lane_drop_join: bad argument"); c->dev_drop_join = k; });
}

int ss4k_dev_glue_routes_reset(void) { return guard([&] { glue_routes_reset(); }); }
int ss4k_dev_glue_routes_read(int index, char* name, size_t name_capacity, int64_t* launches) {
  return guard([&] {
    SS4K_REQUIRE(index >= 0 && name && name_capacity > 0 && launches, "ss4k_dev_glue_routes_read: bad argument");
    std::string nm;
    SS4K_REQUIRE(glue_routes_read(index, &nm, launches), "ss4k_dev_glue_routes_read: index past the last route");
    std::snprintf(name, name_capacity, "%s", nm.c_str());
  });
}

// ---- guard mode ----------------------------------------------------------------------------------
int ss4k_dev_guard_enable(int on_) {
  std::lock_guard<std::mutex> l(ss4k::guardmode::g_mu);
  ss4k::guardmode::g_on = on_ != 0;
  return SS4K_OK;
}
int ss4k_dev_guard_check(int* guarded, int* unguarded, int* damaged, char* text, size_t text_capacity) {
  return guard([&] {
    using namespace ss4k::guardmode;
    SS4K_REQUIRE(guarded && unguarded && damaged, "ss4k_dev_guard_check: NULL argument");
    SS4K_HIP(hipDeviceSynchronize());
    std::lock_guard<std::mutex> l(g_mu);
    std::vector<Damage> found = g_sticky;
    for (auto& kv : g_live) scan(kv.first, kv.second, false, found);
    *guarded = (int)g_live.size(); *unguarded = (int)g_unguarded.size(); *damaged = (int)found.size();
    if (text && text_capacity) std::snprintf(text, text_capacity, "%s", found.empty() ? "" : describe(found[0]).c_str());
  });
}
int ss4k_dev_guard_poison(ss4k_ctx* c, ss4k_model* m, ss4k_upscaler* up, int* buffers, size_t* bytes, size_t* bytes_256) {
  return guard([&] {
    SS4K_REQUIRE(buffers && bytes && bytes_256, "ss4k_dev_guard_poison: NULL argument");
    *buffers = 0; *bytes = 0; *bytes_256 = 0;
    SS4K_HIP(hipDeviceSynchronize());
    if (c) for (auto& kv : c->scratch) poison_one(kv.second, buffers, bytes, bytes_256);
    if (m) for (auto& b : m->m.acts) poison_one(b, buffers, bytes, bytes_256);
    if (up) up->u.for_each_job_buf([&](DevBuf& b) { poison_one(b, buffers, bytes, bytes_256); });
    SS4K_HIP(hipDeviceSynchronize());
  });
}
int ss4k_dev_guard_poison_frvsr(ss4k_frvsr* m, ss4k_frvsr_upscaler* up, int* buffers, size_t* bytes, size_t* bytes_256) {
  return guard([&] {
    SS4K_REQUIRE(buffers && bytes && bytes_256, "ss4k_dev_guard_poison_frvsr: NULL argument");
    *buffers = 0; *bytes = 0; *bytes_256 = 0;
    SS4K_HIP(hipDeviceSynchronize());
    if (m) {
      for (auto& b : m->f.net.acts) poison_one(b, buffers, bytes, bytes_256);
      for (DevBuf* b : {&m->f.flow_raw, &m->f.flow, &m->f.tap_s2d}) poison_one(*b, buffers, bytes, bytes_256);
    }
    if (up) for (DevBuf* b : {&up->u.img, &up->u.hrc, &up->u.outf}) poison_one(*b, buffers, bytes, bytes_256);
    SS4K_HIP(hipDeviceSynchronize());
  });
}
int ss4k_dev_guard_poison_temporal(ss4k_upscaler_temporal* up, int* buffers, size_t* bytes, size_t* bytes_256) {
  return guard([&] {
    SS4K_REQUIRE(up && buffers && bytes && bytes_256, "ss4k_dev_guard_poison_temporal: NULL argument");
    *buffers = 0; *bytes = 0; *bytes_256 = 0;
    SS4K_HIP(hipDeviceSynchronize());
    up->t.up.for_each_job_buf([&](DevBuf& b) { poison_one(b, buffers, bytes, bytes_256); });
    for (DevBuf* b : {&up->t.lr4, &up->t.den, &up->t.den_flush, &up->t.lrk, &up->t.blend}) poison_one(*b, buffers, bytes, bytes_256);
    SS4K_HIP(hipDeviceSynchronize());
  });
}
int ss4k_dev_guard_selftest(ss4k_ctx* c) {
  return guard([&] {
    using namespace ss4k::guardmode;
    SS4K_REQUIRE(c, "ss4k_dev_guard_selftest: NULL ctx");
    SS4K_HIP(hipSetDevice(c->device));
    int g0 = 0, u0 = 0, d0 = 0, g1 = 0, u1 = 0, d1 = 0;
    char text[256];
    SS4K_REQUIRE(ss4k_dev_guard_check(&g0, &u0, &d0, nullptr, 0) == SS4K_OK, "guard selftest: the check itself failed");
    SS4K_REQUIRE(d0 == 0, "guard selftest: damage is already on record (run the selftest first)");
    const size_t need = 1000;   // not a multiple of 256: the back zone must start at the requested size
    bool was_on;
    { std::lock_guard<std::mutex> l(g_mu); was_on = g_on; g_on = true; }
    DevBuf b;
    try { b.ensure(need); } catch (...) { std::lock_guard<std::mutex> l(g_mu); g_on = was_on; throw; }
    { std::lock_guard<std::mutex> l(g_mu); g_on = was_on; }
    SS4K_REQUIRE(b.guarded && b.bytes == need, "guard selftest: the buffer was not allocated in guard mode");
    SS4K_HIP(hipMemset(b.as<char>() - 1, 0, 1));        // last byte of the front red zone
    SS4K_HIP(hipMemset(b.as<char>() + need, 0, 1));     // first byte of the back red zone
    const int rc = ss4k_dev_guard_check(&g1, &u1, &d1, text, sizeof(text));
    std::vector<Damage> mine;
    { std::lock_guard<std::mutex> l(g_mu); scan(b.as<char>() - RZ, g_live.at(b.as<char>() - RZ), false, mine); }
    b.release();
    size_t sticky;
    { std::lock_guard<std::mutex> l(g_mu); sticky = g_sticky.size(); g_sticky.clear(); }
    SS4K_REQUIRE(rc == SS4K_OK, "guard selftest: the check failed after the two writes");
    SS4K_REQUIRE(g1 == g0 + 1 && u1 == u0 && d1 == 2, "guard selftest: the check did not report exactly the two damaged zones");
    SS4K_REQUIRE(std::string(text).find("front") != std::string::npos && std::string(text).find("offset -1,") != std::string::npos,
                 "guard selftest: the text does not name the front zone's byte at offset -1");
    SS4K_REQUIRE(mine.size() == 2 && !mine[0].back && mine[0].first == -1 && mine[0].last == -1 && mine[1].back &&
                     mine[1].first == (long long)need && mine[1].last == (long long)need && mine[0].need == need,
                 "guard selftest: wrong zones or offsets");
    SS4K_REQUIRE(sticky == 2, "guard selftest: the release did not keep the two damaged zones on record");
  });
}
}  // extern "C"
#endif  // SS4K_DEV
