// EGVSR's frame-recurrent upscaler (FRNet x4, reference src/upscale/model/egvsr/egvsr.py:146-212): the executor behind ss4k_frvsr and
// the service path behind ss4k_frvsr_upscaler (include/ss4k.h), and the launchers of the glue kernels they need (frvsr.hip, frvsr_bi.hip).  One
// Frvsr holds all four (generator, degradation) variants: Frvsr::run branches on `degradation` for the warp stage's launcher and on `generator`
// for the tail (TecoGAN's: frvsr_teco.cpp, conv_up2.hip).  The stages that differ by degradation or addressing alone are one kernel template each
// (frvsr_stages.h); the launchers declared here name its instantiations.
#pragma once
#include "models.h"
#include <memory>

namespace ss4k {

struct SceneCut;

// Base pointers of the items of a batched launch whose tensors are NOT one contiguous batch: stream i's hr_prev / hr_curr, (3, 4 h, 4 w) fp32,
// each in its own allocation.  Passed BY VALUE in the kernel arguments (512 B): no device table, no upload, no synchronisation, and the
// buffers stay separate DevBufs (a red zone around each in the dev library's guard mode).  Entries past the launch's n are not read.
struct FrvsrPtrs { float* p[SS4K_FRVSR_MAX_STREAMS]; };
// ... and of a scattered round's frames (ss4k_frvsr_upscale_streams_at): item i's input and output frame, uint8 HWC, any byte alignment
struct FrvsrFramesIn { const uint8_t* p[SS4K_FRVSR_MAX_STREAMS]; };
struct FrvsrFramesOut { uint8_t* p[SS4K_FRVSR_MAX_STREAMS]; };

// ---- launchers (frvsr.hip).  "planes" tensors are the conv kernels' layout: [plane][pixel][16 channels of T] -----------------------------
// nn.MaxPool2d(2, 2) (egvsr.py:24,31,38): (n, h, w) -> (n, h / 2, w / 2), odd sizes floored
template <typename T> void op_maxpool2_planes(const T* in, T* out, int nplanes, int n, int h, int w, hipStream_t st);
// F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) (egvsr.py:70-75): (n, h, w) -> (n, 2 h, 2 w)
template <typename T> void op_bilinear2_planes(const T* in, T* out, int nplanes, int n, int h, int w, hipStream_t st);
// tanh(raw) * 24 (egvsr.py:76) and F.pad(..., (0, pad_w, 0, pad_h), 'reflect') (:191-194): (n, 2, h8, w8) -> (n, 2, h, w), fp32
void op_flow_finish(const float* raw, float* flow, int n, int h8, int w8, int h, int w, hipStream_t st);
// BicubicUpsample(4) (utils/net_utils.py:112-165): (planes, h, w) -> (planes, 4 h, 4 w), fp32
void op_bicubic_upsample4(const float* in, float* out, int planes, int h, int w, hipStream_t st);
// backward_warp (utils/net_utils.py:50-93): x (n, c, h, w), flow (n, 2, h, w) -> (n, c, h, w), fp32
void op_backward_warp(const float* x, const float* flow, float* out, int n, int c, int h, int w, hipStream_t st);
// 4 * BicubicUpsample(4)(lr_flow), backward_warp(hr_prev, .) and the space-to-depth of egvsr.py:196-208 as one launch: lr_flow (n, 2, h, w),
// hr_prev (n, 3, 4 h, 4 w), both fp32 -> three planes of T (channel (sy * 4 + sx) * 3 + c)
template <typename T> void op_warp_s2d_planes(const float* lr_flow, const float* hr_prev, T* out, int n, int h, int w, hipStream_t st);
// ... item i reading hr_prev.p[i] instead of hr_prev + i * 3 * 16 h w: the same kernel template on the other addressing, bit-identical; n <= 64
template <typename T> void op_warp_s2d_planes_items(const float* lr_flow, const FrvsrPtrs& hr_prev, T* out, int n, int h, int w, hipStream_t st);
// PixelShuffle(4), ReLU, Conv2d(4, 3, 3, 1, 1) (egvsr.py:122-127,139-140): four planes of T (64 channels) at (n, h, w) -> fp32 NCHW
// (n, 3, 4 h, 4 w); wb: 108 weights (OIHW) + 3 biases on the device
template <typename T> void op_ps4_conv_tail(const T* in, const float* wb, float* out, int n, int h, int w, hipStream_t st);
// ... item i written to out.p[i] (3, 4 h, 4 w): bit-identical; n <= 64
template <typename T> void op_ps4_conv_tail_items(const T* in, const float* wb, const FrvsrPtrs& out, int n, int h, int w, hipStream_t st);
// conv + BicubicUpsample(4)(lr) (TecoGAN's SRNet, degradation 'BD': tecogan_nets.py:146-148): conv (n, 3, 4 h, 4 w) and lr (n, 3, h, w) fp32 ->
// out (n, 3, 4 h, 4 w) fp32; the skip goes through op_bicubic_upsample4's device functions, so it is that op bit for bit
void op_bicubic4_add(const float* conv, const float* lr, float* out, int n, int h, int w, hipStream_t st);
// ... item i reading lr.p[i] (3, h, w) and writing out.p[i] (3, 4 h, 4 w); conv stays one contiguous batch: bit-identical; n <= 64
void op_bicubic4_add_items(const float* conv, const FrvsrPtrs& lr, const FrvsrPtrs& out, int n, int h, int w, hipStream_t st);
// ---- launchers of degradation 'BI' (frvsr_bi.hip): the same kernel templates with get_upsampling_func's F.interpolate(scale_factor=4, 'bilinear',
// align_corners=False) (utils/net_utils.py:96-108) in the places of BicubicUpsample(4)
// (planes, h, w) -> (planes, 4 h, 4 w), fp32
void op_bilinear_upsample4(const float* in, float* out, int planes, int h, int w, hipStream_t st);
// op_warp_s2d_planes[_items] with 4 * bilinear x4 of the flow: the same warp, the same records, the same requirements and grid
template <typename T> void op_warp_s2d_bi_planes(const float* lr_flow, const float* hr_prev, T* out, int n, int h, int w, hipStream_t st);
template <typename T> void op_warp_s2d_bi_planes_items(const float* lr_flow, const FrvsrPtrs& hr_prev, T* out, int n, int h, int w, hipStream_t st);
// op_bicubic4_add[_items] with the bilinear skip: op_bilinear_upsample4's value bit for bit, then one rounded add
void op_bilinear4_add(const float* conv, const float* lr, float* out, int n, int h, int w, hipStream_t st);
void op_bilinear4_add_items(const float* conv, const FrvsrPtrs& lr, const FrvsrPtrs& out, int n, int h, int w, hipStream_t st);
// planes of T -> fp32 NCHW (n, channels, h, w) (the parity taps)
template <typename T> void op_planes_to_nchw(const T* in, float* out, int n, int channels, int h, int w, hipStream_t st);
// clamp(x, 0, 1) into another tensor (egvsr_upscaler.py:209: the recurrent state keeps the unclamped one)
void op_clamp01_to(const float* in, float* out, size_t n, hipStream_t st);

// ---- the glue of a scattered round: ONE launch each for all n items, bit-identical to the per-item chains of FrvsrUpscaler::round ---------
// item i: uint8 HWC (h, w, 3) at in.p[i] -> / 255 -> area to (lh, lw) when the sizes differ -> fp32 (3, lh, lw) at lr_curr.p[i]
// (op_u8nhwc_to_f32nchw [+ op_area] of glue.hip, every window route of it)
void op_frames_in_items(const FrvsrFramesIn& in, const FrvsrPtrs& lr_curr, int n, int h, int w, int lh, int lw, hipStream_t st);
// item i's lr_curr.p[i] / lr_prev.p[i] (3, h, w) fp32 -> item i's run of the single planes a / b (op_pack_input<T> with r = 1, c = 3, one plane)
template <typename T> void op_pack_lr_items(const FrvsrPtrs& lr_curr, const FrvsrPtrs& lr_prev, T* a, T* b, int n, int h, int w, hipStream_t st);
// item i: hr.p[i] (3, H, W) fp32, left untouched -> clamp to [0, 1] -> area to (oh, ow) when the sizes differ -> clamp, * 255 truncated ->
// uint8 HWC (oh, ow, 3) at out.p[i] (op_clamp01_to + op_area + op_f32nchw_to_u8nhwc, or the last alone); no fp32 intermediate in memory
void op_frames_out_items(const FrvsrPtrs& hr, const FrvsrFramesOut& out, int n, int H, int W, int oh, int ow, hipStream_t st);

// 0 for a description, a generator or a degradation that is refused.  generator: SS4K_FRVSR_EGVSR | SS4K_FRVSR_TECOGAN, degradation:
// SS4K_FRVSR_BD | SS4K_FRVSR_BI (include/ss4k.h).  'BI': the two 16-scalar `kernels` buffers are not in the state_dict
size_t frvsr_param_count(const ss4k_frvsr_desc& d, int generator = SS4K_FRVSR_EGVSR, int degradation = SS4K_FRVSR_BD);

// stages of a step, for the per-stage event timing (ss4k_frvsr_prof_read)
// (7..9 are TecoGAN's tail: its two transposed convolutions, conv_out, the bicubic skip; FRV_TAIL is EGVSR's tail alone)
enum { FRV_FNET_CONV = 0, FRV_SRNET_CONV = 1, FRV_POOL_UP = 2, FRV_FLOW = 3, FRV_WARP = 4, FRV_TAIL = 5, FRV_GLUE = 6, FRV_CONVT = 7, FRV_CONV_OUT = 8,
       FRV_SKIP = 9, FRV_STAGES = 10 };

// ---- conv_up2.hip: ConvTranspose2d(64, 64, 3, 2, 1, output_padding=1) + bias + ReLU on planes, (N, H, W) -> (N, 2 H, 2 W), by output phase
constexpr int CONVT_TH = 8, CONVT_TW = 32;   // input pixels per workgroup tile
struct ConvtArgs {
  const char* in; size_t in_plane_bytes;     // four planes (64 channels) at (N, H, W)
  char* out; size_t out_plane_bytes;         // four planes at (N, 2 H, 2 W)
  const char* w;                             // pack_convt3x3s2's blob (pack.cpp)
  const float* bias;                         // 64
  int N, H, W, tiles_x, tiles_y;             // (the launcher fills the tile counts)
};
// max_workgroups > 0 caps the persistent grid (dev: a walk of more tiles than workgroups at small shapes)
void launch_convt3x3s2(ss4k_ctx* ctx, const ConvtArgs& a, int dtype, int max_workgroups, hipStream_t st);

// W_eq (4 nf, nf, 3, 3) OIHW + 4 nf biases: the transposed layer (Wt (nf, nf, 3, 3) + nf biases) as a pad-1 3x3 convolution + PixelShuffle(2)
std::vector<float> embed_convt(const float* wt_and_bias, int nf);
// dev library: the tail alone on a chosen body tensor (n, nf, h, w) fp32 NCHW, with both transposed layers' outputs copied out as fp32 NCHW
// (up1 (n, nf, 2 h, 2 w), up2 (n, nf, 4 h, 4 w)).  group_items: items per group of the tail's walk (0 = default); max_workgroups: a cap
// on the phase kernel's grid (launch_convt3x3s2; the embedded route has no grid of its own: accepted and unused)
struct TecoTailDev { float* up1 = nullptr; float* up2 = nullptr; int group_items = 0, max_workgroups = 0; };
// TecoGAN's tail (frvsr_teco.cpp: Frvsr::build_teco_tail / run_teco_tail); unused by EGVSR
struct TecoTail {
  bool embedded = true;                         // the transposed layers' route (route_flags; unpinned: embedded, the faster one as measured)
  int up_layer[2] = {-1, -1}, out_layer = -1;   // embedded route: the W_eq layers of net; conv_out
  DevBuf up_w[2], up_b[2];                      // phase route: pack_convt3x3s2's blob and the 64 biases
  TecoTailDev dev{};
};

// `body` with T = __half or float by a model's dtype, so that a planes launcher is named once per call site
#define SS4K_PLANES_T(dtype, ...) do { if ((dtype) == SS4K_F16) { using T = __half; __VA_ARGS__; } else { using T = float; __VA_ARGS__; } } while (0)

struct Frvsr {
  ss4k_ctx* ctx = nullptr;
  ss4k_frvsr_desc desc{};
  int generator = SS4K_FRVSR_EGVSR;     // | SS4K_FRVSR_TECOGAN: which tail follows SRNet's last residual block
  int degradation = SS4K_FRVSR_BD;      // | SS4K_FRVSR_BI: which x4 up-sampling the warp stage (and TecoGAN's skip) uses
  int route_flags = 0;                  // SS4K_FRVSR_CONVT_* (include/ss4k.h): TecoGAN only, at most one pin
  TecoTail teco;
  Model net;                 // container of the conv layers and the activation workspaces (Model::conv / Model::act)
  DevBuf tail_wb;            // EGVSR's srnet.conv_out: 108 weights + 3 biases, fp32
  DevBuf flow_raw, flow;     // fp32 in both dtypes
  int fnet0 = 0, srnet0 = 0; // first layer of each network in net.layers
  bool keep_taps = false;    // step() leaves copies for the service's parity taps
  DevBuf tap_s2d;            // fp32 NCHW (n, 48, h, w)
  // per-stage timing with events on the caller's stream (off by default)
  bool prof = false;
  struct Span { hipEvent_t a, b; int stage; };
  std::vector<Span> spans;
  double stage_ms[FRV_STAGES] = {};
  void prof_collect();
  // body() as one span of stage `s` on `st` (nothing is recorded while the timing is off or the step only plans)
  template <typename F> void timed(int s, hipStream_t st, F&& body) {
    if (!prof || net.plan_only) { body(); return; }
    Span sp{nullptr, nullptr, s};
    SS4K_HIP(hipEventCreate(&sp.a));
    if (hipEventCreate(&sp.b) != hipSuccess) { (void)hipEventDestroy(sp.a); throw Error(SS4K_EHIP, "hipEventCreate failed"); }
    spans.push_back(sp);
    SS4K_HIP(hipEventRecord(sp.a, st));
    body();
    SS4K_HIP(hipEventRecord(sp.b, st));
  }
  ~Frvsr();

  // validates (desc, generator, degradation, route_flags) and the blob size - the one place - then packs the weights
  void build(const float* w, size_t n);
  // FRNet.forward (egvsr.py:180-212)
  void step(const float* lr_curr, const float* lr_prev, const float* hr_prev, float* hr_out, int n, int h, int w, hipStream_t st);
  // the same step over n <= SS4K_FRVSR_MAX_STREAMS items that each live in buffers of their own (the service's streams): item i reads lr_curr[i],
  // lr_prev[i] (3, h, w) and hr_prev.p[i], writes hr_out.p[i].  Every conv, pool, x2, flow, warp and tail launch covers all n items; only the
  // input packing runs per item.  Bit-identical, item by item, to step() on a contiguous batch.
  // pack_batched: the items' lr_curr / lr_prev are packed by ONE launch (op_pack_lr_items) instead of two per item
  struct Items { const float* const* lr_curr; const float* const* lr_prev; const FrvsrPtrs* hr_prev; const FrvsrPtrs* hr_out; bool pack_batched = false; };
  void step_items(const Items& items, int n, int h, int w, hipStream_t st);
  size_t workspace_bytes(int n, int h, int w);
  // dev library: TecoGAN's tail alone (TecoTailDev above); refused on an EGVSR object
  void tecogan_tail_taps(const float* body_nchw, const float* lr_curr, float* up1, float* up2, float* hr_out, int n, int h, int w, const TecoTailDev& opts, hipStream_t st);
 private:
  void run(const float* lr_curr, const float* lr_prev, const float* hr_prev, float* hr_out, const Items* items, int n, int h, int w, hipStream_t st);
  // frvsr_teco.cpp.  build: srnet.conv_up.{0,2} as the state_dict holds them ((C_in, C_out, 3, 3) + bias each) and srnet.conv_out (OIHW + bias).
  // run: body is the last residual block's output, nf channels at (n, h, w); lr_curr / hr_out are the contiguous batches, or (items != null)
  // unused; slot is the first free activation slot of net.  Plans (net.plan_only) like every other part of a step
  void build_teco_tail(const float* up0, const float* up2, const float* out_w);
  void run_teco_tail(const Tens& body, int slot, const float* lr_curr, float* hr_out, const Items* items, int n, int h, int w, hipStream_t st);
};

struct FrvsrUpscaler {
  ss4k_ctx* ctx = nullptr;
  Frvsr* m = nullptr;
  int lr_h = 0, lr_w = 0, out_h = 0, out_w = 0;
  // one slot per stream: its own recurrent state, allocated on the slot's first frame
  struct Slot {
    bool have_state = false;
    int cur = 0;             // which of lr[2] / hr[2] holds the previous frame
    DevBuf lr[2], hr[2];
  };
  std::vector<Slot> slots;   // max_streams of them (ss4k_frvsr_upscaler_create_streams); slot 0 is the stream of frames()
  DevBuf img, hrc, outf;     // resize scratch, reused item after item (stream order)
  bool taps_on = false;      // read_tap copies from the live buffers of the LAST item of the last round: its slot's lr[cur] / hr[cur], m->flow, m->tap_s2d
  int tap_dims[4][4] = {};
  int tap_slot = 0, tap_item = 0;
  void out_shape(int* oh, int* ow) const;
  // one frame for each of S distinct slots, as one n = S step: in (S, h, w, 3) -> out (S, oh, ow, 3), in the order of `slot_ids`
  void round(const uint8_t* in, const int32_t* slot_ids, int S, int h, int w, uint8_t* out, hipStream_t st);
  // the same round with item i's frame at in[i] and its result at out[i] (host arrays of device pointers): three glue launches whatever S is
  void round_at(const uint8_t* const* in, const int32_t* slot_ids, int S, int h, int w, uint8_t* const* out, hipStream_t st);
  void frames(const uint8_t* in, int n, int h, int w, uint8_t* out, hipStream_t st);   // n consecutive frames of slot 0
  size_t state_bytes() const;
 private:
  friend struct SceneCut;   // (scene_cut.h: the detector makes a round's refusals - check_round - before its own launches, from outside)
  friend struct FrvsrTemporal;   // (frvsr_temporal.h: the chain with the online denoiser in front runs its waves as rounds, from outside)
  // a round's per-item pointers into the slots' state: lr_curr (= lr_dst, as a table), lr_prev, hr_prev, hr_curr
  struct RoundPtrs { const float* lr_curr[SS4K_FRVSR_MAX_STREAMS]; const float* lr_prev[SS4K_FRVSR_MAX_STREAMS]; FrvsrPtrs lr_dst, hr_prev, hr_curr; };
  // every refusal of a round, before any slot changes; area_chain: the round resizes with op_area (round), not inside the frame kernels (round_at)
  void check_round(const int32_t* slot_ids, int S, int h, int w, bool area_chain) const;
  void open_slots(const int32_t* slot_ids, int S, hipStream_t st, RoundPtrs& r);
  void close_slots(const int32_t* slot_ids, int S);
};

}  // namespace ss4k

struct ss4k_frvsr { ss4k::Frvsr f; };
// the scene-cut detector (scene_cut.h, api_scene_cut.cpp) lives beside the upscaler, not in it: null until ss4k_frvsr_upscaler_set_scene_cut
struct ss4k_frvsr_upscaler { ss4k::FrvsrUpscaler u; ss4k::SceneCut* cut = nullptr; ~ss4k_frvsr_upscaler(); };
