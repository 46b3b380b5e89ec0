/*
 * ss4k_dev.h - measurement-only entry points of libss4k_hip_dev.so (built with -DSS4K_DEV from the
 * same sources as libss4k_hip.so; a superset of include/ss4k.h).  Not part of the product library:
 * the instrumented / alternative-tile-shape instantiations of the conv kernel live only here.
 * Used by tools/stamp4.py, tools/traffic_ablate.py, tools/conv5_routes.py, tests/test_gpu_glue_budget.py,
 * tests/test_gpu_frvsr_glue_budget.py (the ss4k_dev_op_frvsr_* launchers), tests/test_gpu_frvsr_budget.py (ss4k_dev_frvsr_step_taps), tests/test_gpu_memory_hygiene.py (guard mode,
 * through tests/drive_guarded.py), tests/test_gpu_lane_order.py and tests/test_gpu_host_io_order.py (ss4k_dev_op_spin, ss4k_dev_lane_*).
 */
#ifndef SS4K_DEV_H
#define SS4K_DEV_H
#include "ss4k.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ss4k_model_desc.flags: both libraries accept exactly SS4K_MODEL_FLAGS_ALL (include/ss4k.h). */

/* Times ONE 3x3 conv layer (cin0 [+ cin1 concat] -> cout) in isolation on random operands: average
 * microseconds per launch over `iters` launches.
 * flags: 0 = the production kernel for that shape;
 *        32 (DBG_STAMP) = phase stamps (s_memtime per phase, printed to stderr), optionally combined with
 *        the timing-only ablations 1 (no output stores), 2 (every DMA reads one hot line), 16 (with 1:
 *        halo tiles from a 2 MB L2-resident window) - results are garbage in those builds;
 *        | shape_id << 8 selects another compiled tile shape (conv_mfma.hip, launch_conv3x3);
 *        | 2048 makes it conv5 of an RDB (no activation, out = conv * 0.2 + x).
 * Bits 4096 and 8192 (the removed register-stationary kernel) are rejected with SS4K_EINVAL. */
int ss4k_bench_conv(ss4k_ctx* ctx, int dtype, int cin0, int cin1, int cout, int n, int h, int w, int flags,
                    int iters, double* avg_us, void* hip_stream);

/* ---- glue launchers (csrc/glue.hip) that the public ss4k_op_* calls do not reach, or reach with fixed arguments: what
 * tests/test_gpu_glue_budget.py bounds against float64.  Conventions of the ss4k_op_* set: SS4K_OK or an error code with
 * ss4k_last_error(), every pointer is device memory of the caller (except taps17 of ss4k_dev_gauss17_taps), asynchronous
 * on hip_stream.  *_half != 0: that tensor holds __half, otherwise float.  Statistics accumulators `acc` hold
 * 32 (slots) x planes x 2 doubles; st_hr / st_lr / stats hold {mean, std} per plane. */
int ss4k_dev_op_area_normalized(ss4k_ctx* ctx, const void* in, int in_half, float* out, int planes, int h, int w, int oh,
                                int ow, const float* st_hr, const float* st_lr, void* hip_stream);
/* st_hr + st_lr (normalise), diff (dh x dw map, bilinear, subtracted) and out_u8 (uint8 NHWC result; NULL: clamped in place) may be NULL */
int ss4k_dev_op_tail_fused(ss4k_ctx* ctx, void* hr, int hr_half, uint8_t* out_u8, const float* diff, int n, int c, int h,
                           int w, int dh, int dw, const float* st_hr, const float* st_lr, void* hip_stream);
int ss4k_dev_op_bicubic_u8(ss4k_ctx* ctx, const void* in, int in_half, uint8_t* out, int n, int c, int h, int w, int oh,
                           int ow, void* hip_stream);
int ss4k_dev_op_bicubic(ss4k_ctx* ctx, const float* in, float* out, int planes, int h, int w, int oh, int ow, int clamp01,
                        void* hip_stream);
int ss4k_dev_op_bilinear(ss4k_ctx* ctx, const float* in, float* out, int planes, int h, int w, int oh, int ow,
                         int subtract_from_out, int clamp01, void* hip_stream);
/* the 17 taps (host memory) an upscaler uploads for its colour-match blur */
int ss4k_dev_gauss17_taps(float* taps17);
int ss4k_dev_op_gauss17_reflect(ss4k_ctx* ctx, const float* in, float* tmp, float* out, const float* taps17_dev, int planes,
                                int h, int w, void* hip_stream);
/* k = 3 or 17, taps_dev: k x k; out = [clamp01] conv; with blend_src: out * blend_a + blend_b * blend_src */
int ss4k_dev_op_depthwise_reflect(ss4k_ctx* ctx, const float* in, float* out, const float* taps_dev, int planes, int h,
                                  int w, int k, int clamp01, const float* blend_src, float blend_a, float blend_b,
                                  void* hip_stream);
int ss4k_dev_op_normalize(ss4k_ctx* ctx, float* x, const float* st_hr, const float* st_lr, int planes, int hw, void* hip_stream);
int ss4k_dev_op_sub(ss4k_ctx* ctx, const float* a, const float* b, float* out, size_t n, void* hip_stream);
int ss4k_dev_op_clamp01(ss4k_ctx* ctx, float* x, size_t n, void* hip_stream);
int ss4k_dev_op_plane_stats(ss4k_ctx* ctx, double* acc, const void* in, int in_half, float* stats, int planes, int hw,
                            void* hip_stream);
int ss4k_dev_op_plane_stats_u8nhwc(ss4k_ctx* ctx, double* acc, const uint8_t* in, float* stats, int n, int hw, void* hip_stream);
/* the halves of the two above: partial sums into planes [plane0, plane0 + planes) of an accumulator of acc_planes planes (zeroed by
 * the caller, or by an earlier ss4k_dev_op_plane_stats_finish2 with rezero), then one finishing launch */
int ss4k_dev_op_plane_stats_partial(ss4k_ctx* ctx, double* acc, const void* in, int in_half, int planes, int hw,
                                    int acc_planes, int plane0, void* hip_stream);
int ss4k_dev_op_plane_stats_u8nhwc_partial(ss4k_ctx* ctx, double* acc, const uint8_t* in, int n, int hw, int acc_planes,
                                           int plane0, void* hip_stream);
int ss4k_dev_op_plane_stats_finish(ss4k_ctx* ctx, const double* acc, float* stats, int planes, int hw, void* hip_stream);
int ss4k_dev_op_plane_stats_finish2(ss4k_ctx* ctx, double* acc, float* stats_a, float* stats_b, int planes, int hw_a,
                                    int hw_b, int rezero, void* hip_stream);
/* src: "planes" layout (16-channel records), cq * r * r channels; stats_acc (may be NULL): the output's plane sums ride along */
int ss4k_dev_op_ps_nchw_addbase(ss4k_ctx* ctx, const void* src, int src_half, void* out, int out_half, const float* base,
                                int n, int h, int w, int r, int cq, double* stats_acc, void* hip_stream);
int ss4k_dev_op_pack_input(ss4k_ctx* ctx, const float* in, void* out, int out_half, int n, int c, int h, int w, int r,
                           int nplanes, void* hip_stream);
int ss4k_dev_op_temporal_shift(ss4k_ctx* ctx, const void* in, void* out, int nplanes, int frames, size_t frame_px,
                               int slots_per_record, int ch_per_plane, int fold, void* hip_stream);

/* ---- the two kernels of the online BSVD executor (csrc/bsvd_online.hip) on caller buffers; routes "bsvdo::...".  Both only select and copy
 * 16-byte slots of the planes layout.
 * shift: the ShiftConv input of `frames` output frames whose centres sit in slots slot0 .. slot0 + frames - 1 of `in` (in_frames frames per
 * plane): channels [0, fold) from the next slot, zeros for output frames i >= n_next; [fold, 2 fold) from the previous slot, zeros for i = 0
 * unless first_has_prev; the rest from the centre.  out: nplanes planes of `frames` frames.  SS4K_EINVAL where a read would leave `in`. */
int ss4k_dev_op_bsvd_online_shift(ss4k_ctx* ctx, const void* in, void* out, int nplanes, int in_frames, int slot0, int frames, size_t frame_px,
                                  int slots_per_record, int ch_per_plane, int fold, int first_has_prev, int n_next, void* hip_stream);
/* shift_cuts: the cut-aware build (include/ss4k.h: ss4k_bsvd_online_push_cuts).  flag_ring: ring_mask + 1 DEVICE words (ring_mask = 2^k - 1),
 * flag_ring[f & ring_mask] != 0: stream frame f starts a scene; f0: the stream frame of output frame 0.  The next group of output frame t is
 * also zeros where flag[f0 + t + 1] is set, the previous group where flag[f0 + t] is set.  Routes "bsvdo::shift_window_cuts<half|float>". */
int ss4k_dev_op_bsvd_online_shift_cuts(ss4k_ctx* ctx, const void* in, void* out, int nplanes, int in_frames, int slot0, int frames, size_t frame_px,
                                       int slots_per_record, int ch_per_plane, int fold, int first_has_prev, int n_next, const uint32_t* flag_ring,
                                       unsigned ring_mask, int f0, void* hip_stream);
/* noise_planes: channel 3 of each of the n (1..64) packed (4, plane_px) fp32 frames becomes level_start where flags[i] != 0 or (i == 0 and
 * stream_first), else level.  flags: n DEVICE words.  Route "bsvdo::noise_planes". */
int ss4k_dev_op_bsvd_noise_planes(ss4k_ctx* ctx, float* frames4, int n, size_t plane_px, const uint32_t* flags, int stream_first,
                                  float level_start, float level, void* hip_stream);
/* carry: ONE launch for `entries` (1..22) tensors, HOST arrays of one value per entry: in each of nplanes[i] planes, count[i] frames from frame
 * src_first[i] of src[i] (src_frames[i] frames per plane) to the front of dst[i] (dst_frames[i] frames per plane); frame_slots[i]: 16-byte
 * slots per frame.  SS4K_EINVAL where src[i] and dst[i] overlap or the move leaves either buffer. */
int ss4k_dev_op_bsvd_online_carry(ss4k_ctx* ctx, int entries, const void* const* src, void* const* dst, const int* nplanes, const int* src_frames,
                                  const int* dst_frames, const int* src_first, const int* count, const size_t* frame_slots, void* hip_stream);
/* ---- the kernel of a temporal round (csrc/temporal_round.hip) on caller buffers; routes "tround::gather_planes<3>" / "<4>".  src: k (1..64) HOST
 * entries, frame j's three fp32 planes (3 * plane_px floats, 16-byte aligned) -> dst (k, planes, plane_px) fp32, 16-byte aligned.  planes == 4:
 * plane 3 of frame j is level_start where bit j of start_bits is set or *flags[j] != 0 (flags: NULL, or k HOST entries of DEVICE words, each
 * may be NULL), level otherwise.  SS4K_EINVAL: k outside 1..64, planes not 3 or 4, a NULL or misaligned pointer, a source inside dst. */
int ss4k_dev_op_temporal_gather(ss4k_ctx* ctx, const float* const* src, const uint32_t* const* flags, int k, size_t plane_px, int planes,
                                uint64_t start_bits, float level_start, float level, float* dst, void* hip_stream);
/* ... with a level per frame, as a round of slots at different denoise rates launches it: levels holds k HOST floats, frame j's plane 3 is
 * levels[j] where the one above writes level.  Same routes, same refusals, and SS4K_EINVAL for NULL levels. */
int ss4k_dev_op_temporal_gather_levels(ss4k_ctx* ctx, const float* const* src, const uint32_t* const* flags, int k, size_t plane_px, int planes,
                                       uint64_t start_bits, float level_start, const float* levels, float* dst, void* hip_stream);
/* ... and the padded four-plane form of the frame-recurrent chain at an lr_shape that 4 does not divide; route "tround::gather_planes_pad".
 * src[j]: (3, lh, lw) fp32 at any 4-byte address -> dst (k, 4, ph, pw) fp32, 16-byte aligned, (ph, pw) = (lh, lw) rounded up to multiples of
 * 4: planes 0..2 padded at the bottom and on the right by 'reflect' (row y >= lh is row 2 (lh - 1) - y, columns likewise), plane 3 by the
 * rule above, over the whole (ph, pw).  SS4K_EINVAL before any launch: what the one above refuses, lh < 4 or lw < 4, 4 ph pw >= 2^31. */
int ss4k_dev_op_temporal_gather_pad(ss4k_ctx* ctx, const float* const* src, const uint32_t* const* flags, int k, int lh, int lw,
                                    uint64_t start_bits, float level_start, const float* levels, float* dst, void* hip_stream);
/* ... and the four-plane gathers with the motion-adaptive noise map (include/ss4k.h: SS4K_NOISE_MAP_MOTION); routes
 * "tround::gather_planes_motion" / "tround::gather_planes_motion_pad".  src, flags, k, start_bits, level_start, dst as above; (lh, lw) is the
 * frame's shape - the unpadded form needs lw divisible by 4 and 16-byte aligned frames, the padded form takes what _gather_pad takes.  prev: k
 * HOST entries, the three planes of the frame before frame j in its stream, aligned as src[j]; a NULL entry sets frame j's start bit (it gets
 * the constant level_start).  scales: k HOST floats, frame j's (float)(0.35 * rate).  Plane 3 of frame j is level_start where its start bit is
 * set or *flags[j] != 0, else min(max(10 B, 0), 0.1f) * scales[j] per pixel.  SS4K_EINVAL before any launch: what the forms above refuse, NULL
 * prev or scales, a misaligned previous frame or one that overlaps dst, lh < 2 or lw < 2. */
int ss4k_dev_op_temporal_gather_motion(ss4k_ctx* ctx, const float* const* src, const float* const* prev, const uint32_t* const* flags, int k,
                                       int lh, int lw, uint64_t start_bits, float level_start, const float* scales, float* dst, void* hip_stream);
int ss4k_dev_op_temporal_gather_motion_pad(ss4k_ctx* ctx, const float* const* src, const float* const* prev, const uint32_t* const* flags, int k,
                                           int lh, int lw, uint64_t start_bits, float level_start, const float* scales, float* dst,
                                           void* hip_stream);
/* the pixel tile a workgroup of those kernels takes (rows of the frame, columns of the padded width), and the nine fp32 taps they use, row-major */
int ss4k_dev_temporal_motion_tile(int* tile_h, int* tile_w);
int ss4k_dev_temporal_motion_taps(float* taps9);

/* ---- launchers of the frame-recurrent upscaler's glue (csrc/frvsr.hip, csrc/frvsr.h) that the public API reaches only inside a whole
 * step or round: what tests/test_gpu_frvsr_glue_budget.py bounds against float64.  Same conventions as above; their routes are reported
 * as "frvsr::...", and so are those of ss4k_op_bicubic_upsample4 / ss4k_op_backward_warp (include/ss4k.h) when called through this library.
 * "planes": [plane][pixel (n, y, x)][16 channels] of float, or of __half where `half` != 0.  The _items forms take HOST arrays of n
 * (1..64) device pointers, one per item, and pass them to the kernel by value. */
int ss4k_dev_op_frvsr_maxpool2_planes(ss4k_ctx* ctx, const void* in, void* out, int half, int nplanes, int n, int h, int w, void* hip_stream);
int ss4k_dev_op_frvsr_bilinear2_planes(ss4k_ctx* ctx, const void* in, void* out, int half, int nplanes, int n, int h, int w, void* hip_stream);
/* raw (n, 2, h8, w8) -> tanh * 24, reflect-padded on the right and at the bottom to (n, 2, h, w); h - h8, w - w8 in 0..7 */
int ss4k_dev_op_frvsr_flow_finish(ss4k_ctx* ctx, const float* raw, float* flow, int n, int h8, int w8, int h, int w, void* hip_stream);
/* lr_flow (n, 2, h, w), hr_prev (n, 3, 4 h, 4 w) [items: hr_prev[i] (3, 4 h, 4 w)] -> three planes at (n, h, w) */
int ss4k_dev_op_frvsr_warp_s2d_planes(ss4k_ctx* ctx, const float* lr_flow, const float* hr_prev, void* out, int half, int n, int h, int w,
                                      void* hip_stream);
int ss4k_dev_op_frvsr_warp_s2d_planes_items(ss4k_ctx* ctx, const float* lr_flow, const float* const* hr_prev, void* out, int half, int n,
                                            int h, int w, void* hip_stream);
/* four planes at (n, h, w), wb: 108 weights (OIHW) + 3 biases -> (n, 3, 4 h, 4 w) [items: out[i] (3, 4 h, 4 w)] */
int ss4k_dev_op_frvsr_ps4_conv_tail(ss4k_ctx* ctx, const void* in, int half, const float* wb, float* out, int n, int h, int w, void* hip_stream);
int ss4k_dev_op_frvsr_ps4_conv_tail_items(ss4k_ctx* ctx, const void* in, int half, const float* wb, float* const* out, int n, int h, int w,
                                          void* hip_stream);
int ss4k_dev_op_frvsr_planes_to_nchw(ss4k_ctx* ctx, const void* in, int half, float* out, int n, int channels, int h, int w, void* hip_stream);
int ss4k_dev_op_frvsr_clamp01_to(ss4k_ctx* ctx, const float* in, float* out, size_t n, void* hip_stream);
/* the three launches of a scattered round: in[i] uint8 (h, w, 3) -> lr_curr[i] (3, lh, lw); lr_curr[i] / lr_prev[i] (3, h, w) -> item i's
 * run of the single planes a / b; hr[i] (3, H, W) -> out[i] uint8 (oh, ow, 3), any byte alignment */
int ss4k_dev_op_frvsr_frames_in_items(ss4k_ctx* ctx, const uint8_t* const* in, float* const* lr_curr, int n, int h, int w, int lh, int lw,
                                      void* hip_stream);
int ss4k_dev_op_frvsr_pack_lr_items(ss4k_ctx* ctx, const float* const* lr_curr, const float* const* lr_prev, void* a, void* b, int half, int n,
                                    int h, int w, void* hip_stream);
int ss4k_dev_op_frvsr_frames_out_items(ss4k_ctx* ctx, const float* const* hr, uint8_t* const* out, int n, int H, int W, int oh, int ow,
                                       void* hip_stream);

/* ---- launchers of degradation 'BI' (csrc/frvsr_bi.hip): the twins of ss4k_op_bicubic_upsample4, ss4k_dev_op_frvsr_warp_s2d_planes[_items]
 * and of the bicubic skip of a TecoGAN tail, with F.interpolate(scale_factor=4, mode='bilinear', align_corners=False) as the up-sampling
 * function.  Same conventions; their routes are reported as "frvsr_bi::...".  What tests/test_gpu_frvsr_bi_glue_budget.py bounds.  (Their
 * prefix is ss4k_dev_op_frvsrbi_: the ss4k_dev_op_frvsr_ set is the twelve launchers of csrc/frvsr.hip, and a test counts them.) */
/* (planes, h, w) -> (planes, 4 h, 4 w), fp32 */
int ss4k_dev_op_frvsrbi_bilinear_upsample4(ss4k_ctx* ctx, const float* in, float* out, int planes, int h, int w, void* hip_stream);
int ss4k_dev_op_frvsrbi_warp_s2d_planes(ss4k_ctx* ctx, const float* lr_flow, const float* hr_prev, void* out, int half, int n, int h, int w,
                                         void* hip_stream);
int ss4k_dev_op_frvsrbi_warp_s2d_planes_items(ss4k_ctx* ctx, const float* lr_flow, const float* const* hr_prev, void* out, int half, int n,
                                               int h, int w, void* hip_stream);
/* conv (n, 3, 4 h, 4 w) + bilinear x4 of lr (n, 3, h, w) [items: lr[i] (3, h, w)] -> out (n, 3, 4 h, 4 w) [items: out[i]], fp32 */
int ss4k_dev_op_frvsrbi_bilinear4_add(ss4k_ctx* ctx, const float* conv, const float* lr, float* out, int n, int h, int w, void* hip_stream);
int ss4k_dev_op_frvsrbi_bilinear4_add_items(ss4k_ctx* ctx, const float* conv, const float* const* lr, float* const* out, int n, int h, int w,
                                          void* hip_stream);

/* ---- the glue kernel of the frame-recurrent chain with the online denoiser in front (csrc/frvsr_temporal.hip); route "frvt::denoised_in_items".
 * den / lr / dst: HOST arrays of n_items (1..64) device pointers, 3 planes of (h, w) fp32 each; taps_dev: nine DEVICE floats.  One launch:
 * dst[i] = 0.8 * clamp01(depthwise3x3_reflect(den[i], taps)) + 0.2 * lr[i], bit for bit ss4k_dev_op_depthwise_reflect (k = 3, clamp01,
 * blend 0.8f / (float)(1 - 0.8)) per item.  SS4K_EINVAL before any launch: n_items outside 1..64, h < 2 or w < 2, 3 h w >= 2^31, a NULL or
 * misaligned pointer, a destination inside its item's sources.  (Its prefix is ss4k_dev_op_frvsrt_, for the reason given at
 * ss4k_dev_op_frvsrbi_ below.) */
int ss4k_dev_op_frvsrt_denoised_in(ss4k_ctx* ctx, const float* const* den, const float* const* lr, float* const* dst, int n_items, int h, int w,
                                   const float* taps_dev, void* hip_stream);
/* ... on the top-left (h, w) of denoised planes of (ph, pw) >= (h, w); route "frvt::denoised_in_crop_items".  den[i]: 3 planes of (ph, pw),
 * lr[i] and dst[i]: 3 planes of (h, w).  Bit for bit the one above on a contiguous copy of the crop; nothing of den outside the crop is read.
 * SS4K_EINVAL before any launch: what the one above refuses, ph < h or pw < w, 3 ph pw >= 2^31; the overlap check takes den at (ph, pw). */
int ss4k_dev_op_frvsrt_denoised_in_crop(ss4k_ctx* ctx, const float* const* den, const float* const* lr, float* const* dst, int n_items, int h,
                                        int w, int ph, int pw, const float* taps_dev, void* hip_stream);
/* ... and the late reset of a scene cut; route "frvt::clear_flagged_items".  flag_ptrs / lr_ptrs / hr_ptrs: HOST arrays of n_items (1..64) device
 * pointers.  One launch: lr_ptrs[i] (lr_bytes) and hr_ptrs[i] (hr_bytes) become zero for every item whose flag pointer is not NULL and whose
 * 32-bit word is not 0; nothing else is written.  SS4K_EINVAL before any launch: n_items outside 1..64, a size that is 0 or no multiple of 4, a
 * NULL or not 16-byte aligned lr / hr of ANY item, a flag pointer that is not 4-byte aligned. */
int ss4k_dev_op_frvsrt_clear_flagged(ss4k_ctx* ctx, const uint32_t* const* flag_ptrs, void* const* lr_ptrs, void* const* hr_ptrs, int n_items,
                                     size_t lr_bytes, size_t hr_bytes, void* hip_stream);

/* ss4k_frvsr_step (include/ss4k.h) on a contiguous batch of n items, with the two tensors between FNet, the warp and SRNet copied out for
 * EVERY item: flow_out (n, 2, h, w) = the padded LR flow, s2d_out (n, 48, h, w) = the warped, space-to-depth hr_prev as SRNet's first conv read
 * it (an fp16 model: exactly the fp16 values), both fp32 device memory of the caller.  The public taps describe only the last item of a round.
 * What tests/test_gpu_frvsr_budget.py bounds FNet's and SRNet's convolutions with, each against float64 on its own. */
int ss4k_dev_frvsr_step_taps(ss4k_frvsr* m, const float* lr_curr, const float* lr_prev, const float* hr_prev, float* hr_out, float* flow_out,
                             float* s2d_out, int n, int h, int w, void* hip_stream);

/* The tail of a TecoGAN generator (ss4k_frvsr_create_as, SS4K_FRVSR_TECOGAN) alone: body_nchw (n, 64, h, w) fp32 stands for the last residual
 * block's output and is packed into the model's dtype; lr_curr (n, 3, h, w).  Next to hr_out (n, 3, 4 h, 4 w) it returns both transposed
 * layers' outputs after ReLU as fp32 NCHW: up1_out (n, 64, 2 h, 2 w), up2_out (n, 64, 4 h, 4 w) (an fp16 model: exactly its fp16 values).
 * group_items: items per group of the tail's walk (0 = the default: as many as keep every HR plane below 2^32 bytes).  max_workgroups: a cap on
 * the grid of the phase kernel (0 = none); the embedded route has no grid of its own and ignores it.  SS4K_EINVAL on an EGVSR object. */
int ss4k_dev_frvsr_tail_taps(ss4k_frvsr* m, const float* body_nchw, const float* lr_curr, float* up1_out, float* up2_out, float* hr_out, int n, int h,
                             int w, int max_workgroups, int group_items, void* hip_stream);
/* Host only: one transposed layer's state_dict entries (Wt (nf, nf, 3, 3), then nf biases) as the pad-1 3x3 convolution + PixelShuffle(2) the
 * library runs: W_eq (4 nf, nf, 3, 3) OIHW, then 4 nf biases (csrc/frvsr_teco.cpp states the map) */
int ss4k_dev_frvsr_embed_convt(const float* wt_and_bias, int nf, float* out, size_t capacity_floats);
/* Host only: Wt (64, 64, 3, 3) in the fragment order of the phase kernel (csrc/conv_up2.hip states the map), in `dtype`: 36 864 values of
 * fp16 (73 728 bytes) or fp32 (147 456 bytes) */
int ss4k_dev_frvsr_pack_convt(const float* wt, int dtype, void* out, size_t capacity_bytes);

/* ---- stream ordering: what tests/test_gpu_lane_order.py and tests/test_gpu_host_io_order.py delay streams with, and the frame lanes'
 * (csrc/models.cpp: launch_lanes, lanes_begin, lanes_join, abort_forward) handicap, counters and positive control.  The state belongs
 * to the context; none of it exists in the product library. */
/* One idle wave that occupies hip_stream for `ticks` of the 100 MHz clock (op_lane_spin, csrc/glue.h); the kernel itself caps a launch at
 * 50 000 ticks = 0.5 ms: a longer delay is several launches. */
int ss4k_dev_op_spin(ss4k_ctx* ctx, unsigned ticks, void* hip_stream);
/* While ticks != 0, and only on the two-chain branch of launch_lanes, every launch pair is preceded by one spin of `ticks`: on the context's
 * lane stream (lane = 1: the second chain trails at every join) or on the caller's stream (lane = 0: the caller's chain trails at every
 * re-fork, i.e. after a join + op_temporal_shift).  ticks = 0 switches it off.  SS4K_EINVAL for another lane. */
int ss4k_dev_lane_handicap(ss4k_ctx* ctx, int lane, unsigned ticks);
/* forks: fork events recorded; joins: joins that made the caller's stream wait - lanes_join with a fork open, and abort_forward's join of a
 * forward that failed; spins: handicap spins launched.  Since the context was made or the last _reset. */
int ss4k_dev_lane_counts(ss4k_ctx* ctx, int64_t* forks, int64_t* joins, int64_t* spins);
int ss4k_dev_lane_counts_reset(ss4k_ctx* ctx);
/* Positive control: in the NEXT forward of a model of this context that may fork, the k-th (1-based) join that is not the end-of-forward
 * join records the lane's event but leaves the caller's hipStreamWaitEvent out (and is not counted in `joins`); the next launch re-forks as
 * usual.  k = 0 disarms.  The end-of-forward join and abort_forward are never skipped: when the call returns, the caller's stream is
 * ordered after every launch of both chains.  Honoured only when the forward repeats the (n, h, w) of the model's last completed forward -
 * every activation request then fits the buffer it finds, so nothing is allocated, re-grown or released between the dropped join and the
 * final one, and every access stays inside the buffers: the skipped wait only lets op_temporal_shift and the caller's chain read
 * activations before the second chain wrote them (wrong VALUES, never a fault).  Ignored (and disarmed) on any other shape. */
int ss4k_dev_lane_drop_join(ss4k_ctx* ctx, int k);

/* Route report: every glue launcher counts the kernel route it chose under a static name ("glue::area_whole<NORM,8,half>", ...).
 * _read returns the index-th route in name order (SS4K_EINVAL past the last), _reset clears the table.  Process-wide. */
int ss4k_dev_glue_routes_reset(void);
int ss4k_dev_glue_routes_read(int index, char* name, size_t name_capacity, int64_t* launches);

/* ---- guard mode: red zones around, and 0xFF poison in, every device buffer the library allocates (csrc/common.h, DevBuf).
 * Process-wide, off by default.  With it on, an allocation of `need` bytes is 64 KiB + need + 64 KiB, all 0xFF (NaN in fp16 / fp32 /
 * fp64) when it is handed out, and the back red zone starts at the requested size, not at the 256-rounded one.  Nothing here makes a
 * kernel touch memory outside an allocation of the library. */
/* affects later allocations only; buffers that exist already stay as they are and are counted as "unguarded" */
int ss4k_dev_guard_enable(int on);
/* Synchronises the device, scans the red zones of every live guarded buffer and adds the damage recorded when buffers were freed or
 * re-grown (the sticky list).  guarded / unguarded: live buffers of each kind; damaged: zones with at least one byte != 0xFF; text
 * (may be NULL): the first damage - front or back, requested bytes, offsets of the first and last damaged byte relative to the payload. */
int ss4k_dev_guard_check(int* guarded, int* unguarded, int* damaged, char* text, size_t text_capacity);
/* Refills the payload of the TRANSIENT buffers of the objects given (each may be NULL) with 0xFF, after a synchronisation: a model's
 * activations, an upscaler's intermediates and taps, a context's named scratch other than the zero page and the cv-area tables.
 * buffers / bytes: what was filled; bytes_256: the same sizes, each rounded up to 256 (what the product library allocates for them). */
int ss4k_dev_guard_poison(ss4k_ctx* ctx, ss4k_model* model, ss4k_upscaler* upscaler, int* buffers, size_t* bytes, size_t* bytes_256);
/* ... the same for the frame-recurrent upscaler (include/ss4k.h, ss4k_frvsr_*; each may be NULL): the executor's activations, flow buffers
 * and tap, the service path's staging buffers.  The recurrent state (lr_prev / hr_prev) is NOT transient: the next frame is entitled to it. */
int ss4k_dev_guard_poison_frvsr(ss4k_frvsr* m, ss4k_frvsr_upscaler* up, int* buffers, size_t* bytes, size_t* bytes_256);
/* ... and for a temporal upscaler (ss4k_upscaler_temporal_*): the chain's intermediates and the job buffers its slots share (the packed denoiser
 * input, the denoised frames, the gathered LR planes, the blend).  What a slot owns - the denoiser's state, the ring, the detector - is state. */
int ss4k_dev_guard_poison_temporal(ss4k_upscaler_temporal* up, int* buffers, size_t* bytes, size_t* bytes_256);
/* ... and for the frame-recurrent chain with the denoiser in front (ss4k_frvsr_temporal_*): the packed denoiser input and the denoised frames.
 * What a slot owns - the denoiser's state, the ring, lr_prev / hr_prev - is state; the two models' activations are theirs (_poison, _poison_frvsr). */
int ss4k_dev_guard_poison_frvsr_temporal(ss4k_frvsr_temporal* up, int* buffers, size_t* bytes, size_t* bytes_256);
/* Positive control without a fault: allocates a guarded buffer, writes one byte at payload - 1 and one at payload + need with hipMemset
 * (both inside the allocation), requires the check to report exactly those two zones with those offsets, releases the buffer and clears
 * the sticky list.  SS4K_EINVAL with a text if the guard does not see them (or if damage was already on record: run it first). */
int ss4k_dev_guard_selftest(ss4k_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* SS4K_DEV_H */
