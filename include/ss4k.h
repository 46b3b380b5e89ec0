/*
 * ss4k.h — C ABI of libss4k_hip.so: the MI355X (gfx950) replacement for the arithmetic on
 * sharkshark-4k's per-frame upscale path (reference: src/upscale/, Python only).
 *
 * The reference has no C interface; every entry point below cites the Python call it replaces
 * (paths relative to the reference repo).  Conventions:
 *   - return 0 on success, a negative SS4K_E* code on failure; ss4k_last_error() gives the text
 *     (thread-local).  Nothing throws across this boundary.
 *   - *_dev pointers are device (HIP) pointers BORROWED from the caller (PyTorch owns the I/O
 *     tensors); the library owns weights and workspaces.
 *   - work is enqueued on the caller's stream (hipStream_t passed as void*; NULL = default
 *     stream) with no hidden synchronisation, like the reference's eager torch calls.  One
 *     exception, once per (ctx, stream): the first multi-frame fp16 forward from a stream tests
 *     that the ctx's second launch chain really runs beside it (~ 3 ms, the host waits for the
 *     stream once; see ss4k_stream_pair_check).
 *   - one ss4k_ctx per device; a ctx and its children are not thread-safe (the reference's
 *     worker is a single-threaded process loop, base_service.py:33-60).
 *   - a ctx and everything created from it (models, upscalers) is SINGLE-STREAM: a model reuses its
 *     activation workspace and an upscaler its staging buffers on every call, and the granular
 *     ss4k_op_* calls share small per-context scratch.  Calls that touch the same ctx must be
 *     enqueued on one stream (or be serialised by the caller with events); two services that
 *     should overlap on one GPU take one ctx each.  Matches the reference (one worker process,
 *     default stream, fsrcnn_upscaler.py:118-166).
 *   - there is no CPU fallback: without a HIP device ss4k_ctx_create fails.
 */
#ifndef SS4K_H
#define SS4K_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS4K_ABI_VERSION 3   /* 3: the register-stationary kernel and the cross-layer chain left the product library (dev library only): flag bits 8
                                 (NO_RS), 64 (NO_CHAIN), 128 (CHAIN), 2048 (DENSE) and 16384 (CONV5_RS) are no longer accepted;
                                 ss4k_prof_read_family, ss4k_stream_pair_check and ss4k_op_cv_area_* were added.  2: ss4k_model_desc.reserved[0] became the validated `flags` word */

enum { SS4K_OK = 0, SS4K_EINVAL = -22, SS4K_ENOMEM = -12, SS4K_EHIP = -5, SS4K_ENODEV = -19 };

typedef struct ss4k_ctx ss4k_ctx;
typedef struct ss4k_model ss4k_model;
typedef struct ss4k_upscaler ss4k_upscaler;

/* network families on the path */
enum ss4k_model_kind {
  SS4K_FSRCNN = 1,  /* model/fsrcnn/model.py:6-62 */
  SS4K_RRDBNET = 2, /* basicsr RRDBNet, instantiated realesrgan/factory.py:113-125 */
  SS4K_SRVGG = 3,   /* SRVGGNetCompact, realesrgan/factory.py:18-82 */
  SS4K_BSVD = 4     /* BSVD driven with F = 1, bsvd/model.py:467-588, fsrcnn_upscaler.py:277 */
};

/* arithmetic/storage type of activations and weights inside the network.
 * F32: fp32 storage, exact-fp32 MFMA (parity gate, rtol 1e-3 / atol 1e-4 vs PyTorch CPU).
 * F16: fp16 storage, fp32 accumulate (what RealESRGANer(half=True) + TensorRT fp16 does,
 *      realesrgan/factory.py:168,206-230).  FSRCNN with F16 (fsrcnn/factory.py:47-69 builds a TensorRT fp16 engine):
 *      fp16 operands and intermediates, fp32 accumulation, input and output planes stay fp32; FSRCNN with F32 is
 *      fp32-grade (hi/lo-split fp16 MFMA or, SS4K_MODEL_FS_EXACT, exact-fp32 kernels). */
enum ss4k_dtype { SS4K_F32 = 0, SS4K_F16 = 1 };

typedef struct ss4k_model_desc {
  int32_t kind;        /* ss4k_model_kind */
  int32_t dtype;       /* ss4k_dtype */
  int32_t scale;       /* FSRCNN: deconv stride 2|4; RRDBNet: 1|2|4; SRVGG: 2|4; BSVD: 1 */
  int32_t num_feat;    /* RRDBNet/SRVGG trunk width (64); multiple of 16 */
  int32_t num_block;   /* RRDBNet: #RRDB (23|6); SRVGG: num_conv (32|16) */
  int32_t num_grow_ch; /* RRDBNet growth (32) */
  int32_t bsvd_chns[3];/* BSVD U-Net widths (32,64,128) */
  int32_t bsvd_mid_ch; /* 32 */
  int32_t bsvd_interm_ch; /* 30 */
  int32_t bsvd_stream; /* 0: every frame of a forward call is independent - how the service drives BSVD
                          (F = 1, fsrcnn_upscaler.py:277); 1: the n frames of one ss4k_model_forward call are ONE
                          stream run through the bidirectional buffers (BSVD.forward, bsvd/model.py:515-580) */
  int32_t flags;       /* SS4K_MODEL_* bits below; 0 = defaults.  None of them changes what is computed beyond what its
                          comment says: they choose between kernels / schedules that the tests hold bit-identical (or, for
                          FS_EXACT, inside the path's tolerance), and exist so that a caller - and the parity tests - can
                          pin a route without environment variables */
  int32_t reserved[3];
} ss4k_model_desc;
/* Every channel width of a description (num_feat, num_grow_ch, bsvd_chns, bsvd_mid_ch) is positive and at most SS4K_DESC_MAX_WIDTH,
 * num_block at most SS4K_DESC_MAX_BLOCKS; anything else is refused with SS4K_EINVAL and a message that names the field. */
enum { SS4K_DESC_MAX_WIDTH = 512, SS4K_DESC_MAX_BLOCKS = 64 };

enum {
  /* --- what a deployment may want to choose ---------------------------------------------------------------------------------- */
  SS4K_MODEL_FS_EXACT = 1,      /* FSRCNN: exact-fp32 kernels for every stage instead of the fp16 hi/lo-split matrix-core
                                   stages (fp32-grade, ~1e-6 of the exact ones); also chosen automatically when the
                                   checkpoint's range does not fit the split: a value the matrix-core stages would receive
                                   >= 6e4 in magnitude - weights and biases after their PReLU scaling by (1 + s) / 2, the
                                   tail's weights and bias (Model::build, csrc/models.cpp) */
  SS4K_MODEL_ONE_CHAIN = 2,     /* a multi-frame job never runs as two concurrent launch chains (frame lanes) */
  SS4K_MODEL_TWO_CHAINS = 4,    /* ... always does (default: measured per shape over the first calls) */
  SS4K_MODEL_HR_F32 = 512,      /* fp16 SRVGG / fp16-mode FSRCNN on the service paths: keep the network's output tensor (x4 on 720p: 2880 x 5120 x 3
                                   per frame) in fp32; default: fp16 (half the bytes of the service's four passes over it; the uint8 frames
                                   differ by at most 1 LSB in a few per cent of the bytes - an fp16 model's own error is 30 dB above that) */
  SS4K_MODEL_NO_UPS_PRESUM = 8192, /* RRDBNet fp16: conv_up1 / conv_up2 (3x3 convs on a nearest-x2 up-sampled tensor) in the direct form.
                                   Default: two of the three input rows an output row reads are the same low-resolution row, so their two
                                   MFMAs per tap column run as one with the weight fragments added in fp16 (6 instead of 9 MFMAs per
                                   pixel): one more fp16 rounding of a weight sum, NOT bit-identical to the direct form */
  SS4K_MODEL_NO_W16 = 32768,    /* fp16 layers with 64-cout groups and an even number of 16-channel input planes (SRVGG body, RRDBNet conv5 / trunk /
                                   tail, BSVD) on the v_mfma_f32_32x32x16_f16 build of the tile (conv_dense.hip's wide kernel) instead of
                                   conv_w16.hip's v_mfma_f32_16x16x32_f16 build (default: the chip runs these layers at its power cap and holds
                                   a 10 % higher clock on that shape; SRVGG x4 720p + 12 %).  The two builds add the same products in a
                                   different order: results differ in the last bits, the accuracy against the oracle is the same */
  /* --- pins of a fallback route the library takes by itself for some shapes: BIT-IDENTICAL results, used by the parity tests -------- */
  SS4K_MODEL_TILE_ROWS_16 = 16, /* 32-cout layers (conv_mfma.hip) on 16-row tiles ... */
  SS4K_MODEL_TILE_ROWS_20 = 32, /* ... or on 20-row tiles (default: by image height) */
  SS4K_MODEL_NO_PAIR = 256,     /* BSVD: the full-resolution layer pairs (inc, outc) as two launches each instead of the fused
                                   row-marching kernel (conv_pair.hip) */
  SS4K_MODEL_NO_DENSE = 1024,   /* RRDBNet: conv1..conv4 of every dense block as four launches, never as two fused layer pairs
                                   (csrc/conv_dense.hip: (conv1, conv2) and (conv3, conv4) stream their shared input planes once and
                                   hand x1 / x3 over in LDS) - what a job whose planes exceed 4 GB gets anyway */
  SS4K_MODEL_NO_WIDE = 4096,    /* fp16 layers with 64-cout groups and a plain epilogue on conv_mfma.hip's <2,4,4> build - what a layer of a job
                                   whose planes exceed 4 GB gets anyway - instead of conv_dense.hip's single-layer build (bit-identical to it);
                                   implies NO_W16 */
  SS4K_MODEL_FLAGS_ALL = 1 | 2 | 4 | 16 | 32 | 256 | 512 | 1024 | 4096 | 8192 | 32768
};

int ss4k_abi_version(void);
const char* ss4k_last_error(void);

/* one per HIP device; replaces `.to(device)` / torch's implicit CUDA context. */
int ss4k_ctx_create(int hip_device, ss4k_ctx** out);
void ss4k_ctx_destroy(ss4k_ctx* ctx);
int ss4k_ctx_device(const ss4k_ctx* ctx);

/* Number of fp32 scalars ss4k_model_create expects: the model's state_dict tensors flattened and
 * concatenated in state_dict order (OIHW conv weights, then bias, PReLU slopes; ConvTranspose
 * weight as (C_in, C_out, kH, kW)).  Host-only, no GPU needed.  Returns 0 for a bad desc. */
size_t ss4k_model_param_count(const ss4k_model_desc* desc);

/* Replaces build_model(...) (fsrcnn/factory.py:5, realesrgan/factory.py:108, bsvd/factory.py:21):
 * repacks the state_dict blob into MFMA-fragment order and uploads it.  host_weights may be
 * freed on return. */
int ss4k_model_create(ss4k_ctx* ctx, const ss4k_model_desc* desc, const float* host_weights,
                      size_t n_floats, ss4k_model** out);
void ss4k_model_destroy(ss4k_model* m);

/* Output geometry of ss4k_model_forward for an (n, c, h, w) input. */
int ss4k_model_out_shape(const ss4k_model* m, int n, int h, int w, int* out_c, int* out_h, int* out_w);
/* Input channel count the model expects (FSRCNN 1, RRDBNet/SRVGG 3, BSVD 4). */
int ss4k_model_in_channels(const ss4k_model* m);

/* Device bytes of activation workspace the model holds after a forward of n frames of h x w (it grows
 * to the largest shape seen and is reused); nothing is allocated or launched by this call.  The
 * size query of SURVEY.md 8(b) (`ss4k_workspace_bytes`). */
int ss4k_model_workspace_bytes(ss4k_model* m, int n, int h, int w, size_t* bytes);
/* Replaces `self.model(x)` (fsrcnn_upscaler.py:181,293-297) and `self.denoise_model(x)`
 * (:277): x is contiguous NCHW fp32 in [0,1] on the device; result contiguous NCHW fp32.
 * BSVD: in (n,4,h,w) = the reference's (n,1,4,h,w); out (n,3,h,w).  FSRCNN: (planes,1,h,w). */
int ss4k_model_forward(ss4k_model* m, const float* in_nchw_dev, float* out_nchw_dev, int n, int h,
                       int w, void* hip_stream);

/* Asynchronous status of the model's earlier forwards.  No kernel of either library has an asynchronous failure mode: always SS4K_OK, at
 * once, whatever `wait` is (SS4K_EINVAL for a NULL model).  Kept for ABI 3: the one kernel that could fail this way was removed. */
int ss4k_model_check(ss4k_model* m, int wait);

/* ---- the service's frame-in/frame-out hot path ------------------------------------------- */
typedef struct ss4k_upscale_cfg {
  int32_t lr_h, lr_w;       /* self.lr_shape (fsrcnn_upscaler.py:93-100) */
  int32_t out_h, out_w;     /* self.output_shape, 0,0 = None (fsrcnn_upscaler.py:107) */
  int32_t lr_hr_resize;     /* :92 */
  int32_t single_mode;      /* :109  (per-frame path upscale_single vs batched upscale_multi) */
  int32_t sr_is_realesrgan; /* upscaler_model == 'realesrgan' (model gets (1,3,H,W)); else FSRCNN planes */
  int32_t denoising;        /* :111 */
  int32_t reserved0;
  double denoise_rate;      /* :102 (python float = double) */
  int32_t reserved[6];
} ss4k_upscale_cfg;

/* Replaces FsrcnnUpscalerService.proc_init (fsrcnn_upscaler.py:118-139): binds the SR model,
 * the optional BSVD model, and builds the four fixed depthwise kernels (:135-138). */
int ss4k_upscaler_create(ss4k_ctx* ctx, const ss4k_upscale_cfg* cfg, ss4k_model* sr,
                         ss4k_model* denoise /* NULL unless cfg->denoising */, ss4k_upscaler** out);
void ss4k_upscaler_destroy(ss4k_upscaler* up);
/* forget `lr_prev` state: the next frame is a "first frame" again (noise map 0.05, :269-271) */
int ss4k_upscaler_reset(ss4k_upscaler* up);
int ss4k_upscaler_out_shape(const ss4k_upscaler* up, int n, int h, int w, int* out_h, int* out_w);
/* Host milliseconds the last ss4k_upscale_frames spent ENQUEUEING the denoise stage and the SR model:
 * exactly what the reference's 'fsrcnn.denoise' / 'fsrcnn.model' profiler spans measure (host
 * time.time() around asynchronous launches, fsrcnn_upscaler.py:276-278,290-300; util/profiler.py:12-24).
 * denoise_ms = 0 when the job did not denoise. */
int ss4k_upscaler_last_enqueue_ms(const ss4k_upscaler* up, double* denoise_ms, double* model_ms);

/* Replaces FsrcnnUpscalerService.upscale(frames) (fsrcnn_upscaler.py:144-326): uint8 NHWC
 * (n,h,w,3) device frames in, uint8 NHWC (n,out_h,out_w,3) device frames out. */
int ss4k_upscale_frames(ss4k_upscaler* up, const uint8_t* in_nhwc_dev, int n, int h, int w,
                        uint8_t* out_nhwc_dev, size_t out_capacity_bytes, void* hip_stream);

/* Parity taps: fp32 NCHW copies of the intermediates of the LAST ss4k_upscale_frames call
 * (the oracle exposes the same points).  which: 0 = lr (after pre-resize/denoise),
 * 1 = model output (after sharpen_hr if denoising), 2 = after mean/std match,
 * 3 = after local colour match (multi mode only), 4 = final float before *255 truncation.
 * Enable with ss4k_upscaler_enable_taps before the call; shape returned via dims[4] (n,c,h,w). */
int ss4k_upscaler_enable_taps(ss4k_upscaler* up, int enable);
int ss4k_upscaler_read_tap(ss4k_upscaler* up, int which, float* out_dev, size_t capacity_floats,
                           int dims[4], void* hip_stream);

/* ---- granular glue ops (each replaces one torch call on the path; used by the parity tests) */
/* img.permute(0,3,1,2) / 255.0  (fsrcnn_upscaler.py:170-171) */
int ss4k_op_u8nhwc_to_f32nchw(ss4k_ctx* ctx, const uint8_t* in_dev, float* out_dev, int n, int h, int w,
                              int c, void* hip_stream);
/* F.interpolate(mode='area') == adaptive average pooling (:174-176, :205-210, :239-241) */
int ss4k_op_area_resize(ss4k_ctx* ctx, const float* in_dev, float* out_dev, int planes, int h, int w,
                        int oh, int ow, void* hip_stream);
/* F.interpolate(mode='bicubic'), A=-0.75, align_corners=False (:226-228, :319-321) */
int ss4k_op_bicubic_resize(ss4k_ctx* ctx, const float* in_dev, float* out_dev, int planes, int h, int w,
                           int oh, int ow, void* hip_stream);
/* F.interpolate(mode='bilinear'), align_corners=False (:214-216) */
int ss4k_op_bilinear_resize(ss4k_ctx* ctx, const float* in_dev, float* out_dev, int planes, int h, int w,
                            int oh, int ow, void* hip_stream);
/* depthwise KxK conv with padding_mode='reflect' (blur_ker / sharpen_ker, :20-84); k2d_host = K*K
 * fp32 taps on the host, K = 3 or 17 (the service's sharpen and blur kernels) */
int ss4k_op_depthwise_reflect(ss4k_ctx* ctx, const float* in_dev, float* out_dev, int planes, int h, int w,
                              const float* k2d_host, int k, void* hip_stream);
/* per-plane mean and unbiased std (:192-197): stats_dev[2*p] = mean, [2*p+1] = std */
int ss4k_op_plane_stats(ss4k_ctx* ctx, const float* in_dev, float* stats_dev, int planes, int hw,
                        void* hip_stream);
/* (clamp(x,0,1) * 255).permute(0,2,3,1).to(uint8) — truncation (:232-233) */
int ss4k_op_f32nchw_to_u8nhwc(ss4k_ctx* ctx, const float* in_dev, uint8_t* out_dev, int n, int c, int h,
                              int w, void* hip_stream);

/* cv2.resize(img, None, fx=fx, fy=fy, interpolation=cv2.INTER_AREA) on uint8 NHWC frames for SHRINKING factors whose inverse is not an integer -
 * the image server's pre / post scale (0.8 / 0.85 / 0.66: image_pipeline.py:149-150, 259-261, 272-273, 347-348), so that a caller can keep both
 * on the device next to the upload / download.  OpenCV's general area path (computeResizeAreaTab + ResizeArea_Invoker<uchar, float>), restated
 * in oracle/cv_area.py; PARITY UNPINNED: the reference pins no OpenCV version and cv2 is not in the build image.  Output size: (cvRound(h * fy),
 * cvRound(w * fx)) - ss4k_op_cv_area_shape (host only).  Other factors return SS4K_EINVAL.  The first call for a new (h, w, fx, fy) builds and
 * uploads two small tables (kept per context, at most 64 shapes; no synchronisation unless that cache overflows). */
int ss4k_op_cv_area_shape(int h, int w, double fx, double fy, int* out_h, int* out_w);
int ss4k_op_cv_area_resize_u8(ss4k_ctx* ctx, const uint8_t* in_nhwc_dev, uint8_t* out_nhwc_dev, size_t out_capacity_bytes, int n, int h, int w,
                              int channels, double fx, double fy, void* hip_stream);

/* ---- the frame-recurrent upscaler: EGVSR's FRNet x4 (model/egvsr/egvsr.py:146-212), the network behind EgvsrUpscalerService
 * (egvsr_upscaler.py:145-212).  An object of its own, not a model kind: a step takes three tensors and frame t needs frame t - 1's output,
 * so there are no frame lanes and no job sets.  FRNet(in_nc=3, out_nc=3, nf=num_feat, nb=num_block, degradation='BD', scale=4)
 * (egvsr_upscaler.py:26; degradation 'BI': ss4k_frvsr_create_ex below): FNet (egvsr.py:12-78), 4 x BicubicUpsample(4) of the flow (utils/net_utils.py:112-165), backward_warp of the previous
 * output (net_utils.py:50-93), space-to-depth (egvsr.py:203-208), SRNet (egvsr.py:99-143).  SS4K_F16: fp16 activations with fp32 accumulation;
 * the flow, hr_prev and hr_curr stay fp32 in both dtypes. */
typedef struct ss4k_frvsr ss4k_frvsr;
typedef struct ss4k_frvsr_upscaler ss4k_frvsr_upscaler;
typedef struct ss4k_frvsr_desc {
  int32_t dtype;       /* ss4k_dtype */
  int32_t num_feat;    /* nf: SRNet's tail is PixelShuffle(4) + Conv2d(4, 3) (egvsr.py:122-127), which fixes nf = 64; anything else is refused */
  int32_t num_block;   /* nb: residual blocks, 0..SS4K_DESC_MAX_BLOCKS (the service: 10) */
  int32_t flags;       /* must be 0 */
  int32_t reserved[4];
} ss4k_frvsr_desc;
/* fp32 scalars of FRNet's state_dict, flattened in state_dict order like every other model's blob: it INCLUDES the entries forward() never
 * uses (upsample_func.kernels, srnet.conv_up.*, srnet.upsample_func.kernels: skipped).  2 587 505 at 64 / 10.  Host only; 0 for a bad desc. */
size_t ss4k_frvsr_param_count(const ss4k_frvsr_desc* desc);
/* Replaces build_egvsr_model's FRNet(...) + load_state_dict (egvsr_upscaler.py:25-29) */
int ss4k_frvsr_create(ss4k_ctx* ctx, const ss4k_frvsr_desc* desc, const float* host_weights, size_t n_floats, ss4k_frvsr** out);
void ss4k_frvsr_destroy(ss4k_frvsr* m);
/* The generator the same description builds.  SS4K_FRVSR_EGVSR: the above.  SS4K_FRVSR_TECOGAN: TecoGAN's FRNet, which EGVSR's was cut down from
 * (model/egvsr/models/networks/tecogan_nets.py:101-202; the service's nb is 16): identical up to the last residual block, then
 * ConvTranspose2d(64, 64, 3, 2, 1, output_padding=1) + ReLU twice, Conv2d(64, 3, 3, 1, 1) at (4 h, 4 w), + BicubicUpsample(4)(lr_curr)
 * (degradation 'BD').  Its blob is that class's whole state_dict in key order: the same 46 tensors, srnet.conv_out being (3, 64, 3, 3) -
 * 3 032 261 scalars at 64 / 16.  num_feat must be 64 here too.  route_flags pin the route of the transposed layers:
 * SS4K_FRVSR_CONVT_EMBEDDED - each embedded in a pad-1 3x3 convolution 64 -> 256 + PixelShuffle(2) on the conv kernels the other layers use -
 * or SS4K_FRVSR_CONVT_PHASE - the kernel of their own that computes them phase by phase with a quarter of the matrix work
 * (csrc/conv_up2.hip).  0 = the faster of the two as measured: today the embedded route.  Both pins at once are refused.
 * A wrong generator or unknown route flags: SS4K_EINVAL, and a count of 0.  ss4k_frvsr_create / ss4k_frvsr_param_count are generator 0.
 * Every other ss4k_frvsr_* entry point works on either generator.  A TecoGAN step walks its tail in groups of items such that no (4 h, 4 w)
 * plane reaches 2^32 bytes; ss4k_frvsr_workspace_bytes counts one group's tensors, and no result depends on the grouping. */
enum { SS4K_FRVSR_EGVSR = 0, SS4K_FRVSR_TECOGAN = 1 };
enum { SS4K_FRVSR_CONVT_EMBEDDED = 1, SS4K_FRVSR_CONVT_PHASE = 4 };
size_t ss4k_frvsr_param_count_as(const ss4k_frvsr_desc* desc, int generator);
int ss4k_frvsr_create_as(ss4k_ctx* ctx, const ss4k_frvsr_desc* desc, int generator, int route_flags, const float* host_weights, size_t n_floats,
                         ss4k_frvsr** out);
int ss4k_frvsr_generator(const ss4k_frvsr* m);
/* The degradation the generator was trained for: FRNet's `degradation` argument, which picks the up-sampling function (utils/net_utils.py:96-108).
 * SS4K_FRVSR_BD: BicubicUpsample(4) - everything above.  SS4K_FRVSR_BI: F.interpolate(scale_factor=4, mode='bilinear', align_corners=False),
 * the reference classes' own default.  The function up-samples the LR flow before the warp (both generators) and is TecoGAN's skip
 * conv_out + upsample_func(lr_curr); both run on kernels of their own (csrc/frvsr_bi.hip).  With 'BI' the function is no module, so the
 * state_dict holds neither upsample_func.kernels nor srnet.upsample_func.kernels: the blob is still the whole state_dict in key order, 44
 * tensors and 32 scalars fewer, and a blob of the other degradation is refused by its size.  An unknown degradation: SS4K_EINVAL, and a count
 * of 0.  Degradation SS4K_FRVSR_BD is ss4k_frvsr_param_count_as / ss4k_frvsr_create_as, bit for bit; either degradation goes with either
 * generator and either route of the transposed layers, and every other ss4k_frvsr_* entry point works on the object unchanged (stage 4 stays
 * the flow x4 + warp, stage 9 the skip). */
enum { SS4K_FRVSR_BD = 0, SS4K_FRVSR_BI = 1 };
size_t ss4k_frvsr_param_count_ex(const ss4k_frvsr_desc* desc, int generator, int degradation);
int ss4k_frvsr_create_ex(ss4k_ctx* ctx, const ss4k_frvsr_desc* desc, int generator, int degradation, int route_flags, const float* host_weights,
                         size_t n_floats, ss4k_frvsr** out);
int ss4k_frvsr_degradation(const ss4k_frvsr* m);
/* Replaces `self.model(lr_curr, self.lr_prev, self.hr_prev)` (egvsr_upscaler.py:204) = FRNet.forward (egvsr.py:180-212): lr_curr, lr_prev
 * (n, 3, h, w), hr_prev (n, 3, 4 h, 4 w) -> hr_out (n, 3, 4 h, 4 w), contiguous fp32 NCHW on the device; the n items are independent streams.
 * Stateless.  h, w >= 8 (the reference's reflect pad fails below that): SS4K_EINVAL otherwise. */
int ss4k_frvsr_step(ss4k_frvsr* m, const float* lr_curr_dev, const float* lr_prev_dev, const float* hr_prev_dev, float* hr_out_dev, int n, int h,
                    int w, void* hip_stream);
/* Device bytes of workspace the object holds after a step of n x h x w (nothing is allocated or launched) */
int ss4k_frvsr_workspace_bytes(ss4k_frvsr* m, int n, int h, int w, size_t* bytes);
/* Per-stage time of the steps since the last enable(1), from events on the caller's stream (tools/frvsr_time.py): stage 0 = FNet convs, 1 = SRNet
 * convs, 2 = pool and x2, 3 = flow finish (tanh, pad), 4 = flow x4 + warp + space-to-depth, 5 = tail, 6 = the rest (input packing, service glue);
 * a TecoGAN generator's tail: 7 = the two transposed convolutions, 8 = conv_out, 9 = the bicubic skip (5 stays 0).
 * ss4k_frvsr_prof_read synchronises with the recorded events. */
int ss4k_frvsr_prof_enable(ss4k_frvsr* m, int enable);
int ss4k_frvsr_prof_read(ss4k_frvsr* m, int stage, double* total_ms);

/* The service path.  Replaces EgvsrUpscalerService.proc_init / upscale (egvsr_upscaler.py:159-212): lr_shape = (lr_h, lr_w), output_shape =
 * (out_h, out_w), 0, 0 = None.  The n frames of ss4k_frvsr_upscale_frames are CONSECUTIVE FRAMES OF ONE STREAM, processed in order (:182-186); the
 * state (lr_prev, hr_prev) is carried across calls, so a stream must stay on one object.  Per frame (:192-212): / 255, area to lr_shape, step, the state
 * keeps the unclamped output, clamp to [0, 1], F.interpolate(mode='area') to the output shape if set, * 255 truncated to uint8 HWC.
 *
 * One object serves up to SS4K_FRVSR_MAX_STREAMS streams.  It has max_streams SLOTS, each with the recurrent state of one stream (allocated
 * on the slot's first frame: 2 x (lr + hr) fp32, 376 MB at lr 720 x 1280); which stream sits in which slot is the caller's business.
 * ss4k_frvsr_upscale_streams runs one ROUND: one frame for each of n_streams DISTINCT slots, as ONE step of n_streams items - every conv, pool,
 * x2, flow, warp and tail launch covers the whole round, and the streams' HR state is read and written where it lives (never gathered into a
 * batch).  in: (n_streams, h, w, 3) uint8; out: (n_streams, out_h, out_w, 3) uint8, item i belonging to slots[i].  Each stream's frames are bit for
 * bit what an object of its own would have produced.  SS4K_EINVAL - and no slot's state changed - for a slot outside 0..max_streams-1, a slot
 * named twice, n_streams outside 1..max_streams, a too small output buffer, or a round of 2^31 or more output pixels per plane
 * (n_streams x 16 lr_h lr_w).  ss4k_frvsr_upscaler_create is max_streams = 1; ss4k_frvsr_upscale_frames on any object is the stream of slot 0. */
#define SS4K_FRVSR_MAX_STREAMS 64
int ss4k_frvsr_upscaler_create(ss4k_ctx* ctx, ss4k_frvsr* m, int lr_h, int lr_w, int out_h, int out_w, ss4k_frvsr_upscaler** out);
int ss4k_frvsr_upscaler_create_streams(ss4k_ctx* ctx, ss4k_frvsr* m, int lr_h, int lr_w, int out_h, int out_w, int max_streams,
                                       ss4k_frvsr_upscaler** out);
void ss4k_frvsr_upscaler_destroy(ss4k_frvsr_upscaler* up);
/* the next frame of EVERY slot sees zero lr_prev / hr_prev (egvsr_upscaler.py:197-202); _reset_stream: of that slot only */
int ss4k_frvsr_upscaler_reset(ss4k_frvsr_upscaler* up);
int ss4k_frvsr_upscaler_reset_stream(ss4k_frvsr_upscaler* up, int slot);
int ss4k_frvsr_upscaler_out_shape(const ss4k_frvsr_upscaler* up, int* out_h, int* out_w);
/* device bytes of recurrent state the object holds now (slots that never saw a frame hold none; a reset frees nothing) */
int ss4k_frvsr_upscaler_state_bytes(const ss4k_frvsr_upscaler* up, size_t* bytes);
int ss4k_frvsr_upscale_frames(ss4k_frvsr_upscaler* up, const uint8_t* in_nhwc_dev, int n, int h, int w, uint8_t* out_nhwc_dev,
                              size_t out_capacity_bytes, void* hip_stream);
int ss4k_frvsr_upscale_streams(ss4k_frvsr_upscaler* up, const int32_t* slots, int n_streams, const uint8_t* in_nhwc_dev, int h, int w,
                               uint8_t* out_nhwc_dev, size_t out_capacity_bytes, void* hip_stream);
/* One round like ss4k_frvsr_upscale_streams with the frames SCATTERED: item i's input frame is in_frames_dev[i] (h, w, 3) uint8 and its result goes to
 * out_frames_dev[i] (out_h, out_w, 3) uint8 - host arrays of n_streams DEVICE pointers, the frames anywhere in device memory (rows of a ring's staging
 * tensor, allocations of their own), at any byte alignment.  The tables travel by value in the kernel arguments: no device table, no upload, no
 * synchronisation.  A round's glue is three launches whatever n_streams is (frames in, pack, frames out) and writes no fp32 intermediate.  Every
 * output byte and every slot's state is bit for bit what ss4k_frvsr_upscale_streams gives for the same frames and slots, and the two may be mixed on
 * one object.  Refuses what that call refuses, and NULL tables or entries, with SS4K_EINVAL before any slot changes; out_frame_capacity_bytes is the
 * size of EACH output frame. */
int ss4k_frvsr_upscale_streams_at(ss4k_frvsr_upscaler* up, const int32_t* slots, int n_streams, const uint8_t* const* in_frames_dev, int h, int w,
                                  uint8_t* const* out_frames_dev, size_t out_frame_capacity_bytes, void* hip_stream);
/* Parity taps of the LAST frame of the last call - after ss4k_frvsr_upscale_streams: of the LAST ITEM of the last round -, fp32 NCHW: 0 = lr_curr,
 * 1 = lr flow (padded, (1, 2, h, w)), 2 = the warped and space-to-depth tensor (1, 48, h, w), 3 = hr_curr (unclamped).  As
 * ss4k_upscaler_enable_taps / _read_tap. */
int ss4k_frvsr_upscaler_enable_taps(ss4k_frvsr_upscaler* up, int enable);
int ss4k_frvsr_upscaler_read_tap(ss4k_frvsr_upscaler* up, int which, float* out_dev, size_t capacity_floats, int dims[4], void* hip_stream);

/* Scene cuts (an addition to the reference, whose service never resets a stream: after a hard cut it warps a 4x image of the old scene into the new
 * one).  Off by default, and a stream with it off is bit for bit what it is without.  With a threshold set, every round of the three ss4k_frvsr_upscale_*
 * entry points is preceded by three launches on the round's stream - no host round trip, no synchronisation - that apply this rule per slot, in
 * exact integer arithmetic on the input frames AS THEY ARRIVE (uint8 HWC, before the area resize):
 *   1. the slot has no recurrent state (its first frame, after a reset, ...) or the frame's (h, w) differs from the stored frame's: no comparison;
 *      the frame is stored, S_prev = 0.
 *   2. otherwise S = sum over the 3 h w bytes of |frame - stored|, score = min(S, |S - S_prev|) - the second term keeps sustained fast motion from
 *      firing on every frame -, a CUT iff score >= T = max(1, ceil(threshold * 3 h w)); then S_prev = S, the frame is stored, compared += 1.  On a
 *      cut, cuts += 1 and the slot's lr_prev / hr_prev become zero: the step that follows treats the frame exactly as a new stream's first.
 * threshold is the mean absolute byte difference in 8-bit levels, in (0, 255]; 0 turns the detector off, which drops the stored frames and the
 * counters (turning it on again starts every slot at 1.); NaN, negative values and values above 255: SS4K_EINVAL.  A round that is refused
 * changes nothing of the detector either.  ss4k_frvsr_upscaler_state_bytes includes the stored frames.
 * _stats synchronises with hip_stream and reads the slot's counters and the last frame's values (all 0 after a frame that was not compared);
 * _total never synchronises: the cuts of all slots in the rounds that have COMPLETED (a pinned host array that every round refreshes by an
 * asynchronous copy on its stream). */
typedef struct ss4k_scene_cut_stats { uint64_t compared, cuts, last_sad, last_score; int32_t last_was_cut, reserved; } ss4k_scene_cut_stats;
int ss4k_frvsr_upscaler_set_scene_cut(ss4k_frvsr_upscaler* up, double threshold);      /* 0 = off (default) */
int ss4k_frvsr_upscaler_scene_cut(const ss4k_frvsr_upscaler* up, double* threshold);
int ss4k_frvsr_upscaler_scene_cut_stats(ss4k_frvsr_upscaler* up, int slot, ss4k_scene_cut_stats* out, void* hip_stream);  /* synchronises */
int ss4k_frvsr_upscaler_scene_cut_total(const ss4k_frvsr_upscaler* up, uint64_t* cuts); /* never synchronises: cuts of rounds that have completed */
/* The detector's sum on its own: sad_out_dev[i] = sum over bytes_per_frame bytes of |a_dev[i][k] - b_dev[i][k]|, exact.  a_dev / b_dev: HOST arrays
 * of n_items (1..64) DEVICE pointers, frames at any byte address; sad_out_dev: n_items uint64 on the device, 8-byte aligned.  Nothing else is
 * written.  (The temporal BSVD service needs no caller-side decision any more: ss4k_upscaler_temporal_set_scene_cut runs this sum and the rule on
 * the device and keeps a cut out of the denoiser without a flush.) */
int ss4k_op_frame_sad_u8(ss4k_ctx* ctx, const uint8_t* const* a_dev, const uint8_t* const* b_dev, int n_items, size_t bytes_per_frame,
                         uint64_t* sad_out_dev, void* hip_stream);

/* backward_warp(x, flow) (utils/net_utils.py:50-93): grid_sample(bilinear, padding_mode='border', align_corners=True) at linspace(-1, 1) +
 * flow / ((size - 1) / 2).  x (n, c, h, w), flow (n, 2, h, w) (channel 0 = x displacement in pixels), out (n, c, h, w); h, w >= 2 */
int ss4k_op_backward_warp(ss4k_ctx* ctx, const float* x_dev, const float* flow_dev, float* out_dev, int n, int c, int h, int w, void* hip_stream);
/* BicubicUpsample(4)(input) (utils/net_utils.py:112-165): replicate pad (1, 2, 1, 2), four 4-tap phase kernels of the cubic with a = -0.75, height
 * pass then width pass - NOT F.interpolate's bicubic.  (planes, h, w) -> (planes, 4 h, 4 w) */
int ss4k_op_bicubic_upsample4(ss4k_ctx* ctx, const float* in_dev, float* out_dev, int planes, int h, int w, void* hip_stream);

/* ---- BSVD as an online machine: temporal denoising whose state crosses job boundaries (reference bsvd/model.py:510-513
 * feedin_one_element).  The object holds a BSVD model created with bsvd_stream = 1 (not owned: it must outlive the object, and a clip forward
 * of the same model may run between pushes) plus the per-stream history of its 16 BiBufferConvs and skip queues, allocated on the first
 * push.  The frames a stream emits are bit for bit those of ONE ss4k_model_forward over all its frames, however the pushes cut it.
 * max_push: 1..64 frames per push; the workspace of a push never exceeds ss4k_model_workspace_bytes(model, max_push, h, w). */
typedef struct ss4k_bsvd_online ss4k_bsvd_online;
int ss4k_bsvd_online_create(ss4k_ctx* ctx, ss4k_model* bsvd_stream_model, int max_push, ss4k_bsvd_online** out);
void ss4k_bsvd_online_destroy(ss4k_bsvd_online* o);
/* number of BiBufferConvs = frames a stream holds back: 16 */
int ss4k_bsvd_online_lag(const ss4k_bsvd_online* o);
/* feedin_one_element for n frames: in (n, 4, h, w) fp32 NCHW; out receives the *n_out frames that became ready, (3, h, w) fp32 each, oldest
 * first.  *n_out is known on the host without a synchronisation: emitted so far = max(0, pushed - lag).  SS4K_EINVAL - before the first launch
 * and before any state changes - for n outside 1..max_push, h or w not a multiple of 4, a size other than the stream's first push, an output
 * capacity below the frames that become ready, or a NULL pointer. */
int ss4k_bsvd_online_push(ss4k_bsvd_online* o, const float* in_dev, int n, int h, int w, float* out_dev, size_t out_capacity_frames, int* n_out,
                          void* hip_stream);
/* ss4k_bsvd_online_push with scene cuts: cuts_dev points to n 32-bit DEVICE words, read in stream order on hip_stream (an earlier kernel on that
 * stream may have produced them); word i != 0: frame i of this push is the FIRST FRAME OF A NEW SCENE.  The only thing that joins two frames in this
 * network is the temporal shift in front of each BiBufferConv; across a cut it gives zeros, exactly as at either end of a stream.  So a stream
 * with cuts is, frame for frame and bit for bit, the concatenation of its scenes pushed and flushed as streams of their own - while the lag stays
 * 16 and every push returns the frames it would return without cuts.  The flags live in a ring of 128 frames on the device (part of
 * ss4k_bsvd_online_state_bytes from the first push that brings flags).  cuts_dev = NULL: no cut in this push (ss4k_bsvd_online_push); flags of
 * earlier pushes keep acting until their frames have left, flush rounds included.  A flag on a stream's first frame has no effect.  reset and
 * the end of a flush clear the flags.  A refused push changes nothing, the flags included. */
int ss4k_bsvd_online_push_cuts(ss4k_bsvd_online* o, const float* in_dev, const uint32_t* cuts_dev, int n, int h, int w, float* out_dev,
                               size_t out_capacity_frames, int* n_out, void* hip_stream);
/* feedin_one_element(None) until drained, then reset: the remaining min(lag, pushed) frames, in rounds of at most max_push feed calls */
int ss4k_bsvd_online_flush(ss4k_bsvd_online* o, float* out_dev, size_t out_capacity_frames, int* n_out, void* hip_stream);
/* drops the stream: the next push starts a new one (of any size).  The state buffers stay allocated */
int ss4k_bsvd_online_reset(ss4k_bsvd_online* o);
/* frames pushed and not yet emitted */
int ss4k_bsvd_online_pending(const ss4k_bsvd_online* o, int* frames);
/* device bytes of the per-stream state (0 before the first push) */
int ss4k_bsvd_online_state_bytes(const ss4k_bsvd_online* o, size_t* bytes);

/* ---- the per-frame service chain (ss4k_upscale_frames with single_mode and denoising) with the ONLINE denoiser in the place of the per-frame
 * one: every frame is denoised with its 16 neighbours on either side, across job boundaries, and meets its own undenoised LR planes - for the
 * 0.8 / 0.2 blend and the mean / std match - when it comes out, 16 frames later.  cfg must have single_mode and denoising set and an lr_shape
 * divisible by 4; sr and bsvd_stream_model (created with bsvd_stream = 1) are held, not owned.  Noise map: 0.05 for the stream's first frame,
 * 0.1 * denoise_rate after, as ss4k_upscale_frames. */
typedef struct ss4k_upscaler_temporal ss4k_upscaler_temporal;
int ss4k_upscaler_temporal_create(ss4k_ctx* ctx, const ss4k_upscale_cfg* cfg, ss4k_model* sr, ss4k_model* bsvd_stream_model, int max_push,
                                  ss4k_upscaler_temporal** out);
void ss4k_upscaler_temporal_destroy(ss4k_upscaler_temporal* up);
/* n (1..max_push) uint8 NHWC frames in; out receives the *n_out frames that became ready, (out_h, out_w, 3) uint8 each, oldest first: 0 during
 * the first 16 frames of a stream, n after.  The bytes of a frame do not depend on how the jobs cut the stream.  Refusals (SS4K_EINVAL) come
 * before the first launch and change nothing. */
int ss4k_upscale_frames_temporal(ss4k_upscaler_temporal* up, const uint8_t* in_nhwc_dev, int n, int h, int w, uint8_t* out_nhwc_dev,
                                 size_t out_capacity_bytes, int* n_out, void* hip_stream);
/* the frames still inside (min(16, pushed)), then the stream ends: the next frame is a first frame again */
int ss4k_upscaler_temporal_flush(ss4k_upscaler_temporal* up, uint8_t* out_nhwc_dev, size_t out_capacity_bytes, int* n_out, void* hip_stream);
/* drops the stream without emitting what is inside */
int ss4k_upscaler_temporal_reset(ss4k_upscaler_temporal* up);
int ss4k_upscaler_temporal_out_shape(const ss4k_upscaler_temporal* up, int h, int w, int* out_h, int* out_w);
int ss4k_upscaler_temporal_pending(const ss4k_upscaler_temporal* up, int* frames);
/* the denoiser's state plus the ring of waiting LR planes (plus the detector's stored frame, below) */
int ss4k_upscaler_temporal_state_bytes(const ss4k_upscaler_temporal* up, size_t* bytes);
/* Scene cuts for the temporal stream.  Off by default, and with it off every job runs the launches it ran before there was a detector.  With
 * a threshold set (validated as ss4k_frvsr_upscaler_set_scene_cut: (0, 255], 0 = off, else SS4K_EINVAL) every job is preceded, after all its
 * refusals, by the rule above on its input bytes AS THEY ARRIVE - frame i against frame i - 1 of the job, frame 0 against a device copy of the
 * previous job's last frame; no comparison for a stream's first frame or after a change of (h, w) - and the flags go to the denoiser as in
 * ss4k_bsvd_online_push_cuts; a scene's first frame also gets the noise map of a stream's first frame (0.05).  The output is, byte for byte,
 * that of the scenes run as separate streams (frames + flush), a job returns exactly the frames it returns without the detector, and the host
 * is never asked: no round trip, no synchronisation.  Setting 0 stops detection for later frames (and drops the stored frame and the
 * counters); flags already inside keep acting until their frames have left.  reset and flush end the detector's stream: the next frame is
 * not compared.  _stats synchronises with hip_stream; _total never does: the cuts of the jobs that have COMPLETED (a pinned host block that
 * every job refreshes by an asynchronous copy on its stream). */
int ss4k_upscaler_temporal_set_scene_cut(ss4k_upscaler_temporal* up, double threshold);   /* 0 = off (default) */
int ss4k_upscaler_temporal_scene_cut(const ss4k_upscaler_temporal* up, double* threshold);
int ss4k_upscaler_temporal_scene_cut_stats(ss4k_upscaler_temporal* up, ss4k_scene_cut_stats* out, void* hip_stream);   /* synchronises */
int ss4k_upscaler_temporal_scene_cut_total(const ss4k_upscaler_temporal* up, uint64_t* cuts);   /* never synchronises */
/* Several streams on one object.  _create_streams makes max_streams (1..64) SLOTS; a slot owns one stream's denoiser state, its ring of waiting LR
 * planes, its counters and its scene-cut detector, and allocates them with its first push.  The SR model, the glue and the job buffers are
 * shared.  _create means max_streams = 1, and every call above is slot 0 and launches what it launched before there were slots;
 * _set_scene_cut applies to every slot, _scene_cut_total sums over them, _state_bytes sums the slots in use.
 * A ROUND takes k_frames (1..64) frames of one (h, w), frame i of slot slots[i] at frames_dev[i] - HOST arrays; each frame is uint8 HWC at any
 * byte address, read where it lies.  Frames of one slot enter in the order they appear, at most max_push per slot.  The slots of the round become
 * ITEMS in order of first appearance: *n_items of them, item t being slot item_slots[t] with n_out_per_item[t] frames ready (both arrays hold
 * k_frames entries; the counts are known on the host without a synchronisation).  out receives the ready frames contiguously, item after item,
 * oldest first within an item.  Every stream's bytes are those of the same frames through a one-stream object.  The round's frames that became
 * ready share the SR forward, in chunks of at most max_push frames.  Refusals (SS4K_EINVAL: k_frames outside 1..64, a slot outside
 * 0..max_streams-1, more than max_push frames of one slot, a NULL frame, an output capacity below the ready frames) are decided for the whole
 * round before the first launch and change nothing, and so does a failed allocation of the round's buffers, the slots' rings or detectors (all
 * made before the first launch).  A round that fails after its first launch - a HIP error, or the allocation of a denoiser's state inside a
 * slot's first push - resets every slot it named. */
int ss4k_upscaler_temporal_create_streams(ss4k_ctx* ctx, const ss4k_upscale_cfg* cfg, ss4k_model* sr, ss4k_model* bsvd_stream_model, int max_push,
                                          int max_streams, ss4k_upscaler_temporal** out);
int ss4k_upscale_round_temporal(ss4k_upscaler_temporal* up, const uint8_t* const* frames_dev, const int* slots, int k_frames, int h, int w,
                                uint8_t* out_dev, size_t out_capacity_bytes, int* n_out_per_item, int* item_slots, int* n_items, void* hip_stream);
int ss4k_upscaler_temporal_flush_stream(ss4k_upscaler_temporal* up, int slot, uint8_t* out_nhwc_dev, size_t out_capacity_bytes, int* n_out,
                                        void* hip_stream);
int ss4k_upscaler_temporal_reset_stream(ss4k_upscaler_temporal* up, int slot);
int ss4k_upscaler_temporal_pending_stream(const ss4k_upscaler_temporal* up, int slot, int* frames);
int ss4k_upscaler_temporal_scene_cut_stats_stream(ss4k_upscaler_temporal* up, int slot, ss4k_scene_cut_stats* out, void* hip_stream);
/* what ONE slot will hold once its stream runs: the denoiser's state plus the ring, before any push.  Not counted: what scene cuts add to a slot
 * (the 512-byte flag ring, which _state_bytes counts once a stream carries flags, the stored frame of 3 h w bytes, which it counts too, and the
 * detector's sums, flags and counters - under 1 KiB and a pinned host block of 176 bytes -, which it does not) */
int ss4k_upscaler_temporal_stream_state_bytes_for(const ss4k_upscaler_temporal* up, size_t* bytes);
/* frees the device memory of every slot with no running stream (never pushed, flushed or reset): the denoiser's state, the flag ring, the LR ring
 * and the detector's device buffers - that slot's cut counters start over, as after _set_scene_cut(0), and _scene_cut_total no longer holds
 * them; the threshold stays.  Such a slot allocates again with its next push. */
int ss4k_upscaler_temporal_release_idle(ss4k_upscaler_temporal* up);
/* The denoise rate of ONE slot's stream: the noise level of every frame of that slot that enters from the next push or round on is 0.1 * rate
 * (a stream's or a scene's first frame keeps 0.05).  A slot that was never set uses cfg.denoise_rate.  The rate belongs to the stream: _reset,
 * _reset_stream, _flush, _flush_stream and - for a slot with no running stream - _release_idle put the slot back to cfg.denoise_rate, so the next
 * stream in it starts with the default.  Slot 0 is also the stream of the one-stream calls.  SS4K_EINVAL, changing nothing: a slot outside
 * 0..max_streams-1, a rate that is not finite or is negative.  A stream at rate r gives the bytes of an object created with denoise_rate = r. */
int ss4k_upscaler_temporal_set_denoise_rate_stream(ss4k_upscaler_temporal* up, int slot, float rate);
/* THE NOISE MAP.  BSVD's fourth input plane says, pixel by pixel, how much noise to assume.  SS4K_NOISE_MAP_CONSTANT (the default) is the plane
 * above: 0.05 for a stream's or a scene's first frame, 0.1 * rate after.  SS4K_NOISE_MAP_MOTION is the rule the reference computes and then
 * overwrites (fsrcnn_upscaler.py:250-254, :262): first frames keep the constant 0.05; every other frame t of a stream gets
 *   m_t = min(max(10 B, 0), 0.1f) * (float)(0.35 * rate),   B = gauss3x3(sigma 0.5, 'reflect')(mean over the planes of |lr_t - lr_{t-1}|)
 * in fp32, with lr_t the frame's LR planes as they enter (step 1) and rate the slot's denoise rate.  ONE DEPARTURE from the reference: its
 * lr_{t-1} is the previous frame after denoising and blending, which here exists only 16 frames later; ours is the previous frame as it went
 * in - it is still in the slot's LR ring, so the mode adds no state, no launch and no host round trip.  The mode holds for every slot and both
 * for rounds and the one-stream calls, which stay bit-identical on slot 0.  _set_noise_map: SS4K_EINVAL, changing nothing, for another mode
 * and while ANY slot has a running stream (pushed and neither flushed nor reset). */
#define SS4K_NOISE_MAP_CONSTANT 0
#define SS4K_NOISE_MAP_MOTION 1
int ss4k_upscaler_temporal_set_noise_map(ss4k_upscaler_temporal* up, int mode);
int ss4k_upscaler_temporal_noise_map(const ss4k_upscaler_temporal* up, int* mode);

/* ---- the frame-recurrent service chain (ss4k_frvsr_upscaler) with the ONLINE denoiser in front, per stream.  A recurrent generator warps hr_prev
 * forward frame after frame, so the noise of a block-compressed stream accumulates where a per-frame network forgets it; the reference's main
 * service always denoises before it upscales (fsrcnn_upscaler.py:245-284), its EGVSR service never got that step.  For one stream, frame t
 * (uint8 HWC, any size):
 *   1. lr_before_t = area(img / 255, lr_shape)
 *   2. den_t = the online BSVD output for frame t of the stream whose 4-plane inputs are (lr_before, noise); noise is 0.05 for a stream's first
 *      frame and 0.1 * rate after it.  den_t exists once frame t + 16 has entered, or at a flush.
 *   3. lr_curr_t = 0.8 * clamp01(sharpen3x3_reflect(den_t)) + 0.2 * lr_before_t   (sharpen_ker(strength = 0.00002), fsrcnn_upscaler.py:279-281)
 *   4. hr_t = FRNet(lr_curr_t, lr_curr_{t-1}, hr_{t-1}), zeros for a stream's first frame; then clamp, area to (out_h, out_w) if set, * 255
 *      truncated to uint8 (egvsr_upscaler.py:197-212).  lr_prev is the denoised, blended previous frame.
 *   5. nothing of the per-frame tail follows (no HR sharpening, no mean / std match): hr_prev stays the generator's own output.
 * A stream returns nothing for its first 16 frames and one frame per frame after; a flush returns the up to 16 frames still inside, through the
 * generator in order, and ends the stream - denoiser state, LR ring and recurrent state count as gone and the slot is free.
 * frvsr (either generator, either degradation) and bsvd_stream_model (created with bsvd_stream = 1) are held, not owned.  lr_h and lr_w are at
 * least 8 and divisible by 4; (out_h, out_w) = (0, 0) is None; max_push 1..64 frames of one slot per round; max_streams 1..64 SLOTS.  A slot owns
 * one stream's denoiser state, its ring of 16 + max_push waiting LR frames and its recurrent state (2 x (lr + hr) fp32), all allocated with the
 * stream's first frame; the models and the job buffers are shared.
 * A ROUND is ss4k_upscale_round_temporal's: k_frames (1..64) frames of one (h, w), frame i of slot slots[i] at frames_dev[i] - HOST arrays, each
 * frame uint8 HWC at any byte address.  The slots become ITEMS in order of first appearance (*n_items, item_slots[t], n_out_per_item[t]; both
 * arrays hold k_frames entries, the counts are known without a synchronisation); out receives the ready frames contiguously, item after item,
 * oldest first within an item.  Behind the denoiser the ready frames pass the generator in waves - wave r is frame r of every item that has
 * one, as ONE batched step - so a wave costs a fixed number of launches whatever its size.  Every stream's bytes are those of the same frames
 * through an object of its own, however the rounds cut them.  Refusals (SS4K_EINVAL: what ss4k_upscale_round_temporal refuses) are decided for
 * the whole round before the first launch and change nothing, and so does a failed allocation of the round's buffers or a slot's ring and
 * recurrent state.  A round that fails after its first launch resets every slot it named.
 * _set_denoise_rate_stream, _stream_state_bytes_for, _state_bytes and _release_idle are their ss4k_upscaler_temporal_* counterparts (a slot's
 * share includes its recurrent state).
 * SCENE CUTS.  Off by default, and with it off a round launches exactly what it launches without a detector.  _set_scene_cut (every slot;
 * validated as ss4k_frvsr_upscaler_set_scene_cut: (0, 255], 0 = off, NaN / negative / > 255 SS4K_EINVAL) puts the rule above in front of
 * every round, per slot, on the input bytes AS THEY ARRIVE - frame i of an item against frame i - 1, frame 0 against a device copy of the
 * slot's previous frame; no comparison for a stream's first frame or after a change of (h, w) - exactly as ss4k_upscaler_temporal_set_scene_cut.
 * With a threshold set a stream is the concatenation of its scenes, frame for frame and bit for bit, each scene as if it had been pushed into
 * and flushed out of an object of its own: when stream frame f of a slot is flagged, (1) the denoiser does not reach across f, (2) f's noise
 * plane is 0.05, and (3) in the wave in which frame f LEAVES the denoiser - 16 frames later, or at the flush - the slot's lr_prev / hr_prev
 * read as zero, as for a stream's first frame.  The lag stays 16, a round returns the frames it returns without the detector in the same order,
 * and the flags never leave the device.  Setting 0 stops detection for later frames and drops the stored frames and the counters; flags already
 * inside keep acting, on the denoiser and on the generator, until their frames have left.  _reset_stream and _flush_stream end the detector's
 * stream (the next frame is not compared); _release_idle frees an idle slot's detector buffers, and that slot's counters start over.
 * _state_bytes includes the detectors' device buffers (the stored frame of 3 h w bytes and under 1 KiB of sums, flags and counters per slot);
 * _stream_state_bytes_for does not.  _scene_cut_stats_stream synchronises with hip_stream; _scene_cut_total never does: the cuts of the rounds
 * that have COMPLETED, summed over the slots.  A refused round changes nothing, the detectors included.
 * ANY LR SHAPE (_create_padded).  BSVD's two 2x poolings need planes divisible by 4, and the reference never runs the denoiser at another
 * shape, so this library defines it.  For (lr_h, lr_w), both at least 8, let (ph, pw) be (lr_h, lr_w) rounded up to multiples of 4.  Step 1 and
 * the slot's LR ring stay at (lr_h, lr_w).  The denoiser sees each colour plane padded at the bottom and on the right by reflection without
 * repeating the edge (torch's and numpy's 'reflect': padded row y >= lr_h is row 2 (lr_h - 1) - y, columns likewise; at most 3 rows or columns,
 * fewer than the 8 a plane has), the noise plane is its constant over the whole (ph, pw), and the denoiser runs - and keeps its state - at
 * (ph, pw).  den_t is cropped to its top-left (lr_h, lr_w); step 3 acts on the crop, and the sharpening kernel's own reflection is at the
 * crop's borders and never reads the padding.  The generator, lr_prev / hr_prev, the output, scene cuts, rates, flush and reset are at
 * (lr_h, lr_w), exactly as above.  _create_padded takes _create's arguments; a shape divisible by 4 builds the very object _create builds (the
 * same launches), any other shape of at least 8 x 8 the padded form.  _create itself keeps refusing such a shape. */
typedef struct ss4k_frvsr_temporal ss4k_frvsr_temporal;
int ss4k_frvsr_temporal_create(ss4k_ctx* ctx, ss4k_frvsr* frvsr, ss4k_model* bsvd_stream_model, int lr_h, int lr_w, int out_h, int out_w,
                               double denoise_rate, int max_push, int max_streams, ss4k_frvsr_temporal** out);
int ss4k_frvsr_temporal_create_padded(ss4k_ctx* ctx, ss4k_frvsr* frvsr, ss4k_model* bsvd_stream_model, int lr_h, int lr_w, int out_h, int out_w,
                                      double denoise_rate, int max_push, int max_streams, ss4k_frvsr_temporal** out);
void ss4k_frvsr_temporal_destroy(ss4k_frvsr_temporal* up);
int ss4k_frvsr_temporal_round(ss4k_frvsr_temporal* up, const uint8_t* const* frames_dev, const int* slots, int k_frames, int h, int w,
                              uint8_t* out_dev, size_t out_capacity_bytes, int* n_out_per_item, int* item_slots, int* n_items, void* hip_stream);
int ss4k_frvsr_temporal_flush_stream(ss4k_frvsr_temporal* up, int slot, uint8_t* out_nhwc_dev, size_t out_capacity_bytes, int* n_out,
                                     void* hip_stream);
/* drops the slot's stream without emitting what is inside */
int ss4k_frvsr_temporal_reset_stream(ss4k_frvsr_temporal* up, int slot);
int ss4k_frvsr_temporal_pending_stream(const ss4k_frvsr_temporal* up, int slot, int* frames);
int ss4k_frvsr_temporal_set_denoise_rate_stream(ss4k_frvsr_temporal* up, int slot, float rate);
int ss4k_frvsr_temporal_out_shape(const ss4k_frvsr_temporal* up, int* out_h, int* out_w);
int ss4k_frvsr_temporal_state_bytes(const ss4k_frvsr_temporal* up, size_t* bytes);
int ss4k_frvsr_temporal_stream_state_bytes_for(const ss4k_frvsr_temporal* up, size_t* bytes);
int ss4k_frvsr_temporal_release_idle(ss4k_frvsr_temporal* up);
int ss4k_frvsr_temporal_set_scene_cut(ss4k_frvsr_temporal* up, double threshold);   /* 0 = off (default) */
int ss4k_frvsr_temporal_scene_cut(const ss4k_frvsr_temporal* up, double* threshold);
int ss4k_frvsr_temporal_scene_cut_stats_stream(ss4k_frvsr_temporal* up, int slot, ss4k_scene_cut_stats* out, void* hip_stream);   /* synchronises */
int ss4k_frvsr_temporal_scene_cut_total(const ss4k_frvsr_temporal* up, uint64_t* cuts);   /* never synchronises */
/* the noise map of step 2, as ss4k_upscaler_temporal_set_noise_map: SS4K_NOISE_MAP_CONSTANT (default) or SS4K_NOISE_MAP_MOTION.  In the padded
 * form the map is computed on the (lr_h, lr_w) frame and padded to (ph, pw) by the reflection that pads the colour planes. */
int ss4k_frvsr_temporal_set_noise_map(ss4k_frvsr_temporal* up, int mode);
int ss4k_frvsr_temporal_noise_map(const ss4k_frvsr_temporal* up, int* mode);

/* ---- measurement hooks (bench.py: live per-kernel timing with HIP events on the launch stream) */
/* When enabled, every launch of the dominant conv kernel is bracketed with hipEvents on the
 * stream it is launched on; ss4k_prof_read returns (#launches, total ms, algorithmic FLOPs). */
int ss4k_prof_enable(ss4k_ctx* ctx, int enable);
int ss4k_prof_reset(ss4k_ctx* ctx);
int ss4k_prof_read(ss4k_ctx* ctx, int64_t* launches, double* total_ms, double* flops);
/* The same per kernel family: kind 0 = the 3x3 conv kernels (what ss4k_prof_read returns), 1 / 2 / 3 = FSRCNN's head (5x5 conv +
 * shrink), mapping (4 x conv3x3 12->12) and tail (expand + 9x9 transposed conv) stages, each bracketed as one unit. */
int ss4k_prof_read_kind(ss4k_ctx* ctx, int kind, int64_t* launches, double* total_ms, double* flops);
/* ... and per kernel BUILD of the conv launches (which tile / MFMA shape / epilogue form a launch was routed to), since the last reset:
 * index 0 .. n-1 in name order, SS4K_EINVAL past the last one.  `name` receives a NUL-terminated description that starts with the kernel's
 * C++ name as rocprofv3 prints it (e.g. "w16::conv3x3_w16_kernel<RL> (...)").  With two launch chains in flight the per-launch times overlap:
 * read these from a one-chain run (SS4K_MODEL_ONE_CHAIN) when a kernel's own rate is wanted. */
int ss4k_prof_read_family(ss4k_ctx* ctx, int index, char* name, size_t name_capacity, int64_t* launches, double* total_ms, double* flops);
/* ---- streams
 * HIP serves a process's streams from a few hardware queues.  Two streams on one queue run in order whatever the program says, and
 * some pairs of queues launch slowly while both are busy (measured: 14 us per launch instead of 2.5, profiles/earlier/r05/r05_lane_queue.txt);
 * which queue a stream gets depends on how many the process created before it.  This call MEASURES a pair (a 0.2 ms idle kernel on
 * each, then 200 x 1 us kernels interleaved; ~ 3 ms, synchronises both streams) and sets *side_by_side to 1 or 0.  A host that runs
 * several contexts on its own streams calls it once per pair and replaces a stream that fails (keep the failed one alive until the
 * replacement exists, or the new stream lands on the same queue).  The library does this itself for each ctx's internal lane stream
 * (once per ctx and caller stream, before the first two-chain forward); that built-in test is switched off by the environment variable
 * SS4K_NO_LANE_CHECK=1, is skipped while the caller's stream is being captured into a graph or a profiler has preloaded itself
 * (ROCP_TOOL_LIBRARIES / LD_PRELOAD of rocprofiler: counter collection serialises kernels), and leaves the NULL stream alone while any
 * other stream of the process is under a global-mode capture. */
int ss4k_stream_pair_check(ss4k_ctx* ctx, void* hip_stream_a, void* hip_stream_b, int* side_by_side);

/* Conv sections: wall time, on the caller's stream, from the first conv launch of every network forward to the end
 * of its last one (launch boundaries included).  A job's frames may go through the conv layers as two CONCURRENT launch
 * chains (frame lanes): the per-launch times of ss4k_prof_read then overlap, and sum(FLOPs) / section time is the rate
 * the chip sustained; total_ms / section_ms = average number of conv launches in flight. */
int ss4k_prof_read_section_ms(ss4k_ctx* ctx, double* section_ms);

#ifdef __cplusplus
}
#endif
#endif /* SS4K_H */
