// Launch auditors: they stand where the launchers and glue ops of the .hip files stand in the product library, take the argument
// structs the model executor filled in, launch nothing, and restate every byte range the real kernel reads or writes for those
// arguments.  Each range must lie inside ONE live allocation of the registry.  Every formula names the kernel code it restates
// (paths under sharkshark-4k_amd/csrc/).
#include "hostcheck.h"
#include "../../sharkshark-4k_amd/csrc/models.h"

namespace {

using hc::g_where;

int layer_of(const void* wpk) {
  if (!g_where.model) return -1;
  const auto& L = g_where.model->layers;
  for (size_t i = 0; i < L.size(); ++i) if (L[i].w.ptr == wpk) return (int)i;
  return -1;
}

void need(const char* kind, int layer, const char* operand, const char* ref, const void* p, size_t bytes) {
  size_t off = 0, ab = 0;
  if (hc::reg_inside(p, bytes, &off, &ab)) return;
  if (++hc::g_violations > 40) return;   // (the count goes on; the first ones name the defect)
  if (ab) std::printf("VIOLATION %s | %s | launch %d (%s) layer %d | %s [%s] | bytes [%zu, %zu) of an allocation of %zu\n", g_where.desc.c_str(), g_where.shape.c_str(),
                      g_where.launch, kind, layer, operand, ref, off, off + bytes, ab);
  else std::printf("VIOLATION %s | %s | launch %d (%s) layer %d | %s [%s] | %zu bytes at %p: outside every live allocation\n", g_where.desc.c_str(), g_where.shape.c_str(),
                   g_where.launch, kind, layer, operand, ref, bytes, p);
}

// `nplanes` planes from plane0, frames [n0, n0 + N) of frame_bytes each; a plane must also hold those frames
void planes(const char* kind, int layer, const char* operand, const char* ref, const char* base, size_t plane_bytes, int plane0, int nplanes, size_t frame_bytes, int n0, int N) {
  if (nplanes > 0 && (size_t)(n0 + N) * frame_bytes > plane_bytes) {
    ++hc::g_violations;
    std::printf("VIOLATION %s | %s | launch %d (%s) layer %d | %s [%s] | frames [%d, %d) of %zu bytes do not fit a plane of %zu\n", g_where.desc.c_str(), g_where.shape.c_str(), g_where.launch,
                kind, layer, operand, ref, n0, n0 + N, frame_bytes, plane_bytes);
  }
  for (int k = 0; k < nplanes; ++k)
    need(kind, layer, operand, ref, base + (size_t)(plane0 + k) * plane_bytes + (size_t)n0 * frame_bytes, (size_t)N * frame_bytes);
}

void begin_launch(const char* kind = nullptr, int layer = -1, bool w16 = false) {
  ++hc::g_launches;
  if (hc::g_trace && kind) std::printf("LAUNCH %d %s layer %d%s\n", g_where.launch, kind, layer, w16 ? " w16" : "");
}
void end_launch() { ++g_where.launch; }

// bytes of pack_conv3x3's blob for one (group, K-chunk): 9 taps x KS k-steps x nb blocks x 64 lanes x 16 bytes (pack.cpp:52,62)
size_t wpk_chunk_bytes(int dtype, int nb) { return (size_t)9 * (dtype == SS4K_F16 ? 1 : 2) * nb * 1024; }

}  // namespace

namespace ss4k {

void launch_conv3x3(ss4k_ctx*, const ConvArgs& a, int dtype, hipStream_t) {
  const char* K = "conv3x3";
  const int li = layer_of(a.wpk);
  begin_launch(K, li, a.w16 != nullptr);
  const size_t rec = conv_rec_bytes(dtype);
  const int nb = a.cout_pad <= 32 ? 1 : 2, groups = (a.cout_pad + nb * 32 - 1) / (nb * 32);   // conv_mfma.hip:727-728
  const int nch = a.nchunks0 + a.nchunks1;
  // input: one plane per K-chunk, source grid (H/2, W/2) under ups2; pixel index (n * Hs + sy) * Ws + sx, n in [n0, n0 + N)
  const size_t in_frame = (size_t)(a.ups2 ? a.H / 2 : a.H) * (a.ups2 ? a.W / 2 : a.W) * rec;
  planes(K, li, "in0", "conv_mfma.hip:123-129,142,154", a.in0, a.in0_plane_bytes, a.in0_plane0, a.nchunks0, in_frame, a.n0, a.N);
  planes(K, li, "in1", "conv_mfma.hip:123-129,143,154", a.in1, a.in1_plane_bytes, a.in1_plane0, a.nchunks1, in_frame, a.n0, a.N);
  // weights: groups x chunks of 9 * KS * NB KB; the 16x16x32 routes read the w16 / w16n blob of the same layer
  need(K, li, "wpk", "pack.cpp:62; conv_mfma.hip:145,161", a.wpk, (size_t)groups * nch * wpk_chunk_bytes(dtype, nb));
  if (a.w16) {
    const size_t b = a.cout_pad >= 64 ? (size_t)(a.cout_pad / 64) * (nch / 2) * 3 * 3 * 4 * 64 * 16    // pack.cpp:104
                                      : (size_t)(nch / 2) * 3 * 3 * 64 * 16;                           // pack.cpp:133
    need(K, li, "w16", a.cout_pad >= 64 ? "pack.cpp:104 (conv_w16.hip)" : "pack.cpp:133 (conv_w16n.hip)", a.w16, b);
  }
  need(K, li, "bias", "conv_mfma.hip:169", a.bias, (size_t)a.cout_pad * 4);
  if (a.act == ACT_PRELU) need(K, li, "prelu", "conv_mfma.hip:170", a.prelu, (size_t)a.cout_pad * 4);
  const size_t frame = (size_t)a.H * a.W * rec;
  const int out_planes = a.cout_pad / 16;   // every 32-cout block below cout_pad stores its two planes (conv_mfma.hip:383,491,551)
  const bool plain = a.epi == EPI_NHWC && !a.bsvd_resid;   // EK_PLAIN (conv_mfma.hip:765)
  if (a.epi == EPI_NHWC) {
    planes(K, li, "out", "conv_mfma.hip:383,394-395,426-427,646", a.out, a.out_plane_bytes, a.out_plane0, out_planes, frame, a.n0, a.N);
  } else if (a.epi == EPI_NHWC_SUB2) {
    const size_t f2 = (size_t)((a.H + 1) / 2) * ((a.W + 1) / 2) * rec;
    planes(K, li, "out (stride 2)", "conv_mfma.hip:491,503-504,514,529-530", a.out, a.out_plane_bytes, a.out_plane0, out_planes, f2, a.n0, a.N);
  } else if (a.epi == EPI_NHWC_PS2) {
    const int cpb = (a.cout_real / 4) / 16;
    planes(K, li, "out (PixelShuffle 2)", "conv_mfma.hip:501-504,516,529-530", a.out, a.out_plane_bytes, a.out_plane0, cpb, 4 * frame, a.n0, a.N);
    if (a.res1) planes(K, li, "res1 (PixelShuffle 2)", "conv_mfma.hip:505,533-534", a.res1, a.r1_plane_bytes, a.r1_plane0, cpb, 4 * frame, a.n0, a.N);
  } else {  // EPI_NCHW_F32
    const size_t f32_frame = (size_t)a.cout_real * a.H * a.W * 4;
    need(K, li, "out (NCHW fp32)", "conv_mfma.hip:648-653", a.out + (size_t)a.n0 * f32_frame, (size_t)a.N * f32_frame);
  }
  if (a.epi != EPI_NHWC_PS2) {
    if (a.res1) {
      if (plain) planes(K, li, "res1", "conv_mfma.hip:392,447", a.res1, a.r1_plane_bytes, a.r1_plane0, out_planes, frame, a.n0, a.N);
      else if (a.bsvd_resid) planes(K, li, "res1 (skip - conv, channels 0..2)", "conv_mfma.hip:624-627", a.res1, a.r1_plane_bytes, a.r1_plane0, 1, frame, a.n0, a.N);
      else planes(K, li, "res1", "conv_mfma.hip:552,624-627", a.res1, a.r1_plane_bytes, a.r1_plane0, (a.cout_real + 15) / 16, frame, a.n0, a.N);
    }
    if (a.res2) planes(K, li, "res2", "conv_mfma.hip:393,448,638", a.res2, a.r2_plane_bytes, a.r2_plane0, out_planes, frame, a.n0, a.N);
  }
  end_launch();
}

void launch_conv3x3_pair(ss4k_ctx*, const PairArgs& a, hipStream_t) {
  const char* K = "pair";
  const int li = layer_of(a.wA);
  begin_launch(K, li);
  const size_t frame = (size_t)a.H * a.W * 32;
  planes(K, li, "in", "conv_pair.hip:132", a.in, a.in_plane_bytes, a.in_plane0, a.planes_a, frame, a.n0, a.N);
  need(K, li, "wA", "conv_pair.hip:79; pack.cpp:62", a.wA, (size_t)a.planes_a * wpk_chunk_bytes(SS4K_F16, 1));
  need(K, li, "wB", "conv_pair.hip:79; pack.cpp:62", a.wB, (size_t)2 * wpk_chunk_bytes(SS4K_F16, 1));
  need(K, li, "biasA", "conv_pair.hip:89", a.biasA, 32 * 4);
  need(K, li, "biasB", "conv_pair.hip:89", a.biasB, 32 * 4);
  if (a.epi != 0) planes(K, li, "res", "conv_pair.hip:138,155", a.res, a.res_plane_bytes, a.res_plane0, 1, frame, a.n0, a.N);
  if (a.epi == 2) {
    const size_t f32_frame = (size_t)a.cout_real * a.H * a.W * 4;
    need(K, li, "out (NCHW fp32)", "conv_pair.hip:266", a.out + (size_t)a.n0 * f32_frame, (size_t)a.N * f32_frame);
  } else {
    planes(K, li, "out", "conv_pair.hip:272-274", a.out, a.out_plane_bytes, a.out_plane0, 2, frame, a.n0, a.N);
  }
  end_launch();
}

void launch_conv3x3_dense2(ss4k_ctx*, const DenseArgs& a, hipStream_t) {
  const char* K = "dense2";
  const int li = layer_of(a.w1);
  begin_launch(K, li);
  const size_t frame = (size_t)a.H * a.W * 32;
  const int k1 = a.nchunks0 + a.nchunks1;
  planes(K, li, "in0", "conv_dense.hip:167", a.in0, a.in0_plane_bytes, a.in0_plane0, a.nchunks0, frame, a.n0, a.N);
  planes(K, li, "in1", "conv_dense.hip:168", a.in1, a.in1_plane_bytes, a.in1_plane0, a.nchunks1, frame, a.n0, a.N);
  need(K, li, "w1", "conv_dense.hip:177; pack.cpp:62", a.w1, (size_t)k1 * wpk_chunk_bytes(SS4K_F16, 1));
  need(K, li, "w2", "conv_dense.hip:177-178; pack.cpp:62", a.w2, (size_t)(k1 + 2) * wpk_chunk_bytes(SS4K_F16, 1));
  need(K, li, "bias1", "conv_dense.hip:201", a.bias1, 32 * 4);
  need(K, li, "bias2", "conv_dense.hip:201", a.bias2, 32 * 4);
  planes(K, li, "out1", "conv_dense.hip:323,344", a.out1, a.out1_plane_bytes, a.out1_plane0, 2, frame, a.n0, a.N);
  planes(K, li, "out2", "conv_dense.hip:427,436", a.out2, a.out2_plane_bytes, a.out2_plane0, 2, frame, a.n0, a.N);
  end_launch();
}

void fsrcnn_forward(ss4k_ctx*, const FsrcnnWeights& W, int factor, const float* in, float* out, int n, int h, int w, float* ws12a, float* ws12b, int mode,
                    hipStream_t, bool out_half, bool in_u8) {
  begin_launch();
  const char* K = "fsrcnn";
  const size_t px = (size_t)n * h * w;
  need(K, -1, "in", "fsrcnn.hip:1315,1337", in, px * (in_u8 ? 1 : 4));
  need(K, -1, "out", "fsrcnn.hip:1309 (HR planes)", out, px * factor * factor * (out_half ? 2 : 4));
  // the two stage buffers: 12 channels per pixel, fp32 at most (the fp16 mode packs them tighter)
  need(K, -1, "ws12a", "models.cpp:702; fsrcnn.hip:1337,1352", ws12a, px * 12 * 4);
  need(K, -1, "ws12b", "models.cpp:702; fsrcnn.hip:1352-1356", ws12b, px * 12 * 4);
  (void)mode;
  need(K, -1, "w_feat", "glue.h:77", W.w_feat, 25 * 56 * 4); need(K, -1, "b_feat", "glue.h:78", W.b_feat, 56 * 4); need(K, -1, "a_feat", "glue.h:79", W.a_feat, 56 * 4);
  need(K, -1, "w_shrink", "glue.h:80", W.w_shrink, 56 * 12 * 4); need(K, -1, "b_shrink", "glue.h:81", W.b_shrink, 12 * 4); need(K, -1, "a_shrink", "glue.h:81", W.a_shrink, 12 * 4);
  for (int l = 0; l < 4; ++l) {
    need(K, -1, "w_map", "glue.h:82", W.w_map[l], 9 * 12 * 12 * 4); need(K, -1, "b_map", "glue.h:83", W.b_map[l], 12 * 4); need(K, -1, "a_map", "glue.h:83", W.a_map[l], 12 * 4);
  }
  need(K, -1, "w_expand", "glue.h:84", W.w_expand, 12 * 56 * 4); need(K, -1, "b_expand", "glue.h:85", W.b_expand, 56 * 4); need(K, -1, "a_expand", "glue.h:85", W.a_expand, 56 * 4);
  need(K, -1, "w_deconv", "glue.h:86", W.w_deconv, 81 * 56 * 4);
  end_launch();
}

template <typename T>
void op_pack_input(const float* in, T* out, int n, int c, int h, int w, int r, int nplanes, hipStream_t) {
  begin_launch();
  need("pack_input", -1, "in", "glue.hip:882", in, (size_t)n * c * h * w * 4);
  need("pack_input", -1, "out", "glue.hip:869,886", out, (size_t)nplanes * n * (h / r) * (w / r) * 16 * sizeof(T));
  end_launch();
}
template void op_pack_input<float>(const float*, float*, int, int, int, int, int, int, hipStream_t);
template void op_pack_input<__half>(const float*, __half*, int, int, int, int, int, int, hipStream_t);

template <typename T, typename HT>
void op_ps_nchw_addbase(const T* src, HT* out, const float* base, int n, int h, int w, int r, int cq, double* stats_acc, hipStream_t) {
  begin_launch();
  const size_t px = (size_t)n * h * w;
  // colour c reads channels [c r^2, (c + 1) r^2): planes 0 .. (cq r^2 - 1) / 16 of n*h*w records
  need("ps_nchw_addbase", -1, "src", "glue.hip:920,925-926", src, (size_t)((cq * r * r + 15) / 16) * px * 16 * sizeof(T));
  need("ps_nchw_addbase", -1, "base", "glue.hip:934", base, px * cq * 4);
  need("ps_nchw_addbase", -1, "out", "glue.hip:935,941-942", out, px * cq * r * r * sizeof(HT));
  if (stats_acc) need("ps_nchw_addbase", -1, "stats_acc", "glue.hip:965,975", stats_acc, sizeof(double) * 2 * n * cq * STATS_SLOTS);
  end_launch();
}
template void op_ps_nchw_addbase<float, float>(const float*, float*, const float*, int, int, int, int, int, double*, hipStream_t);
template void op_ps_nchw_addbase<__half, float>(const __half*, float*, const float*, int, int, int, int, int, double*, hipStream_t);
template void op_ps_nchw_addbase<__half, __half>(const __half*, __half*, const float*, int, int, int, int, int, double*, hipStream_t);

void op_temporal_shift(const void* in, void* out, int nplanes, int frames, size_t frame_px, int slots_per_record, int, int, hipStream_t) {
  begin_launch();
  const size_t bytes = (size_t)nplanes * frames * frame_px * slots_per_record * 16;   // one thread per 16-byte slot, in[i + k] with 0 <= i + k < total
  need("temporal_shift", -1, "in", "glue.hip:1006-1007,1015", in, bytes);
  need("temporal_shift", -1, "out", "glue.hip:1006-1007,1016", out, bytes);
  end_launch();
}

void op_lane_spin(unsigned, hipStream_t) {}

}  // namespace ss4k
