// Launch auditors: they stand where the launchers and glue ops of the .hip files stand in the product library, take the argument
// structs the model executor filled in, launch nothing, and restate every byte range the real kernel reads or writes for those
// arguments.  Each range must lie inside ONE live allocation of the registry.  Every formula names the kernel code it restates
// (paths under sharkshark-4k_amd/csrc/).  While hc::g_log is set every launch is also recorded - kind, and every range with whether it was read or
// written - and checked on the spot: no read of bytes nothing has written since the buffer was allocated, no write over a range the same launch reads.
#include "hostcheck.h"
#include "../../sharkshark-4k_amd/csrc/frvsr.h"

namespace {

using hc::g_where;

int layer_of(const void* wpk) {
  if (!g_where.model) return -1;
  const auto& L = g_where.model->layers;
  for (size_t i = 0; i < L.size(); ++i) if (L[i].w.ptr == wpk) return (int)i;
  return -1;
}

hc::Launch g_cur;   // the launch being audited (recorded only while hc::g_log is set)

void report(const char* kind, int layer, const char* operand, const char* ref, const char* what) {
  if (++hc::g_violations > 40) return;   // (the count goes on; the first ones name the defect)
  std::printf("VIOLATION %s | %s | launch %d (%s) layer %d | %s [%s] | %s\n", g_where.desc.c_str(), g_where.shape.c_str(), g_where.launch, kind, layer, operand, ref, what);
}

void need(const char* kind, int layer, const char* operand, const char* ref, const void* p, size_t bytes, bool write = false, int item = -1) {
  size_t off = 0, ab = 0;
  if (hc::g_log && bytes) g_cur.r.push_back({static_cast<const char*>(p), bytes, write, operand, item});
  if (hc::reg_inside(p, bytes, &off, &ab)) {
    if (!hc::g_log || !bytes) return;
    if (!write && !hc::cov_covered(p, bytes)) report(kind, layer, operand, ref, "reads bytes that nothing has written since the buffer was allocated");
    return;
  }
  if (++hc::g_violations > 40) return;
  if (ab) std::printf("VIOLATION %s | %s | launch %d (%s) layer %d | %s [%s] | bytes [%zu, %zu) of an allocation of %zu\n", g_where.desc.c_str(), g_where.shape.c_str(),
                      g_where.launch, kind, layer, operand, ref, off, off + bytes, ab);
  else std::printf("VIOLATION %s | %s | launch %d (%s) layer %d | %s [%s] | %zu bytes at %p: outside every live allocation\n", g_where.desc.c_str(), g_where.shape.c_str(),
                   g_where.launch, kind, layer, operand, ref, bytes, p);
}

// `nplanes` planes from plane0, frames [n0, n0 + N) of frame_bytes each; a plane must also hold those frames
void planes(const char* kind, int layer, const char* operand, const char* ref, const char* base, size_t plane_bytes, int plane0, int nplanes, size_t frame_bytes, int n0, int N,
            bool write = false) {
  if (nplanes > 0 && (size_t)(n0 + N) * frame_bytes > plane_bytes) {
    ++hc::g_violations;
    std::printf("VIOLATION %s | %s | launch %d (%s) layer %d | %s [%s] | frames [%d, %d) of %zu bytes do not fit a plane of %zu\n", g_where.desc.c_str(), g_where.shape.c_str(), g_where.launch,
                kind, layer, operand, ref, n0, n0 + N, frame_bytes, plane_bytes);
  }
  for (int k = 0; k < nplanes; ++k)
    need(kind, layer, operand, ref, base + (size_t)(plane0 + k) * plane_bytes + (size_t)n0 * frame_bytes, (size_t)N * frame_bytes, write);
}

void begin_launch(const char* kind = nullptr, int layer = -1, bool w16 = false) {
  ++hc::g_launches;
  if (hc::g_trace && kind) std::printf("LAUNCH %d %s layer %d%s\n", g_where.launch, kind, layer, w16 ? " w16" : "");
  if (hc::g_log) { g_cur.index = g_where.launch; g_cur.kind = kind ? kind : "?"; g_cur.layer = layer; g_cur.r.clear(); }
}
// in_place: the kernel is documented to write what it reads (none of the frame-recurrent launches is)
void end_launch(bool in_place = false) {
  if (hc::g_log) {
    // no written range overlaps a range the same launch reads
    if (!in_place)
      for (const hc::Range& w : g_cur.r) if (w.write)
        for (const hc::Range& r : g_cur.r) if (!r.write && w.p < r.p + r.bytes && r.p < w.p + w.bytes) report(g_cur.kind, g_cur.layer, w.operand, r.operand, "a written range overlaps a range the same launch reads");
    for (const hc::Range& w : g_cur.r) if (w.write) hc::cov_write(w.p, w.bytes);
    hc::g_launch_log.push_back(g_cur);
  }
  ++g_where.launch;
}

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
    planes(K, li, "out", "conv_mfma.hip:383,394-395,426-427,646", a.out, a.out_plane_bytes, a.out_plane0, out_planes, frame, a.n0, a.N, true);
  } else if (a.epi == EPI_NHWC_SUB2) {
    const size_t f2 = (size_t)((a.H + 1) / 2) * ((a.W + 1) / 2) * rec;
    planes(K, li, "out (stride 2)", "conv_mfma.hip:491,503-504,514,529-530", a.out, a.out_plane_bytes, a.out_plane0, out_planes, f2, a.n0, a.N, true);
  } else if (a.epi == EPI_NHWC_PS2) {
    const int cpb = (a.cout_real / 4) / 16;
    planes(K, li, "out (PixelShuffle 2)", "conv_mfma.hip:501-504,516,529-530", a.out, a.out_plane_bytes, a.out_plane0, cpb, 4 * frame, a.n0, a.N, true);
    if (a.res1) planes(K, li, "res1 (PixelShuffle 2)", "conv_mfma.hip:505,533-534", a.res1, a.r1_plane_bytes, a.r1_plane0, cpb, 4 * frame, a.n0, a.N);
  } else {  // EPI_NCHW_F32
    const size_t f32_frame = (size_t)a.cout_real * a.H * a.W * 4;
    need(K, li, "out (NCHW fp32)", "conv_mfma.hip:648-653", a.out + (size_t)a.n0 * f32_frame, (size_t)a.N * f32_frame, true);
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
    need(K, li, "out (NCHW fp32)", "conv_pair.hip:266", a.out + (size_t)a.n0 * f32_frame, (size_t)a.N * f32_frame, true);
  } else {
    planes(K, li, "out", "conv_pair.hip:272-274", a.out, a.out_plane_bytes, a.out_plane0, 2, frame, a.n0, a.N, true);
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
  planes(K, li, "out1", "conv_dense.hip:323,344", a.out1, a.out1_plane_bytes, a.out1_plane0, 2, frame, a.n0, a.N, true);
  planes(K, li, "out2", "conv_dense.hip:427,436", a.out2, a.out2_plane_bytes, a.out2_plane0, 2, frame, a.n0, a.N, true);
  end_launch();
}

void fsrcnn_forward(ss4k_ctx*, const FsrcnnWeights& W, int factor, const float* in, float* out, int n, int h, int w, float* ws12a, float* ws12b, int mode,
                    hipStream_t, bool out_half, bool in_u8) {
  begin_launch();
  const char* K = "fsrcnn";
  const size_t px = (size_t)n * h * w;
  need(K, -1, "in", "fsrcnn.hip fs_head (k_fs_head, k_fs_head_m)", in, px * (in_u8 ? 1 : 4));
  need(K, -1, "out", "fsrcnn.hip fs_tail (HR planes)", out, px * factor * factor * (out_half ? 2 : 4), true);
  // the two stage buffers: 12 channels per pixel, fp32 at most (the fp16 mode packs them tighter)
  need(K, -1, "ws12a", "models.cpp Model::forward_impl; fsrcnn.hip fs_head, fs_maps", ws12a, px * 12 * 4, true);
  need(K, -1, "ws12b", "models.cpp Model::forward_impl; fsrcnn.hip fs_maps", ws12b, px * 12 * 4, true);
  (void)mode;
  const char* L = "fsrcnn.h FsrcnnWeights";   // the layouts fsrcnn_pack_weights (fsrcnn_weights.cpp) produces
  need(K, -1, "w_feat", L, W.w_feat, 25 * 56 * 4); need(K, -1, "b_feat", L, W.b_feat, 56 * 4); need(K, -1, "a_feat", L, W.a_feat, 56 * 4);
  need(K, -1, "w_shrink", L, W.w_shrink, 56 * 12 * 4); need(K, -1, "b_shrink", L, W.b_shrink, 12 * 4); need(K, -1, "a_shrink", L, W.a_shrink, 12 * 4);
  for (int l = 0; l < 4; ++l) {
    need(K, -1, "w_map", L, W.w_map[l], 9 * 12 * 12 * 4); need(K, -1, "b_map", L, W.b_map[l], 12 * 4); need(K, -1, "a_map", L, W.a_map[l], 12 * 4);
  }
  need(K, -1, "w_expand", L, W.w_expand, 12 * 56 * 4); need(K, -1, "b_expand", L, W.b_expand, 56 * 4); need(K, -1, "a_expand", L, W.a_expand, 56 * 4);
  need(K, -1, "w_deconv", L, W.w_deconv, 81 * 56 * 4);
  end_launch();
}

template <typename T>
void op_pack_input(const float* in, T* out, int n, int c, int h, int w, int r, int nplanes, hipStream_t) {
  begin_launch(hc::g_log ? "pack_input" : nullptr);
  need("pack_input", -1, "in", "glue.hip:882", in, (size_t)n * c * h * w * 4);
  need("pack_input", -1, "out", "glue.hip:869,886", out, (size_t)nplanes * n * (h / r) * (w / r) * 16 * sizeof(T), true);
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
  need("ps_nchw_addbase", -1, "out", "glue.hip:935,941-942", out, px * cq * r * r * sizeof(HT), true);
  if (stats_acc) need("ps_nchw_addbase", -1, "stats_acc", "glue.hip:965,975", stats_acc, sizeof(double) * 2 * n * cq * STATS_SLOTS, true);
  end_launch();
}
template void op_ps_nchw_addbase<float, float>(const float*, float*, const float*, int, int, int, int, int, double*, hipStream_t);
template void op_ps_nchw_addbase<__half, float>(const __half*, float*, const float*, int, int, int, int, int, double*, hipStream_t);
template void op_ps_nchw_addbase<__half, __half>(const __half*, __half*, const float*, int, int, int, int, int, double*, hipStream_t);

void op_temporal_shift(const void* in, void* out, int nplanes, int frames, size_t frame_px, int slots_per_record, int, int, hipStream_t) {
  begin_launch();
  const size_t bytes = (size_t)nplanes * frames * frame_px * slots_per_record * 16;   // one thread per 16-byte slot, in[i + k] with 0 <= i + k < total
  need("temporal_shift", -1, "in", "glue.hip:1006-1007,1015", in, bytes);
  need("temporal_shift", -1, "out", "glue.hip:1006-1007,1016", out, bytes, true);
  end_launch();
}

// ---- the glue of the frame-recurrent upscaler (frvsr.hip) and of its service path (glue.hip).  Every auditor restates its launcher's
// SS4K_REQUIRE lines first: the executor meets the refusals the product meets, at the same place.
template <typename T>
void op_maxpool2_planes(const T* in, T* out, int nplanes, int n, int h, int w, hipStream_t) {
  SS4K_REQUIRE(nplanes > 0 && n > 0 && h >= 2 && w >= 2, "maxpool2: needs at least 2 x 2 pixels");   // op_maxpool2_planes (frvsr.hip)
  const char* K = "maxpool2_planes";
  begin_launch(K);
  const size_t rec = 16 * sizeof(T), ipx = (size_t)n * h * w, opx = (size_t)n * (h / 2) * (w / 2);
  // plane p reads pixels 2 oy, 2 oy + 1 x 2 ox, 2 ox + 1 of every image: up to ((n - 1) h + 2 (h / 2) - 1) w + 2 (w / 2) - 1 of its n h w
  const size_t last = ((size_t)(n - 1) * h + 2 * (size_t)(h / 2) - 1) * w + 2 * (size_t)(w / 2) - 1;
  for (int p = 0; p < nplanes; ++p) need(K, -1, "in", "frvsr.hip: k_maxpool2_planes", reinterpret_cast<const char*>(in) + (size_t)p * ipx * rec, (last + 1) * rec);
  need(K, -1, "out", "frvsr.hip: k_maxpool2_planes", out, (size_t)nplanes * opx * rec, true);
  end_launch();
}
template void op_maxpool2_planes<float>(const float*, float*, int, int, int, int, hipStream_t);
template void op_maxpool2_planes<__half>(const __half*, __half*, int, int, int, int, hipStream_t);

template <typename T>
void op_bilinear2_planes(const T* in, T* out, int nplanes, int n, int h, int w, hipStream_t) {
  SS4K_REQUIRE(nplanes > 0 && n > 0 && h > 0 && w > 0, "bilinear x2: empty tensor");   // op_bilinear2_planes (frvsr.hip)
  const char* K = "bilinear2_planes";
  begin_launch(K);
  const size_t rec = 16 * sizeof(T), ipx = (size_t)n * h * w;
  need(K, -1, "in", "frvsr.hip: k_bilinear2_planes", in, (size_t)nplanes * ipx * rec);           // rows and columns 0 .. size - 1 of every image
  need(K, -1, "out", "frvsr.hip: k_bilinear2_planes", out, (size_t)nplanes * ipx * 4 * rec, true);
  end_launch();
}
template void op_bilinear2_planes<float>(const float*, float*, int, int, int, int, hipStream_t);
template void op_bilinear2_planes<__half>(const __half*, __half*, int, int, int, int, hipStream_t);

void op_flow_finish(const float* raw, float* flow, int n, int h8, int w8, int h, int w, hipStream_t) {
  SS4K_REQUIRE(n > 0 && h8 >= 8 && w8 >= 8 && h >= h8 && w >= w8 && h - h8 < 8 && w - w8 < 8, "flow pad: sizes");   // op_flow_finish (frvsr.hip)
  const char* K = "flow_finish";
  begin_launch(K);
  need(K, -1, "raw", "frvsr.hip: k_flow_finish", raw, (size_t)n * 2 * h8 * w8 * 4);   // sy in [2 (h8 - 1) - (h - 1), h8): inside as h - h8 < 8 <= h8
  need(K, -1, "flow", "frvsr.hip: k_flow_finish", flow, (size_t)n * 2 * h * w * 4, true);
  end_launch();
}

// degradation 'BD' (frvsr.hip) and 'BI' (frvsr_bi.hip): the launchers are one launch helper and one kernel template (frvsr_stages.h) and differ in the
// flow's up-sampler alone, which reads the same (n, 2, h, w) flow; the warp, the records, the requirements and the grid are the same
template <typename T>
void warp_s2d(const char* K, const float* lr_flow, const float* hr_prev, T* out, int n, int h, int w) {
  SS4K_REQUIRE(n > 0 && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull, "warp: sizes");   // launch_warp_s2d (frvsr_stages.h), "<what>: sizes"
  begin_launch(K);
  const size_t hw = (size_t)h * w;
  need(K, -1, "lr_flow", "frvsr_stages.h: k_warp_s2d", lr_flow, (size_t)n * 2 * hw * 4);
  // a tap lies anywhere in [0, 4 h - 1] x [0, 4 w - 1] of the item's three colour planes (warp_pos clips)
  need(K, -1, "hr_prev", "frvsr_stages.h: k_warp_s2d", hr_prev, (size_t)n * 3 * 16 * hw * 4, false, n == 1 ? 0 : -1);
  need(K, -1, "out", "frvsr_stages.h: k_warp_s2d", out, (size_t)3 * n * hw * 16 * sizeof(T), true);
  end_launch();
}
template <typename T>
void warp_s2d_items(const char* K, const float* lr_flow, const FrvsrPtrs& hr_prev, T* out, int n, int h, int w) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull, "warp (items): sizes");   // launch_warp_s2d (frvsr_stages.h), "<what>: sizes"
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(hr_prev.p[i], "warp (items): NULL item");   // launch_warp_s2d (frvsr_stages.h), "<what>: NULL item"
  begin_launch(K);
  const size_t hw = (size_t)h * w;
  need(K, -1, "lr_flow", "frvsr_stages.h: k_warp_s2d", lr_flow, (size_t)n * 2 * hw * 4);
  for (int i = 0; i < n; ++i) need(K, -1, "hr_prev[i]", "frvsr_stages.h: k_warp_s2d", hr_prev.p[i], (size_t)3 * 16 * hw * 4, false, i);
  need(K, -1, "out", "frvsr_stages.h: k_warp_s2d", out, (size_t)3 * n * hw * 16 * sizeof(T), true);
  end_launch();
}
template <typename T> void op_warp_s2d_planes(const float* f, const float* hp, T* out, int n, int h, int w, hipStream_t) { warp_s2d("warp_s2d_planes", f, hp, out, n, h, w); }
template <typename T> void op_warp_s2d_bi_planes(const float* f, const float* hp, T* out, int n, int h, int w, hipStream_t) { warp_s2d("warp_s2d_bi_planes", f, hp, out, n, h, w); }
template <typename T> void op_warp_s2d_planes_items(const float* f, const FrvsrPtrs& hp, T* out, int n, int h, int w, hipStream_t) { warp_s2d_items("warp_s2d_planes(items)", f, hp, out, n, h, w); }
template <typename T> void op_warp_s2d_bi_planes_items(const float* f, const FrvsrPtrs& hp, T* out, int n, int h, int w, hipStream_t) { warp_s2d_items("warp_s2d_bi_planes(items)", f, hp, out, n, h, w); }
template void op_warp_s2d_planes<float>(const float*, const float*, float*, int, int, int, hipStream_t);
template void op_warp_s2d_planes<__half>(const float*, const float*, __half*, int, int, int, hipStream_t);
template void op_warp_s2d_bi_planes<float>(const float*, const float*, float*, int, int, int, hipStream_t);
template void op_warp_s2d_bi_planes<__half>(const float*, const float*, __half*, int, int, int, hipStream_t);
template void op_warp_s2d_planes_items<float>(const float*, const FrvsrPtrs&, float*, int, int, int, hipStream_t);
template void op_warp_s2d_planes_items<__half>(const float*, const FrvsrPtrs&, __half*, int, int, int, hipStream_t);
template void op_warp_s2d_bi_planes_items<float>(const float*, const FrvsrPtrs&, float*, int, int, int, hipStream_t);
template void op_warp_s2d_bi_planes_items<__half>(const float*, const FrvsrPtrs&, __half*, int, int, int, hipStream_t);

template <typename T>
void op_ps4_conv_tail(const T* in, const float* wb, float* out, int n, int h, int w, hipStream_t) {
  SS4K_REQUIRE(n > 0 && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull / 16, "tail: sizes");   // launch_ps4_conv_tail (frvsr_stages.h), "<what>: sizes"
  const char* K = "ps4_conv_tail";
  begin_launch(K);
  const size_t hw = (size_t)h * w;
  need(K, -1, "in", "frvsr_stages.h: k_ps4_conv_tail", in, (size_t)4 * n * hw * 16 * sizeof(T));   // planes 0..3, every pixel's 16 sub-pixel elements
  need(K, -1, "wb", "frvsr_stages.h: k_ps4_conv_tail", wb, 111 * 4);
  need(K, -1, "out", "frvsr_stages.h: k_ps4_conv_tail", out, (size_t)n * 3 * 16 * hw * 4, true, n == 1 ? 0 : -1);
  end_launch();
}
template void op_ps4_conv_tail<float>(const float*, const float*, float*, int, int, int, hipStream_t);
template void op_ps4_conv_tail<__half>(const __half*, const float*, float*, int, int, int, hipStream_t);

template <typename T>
void op_ps4_conv_tail_items(const T* in, const float* wb, const FrvsrPtrs& out, int n, int h, int w, hipStream_t) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull / 16, "tail (items): sizes");   // launch_ps4_conv_tail (frvsr_stages.h), "<what>: sizes"
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(out.p[i], "tail (items): NULL item");   // launch_ps4_conv_tail (frvsr_stages.h), "<what>: NULL item"
  const char* K = "ps4_conv_tail(items)";
  begin_launch(K);
  const size_t hw = (size_t)h * w;
  need(K, -1, "in", "frvsr_stages.h: k_ps4_conv_tail", in, (size_t)4 * n * hw * 16 * sizeof(T));
  need(K, -1, "wb", "frvsr_stages.h: k_ps4_conv_tail", wb, 111 * 4);
  for (int i = 0; i < n; ++i) need(K, -1, "out[i]", "frvsr_stages.h: k_ps4_conv_tail", out.p[i], (size_t)3 * 16 * hw * 4, true, i);
  end_launch();
}
template void op_ps4_conv_tail_items<float>(const float*, const float*, const FrvsrPtrs&, int, int, int, hipStream_t);
template void op_ps4_conv_tail_items<__half>(const __half*, const float*, const FrvsrPtrs&, int, int, int, hipStream_t);

// TecoGAN's skip: out = conv + x4 up-sampling of lr, bicubic (frvsr.hip) or bilinear (frvsr_bi.hip) through launch_x4_add: every tap is clamped into the
// item's (3, h, w) planes, conv and out are read and written element by element
void x4_add(const char* K, const float* conv, const float* lr, float* out, int n, int h, int w) {
  SS4K_REQUIRE(n > 0 && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull / 16, "x4_add: sizes");   // launch_x4_add (frvsr_stages.h), "<what>: sizes"
  begin_launch(K);
  const size_t hw = (size_t)h * w;
  need(K, -1, "conv", "frvsr_stages.h: k_x4_add", conv, (size_t)n * 48 * hw * 4);
  need(K, -1, "lr", "frvsr_stages.h: k_x4_add", lr, (size_t)n * 3 * hw * 4, false, n == 1 ? 0 : -1);
  need(K, -1, "out", "frvsr_stages.h: k_x4_add", out, (size_t)n * 48 * hw * 4, true, n == 1 ? 0 : -1);
  end_launch();
}
void x4_add_items(const char* K, const float* conv, const FrvsrPtrs& lr, const FrvsrPtrs& out, int n, int h, int w) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && h > 0 && w > 0 && (size_t)n * h * w < 2147483648ull / 16, "x4_add (items): sizes");   // launch_x4_add (frvsr_stages.h), "<what>: sizes"
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(lr.p[i] && out.p[i], "x4_add (items): NULL item");   // launch_x4_add (frvsr_stages.h), "<what>: NULL item"
  begin_launch(K);
  const size_t hw = (size_t)h * w;
  need(K, -1, "conv", "frvsr_stages.h: k_x4_add", conv, (size_t)n * 48 * hw * 4);
  for (int i = 0; i < n; ++i) {
    need(K, -1, "lr[i]", "frvsr_stages.h: k_x4_add", lr.p[i], 3 * hw * 4, false, i);
    need(K, -1, "out[i]", "frvsr_stages.h: k_x4_add", out.p[i], 48 * hw * 4, true, i);
  }
  end_launch();
}
void op_bicubic4_add(const float* conv, const float* lr, float* out, int n, int h, int w, hipStream_t) { x4_add("bicubic4_add", conv, lr, out, n, h, w); }
void op_bilinear4_add(const float* conv, const float* lr, float* out, int n, int h, int w, hipStream_t) { x4_add("bilinear4_add", conv, lr, out, n, h, w); }
void op_bicubic4_add_items(const float* conv, const FrvsrPtrs& lr, const FrvsrPtrs& out, int n, int h, int w, hipStream_t) { x4_add_items("bicubic4_add(items)", conv, lr, out, n, h, w); }
void op_bilinear4_add_items(const float* conv, const FrvsrPtrs& lr, const FrvsrPtrs& out, int n, int h, int w, hipStream_t) { x4_add_items("bilinear4_add(items)", conv, lr, out, n, h, w); }

// ConvTranspose2d(64, 64, 3, 2, 1, output_padding=1) + bias + ReLU by output phase (conv_up2.hip): four planes at (N, H, W) -> four at (N, 2 H, 2 W)
void launch_convt3x3s2(ss4k_ctx*, const ConvtArgs& a, int dtype, int, hipStream_t) {
  SS4K_REQUIRE(a.N > 0 && a.H > 0 && a.W > 0 && (double)a.N * 4.0 * a.H * a.W < 2147483648.0, "convt3x3s2: sizes");   // conv_up2.hip: conv_up2.hip:178
  const char* K = "convt3x3s2";
  begin_launch(K);
  const size_t rec = conv_rec_bytes(dtype), px = (size_t)a.N * a.H * a.W;
  // the halo tile reads pixels (y, x), y < H, x < W of every item (row H and column W are zero-filled, not read)
  planes(K, -1, "in", "conv_up2.hip:87-88", a.in, a.in_plane_bytes, 0, 4, px * rec, 0, 1);
  need(K, -1, "w", "conv_up2.hip:72-73 (pack.cpp: pack_convt3x3s2)", a.w, (size_t)64 * 64 * 9 * (dtype == SS4K_F16 ? 2 : 4));
  need(K, -1, "bias", "conv_up2.hip:147", a.bias, 64 * 4);
  planes(K, -1, "out", "conv_up2.hip:157-163", a.out, a.out_plane_bytes, 0, 4, 4 * px * rec, 0, 1, true);
  end_launch();
}

template <typename T>
void op_planes_to_nchw(const T* in, float* out, int n, int channels, int h, int w, hipStream_t) {
  const char* K = "planes_to_nchw";
  begin_launch(K);
  const size_t npix = (size_t)n * h * w;
  need(K, -1, "in", "frvsr.hip: k_planes_to_nchw", in, (size_t)((channels + 15) / 16) * npix * 16 * sizeof(T));
  need(K, -1, "out", "frvsr.hip: k_planes_to_nchw", out, npix * channels * 4, true);
  end_launch();
}
template void op_planes_to_nchw<float>(const float*, float*, int, int, int, int, hipStream_t);
template void op_planes_to_nchw<__half>(const __half*, float*, int, int, int, int, hipStream_t);

void op_clamp01_to(const float* in, float* out, size_t n, hipStream_t) {
  const char* K = "clamp01_to";
  begin_launch(K);
  need(K, -1, "in", "frvsr.hip: k_clamp01_to", in, n * 4);
  need(K, -1, "out", "frvsr.hip: k_clamp01_to", out, n * 4, true);
  end_launch();
}

void op_frames_in_items(const FrvsrFramesIn& in, const FrvsrPtrs& lr_curr, int n, int h, int w, int lh, int lw, hipStream_t) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && h > 0 && w > 0 && lh > 0 && lw > 0, "frames in (items): sizes");   // op_frames_in_items (frvsr.hip)
  SS4K_REQUIRE((double)h * lh < 2147483648.0 && (double)w * lw < 2147483648.0, "frames in (items): a window bound would overflow");   // op_frames_in_items (frvsr.hip)
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(in.p[i] && lr_curr.p[i], "frames in (items): NULL item");   // op_frames_in_items (frvsr.hip)
  const char* K = "frames_in(items)";
  begin_launch(K);
  for (int i = 0; i < n; ++i) {
    // the windows [floor(i h / lh), ceil((i + 1) h / lh)) cover rows 0 .. h - 1 whichever of h, lh is larger (area_lo / area_hi)
    need(K, -1, "in[i]", "frvsr.hip: k_frames_in_items", in.p[i], (size_t)h * w * 3, false, i);
    need(K, -1, "lr_curr[i]", "frvsr.hip: k_frames_in_items", lr_curr.p[i], (size_t)3 * lh * lw * 4, true, i);
  }
  end_launch();
}

template <typename T>
void op_pack_lr_items(const FrvsrPtrs& lr_curr, const FrvsrPtrs& lr_prev, T* a, T* b, int n, int h, int w, hipStream_t) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && h > 0 && w > 0 && a && b, "pack (items): sizes");   // op_pack_lr_items (frvsr.hip)
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(lr_curr.p[i] && lr_prev.p[i], "pack (items): NULL item");   // op_pack_lr_items (frvsr.hip)
  const char* K = "pack_lr(items)";
  begin_launch(K);
  const size_t hw = (size_t)h * w;
  for (int i = 0; i < n; ++i) {
    need(K, -1, "lr_curr[i]", "frvsr.hip: k_pack_lr_items", lr_curr.p[i], 3 * hw * 4, false, i);
    need(K, -1, "lr_prev[i]", "frvsr.hip: k_pack_lr_items", lr_prev.p[i], 3 * hw * 4, false, i);
  }
  need(K, -1, "a", "frvsr.hip: k_pack_lr_items", a, (size_t)n * hw * 16 * sizeof(T), true);
  need(K, -1, "b", "frvsr.hip: k_pack_lr_items", b, (size_t)n * hw * 16 * sizeof(T), true);
  end_launch();
}
template void op_pack_lr_items<float>(const FrvsrPtrs&, const FrvsrPtrs&, float*, float*, int, int, int, hipStream_t);
template void op_pack_lr_items<__half>(const FrvsrPtrs&, const FrvsrPtrs&, __half*, __half*, int, int, int, hipStream_t);

void op_frames_out_items(const FrvsrPtrs& hr, const FrvsrFramesOut& out, int n, int H, int W, int oh, int ow, hipStream_t) {
  SS4K_REQUIRE(n > 0 && n <= SS4K_FRVSR_MAX_STREAMS && H > 0 && W > 0 && oh > 0 && ow > 0, "frames out (items): sizes");   // op_frames_out_items (frvsr.hip)
  SS4K_REQUIRE((double)H * oh < 2147483648.0 && (double)W * ow < 2147483648.0, "frames out (items): a window bound would overflow");   // op_frames_out_items (frvsr.hip)
  for (int i = 0; i < n; ++i) SS4K_REQUIRE(hr.p[i] && out.p[i], "frames out (items): NULL item");   // op_frames_out_items (frvsr.hip)
  const char* K = "frames_out(items)";
  begin_launch(K);
  for (int i = 0; i < n; ++i) {
    need(K, -1, "hr[i]", "frvsr.hip: k_frames_out_items", hr.p[i], (size_t)3 * H * W * 4, false, i);
    // groups of four pixels, twelve bytes each, the last group cut at oh * ow pixels: 4-byte stores only in whole groups
    need(K, -1, "out[i]", "frvsr.hip: k_frames_out_items", out.p[i], (size_t)oh * ow * 3, true, i);
  }
  end_launch();
}

void op_u8nhwc_to_f32nchw(const uint8_t* in, float* out, int n, int h, int w, int c, hipStream_t) {
  const char* K = "u8nhwc_to_f32nchw";
  begin_launch(K);
  need(K, -1, "in", "glue.hip:76", in, (size_t)n * h * w * c);
  need(K, -1, "out", "glue.hip:76", out, (size_t)n * c * h * w * 4, true);
  end_launch();
}

void op_area(const float* in, float* out, int planes, int h, int w, int oh, int ow, hipStream_t) {
  const bool same = h == oh && w == ow;   // a device-to-device copy in the product (glue.hip:151-154)
  if (!same) SS4K_REQUIRE(oh <= 65535 && planes <= 65535, "area: grid limits");   // glue.hip:156
  const char* K = same ? "area(identity)" : "area";
  begin_launch(K);
  // the windows cover every row and column of the source (glue.hip:86-87,97-104; the whole-number route reads ky rows of KX columns: :117-125)
  need(K, -1, "in", "glue.hip:98,104,117,125,153", in, (size_t)planes * h * w * 4);
  need(K, -1, "out", "glue.hip:99,105,118,130,153", out, (size_t)planes * oh * ow * 4, true);
  end_launch();
}

void op_f32nchw_to_u8nhwc(const float* in, uint8_t* out, int n, int c, int h, int w, hipStream_t) {
  const char* K = "f32nchw_to_u8nhwc";
  begin_launch(K);
  need(K, -1, "in", "glue.hip:849", in, (size_t)n * c * h * w * 4);
  need(K, -1, "out", "glue.hip:851", out, (size_t)n * h * w * c, true);
  end_launch();
}

// ---- the rest of the service glue (glue.hip), as upscaler.cpp uses it.  The statistics accumulators really change: a partial sum leaves 1.0
// in every entry it adds to and the rezeroing finish leaves 0.0, so that the walk can look at the bytes st_acc2 holds after a job.
size_t stats_slots_used(int hw) { return (size_t)std::min(std::max(1, std::min((hw + 256 * 16 - 1) / (256 * 16), 128)), STATS_SLOTS); }   // glue.hip:219,261-262: blockIdx.x % STATS_SLOTS
void stats_acc(const char* K, const char* ref, double* acc, int hw, int acc_planes, int plane0, int planes) {
  for (size_t sl = 0; sl < stats_slots_used(hw); ++sl) {
    double* a = acc + (sl * acc_planes + plane0) * 2;
    const size_t before = hc::g_violations;
    need(K, -1, "acc (read)", ref, a, (size_t)planes * 16);
    need(K, -1, "acc", ref, a, (size_t)planes * 16, true);
    if (before == (size_t)hc::g_violations) for (int i = 0; i < 2 * planes; ++i) a[i] = 1.0;
  }
}
template <typename HT>
void op_plane_stats_partial(double* acc, const HT* in, int planes, int hw, int acc_planes, int plane0, hipStream_t) {
  const char* K = "stats_partial";
  begin_launch(K);
  need(K, -1, "in", "glue.hip:180,191,200,208", in, (size_t)planes * hw * sizeof(HT));
  stats_acc(K, "glue.hip:219-221", acc, hw, acc_planes, plane0, planes);
  end_launch(true);   // atomic adds: in place
}
template void op_plane_stats_partial<float>(double*, const float*, int, int, int, int, hipStream_t);
template void op_plane_stats_partial<__half>(double*, const __half*, int, int, int, int, hipStream_t);
void op_plane_stats_u8nhwc_partial(double* acc, const uint8_t* in, int n, int hw, int acc_planes, int plane0, hipStream_t) {
  const char* K = "stats_partial_u8";
  begin_launch(K);
  need(K, -1, "in", "glue.hip:272,282,291", in, (size_t)n * hw * 3);
  stats_acc(K, "glue.hip:305-307", acc, hw, acc_planes, plane0, 3 * n);
  end_launch(true);
}
void op_plane_stats_finish(const double* acc, float* stats, int planes, int hw, hipStream_t) {
  const char* K = "stats_final";
  begin_launch(K);
  need(K, -1, "acc", "glue.hip:228", acc, (size_t)STATS_SLOTS * planes * 16);
  need(K, -1, "stats", "glue.hip:233-234", stats, (size_t)planes * 8, true);
  end_launch();
}
template <typename HT>
void op_plane_stats(double* acc, const HT* in, float* stats, int planes, int hw, hipStream_t st) {
  SS4K_REQUIRE(planes <= STATS_MAX_PLANES, "plane_stats: too many planes");                     // glue.hip:259
  SS4K_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 2 * planes * STATS_SLOTS, st));             // glue.hip:260
  op_plane_stats_partial<HT>(acc, in, planes, hw, planes, 0, st);                               // glue.hip:264 (acc_planes = gridDim.y)
  op_plane_stats_finish(acc, stats, planes, hw, st);
}
template void op_plane_stats<float>(double*, const float*, float*, int, int, hipStream_t);
template void op_plane_stats<__half>(double*, const __half*, float*, int, int, hipStream_t);
void op_plane_stats_u8nhwc(double* acc, const uint8_t* in, float* stats, int n, int hw, hipStream_t st) {
  SS4K_REQUIRE(3 * n <= STATS_MAX_PLANES, "plane_stats: too many planes");                      // glue.hip:312
  SS4K_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 2 * 3 * n * STATS_SLOTS, st));              // glue.hip:313
  op_plane_stats_u8nhwc_partial(acc, in, n, hw, 3 * n, 0, st);
  op_plane_stats_finish(acc, stats, 3 * n, hw, st);
}
void op_plane_stats_finish2(double* acc, float* stats_a, float* stats_b, int planes, int hw_a, int hw_b, bool rezero, hipStream_t) {
  const char* K = "stats_final2";
  begin_launch(K);
  const size_t bytes = (size_t)STATS_SLOTS * 2 * planes * 16;   // slot s, plane p < 2 planes: (s * 2 planes + p) * 2 doubles (glue.hip:342)
  const size_t before = hc::g_violations;
  need(K, -1, "acc (read)", "glue.hip:342-343", acc, bytes);
  if (rezero) need(K, -1, "acc", "glue.hip:345", acc, bytes, true);
  need(K, -1, "stats_a", "glue.hip:351-353", stats_a, (size_t)planes * 8, true);
  need(K, -1, "stats_b", "glue.hip:351-353", stats_b, (size_t)planes * 8, true);
  if (rezero && before == (size_t)hc::g_violations) std::memset(acc, 0, bytes);
  end_launch(true);   // the rezeroing finish writes what it has read
}

template <typename HT>
void op_area_normalized(const HT* in, float* out, int planes, int h, int w, int oh, int ow, const float* st_hr, const float* st_lr, hipStream_t) {
  SS4K_REQUIRE(oh <= 65535 && planes <= 65535, "area: grid limits");   // glue.hip:164
  const char* K = "area_normalized";
  begin_launch(K);
  need(K, -1, "in", "glue.hip:98,104,117,125", in, (size_t)planes * h * w * sizeof(HT));
  need(K, -1, "st_hr", "glue.hip:96,116", st_hr, (size_t)planes * 8);
  need(K, -1, "st_lr", "glue.hip:96,116", st_lr, (size_t)planes * 8);
  need(K, -1, "out", "glue.hip:99,105,118,130", out, (size_t)planes * oh * ow * 4, true);
  end_launch();
}
template void op_area_normalized<float>(const float*, float*, int, int, int, int, int, const float*, const float*, hipStream_t);
template void op_area_normalized<__half>(const __half*, float*, int, int, int, int, int, const float*, const float*, hipStream_t);

template <typename HT>
void op_tail_fused(HT* hr, uint8_t* out_u8, const float* diff, int n, int c, int h, int w, int dh, int dw, const float* st_hr, const float* st_lr, hipStream_t) {
  SS4K_REQUIRE(h <= 65535 && n <= 65535, "fused tail: grid limits");   // glue.hip:644
  const char* K = "tail_fused";
  begin_launch(K);
  const size_t px = (size_t)n * c * h * w;
  need(K, -1, "hr", "glue.hip:571-572,610-611", hr, px * sizeof(HT));
  if (st_hr) { need(K, -1, "st_hr", "glue.hip:573,614", st_hr, (size_t)n * c * 8); need(K, -1, "st_lr", "glue.hip:573,614", st_lr, (size_t)n * c * 8); }
  if (diff) need(K, -1, "diff", "glue.hip:575-576,616,621", diff, (size_t)n * c * dh * dw * 4);   // rows y0, y1 < dh, columns x0, x1 < dw of every plane
  if (out_u8) need(K, -1, "out", "glue.hip:580,636-637", out_u8, px, true);
  else need(K, -1, "hr (in place)", "glue.hip:581,627", hr, px * sizeof(HT), true);
  end_launch(true);   // "else write the clamped float back in place" (glue.hip:555)
}
template void op_tail_fused<float>(float*, uint8_t*, const float*, int, int, int, int, int, int, const float*, const float*, hipStream_t);
template void op_tail_fused<__half>(__half*, uint8_t*, const float*, int, int, int, int, int, int, const float*, const float*, hipStream_t);

template <typename HT>
void op_bicubic_u8(const HT* in, uint8_t* out, int n, int c, int h, int w, int oh, int ow, hipStream_t) {
  SS4K_REQUIRE(oh <= 65535 && n <= 65535, "bicubic: grid limits");   // glue.hip:768
  const char* K = "bicubic_u8";
  begin_launch(K);
  need(K, -1, "in", "glue.hip:693,700,702-707,737,741-747", in, (size_t)n * c * h * w * sizeof(HT));   // rows and columns clamped to the plane
  need(K, -1, "out", "glue.hip:710,762-763", out, (size_t)n * oh * ow * c, true);
  end_launch();
}
template void op_bicubic_u8<float>(const float*, uint8_t*, int, int, int, int, int, int, hipStream_t);
template void op_bicubic_u8<__half>(const __half*, uint8_t*, int, int, int, int, int, int, hipStream_t);

void op_normalize(float* x, const float* st_hr, const float* st_lr, int planes, int hw, hipStream_t) {
  const char* K = "normalize";
  begin_launch(K);
  need(K, -1, "x", "glue.hip:370-372", x, (size_t)planes * hw * 4);
  need(K, -1, "st_hr", "glue.hip:369", st_hr, (size_t)planes * 8);
  need(K, -1, "st_lr", "glue.hip:369", st_lr, (size_t)planes * 8);
  need(K, -1, "x (in place)", "glue.hip:372", x, (size_t)planes * hw * 4, true);
  end_launch(true);
}

void op_depthwise_reflect(const float* in, float* out, const float* taps_dev, int planes, int h, int w, int k, int clamp01, const float* blend_src, float, float, hipStream_t) {
  SS4K_REQUIRE(h <= 65535 && planes <= 65535, "depthwise: grid limits");                                                                   // glue.hip:409
  SS4K_REQUIRE(k == 3 || k == 17, "depthwise: kernel size 3 or 17 (the service's sharpen / blur kernels)");                                // glue.hip:410
  SS4K_REQUIRE(h > k / 2 && w > k / 2, "depthwise reflect: padding (k/2) must be smaller than the plane, as torch requires");             // glue.hip:412
  const char* K = "depthwise_reflect";
  begin_launch(K);
  (void)clamp01;
  need(K, -1, "in", "glue.hip:381,394,398-400", in, (size_t)planes * h * w * 4);   // reflect(i, n) in [0, n) for -n < i < 2 n - 1
  need(K, -1, "taps", "glue.hip:400", taps_dev, (size_t)k * k * 4);
  if (blend_src) need(K, -1, "blend_src", "glue.hip:403", blend_src, (size_t)planes * h * w * 4);
  need(K, -1, "out", "glue.hip:404", out, (size_t)planes * h * w * 4, true);
  end_launch();
}

void op_gauss17_reflect(const float* in, float* tmp, float* out, const float* g17_dev, int planes, int h, int w, hipStream_t) {
  SS4K_REQUIRE(h <= 65535 && planes <= 65535, "gauss17: grid limits");                                                             // glue.hip:445
  SS4K_REQUIRE(h > 8 && w > 8, "gauss17 reflect: padding (8) must be smaller than the plane, as torch requires");                 // glue.hip:446
  const size_t b = (size_t)planes * h * w * 4;
  for (int pass = 0; pass < 2; ++pass) {
    const char* K = pass ? "gauss17(vertical)" : "gauss17(horizontal)";
    begin_launch(K);
    need(K, -1, "in", "glue.hip:431,440", pass ? tmp : in, b);
    need(K, -1, "g", "glue.hip:435", g17_dev, 17 * 4);
    need(K, -1, "out", "glue.hip:432,441", pass ? out : tmp, b, true);
    end_launch();
  }
}

void op_bilinear(const float* in, float* out, int planes, int h, int w, int oh, int ow, int subtract_from_out, int, hipStream_t) {
  SS4K_REQUIRE(oh <= 65535 && planes <= 65535, "bilinear: grid limits");   // glue.hip:489
  const char* K = "bilinear";
  begin_launch(K);
  need(K, -1, "in", "glue.hip:460,463-465,476-478", in, (size_t)planes * h * w * 4);
  if (subtract_from_out) need(K, -1, "out (read)", "glue.hip:469-470", out, (size_t)planes * oh * ow * 4);
  need(K, -1, "out", "glue.hip:461,483-484", out, (size_t)planes * oh * ow * 4, true);
  end_launch(subtract_from_out != 0);
}

void op_bicubic(const float* in, float* out, int planes, int h, int w, int oh, int ow, int, hipStream_t) {
  SS4K_REQUIRE(oh <= 65535 && planes <= 65535, "bicubic: grid limits");   // glue.hip:545
  const char* K = "bicubic";
  begin_launch(K);
  need(K, -1, "in", "glue.hip:521,529,536,539", in, (size_t)planes * h * w * 4);
  need(K, -1, "out", "glue.hip:522,541", out, (size_t)planes * oh * ow * 4, true);
  end_launch();
}

void op_sub(const float* a, const float* b, float* out, size_t n, hipStream_t) {
  const char* K = "sub";
  begin_launch(K);
  need(K, -1, "a", "glue.hip:783", a, n * 4); need(K, -1, "b", "glue.hip:783", b, n * 4);
  need(K, -1, "out", "glue.hip:783", out, n * 4, true);
  end_launch();
}
void op_clamp01(float* x, size_t n, hipStream_t) {
  const char* K = "clamp01";
  begin_launch(K);
  need(K, -1, "x", "glue.hip:791", x, n * 4);
  need(K, -1, "x (in place)", "glue.hip:791", x, n * 4, true);
  end_launch(true);
}

void op_lane_spin(unsigned, hipStream_t) {}

}  // namespace ss4k
