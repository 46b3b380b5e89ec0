// FSRCNN's weight blob: the reference's state_dict (src/upscale/model/fsrcnn/model.py) in the layouts of FsrcnnWeights (fsrcnn.h), scaled
// for the matrix-core modes' one-fma PReLU where the checkpoint allows it.
#include "models.h"
#include <cmath>

namespace ss4k {

namespace {

// the seven conv + PReLU layers in state_dict order; the ConvTranspose follows them
enum { L_FEAT = 0, L_SHRINK, L_MAP0, L_EXPAND = L_MAP0 + 4, LAYERS };
struct LayerShape { int cout, cin, taps; };
constexpr LayerShape SHAPE[LAYERS] = {{56, 1, 25}, {12, 56, 1}, {12, 12, 9}, {12, 12, 9}, {12, 12, 9}, {12, 12, 9}, {56, 12, 1}};
// where the blob holds them: weights [tap][cin][cout], bias [cout], PReLU slope [cout]; every array starts at a multiple of four floats
struct LayerAt { size_t w, b, a; };
struct BlobAt { LayerAt layer[LAYERS]; size_t w_deconv; };   // w_deconv: [tap][cin]

}  // namespace

size_t fsrcnn_pack_weights(ParamCursor& pc, bool& exact, DevBuf& dev, FsrcnnWeights& W) {
  std::vector<float> blob;
  auto push = [&](const float* p, size_t k) { const size_t o = blob.size(); blob.insert(blob.end(), p, p + k); while (blob.size() % 4) blob.push_back(0.f); return o; };
  BlobAt at{};
  for (int l = 0; l < LAYERS; ++l) {
    const int co = SHAPE[l].cout, ci = SHAPE[l].cin, k2 = SHAPE[l].taps;
    const float* p = pc.take((size_t)co * ci * k2);   // OIHW -> [tap][ci][co]
    std::vector<float> t((size_t)k2 * ci * co);
    for (int a = 0; a < co; ++a) for (int b = 0; b < ci; ++b) for (int k = 0; k < k2; ++k)
      t[((size_t)k * ci + b) * co + a] = p[((size_t)a * ci + b) * k2 + k];
    at.layer[l].w = push(t.data(), t.size());
    at.layer[l].b = push(pc.take(co), co);
    at.layer[l].a = push(pc.take(co), co);
  }
  {
    const float* p = pc.take(56 * 81);  // ConvTranspose weight (C_in=56, C_out=1, 9, 9) -> [tap][cin]
    std::vector<float> wd(81 * 56);
    for (int c = 0; c < 56; ++c) for (int t = 0; t < 81; ++t) wd[(size_t)t * 56 + c] = p[(size_t)c * 81 + t];
    at.w_deconv = push(wd.data(), wd.size());
  }
  W.b_deconv = *pc.take(1);
  W.prelu_abs = false;
  // Matrix-core modes: PReLU(x) = a x + b |x| with a = (1 + s) / 2, b = (1 - s) / 2.  The weights and the bias that PRODUCE a channel are
  // scaled by its a here, so the kernels' accumulators hold y = a x, and PReLU(x) = y + c |y| with c = b / a = (1 - s) / (1 + s) - one fma
  // with a free |.| modifier per value (fsrcnn.hip prelu_mx).  The slope arrays of the blob hold c.  Needs a > 0, i.e. s > -1, for every
  // channel (real checkpoints: T91 x2 0.0 .. 1.04, x4 up to 9.1); a slope at or below -1 + 1/8 - where c would exceed 15 and the scaled
  // weights lose their bits - sends the model to the exact kernels.
  for (int l = 0; l < LAYERS && !exact; ++l)
    for (int c = 0; c < SHAPE[l].cout; ++c) if (!(blob[at.layer[l].a + c] > -0.875f)) exact = true;
  if (!exact) {   // (both matrix-core modes: fp16 and fp32-grade)
    std::vector<float> scaled = blob;
    float* B = scaled.data();
    for (int l = 0; l < LAYERS; ++l) {
      const int co = SHAPE[l].cout, per_channel = SHAPE[l].cin * SHAPE[l].taps;   // a channel's producing weights: co apart, first at w + channel
      for (int c = 0; c < co; ++c) {
        const float sl = B[at.layer[l].a + c], sa = 0.5f * (1.f + sl);
        for (int i = 0; i < per_channel; ++i) B[at.layer[l].w + c + (size_t)i * co] *= sa;
        B[at.layer[l].b + c] *= sa;
        B[at.layer[l].a + c] = (1.f - sl) / (1.f + sl);
      }
    }
    // The fp16 hi/lo split (fsrcnn.hip split2) needs every operand inside the fp16 range: |x| < 65504 (below 2^-14 the hi part is an fp16
    // subnormal and the lo part makes up the difference, absolute error < 2^-24 |w|).  Checked on what the kernels get - every scaled weight
    // and bias (the scaling multiplies by up to (1 + s) / 2: x 5.05 on the T91 x4 checkpoint's s = 9.1), the slopes' c, the tail's weights and
    // bias; a checkpoint that does not fit runs the exact-fp32 kernels, which take the unscaled layout.  Activations of an image-range
    // network are orders of magnitude inside (T91: < 120 for inputs in [0,1], tests/test_oracle_golden.py::test_fsrcnn_t91_activation_range),
    // and SS4K_MODEL_FS_EXACT is the caller's switch for a network that is not.
    bool fits = std::fabs(W.b_deconv) < 6.0e4f;
    for (float v : scaled) fits = fits && std::fabs(v) < 6.0e4f;
    if (fits) { blob.swap(scaled); W.prelu_abs = true; }
    else exact = true;
  }
  const size_t bytes = blob.size() * 4;
  dev.ensure(std::max<size_t>(bytes, 16));
  SS4K_HIP(hipMemcpy(dev.ptr, blob.data(), bytes, hipMemcpyHostToDevice));
  const float* d = dev.as<float>();
  auto point = [&](int l, const float*& w, const float*& b, const float*& a) { w = d + at.layer[l].w; b = d + at.layer[l].b; a = d + at.layer[l].a; };
  point(L_FEAT, W.w_feat, W.b_feat, W.a_feat);
  point(L_SHRINK, W.w_shrink, W.b_shrink, W.a_shrink);
  for (int l = 0; l < 4; ++l) point(L_MAP0 + l, W.w_map[l], W.b_map[l], W.a_map[l]);
  point(L_EXPAND, W.w_expand, W.b_expand, W.a_expand);
  W.w_deconv = d + at.w_deconv;
  return bytes;
}

}  // namespace ss4k
