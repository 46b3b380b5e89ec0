// Walks the lattice of model descriptions the library accepts ("Host check"): every accepted description is built from a
// generated weight blob and run through workspace_bytes and a real forward for every shape, with the launch auditors
// (auditors.cpp) in place of the kernels; every invalid description must be refused with SS4K_EINVAL.  Then the shape space of the
// frame-recurrent upscaler (frvsr.cpp: FRNet descriptions, Frvsr::step / step_items, FrvsrUpscaler rounds) and of the frame upscaler
// (upscaler.cpp: Upscaler::multi / single), every launch recorded with what it read and wrote.  Built with ASan + UBSan.
//
//   hostcheck                      the whole walk; prints one HOSTCHECK line with the counts, exit status 1 on any finding
//   hostcheck --shard I N          every N-th point of every walk from the I-th (shard 0 also takes the invalid descriptions and the tables)
//   hostcheck --only PART          rrdbnet | srvgg | bsvd | bounds | fsrcnn | invalid | tables | frvsr-descs | frvsr-steps | frvsr-rounds | upscaler | variants (for measuring)
//   hostcheck --trace kind dtype scale num_feat num_block num_grow_ch c0 c1 c2 mid_ch interm_ch stream flags frames H W
//                                  one line per launch of that description at that layer-resolution shape (which route a width takes)
//   hostcheck --control-shrink I   positive control: one RRDBNet forward with activation buffer I registered one plane short
//   hostcheck --control-short-blob positive control: a blob one float short must be refused with SS4K_EINVAL
//   hostcheck --trace-frvsr dtype num_block n h w [generator degradation route_flags]
//                                  one line per launch of one step through each of its three input-packing routes (default: EGVSR, 'BD', 0)
//   hostcheck --control-frvsr hr-short | out-short | cur | teco-hr-short
//                                  positive controls of the round walk: a slot's hr buffer registered 4 bytes short (teco-: on a TecoGAN / 'BI'
//                                  upscaler), a caller's output frame one byte short, a slot's `cur` not flipped after a round (a hook of this
//                                  program, not of the product)
#include "hostcheck.h"
#include "../../sharkshark-4k_amd/csrc/frvsr.h"
#include "../../sharkshark-4k_amd/csrc/upscaler.h"
#include "../../sharkshark-4k_amd/csrc/host_tables.h"
#include <array>
#include <chrono>
#include <climits>
#include <cmath>
#include <map>
#include <memory>

using namespace ss4k;

namespace {

long g_accepted = 0, g_refused = 0, g_shapes = 0, g_findings = 0, g_bij_layers = 0;
double g_weights = 0;   // parameters packed so far (what the wall time goes with)

void finding(const std::string& what) { ++g_findings; std::printf("FINDING %s\n", what.c_str()); }

std::string desc_str(const ss4k_model_desc& d) {
  char b[256];
  std::snprintf(b, sizeof b, "kind %d dtype %d scale %d nf %d nb %d g %d chns %d,%d,%d mid %d interm %d stream %d flags %d", d.kind, d.dtype, d.scale, d.num_feat, d.num_block,
                d.num_grow_ch, d.bsvd_chns[0], d.bsvd_chns[1], d.bsvd_chns[2], d.bsvd_mid_ch, d.bsvd_interm_ch, d.bsvd_stream, d.flags);
  return b;
}

ss4k_model_desc rrdb(int dtype, int scale, int nf, int g, int flags) {
  ss4k_model_desc d{}; d.kind = SS4K_RRDBNET; d.dtype = dtype; d.scale = scale; d.num_feat = nf; d.num_grow_ch = g; d.num_block = 1; d.flags = flags; return d;
}
ss4k_model_desc srvgg(int dtype, int scale, int nf, int nb, int flags) {
  ss4k_model_desc d{}; d.kind = SS4K_SRVGG; d.dtype = dtype; d.scale = scale; d.num_feat = nf; d.num_block = nb; d.flags = flags; return d;
}
ss4k_model_desc bsvd(int dtype, int c0, int c1, int c2, int mid, int interm, int stream, int flags) {
  ss4k_model_desc d{}; d.kind = SS4K_BSVD; d.dtype = dtype; d.scale = 1; d.bsvd_chns[0] = c0; d.bsvd_chns[1] = c1; d.bsvd_chns[2] = c2; d.bsvd_mid_ch = mid;
  d.bsvd_interm_ch = interm; d.bsvd_stream = stream; d.flags = flags; return d;
}
ss4k_model_desc fsr(int dtype, int scale, int flags) { ss4k_model_desc d{}; d.kind = SS4K_FSRCNN; d.dtype = dtype; d.scale = scale; d.flags = flags; return d; }

// the conv layers of a description in state_dict order: what the bijection check expects add_conv to have packed
struct LSpec { int cout, cin; bool prelu; int live_from; };
std::vector<LSpec> layer_specs(const ss4k_model_desc& d) {
  std::vector<LSpec> v;
  if (d.kind == SS4K_RRDBNET) {
    const int nf = d.num_feat, g = d.num_grow_ch, cin0 = 3 * (d.scale == 2 ? 4 : d.scale == 1 ? 16 : 1);
    v.push_back({nf, cin0, false, 0});
    for (int b = 0; b < d.num_block * 3; ++b) for (int c = 0; c < 5; ++c) v.push_back({c < 4 ? g : nf, nf + c * g, false, 0});
    for (int i = 0; i < 4; ++i) v.push_back({nf, nf, false, 0});
    v.push_back({3, nf, false, 0});
  } else if (d.kind == SS4K_SRVGG) {
    v.push_back({d.num_feat, 3, true, 0});
    for (int i = 0; i < d.num_block; ++i) v.push_back({d.num_feat, d.num_feat, true, 0});
    v.push_back({3 * d.scale * d.scale, d.num_feat, false, 0});
  } else if (d.kind == SS4K_BSVD) {
    const int c0 = d.bsvd_chns[0], c1 = d.bsvd_chns[1], c2 = d.bsvd_chns[2], im = d.bsvd_interm_ch;
    for (int blk = 0; blk < 2; ++blk) {
      const int ci = blk == 0 ? 4 : d.bsvd_mid_ch, co = blk == 0 ? d.bsvd_mid_ch : 3;
      const int s[16][2] = {{im, ci}, {c0, im}, {c1, c0}, {c1, c1}, {c1, c1}, {c2, c1}, {c2, c2}, {c2, c2}, {c2, c2}, {c2, c2}, {c1 * 4, c2}, {c1, c1}, {c1, c1}, {c0 * 4, c1}, {c0, c0}, {co, c0}};
      for (int i = 0; i < 16; ++i) {
        const bool masked = i == 3 || i == 4 || (i >= 6 && i <= 9) || i == 11 || i == 12;   // BiBufferConv: one frame leaves channels < c/4 dead
        v.push_back({s[i][0], s[i][1], false, masked && !d.bsvd_stream ? s[i][1] / 4 : 0});
      }
    }
  }
  return v;
}

// Index-coded weights: weight i of a layer carries digit `which` (0 low, 1 high) of i in base 2048, plus one - integers 1..2048, exact in
// fp16 (11 significand bits).  Base 2048 and not 1024: the widest layer of the lattice (256 x 896 x 9 weights) has more than 1024^2.
constexpr int BASE = 2048;
std::vector<float> make_blob(const ss4k_model_desc& d, int which) {
  const size_t n = model_param_count(d);
  std::vector<float> blob(n);
  uint32_t s = 2463534242u;
  for (auto& v : blob) { s = s * 1664525u + 1013904223u; v = ((s >> 8) & 0xffff) / 65536.0f * 0.02f - 0.01f; }
  size_t pos = 0;
  for (const LSpec& L : layer_specs(d)) {
    const size_t nw = (size_t)L.cout * L.cin * 9;
    if (pos + nw + L.cout * (L.prelu ? 2 : 1) > n) throw std::logic_error("layer_specs asks for more parameters than model_param_count gives");
    for (size_t i = 0; i < nw; ++i) blob[pos + i] = (float)((which == 0 ? i % BASE : i / BASE) + 1);
    pos += nw + L.cout * (L.prelu ? 2 : 1);
  }
  // the restated layer list is itself checked: it consumes exactly the parameters the library counts
  if (d.kind != SS4K_FSRCNN && pos != n) throw std::logic_error("layer_specs consumes " + std::to_string(pos) + " parameters, model_param_count gives " + std::to_string(n));
  return blob;
}

float half_bits_to_float(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 1023;
  float v = e == 0 ? std::ldexp((float)m, -24) : e == 31 ? INFINITY : std::ldexp((float)(m | 1024), e - 25);
  return (h & 0x8000) ? -v : v;
}

// One packed blob of one layer, from the two builds: every non-zero slot maps onto a distinct live weight, every live weight is hit, the rest is zero
void bijection_blob(const std::string& where, const LSpec& L, const void* pa, const void* pb, bool f16) {
  size_t off, bytes = 0, bytes_b = 0;
  if (!hc::reg_inside(pa, 1, &off, &bytes) || !hc::reg_inside(pb, 1, &off, &bytes_b) || bytes != bytes_b) { finding(where + ": packed blobs of the two builds differ in size"); return; }
  const size_t nslots = bytes / (f16 ? 2 : 4), nw = (size_t)L.cout * L.cin * 9;
  std::vector<uint8_t> seen(nw, 0);
  auto val = [&](const void* p, size_t i) {
    if (f16) { uint16_t h; std::memcpy(&h, static_cast<const char*>(p) + 2 * i, 2); return half_bits_to_float(h); }
    float f; std::memcpy(&f, static_cast<const char*>(p) + 4 * i, 4); return f;
  };
  long bad = 0;
  for (size_t i = 0; i < nslots; ++i) {
    const float lo = val(pa, i), hi = val(pb, i);
    if (lo == 0.f && hi == 0.f) continue;
    if (!(lo >= 1.f && lo <= BASE && hi >= 1.f && hi <= BASE && lo == std::floor(lo) && hi == std::floor(hi))) { if (!bad++) finding(where + ": slot " + std::to_string(i) + " holds no index code"); continue; }
    const size_t idx = (size_t)(lo - 1) + (size_t)(hi - 1) * BASE;
    if (idx >= nw) { if (!bad++) finding(where + ": slot " + std::to_string(i) + " decodes past the layer's weights"); continue; }
    const int ci = (int)(idx / 9 % L.cin);
    if (ci < L.live_from) { if (!bad++) finding(where + ": slot " + std::to_string(i) + " holds a dead input channel's weight"); continue; }
    if (seen[idx]++) { if (!bad++) finding(where + ": weight " + std::to_string(idx) + " packed twice"); }
  }
  size_t missing = 0;
  for (size_t idx = 0; idx < nw; ++idx) if ((int)(idx / 9 % L.cin) >= L.live_from && !seen[idx]) ++missing;
  if (missing) finding(where + ": " + std::to_string(missing) + " live weights are in no slot");
}

void bijection(const ss4k_model_desc& d, const Model& a, ss4k_ctx& ctx) {
  const std::vector<float> blob = make_blob(d, 1);
  Model b; b.ctx = &ctx; b.desc = d;
  b.build(blob.data(), blob.size());
  g_weights += (double)blob.size();
  const std::vector<LSpec> specs = layer_specs(d);
  if (specs.size() != a.layers.size() || specs.size() != b.layers.size()) { finding(desc_str(d) + ": layer count differs from the state_dict's"); return; }
  for (size_t li = 0; li < specs.size(); ++li) {
    const std::string where = desc_str(d) + " layer " + std::to_string(li);
    if (a.layers[li].cout_real != specs[li].cout) { finding(where + ": cout_real"); continue; }
    bijection_blob(where + " (pack_conv3x3)", specs[li], a.layers[li].w.ptr, b.layers[li].w.ptr, d.dtype == SS4K_F16);
    if ((a.layers[li].w16.ptr != nullptr) != (b.layers[li].w16.ptr != nullptr)) { finding(where + ": w16 blob in one build only"); continue; }
    if (a.layers[li].w16.ptr) bijection_blob(where + (specs[li].cout <= 4 ? " (pack_conv3x3_w16n)" : " (pack_conv3x3_w16)"), specs[li], a.layers[li].w16.ptr, b.layers[li].w16.ptr, true);
    ++g_bij_layers;
  }
}

struct Shape { int n, H, W; };
const Shape SHAPES[] = {{1, 1, 1}, {1, 1, 33}, {1, 7, 9}, {1, 17, 33}, {3, 1, 1}, {3, 1, 33}, {3, 7, 9}, {3, 17, 33}};

// layer resolution -> the model's input size
void input_size(const ss4k_model_desc& d, const Shape& s, int* h, int* w) {
  const int r = d.kind == SS4K_RRDBNET ? (d.scale == 2 ? 2 : d.scale == 1 ? 4 : 1) : d.kind == SS4K_BSVD ? 4 : 1;
  *h = s.H * r; *w = s.W * r;
}

struct Buf {   // a caller's buffer, through the same registry
  void* p; explicit Buf(size_t bytes) : p(hc::reg_alloc(bytes)) {} ~Buf() { hc::reg_free(p); }
  Buf(const Buf&) = delete; Buf& operator=(const Buf&) = delete;
};

void run_shape(Model& m, const Shape& s) {
  const ss4k_model_desc& d = m.desc;
  int h, w; input_size(d, s, &h, &w);
  char sb[96]; std::snprintf(sb, sizeof sb, "%d frames, layer %d x %d (input %d x %d)", s.n, s.H, s.W, h, w);
  hc::g_where.shape = sb; hc::g_where.launch = 0;
  m.acts.clear();   // fresh activation buffers: every shape is audited against exactly what it asks for
  const size_t ws = m.workspace_bytes(s.n, h, w);
  int oc, oh, ow; m.out_shape(s.n, h, w, &oc, &oh, &ow);
  Buf in((size_t)s.n * m.in_channels() * h * w * 4), out((size_t)s.n * oc * oh * ow * 4);
  m.forward(static_cast<const float*>(in.p), static_cast<float*>(out.p), s.n, h, w, nullptr);
  size_t got = 0;
  for (const DevBuf& b : m.acts) got += (b.bytes + 255) & ~size_t(255);
  // (BSVD's plan counts the tensors inside the inc / outc pairs whichever route runs: models.cpp, forward_impl)
  if (d.kind == SS4K_BSVD ? got > ws : got != ws)
    finding(hc::g_where.desc + " | " + sb + ": workspace_bytes " + std::to_string(ws) + ", the forward allocated " + std::to_string(got));
  ++g_shapes;
}

// --shard I N: this process takes every N-th lattice point, starting at the I-th (neighbours in the walk cost about the same, so the
// shards finish together); the test runs the shards side by side and adds up their counts
int g_shard = 0, g_shards = 1;
long g_point = 0;

// a lattice point: must be accepted
void accept(ss4k_ctx& ctx, const ss4k_model_desc& d, bool with_bijection) {
  if (g_point++ % g_shards != g_shard) return;
  hc::g_where.desc = desc_str(d); hc::g_where.shape = "build"; hc::g_where.launch = 0;
  try {
    const std::vector<float> blob = make_blob(d, 0);
    Model m; m.ctx = &ctx; m.desc = d;
    hc::g_where.model = &m;
    m.build(blob.data(), blob.size());
    ++g_accepted; g_weights += (double)blob.size();
    for (const Shape& s : SHAPES) run_shape(m, s);
    hc::g_where.model = nullptr;
    if (with_bijection && d.kind != SS4K_FSRCNN) bijection(d, m, ctx);
  } catch (const Error& e) {
    finding(hc::g_where.desc + " | " + hc::g_where.shape + ": refused or failed with code " + std::to_string(e.code) + ": " + e.what());
  } catch (const std::exception& e) {
    finding(hc::g_where.desc + " | " + hc::g_where.shape + ": exception " + e.what());
  }
  hc::g_where.model = nullptr;
}

// an invalid description (or blob size): the only acceptable outcome is ss4k::Error with SS4K_EINVAL
void refuse(ss4k_ctx& ctx, const char* name, const ss4k_model_desc& d, long blob_delta = LONG_MIN) {
  hc::g_where.desc = std::string("invalid: ") + name; hc::g_where.shape = "build";
  try {
    // (a valid description with a wrong blob size takes its real count; an invalid one must be refused before the count is looked at)
    std::vector<float> blob(blob_delta == LONG_MIN ? 64 : (size_t)((long)model_param_count(d) + blob_delta), 0.01f);
    Model m; m.ctx = &ctx; m.desc = d;
    m.build(blob.data(), blob.size());
    finding(std::string(name) + ": built (" + desc_str(d) + ")");
  } catch (const Error& e) {
    if (e.code == SS4K_EINVAL) ++g_refused;
    else finding(std::string(name) + ": Error code " + std::to_string(e.code) + ": " + e.what());
  } catch (const std::exception& e) {
    finding(std::string(name) + ": exception " + e.what());
  }
}

void walk_invalid(ss4k_ctx& ctx) {
  const int BIG32 = INT_MAX / 32 * 32, BIG64 = INT_MAX / 64 * 64, BIG16 = INT_MAX / 16 * 16;
  ss4k_model_desc d;
  for (int v : {0, -32, BIG32, 1 << 29, 1 << 20, 33, SS4K_DESC_MAX_WIDTH + 32}) {
    d = rrdb(SS4K_F16, 2, 64, 32, 0); d.num_feat = v; refuse(ctx, "RRDBNet num_feat", d);
    d = rrdb(SS4K_F16, 2, 64, 32, 0); d.num_grow_ch = v; refuse(ctx, "RRDBNet num_grow_ch", d);
  }
  for (int v : {0, -1, INT_MAX, 1 << 20, SS4K_DESC_MAX_BLOCKS + 1}) { d = rrdb(SS4K_F16, 2, 64, 32, 0); d.num_block = v; refuse(ctx, "RRDBNet num_block", d); }
  for (int v : {0, 3, -2, 8}) { d = rrdb(SS4K_F16, v, 64, 32, 0); refuse(ctx, "RRDBNet scale", d); }
  for (int v : {0, -16, BIG16, 1 << 29, 1 << 20, 17, SS4K_DESC_MAX_WIDTH + 16}) { d = srvgg(SS4K_F16, 4, v, 2, 0); refuse(ctx, "SRVGG num_feat", d); }
  for (int v : {-1, INT_MAX, 1 << 20, SS4K_DESC_MAX_BLOCKS + 1}) { d = srvgg(SS4K_F16, 4, 64, v, 0); refuse(ctx, "SRVGG num_block", d); }
  for (int v : {0, 1, 3, -4}) { d = srvgg(SS4K_F16, v, 64, 2, 0); refuse(ctx, "SRVGG scale", d); }
  for (int k = 0; k < 3; ++k)
    for (int v : {0, -32, -64, BIG64, 1 << 29, 1 << 20, 48, SS4K_DESC_MAX_WIDTH + 64}) { d = bsvd(SS4K_F16, 32, 64, 128, 32, 30, 0, 0); d.bsvd_chns[k] = v; refuse(ctx, "BSVD chns", d); }
  for (int v : {0, -32, BIG32, 1 << 20, 40, SS4K_DESC_MAX_WIDTH + 32}) { d = bsvd(SS4K_F16, 32, 64, 128, v, 30, 0, 0); refuse(ctx, "BSVD mid_ch", d); }
  for (int v : {0, -1, 257, INT_MAX}) { d = bsvd(SS4K_F16, 32, 64, 128, 32, v, 0, 0); refuse(ctx, "BSVD interm_ch", d); }
  for (int v : {0, 1, 3, -4}) { d = fsr(SS4K_F32, v, 0); refuse(ctx, "FSRCNN scale", d); }
  for (int v : {0, 5, -1, INT_MAX}) { d = rrdb(SS4K_F16, 2, 64, 32, 0); d.kind = v; refuse(ctx, "unknown kind", d); }
  for (int v : {2, -1, INT_MAX}) { d = rrdb(v, 2, 64, 32, 0); refuse(ctx, "unknown dtype", d); }
  for (int v : {8, 64, 128, 2048, 16384, 65536, INT_MIN}) { d = srvgg(SS4K_F16, 4, 64, 2, v); refuse(ctx, "unknown flag bit", d); }
  d = rrdb(SS4K_F16, 2, 64, 32, SS4K_MODEL_ONE_CHAIN | SS4K_MODEL_TWO_CHAINS); refuse(ctx, "ONE_CHAIN with TWO_CHAINS", d);
  d = rrdb(SS4K_F16, 2, 64, 32, SS4K_MODEL_TILE_ROWS_16 | SS4K_MODEL_TILE_ROWS_20); refuse(ctx, "TILE_ROWS_16 with TILE_ROWS_20", d);
  for (int kind : {SS4K_FSRCNN, SS4K_RRDBNET, SS4K_SRVGG}) {
    d = kind == SS4K_FSRCNN ? fsr(SS4K_F32, 2, 0) : kind == SS4K_RRDBNET ? rrdb(SS4K_F16, 2, 64, 32, 0) : srvgg(SS4K_F16, 4, 64, 2, 0);
    d.bsvd_stream = 1; refuse(ctx, "bsvd_stream on a non-BSVD kind", d);
  }
  d = bsvd(SS4K_F16, 32, 64, 128, 32, 30, 2, 0); refuse(ctx, "bsvd_stream 2", d);
  for (long delta : {-1L, 1L}) {
    refuse(ctx, "FSRCNN blob off by one", fsr(SS4K_F32, 2, 0), delta);
    refuse(ctx, "RRDBNet blob off by one", rrdb(SS4K_F16, 2, 64, 32, 0), delta);
    refuse(ctx, "SRVGG blob off by one", srvgg(SS4K_F32, 2, 48, 1, 0), delta);
    refuse(ctx, "BSVD blob off by one", bsvd(SS4K_F16, 32, 64, 128, 32, 30, 0, 0), delta);
  }
}

// The lattice ("Host check").  Every axis keeps both ends.  Thinned from the full cross product, which takes 40 minutes under the
// sanitizers (the time goes with the number of weights packed):
//   * a routing flag changes no packed weight and no buffer size, and NO_DENSE / NO_W16 / NO_WIDE / NO_PAIR only choose between fp16
//     kernels: non-zero flags run in fp16 at one scale (RRDBNet 2, SRVGG 4); flags 0 runs at every scale and dtype, with the bijection check;
//   * RRDBNet num_feat 32, 64, 96, 128, 160, 256 (of 32..256 step 32) and num_grow_ch 32, 64, 96, 160 (of 32..160 step 32);
//   * BSVD: the 16 corners of (chns[0], chns[1], chns[2], mid_ch) in {32, 96} x {64, 192} x {64, 192} x {32, 96}, the centre
//     (64, 128, 128, 64) and the three interior points the GPU cases run (tests/test_gpu_error_budget.py) with every interm_ch (and 48,
//     which a GPU case uses) at stream 0, fp16; stream 1, fp32 and NO_PAIR at interm_ch 1, 30, 33, 256.
// Every description a GPU test runs is a point of this walk: a width goes to a GPU only after the walk is clean for it.
void walk_lattice(ss4k_ctx& ctx, const char* only) {
  auto want = [&](const char* k) { return !only || !std::strcmp(only, k); };
  const int dtypes[] = {SS4K_F16, SS4K_F32};
  const int TWO = SS4K_MODEL_TWO_CHAINS;
  if (want("rrdbnet"))
    for (int nf : {32, 64, 96, 128, 160, 256})
      for (int g : {32, 64, 96, 160}) {
        for (int scale : {1, 2, 4}) for (int dt : dtypes) accept(ctx, rrdb(dt, scale, nf, g, 0), true);
        for (int fl : {(int)SS4K_MODEL_NO_DENSE, (int)SS4K_MODEL_NO_W16, (int)SS4K_MODEL_NO_WIDE, SS4K_MODEL_NO_W16 | SS4K_MODEL_NO_DENSE, TWO}) accept(ctx, rrdb(SS4K_F16, 2, nf, g, fl), false);
      }
  if (want("srvgg"))
    for (int nf = 16; nf <= 256; nf += 16)
      for (int nb : {0, 1, 3}) {
        for (int scale : {2, 4}) for (int dt : dtypes) accept(ctx, srvgg(dt, scale, nf, nb, 0), true);
        for (int fl : {(int)SS4K_MODEL_NO_W16, (int)SS4K_MODEL_NO_WIDE, TWO}) accept(ctx, srvgg(SS4K_F16, 4, nf, nb, fl), false);
      }
  if (want("bsvd")) {
    std::vector<std::array<int, 4>> widths = {{64, 128, 128, 64}, {32, 64, 128, 32}, {64, 64, 128, 64}, {96, 128, 192, 96}};
    for (int c0 : {32, 96}) for (int c1 : {64, 192}) for (int c2 : {64, 192}) for (int mid : {32, 96}) widths.push_back({c0, c1, c2, mid});
    for (const auto& wd : widths)
      for (int im : {1, 16, 30, 32, 33, 48, 64, 256}) {
        accept(ctx, bsvd(SS4K_F16, wd[0], wd[1], wd[2], wd[3], im, 0, 0), true);
        if (im == 1 || im == 30 || im == 33 || im == 256) {
          accept(ctx, bsvd(SS4K_F16, wd[0], wd[1], wd[2], wd[3], im, 1, 0), true);
          accept(ctx, bsvd(SS4K_F32, wd[0], wd[1], wd[2], wd[3], im, 0, 0), true);
          accept(ctx, bsvd(SS4K_F32, wd[0], wd[1], wd[2], wd[3], im, 1, 0), false);
          accept(ctx, bsvd(SS4K_F16, wd[0], wd[1], wd[2], wd[3], im, 0, SS4K_MODEL_NO_PAIR), false);
          accept(ctx, bsvd(SS4K_F16, wd[0], wd[1], wd[2], wd[3], im, 1, SS4K_MODEL_NO_PAIR | TWO), false);
        }
      }
  }
  // the bounds validate_desc sets (SS4K_DESC_MAX_WIDTH, SS4K_DESC_MAX_BLOCKS): one point per network at the widest and one at the deepest
  // description it accepts, both dtypes, every shape; no bijection check (500 M parameters to pack as it is)
  if (want("bounds")) {
    const int WMAX = SS4K_DESC_MAX_WIDTH, BMAX = SS4K_DESC_MAX_BLOCKS;
    for (int dt : dtypes) {
      accept(ctx, rrdb(dt, 2, WMAX, WMAX, 0), false);
      { ss4k_model_desc d = rrdb(dt, 4, 32, 32, 0); d.num_block = BMAX; accept(ctx, d, false); }
      accept(ctx, srvgg(dt, 4, WMAX, 1, 0), false);
      accept(ctx, srvgg(dt, 2, 16, BMAX, 0), false);
      accept(ctx, bsvd(dt, WMAX, WMAX, WMAX, WMAX, 256, 0, 0), false);
      accept(ctx, bsvd(dt, WMAX, WMAX, WMAX, WMAX, 256, 1, 0), false);
    }
  }
  if (want("fsrcnn"))
    for (int scale : {2, 4})
      for (int dt : dtypes)
        for (int fl : {0, (int)SS4K_MODEL_FS_EXACT, TWO}) accept(ctx, fsr(dt, scale, fl), false);
}

// the service's host-side tables: every entry inside the source, offsets monotonic, weights of a cell summing to one
void walk_tables() {
  for (int k : {1, 3, 9, 17, 31}) for (float sigma : {0.5f, 2.f, 8.f}) {
    const std::vector<float> g = gaussian_taps_1d(k, sigma);
    double s = 0; for (float v : g) s += v;
    if ((int)g.size() != k || std::fabs(s - 1.0) > 1e-5) finding("gaussian_taps_1d(" + std::to_string(k) + "): size or sum");
  }
  for (int ssize : {2, 3, 7, 17, 100, 719, 1080, 4320})
    for (double f : {0.9, 0.75, 0.6, 0.37, 0.11, 0.013}) {
      const int dsize = (int)std::nearbyint(ssize * f);
      if (dsize <= 0) continue;
      std::vector<CvEnt> ent; std::vector<int> ofs;
      cv_area_tab(ssize, dsize, 1.0 / f, ent, ofs);
      bool ok = (int)ofs.size() == dsize + 1 && ofs[0] == 0 && ofs[dsize] == (int)ent.size();
      for (int d = 0; ok && d < dsize; ++d) {
        ok = ofs[d] <= ofs[d + 1];
        double s = 0;
        for (int e = ofs[d]; ok && e < ofs[d + 1]; ++e) { ok = ent[e].si >= 0 && ent[e].si < ssize && ent[e].a >= 0.f; s += ent[e].a; }
        ok = ok && ofs[d + 1] > ofs[d] && std::fabs(s - 1.0) < 1e-3;
      }
      if (!ok) finding("cv_area_tab(" + std::to_string(ssize) + " -> " + std::to_string(dsize) + "): entry outside the source, empty cell or weights not summing to one");
    }
}

int control_shrink(int idx) {
  ss4k_ctx ctx;
  const ss4k_model_desc d = rrdb(SS4K_F16, 4, 64, 32, SS4K_MODEL_NO_DENSE);
  const std::vector<float> blob = make_blob(d, 0);
  Model m; m.ctx = &ctx; m.desc = d;
  m.build(blob.data(), blob.size());
  hc::g_where.desc = desc_str(d); hc::g_where.model = &m;
  const int n = 1, h = 7, w = 9;
  Buf in((size_t)n * 3 * h * w * 4), out((size_t)n * 3 * 16 * h * w * 4);
  hc::g_where.shape = "1 frame, layer 7 x 9"; hc::g_where.launch = 0;
  m.forward(static_cast<const float*>(in.p), static_cast<float*>(out.p), n, h, w, nullptr);   // allocates the activation buffers
  if (hc::g_violations || idx < 0 || idx >= (int)m.acts.size() || !m.acts[idx].ptr) { std::printf("CONTROL setup failed\n"); return 2; }
  const size_t px = (size_t)n * h * w * (idx >= 7 ? 16 : idx == 6 ? 4 : 1);
  hc::reg_shrink(m.acts[idx].ptr, px * m.rec());   // the buffer's last plane
  hc::g_where.launch = 0;
  m.forward(static_cast<const float*>(in.p), static_cast<float*>(out.p), n, h, w, nullptr);
  hc::g_where.model = nullptr;
  std::printf("CONTROL shrink buffer %d violations=%ld\n", idx, hc::g_violations);
  return 0;
}

int control_short_blob() {
  ss4k_ctx ctx;
  const ss4k_model_desc d = rrdb(SS4K_F16, 2, 64, 32, 0);
  std::vector<float> blob = make_blob(d, 0);
  blob.pop_back();
  try {
    Model m; m.ctx = &ctx; m.desc = d;
    m.build(blob.data(), blob.size());
    std::printf("CONTROL short blob: built\n");
  } catch (const Error& e) {
    std::printf("CONTROL short blob: %s (%d): %s\n", e.code == SS4K_EINVAL ? "SS4K_EINVAL" : "other code", e.code, e.what());
  }
  return 0;
}

// --trace: the launches one description makes for one shape (which route a width takes, without a GPU)
int trace(char** v) {
  ss4k_model_desc d{};
  int32_t* f[] = {&d.kind, &d.dtype, &d.scale, &d.num_feat, &d.num_block, &d.num_grow_ch, &d.bsvd_chns[0], &d.bsvd_chns[1], &d.bsvd_chns[2], &d.bsvd_mid_ch, &d.bsvd_interm_ch, &d.bsvd_stream, &d.flags};
  for (int i = 0; i < 13; ++i) *f[i] = std::atoi(v[i]);
  const Shape s{std::atoi(v[13]), std::atoi(v[14]), std::atoi(v[15])};
  ss4k_ctx ctx;
  try {
    const std::vector<float> blob = make_blob(d, 0);
    Model m; m.ctx = &ctx; m.desc = d;
    m.build(blob.data(), blob.size());
    hc::g_where.desc = desc_str(d); hc::g_where.model = &m; hc::g_trace = true;
    run_shape(m, s);
    hc::g_where.model = nullptr;
  } catch (const Error& e) { std::printf("refused (%d): %s\n", e.code, e.what()); }
  return hc::g_violations || g_findings ? 1 : 0;
}

// =================================================================== the frame-recurrent upscaler (frvsr.cpp; DESIGN.md, "Host check")
long g_fr_accepted = 0, g_fr_refused = 0, g_steps = 0, g_refused_steps = 0, g_rounds = 0, g_refused_rounds = 0;
// ... and of the walk of the other five (generator, degradation, route) variants (walk_variants), which counts apart: the totals above stay what they were
long g_var_accepted = 0, g_var_refused = 0, g_var_steps = 0, g_var_rounds = 0, g_var_refused_rounds = 0;
long *g_step_count = &g_steps, *g_round_count = &g_rounds, *g_refused_round_count = &g_refused_rounds;

// which of the executor's variants an object is: generator, degradation, TecoGAN's transposed-conv route (include/ss4k.h)
struct Variant { const char* name; int gen, deg, route; };
const Variant EGVSR_BD{"EGVSR 'BD'", SS4K_FRVSR_EGVSR, SS4K_FRVSR_BD, 0};
const Variant VARIANTS[] = {{"EGVSR 'BI'", SS4K_FRVSR_EGVSR, SS4K_FRVSR_BI, 0},
                            {"TecoGAN 'BD' embedded", SS4K_FRVSR_TECOGAN, SS4K_FRVSR_BD, SS4K_FRVSR_CONVT_EMBEDDED},
                            {"TecoGAN 'BD' phase", SS4K_FRVSR_TECOGAN, SS4K_FRVSR_BD, SS4K_FRVSR_CONVT_PHASE},
                            {"TecoGAN 'BI' embedded", SS4K_FRVSR_TECOGAN, SS4K_FRVSR_BI, SS4K_FRVSR_CONVT_EMBEDDED},
                            {"TecoGAN 'BI' phase", SS4K_FRVSR_TECOGAN, SS4K_FRVSR_BI, SS4K_FRVSR_CONVT_PHASE}};

ss4k_frvsr_desc frdesc(int dtype, int nb) { ss4k_frvsr_desc d{}; d.dtype = dtype; d.num_feat = 64; d.num_block = nb; return d; }
std::string frdesc_str(const ss4k_frvsr_desc& d) {
  char b[160];
  std::snprintf(b, sizeof b, "frvsr dtype %d nf %d nb %d flags %d reserved %d,%d,%d,%d", d.dtype, d.num_feat, d.num_block, d.flags, d.reserved[0], d.reserved[1], d.reserved[2], d.reserved[3]);
  return b;
}

// FRNet's convolutions in state_dict order, restated from the reference's module list (egvsr.py:19-61 FNet, :104-127 SRNet; TecoGAN's SRNet:
// tecogan_nets.py:101-149), and where each one's weights start in the blob: the 16 floats of upsample_func.kernels first ('BD'; a 'BI' state_dict has
// no such buffer); after the residual blocks conv_up.{0,2} (transposed, (C_in, C_out, 3, 3): `up_at`, in no `specs` entry), conv_out (Conv2d(4, 3)
// for EGVSR, Conv2d(nf, 3) for TecoGAN) and the kernels again
struct FrLayers { std::vector<LSpec> specs; std::vector<size_t> at; size_t up_at[2] = {0, 0}, total = 0; };
FrLayers fr_layers(const ss4k_frvsr_desc& d, const Variant& v = EGVSR_BD) {
  FrLayers L;
  const int nf = d.num_feat;
  const int fnet[14][2] = {{32, 6}, {32, 32}, {64, 32}, {64, 64}, {128, 64}, {128, 128}, {256, 128}, {256, 256}, {128, 256}, {128, 128}, {64, 128}, {64, 64}, {32, 64}, {2, 32}};
  const size_t kernels = v.deg == SS4K_FRVSR_BD ? 16 : 0;
  size_t pos = kernels;
  auto add = [&](int cout, int cin) { L.specs.push_back({cout, cin, false, 0}); L.at.push_back(pos); pos += (size_t)cout * cin * 9 + cout; };
  for (auto& c : fnet) add(c[0], c[1]);
  add(nf, 51);
  for (int i = 0; i < 2 * d.num_block; ++i) add(nf, nf);
  for (int k = 0; k < 2; ++k) { L.up_at[k] = pos; pos += (size_t)nf * nf * 9 + nf; }
  pos += (size_t)3 * (v.gen == SS4K_FRVSR_TECOGAN ? nf : 4) * 9 + 3 + kernels;
  L.total = pos;
  return L;
}
std::vector<float> fr_blob(const ss4k_frvsr_desc& d, int which, const Variant& v = EGVSR_BD) {
  const size_t n = frvsr_param_count(d, v.gen, v.deg);
  const FrLayers L = fr_layers(d, v);
  if (L.total != n) throw std::logic_error("fr_layers consumes " + std::to_string(L.total) + " parameters, frvsr_param_count gives " + std::to_string(n));
  std::vector<float> blob(n);
  uint32_t s = 2463534242u;
  for (auto& v : blob) { s = s * 1664525u + 1013904223u; v = ((s >> 8) & 0xffff) / 65536.0f * 0.02f - 0.01f; }
  for (size_t l = 0; l < L.specs.size(); ++l) {
    const size_t nw = (size_t)L.specs[l].cout * L.specs[l].cin * 9;
    for (size_t i = 0; i < nw; ++i) blob[L.at[l] + i] = (float)((which == 0 ? i % BASE : i / BASE) + 1);
  }
  if (v.gen == SS4K_FRVSR_TECOGAN)   // the transposed layers' weights too (pack_convt3x3s2's blobs go through the bijection check)
    for (size_t at : L.up_at) for (size_t i = 0; i < (size_t)d.num_feat * d.num_feat * 9; ++i) blob[at + i] = (float)((which == 0 ? i % BASE : i / BASE) + 1);
  return blob;
}

struct BufAt {   // a caller's frame: registered at its exact size, at an odd byte offset of its host block
  void* p; size_t bytes;
  explicit BufAt(size_t b, size_t lead = 0) : p(hc::reg_alloc_at(lead, b)), bytes(b) {}
  ~BufAt() { hc::reg_free(p); }
  BufAt(const BufAt&) = delete; BufAt& operator=(const BufAt&) = delete;
  void filled() const { hc::cov_write(p, bytes); }   // an input: the caller wrote all of it
};
using BufP = std::unique_ptr<BufAt>;

size_t r256(size_t b) { return (b + 255) & ~size_t(255); }
// fresh activation buffers: every shape is audited against exactly what it asks for
void fr_clear(Frvsr& f) { f.net.acts.clear(); f.flow_raw.release(); f.flow.release(); f.tap_s2d.release(); }

// the launches of the log apart from the input packing, item launchers under their contiguous names
std::string launch_sequence() {
  std::string s;
  for (const hc::Launch& l : hc::g_launch_log) {
    std::string k = l.kind;
    if (k == "pack_input" || k == "pack_lr(items)") continue;
    const size_t par = k.find("(items)");
    if (par != std::string::npos) k.erase(par);
    s += k + ":" + std::to_string(l.layer) + " ";
  }
  return s;
}

enum { ROUTE_CONTIG = 0, ROUTE_ITEMS = 1, ROUTE_ITEMS_BATCHED = 2 };
const char* ROUTE_NAMES[3] = {"contiguous", "items", "items, pack_batched"};

// one step at (n, h, w) through one route; returns the launch sequence ("" after a finding)
std::string run_step(Frvsr& f, int n, int h, int w, int route, bool keep_taps) {
  char sb[128]; std::snprintf(sb, sizeof sb, "step n %d, %d x %d, %s, taps %d", n, h, w, ROUTE_NAMES[route], (int)keep_taps);
  hc::g_where.shape = sb; hc::g_where.launch = 0; hc::g_where.model = &f.net;
  hc::log_clear(); fr_clear(f);
  f.keep_taps = keep_taps;
  const size_t hw = (size_t)h * w, ws = f.workspace_bytes(n, h, w);
  std::vector<BufP> bufs;
  auto mk = [&](size_t bytes, bool input) { bufs.push_back(std::make_unique<BufAt>(bytes)); if (input) bufs.back()->filled(); return static_cast<float*>(bufs.back()->p); };
  std::vector<float*> outs;
  if (route == ROUTE_CONTIG) {
    float* c = mk(n * 3 * hw * 4, true); float* p = mk(n * 3 * hw * 4, true); float* hp = mk(n * 48 * hw * 4, true); float* ho = mk(n * 48 * hw * 4, false);
    outs.push_back(ho);
    f.step(c, p, hp, ho, n, h, w, nullptr);
  } else {
    std::vector<const float*> c(n), p(n); FrvsrPtrs hp{}, ho{};
    for (int i = 0; i < n; ++i) { c[i] = mk(3 * hw * 4, true); p[i] = mk(3 * hw * 4, true); hp.p[i] = mk(48 * hw * 4, true); ho.p[i] = mk(48 * hw * 4, false); outs.push_back(ho.p[i]); }
    f.step_items(Frvsr::Items{c.data(), p.data(), &hp, &ho, route == ROUTE_ITEMS_BATCHED}, n, h, w, nullptr);
  }
  f.keep_taps = false;
  ++*g_step_count;
  const std::string where = hc::g_where.desc + " | " + sb;
  // the activation requests, rounded as the product's DevBuf rounds them, and the two flow buffers are what workspace_bytes promised.  (It counts
  // flow_raw at flow's size, "at most as large": the raw flow is (n, 2, h // 8 * 8, w // 8 * 8) fp32 - egvsr.py:191-194 - and must be exactly that.)
  size_t got = 0;
  for (const DevBuf& b : f.net.acts) got += r256(b.bytes);
  const size_t flow_b = (size_t)n * 2 * hw * 4, raw_b = (size_t)n * 2 * (h / 8 * 8) * (w / 8 * 8) * 4;
  if (got + 2 * r256(flow_b) != ws) finding(where + ": workspace_bytes " + std::to_string(ws) + ", the step allocated " + std::to_string(got) + " + 2 x " + std::to_string(r256(flow_b)));
  if (f.flow.bytes != flow_b || f.flow_raw.bytes != raw_b) finding(where + ": flow buffers of " + std::to_string(f.flow_raw.bytes) + " and " + std::to_string(f.flow.bytes) + " bytes, " + std::to_string(raw_b) + " and " + std::to_string(flow_b) + " expected");
  if (keep_taps ? f.tap_s2d.bytes != (size_t)n * 48 * hw * 4 : f.tap_s2d.ptr != nullptr) finding(where + ": tap buffer of " + std::to_string(f.tap_s2d.bytes) + " bytes");
  for (float* o : outs) if (!hc::cov_covered(o, (outs.size() == 1 ? (size_t)n : 1) * 48 * hw * 4)) { finding(where + ": the step left part of hr_out unwritten"); break; }
  return launch_sequence();
}

// a step the library must refuse: SS4K_EINVAL, no launch, no allocation
template <typename F>
void refuse_step(Frvsr& f, const char* name, F&& call) {
  hc::g_where.shape = std::string("refused step: ") + name;
  fr_clear(f);
  const long l0 = hc::g_launches, a0 = hc::g_allocs, m0 = hc::g_memsets; const size_t live0 = hc::reg_live();
  try { call(); finding(hc::g_where.desc + " | " + hc::g_where.shape + ": accepted"); }
  catch (const Error& e) { if (e.code != SS4K_EINVAL) finding(hc::g_where.desc + " | " + hc::g_where.shape + ": Error code " + std::to_string(e.code)); else ++g_refused_steps; }
  if (l0 != hc::g_launches || a0 != hc::g_allocs || m0 != hc::g_memsets || live0 != hc::reg_live())
    finding(hc::g_where.desc + " | " + hc::g_where.shape + ": the refusal came after " + std::to_string(hc::g_launches - l0) + " launches and " + std::to_string(hc::g_allocs - a0) + " allocations");
}

bool mine() { return g_point++ % g_shards == g_shard; }

std::string frdesc_str(const ss4k_frvsr_desc& d, const Variant& v) { return &v == &EGVSR_BD ? frdesc_str(d) : frdesc_str(d) + " " + v.name; }

std::unique_ptr<Frvsr> fr_build(ss4k_ctx& ctx, const ss4k_frvsr_desc& d, int which = 0, const Variant& v = EGVSR_BD) {
  const std::vector<float> blob = fr_blob(d, which, v);
  auto f = std::make_unique<Frvsr>();
  f->ctx = &ctx; f->desc = d; f->generator = v.gen; f->degradation = v.deg; f->route_flags = v.route;   // api.cpp: ss4k_frvsr_create_ex
  hc::g_where.desc = frdesc_str(d, v); hc::g_where.shape = "build"; hc::g_where.model = nullptr;
  f->build(blob.data(), blob.size());
  g_weights += (double)blob.size();
  return f;
}

void walk_frvsr_descs(ss4k_ctx& ctx) {
  // accepted: num_feat 64 x num_block 0, 1, 2, 10, 64 x both dtypes, one step each; the bijection check at num_block 2
  for (int nb : {0, 1, 2, 10, 64})
    for (int dt : {SS4K_F16, SS4K_F32}) {
      if (!mine()) continue;
      const ss4k_frvsr_desc d = frdesc(dt, nb);
      try {
        std::unique_ptr<Frvsr> a = fr_build(ctx, d);
        ++g_fr_accepted;
        if ((int)a->net.layers.size() != 15 + 2 * nb) finding(frdesc_str(d) + ": layer count");
        run_step(*a, 1, 9, 15, ROUTE_CONTIG, false);
        if (nb == 2) {
          std::unique_ptr<Frvsr> b = fr_build(ctx, d, 1);
          const FrLayers L = fr_layers(d);
          for (size_t li = 0; li < L.specs.size(); ++li) {
            const std::string where = frdesc_str(d) + " layer " + std::to_string(li);
            const ConvLayer &la = a->net.layers[li], &lb = b->net.layers[li];
            if (la.cout_real != L.specs[li].cout) { finding(where + ": cout_real"); continue; }
            bijection_blob(where + " (pack_conv3x3)", L.specs[li], la.w.ptr, lb.w.ptr, dt == SS4K_F16);
            if ((la.w16.ptr != nullptr) != (lb.w16.ptr != nullptr)) { finding(where + ": w16 blob in one build only"); continue; }
            if (la.w16.ptr) bijection_blob(where + (L.specs[li].cout <= 4 ? " (pack_conv3x3_w16n)" : " (pack_conv3x3_w16)"), L.specs[li], la.w16.ptr, lb.w16.ptr, true);
            ++g_bij_layers;
          }
        }
      } catch (const std::exception& e) { finding(frdesc_str(d) + " | " + hc::g_where.shape + ": exception " + e.what()); }
      hc::g_where.model = nullptr;
    }
  if (g_shard != 0) return;
  // refused: SS4K_EINVAL from build, 0 from frvsr_param_count
  auto refuse_desc = [&](const char* name, const ss4k_frvsr_desc& d, long blob_delta = LONG_MIN) {
    hc::g_where.desc = std::string("invalid frvsr: ") + name; hc::g_where.shape = "build";
    try {
      std::vector<float> blob(blob_delta == LONG_MIN ? 64 : (size_t)((long)frvsr_param_count(d) + blob_delta), 0.01f);
      if (blob_delta == LONG_MIN && frvsr_param_count(d) != 0) finding(std::string(name) + ": frvsr_param_count answers " + std::to_string(frvsr_param_count(d)));
      Frvsr f; f.ctx = &ctx; f.desc = d;
      f.build(blob.data(), blob.size());
      finding(std::string(name) + ": built (" + frdesc_str(d) + ")");
    } catch (const Error& e) {
      if (e.code == SS4K_EINVAL) ++g_fr_refused; else finding(std::string(name) + ": Error code " + std::to_string(e.code));
    } catch (const std::exception& e) { finding(std::string(name) + ": exception " + e.what()); }
  };
  ss4k_frvsr_desc d;
  for (int v : {0, -16, 16, 48, 128, 528}) { d = frdesc(SS4K_F16, 2); d.num_feat = v; refuse_desc("num_feat", d); }
  for (int v : {-1, 65}) { d = frdesc(SS4K_F16, v); refuse_desc("num_block", d); }
  d = frdesc(SS4K_F16, 2); d.flags = 1; refuse_desc("flags", d);
  for (int k = 0; k < 4; ++k) { d = frdesc(SS4K_F16, 2); d.reserved[k] = 1; refuse_desc("reserved", d); }
  d = frdesc(2, 2); refuse_desc("unknown dtype", d);
  for (long delta : {-1L, 1L}) refuse_desc("blob off by one", frdesc(SS4K_F32, 1), delta);
}

// Frvsr::step / step_items over the shape space.  Every (h, w) in 8..40 x 8..40 at n = 1 (all residues at every pyramid level), both
// dtypes, the three input-packing routes, taps on and off; the thinned set at n = 2, 3, 64 (taps on: a superset of the launches).
void walk_frvsr_steps(ss4k_ctx& ctx) {
  hc::g_log = true;
  for (int dt : {SS4K_F16, SS4K_F32}) {
    std::unique_ptr<Frvsr> fp;
    auto model = [&]() -> Frvsr& { if (!fp) fp = fr_build(ctx, frdesc(dt, 1)); hc::g_where.desc = frdesc_str(fp->desc); return *fp; };
    auto point = [&](int n, int h, int w, std::initializer_list<bool> taps) {
      if (!mine()) return;
      Frvsr& f = model();
      try {
        for (bool kt : taps) {
          std::string seq[3];
          for (int route = 0; route < 3; ++route) seq[route] = run_step(f, n, h, w, route, kt);
          if (seq[0] != seq[1] || seq[0] != seq[2]) finding(hc::g_where.desc + " | n " + std::to_string(n) + " " + std::to_string(h) + " x " + std::to_string(w) + ": the three routes differ in their launch sequence");
        }
      } catch (const std::exception& e) { finding(hc::g_where.desc + " | " + hc::g_where.shape + ": exception " + e.what()); }
    };
    for (int h = 8; h <= 40; ++h) for (int w = 8; w <= 40; ++w) point(1, h, w, {false, true});
    const int thin[] = {8, 9, 15, 16, 17, 23, 31, 33};
    for (int n : {2, 3, 64}) for (int h : thin) for (int w : thin) point(n, h, w, {true});
    if (g_shard == (dt == SS4K_F16 ? 0 : g_shards - 1)) {   // the refusals: one shard per dtype
      Frvsr& f = model();
      BufAt a(3 * 64 * 4), hp(48 * 64 * 4); a.filled(); hp.filled();
      float* x = static_cast<float*>(a.p); float* y = static_cast<float*>(hp.p);
      for (int v : {7, 0, -8}) {
        refuse_step(f, "h", [&] { f.step(x, x, y, y, 1, v, 8, nullptr); });
        refuse_step(f, "w", [&] { f.step(x, x, y, y, 1, 8, v, nullptr); });
      }
      refuse_step(f, "n 0", [&] { f.step(x, x, y, y, 0, 8, 8, nullptr); });
      // the first sizes with n * 16 * h * w >= 2^31: one frame of 8 x 2^24, and 64 of 1449 x 1449 (1448 x 1448 x 1024 < 2^31 <= 1449 x 1449 x 1024)
      refuse_step(f, "2^31 (n 1)", [&] { f.step(x, x, y, y, 1, 8, 1 << 24, nullptr); });
      refuse_step(f, "2^31 (n 64)", [&] { f.step(x, x, y, y, 64, 1449, 1449, nullptr); });
      const float* tab[65]; FrvsrPtrs ps{};
      for (int i = 0; i < 65; ++i) tab[i] = x;
      for (auto& q : ps.p) q = y;
      refuse_step(f, "step_items n 65", [&] { f.step_items(Frvsr::Items{tab, tab, &ps, &ps}, 65, 8, 8, nullptr); });
      refuse_step(f, "step_items NULL table", [&] { f.step_items(Frvsr::Items{tab, nullptr, &ps, &ps}, 2, 8, 8, nullptr); });
      refuse_step(f, "step_items NULL table", [&] { f.step_items(Frvsr::Items{tab, tab, nullptr, &ps}, 2, 8, 8, nullptr); });
    }
    hc::g_where.model = nullptr;
  }
  hc::g_log = false;
}

// ---- FrvsrUpscaler rounds.  The creation checks live in api.cpp, which is not linked: the walk builds the object the way
// ss4k_frvsr_upscaler_create_streams does (api.cpp:292-297) and resets slots the way ss4k_frvsr_upscaler_reset[_stream] do (api.cpp:305-315).
struct Geo { const char* name; int lh, lw, ih, iw, oh, ow; };   // oh = ow = 0: no output_shape
const Geo GEOS[] = {
  {"identity", 8, 8, 8, 8, 0, 0},
  {"area in", 15, 17, 40, 50, 0, 0},
  {"area out", 15, 17, 15, 17, 37, 45},
  {"both, non-integer ratios", 33, 41, 70, 90, 100, 120},
  {"in = 4 x lr", 8, 8, 32, 32, 0, 0},
  {"in = 8 x lr, out = lr", 8, 8, 64, 64, 8, 8},
  {"in 1 x 1", 15, 17, 1, 1, 0, 0},
  {"in 5 x 9", 15, 17, 5, 9, 0, 0},
  {"out 1 x 1", 8, 8, 8, 8, 1, 1},
  {"out larger than 4 x lr", 8, 8, 9, 9, 50, 70},
};

std::unique_ptr<FrvsrUpscaler> make_upscaler(ss4k_ctx& ctx, Frvsr& f, int lh, int lw, int oh, int ow, int max_streams) {
  auto u = std::make_unique<FrvsrUpscaler>();   // api.cpp:292-297
  u->ctx = &ctx; u->m = &f; u->lr_h = lh; u->lr_w = lw; u->out_h = oh; u->out_w = ow;
  u->slots.resize((size_t)max_streams);
  for (DevBuf* b : {&u->img, &u->hrc, &u->outf}) b->transient = true;
  return u;
}

struct SlotSnap {
  bool have; int cur; const void* p[4]; size_t b[4];
  bool operator==(const SlotSnap& o) const { return have == o.have && cur == o.cur && !std::memcmp(p, o.p, sizeof p) && !std::memcmp(b, o.b, sizeof b); }
};
std::vector<SlotSnap> snap_slots(const FrvsrUpscaler& u) {
  std::vector<SlotSnap> v;
  for (const auto& s : u.slots) v.push_back({s.have_state, s.cur, {s.lr[0].ptr, s.lr[1].ptr, s.hr[0].ptr, s.hr[1].ptr}, {s.lr[0].bytes, s.lr[1].bytes, s.hr[0].bytes, s.hr[1].bytes}});
  return v;
}

// what the walk itself knows about a slot: whether it has a state, and which buffers its last round wrote as the current frame
struct SlotModel { bool named = false, has = false; const char* lr = nullptr; const char* hr = nullptr; };

struct RoundWalk {
  ss4k_ctx& ctx; Frvsr& f; FrvsrUpscaler& u; const Geo& g; bool at;
  std::vector<SlotModel> model;
  int round_no = 0;
  bool keep_launch_index = false;   // the controls number their launches through all rounds
  long short_out_item = -1;         // control: this item's output frame is registered one byte short
  RoundWalk(ss4k_ctx& c, Frvsr& fr, FrvsrUpscaler& up, const Geo& ge, bool a) : ctx(c), f(fr), u(up), g(ge), at(a), model(up.slots.size()) {}

  void violation(const hc::Launch& l, const char* operand, const std::string& what) {
    if (++hc::g_violations > 40) return;
    std::printf("VIOLATION %s | %s | launch %d (%s) layer %d | %s [slot state] | %s\n", hc::g_where.desc.c_str(), hc::g_where.shape.c_str(), l.index, l.kind, l.layer, operand, what.c_str());
  }
  void reset_stream(int s) { u.slots[(size_t)s].have_state = false; model[(size_t)s].has = false; }   // api.cpp:310-315
  void reset_all() { for (auto& s : u.slots) s.have_state = false; for (auto& m : model) m.has = false; }   // api.cpp:305-309

  // runs the round; frames registered at their exact sizes (round_at: each frame its own allocation, at an odd byte offset of its block)
  void call(const std::vector<int32_t>& ids, int S, int h, int w, bool null_frame = false) {
    int oh, ow; u.out_shape(&oh, &ow);
    const size_t in_b = (size_t)std::max(h, 0) * std::max(w, 0) * 3, out_b = (size_t)oh * ow * 3;
    const int n = std::max(S, 0);
    if (!at) {
      BufAt in((size_t)n * in_b), out((size_t)n * out_b); in.filled();
      u.round(static_cast<const uint8_t*>(in.p), ids.data(), S, h, w, static_cast<uint8_t*>(out.p), nullptr);
      if (!hc::cov_covered(out.p, out.bytes)) finding(hc::g_where.desc + " | " + hc::g_where.shape + ": the round left part of the output unwritten");
    } else {
      std::vector<BufP> bufs; std::vector<const uint8_t*> in(n + 1, nullptr); std::vector<uint8_t*> out(n + 1, nullptr);
      for (int i = 0; i < n; ++i) {
        bufs.push_back(std::make_unique<BufAt>(in_b, 1 + 2 * (i % 3))); bufs.back()->filled(); in[i] = static_cast<const uint8_t*>(bufs.back()->p);
        bufs.push_back(std::make_unique<BufAt>(out_b, 3 + 2 * (i % 2))); out[i] = static_cast<uint8_t*>(bufs.back()->p);
        if (i == short_out_item) hc::reg_shrink(out[i], 1);
      }
      if (null_frame && n > 1) in[1] = nullptr;
      u.round_at(in.data(), ids.data(), S, h, w, out.data(), nullptr);
      for (int i = 0; i < n; ++i) if (i != short_out_item && !hc::cov_covered(out[i], out_b)) { finding(hc::g_where.desc + " | " + hc::g_where.shape + ": the round left part of an output frame unwritten"); break; }
    }
  }

  // a slot's buffer that holds q: 0, 1 = lr[0], lr[1]; 2, 3 = hr[0], hr[1]
  bool owner_of(const char* q, int* slot, int* which) const {
    for (size_t s = 0; s < u.slots.size(); ++s)
      for (int k = 0; k < 4; ++k) {
        const DevBuf& b = k < 2 ? u.slots[s].lr[k] : u.slots[s].hr[k - 2];
        if (b.ptr && q >= b.as<char>() && q < b.as<char>() + b.bytes) { *slot = (int)s; *which = k; return true; }
      }
    return false;
  }

  void good(const std::vector<int32_t>& ids) {
    const int S = (int)ids.size();
    char sb[160]; std::snprintf(sb, sizeof sb, "%s | max_streams %zu | %s %d of %d slots, first %d", g.name, u.slots.size(), at ? "round_at" : "round", round_no, S, ids[0]);
    hc::g_where.shape = sb; hc::g_where.model = &f.net;
    if (!keep_launch_index) hc::g_where.launch = 0;
    if (hc::g_trace) std::printf("ROUND %d\n", round_no);
    hc::log_clear(); fr_clear(f);
    std::vector<bool> had(S);
    for (int i = 0; i < S; ++i) had[i] = model[(size_t)ids[i]].has;
    try { call(ids, S, g.ih, g.iw); }
    catch (const std::exception& e) { finding(hc::g_where.desc + " | " + sb + ": exception " + e.what()); ++round_no; return; }
    ++*g_round_count; ++round_no;
    const size_t lr_b = (size_t)3 * g.lh * g.lw * 4, hr_b = 16 * lr_b;
    // per slot buffer: the launches that read it, the ranges written into it
    struct Use { std::vector<const hc::Launch*> reads; int writes = 0; size_t written = 0; };
    std::map<std::pair<int, int>, Use> use;
    for (const hc::Launch& l : hc::g_launch_log)
      for (const hc::Range& r : l.r) {
        int s, k;
        if (!owner_of(r.p, &s, &k)) continue;
        Use& us = use[{s, k}];
        if (r.write) { ++us.writes; us.written += r.bytes; } else us.reads.push_back(&l);
        // an operand tagged with its item belongs to the slot the round names for that item
        if (r.item >= 0 && r.item < S && ids[(size_t)r.item] != s) violation(l, r.operand, "item " + std::to_string(r.item) + " (slot " + std::to_string(ids[(size_t)r.item]) + ") touches a buffer of slot " + std::to_string(s));
      }
    std::vector<bool> in_round(u.slots.size(), false);
    for (int i = 0; i < S; ++i) {
      const int s = ids[(size_t)i];
      in_round[(size_t)s] = true;
      SlotModel& m = model[(size_t)s];
      const FrvsrUpscaler::Slot& sl = u.slots[(size_t)s];
      const char* wrote[2] = {nullptr, nullptr};
      for (int t = 0; t < 2; ++t) {   // t = 0: lr, 1: hr
        const size_t want = t ? hr_b : lr_b;
        int nw = 0;
        for (int k = 0; k < 2; ++k) {
          const DevBuf& b = t ? sl.hr[k] : sl.lr[k];
          if (b.bytes != want) finding(hc::g_where.desc + " | " + sb + ": slot " + std::to_string(s) + " holds a buffer of " + std::to_string(b.bytes) + " bytes, " + std::to_string(want) + " expected");
          auto it = use.find({s, 2 * t + k});
          const Use none;
          const Use& us = it == use.end() ? none : it->second;
          if (us.writes) {   // the round's current frame: written once, by one item, in full
            ++nw; wrote[t] = b.as<char>();
            if (us.writes != 1 || us.written != want) finding(hc::g_where.desc + " | " + sb + ": slot " + std::to_string(s) + (t ? " hr" : " lr") + " written by " + std::to_string(us.writes) + " ranges, " + std::to_string(us.written) + " bytes");
            continue;
          }
          // read and not written: the previous frame
          if (us.reads.empty()) { finding(hc::g_where.desc + " | " + sb + ": slot " + std::to_string(s) + (t ? " hr" : " lr") + ": no launch read a previous frame"); continue; }
          if (had[(size_t)i]) {
            const char* expect = t ? m.hr : m.lr;
            if (b.as<char>() != expect)
              for (const hc::Launch* l : us.reads) violation(*l, t ? "hr_prev" : "lr_prev", "slot " + std::to_string(s) + ": read as the previous frame, but the slot's last round wrote the other buffer as current");
          } else {   // a first frame, or the first after a reset: this round's memsets covered it in full
            bool zeroed = false;
            for (const hc::Memset& ms : hc::g_memset_log) zeroed = zeroed || (ms.p <= b.as<char>() && ms.p + ms.bytes >= b.as<char>() + want);
            if (!zeroed) for (const hc::Launch* l : us.reads) violation(*l, t ? "hr_prev" : "lr_prev", "slot " + std::to_string(s) + ": a stream's first frame reads a previous frame this round did not zero");
          }
        }
        if (nw != 1) finding(hc::g_where.desc + " | " + sb + ": slot " + std::to_string(s) + (t ? " hr" : " lr") + ": " + std::to_string(nw) + " of its two buffers written");
      }
      m.named = m.has = true; m.lr = wrote[0]; m.hr = wrote[1];
    }
    size_t expect_state = 0;
    for (size_t s = 0; s < u.slots.size(); ++s) {
      const FrvsrUpscaler::Slot& sl = u.slots[s];
      if (model[s].named) expect_state += 2 * (lr_b + hr_b);
      else if (sl.lr[0].ptr || sl.lr[1].ptr || sl.hr[0].ptr || sl.hr[1].ptr || sl.have_state) finding(hc::g_where.desc + " | " + sb + ": slot " + std::to_string(s) + " was never named and owns memory");
      if (!in_round[s]) for (int k = 0; k < 4; ++k) if (use.count({(int)s, k})) finding(hc::g_where.desc + " | " + sb + ": slot " + std::to_string(s) + " is not in the round and was touched");
      if (sl.have_state != model[s].has) finding(hc::g_where.desc + " | " + sb + ": slot " + std::to_string(s) + " have_state");
    }
    if (u.state_bytes() != expect_state) finding(hc::g_where.desc + " | " + sb + ": state_bytes " + std::to_string(u.state_bytes()) + ", " + std::to_string(expect_state) + " expected");
  }

  // a round the library must refuse with SS4K_EINVAL, leaving every slot, and the launch, memset and allocation counters, as they were
  void refused(const char* name, const std::vector<int32_t>& ids, int S, int h, int w, bool null_frame = false) {
    hc::g_where.shape = std::string(g.name) + " | refused " + (at ? "round_at: " : "round: ") + name;
    const std::vector<SlotSnap> before = snap_slots(u);
    const long l0 = hc::g_launches, m0 = hc::g_memsets;
    const size_t st0 = u.state_bytes(), live0 = hc::reg_live();
    bool threw = false;
    try { call(ids, S, h, w, null_frame); }
    catch (const Error& e) { threw = true; if (e.code != SS4K_EINVAL) finding(hc::g_where.desc + " | " + hc::g_where.shape + ": Error code " + std::to_string(e.code)); }
    if (!threw) finding(hc::g_where.desc + " | " + hc::g_where.shape + ": accepted");
    ++*g_refused_round_count;
    if (live0 != hc::reg_live()) finding(hc::g_where.desc + " | " + hc::g_where.shape + ": the refusal came after " + std::to_string((long)hc::reg_live() - (long)live0) + " allocations");
    if (!(snap_slots(u) == before) || st0 != u.state_bytes()) finding(hc::g_where.desc + " | " + hc::g_where.shape + ": the refusal came after a slot had changed");
    if (l0 != hc::g_launches || m0 != hc::g_memsets) finding(hc::g_where.desc + " | " + hc::g_where.shape + ": the refusal came after " + std::to_string(hc::g_launches - l0) + " launches and " + std::to_string(hc::g_memsets - m0) + " memsets");
  }
};

std::vector<int32_t> iota_ids(int n, int from = 0, int step = 1) { std::vector<int32_t> v; for (int i = 0; i < n; ++i) v.push_back(from + i * step); return v; }

// the ragged schedule (the pattern of tests/drive_guarded_frvsr_streams.py: ROUNDS) for an upscaler of M slots, with the refused rounds in the middle of it
void schedule(RoundWalk& rw, int M) {
  const Geo& g = rw.g;
  auto refusals = [&] {
    std::vector<int32_t> many = iota_ids(M + 1); many[(size_t)M] = 0;
    rw.refused("S 0", {0}, 0, g.ih, g.iw);
    rw.refused("S > max_streams", many, M + 1, g.ih, g.iw);
    if (M > 1) rw.refused("a slot named twice", {0, 0}, 2, g.ih, g.iw);
    rw.refused("slot max_streams", {M}, 1, g.ih, g.iw);
    rw.refused("slot -1", {-1}, 1, g.ih, g.iw);
    rw.refused("h 0", {0}, 1, 0, g.iw);
    if (rw.at && M > 1) rw.refused("NULL frame", {0, 1}, 2, g.ih, g.iw, true);
  };
  if (M == 1) {
    rw.good({0}); rw.good({0}); refusals(); rw.reset_stream(0); rw.good({0}); rw.good({0}); rw.reset_all(); rw.good({0});
  } else if (M == 4) {   // slot 1 is never named... until the last round
    rw.good({2, 0}); rw.good({2}); rw.good({3, 2, 0}); refusals(); rw.good({2, 3}); rw.reset_stream(2); rw.good({3, 2, 0}); rw.reset_all(); rw.good({0, 3}); rw.good({1, 0, 2, 3});
  } else {
    std::vector<int32_t> all = iota_ids(M), perm;
    for (int i = 0; i < M - 1; ++i) perm.push_back((int32_t)((i * 37 + 11) % M));   // M - 1 distinct slots, permuted (37 is coprime to 64)
    rw.good({9, 3}); rw.good(all); rw.good(perm); refusals(); rw.reset_stream(5); rw.good({5, 9, 1}); rw.reset_all(); rw.good({7, 5}); rw.good(all);
  }
}

void walk_frvsr_rounds(ss4k_ctx& ctx) {
  hc::g_log = true;
  for (int dt : {SS4K_F16, SS4K_F32}) {
    std::unique_ptr<Frvsr> fp;
    auto model = [&]() -> Frvsr& { if (!fp) fp = fr_build(ctx, frdesc(dt, 1)); hc::g_where.desc = frdesc_str(fp->desc); return *fp; };
    for (const Geo& g : GEOS)
      for (int M : {1, 4, 64})
        for (bool at : {false, true}) {
          if (!mine()) continue;
          Frvsr& f = model();
          std::unique_ptr<FrvsrUpscaler> u = make_upscaler(ctx, f, g.lh, g.lw, g.oh, g.ow, M);
          RoundWalk rw(ctx, f, *u, g, at);
          schedule(rw, M);
        }
    // every size a launcher refuses, through round: op_area's grid limit (glue.hip:156) on the way out (out_h 65536) and on the way in (lr_h 65536).
    // ss4k_frvsr_upscaler_create_streams accepts both sizes (api.cpp:288-291)
    if (g_shard == (dt == SS4K_F16 ? 0 : g_shards - 1)) {
      Frvsr& f = model();
      const Geo tall_out{"out_h 65536", 8, 8, 8, 8, 65536, 1}, tall_lr{"lr_h 65536", 65536, 8, 8, 8, 0, 0};
      for (const Geo* g : {&tall_out, &tall_lr}) {
        std::unique_ptr<FrvsrUpscaler> u = make_upscaler(ctx, f, g->lh, g->lw, g->oh, g->ow, 4);
        RoundWalk rw(ctx, f, *u, *g, false);
        fr_clear(f);
        rw.refused(g->name, {2, 0}, 2, g->ih, g->iw);
      }
    }
    hc::g_where.model = nullptr;
  }
  hc::g_log = false;
}

// =================================================================== the frame upscaler (upscaler.cpp: Upscaler::multi / single)
long g_jobs = 0, g_refused_jobs = 0;

std::unique_ptr<Model> build_model(ss4k_ctx& ctx, const ss4k_model_desc& d) {
  const std::vector<float> blob = make_blob(d, 0);
  auto m = std::make_unique<Model>();
  m->ctx = &ctx; m->desc = d;
  hc::g_where.desc = desc_str(d); hc::g_where.shape = "build"; hc::g_where.model = nullptr;
  m->build(blob.data(), blob.size());
  g_weights += (double)blob.size();
  return m;
}

// the way ss4k_upscaler_create builds the object (api.cpp:103-108); its refusals (api.cpp:98-102) are the caller's to respect here
std::unique_ptr<Upscaler> make_frame_upscaler(ss4k_ctx& ctx, const ss4k_upscale_cfg& cfg, Model* sr, Model* dn) {
  auto u = std::make_unique<Upscaler>();
  u->ctx = &ctx; u->cfg = cfg; u->sr = sr; u->dn = dn;
  u->upload_taps();
  u->for_each_job_buf([](DevBuf& b) { b.transient = true; });
  return u;
}

// what Upscaler::multi / single refuse, restated from the reference's constraints and the launchers' own: RRDBNet's pixel-unshuffle factor
// (models.cpp: "divisible by the pixel-unshuffle factor"), BSVD's two 2 x 2 poolings (models.cpp: "divisible by 4"), the 17-tap blur's reflect
// padding on an HR / 8 map no wider than 8 (upscaler.cpp: "local colour match")
bool job_must_be_refused(const Upscaler& u, int n, int h, int w) {
  const ss4k_upscale_cfg& c = u.cfg;
  const bool to_lr = c.single_mode || ((w > c.lr_w || h > c.lr_h) && c.lr_hr_resize);   // fsrcnn_upscaler.py:173-176,239-241
  const int lh = to_lr ? c.lr_h : h, lw = to_lr ? c.lr_w : w, s = u.sr->desc.scale;
  if (u.sr->desc.kind == SS4K_RRDBNET && s != 4) { const int r = s == 2 ? 2 : 4; if (lh % r || lw % r) return true; }
  if (c.denoising && (lh % 4 || lw % 4)) return true;
  if (!c.single_mode) { const int H = lh * s, W = lw * s; if (H / 8 > 8 && H > 64 && W > 64 && W / 8 <= 8) return true; }
  // one statistics record per colour plane, STATS_MAX_PLANES of them (glue.h); FSRCNN reading the uint8 frames itself sums the frames' planes and the
  // output's into one set (upscaler.cpp: u8_direct)
  const bool u8_direct = c.single_mode && !u.taps_on && !c.denoising && !c.sr_is_realesrgan && h == lh && w == lw && u.sr->can_u8_in();
  if (3 * n > STATS_MAX_PLANES || (u8_direct && 6 * n > STATS_MAX_PLANES)) return true;
  return false;
}

struct JobWalk {
  Upscaler& u; std::string name;
  void clear() {   // fresh per-job buffers and activations: the job is audited against exactly what it asks for
    u.for_each_job_buf([](DevBuf& b) { b.release(); });
    u.sr->acts.clear(); if (u.dn) u.dn->acts.clear();
  }
  void job(int n, int h, int w, bool cleared = true) {
    char sb[200]; std::snprintf(sb, sizeof sb, "%s | job of %d frames %d x %d%s", name.c_str(), n, h, w, cleared ? "" : " (buffers kept)");
    hc::g_where.shape = sb; hc::g_where.launch = 0; hc::g_where.model = u.sr; hc::g_where.desc = desc_str(u.sr->desc);
    hc::log_clear();
    if (cleared) clear();
    int oh = 0, ow = 0; u.out_shape(h, w, &oh, &ow);
    BufAt in((size_t)n * h * w * 3), out((size_t)n * oh * ow * 3); in.filled();
    const bool must_refuse = job_must_be_refused(u, n, h, w), first0 = u.first_frame, clean0 = u.acc2_clean;
    const long l0 = hc::g_launches, a0 = hc::g_allocs, m0 = hc::g_memsets; const size_t live0 = hc::reg_live();
    const std::string where = hc::g_where.desc + " | " + sb;
    try {
      if (u.cfg.single_mode) u.single(static_cast<const uint8_t*>(in.p), n, h, w, static_cast<uint8_t*>(out.p), nullptr);   // api.cpp:125-126
      else u.multi(static_cast<const uint8_t*>(in.p), n, h, w, static_cast<uint8_t*>(out.p), nullptr);
    } catch (const Error& e) {
      ++g_refused_jobs;
      if (e.code != SS4K_EINVAL) finding(where + ": Error code " + std::to_string(e.code) + ": " + e.what());
      else if (!must_refuse) finding(where + ": refused: " + e.what());
      if (l0 != hc::g_launches || a0 != hc::g_allocs || m0 != hc::g_memsets || live0 != hc::reg_live() || first0 != u.first_frame || clean0 != u.acc2_clean)
        finding(where + ": the refusal (" + e.what() + ") came after " + std::to_string(hc::g_launches - l0) + " launches and " + std::to_string(hc::g_allocs - a0) + " allocations");
      return;
    } catch (const std::exception& e) { finding(where + ": exception " + e.what()); return; }
    ++g_jobs;
    if (must_refuse) finding(where + ": accepted, a refusal was expected");
    if (!hc::cov_covered(out.p, out.bytes)) finding(where + ": the job left part of the output unwritten");
    if (u.acc2_clean && u.st_acc2.ptr) {   // the contract of upscaler.h: clean after the finishing launch
      const char* p = u.st_acc2.as<char>(); size_t nz = 0;
      for (size_t i = 0; i < u.st_acc2.bytes; ++i) nz += p[i] != 0;
      if (nz) finding(where + ": acc2_clean is set and st_acc2 holds " + std::to_string(nz) + " non-zero bytes");
    }
  }
};

void walk_upscaler(ss4k_ctx& ctx) {
  hc::g_log = true;
  // SR models: FSRCNN x2 / x4, SRVGG 16 x 1 (fp16: the half HR tensor), RRDBNet 32 x 32 with one block (x2: the pixel-unshuffle front end); the
  // models of tests/drive_guarded.py: SRVGG 16 x 2 fp32, SRVGG 64 x 4 fp16, FSRCNN x2 in both dtypes, BSVD (32, 64, 128), mid 32, interm 30
  struct Sr { const char* name; ss4k_model_desc d; bool rgb; std::unique_ptr<Model> m; };
  Sr srs[] = {{"fsrcnn x2 f32", fsr(SS4K_F32, 2, 0), false, nullptr}, {"fsrcnn x4 f16", fsr(SS4K_F16, 4, 0), false, nullptr}, {"srvgg 16x1 x4 f16", srvgg(SS4K_F16, 4, 16, 1, 0), true, nullptr},
              {"rrdbnet 32x32 x2 f32", rrdb(SS4K_F32, 2, 32, 32, 0), true, nullptr}, {"srvgg 16x2 x4 f32", srvgg(SS4K_F32, 4, 16, 2, 0), true, nullptr},
              {"srvgg 64x4 x4 f16", srvgg(SS4K_F16, 4, 64, 4, 0), true, nullptr}, {"fsrcnn x2 f16", fsr(SS4K_F16, 2, 0), false, nullptr}};
  std::unique_ptr<Model> dn;
  auto sr_model = [&](Sr& s) -> Model* { if (!s.m) s.m = build_model(ctx, s.d); return s.m.get(); };
  auto dn_model = [&]() -> Model* { if (!dn) dn = build_model(ctx, bsvd(SS4K_F16, 32, 64, 128, 32, 30, 0, 0)); return dn.get(); };
  auto config = [&](Sr& s, bool single, bool denoise, bool lr_hr_resize, int lr_h, int lr_w, int out_h, int out_w, bool taps, const char* tag) {
    ss4k_upscale_cfg c{}; c.lr_h = lr_h; c.lr_w = lr_w; c.out_h = out_h; c.out_w = out_w; c.lr_hr_resize = lr_hr_resize; c.single_mode = single; c.sr_is_realesrgan = s.rgb;
    c.denoising = denoise; c.denoise_rate = 1.0;
    std::unique_ptr<Upscaler> u = make_frame_upscaler(ctx, c, sr_model(s), denoise ? dn_model() : nullptr);
    u->taps_on = taps;
    char nb[200]; std::snprintf(nb, sizeof nb, "%s%s | %s%s%s lr %d x %d out %d x %d taps %d", tag, s.name, single ? "single" : "multi", denoise ? " denoise" : "", lr_hr_resize ? " lr_hr_resize" : "", lr_h, lr_w, out_h, out_w, (int)taps);
    return std::make_pair(std::move(u), std::string(nb));
  };
  // ---- the 14 configurations of tests/drive_guarded.py (SERVICE), their jobs of 3, 1 and 2 frames on one upscaler
  struct Dg { int sr; bool dn; int lh, lw, oh, ow; bool single; int h, w; bool taps; };
  const Dg dgs[] = {{4, false, 72, 128, 144, 256, false, 72, 128, false}, {0, false, 90, 124, 0, 0, true, 90, 124, false}, {5, false, 72, 128, 0, 0, false, 72, 128, false},
                    {0, true, 72, 128, 100, 180, true, 72, 128, false}, {4, false, 72, 128, 0, 0, false, 108, 192, false}, {4, false, 72, 128, 144, 256, false, 72, 128, true},
                    {4, false, 12, 16, 0, 0, false, 12, 16, true}, {4, false, 12, 16, 0, 0, false, 12, 16, false}, {5, false, 24, 32, 60, 90, false, 24, 32, false},
                    {6, false, 45, 62, 0, 0, true, 90, 124, false}, {0, false, 45, 62, 100, 150, true, 90, 124, false}, {0, true, 40, 64, 100, 150, true, 40, 64, true},
                    {5, false, 24, 32, 0, 0, true, 24, 32, false}, {6, false, 45, 62, 100, 150, true, 45, 62, false}};
  for (const Dg& d : dgs) {
    if (!mine()) continue;
    auto [u, name] = config(srs[d.sr], d.single, d.dn, true, d.lh, d.lw, d.oh, d.ow, d.taps, "drive_guarded: ");
    JobWalk jw{*u, name};
    for (int n : {3, 1, 2}) jw.job(n, d.h, d.w);
  }
  // ---- the cross product of the axes, every end of every axis: single_mode x SR model (the first four) x denoising x lr_hr_resize x output_shape
  // none, smaller, larger x taps x frame size x lr_shape equal to the frame size or not (12 x 20).  Per configuration: a job of 5 frames, then
  // jobs of 2 and 1 on the same object with the per-job buffers cleared in between, then one of 2 with everything kept (acc2_clean)
  const int frames[][2] = {{1, 1}, {7, 9}, {17, 33}, {36, 64}}, outs[][2] = {{0, 0}, {5, 7}, {150, 270}};
  for (int single = 0; single < 2; ++single)
    for (int si = 0; si < 4; ++si)
      for (int denoise = 0; denoise < 2; ++denoise)
        for (int rs = 0; rs < 2; ++rs)
          for (auto& o : outs)
            for (int taps = 0; taps < 2; ++taps)
              for (auto& fr : frames)
                for (int same_lr = 0; same_lr < 2; ++same_lr) {
                  // what ss4k_upscaler_create refuses (api.cpp:100-101): denoising on the batched path, a one-channel SR model on the batched path
                  if ((denoise && !single) || (!single && !srs[si].rgb)) continue;
                  if (!mine()) continue;
                  auto [u, name] = config(srs[si], single, denoise, rs, same_lr ? fr[0] : 12, same_lr ? fr[1] : 20, o[0], o[1], taps, "");
                  JobWalk jw{*u, name};
                  jw.job(5, fr[0], fr[1]); jw.job(2, fr[0], fr[1]); jw.job(1, fr[0], fr[1]); jw.job(2, fr[0], fr[1], false);
                }
  // ---- the refusals no point above reaches: an HR tensor 68 wide under the local colour match (its HR / 8 map is as wide as the blur's reflect
  // padding), and jobs of more colour planes than the statistics hold: 683 frames where two sets share the accumulators, 1366 anywhere
  if (mine()) {
    auto [u, name] = config(srs[2], false, false, false, 20, 17, 0, 0, false, "colour map 8 wide: ");
    JobWalk jw{*u, name};
    jw.job(1, 20, 17); jw.job(1, 20, 18);   // (72 wide: accepted)
  }
  for (int taps = 0; taps < 2; ++taps) {
    if (!mine()) continue;
    auto [u, name] = config(srs[0], true, false, false, 1, 1, 0, 0, taps, "statistics planes: ");
    JobWalk jw{*u, name};
    jw.job(682, 1, 1); jw.job(683, 1, 1); jw.job(1365, 1, 1); jw.job(1366, 1, 1);
  }
  hc::g_where.model = nullptr;
  hc::g_log = false;
}

// =================================================================== the other five (generator, degradation, route) variants of the executor
// Descriptions, steps and rounds as above, thinned, with counters of their own (g_var_*): the walk above and its totals stay what they were.
void walk_variants(ss4k_ctx& ctx) {
  hc::g_log = true;
  g_step_count = &g_var_steps; g_round_count = &g_var_rounds; g_refused_round_count = &g_var_refused_rounds;
  const int thin[] = {8, 9, 15, 16, 17, 23, 31, 33};
  for (const Variant& v : VARIANTS) {
    const bool teco = v.gen == SS4K_FRVSR_TECOGAN, phase = v.route == SS4K_FRVSR_CONVT_PHASE;
    // ---- descriptions: num_block 0, 2 x both dtypes, one step each; on the phase route at num_block 2 both pack_convt3x3s2 blobs are bijections
    for (int nb : {0, 2})
      for (int dt : {SS4K_F16, SS4K_F32}) {
        if (!mine()) continue;
        const ss4k_frvsr_desc d = frdesc(dt, nb);
        try {
          std::unique_ptr<Frvsr> a = fr_build(ctx, d, 0, v);
          ++g_var_accepted;
          // FNet's 14, conv_in, the blocks' two each; TecoGAN: conv_out, and on the embedded route the two W_eq layers
          if ((int)a->net.layers.size() != 15 + 2 * nb + (teco ? (phase ? 1 : 3) : 0)) finding(hc::g_where.desc + ": layer count");
          run_step(*a, 1, 9, 15, ROUTE_CONTIG, false);
          if (nb == 2 && phase) {
            std::unique_ptr<Frvsr> b = fr_build(ctx, d, 1, v);
            for (int k = 0; k < 2; ++k) {
              bijection_blob(frdesc_str(d, v) + " conv_up." + std::to_string(2 * k) + " (pack_convt3x3s2)", LSpec{64, 64, false, 0}, a->teco.up_w[k].ptr, b->teco.up_w[k].ptr, dt == SS4K_F16);
              ++g_bij_layers;
            }
          }
        } catch (const std::exception& e) { finding(frdesc_str(d, v) + " | " + hc::g_where.shape + ": exception " + e.what()); }
        hc::g_where.model = nullptr;
      }
    for (int dt : {SS4K_F16, SS4K_F32}) {
      std::unique_ptr<Frvsr> fp;
      auto model = [&]() -> Frvsr& { if (!fp) fp = fr_build(ctx, frdesc(dt, 1), 0, v); hc::g_where.desc = frdesc_str(fp->desc, v); return *fp; };
      // ---- steps: the thinned (h, w) set at n = 1 (taps off and on), 2, 3 (taps on); n = 64 at {8, 9}^2 alone (a 64-channel (4 h, 4 w) tensor for
      // 64 items of 33 x 33 is 285 MB under the sanitizers); the three packing routes, run_step's checks as they are
      auto point = [&](int n, int h, int w, std::initializer_list<bool> taps) {
        if (!mine()) return;
        Frvsr& f = model();
        try {
          for (bool kt : taps) {
            std::string seq[3];
            for (int route = 0; route < 3; ++route) seq[route] = run_step(f, n, h, w, route, kt);
            if (seq[0] != seq[1] || seq[0] != seq[2]) finding(hc::g_where.desc + " | n " + std::to_string(n) + " " + std::to_string(h) + " x " + std::to_string(w) + ": the three routes differ in their launch sequence");
          }
        } catch (const std::exception& e) { finding(hc::g_where.desc + " | " + hc::g_where.shape + ": exception " + e.what()); }
      };
      for (int h : thin) for (int w : thin) point(1, h, w, {false, true});
      for (int n : {2, 3}) for (int h : thin) for (int w : thin) point(n, h, w, {true});
      for (int h : {8, 9}) for (int w : {8, 9}) point(64, h, w, {true});
      // ---- TecoGAN's group walk: groups of 1 and 2 items at n = 3, 5 - a group offset i0 > 0 and a short last group.  run_step holds that every
      // item's hr_out is covered and that the activations are what workspace_bytes planned; here: the tail's three workspaces are ONE group's
      if (teco)
        for (int gi : {1, 2}) for (int n : {3, 5}) for (auto hw : {std::pair<int, int>{9, 15}, {17, 8}}) for (int route : {ROUTE_CONTIG, ROUTE_ITEMS}) {
          if (!mine()) continue;
          Frvsr& f = model();
          f.teco.dev.group_items = gi;
          try {
            run_step(f, n, hw.first, hw.second, route, true);
            // slots 0..24 are the step's (2 inputs, FNet's 19, the warp's planes, SRNet's 3); 25..27 the tail's U1, U2 (four planes each) and conv_out's
            const size_t px = (size_t)gi * hw.first * hw.second, rec = (size_t)f.net.rec();
            const size_t want[3] = {4 * px * rec * 4, 16 * px * rec * 4, 16 * px * rec};
            bool ok = f.net.acts.size() == 28;
            for (int k = 0; ok && k < 3; ++k) ok = f.net.acts[25 + (size_t)k].bytes == want[k];
            if (!ok) finding(hc::g_where.desc + " | " + hc::g_where.shape + ", group_items " + std::to_string(gi) + ": the tail's workspaces are not one group's");
          } catch (const std::exception& e) { finding(hc::g_where.desc + " | " + hc::g_where.shape + ": exception " + e.what()); }
          f.teco.dev.group_items = 0;
        }
      // ---- rounds: a geometry without resize, one with an input resize, one with an output_shape; max_streams 4; the ragged schedule with its refusals
      for (const Geo* g : {&GEOS[0], &GEOS[1], &GEOS[2]})
        for (bool at : {false, true}) {
          if (!mine()) continue;
          Frvsr& f = model();
          std::unique_ptr<FrvsrUpscaler> u = make_upscaler(ctx, f, g->lh, g->lw, g->oh, g->ow, 4);
          RoundWalk rw(ctx, f, *u, *g, at);
          schedule(rw, 4);
        }
      hc::g_where.model = nullptr;
    }
  }
  g_step_count = &g_steps; g_round_count = &g_rounds; g_refused_round_count = &g_refused_rounds;
  hc::g_log = false;
  if (g_shard != 0) return;
  // ---- refused, with SS4K_EINVAL (and 0 from frvsr_param_count where the generator or the degradation is none): the triple is validated in Frvsr::build
  const ss4k_frvsr_desc d = frdesc(SS4K_F16, 1);
  auto refuse_variant = [&](const char* name, const Variant& obj, const Variant& blob_of, bool no_count) {
    hc::g_where.desc = std::string("invalid frvsr variant: ") + name; hc::g_where.shape = "build";
    try {
      if (no_count && frvsr_param_count(d, obj.gen, obj.deg) != 0) finding(std::string(name) + ": frvsr_param_count answers " + std::to_string(frvsr_param_count(d, obj.gen, obj.deg)));
      const std::vector<float> blob = fr_blob(d, 0, blob_of);
      Frvsr f; f.ctx = &ctx; f.desc = d; f.generator = obj.gen; f.degradation = obj.deg; f.route_flags = obj.route;
      f.build(blob.data(), blob.size());
      finding(std::string(name) + ": built");
    } catch (const Error& e) {
      if (e.code == SS4K_EINVAL) ++g_var_refused; else finding(std::string(name) + ": Error code " + std::to_string(e.code));
    } catch (const std::exception& e) { finding(std::string(name) + ": exception " + e.what()); }
  };
  const Variant &EGVSR_BI = VARIANTS[0], &TECO_BD = VARIANTS[1];
  for (int g : {-1, 2}) refuse_variant("generator", Variant{"", g, SS4K_FRVSR_BD, 0}, EGVSR_BD, true);
  for (int g : {-1, 2}) refuse_variant("degradation", Variant{"", SS4K_FRVSR_EGVSR, g, 0}, EGVSR_BD, true);
  refuse_variant("route flags 2 (unknown bit)", Variant{"", SS4K_FRVSR_TECOGAN, SS4K_FRVSR_BD, 2}, TECO_BD, false);
  refuse_variant("route flags 5 (both pins)", Variant{"", SS4K_FRVSR_TECOGAN, SS4K_FRVSR_BD, 5}, TECO_BD, false);
  refuse_variant("route flags 1 on EGVSR", Variant{"", SS4K_FRVSR_EGVSR, SS4K_FRVSR_BD, 1}, EGVSR_BD, false);
  refuse_variant("a 'BD' blob on a 'BI' object", EGVSR_BI, EGVSR_BD, false);
  refuse_variant("a 'BI' blob on a 'BD' object", EGVSR_BD, EGVSR_BI, false);
  refuse_variant("EGVSR's blob on TecoGAN", TECO_BD, EGVSR_BD, false);
}

// ---- positive controls of the round walk: each must be reported at exactly the launches that touch the object named (the test reads the launch
// kinds from the trace).  One fp32 upscaler of 4 slots at lr 8 x 8, round_at, launches numbered through all rounds.  teco-hr-short: hr-short on a
// TecoGAN / 'BI' generator, whose warp and skip are the launchers of frvsr_bi.hip.
int control_frvsr(const char* what) {
  ss4k_ctx ctx;
  hc::g_log = true; hc::g_trace = true;
  const bool teco = !std::strncmp(what, "teco-", 5);
  const Variant& v = teco ? VARIANTS[3] : EGVSR_BD;
  std::unique_ptr<Frvsr> f = fr_build(ctx, frdesc(SS4K_F32, 1), 0, v);
  hc::g_where.desc = frdesc_str(f->desc, v);
  std::unique_ptr<FrvsrUpscaler> u = make_upscaler(ctx, *f, 8, 8, 0, 0, 4);
  RoundWalk rw(ctx, *f, *u, GEOS[0], true);
  rw.keep_launch_index = true; hc::g_where.launch = 0;
  rw.good({2, 0});
  if (hc::g_violations || g_findings) { std::printf("CONTROL setup failed\n"); return 2; }
  if (!std::strcmp(what, "hr-short") || !std::strcmp(what, "teco-hr-short")) {   // slot 2's previous HR frame registered 4 bytes short: read by round 1's warp, written by round 2's tail, read by its output glue
    hc::reg_shrink(u->slots[2].hr[u->slots[2].cur].ptr, 4);
    rw.good({2}); rw.good({3, 2, 0});
  } else if (!std::strcmp(what, "out-short")) {  // item 1's output frame one byte short: the round's output glue
    rw.short_out_item = 1;
    rw.good({3, 2, 0});
  } else if (!std::strcmp(what, "cur")) {        // test-only hook: slot 2's `cur` as if close_slots had not flipped it: round 1 reads the wrong previous frames
    u->slots[2].cur ^= 1;
    rw.good({2});
  } else return 2;
  hc::g_where.model = nullptr;
  std::printf("CONTROL frvsr %s violations=%ld findings=%ld\n", what, hc::g_violations, g_findings);
  return 0;
}

// --trace-frvsr dtype num_block n h w [generator degradation route_flags]: the launches of one step through each of the three routes
int trace_frvsr(char** v, bool with_variant) {
  ss4k_ctx ctx;
  hc::g_log = true;
  try {
    const Variant var = with_variant ? Variant{"(--trace-frvsr)", std::atoi(v[5]), std::atoi(v[6]), std::atoi(v[7])} : EGVSR_BD;
    std::unique_ptr<Frvsr> f = fr_build(ctx, frdesc(std::atoi(v[0]), std::atoi(v[1])), 0, with_variant ? var : EGVSR_BD);
    hc::g_where.desc = frdesc_str(f->desc, with_variant ? var : EGVSR_BD); hc::g_trace = true;
    for (int route = 0; route < 3; ++route) {
      std::printf("ROUTE %s\n", ROUTE_NAMES[route]);
      run_step(*f, std::atoi(v[2]), std::atoi(v[3]), std::atoi(v[4]), route, true);
    }
    hc::g_where.model = nullptr;
  } catch (const Error& e) { std::printf("refused (%d): %s\n", e.code, e.what()); }
  return hc::g_violations || g_findings ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  std::setvbuf(stdout, nullptr, _IOLBF, 0);
  if (argc == 18 && !std::strcmp(argv[1], "--trace")) return trace(argv + 2);
  if (argc >= 3 && !std::strcmp(argv[1], "--control-shrink")) return control_shrink(std::atoi(argv[2]));
  if (argc >= 2 && !std::strcmp(argv[1], "--control-short-blob")) return control_short_blob();
  if (argc >= 3 && !std::strcmp(argv[1], "--control-frvsr")) return control_frvsr(argv[2]);
  if ((argc == 7 || argc == 10) && !std::strcmp(argv[1], "--trace-frvsr")) return trace_frvsr(argv + 2, argc == 10);
  const char* only = (argc >= 3 && !std::strcmp(argv[1], "--only")) ? argv[2] : nullptr;   // one part of the walk (measurement)
  if (argc >= 4 && !std::strcmp(argv[1], "--shard")) { g_shard = std::atoi(argv[2]); g_shards = std::max(1, std::atoi(argv[3])); }
  if (g_shard < 0 || g_shard >= g_shards) { std::printf("usage: hostcheck [--shard I N | --only PART | --control-shrink BUFFER | --control-short-blob | --control-frvsr WHAT | --trace-frvsr DTYPE NB N H W [GENERATOR DEGRADATION ROUTE]]\n"); return 2; }
  const auto t0 = std::chrono::steady_clock::now();
  {
    ss4k_ctx ctx;
    if ((!only && g_shard == 0) || (only && !std::strcmp(only, "invalid"))) walk_invalid(ctx);   // (the invalid descriptions and the tables: first shard)
    walk_lattice(ctx, only);
    if (!only || !std::strcmp(only, "frvsr-descs")) walk_frvsr_descs(ctx);
    if (!only || !std::strcmp(only, "frvsr-steps")) walk_frvsr_steps(ctx);
    if (!only || !std::strcmp(only, "frvsr-rounds")) walk_frvsr_rounds(ctx);
    if (!only || !std::strcmp(only, "upscaler")) walk_upscaler(ctx);
    if (!only || !std::strcmp(only, "variants")) walk_variants(ctx);
    if ((!only && g_shard == 0) || (only && !std::strcmp(only, "tables"))) walk_tables();
  }
  if (hc::reg_live()) finding(std::to_string(hc::reg_live()) + " allocations still live at the end");
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("HOSTCHECK accepted=%ld refused=%ld shapes=%ld launches=%ld bijection_layers=%ld frvsr_accepted=%ld frvsr_refused=%ld steps=%ld refused_steps=%ld rounds=%ld refused_rounds=%ld jobs=%ld refused_jobs=%ld "
              "variant_accepted=%ld variant_refused=%ld variant_steps=%ld variant_rounds=%ld variant_refused_rounds=%ld violations=%ld findings=%ld\n",
              g_accepted, g_refused, g_shapes, hc::g_launches, g_bij_layers, g_fr_accepted, g_fr_refused, g_steps, g_refused_steps, g_rounds, g_refused_rounds, g_jobs, g_refused_jobs,
              g_var_accepted, g_var_refused, g_var_steps, g_var_rounds, g_var_refused_rounds, hc::g_violations, g_findings);
  std::printf("TIME %.1f s for %.0f M parameters packed\n", sec, g_weights / 1e6);
  return (hc::g_violations || g_findings) ? 1 : 0;
}
