// Walks the lattice of model descriptions the library accepts ("Host check"): every accepted description is built from a
// generated weight blob and run through workspace_bytes and a real forward for every shape, with the launch auditors
// (auditors.cpp) in place of the kernels; every invalid description must be refused with SS4K_EINVAL.  Built with ASan + UBSan.
//
//   hostcheck                      the whole walk; prints one HOSTCHECK line with the counts, exit status 1 on any finding
//   hostcheck --shard I N          every N-th lattice point from the I-th (shard 0 also takes the invalid descriptions and the tables)
//   hostcheck --only PART          rrdbnet | srvgg | bsvd | bounds | fsrcnn | invalid | tables (for measuring)
//   hostcheck --trace kind dtype scale num_feat num_block num_grow_ch c0 c1 c2 mid_ch interm_ch stream flags frames H W
//                                  one line per launch of that description at that layer-resolution shape (which route a width takes)
//   hostcheck --control-shrink I   positive control: one RRDBNet forward with activation buffer I registered one plane short
//   hostcheck --control-short-blob positive control: a blob one float short must be refused with SS4K_EINVAL
#include "hostcheck.h"
#include "../../sharkshark-4k_amd/csrc/models.h"
#include "../../sharkshark-4k_amd/csrc/host_tables.h"
#include <array>
#include <chrono>
#include <climits>
#include <cmath>

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

}  // namespace

int main(int argc, char** argv) {
  std::setvbuf(stdout, nullptr, _IOLBF, 0);
  if (argc == 18 && !std::strcmp(argv[1], "--trace")) return trace(argv + 2);
  if (argc >= 3 && !std::strcmp(argv[1], "--control-shrink")) return control_shrink(std::atoi(argv[2]));
  if (argc >= 2 && !std::strcmp(argv[1], "--control-short-blob")) return control_short_blob();
  const char* only = (argc >= 3 && !std::strcmp(argv[1], "--only")) ? argv[2] : nullptr;   // one part of the walk (measurement)
  if (argc >= 4 && !std::strcmp(argv[1], "--shard")) { g_shard = std::atoi(argv[2]); g_shards = std::max(1, std::atoi(argv[3])); }
  if (g_shard < 0 || g_shard >= g_shards) { std::printf("usage: hostcheck [--shard I N | --only PART | --control-shrink BUFFER | --control-short-blob]\n"); return 2; }
  const auto t0 = std::chrono::steady_clock::now();
  {
    ss4k_ctx ctx;
    if ((!only && g_shard == 0) || (only && !std::strcmp(only, "invalid"))) walk_invalid(ctx);   // (the invalid descriptions and the tables: first shard)
    walk_lattice(ctx, only);
    if ((!only && g_shard == 0) || (only && !std::strcmp(only, "tables"))) walk_tables();
  }
  if (hc::reg_live()) finding(std::to_string(hc::reg_live()) + " allocations still live at the end");
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("HOSTCHECK accepted=%ld refused=%ld shapes=%ld launches=%ld bijection_layers=%ld violations=%ld findings=%ld\n", g_accepted, g_refused, g_shapes,
              hc::g_launches, g_bij_layers, hc::g_violations, g_findings);
  std::printf("TIME %.1f s for %.0f M parameters packed\n", sec, g_weights / 1e6);
  return (hc::g_violations || g_findings) ? 1 : 0;
}
