// Pure host-side table builders of the C ABI (api.cpp, upscaler.cpp): no HIP call, no state.  They live in a header so that a host-only
// program (tests/hostcheck) can run them under the sanitizers exactly as the library does.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace ss4k {

// blur_ker (fsrcnn_upscaler.py:20-52) as its 1-D factor: the reference's normalised 2-D kernel
// (1 / (2 pi var)) exp(-(dx^2 + dy^2) / (2 var)) / sum is g[y] * g[x] with g = e / sum(e)
inline std::vector<float> gaussian_taps_1d(int k, float sigma) {
  std::vector<float> g(k);
  const float mean = (k - 1) / 2.0f, var = sigma * sigma;
  double sum = 0.0;
  for (int i = 0; i < k; ++i) { const float d = i - mean; g[i] = expf(-(d * d) / (2 * var)); sum += g[i]; }
  for (auto& v : g) v = (float)(v / sum);
  return g;
}

// cv2.resize(..., INTER_AREA) tables (ss4k_op_cv_area_resize_u8; oracle/cv_area.py states the algorithm)
struct CvEnt { int si; float a; };
// computeResizeAreaTab: the entries of every output cell [d * scale, (d + 1) * scale), in order; ofs[d] = first entry of cell d
inline void cv_area_tab(int ssize, int dsize, double scale, std::vector<CvEnt>& ent, std::vector<int>& ofs) {
  ent.clear(); ofs.assign(dsize + 1, 0);
  for (int d = 0; d < dsize; ++d) {
    ofs[d] = (int)ent.size();
    const double fs1 = d * scale, fs2 = fs1 + scale, cell = std::min(scale, ssize - fs1);
    int s1 = (int)std::ceil(fs1), s2 = (int)std::floor(fs2);
    s2 = std::min(s2, ssize - 1);
    s1 = std::min(s1, s2);
    if (s1 - fs1 > 1e-3) ent.push_back({s1 - 1, (float)((s1 - fs1) / cell)});
    for (int sx = s1; sx < s2; ++sx) ent.push_back({sx, float(1.0 / cell)});
    if (fs2 - s2 > 1e-3) ent.push_back({s2, (float)(std::min(std::min(fs2 - s2, 1.), cell) / cell)});
  }
  ofs[dsize] = (int)ent.size();
}

}  // namespace ss4k
