// The FRV_WARP stage of a frame-recurrent generator built with degradation 'BI' (reference utils/net_utils.py:96-108: the up-sampling function
// is F.interpolate(scale_factor=4, mode='bilinear', align_corners=False)): hr_flow = 4 * bilinear x4 (lr_flow), backward_warp(hr_prev, hr_flow),
// space-to-depth (egvsr.py:196-208), one launch of frvsr_bi.hip.  Frvsr::run (frvsr.cpp) calls it through FrvsrWarp; the file holds the stage
// together with the launchers it names, so that frvsr.cpp links wherever it linked before.  TecoGAN's 'BI' skip is in its tail (frvsr_teco.cpp).
#include "frvsr.h"

namespace ss4k {

namespace {

struct BilinearWarp final : FrvsrWarp {
  void run(Frvsr& f, const Call& c, hipStream_t st) override {
    const bool f16 = f.desc.dtype == SS4K_F16;
    if (c.items) {
      if (f16) op_warp_s2d_bi_planes_items<__half>(c.flow, *c.items, reinterpret_cast<__half*>(c.out), c.n, c.h, c.w, st);
      else op_warp_s2d_bi_planes_items<float>(c.flow, *c.items, reinterpret_cast<float*>(c.out), c.n, c.h, c.w, st);
    } else if (f16) op_warp_s2d_bi_planes<__half>(c.flow, c.hr_prev, reinterpret_cast<__half*>(c.out), c.n, c.h, c.w, st);
    else op_warp_s2d_bi_planes<float>(c.flow, c.hr_prev, reinterpret_cast<float*>(c.out), c.n, c.h, c.w, st);
  }
};

}  // namespace

std::unique_ptr<FrvsrWarp> make_bilinear_warp() { return std::make_unique<BilinearWarp>(); }

}  // namespace ss4k
