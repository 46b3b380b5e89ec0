// The motion-adaptive noise map of a round (upscaler_temporal.cpp, frvsr_temporal.cpp; the kernel is tround::gather_planes_motion in
// temporal_round.hip): which frames of a round get the constant plane, where every other frame finds its stream's PREVIOUS LR frame, and the
// numbers of the rule.  A pure function of the round's plan: no HIP and no allocation; it includes the two plan headers it sits on.
// tests/temporal_motion_plan_check.cpp replays random rounds against a naive per-stream simulation.
//
// The rule (the reference computes it and then overwrites it with the constant: fsrcnn_upscaler.py:250-254, :262).  Frame t of a stream, t > 0,
// not flagged as a scene's first:
//   D = mean over the three planes of |x_t - x_{t-1}|;  B = D correlated with the 3 x 3 Gaussian of sigma 0.5, borders by 'reflect';
//   m_t = min(max(10 B, 0), 0.1f) * (float)(0.35 * rate).
// x_{t-1} is the frame as it went IN (the reference's is the previous frame after denoising and blending, which does not exist here until 16
// frames later).  It is still in the stream's LR ring: frame n of a stream sits in ring slot n % R, R = LAG + max_push, and a round writes the
// slots before.pushed .. before.pushed + n_item - 1 (mod R) of an item's stream - at most max_push <= R - LAG slots starting at before.pushed - so
// slot (before.pushed - 1) % R, the predecessor of an item's first frame, is not among them, and a later frame's predecessor is a slot this round
// writes for the SAME stream with its frames-in launch, before the gather on the same stream.
#pragma once
#include "bsvd_online_plan.h"
#include "temporal_round_plan.h"
#include <cmath>

namespace ss4k {
namespace temporal_round {

struct Motion {
  int ring_prev[MAX_FRAMES] = {};          // for frame order[q] of the plan: the ring slot of its stream's previous frame, -1: it has none
  unsigned long long constant_bits = 0;    // bit q: frame order[q] is its stream's first and gets the constant plane
};

inline Motion make_motion(const Plan& p, int max_push) {
  Motion m;
  const int R = ring_frames(max_push);
  for (int t = 0; t < p.n_items; ++t) {
    const Item& it = p.items[t];
    for (int j = 0; j < it.n; ++j) {
      const int q = it.first + j;
      const long long n = (long long)it.before.pushed + j;   // the frame's number in its stream
      if (n == 0) { m.ring_prev[q] = -1; m.constant_bits |= 1ull << q; }
      else m.ring_prev[q] = (int)((n - 1) % R);
    }
  }
  return m;
}

// blur_ker(): g = exp(-(i - 1)^2 / (2 sigma^2)), sigma 0.5, normalised to sum 1 in double; tap [i][j] = (float)(g[i] g[j]), row-major
inline void motion_taps(float w[9]) {
  double g[3], sum = 0;
  for (int i = 0; i < 3; ++i) { g[i] = std::exp(-(double)((i - 1) * (i - 1)) / 0.5); sum += g[i]; }
  for (int i = 0; i < 3; ++i) g[i] /= sum;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) w[3 * i + j] = (float)(g[i] * g[j]);
}

// what a frame's map is multiplied with after the clamp
inline float motion_scale(double rate) { return (float)(0.35 * rate); }

constexpr int NOISE_MAP_CONSTANT = 0, NOISE_MAP_MOTION = 1;   // SS4K_NOISE_MAP_* of include/ss4k.h

}  // namespace temporal_round
}  // namespace ss4k
