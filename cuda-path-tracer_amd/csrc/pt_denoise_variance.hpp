// pt_denoise_variance.hpp -- the variance-guided A-Trous rule (ptc_set_param "denoise_variance", ptc_denoise_variance; DESIGN section
// 5s): a per-pixel spatial variance of the plane the passes filter, the colour weight it steers, and the variance that travels beside
// the colour through the passes.  Host-callable: k_variance_estimate, k_variance_prefilter, k_denoise_var and k_denoise_var_lds
// (pt_denoise_variance.hip) and the host's check (ptc_check_denoise_variance) call these per-tap functions;
// tests/denoise_variance_ref.py restates the rule in numpy.  The stage is compared under a tolerance, not bit for bit (as the plain
// passes are, pt_post.hip), so contraction into FMAs is allowed inside these bodies.
//
// Two sums are taken about the centre pixel, not about zero -- m = c_p + sum g (c_q - c_p) / sum g, c' = c_p + sum w (c_q - c_p) / sum w:
// the same numbers as sum g c / sum g and sum w c / sum w, but a window or a tap set of equal colours gives back c_p bit for bit
// (every difference is an exact zero), which the rounded quotient of two rounded sums does not.
#pragma once

#include "pt_math.hpp"
#include <math.h>

namespace pt {
namespace dvar {

// What is added to sigma x the prefiltered variance under the colour distance, a design constant: 2^-53.  One binary32 rounding of a
// colour of order 1 has variance ulp^2 / 12 = 2^-46 / 12 = 1.2e-15 a channel, 3.6e-15 a pixel; the floor sits a factor of 30 below
// that, so it never overrides a real estimate, and its reciprocal (9.0e15) is finite: where the variance is zero, a colour
// distance of zero gives 0 x 9.0e15 = 0 (the taps average) and any distance above 1e-7 gives a weight of exp(-90) or less.
constexpr float kVarianceFloor = 0x1p-53f;
constexpr int kVarRadius = 3;  // the estimate's window: 7 x 7 at one-pixel spacing
constexpr float kLog2e = 1.4426950408889634f;

// 2^a: v_exp_f32 on the device, exp2f on the host
PT_HD float exp2_of(const float a)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(a);
#else
  return exp2f(a);
#endif
}

// exp(-d / phi) = 2^(d x scale): the scale of one edge-stopping term, once per pixel or pass (a zero phi: -inf, and 0 x -inf = NaN at
// the centre tap, as in the plain passes)
PT_HD float term_scale(const float phi) { return -kLog2e / phi; }

PT_HD float dist2(const f3 a, const f3 b)
{
#pragma clang fp contract(fast)
  const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
  return x * x + y * y + z * z;
}

// ---- the estimate (k_variance_estimate) ----
// g_q of a window tap: normal and position only (kn, kp: term_scale of n_phi and p_phi; the window is at step 1)
PT_HD float estimate_weight(const f3 np, const f3 nq, const f3 xp, const f3 xq, const float kn, const float kp)
{
#pragma clang fp contract(fast)
  return exp2_of(dist2(np, nq) * kn + dist2(xp, xq) * kp);
}

struct MeanSum {
  f3 d;     // sum g (c_q - c_p)
  float g;  // sum g
};
// sweep 1
PT_HD void mean_tap(MeanSum& s, const float g, const f3 cp, const f3 cq)
{
#pragma clang fp contract(fast)
  s.d.x += g * (cq.x - cp.x);
  s.d.y += g * (cq.y - cp.y);
  s.d.z += g * (cq.z - cp.z);
  s.g += g;
}
PT_HD f3 mean_of(const MeanSum& s, const f3 cp)
{
#pragma clang fp contract(fast)
  const float inv = 1.0f / s.g;
  return mk3(cp.x + s.d.x * inv, cp.y + s.d.y * inv, cp.z + s.d.z * inv);
}
// sweep 2: acc += g |c_q - m|^2, and v = acc / sum g
PT_HD void variance_tap(float& acc, const float g, const f3 cq, const f3 m)
{
#pragma clang fp contract(fast)
  acc += g * dist2(cq, m);
}
PT_HD float variance_of(const float acc, const float g_sum) { return acc / g_sum; }

// ---- the prefilter: (1 2 1; 2 4 2; 1 2 1) / 16 of the variance plane around the centre, v[3 (dy + 1) + dx + 1] ----
PT_HD float prefilter(const float v[9])
{
#pragma clang fp contract(fast)
  const float corners = (v[0] + v[2]) + (v[6] + v[8]), edges = (v[1] + v[7]) + (v[3] + v[5]);
  return corners * 0.0625f + edges * 0.125f + v[4] * 0.25f;
}
PT_HD bool floored(const float prefiltered) { return prefiltered < kVarianceFloor; }

// ---- a pass ----
// the colour term's scale of a pixel, once per pixel: exp(-d / (sigma v + floor)) = 2^(d x colour_scale)
PT_HD float colour_scale(const float sigma, const float prefiltered)
{
#pragma clang fp contract(fast)
  return -kLog2e / (sigma * prefiltered + kVarianceFloor);
}
// the edge-stopping weight of a tap (kn: term_scale(step^2 n_phi), as the plain passes divide the normal distance by step^2)
PT_HD float pass_weight(const float dc, const float dn, const float dp, const float kc, const float kn, const float kp)
{
#pragma clang fp contract(fast)
  return exp2_of(dc * kc + dn * kn + dp * kp);
}
struct PassSum {
  f3 d;     // sum w (c_q - c_p)
  float w;  // sum w
  float v;  // sum w^2 v_q
};
// wk: the edge-stopping weight x the tap's kernel weight; diff = c_p - c_q (what the weight was made from)
PT_HD void pass_tap(PassSum& s, const float wk, const f3 diff, const float vq)
{
#pragma clang fp contract(fast)
  s.d.x -= diff.x * wk;
  s.d.y -= diff.y * wk;
  s.d.z -= diff.z * wk;
  s.w += wk;
  s.v += (wk * wk) * vq;
}
PT_HD void pass_result(const PassSum& s, const f3 cp, f3& c_out, float& v_out)
{
#pragma clang fp contract(fast)
  const float inv = 1.0f / s.w;
  c_out = mk3(cp.x + s.d.x * inv, cp.y + s.d.y * inv, cp.z + s.d.z * inv);
  v_out = s.v * (inv * inv);
}

// the kernel weight {3/8, 1/4, 1/16}[min(|dx|, |dy|)] of the 5 x 5 taps
PT_HD float kernel_weight(const int dx, const int dy)
{
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, k = ax < ay ? ax : ay;
  return k == 0 ? 0.375f : (k == 1 ? 0.25f : 0.0625f);
}

}  // namespace dvar
}  // namespace pt
