// pt_mis.hpp -- multiple importance sampling in the megakernel (ptc_set_param "mis"): the balance heuristic's weight
// and the two densities that are no light sampler's own -- the cosine lobe's and a lamp point's as seen from the surface.  The
// environment's density: env_light::density (pt_env_light.hpp).  Host-callable; every line is one IEEE binary32 operation of the order
// written down in section 5l (-ffp-contract=off, correctly rounded divide); tests/mis_ref.py restates it in numpy.
#pragma once

#include "pt_math.hpp"

#include <float.h>

namespace pt {
namespace mis {

constexpr float kPi = 3.14159265358979323846264338327950288f;

// The weight of the strategy whose density is a against the one whose density is b: a / (a + b).  A sum that is not > 0 (both
// densities 0) and a density past FLT_MAX leave the weight 1: neither is a number the rule could divide by.
PT_HD float balance(const float a, const float b)
{
  const float s = a + b;
  const float w = a / s;
  return s > 0.0f && a <= FLT_MAX ? w : 1.0f;
}

// The solid-angle density of a lamp's point at squared distance d2 whose cosine is cos_l, from the lamp's area density 1 / inv_pdf:
// d2 / (cos_l inv_pdf); a product that is not > 0 (a grazing lamp, a lamp of luminance 0, a material that is no lamp) gives 0.
PT_HD float lamp_density(const float d2, const float cos_l, const float inv_pdf)
{
  const float den = cos_l * inv_pdf;
  const float p = d2 / den;
  return den > 0.0f ? p : 0.0f;
}

// The cosine lobe's density of a direction whose cosine with the normal is c: c / pi, 0 where c <= 0
PT_HD float lobe_density(const float c)
{
  const float p = c / kPi;
  return c > 0.0f ? p : 0.0f;
}

}  // namespace mis
}  // namespace pt
