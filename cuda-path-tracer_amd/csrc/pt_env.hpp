// pt_env.hpp -- environment lighting (ptc_set_environment, an extension: the reference's sky is a fixed gradient):
// the lookup of an octahedral HDR map, stated once for the device (the five places a path meets the sky) and the host
// (ptc_check_environment, tests/env_ref.py restates it in numpy), and the apron the host adds at upload.
//
// The map: N x N RGB texels M[j][i], 2 <= N <= 4096, row j along z, column i along x, +y up.  The device holds E, (N + 2) x (N + 2)
// texels of four floats (w = 0): M with a one-texel apron that continues it across the octahedral fold -- the edge u = 0 identifies v
// with 1 - v, the four corners are the -y pole -- so a clamped bilinear fetch on E is continuous over the whole sphere.
// Every line of the lookup is one binary32 operation (-ffp-contract=off): abs, add, multiply, IEEE divide, floor.
#pragma once
#include <stdint.h>
#include <float.h>
#include <math.h>

#ifndef PT_ENV_HD
#if defined(__HIPCC__)
#define PT_ENV_HD __host__ __device__ __forceinline__
#else
#define PT_ENV_HD inline
#endif
#endif

namespace pt {
namespace env_rules {

constexpr uint32_t kMinSize = 2u, kMaxSize = 4096u;

// One axis of the fetch: q in [-1, 1] -> the lower texel of E along that axis (0 .. n) and the weight of the upper one.
PT_ENV_HD void axis(const float q, const uint32_t n, uint32_t& i0, float& t)
{
  const float m = q * 0.5f;
  const float s = m + 0.5f;
  const float f = s * (float)n;
  const float x = f + 0.5f;
  int i = (int)floorf(x);
  i = i < 0 ? 0 : i;
  i = i > (int)n ? (int)n : i;
  i0 = (uint32_t)i;
  t = x - (float)i;
}

PT_ENV_HD float sgn(const float t) { return t < 0.0f ? -1.0f : 1.0f; }  // (-0: +1)

// glm::lerp's form, as background()'s
PT_ENV_HD float mix(const float x, const float y, const float a) { return x * (1.0f - a) + y * a; }

// Where the direction (dx, dy, dz), not normalised, falls on E.  False: the value is (0, 0, 0) and nothing is to be loaded -- a zero
// direction, a NaN, an infinity, a sum that overflows.
// (project: its point (qx, qz) of the octahedral square [-1, 1]^2, which the environment light's density reads as well, pt_env_light.hpp)
PT_ENV_HD bool project(const float dx, const float dy, const float dz, float& qx, float& qz)
{
  const float a = (fabsf(dx) + fabsf(dy)) + fabsf(dz);
  if (!(a > 0.0f) || !(a <= FLT_MAX)) return false;
  const float px = dx / a;
  const float pz = dz / a;
  qx = px, qz = pz;
  if (dy < 0.0f) {  // the lower hemisphere folds outwards (dy = -0: the upper rule)
    qx = (1.0f - fabsf(pz)) * sgn(px);
    qz = (1.0f - fabsf(px)) * sgn(pz);
  }
  return true;
}

PT_ENV_HD bool locate(const float dx, const float dy, const float dz, const uint32_t n, uint32_t& i0, uint32_t& j0, float& tx, float& tz)
{
  float qx, qz;
  if (!project(dx, dy, dz, qx, qz)) return false;
  axis(qx, n, i0, tx);
  axis(qz, n, j0, tz);
  return true;
}

// The value of the environment E (n + 2 texels a row; Texel: four floats x, y, z, w) in the direction (dx, dy, dz).  The four texels
// are loaded together, in front of their first use; nothing is written.
template <class Texel>
PT_ENV_HD void lookup(const Texel* E, const uint32_t n, const float dx, const float dy, const float dz, float& r, float& g, float& b)
{
  uint32_t i0, j0;
  float tx, tz;
  r = g = b = 0.0f;
  if (!locate(dx, dy, dz, n, i0, j0, tx, tz)) return;
  const uint32_t row = n + 2u;
  const Texel* at = E + (size_t)j0 * row + i0;
  const Texel c00 = at[0];
  const Texel c10 = at[1];
  const Texel c01 = at[row];
  const Texel c11 = at[row + 1u];
  r = mix(mix(c00.x, c10.x, tx), mix(c01.x, c11.x, tx), tz);
  g = mix(mix(c00.y, c10.y, tx), mix(c01.y, c11.y, tx), tz);
  b = mix(mix(c00.z, c10.z, tx), mix(c01.z, c11.z, tx), tz);
}

// The apron (host): E[J][I] for I, J in 0 .. n + 1 from M (3 n n floats, row-major).  With i = I - 1, j = J - 1, c = clamp to 0 .. n - 1:
//   both in range M[j][i];  only i out M[n-1-j][c(i)];  only j out M[c(j)][n-1-i];  both out M[n-1-c(j)][n-1-c(i)]
template <class Texel>
inline void apron(const float* rgb, const uint32_t n, Texel* E)
{
  const int N = (int)n;
  const auto c = [N](int t) { return t < 0 ? 0 : (t > N - 1 ? N - 1 : t); };
  for (int J = 0; J < N + 2; ++J)
    for (int I = 0; I < N + 2; ++I) {
      const int i = I - 1, j = J - 1;
      const bool i_out = i < 0 || i >= N, j_out = j < 0 || j >= N;
      int sj = j, si = i;
      if (i_out && j_out) {
        sj = N - 1 - c(j);
        si = N - 1 - c(i);
      } else if (i_out) {
        sj = N - 1 - j;
        si = c(i);
      } else if (j_out) {
        sj = c(j);
        si = N - 1 - i;
      }
      const float* m = rgb + 3u * ((size_t)sj * n + (size_t)si);
      Texel& e = E[(size_t)J * (n + 2u) + (size_t)I];
      e.x = m[0];
      e.y = m[1];
      e.z = m[2];
      e.w = 0.0f;
    }
}

}  // namespace env_rules
}  // namespace pt
