// pt_env_light.hpp -- the environment as a light (ptc_environment_light, ptc_set_param "environment_light"): the
// alias table over the map's N x N texel squares, built on the host, and one environment sample for one surface point -- the function
// k_env_light_sample (pt_env.hip), the megakernel's environment-light instance (pt_mega_direct.hip) and the host hook
// (ptc_check_environment_light) all call.  The lookup a sample ends with is env_rules::lookup (pt_env.hpp), the function a miss calls.
//
// Every line of the sample's arithmetic is one IEEE binary32 operation of the order written down in DESIGN section 5k
// (-ffp-contract=off, correctly rounded divide and sqrt); tests/env_light_ref.py restates it in numpy, operation for operation.
#pragma once

#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_mis.hpp"

#include <float.h>
#include <cmath>
#include <vector>

namespace pt {
namespace env_light {

constexpr float kPi = 3.14159265358979323846264338327950288f;

// One entry of the alias table, 16 bytes, one per texel square k = j n + i (square (i, j): s_x in [i / n, (i + 1) / n], s_z in
// [j / n, (j + 1) / n] of the octahedral unit square).  A draw that lands on the entry keeps its square with probability q and takes
// `alias` otherwise; f_self and f_alias are 1 / (P n^2) of the two squares, so the draw needs no second load.  q == 1: alias is the
// entry itself (a uniform draw may be exactly 1.0f).  A square of weight 0: q 0, f_self 0, and nobody's alias.
struct Entry {
  float q;
  uint32_t alias;
  float f_self, f_alias;
};
static_assert(sizeof(Entry) == 16, "an alias entry is one 16-byte load");

struct Sample {
  f3 w;         // unit direction of the sample
  float tmax;   // FLT_MAX, or 0 for a culled sample (the empty interval [1e-4, 0])
  f3 contrib;   // unshadowed contribution
  bool sampled;
};

// The square and its factor from the raw draw v (Minstd::next, 1 .. 2^31 - 2) and u1: entry e = ((v - 1) n^2) >> 31 in integers, never
// out of range (a float's rounding of u n^2 would give the last entry 1.5 x its share at n = 4096).  table: the entries as four words.
PT_HD void pick(const uint4* table, const uint32_t n, const uint32_t v, const float u1, uint32_t& k, float& f)
{
  const uint32_t e = (uint32_t)(((uint64_t)(v - 1u) * (uint64_t)(n * n)) >> 31);
  const uint4 t = table[e];  // the one load of the draw
  const bool self = u1 < __builtin_bit_cast(float, t.x);
  k = self ? e : t.y;
  f = __builtin_bit_cast(float, self ? t.z : t.w);
}

// The direction of the point (sx, sz) of the octahedral unit square, normalised: the inverse of env_rules::locate -- the upper sheet
// where |q_x| + |q_z| <= 1, else the fold -- and its 1-norm cubed (the Jacobian: d omega = 4 |w|_1^3 ds_x ds_z).
PT_HD f3 decode(const float sx, const float sz, float& l3)
{
  const float tx = sx * 2.0f;
  const float qx = tx - 1.0f;
  const float tz = sz * 2.0f;
  const float qz = tz - 1.0f;
  const float ax = __builtin_fabsf(qx), az = __builtin_fabsf(qz);
  const float s1 = ax + az;
  const float y = 1.0f - s1;
  f3 d = mk3(qx, y, qz);
  if (!(s1 <= 1.0f)) {  // the lower hemisphere, unfolded
    d.x = (1.0f - az) * env_rules::sgn(qx);
    d.z = (1.0f - ax) * env_rules::sgn(qz);
  }
  const float d2 = dot(d, d);
  const float len = ieee_sqrt(d2);
  const float inv = 1.0f / len;
  const f3 w = d * inv;
  const float l1 = (__builtin_fabsf(w.x) + __builtin_fabsf(w.y)) + __builtin_fabsf(w.z);
  l3 = (l1 * l1) * l1;
  return w;
}

// What a sample's two solid-angle densities are made of (multiple importance sampling): jac = (4 f) l^3, the
// reciprocal of the sample's own density, and the cosine at the receiver, as the contribution takes them.
struct Terms {
  float jac, cos_r;
};

// One environment sample for the point with normal nrm from explicit draws: v raw, u1 .. u3 uniform.  E: the aproned map (pt_env.hpp).
// terms: the sample's Terms.
template <class Texel>
PT_HD Sample sample_draws(const uint4* table, const Texel* E, const uint32_t n, const f3 nrm, const uint32_t v, const float u1, const float u2,
                          const float u3, Terms& terms)
{
  uint32_t k;
  float f;
  pick(table, n, v, u1, k, f);
  const uint32_t j = k / n;
  const uint32_t i = k - j * n;
  const float fn = (float)n;
  const float cx = (float)i + u2;
  const float sx = cx / fn;
  const float cz = (float)j + u3;
  const float sz = cz / fn;
  float l3;
  const f3 w = decode(sx, sz, l3);
  float r, g, b;
  env_rules::lookup(E, n, w.x, w.y, w.z, r, g, b);  // (its four texel loads stand in front of the arithmetic that follows)
  const float cos_r = dot(nrm, w);
  const bool sampled = cos_r > 0.0f;
  const float ff = 4.0f * f;
  const float jac = ff * l3;
  const float cj = cos_r * jac;
  const float gk = cj / kPi;
  Sample out;
  out.w = w;
  out.tmax = sampled ? FLT_MAX : 0.0f;
  out.contrib = sampled ? mk3(r * gk, g * gk, b * gk) : mk3(0.0f, 0.0f, 0.0f);
  out.sampled = sampled;
  terms = Terms{jac, cos_r};
  return out;
}
// ... for the callers that take the sample alone
template <class Texel>
PT_HD Sample sample_draws(const uint4* table, const Texel* E, const uint32_t n, const f3 nrm, const uint32_t v, const float u1, const float u2,
                          const float u3)
{
  Terms terms;
  return sample_draws(table, E, n, nrm, v, u1, u2, u3, terms);
}

// ... from the point's stream: Minstd seeded path_seed(index, sample_index) ^ kEnvLightSeedXor, four draws after `discard` (0 for a
// query, 4 * bounce in the render loop: bounce b takes draws 4b .. 4b + 3)
template <class Texel>
PT_HD Sample sample_point(const uint4* table, const Texel* E, const uint32_t n, const f3 nrm, const uint32_t index, const uint32_t sample_index,
                          const uint32_t discard, Terms& terms)
{
  Minstd rng;
  rng.seed(path_seed(index, sample_index) ^ kEnvLightSeedXor);
  if (discard != 0u) rng.discard(discard);
  const uint32_t v = rng.next();
  const float u1 = rng.uniform();
  const float u2 = rng.uniform();
  const float u3 = rng.uniform();
  return sample_draws(table, E, n, nrm, v, u1, u2, u3, terms);
}
template <class Texel>
PT_HD Sample sample_point(const uint4* table, const Texel* E, const uint32_t n, const f3 nrm, const uint32_t index, const uint32_t sample_index,
                          const uint32_t discard)
{
  Terms terms;
  return sample_point(table, E, n, nrm, index, sample_index, discard, terms);
}

// ---- the sample's density (multiple importance sampling, ptc_set_param "mis") -------------------------------------

// The reciprocal of jac = (4 f) l^3, the environment's solid-angle density; f == 0 (a square of weight 0): 0
PT_HD float env_density(const float jac) { return jac > 0.0f ? 1.0f / jac : 0.0f; }

// The square k = j n + i the point (qx, qz) of the octahedral square (env_rules::project) falls in
PT_HD uint32_t square_of(const float qx, const float qz, const uint32_t n)
{
  const float fn = (float)n;
  const float mx = qx * 0.5f;
  const float sx = mx + 0.5f;
  const float fx = floorf(sx * fn);
  const float mz = qz * 0.5f;
  const float sz = mz + 0.5f;
  const float fz = floorf(sz * fn);
  const uint32_t i = fx >= fn ? n - 1u : (fx > 0.0f ? (uint32_t)fx : 0u);
  const uint32_t j = fz >= fn ? n - 1u : (fz > 0.0f ? (uint32_t)fz : 0u);
  return j * n + i;
}

// The environment sample's density in the unit direction w: one 16-byte load of the square's own entry, whose f_self is f of the
// square (build_table).  A direction env_rules::project refuses (zero, NaN, infinite) has density 0 and loads nothing.
PT_HD float density(const uint4* table, const uint32_t n, const f3 w)
{
  float qx, qz;
  if (!env_rules::project(w.x, w.y, w.z, qx, qz)) return 0.0f;
  const uint4 t = table[square_of(qx, qz, n)];
  const float f = __builtin_bit_cast(float, t.z);
  const float l1 = (__builtin_fabsf(w.x) + __builtin_fabsf(w.y)) + __builtin_fabsf(w.z);
  const float l3 = (l1 * l1) * l1;
  const float ff = 4.0f * f;
  const float jac = ff * l3;
  return env_density(jac);
}

// The table of the aproned map E (host, binary64 from the binary32 texels).  Per square the filtered colour -- the
// exact integral of the bilinear lookup over the square: the 3 x 3 neighbourhood of E[j + 1][i + 1] under the separable weights
// (1/8, 6/8, 1/8) --, lum = its largest channel, weight = lum x |w_c|_1^3 at the square's centre; W = their sum in table order; P = weight / W.
// Vose's method on p = P n^2: the squares with p < 1 and those with p >= 1 are put on two stacks in ascending table order; while both
// hold something the top small one s and the top large one l are taken, q_s = p_s, alias_s = l, p_l = (p_l + p_s) - 1, and l goes back
// on the stack its new p belongs to; what is left on either stack keeps itself (q 1).  So the table is a function of the map alone.
// -> W (0: a map without weight, `out` is empty: there is no table); *positive = squares of weight > 0.
template <class Texel>
inline double build_table(const Texel* E, const uint32_t n, std::vector<Entry>& out, uint64_t* positive)
{
  const size_t n2 = (size_t)n * n, row = (size_t)n + 2u;
  std::vector<double> p(n2);
  const double wt[3] = {0.125, 0.75, 0.125};
  double W = 0.0;
  uint64_t pos = 0u;
  for (uint32_t j = 0; j < n; ++j)
    for (uint32_t i = 0; i < n; ++i) {
      double c[3] = {0.0, 0.0, 0.0};
      for (int dj = 0; dj < 3; ++dj)
        for (int di = 0; di < 3; ++di) {
          const Texel& t = E[((size_t)j + (size_t)dj) * row + (size_t)i + (size_t)di];
          const double k = wt[dj] * wt[di];
          c[0] += k * (double)t.x;
          c[1] += k * (double)t.y;
          c[2] += k * (double)t.z;
        }
      const double lum = c[0] < c[1] ? (c[1] < c[2] ? c[2] : c[1]) : (c[0] < c[2] ? c[2] : c[0]);
      const double qx = 2.0 * (((double)i + 0.5) / (double)n) - 1.0, qz = 2.0 * (((double)j + 0.5) / (double)n) - 1.0;
      double x = qx, z = qz;
      const double y = 1.0 - std::fabs(qx) - std::fabs(qz);
      if (y < 0.0) {
        x = (1.0 - std::fabs(qz)) * (qx < 0.0 ? -1.0 : 1.0);
        z = (1.0 - std::fabs(qx)) * (qz < 0.0 ? -1.0 : 1.0);
      }
      const double len = std::sqrt(x * x + y * y + z * z);
      const double l1 = (std::fabs(x) + std::fabs(y) + std::fabs(z)) / len;
      const double w = lum * (l1 * l1 * l1);
      p[(size_t)j * n + i] = w;
      W += w;
      pos += w > 0.0 ? 1u : 0u;
    }
  if (positive) *positive = pos;
  out.clear();
  if (!(W > 0.0)) return 0.0;
  out.resize(n2);
  std::vector<float> f(n2);
  std::vector<uint32_t> small, large;
  uint32_t heaviest = 0u;
  for (size_t k = 0; k < n2; ++k) {
    if (p[k] > p[heaviest]) heaviest = (uint32_t)k;
    const double pk = p[k] / W;
    f[k] = pk > 0.0 ? (float)(1.0 / (pk * (double)n2)) : 0.0f;
    p[k] = pk * (double)n2;
    (p[k] < 1.0 ? small : large).push_back((uint32_t)k);
  }
  const auto keep_self = [&](uint32_t k) { out[k] = Entry{1.0f, k, f[k], f[k]}; };
  while (!small.empty() && !large.empty()) {
    const uint32_t s = small.back(), l = large.back();
    small.pop_back();
    large.pop_back();
    const float q = (float)p[s];
    if (q >= 1.0f) keep_self(s);  // p_s rounds to 1: the entry never leaves its square
    else out[s] = Entry{q, l, f[s], f[l]};
    p[l] = (p[l] + p[s]) - 1.0;
    (p[l] < 1.0 ? small : large).push_back(l);
  }
  for (const uint32_t k : large) keep_self(k);
  // (small squares are left over only by the rounding of the sums, with p a few ulps under 1; one of weight 0 among them -- never seen
  // -- hands its draws to the heaviest square, which nothing of weight 0 can be)
  for (const uint32_t k : small)
    if (f[k] > 0.0f) keep_self(k);
    else out[k] = Entry{0.0f, heaviest, 0.0f, f[heaviest]};
  return W;
}

}  // namespace env_light
}  // namespace pt
