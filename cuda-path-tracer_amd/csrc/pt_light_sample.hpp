// pt_light_sample.hpp -- one light sample for one surface point: the function k_light_sample (pt_light.hip) and
// k_megakernel_direct (pt_mega_direct.hip) both call, and k_megakernel_mis (pt_mega_mis.hip, section 5l) with the sample's terms.  Host-callable, so that the arithmetic can be run on a CPU
// as well (ptc_check_light_sample, ptcore_checks.cpp: light_pick and light_sample_draws on the caller's draws).
//
// Every line of the arithmetic is one IEEE binary32 operation of the order written down in DESIGN section 5f (-ffp-contract=off,
// correctly rounded divide and sqrt); tests/direct_ref.py restates it in numpy, operation for operation.
#pragma once

#include "pt_device.hpp"
#include "pt_rng.hpp"

namespace pt {

constexpr float kPi = 3.14159265358979323846264338327950288f;
constexpr float kTwoPi = 2.0f * kPi;

struct LightSample {
  f3 w;           // direction towards the sampled point (zero when there is none)
  float tmax;     // d * 0.999f, or 0 for a culled sample
  f3 contrib;     // unshadowed contribution
  bool sampled;
};
// What a sample's two solid-angle densities are made of (multiple importance sampling): the squared distance, the
// cosine at the lamp, the record's inv_pdf and the cosine at the receiver, as the contribution's g takes them.
struct LightTerms {
  float d2, cos_l, inv_pdf, cos_r;
};
// The lamp of the raw first draw v (Minstd::next, 1 .. 2^31 - 2): k = min(#{j : T_j <= v - 1}, last) over the table's integer thresholds
// (build_light_table), 4 bytes a step (count and last are kernel arguments: wave-uniform).  Exact: lamp k owns T_k - T_(k-1) of the
// generator's 2^31 - 2 states (a binary32 cdf has a step of 2^-24 near 1, and the lamps below it were never picked).
PT_HD uint32_t light_pick(const DLights& lt, const uint32_t v)
{
  const uint32_t n = v - 1u;
  uint32_t lo = 0u, hi = lt.count;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (lt.thresholds[mid] <= n) lo = mid + 1u;
    else hi = mid;
  }
  return lo < lt.last ? lo : lt.last;
}
// One light sample for the point p with normal nrm from explicit draws: raw = a Minstd::next (it picks the lamp), u1, u2 uniform (the point on it).
// terms: the sample's LightTerms (meaningful where the sample is `sampled`)
PT_HD LightSample light_sample_draws(const DLights& lt, const f3 p, const f3 nrm, const uint32_t raw, const float u1, const float u2,
                                     LightTerms& terms)
{
  const uint32_t k = light_pick(lt, raw);
  const float4* rec = lt.records + 4u * (size_t)k;
  const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
  const f3 p0 = mk3(r0.x, r0.y, r0.z);
  const float inv_pdf = r3.y;
  const uint32_t object = __builtin_bit_cast(uint32_t, r3.z), kind_material = __builtin_bit_cast(uint32_t, r3.w);
  f3 q, nl;
  if (kind_material >> 31) {
    const DObject* obj = lt.objects + object;
    const float4 sph = lt.spheres[obj->index];
    const float z = 1.0f - 2.0f * u1;
    const float r = ieee_sqrt(sel_max(0.0f, 1.0f - z * z));
    const float phi = kTwoPi * u2;
    float s, c;
    det_sincos(phi, s, c);
    const f3 dir = mk3(r * c, r * s, z);
    const f3 qo = mk3(sph.x, sph.y, sph.z) + dir * sph.w;
    q = xform_point(obj->m, qo);
    nl = normalize(q - p0);
  } else {
    const f3 e1 = mk3(r0.w, r1.x, r1.y), e2 = mk3(r1.z, r1.w, r2.x);
    const float su = ieee_sqrt(u1);
    const float b1 = 1.0f - su;
    const float b2 = u2 * su;
    q = (p0 + e1 * b1) + e2 * b2;
    nl = mk3(r2.y, r2.z, r2.w);
  }
  const f3 v = q - p;
  const float d2 = dot(v, v);
  const bool valid = d2 > 0.0f && d2 < __builtin_inff();
  const float d = ieee_sqrt(d2);
  const float inv_d = 1.0f / d;
  const f3 w = v * inv_d;
  const float cos_r = dot(nrm, w);
  const float cos_l = __builtin_fabsf(dot(nl, w));
  const bool sampled = valid && cos_r > 0.0f && inv_pdf > 0.0f;
  const float g = ((cos_r * cos_l) * inv_pdf) / (kPi * d2);
  const DMaterial* mat = lt.materials + (kind_material & 0x7fffffffu);
  const f3 le = mk3(mat->p[0], mat->p[1], mat->p[2]);
  LightSample out;
  // a culled sample keeps a direction the walk can set up with (a zero one would send the ray to the launch's exact redo) and gets
  // the empty interval [1e-4, 0]
  out.w = valid ? w : mk3(0.0f, 0.0f, 0.0f);
  out.tmax = sampled ? d * 0.999f : 0.0f;
  out.contrib = sampled ? le * g : mk3(0.0f, 0.0f, 0.0f);
  out.sampled = sampled;
  terms = LightTerms{d2, cos_l, inv_pdf, cos_r};
  return out;
}
// ... with the draws of the point's light stream.  discard: draws to skip first -- 0 for a query (k_light_sample), 3 * bounce in the
// render loop, whose bounce b so takes draws 3b .. 3b + 2 of the stream (discard(0) leaves a generator as it is, so it is not executed)
PT_HD LightSample light_sample_point(const DLights& lt, const f3 p, const f3 nrm, uint32_t i, uint32_t sample_index, uint32_t discard,
                                     LightTerms& terms)
{
  Minstd rng;
  rng.seed(path_seed(i, sample_index) ^ kLightSeedXor);
  if (discard != 0u) rng.discard(discard);
  const uint32_t v = rng.next();
  const float u1 = rng.uniform();
  const float u2 = rng.uniform();
  return light_sample_draws(lt, p, nrm, v, u1, u2, terms);
}
// ... for the callers that take the sample alone
PT_HD LightSample light_sample_point(const DLights& lt, const f3 p, const f3 nrm, uint32_t i, uint32_t sample_index, uint32_t discard)
{
  LightTerms terms;
  return light_sample_point(lt, p, nrm, i, sample_index, discard, terms);
}

}  // namespace pt
