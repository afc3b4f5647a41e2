// pt_light.hip -- direct-light queries: k_light_sample picks a lamp and a point on it for every surface point
// and writes the shadow ray and the unshadowed contribution; the occlusion launches (pt_occlude.hip, or the exact closest-hit
// kernel under trace variant 0 / 1) decide the rays; k_light_resolve combines the two.  The lamp table (ptc_light, include/ptcore.h)
// is built on the host (ptcore_scene.cpp).  One thread per point, no LDS, no cross-lane work.  Part of libptcore.so.
//
// Every line of k_light_sample's arithmetic is one IEEE binary32 operation of the order written down in DESIGN section 5f
// (-ffp-contract=off, correctly rounded divide and sqrt); tests/direct_ref.py restates it in numpy, operation for operation.
#include "pt_device.hpp"
#include "pt_rng.hpp"

namespace pt {

constexpr float kPi = 3.14159265358979323846264338327950288f;
constexpr float kTwoPi = 2.0f * kPi;

// One light sample: what k_light_sample computes for point i (host-callable, so that the arithmetic can be run on a CPU as well).
struct LightSample {
  f3 w;           // direction towards the sampled point (zero when there is none)
  float tmax;     // d * 0.999f, or 0 for a culled sample
  f3 contrib;     // unshadowed contribution
  bool sampled;
};
PT_HD LightSample light_sample_point(const DLights& lt, const f3 p, const f3 nrm, uint32_t i, uint32_t sample_index)
{
  Minstd rng;
  rng.seed(path_seed(i, sample_index) ^ kLightSeedXor);
  const float u0 = rng.uniform();
  const float u1 = rng.uniform();
  const float u2 = rng.uniform();
  // k = min(#{j : cdf_j <= u0}, last): the dense cdf array, 4 bytes a step (count and last are kernel arguments: wave-uniform)
  uint32_t lo = 0u, hi = lt.count;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (lt.cdf[mid] <= u0) lo = mid + 1u;
    else hi = mid;
  }
  const uint32_t k = lo < lt.last ? lo : lt.last;
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
  return out;
}

__global__ __launch_bounds__(256) void k_light_sample(DLights lt, const float* __restrict__ points, const float* __restrict__ normals, uint32_t n,
                                                      uint32_t sample_index, uint32_t tmin_word, float4* __restrict__ o4, float4* __restrict__ d4,
                                                      float4* __restrict__ contrib)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const f3 p = mk3(points[3u * (size_t)i], points[3u * (size_t)i + 1u], points[3u * (size_t)i + 2u]);
  const f3 nrm = mk3(normals[3u * (size_t)i], normals[3u * (size_t)i + 1u], normals[3u * (size_t)i + 2u]);
  const LightSample s = light_sample_point(lt, p, nrm, i, sample_index);
  o4[i] = make_float4(p.x, p.y, p.z, __uint_as_float(tmin_word));
  d4[i] = make_float4(s.w.x, s.w.y, s.w.z, s.tmax);
  contrib[i] = make_float4(s.contrib.x, s.contrib.y, s.contrib.z, s.sampled ? 1.0f : 0.0f);
}

__global__ __launch_bounds__(256) void k_light_resolve(const float4* __restrict__ o4, const float4* __restrict__ d4, const float4* __restrict__ contrib,
                                                       const uint8_t* __restrict__ occluded, const float4* __restrict__ closest_tp, uint32_t n,
                                                       float* __restrict__ radiance, float* __restrict__ rays, uint8_t* __restrict__ visible,
                                                       uint32_t* __restrict__ stats)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 c = contrib[i];
  const bool sampled = c.w != 0.0f;
  const bool hit = occluded ? occluded[i] != 0u : closest_tp[i].x >= 0.0f;
  const bool vis = sampled && !hit;
  radiance[3u * (size_t)i] = vis ? c.x : 0.0f;
  radiance[3u * (size_t)i + 1u] = vis ? c.y : 0.0f;
  radiance[3u * (size_t)i + 2u] = vis ? c.z : 0.0f;
  if (visible) visible[i] = vis ? (uint8_t)1 : (uint8_t)0;
  if (rays) {
    const float4 o = o4[i], d = d4[i];
    float4* out = reinterpret_cast<float4*>(rays) + 2u * (size_t)i;
    out[0] = make_float4(o.x, o.y, o.z, 1e-4f);
    out[1] = sampled ? d : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  // (one add per wavefront after the compiler's reduction; spread over lines: adds to one line serialise in L2)
  uint32_t* line = stats + 32u * (blockIdx.x % kLightStatLines);
  if (sampled) atomicAdd(&line[0], 1u);
  if (vis) atomicAdd(&line[1], 1u);
}

void launch_light_sample(hipStream_t s, const DLights& lights, const float* points, const float* normals, uint32_t n, uint32_t sample_index,
                         uint32_t tmin_word, float4* o4, float4* d4, float4* contrib)
{
  hipLaunchKernelGGL(k_light_sample, dim3((n + 255u) / 256u), dim3(256), 0, s, lights, points, normals, n, sample_index, tmin_word, o4, d4, contrib);
}
void launch_light_resolve(hipStream_t s, const float4* o4, const float4* d4, const float4* contrib, const uint8_t* occluded,
                          const float4* closest_tp, uint32_t n, float* radiance, float* rays, uint8_t* visible, uint32_t* stats)
{
  hipLaunchKernelGGL(k_light_resolve, dim3((n + 255u) / 256u), dim3(256), 0, s, o4, d4, contrib, occluded, closest_tp, n, radiance, rays, visible,
                     stats);
}
}  // namespace pt
