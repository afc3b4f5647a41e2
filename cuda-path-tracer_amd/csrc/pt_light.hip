// pt_light.hip -- direct-light queries: k_light_sample picks a lamp and a point on it for every surface point
// and writes the shadow ray and the unshadowed contribution; the occlusion launches (pt_occlude.hip, or the exact closest-hit
// kernel under trace variant 0 / 1) decide the rays; k_light_resolve combines the two.  The lamp table (ptc_light, include/ptcore.h)
// is built on the host (ptcore_scene.cpp).  One thread per point, no LDS, no cross-lane work.  Part of libptcore.so.
//
// Every line of k_light_sample's arithmetic is one IEEE binary32 operation of the order written down in DESIGN section 5f
// (-ffp-contract=off, correctly rounded divide and sqrt); tests/direct_ref.py restates it in numpy, operation for operation.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_light_sample.hpp"  // light_sample_point: one sample for one point, shared with the render loop (pt_mega_direct.hip)

namespace pt {

__global__ __launch_bounds__(256) void k_light_sample(DLights lt, const float* __restrict__ points, const float* __restrict__ normals, uint32_t n,
                                                      uint32_t sample_index, uint32_t tmin_word, float4* __restrict__ o4, float4* __restrict__ d4,
                                                      float4* __restrict__ contrib)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const f3 p = mk3(points[3u * (size_t)i], points[3u * (size_t)i + 1u], points[3u * (size_t)i + 2u]);
  const f3 nrm = mk3(normals[3u * (size_t)i], normals[3u * (size_t)i + 1u], normals[3u * (size_t)i + 2u]);
  const LightSample s = light_sample_point(lt, p, nrm, i, sample_index, 0u);
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
