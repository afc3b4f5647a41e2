// pt_mega_tex.hip -- image textures (ptc_set_textures, ptc_set_texcoords, ptc_set_param "textures"): the
// megakernel's four textured instances, k_megakernel_tex<kMis, kSmooth>, the lookup query's kernel, k_texture_sample, and the surface
// query's, k_hit_surface, with launch_mega_tex (the rule that names an instance: pt_mega_rules.hpp) and the queries' launchers -- in a
// translation unit of its own so that every other code object stays what it was.  The loop itself, with what kMegaTex adds to it, is
// mega_path (pt_megakernel.inc); the rule is pt_texture.hpp's; the closest hit that reports its winner is ray_scene<.., true>
// (pt_kernels_common.inc).  Part of libptcore.so.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_light_sample.hpp"
#include "pt_env_light.hpp"
#include "pt_smooth.hpp"
#include "pt_texture.hpp"
#include "pt_mega_rules.hpp"
#include <float.h>
#include <limits.h>

namespace pt {

#include "pt_kernels_common.inc"

#include "pt_megakernel.inc"

// k_megakernel_smooth's shape with kTex, with the balance heuristic and without, with the shading normal and without: emitters and
// roulette compiled in, pinhole or lens by lens.radius, the lamps' samples by lt.records, the environment's by el.table, the
// environment itself by env.texels -- four instances render everything the megakernel renders without textures
template <bool kMis, bool kSmooth>
__global__ __launch_bounds__(kWave) void k_megakernel_tex(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band, uint32_t pix_count,
                                                          int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats,
                                                          int roulette, DLens lens, DEnv env, DEnvLight el, DMis mis, DSmooth sm, DTex tx)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kMegaEnvLit | kMegaTex | (kMis ? kMegaMis : 0u) | (kSmooth ? kMegaSmooth : 0u)>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb,
                                                                                            counters, stats, roulette, s_stack + threadIdx.x, lens,
                                                                                            env, el, mis, sm, tx);
}

// ptc_sample_texture: one thread per coordinate pair, steps 2 .. 7 of the rule on one texture of the pool
__global__ __launch_bounds__(256) void k_texture_sample(DTex tx, uint32_t tex, const float* st, uint32_t n, float* rgb, uint8_t* rejected)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  f3 c;
  const bool ok = texmap::lookup(tx.texels, tx.records[tex], tx.table, st[2u * (size_t)i], st[2u * (size_t)i + 1u], c);
  rgb[3u * (size_t)i] = c.x;
  rgb[3u * (size_t)i + 1u] = c.y;
  rgb[3u * (size_t)i + 2u] = c.z;
  if (rejected) rejected[i] = ok ? (uint8_t)0 : (uint8_t)1;
}

// ptc_hit_surface: k_hit_attributes' walk (one thread per ray, the reference's order, the thread's column of the LDS stack); at the
// winner the interpolated s, t and the albedo mega_path<.., kTex> would hand to evaluate_material there.  A miss: zeros.
__global__ __launch_bounds__(kWave) void k_hit_surface(DScene sc, DTex tx, const float4* rays, uint32_t n, float2* st_out, float* albedo_out,
                                                       uint32_t* flags_out)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  const uint32_t r = blockIdx.x * kWave + threadIdx.x;
  if (r >= n) return;
  const float4 ro = rays[2u * (size_t)r], rd = rays[2u * (size_t)r + 1u];
  Ray ray;
  ray.o = xyz(ro);
  ray.tmin = ro.w;
  ray.d = xyz(rd);
  ray.tmax = rd.w;
  Hit rec;
  rec.t = 0.0f;
  rec.p = rec.n = mk3(0.f, 0.f, 0.f);
  rec.mat = 0u;
  rec.side = 0u;
  HitAttr at;
  Tally tally;
  uint32_t flags = 0u;
  float2 st = make_float2(0.0f, 0.0f);
  f3 alb = mk3(0.0f, 0.0f, 0.0f);
  if (ray_scene<false, true>(ray, sc, rec, s_stack + threadIdx.x, flags, tally, &at)) {
    const DMaterial& mat = sc.materials[rec.mat];
    alb = mk3(mat.p[0], mat.p[1], mat.p[2]);
    if (at.first != kNoChild && tx.st) {
      const uint32_t mesh = sc.object_mesh[at.object];
      const float* c = tx.st + 2u * ((size_t)tx.mesh_first_index[mesh] + at.first);
      st = make_float2(texmap::interpolate(c[0], c[2], c[4], at.u, at.v), texmap::interpolate(c[1], c[3], c[5], at.u, at.v));
      if (tx.texels && mat.type <= 1) {
        const int32_t ti = tx.material_texture[rec.mat];
        if (ti >= 0) (void)texmap::albedo(tx.texels, tx.records[ti], tx.table, c, c + 2, c + 4, at.u, at.v, alb, alb);
      }
    }
  }
  st_out[r] = st;
  albedo_out[3u * (size_t)r] = alb.x;
  albedo_out[3u * (size_t)r + 1u] = alb.y;
  albedo_out[3u * (size_t)r + 2u] = alb.z;
  if (flags) atomicOr(flags_out, flags);
}

void launch_mega_tex(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in)
{
  mega_go_lit(in.b ? (in.a ? k_megakernel_tex<true, true> : k_megakernel_tex<false, true>)
                   : (in.a ? k_megakernel_tex<true, false> : k_megakernel_tex<false, false>),
              s, f, f.lens, f.env, f.el, f.mis, f.sm, f.tx);
}

void launch_texture_sample(hipStream_t s, DTex tx, uint32_t tex, const float* st, uint32_t n, float* rgb, uint8_t* rejected)
{
  const dim3 grid((n + 255u) / 256u), block(256);
  hipLaunchKernelGGL(k_texture_sample, grid, block, 0, s, tx, tex, st, n, rgb, rejected);
}

void launch_hit_surface(hipStream_t s, const DScene& scene, DTex tx, const float4* rays, uint32_t n, float2* st_out, float* albedo_out,
                        uint32_t* flags)
{
  const dim3 grid((n + kWave - 1u) / kWave), block(kWave);
  hipLaunchKernelGGL(k_hit_surface, grid, block, 0, s, scene, tx, rays, n, st_out, albedo_out, flags);
}
}  // namespace pt
