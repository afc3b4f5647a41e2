// pt_denoise_albedo.hip -- the denoiser's albedo factorisation (ptc_set_param "denoise_albedo", ptc_denoise_albedo; DESIGN section
// 5r): k_denoise_albedo, the first-hit albedo plane and the irradiance the A-Trous passes filter in the colour's place, and
// k_remodulate, the colour their result gives back -- in a translation unit of its own so that every other code object stays what it
// was.  The rule is pt_demodulate.hpp's; the albedo is k_hit_surface's (pt_mega_tex.hip: the closest hit that reports its winner,
// ray_scene<.., true>, and pt_texture.hpp's lookup); the ray is k_denoise_positions' (pt_post.hip).  Part of libptcore.so.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_texture.hpp"
#include "pt_demodulate.hpp"
#include <float.h>

namespace pt {

#include "pt_kernels_common.inc"

// One wavefront per 8 x 8 pixel tile (neighbouring pixels walk the same subtree and fetch the same texels; a 64 x 1 strip of a
// 1080p frame spans 3 % of its width), one thread per pixel, the thread's column of the LDS stack.  The pixel-centre view ray --
// generate_ray(cam, x + 0.5, y + 0.5), a primary ray's t_min, no t_max; a pinhole ray under a lens too -- walks to its closest hit as
// k_hit_surface's does.  albedo: at a diffuse or metal hit (type <= 1) what k_hit_surface reports there under tx -- texel x p[0..2]
// where the texture rule applies, else p[0..2]; at glass, an emitter and on a miss (1, 1, 1): that colour carries no albedo factor.
// irradiance: demod::demodulate of the pixel's colour by the effective albedo, per channel.  rays (may be null): the ray, 8 floats
// a pixel.  stats: kLightStatLines lines of kLoopStatWords words, one add per wavefront and word -- 0 pixels, 1 surface hits
// (type <= 1), 2 texel lookups, 3 channels whose albedo took the floor.
__global__ __launch_bounds__(kWave) void k_denoise_albedo(DScene sc, DTex tx, DCamera cam, const float4* color, float4* albedo,
                                                          float4* irradiance, float4* rays, unsigned long long* stats, uint32_t* flags_out)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  const uint32_t tiles_x = (cam.width + 7u) / 8u;
  const uint32_t x = (blockIdx.x % tiles_x) * 8u + (threadIdx.x & 7u), y = (blockIdx.x / tiles_x) * 8u + (threadIdx.x >> 3);
  const bool inside = x < cam.width && y < cam.height;  // (a frame whose sides are no multiple of 8: the last column and row of tiles)
  uint32_t n_surface = 0u, n_lookup = 0u, n_floor = 0u, flags = 0u;
  if (inside) {
    const uint32_t index = x + y * cam.width;
    const float4 c = color[index];  // (ahead of the walk: one load, in flight while the ray is made)
    Ray ray;
    generate_ray(cam, (float)x + 0.5f, (float)y + 0.5f, ray.o, ray.d);
    ray.tmin = 1e-4f;
    ray.tmax = __builtin_inff();
    if (rays) {
      rays[2u * (size_t)index] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.tmin);
      rays[2u * (size_t)index + 1u] = make_float4(ray.d.x, ray.d.y, ray.d.z, ray.tmax);
    }
    Hit rec;
    rec.t = 0.0f;
    rec.p = rec.n = mk3(0.f, 0.f, 0.f);
    rec.mat = 0u;
    rec.side = 0u;
    HitAttr at;
    Tally tally;
    f3 alb = mk3(1.0f, 1.0f, 1.0f);
    if (ray_scene<false, true>(ray, sc, rec, s_stack + threadIdx.x, flags, tally, &at)) {
      const DMaterial& mat = sc.materials[rec.mat];
      if (mat.type <= 1) {
        n_surface = 1u;
        alb = mk3(mat.p[0], mat.p[1], mat.p[2]);
        if (at.first != kNoChild && tx.st && tx.texels) {
          const int32_t ti = tx.material_texture[rec.mat];
          if (ti >= 0) {
            const uint32_t mesh = sc.object_mesh[at.object];
            const float* st = tx.st + 2u * ((size_t)tx.mesh_first_index[mesh] + at.first);
            if (texmap::albedo(tx.texels, tx.records[ti], tx.table, st, st + 2, st + 4, at.u, at.v, alb, alb)) n_lookup = 1u;
          }
        }
      }
    }
    const f3 e = mk3(demod::effective_albedo(alb.x), demod::effective_albedo(alb.y), demod::effective_albedo(alb.z));
    n_floor = (demod::floored(alb.x) ? 1u : 0u) + (demod::floored(alb.y) ? 1u : 0u) + (demod::floored(alb.z) ? 1u : 0u);
    albedo[index] = make_float4(alb.x, alb.y, alb.z, 0.0f);
    irradiance[index] = make_float4(demod::demodulate(c.x, e.x), demod::demodulate(c.y, e.y), demod::demodulate(c.z, e.z), 0.0f);
  }
  // every lane of the wavefront is here again: one add per word
  const uint32_t s_pixels = wave_sum(inside ? 1u : 0u), s_surface = wave_sum(n_surface), s_lookup = wave_sum(n_lookup), s_floor = wave_sum(n_floor);
  if (threadIdx.x == 0u) {
    unsigned long long* line = stats + kLoopStatWords * (blockIdx.x % kLightStatLines);
    atomicAdd(&line[0], (unsigned long long)s_pixels);
    if (s_surface) atomicAdd(&line[1], (unsigned long long)s_surface);
    if (s_lookup) atomicAdd(&line[2], (unsigned long long)s_lookup);
    if (s_floor) atomicAdd(&line[3], (unsigned long long)s_floor);
  }
  if (flags) atomicOr(flags_out, flags);
}

// The passes' result back to a colour, in place: per channel demod::remodulate by the effective albedo of the plane k_denoise_albedo left
__global__ __launch_bounds__(256) void k_remodulate(uint32_t pix_count, const float4* albedo, float4* front)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= pix_count) return;
  const float4 a = albedo[i], f = front[i];
  front[i] = make_float4(demod::remodulate(f.x, demod::effective_albedo(a.x)), demod::remodulate(f.y, demod::effective_albedo(a.y)),
                         demod::remodulate(f.z, demod::effective_albedo(a.z)), f.w);
}

void launch_denoise_albedo(hipStream_t s, const DScene& scene, DTex tx, const DCamera& cam, const float4* color, float4* albedo,
                           float4* irradiance, float4* rays, unsigned long long* stats, uint32_t* flags)
{
  const dim3 grid(((cam.width + 7u) / 8u) * ((cam.height + 7u) / 8u)), block(kWave);
  hipLaunchKernelGGL(k_denoise_albedo, grid, block, 0, s, scene, tx, cam, color, albedo, irradiance, rays, stats, flags);
}

void launch_remodulate(hipStream_t s, uint32_t pix_count, const float4* albedo, float4* front)
{
  hipLaunchKernelGGL(k_remodulate, dim3((pix_count + 255u) / 256u), dim3(256), 0, s, pix_count, albedo, front);
}

}  // namespace pt
