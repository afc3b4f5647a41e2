// pt_mega_nmap.hip -- normal maps (ptc_set_normal_maps, ptc_set_param "normal_maps"): the megakernel's four
// normal-mapped instances, k_megakernel_nmap<kMis, kSmooth>, and the shading-normal query's kernel, k_hit_shading_normal, with
// launch_mega_nmap (the rule that names an instance: pt_mega_rules.hpp) and the query's launcher -- in a translation unit of its own
// so that every other code object stays what it was.  The loop itself, with what kMegaNmap adds to it, is mega_path
// (pt_megakernel.inc); the rule is pt_normal_map.hpp's.  Part of libptcore.so.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_light_sample.hpp"
#include "pt_env_light.hpp"
#include "pt_smooth.hpp"
#include "pt_texture.hpp"
#include "pt_normal_map.hpp"
#include "pt_mega_rules.hpp"
#include <float.h>
#include <limits.h>

namespace pt {

#include "pt_kernels_common.inc"

#include "pt_megakernel.inc"

// k_megakernel_tex's shape with kNmap: the albedo fetch by tx.material_texture, the normal map by nm.material_normal_map (never null
// here: the rule launches these for a frame with a binding only)
template <bool kMis, bool kSmooth>
__global__ __launch_bounds__(kWave) void k_megakernel_nmap(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band, uint32_t pix_count,
                                                           int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats,
                                                           int roulette, DLens lens, DEnv env, DEnvLight el, DMis mis, DSmooth sm, DTex tx, DNmap nm)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kMegaEnvLit | kMegaTex | kMegaNmap | (kMis ? kMegaMis : 0u) | (kSmooth ? kMegaSmooth : 0u)>(
      sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats, roulette, s_stack + threadIdx.x, lens, env, el, mis, sm, tx, nm);
}

// ptc_hit_shading_normal: k_hit_surface's walk; at the winner the normal mega_path would hand to evaluate_material there from what is
// set -- the vertex normals' (sm.normals), then the normal map's (nm.material_normal_map with tx's pool and coordinates) about it.
// A miss: zeros and outcome 0.
__global__ __launch_bounds__(kWave) void k_hit_shading_normal(DScene sc, DSmooth sm, DTex tx, DNmap nm, const float4* rays, uint32_t n,
                                                              float* normal_out, uint8_t* outcome_out, uint32_t* flags_out)
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
  f3 hn = mk3(0.0f, 0.0f, 0.0f);
  uint32_t how = nmap::kMiss;
  if (ray_scene<false, true>(ray, sc, rec, s_stack + threadIdx.x, flags, tally, &at)) {
    hn = rec.n;
    how = nmap::kNone;
    if (at.first != kNoChild) {
      const uint32_t mesh = sc.object_mesh[at.object];
      const uint32_t* idx = sc.mesh_views[mesh].indices + at.first;
      if (sm.normals) {
        const float* vn = sm.normals + 3u * (size_t)sm.mesh_first_vertex[mesh];
        const f3 n0 = ld3(vn + 3u * (size_t)idx[0]), n1 = ld3(vn + 3u * (size_t)idx[1]), n2 = ld3(vn + 3u * (size_t)idx[2]);
        (void)smooth::shading_normal(n0, n1, n2, at.u, at.v, rec.n, ray.d, sc.objects[at.object].inv_m, hn);
      }
      const DMaterial& mat = sc.materials[rec.mat];
      if (nm.material_normal_map && tx.texels && tx.st && mat.type <= 1) {
        const int32_t ni = nm.material_normal_map[rec.mat];
        if (ni >= 0) {
          const float* stp = tx.st + 2u * ((size_t)tx.mesh_first_index[mesh] + at.first);
          const float* pos = sc.mesh_views[mesh].positions;
          const texmap::Record nrec = tx.records[ni];
          const float stc[6] = {stp[0], stp[1], stp[2], stp[3], stp[4], stp[5]};
          const f3 p0 = ld3(pos + 3u * (size_t)idx[0]), p1 = ld3(pos + 3u * (size_t)idx[1]), p2 = ld3(pos + 3u * (size_t)idx[2]);
          f3 nn;
          how = nmap::shade(tx.texels, nrec, nm.table, p0, p1, p2, stc, stc + 2, stc + 4, at.u, at.v, sc.objects[at.object].m, hn, rec.n, ray.d, nn);
          hn = nn;
        }
      }
    }
  }
  normal_out[3u * (size_t)r] = hn.x;
  normal_out[3u * (size_t)r + 1u] = hn.y;
  normal_out[3u * (size_t)r + 2u] = hn.z;
  outcome_out[r] = (uint8_t)how;
  if (flags) atomicOr(flags_out, flags);
}

void launch_mega_nmap(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in)
{
  mega_go_lit(in.b ? (in.a ? k_megakernel_nmap<true, true> : k_megakernel_nmap<false, true>)
                   : (in.a ? k_megakernel_nmap<true, false> : k_megakernel_nmap<false, false>),
              s, f, f.lens, f.env, f.el, f.mis, f.sm, f.tx, f.nm);
}

void launch_hit_shading_normal(hipStream_t s, const DScene& scene, DSmooth sm, DTex tx, DNmap nm, const float4* rays, uint32_t n,
                               float* normal_out, uint8_t* outcome_out, uint32_t* flags)
{
  const dim3 grid((n + kWave - 1u) / kWave), block(kWave);
  hipLaunchKernelGGL(k_hit_shading_normal, grid, block, 0, s, scene, sm, tx, nm, rays, n, normal_out, outcome_out, flags);
}
}  // namespace pt
