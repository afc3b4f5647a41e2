// pt_mega_direct.hip -- direct lighting in the megakernel: k_megakernel_direct is k_megakernel<true>'s loop
// (pt_kernels.hip) with one light sample (section 5f, pt_light_sample.hpp) and one shadow ray at every diffuse hit, a per-path
// radiance sum and the emission gate that keeps a lamp from being counted twice.  The shadow ray takes a per-thread any-hit walk
// (scene_occluded) on the thread's own LDS stack, which is free while the shadow ray runs.  Part of libptcore.so.
//
// The light samples draw from a stream of their own (path_seed(pixel, iteration) ^ kLightSeedXor, draws 3b .. 3b + 2 at bounce b),
// so every material draw, every closest hit, the normal and depth planes and rays_total are those of k_megakernel at the same
// iteration: only the colour differs.  tests/direct_loop_ref.py restates the loop in numpy, operation for operation.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_light_sample.hpp"
#include <float.h>

namespace pt {

#include "pt_kernels_common.inc"

// The any-hit form of mesh_closest_wide (pt_kernels_common.inc): the same set-up, the same inner-box decisions (the shortcut
// unless the slab extremes are closer than its rounding error, then the reference's exact test), the same leaf margins, the
// same culling -- but the limit stays at scale * t_max for the whole walk, a triangle is accepted for !(t < t_min) && !(t > t_max),
// and the first accepted triangle ends the walk.  mesh_closest_wide started at best_t = t_max, best_k = -1 accepts the same set of
// triangles (t < best_t, or t == best_t and k > -1) and culls MORE (its limit shrinks), so "this walk returns true" == "that walk
// finds a triangle" == the reference's answer for the object (no order appears in it).
__device__ __forceinline__ bool mesh_any_wide(const Ray& ray, const DScene& sc, const DMeshView& mv, const DObject* obj,
                                              const uint32_t tri_base, uint32_t* stack, uint32_t& flags)
{
  if (mv.bvh_node_count == 0u) return false;
  // inverse_transform_ray (transform.hpp:51-58); scale = length before the re-normalisation
  const f3 v = xform_vector(obj->inv_m, ray.d);
  const float scale = ieee_sqrt(dot(v, v));
  const f3 od = v * (1.0f / scale);
  const f3 oo = xform_point(obj->inv_m, ray.o);
  const f3 inv = mk3(1.0f / od.x, 1.0f / od.y, 1.0f / od.z);
  const bool exact_only = !(finite_f(inv.x) && finite_f(inv.y) && finite_f(inv.z));
  const float limit = scale * ray.tmax;
  const float ext = fmaxf(fmaxf(fmaxf(fabsf(mv.root_min[0]), fabsf(mv.root_max[0])), fmaxf(fabsf(mv.root_min[1]), fabsf(mv.root_max[1]))),
                          fmaxf(fabsf(mv.root_min[2]), fabsf(mv.root_max[2])));
  const float pad_t = world_rounding_pad(obj, ray.o, ext) * fmaxf(fmaxf(fabsf(inv.x), fabsf(inv.y)), fabsf(inv.z));

  uint32_t cur = mv.root_ref;
  if (!(cur & kLeafBit)) {
    float tn, tf;
    if (!box_pass_inner(ld3(mv.root_min), ld3(mv.root_max), oo, od, inv, exact_only, tn, tf)) return false;
    if (exact_only) slab_cull(ld3(mv.root_min), ld3(mv.root_max), oo, inv, tn, tf);
    if (box_culled(tn, tf, limit, pad_t)) return false;
  }
  const float4* tris = sc.tris + kTriVec4 * (size_t)tri_base;
  int sp = 0;
  for (;;) {
    if (cur & kLeafBit) {
      // ray_triangle_intersection_test (intersections.cuh:49-85) on the precomputed world-space edges
      const uint32_t k = cur & ~kLeafBit;
      const float4 ta = tris[kTriVec4 * k], tb = tris[kTriVec4 * k + 1u], tc = tris[kTriVec4 * k + 2u];
      const f3 p0 = mk3(ta.x, ta.y, ta.z), e1 = mk3(ta.w, tb.x, tb.y), e2 = mk3(tb.z, tb.w, tc.x);
      const f3 h = cross(ray.d, e2);
      const float a = dot(e1, h);
      if (!(a > -0.0000001f && a < 0.0000001f)) {
        const float f = 1.0f / a;
        const f3 sv = ray.o - p0;
        const float u = f * dot(sv, h);
        if (!(u < 0.0f || u > 1.0f)) {
          const f3 q = cross(sv, e1);
          const float w = f * dot(ray.d, q);
          if (!(w < 0.0f || u + w > 1.0f)) {
            const float t = f * dot(e2, q);
            if (!(t < ray.tmin) && !(t > ray.tmax)) return true;  // the first accepted triangle ends the walk
          }
        }
      }
      if (sp == 0) break;
      --sp;
      cur = stack[sp * kWave];
      continue;
    }
    const float4 w0 = mv.wide[4u * (size_t)cur], w1 = mv.wide[4u * (size_t)cur + 1u];
    const float4 w2 = mv.wide[4u * (size_t)cur + 2u], w3 = mv.wide[4u * (size_t)cur + 3u];
    const uint32_t lref = __float_as_uint(w3.x), rref = __float_as_uint(w3.y);
    const f3 lmin = mk3(w0.x, w0.y, w0.z), lmax = mk3(w0.w, w1.x, w1.y);
    const f3 rmin = mk3(w1.z, w1.w, w2.x), rmax = mk3(w2.y, w2.z, w2.w);
    // both children as in mesh_closest_wide: an inner child's decision equals the reference's, a leaf child's triangle is skipped
    // only when the ray misses its box, grown by 1e-5 of its coordinates, by more than the shortcut's rounding
    const bool l_leaf = (lref & kLeafBit) != 0u, r_leaf = (rref & kLeafBit) != 0u;
    auto grow = [&](const f3 lo, const f3 hi, bool leaf) -> f3 {
      const float k = leaf ? 1e-5f : 0.0f;
      return mk3(k * (fabsf(lo.x) + fabsf(hi.x) + fabsf(oo.x)) + (leaf ? 1e-30f : 0.0f),
                 k * (fabsf(lo.y) + fabsf(hi.y) + fabsf(oo.y)) + (leaf ? 1e-30f : 0.0f),
                 k * (fabsf(lo.z) + fabsf(hi.z) + fabsf(oo.z)) + (leaf ? 1e-30f : 0.0f));
    };
    const f3 lm = grow(lmin, lmax, l_leaf), rm = grow(rmin, rmax, r_leaf);
    const f3 lmin_c = lmin - lm, lmax_c = lmax + lm, rmin_c = rmin - rm, rmax_c = rmax + rm;  // inner: unchanged
    float ln, lf, rn, rf;
    slab_fast(lmin_c, lmax_c, oo, inv, ln, lf);
    slab_fast(rmin_c, rmax_c, oo, inv, rn, rf);
    const float lgap = lf - ln, rgap = rf - rn;
    const float ltol = 4e-7f * (fabsf(lf) + fabsf(ln)) + 1e-30f;
    const float rtol = 4e-7f * (fabsf(rf) + fabsf(rn)) + 1e-30f;
    bool go_l = l_leaf ? !(lgap < -(ltol + 2.0f * pad_t)) : (lgap > ltol);
    bool go_r = r_leaf ? !(rgap < -(rtol + 2.0f * pad_t)) : (rgap > rtol);
    const bool l_unsure = !l_leaf && (exact_only || !(lgap > ltol || lgap < -ltol));
    const bool r_unsure = !r_leaf && (exact_only || !(rgap > rtol || rgap < -rtol));
    if (__builtin_expect(l_unsure || r_unsure || exact_only, 0)) {
      if (l_unsure) go_l = slab_exact(lmin, lmax, oo, od, ln, lf);
      if (r_unsure) go_r = slab_exact(rmin, rmax, oo, od, rn, rf);
      if (exact_only) {
        go_l = go_l || l_leaf;
        go_r = go_r || r_leaf;
        slab_cull(lmin_c, lmax_c, oo, inv, ln, lf);
        slab_cull(rmin_c, rmax_c, oo, inv, rn, rf);
      }
    }
    go_l = go_l && !box_culled(ln, lf, limit, pad_t);
    go_r = go_r && !box_culled(rn, rf, limit, pad_t);
    if (go_l && go_r) {
      const bool left_first = !(rn < ln);
      const uint32_t first = left_first ? lref : rref, second = left_first ? rref : lref;
      if (sp >= kWideStack) {
        flags |= kFlagStackOverflow;
      } else {
        stack[sp * kWave] = second;
        ++sp;
      }
      cur = first;
    } else if (go_l || go_r) {
      cur = go_l ? lref : rref;
    } else {
      if (sp == 0) break;
      --sp;
      cur = stack[sp * kWave];
    }
  }
  return false;
}

// occluded(ray) := the reference's ray_scene_intersection_test (path_tracer.cu:110-128) reports a hit.
// Objects in list order, each one from the caller's t_max (the OR-over-groups argument: every object is a group of its own):
// the world box by ray_aabb first, a sphere in object space against the world-space t_max, a mesh by mesh_any_wide.  The first
// object that reports a hit ends the walk.
__device__ __forceinline__ bool scene_occluded(const Ray& ray, const DScene& sc, uint32_t* stack, uint32_t& flags)
{
  for (uint32_t i = 0; i < sc.object_count; ++i) {
    const DObject* obj = sc.objects + i;
    if (!ray_aabb(ray.o, ray.d, ld3(obj->bmin), ld3(obj->bmax))) continue;
    if (obj->type == 0u) {
      Ray tr;
      inverse_transform_ray(obj->inv_m, ray, tr.o, tr.d);
      tr.tmin = ray.tmin;
      tr.tmax = ray.tmax;
      const float4 sp = sc.spheres[obj->index];
      Hit unused;
      if (ray_sphere(tr, xyz(sp), sp.w, unused)) return true;
    } else if (mesh_any_wide(ray, sc, sc.mesh_views[sc.object_mesh[i]], obj, sc.object_tri_base[i], stack, flags)) {
      return true;
    }
  }
  return false;
}

// path_tracing_mega_kernel (path_tracer.cu:227-269) with DESIGN section 5g's rule.  One thread per pixel of the band; launched only
// for a scene with a lamp table of total weight > 0 (so the scene has an emissive material: this is k_megakernel<true>'s loop).
// stats: kLightStatLines lines of kLoopStatWords 64-bit words; word 0 += diffuse hits, word 1 += shadow rays traced, word 2 += unoccluded ones.
// kRoulette: Russian roulette from bounce `roulette` on, the last bounce excepted, as k_megakernel's: a path that
// ends there leaves colour 0, takes no light sample at that hit and adds nothing to the three loop counters; a survivor's light
// sample is weighted with the divided colour.
template <bool kRoulette>
__global__ __launch_bounds__(kWave) void k_megakernel_direct(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band,
                                                             uint32_t pix_count, int max_bounces, DFrame fb,
                                                             DeviceCounters* counters, unsigned long long* stats, int roulette)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  const uint32_t s = blockIdx.x * kWave + threadIdx.x;
  uint32_t rays = 0u, flags = 0u;
  uint32_t n_diffuse = 0u, n_shadow = 0u, n_clear = 0u;
  if (s < pix_count) {
    const uint32_t pixel = band_pixel(band, s);
    const uint32_t x = pixel % cam.width, y = pixel / cam.width;
    Minstd rng;
    rng.seed(path_seed(pixel, iteration));
    const float fx = (float)x + rng.uniform();
    const float fy = (float)y + rng.uniform();
    Ray ray;
    generate_ray(cam, fx, fy, ray.o, ray.d);
    ray.tmin = 1e-4f;
    ray.tmax = FLT_MAX;
    f3 color = mk3(1.0f, 1.0f, 1.0f);
    f3 radiance = mk3(0.0f, 0.0f, 0.0f);
    bool count_emission = true;  // the last vertex drew no light sample (the camera, metal, glass): a lamp hit from it counts
    f3 normal = -ray.d;
    float depth = 1e6f;
    for (int i = 0; i < max_bounces; ++i) {
      Hit rec;
      rec.t = 0.0f;
      rec.p = rec.n = mk3(0.f, 0.f, 0.f);
      rec.mat = 0u;
      rec.side = 0u;
      ++rays;
      Tally tally;
      if (!ray_scene<false>(ray, sc, rec, s_stack + threadIdx.x, flags, tally)) {
        color = color * background(ray.d);
        break;
      }
      if (i == 0) {
        normal = rec.n;
        depth = rec.t;
      }
      bool tmin_flag = ray.tmin != 1e-4f;
      const DMaterial mat = sc.materials[rec.mat];
      if (is_emitter(mat)) {  // the path ends at the emitter: no draw; after a diffuse vertex its light sample has counted the lamp
        color = count_emission ? emit_color(color, mat) : mk3(0.0f, 0.0f, 0.0f);
        break;
      }
      if (kRoulette && i >= roulette && i != max_bounces - 1 && roulette_ends(color, pixel, iteration, (uint32_t)i)) {
        color = mk3(0.0f, 0.0f, 0.0f);  // the path ends by chance: radiance + 0 is deposited, no draw, no light sample
        break;
      }
      evaluate_material(ray.o, ray.d, tmin_flag, rec.p, rec.n, rec.side, mat, rng, color);
      ray.tmin = tmin_flag ? 1e-5f : 1e-4f;
      count_emission = mat.type != 0;
      if (mat.type == 0) {  // diffuse: colour is throughput x albedo now; one light sample at the hit, about the unflipped normal
        ++n_diffuse;
        const LightSample ls = light_sample_point(lt, rec.p, rec.n, pixel, iteration, 3u * (uint32_t)i);
        if (ls.sampled) {
          ++n_shadow;
          Ray shadow;
          shadow.o = rec.p;
          shadow.tmin = 1e-4f;
          shadow.d = ls.w;
          shadow.tmax = ls.tmax;
          if (!scene_occluded(shadow, sc, s_stack + threadIdx.x, flags)) {
            ++n_clear;
            radiance = radiance + color * ls.contrib;
          }
        }
      }
    }
    accumulate_color(fb.color4, s, iteration, radiance + color);
    accumulate_nd(fb.nd4, s, iteration, normal, depth);
    if (flags) atomicOr(&counters->flags, flags);
  }
  // one atomic per counter and wavefront; the three loop counters spread over lines (adds to one line serialise in L2)
  uint32_t sum = rays, sd = n_diffuse, ss = n_shadow, sv = n_clear;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    sd += __shfl_down(sd, off, 64);
    ss += __shfl_down(ss, off, 64);
    sv += __shfl_down(sv, off, 64);
  }
  if (threadIdx.x == 0u) {
    if (sum) atomicAdd(&counters->rays_total, (unsigned long long)sum);
    unsigned long long* line = stats + kLoopStatWords * (blockIdx.x % kLightStatLines);
    if (sd) atomicAdd(&line[0], (unsigned long long)sd);
    if (ss) atomicAdd(&line[1], (unsigned long long)ss);
    if (sv) atomicAdd(&line[2], (unsigned long long)sv);
  }
}

// the plain megakernel's instances that play roulette (pt_megakernel.inc; the plain ones: pt_kernels.hip)
#include "pt_megakernel.inc"

void launch_megakernel_roulette(hipStream_t s, const DScene& scene, const DCamera& cam, uint32_t iteration, DBand band, uint32_t pix_count,
                                int max_bounces, DFrame fb, DeviceCounters* counters, bool emitters, int roulette)
{
  const dim3 grid((pix_count + kWave - 1u) / kWave), block(kWave);
  if (emitters)
    hipLaunchKernelGGL((k_megakernel<true, true>), grid, block, 0, s, scene, cam, iteration, band, pix_count, max_bounces, fb, counters, roulette);
  else
    hipLaunchKernelGGL((k_megakernel<false, true>), grid, block, 0, s, scene, cam, iteration, band, pix_count, max_bounces, fb, counters, roulette);
}

void launch_megakernel_direct(hipStream_t s, const DScene& scene, const DLights& lights, const DCamera& cam, uint32_t iteration, DBand band,
                              uint32_t pix_count, int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats,
                              int roulette)
{
  const dim3 grid((pix_count + kWave - 1u) / kWave), block(kWave);
  if (roulette >= 1 && roulette < max_bounces - 1)  // some bounce plays roulette
    hipLaunchKernelGGL(k_megakernel_direct<true>, grid, block, 0, s, scene, lights, cam, iteration, band, pix_count, max_bounces, fb, counters,
                       stats, roulette);
  else
    hipLaunchKernelGGL(k_megakernel_direct<false>, grid, block, 0, s, scene, lights, cam, iteration, band, pix_count, max_bounces, fb, counters,
                       stats, roulette);
}
}  // namespace pt
