// pt_occlude.hip -- occlusion queries: k_occlude_spheres and k_occlude4, the any-hit counterpart of the
// closest-hit stage (k_spheres, k_traverse4), and their launchers.  occluded(ray) := the reference's
// ray_scene_intersection_test (path_tracer.cu:110-128) reports a hit; the answer is one byte per ray that the host
// zeroes and the kernels only ever set to 1.  The ray feed, the set-aside list and the launch's epilogue are
// pt_walk.inc's.  Part of libptcore.so.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include <float.h>

#ifdef PT_TAILPROF
#undef PT_TAILPROF  // (the per-wavefront timeline belongs to k_traverse4's unit, pt_kernels.hip)
#endif

namespace pt {

#include "pt_kernels_common.inc"
#include "pt_walk.inc"

// The rays of an occlusion query: o4 = origin.xyz, bits(t_min flag << 31) as in the path state (DPaths::o4; t_min is 1e-5
// when the flag is set, else 1e-4), d4 = direction.xyz, t_max.
__device__ __forceinline__ Ray load_shadow_ray(const float4* o4, const float4* d4, uint32_t s)
{
  const float4 o = ldnt(&o4[s]);
  const float4 d = ldnt(&d4[s]);
  Ray r;
  r.o = xyz(o);
  r.d = xyz(d);
  r.tmin = (__float_as_uint(o.w) >> 31) ? 1e-5f : 1e-4f;
  r.tmax = d.w;
  return r;
}

// The sphere objects of [obj_begin, obj_end) as ONE group of the exactness argument: the reference's own sequence
// (sphere_segment: world box, inverse transform, quadratic; the carried t_max shrinks inside the group as in the
// reference's loop) from the caller's t_max.  Mesh objects inside the range are skipped by sphere_segment.  One thread per
// ray that is not flagged yet; the loop over the objects is wave-uniform, so object data comes through scalar loads.
__global__ __launch_bounds__(256) void k_occlude_spheres(DScene sc, uint32_t obj_begin, uint32_t obj_end, const float4* o4, const float4* d4,
                                                         uint32_t n, uint8_t* occ)
{
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  if (occ[s] != 0u) return;
  Ray ray = load_shadow_ray(o4, d4, s);
  Hit rec;
  bool changed = false;
  sphere_segment<true>(sc, obj_begin, obj_end, ray, rec, changed);
  if (changed) occ[s] = (uint8_t)1;
}

// The any-hit walk of one mesh object: traverse4_walk's node and leaf step (duplicated here rather than shared: a shared
// step would have to leave every existing instance of k_traverse4 / k_traverse4m / k_persist byte for byte the same code, and
// the step is woven into that function's best_t / best_k / split state) with what a shadow ray does not need taken out.
//   * per lane: ray, reciprocals, tolerances, stack pointer.  No closest hit so far, no tie rule, no normal, no carried
//     hit; the culling limit is scale * t_max * 1.001 for the whole walk.
//   * the first triangle the lane's test accepts ends the walk; the lane then decides as finalize does -- world box and
//     parent box by their cheap sufficient forms, else the reference's own tests: world box fails -> the reference skips
//     the object, parent box fails -> the ray is set aside for the exact redo (one candidate per ray, never "go on
//     without this triangle").
//   * a ray whose byte is already 1 is not walked.
//   * no work splitting at the end of the launch (traverse4_walk::split): not needed for the answer, it costs four LDS arrays
//     and a dozen registers, and the launch came out below the closest-hit launch on the same rays without it
//     (profiles/occlusion_ab.txt).  Where its tail goes has not been looked at.
__device__ __forceinline__ void occlude4_walk(const DScene& sc, uint32_t obj_index, const float4* rays_o, const float4* rays_d, uint8_t* occ,
                                              int work_slot, DeviceCounters* counters, uint32_t* slow_list, const DBatchInfo& bi)
{
  __shared__ uint32_t s_stack[kLds4 * kWave];
  typedef __attribute__((address_space(3))) uint32_t lds_u32;  // (as a generic pointer the pop compiles to a flat load)
  lds_u32* stack = (lds_u32*)s_stack + threadIdx.x;
  const uint32_t gid = blockIdx.x * kWave + threadIdx.x;
  const uint32_t n = counters->live[0];
  if (n == 0u) return;
  // more wavefronts than batches (the margin keeps every wavefront that owns a static batch, see BatchFeed)
  if (blockIdx.x >= (n + kWave - 1u) / kWave + 8u) return;
  const DObject* obj = sc.objects + obj_index;
  const float4* tris = sc.tris + kTriVec4 * (size_t)sc.object_tri_base[obj_index];
  auto uni = [](float v) { return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v))); };
  const f3 obj_bmin = mk3(uni(obj->bmin[0]), uni(obj->bmin[1]), uni(obj->bmin[2]));
  const f3 obj_bmax = mk3(uni(obj->bmax[0]), uni(obj->bmax[1]), uni(obj->bmax[2]));
  BatchFeed feed;
  feed.init(counters, bi, 0, work_slot, sc.static_eighths, false);
  uint32_t priv_next = 0u, priv_end = 0u;

  bool active = false;
  bool pending = false;  // the lane's walk ended at a triangle its test accepted (`cand`): decided at the next refill
  uint32_t slot = 0u, cur = 0u, cand = 0u, flags = 0u;
  int sp = 0;
  f3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 0), inv = mk3(0, 0, 0);
  f3 oin = mk3(0, 0, 0), oif = mk3(0, 0, 0);
  bool neg_x = false, neg_y = false, neg_z = false;
  float tmin = 0.0f, tmax = 0.0f, limit = 0.0f;

  const int lds_cap = min((int)sc.lds_cap, kLds4);
  auto push = [&](uint32_t ref) {
    if (sp < lds_cap) stack[sp * kWave] = ref;
    else if (sp < lds_cap + (int)sc.spill_cap) sc.spill[(size_t)(sp - lds_cap) * sc.spill_stride + gid].x = ref;
    else {
      flags |= kFlagStackOverflow;
      return;
    }
    ++sp;
  };
  // (traverse4_walk's: the conservative slab pair with the tolerance folded INWARDS -- non-empty: the reference's test passes)
  auto surely_inside = [&](const f3 lo, const f3 hi) -> bool {
    const bool nx = neg_x, ny = neg_y, nz = neg_z;
    const float tn = fmaxf(fmaxf(__builtin_fmaf(nx ? hi.x : lo.x, inv.x, oif.x), __builtin_fmaf(ny ? hi.y : lo.y, inv.y, oif.y)),
                           __builtin_fmaf(nz ? hi.z : lo.z, inv.z, oif.z));
    const float tf = fminf(fminf(__builtin_fmaf(nx ? lo.x : hi.x, inv.x, oin.x), __builtin_fmaf(ny ? lo.y : hi.y, inv.y, oin.y)),
                           __builtin_fmaf(nz ? lo.z : hi.z, inv.z, oin.z));
    return tf >= tn;
  };
  // The candidate is a triangle the reference's test accepts with the caller's t_max.  It occludes iff the reference reaches
  // it: the object's world box passes (path_tracer.cu:84) and the box of its parent passes the reference's own test
  // (nesting) -- traverse4_walk::finalize's two decisions, operation for operation.
  auto finalize = [&]() {
    const size_t win = (size_t)cand;
    const float4 pb0 = sc.cur.leaf_parent[2u * win], pb1 = sc.cur.leaf_parent[2u * win + 1u];
    const f3 bmin = obj_bmin, bmax = obj_bmax;
    const f3 winv = mk3(__builtin_amdgcn_rcpf(rd.x), __builtin_amdgcn_rcpf(rd.y), __builtin_amdgcn_rcpf(rd.z));
    const f3 a0 = (bmin - ro) * winv, a1 = (bmax - ro) * winv;
    const float wn = fmaxf(fmaxf(fminf(a0.x, a1.x), fminf(a0.y, a1.y)), fminf(a0.z, a1.z));
    const float wf = fminf(fminf(fmaxf(a0.x, a1.x), fmaxf(a0.y, a1.y)), fmaxf(a0.z, a1.z));
    const bool box_ok = !(bmin.x > bmax.x || bmin.y > bmax.y || bmin.z > bmax.z);
    const bool world_sure = box_ok && finite_f(winv.x + winv.y + winv.z) && (wf - wn) > 2e-6f * (fabsf(wf) + fabsf(wn));
    const bool parent_sure = surely_inside(xyz(pb0), xyz(pb1));
    bool occluded = true;
    if (__builtin_expect(!(world_sure && parent_sure) || sc.force_slow == 2u, 0)) {
      if (!ray_aabb(ro, rd, bmin, bmax)) {
        occluded = false;  // the reference skips the object
      } else {
        const f3 od = normalize(xform_vector(obj->inv_m, rd));  // inverse_transform_ray, transform.hpp:51-58
        const f3 oo = xform_point(obj->inv_m, ro);
        float en, ef;
        if (!slab_exact(xyz(pb0), xyz(pb1), oo, od, en, ef) || sc.force_slow == 2u) {
          set_aside(counters, slow_list, slot);  // grazes the parent's box within rounding: the launch's epilogue decides exactly
          occluded = false;
        }
      }
    }
    if (occluded) occ[slot] = (uint8_t)1;
  };

  // One step of every active lane: traverse4_walk::step -- the same four 16-byte loads and the stack-top read in ONE asm
  // statement that carries its wait, the same slab arithmetic and tolerance folding, the same triangle arithmetic.
  auto step = [&]() {
    if (active) {
      const bool is_leaf = (cur & kLeafBit) != 0u;
      const uint32_t index = cur & ~kLeafBit;
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      u32x4 w0, w1, w2, w3;
      constexpr bool kLeaf48 = kTriVec4 == 3u;
      const char* rec = is_leaf ? reinterpret_cast<const char*>(tris) + (16u * kTriVec4) * (size_t)index
                                : reinterpret_cast<const char*>(sc.cur.bvh4q) + 64u * (size_t)index;
      const char* rec3 = rec + (kLeaf48 && is_leaf ? 32 : 48);
      const int top = sp - 1;
      const uint32_t below_addr = (uint32_t)(uintptr_t)(stack + min(max(top, 0), lds_cap - 1) * kWave);
      uint32_t below;
      asm volatile(
          "global_load_dwordx4 %0, %5, off\n\t"
          "global_load_dwordx4 %1, %5, off offset:16\n\t"
          "global_load_dwordx4 %2, %5, off offset:32\n\t"
          "global_load_dwordx4 %3, %6, off\n\t"
          "ds_read_b32 %4, %7\n\t"
          "s_waitcnt vmcnt(0) lgkmcnt(0)"
          : "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3), "=&v"(below)
          : "v"(rec), "v"(rec3), "v"(below_addr)
          : "memory");
      if (__builtin_expect(top >= lds_cap, 0)) below = sc.spill[(size_t)(top - lds_cap) * sc.spill_stride + gid].x;
      below = top >= 0 ? below : kNoChild;
      const uint4 q0 = make_uint4(w0.x, w0.y, w0.z, w0.w), q1 = make_uint4(w1.x, w1.y, w1.z, w1.w);
      const uint4 q2 = make_uint4(w2.x, w2.y, w2.z, w2.w), q3 = make_uint4(w3.x, w3.y, w3.z, w3.w);
      if (!is_leaf) {
        const f3 org = mk3(__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z));
        const f3 ax = mk3(__uint_as_float(q0.w) * inv.x, __uint_as_float(q2.z) * inv.y, __uint_as_float(q2.w) * inv.z);
        const f3 bn = mk3(__builtin_fmaf(org.x, inv.x, oin.x), __builtin_fmaf(org.y, inv.y, oin.y), __builtin_fmaf(org.z, inv.z, oin.z));
        const f3 bf = mk3(__builtin_fmaf(org.x, inv.x, oif.x), __builtin_fmaf(org.y, inv.y, oif.y), __builtin_fmaf(org.z, inv.z, oif.z));
        const uint32_t nqx = neg_x ? q1.w : q1.x, fqx = neg_x ? q1.x : q1.w;
        const uint32_t nqy = neg_y ? q2.x : q1.y, fqy = neg_y ? q1.y : q2.x;
        const uint32_t nqz = neg_z ? q2.y : q1.z, fqz = neg_z ? q1.z : q2.y;
        float key[4];
        uint32_t ref[4] = {q3.x, q3.y, q3.z, q3.w};
        // (tn a lower bound of the entry distance, tf an upper bound of the exit distance: the child is skipped when
        // [max(tn, 0), min(tf, limit)] is empty -- missed, behind the origin, or beyond t_max with its 0.1 % margin)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float cnx = (float)((nqx >> (8 * c)) & 0xffu), cny = (float)((nqy >> (8 * c)) & 0xffu), cnz = (float)((nqz >> (8 * c)) & 0xffu);
          const float cfx = (float)((fqx >> (8 * c)) & 0xffu), cfy = (float)((fqy >> (8 * c)) & 0xffu), cfz = (float)((fqz >> (8 * c)) & 0xffu);
          const float tn = fmaxf(fmaxf(fmaxf(__builtin_fmaf(cnx, ax.x, bn.x), __builtin_fmaf(cny, ax.y, bn.y)),
                                       __builtin_fmaf(cnz, ax.z, bn.z)), 0.0f);
          const float tf = fminf(fminf(fminf(__builtin_fmaf(cfx, ax.x, bf.x), __builtin_fmaf(cfy, ax.y, bf.y)),
                                       __builtin_fmaf(cfz, ax.z, bf.z)), limit);
          key[c] = tn <= tf ? tn : __builtin_inff();
        }
        // children nearest first, the others on the stack farthest first (any order gives the same answer, DESIGN section 5e;
        // slot order without the five compare-exchanges measured the same within the run-to-run spread, profiles/occlusion_ab.txt)
        auto cx = [&](int a, int b) {
          const bool sw = key[b] < key[a];
          const float ka = sw ? key[b] : key[a], kb = sw ? key[a] : key[b];
          const uint32_t ra = sw ? ref[b] : ref[a], rb = sw ? ref[a] : ref[b];
          key[a] = ka;
          key[b] = kb;
          ref[a] = ra;
          ref[b] = rb;
        };
        cx(0, 1);
        cx(2, 3);
        cx(0, 2);
        cx(1, 3);
        cx(1, 2);
        if (__builtin_expect(sp + 3 <= lds_cap, 1)) {
          stack[sp * kWave] = ref[3];
          sp += key[3] < __builtin_inff() ? 1 : 0;
          stack[sp * kWave] = ref[2];
          sp += key[2] < __builtin_inff() ? 1 : 0;
          stack[sp * kWave] = ref[1];
          sp += key[1] < __builtin_inff() ? 1 : 0;
        } else {
          if (key[3] < __builtin_inff()) push(ref[3]);
          if (key[2] < __builtin_inff()) push(ref[2]);
          if (key[1] < __builtin_inff()) push(ref[1]);
        }
        if (key[0] < __builtin_inff()) {
          cur = ref[0];
        } else {  // nothing was pushed: `below` is still the top
          cur = below;
          sp = max(sp - 1, 0);
        }
      } else {
        // ray_triangle_intersection_test (intersections.cuh:49-85) on the precomputed world-space edges, straight-line
        const f3 p0 = mk3(__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z));
        const f3 e1 = mk3(__uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y));
        const f3 e2 = mk3(__uint_as_float(q1.z), __uint_as_float(q1.w), __uint_as_float(q2.x));
        const f3 h = cross(rd, e2);
        const float a = dot(e1, h);
        const f3 sv = ro - p0;
        const float f = 1.0f / a;
        const float u = f * dot(sv, h);
        const f3 qv = cross(sv, e1);
        const float w = f * dot(rd, qv);
        const float t = f * dot(e2, qv);
        const bool hit = !(a > -0.0000001f && a < 0.0000001f) & !(u < 0.0f || u > 1.0f) & !(w < 0.0f || u + w > 1.0f) &
                         !(t < tmin) & !(t > tmax);
        if (hit) {
          cand = index;
          pending = true;
          cur = kNoChild;  // the first accepted triangle ends the walk
        } else {
          cur = below;
          sp = max(sp - 1, 0);
        }
      }
      if (cur == kNoChild) active = false;
    }
  };

  for (;;) {
    const uint64_t idle_mask = __ballot(!active);
    const uint32_t idle = (uint32_t)__popcll(idle_mask);
    const bool more = priv_next < priv_end || !feed.exhausted();
    if (more && (idle == (uint32_t)kWave || idle >= sc.refill_lanes)) {
      if (pending) {
        finalize();
        pending = false;
      }
      if (priv_next >= priv_end && !feed.acquire(priv_next, priv_end)) priv_next = priv_end = 0u;
      const uint32_t mine = priv_next + rank_below(idle_mask);
      const uint32_t range_end = priv_end;
      priv_next = min(priv_end, priv_next + idle);
      if (!active && mine < range_end) {
        slot = mine;
        const float4 o4 = ldnt(&rays_o[slot]);
        const float4 d4 = ldnt(&rays_d[slot]);
        const uint32_t known = occ[slot];  // flagged by the spheres or by an earlier object's launch: nothing to find out
        ro = xyz(o4);
        rd = xyz(d4);
        tmin = (__float_as_uint(o4.w) >> 31) ? 1e-5f : 1e-4f;
        tmax = d4.w;
        if (known == 0u && sc.cur.bvh_node_count != 0u) {
          // (traverse4_walk's set-up: hardware rsq / rcp for the walk, their error inside the tolerance; what decides is exact)
          const f3 v = xform_vector(obj->inv_m, rd);
          const float len2 = dot(v, v);
          const float rlen = __builtin_amdgcn_rsqf(len2);
          const float scale = len2 * rlen;
          const f3 od = v * rlen;
          const f4 ow = mul(obj->inv_m, ro.x, ro.y, ro.z, 1.0f);
          const f3 oo_walk = mk3(ow.x, ow.y, ow.z) * __builtin_amdgcn_rcpf(ow.w);
          inv = mk3(__builtin_amdgcn_rcpf(od.x), __builtin_amdgcn_rcpf(od.y), __builtin_amdgcn_rcpf(od.z));
          const f3 oi = mk3(-(oo_walk.x * inv.x), -(oo_walk.y * inv.y), -(oo_walk.z * inv.z));
          const float bx = fmaxf(fabsf(sc.cur.root_min[0]), fabsf(sc.cur.root_max[0]));
          const float by = fmaxf(fabsf(sc.cur.root_min[1]), fabsf(sc.cur.root_max[1]));
          const float bz = fmaxf(fabsf(sc.cur.root_min[2]), fabsf(sc.cur.root_max[2]));
          const float pad = world_rounding_pad(obj, ro, fmaxf(fmaxf(bx, by), bz));
          const f3 tol = mk3(4e-6f * (fabsf(oi.x) + bx * fabsf(inv.x)) + pad * fabsf(inv.x) + 1e-30f,
                             4e-6f * (fabsf(oi.y) + by * fabsf(inv.y)) + pad * fabsf(inv.y) + 1e-30f,
                             4e-6f * (fabsf(oi.z) + bz * fabsf(inv.z)) + pad * fabsf(inv.z) + 1e-30f);
          if (__builtin_expect(!(finite_f(inv.x) && finite_f(inv.y) && finite_f(inv.z) && finite_f(tol.x + tol.y + tol.z)) ||
                               sc.force_slow == 1u, 0)) {
            // degenerate direction: the error bound is void -- set aside for the exact redo, as in traverse4_walk
            set_aside(counters, slow_list, slot);
          } else {
            oin = oi - tol;
            oif = oi + tol;
            neg_x = inv.x < 0.0f;
            neg_y = inv.y < 0.0f;
            neg_z = inv.z < 0.0f;
            limit = scale * tmax * 1.001f;
            cur = sc.cur.bvh4_root;
            sp = 0;
            active = true;
          }
        }
      }
    }
    if (__ballot(active) == 0ull) {
      if (!more) break;
      continue;
    }
    step();
  }
  if (pending) finalize();
  if (flags) atomicOr(&counters->flags, flags);
}

// The rays the launch set aside, with EXACT box decisions (redo_slow_rays' walk): the world box by ray_aabb, then
// mesh_closest_wide from the caller's t_max -- "it found a triangle" is the reference's answer for this object.
__device__ __forceinline__ void redo_occluded(const DScene& sc, uint32_t obj_index, const float4* rays_o, const float4* rays_d, uint8_t* occ,
                                              const uint32_t* slow_list, uint32_t count, DeviceCounters* counters)
{
  const DObject* obj = sc.objects + obj_index;
  const uint32_t tri_base = sc.object_tri_base[obj_index];
  uint32_t flags = 0u;
  for (uint32_t i = threadIdx.x; i < count; i += kWave) {
    const uint32_t slot = __hip_atomic_load(&slow_list[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const Ray ray = load_shadow_ray(rays_o, rays_d, slot);
    float best_t = ray.tmax;
    int best_k = -1;
    Tally unused;
    if (ray_aabb(ray.o, ray.d, ld3(obj->bmin), ld3(obj->bmax)))
      mesh_closest_wide<false>(ray, sc, sc.cur, obj, tri_base, best_t, best_k, sc.slow_stack + threadIdx.x, flags, unused);
    if (best_k >= 0) occ[slot] = (uint8_t)1;
  }
  if (flags) atomicOr(&counters->flags, flags);
}

__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PT_T4_WAVES, PT_T4_WAVES)))
void k_occlude4(DScene sc, uint32_t obj_index, const float4* rays_o, const float4* rays_d, uint8_t* occ, int work_slot,
                DeviceCounters* counters, uint32_t* slow_list, DBatchInfo bi)
{
  occlude4_walk(sc, obj_index, rays_o, rays_d, occ, work_slot, counters, slow_list, bi);
  // Epilogue, as k_traverse4's: every wavefront signs off, the last one redoes what was set aside (agent-scope list) and
  // leaves the counters ready for the next launch on this stream.
  uint32_t prev = 0u;
  if (threadIdx.x == 0u) {
    __builtin_amdgcn_s_waitcnt(0);
    prev = __hip_atomic_fetch_add(&counters->waves_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  prev = (uint32_t)__builtin_amdgcn_readfirstlane((int)prev);
  if (prev + 1u != gridDim.x) return;
  const uint32_t count = __hip_atomic_load(&counters->slow_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (count != 0u) redo_occluded(sc, obj_index, rays_o, rays_d, occ, slow_list, count, counters);
  launch_epilogue(counters, 0, work_slot, count, bi, false);
}

void launch_occlude_spheres(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, const float4* rays_o,
                            const float4* rays_d, uint32_t n, uint8_t* occluded)
{
  hipLaunchKernelGGL(k_occlude_spheres, dim3((n + 255u) / 256u), dim3(256), 0, s, scene, obj_begin, obj_end, rays_o, rays_d, n, occluded);
}
void launch_occlude(hipStream_t s, const DScene& scene, uint32_t obj_index, const float4* rays_o, const float4* rays_d,
                    uint8_t* occluded, int work_slot, DeviceCounters* counters, uint32_t waves, uint32_t* slow_list, const DBatchInfo& bi)
{
  hipLaunchKernelGGL(k_occlude4, dim3(waves), dim3(kWave), 0, s, scene, obj_index, rays_o, rays_d, occluded, work_slot, counters, slow_list, bi);
}
}  // namespace pt
