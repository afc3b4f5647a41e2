// pt_kernels_common.inc -- device functions shared by the kernel translation units (pt_kernels.hip: closest hit;
// pt_shade.hip: ray generation and the end of a bounce; pt_mega_direct.hip: the megakernel's shadow ray, scene_occluded over the
// any-hit option of the one two-wide walk; pt_post.hip: views, gather, denoiser).  Included inside namespace pt;
// everything here is __device__ __forceinline__ or a constant, so every unit gets its own copy of what it uses.
#pragma once


// ------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// number of set bits of `mask` below this lane
__device__ __forceinline__ uint32_t rank_below(uint64_t mask)
{
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ f3 ld3(const float* p) { return mk3(p[0], p[1], p[2]); }
// Path state, hit records and framebuffers stream through the chip once per kernel (hundreds of MB per frame), next to
// a BVH working set (75 MB of nodes and triangles at 1M triangles) that every ray re-reads and that should own the
// 4 MB L2 of its XCD: streaming accesses are marked non-temporal.
#ifndef PT_NT
#define PT_NT 1
#endif
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ldnt(const float4* p)
{
#if PT_NT
  const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
#else
  return *p;
#endif
}
__device__ __forceinline__ void stnt(float4* p, const float4 v)
{
#if PT_NT
  v4f w;
  w.x = v.x;
  w.y = v.y;
  w.z = v.z;
  w.w = v.w;
  __builtin_nontemporal_store(w, reinterpret_cast<v4f*>(p));
#else
  *p = v;
#endif
}
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 ldnt(const float2* p)
{
#if PT_NT
  const v2f v = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(p));
  return make_float2(v.x, v.y);
#else
  return *p;
#endif
}
__device__ __forceinline__ void stnt(float2* p, const float2 v)
{
#if PT_NT
  v2f w;
  w.x = v.x;
  w.y = v.y;
  __builtin_nontemporal_store(w, reinterpret_cast<v2f*>(p));
#else
  *p = v;
#endif
}
__device__ __forceinline__ f3 xyz(float4 v) { return mk3(v.x, v.y, v.z); }

struct Ray {
  f3 o;
  float tmin;
  f3 d;
  float tmax;
};
__device__ __forceinline__ f3 ray_at(const Ray& r, float t) { return r.o + r.d * t; }

// per-lane test counters of the instrumented kernel variant
struct Tally {
  uint32_t boxes = 0u, tris = 0u, nodes = 0u;  // ray/box tests, ray/triangle tests, node records fetched
};

struct Hit {
  float t;
  f3 p;
  f3 n;
  uint32_t mat;
  uint32_t side;  // 0 front, 1 back
};

// wavefront totals of the instrumented kernel variants -> the counter block (one atomic each)
__device__ __forceinline__ void flush_tally(const Tally& tally, DeviceCounters* counters, int bounce, bool per_ray_max)
{
  uint32_t b = tally.boxes, t = tally.tris, nd = tally.nodes, mx = tally.boxes;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    b += __shfl_down(b, off, 64);
    t += __shfl_down(t, off, 64);
    nd += __shfl_down(nd, off, 64);
    mx = max(mx, (uint32_t)__shfl_down(mx, off, 64));
  }
  if ((threadIdx.x & 63u) == 0u) {
    atomicAdd(&counters->box_tests[bounce], (unsigned long long)b);
    atomicAdd(&counters->tri_tests[bounce], (unsigned long long)t);
    atomicAdd(&counters->node_visits[bounce], (unsigned long long)nd);
    if (per_ray_max) atomicMax(&counters->max_box_tests[bounce], mx);  // one lane = one ray in those kernels
  }
}

// ------------------------------------------------------------------------------------------------
// intersection tests (reference intersections.cuh)
// ------------------------------------------------------------------------------------------------
// ray_aabb_intersection_test, intersections.cuh:87-103: no t-range, boxes behind the origin pass
__device__ __forceinline__ bool ray_aabb(const f3 o, const f3 d, const f3 bmin, const f3 bmax)
{
  if (bmin.x > bmax.x || bmin.y > bmax.y || bmin.z > bmax.z) return false;
  const f3 t0 = (bmin - o) / d;
  const f3 t1 = (bmax - o) / d;
  const f3 rmin = min3(t0, t1);
  const f3 rmax = max3(t0, t1);
  const float minmax = sel_min(sel_min(rmax.x, rmax.y), rmax.z);
  const float maxmin = sel_max(sel_max(rmin.x, rmin.y), rmin.z);
  return minmax >= maxmin;
}

// ray_sphere_intersection_test, intersections.cuh:7-41
// (a = dot(d, d) comes from the caller: sphere_segment can test many spheres with the same transformed direction)
__device__ __forceinline__ bool ray_sphere_a(const Ray& ray, const float a, const f3 center, const float radius, Hit& rec);
__device__ __forceinline__ bool ray_sphere(const Ray& ray, const f3 center, const float radius, Hit& rec)
{
  return ray_sphere_a(ray, dot(ray.d, ray.d), center, radius, rec);
}
__device__ __forceinline__ bool ray_sphere_a(const Ray& ray, const float a, const f3 center, const float radius, Hit& rec)
{
  const f3 oc = ray.o - center;
  const float b = 2.0f * dot(ray.d, oc);
  const float c = dot(oc, oc) - radius * radius;
  const float disc = b * b - 4.0f * a * c;
  if (disc < 0.0f) return false;
  const float sq = ieee_sqrt(disc);
  const float t1 = (-b - sq) / (2.0f * a);
  const float t2 = (-b + sq) / (2.0f * a);
  float t;
  if (t1 >= ray.tmin && t1 <= ray.tmax) t = t1;
  else if (t2 >= ray.tmin && t2 <= ray.tmax) t = t2;
  else return false;
  rec.t = t;
  rec.p = ray_at(ray, t);
  const f3 outward = (rec.p - center) / radius;
  rec.side = dot(ray.d, outward) < 0.0f ? 0u : 1u;
  rec.n = rec.side == 0u ? outward : -outward;
  return true;
}

// What a closest hit knows besides its record (smooth shading, DESIGN section 5n; the kAttr forms of ray_triangle, ray_mesh and
// ray_scene below): the winner's object, the offset of its triangle in the mesh's `indices` (kNoChild: a sphere) and the accepted
// test's own u, v.  The forms without kAttr are the instructions they were.
struct HitAttr {
  uint32_t object, first;
  float u, v;
};

// ray_triangle_intersection_test, intersections.cuh:49-85 (t == t_max accepted)
template <bool kAttr = false>
__device__ __forceinline__ bool ray_triangle(const Ray& ray, const f3 p0, const f3 p1, const f3 p2, Hit& rec, HitAttr* at = nullptr)
{
  const float EPS = 0.0000001f;
  const f3 e1 = p1 - p0;
  const f3 e2 = p2 - p0;
  const f3 h = cross(ray.d, e2);
  const float a = dot(e1, h);
  if (a > -EPS && a < EPS) return false;
  const float f = 1.0f / a;
  const f3 s = ray.o - p0;
  const float u = f * dot(s, h);
  if (u < 0.0f || u > 1.0f) return false;
  const f3 q = cross(s, e1);
  const float v = f * dot(ray.d, q);
  if (v < 0.0f || u + v > 1.0f) return false;
  const float t = f * dot(e2, q);
  if (t < ray.tmin || t > ray.tmax) return false;
  rec.t = t;
  rec.p = ray_at(ray, t);
  const f3 outward = normalize(cross(e1, e2));
  rec.side = dot(ray.d, outward) < 0.0f ? 0u : 1u;
  rec.n = rec.side == 0u ? outward : -outward;
  if constexpr (kAttr) {
    at->u = u;
    at->v = v;
  }
  return true;
}

// inverse_transform_ray, transform.hpp:51-58: direction re-normalised, t range copied unscaled
__device__ __forceinline__ void inverse_transform_ray(const m4& inv_m, const Ray& ray, f3& o, f3& d)
{
  o = xform_point(inv_m, ray.o);
  d = normalize(xform_vector(inv_m, ray.d));
}

// ray_mesh_intersection_test, path_tracer.cu:36-76.  Depth-first, left child first, every inner box
// the line crosses is entered (the reference has no t culling).  The stack lives in LDS, laid out
// [depth][lane] so that a push or pop of the whole wavefront touches 64 consecutive banks.
// kAttr: a hit also leaves the winner's place in `indices` and its u, v in *at (an equal t is accepted, so the triangle visited
// last wins a tie).
template <bool kCount, bool kAttr = false>
__device__ __forceinline__ bool ray_mesh(Ray ray, const DMeshView& mv, const DObject* obj, Hit& rec, uint32_t* stack,
                                         uint32_t& flags, Tally& tally, const int stack_cap = kStackDepth, HitAttr* at = nullptr)
{
  bool hit = false;
  f3 oo, od;
  inverse_transform_ray(obj->inv_m, ray, oo, od);
  if (mv.bvh_node_count == 0u) return false;

  int sp = 0;
  stack[0] = 0u;
  sp = 1;
  while (sp > 0) {
    --sp;
    const uint32_t node = stack[sp * kWave];
    const float4 n0 = mv.bvh[2u * node];
    const float4 n1 = mv.bvh[2u * node + 1u];
    const uint32_t first = __float_as_uint(n0.w);
    const uint32_t count = __float_as_uint(n1.w);
    if (count != 0u) {
      const uint32_t i0 = mv.indices[first], i1 = mv.indices[first + 1u], i2 = mv.indices[first + 2u];
      const f3 p0 = xform_point(obj->m, ld3(mv.positions + 3u * (size_t)i0));
      const f3 p1 = xform_point(obj->m, ld3(mv.positions + 3u * (size_t)i1));
      const f3 p2 = xform_point(obj->m, ld3(mv.positions + 3u * (size_t)i2));
      if (kCount) ++tally.tris;
      if (ray_triangle<kAttr>(ray, p0, p1, p2, rec, at)) {
        hit = true;
        ray.tmax = rec.t;
        if constexpr (kAttr) at->first = first;
      }
    } else if ((kCount ? (void)(++tally.boxes, ++tally.nodes) : (void)0), ray_aabb(oo, od, xyz(n0), xyz(n1))) {
      if (sp + 2 > stack_cap) {
        flags |= kFlagStackOverflow;
      } else {
        stack[sp * kWave] = first + 1u;
        stack[(sp + 1) * kWave] = first;
        sp += 2;
      }
    }
  }
  return hit;
}

// ray_scene_intersection_test + ray_object_intersection_test, path_tracer.cu:78-128
// kAttr: a hit also leaves the winner in *at -- its object (the later object wins a tie), HitAttr::first = kNoChild for a sphere.
template <bool kCount, bool kAttr = false>
__device__ __forceinline__ bool ray_scene(Ray ray, const DScene& sc, Hit& rec, uint32_t* stack, uint32_t& flags,
                                          Tally& tally, HitAttr* at = nullptr)
{
  bool hit = false;
  for (uint32_t i = 0; i < sc.object_count; ++i) {
    const DObject* obj = sc.objects + i;
    if (!ray_aabb(ray.o, ray.d, ld3(obj->bmin), ld3(obj->bmax))) continue;
    bool h = false;
    if (obj->type == 0u) {
      Ray tr;
      inverse_transform_ray(obj->inv_m, ray, tr.o, tr.d);
      tr.tmin = ray.tmin;
      tr.tmax = ray.tmax;
      const float4 sp = sc.spheres[obj->index];
      h = ray_sphere(tr, xyz(sp), sp.w, rec);
      if (h) {
        rec.p = xform_point(obj->m, rec.p);
        rec.t = length(rec.p - ray.o);
        rec.n = xform_normal(obj->inv_m, rec.n);
        if constexpr (kAttr) at->first = kNoChild;
      }
    } else {
      h = ray_mesh<kCount, kAttr>(ray, sc.mesh_views[sc.object_mesh[i]], obj, rec, stack, flags, tally, kStackDepth, at);
    }
    if (h) {
      hit = true;
      rec.mat = sc.object_material[i];
      ray.tmax = rec.t;
      if constexpr (kAttr) at->object = i;
    }
  }
  return hit;
}

// ------------------------------------------------------------------------------------------------
// fast closest hit: same result as ray_mesh / ray_scene above, different schedule
// ------------------------------------------------------------------------------------------------
// What the reference computes for one mesh object (path_tracer.cu:36-76) is, independent of visiting order:
// among the triangles whose inner ancestors ALL pass ray_aabb (exact divisions, object-space ray), the one
// with the smallest accepted t; equal t -> the one the depth-first, left-first order reaches last.
// This traversal keeps exactly that result and changes only the schedule:
//   * box decisions are first evaluated with one reciprocal per axis; when the two slab extremes are closer
//     than the rounding error of that shortcut (or anything is non-finite) the exact, division-based test
//     of the reference decides, so every inner-box decision equals the reference's;
//   * triangles are stored in depth-first leaf order, so "reached last" = larger index (tie rule);
//   * subtrees are skipped only when their box lies, with a safety margin, beyond the closest hit found
//     so far or behind the ray origin (such triangles cannot be accepted), and leaves whose own box is
//     missed with a margin are skipped (the reference tests no leaf boxes; those tests would fail);
//   * children are visited nearest first; one LDS stack slot per level.
constexpr int kWideStack = kStackDepth;  // one entry per level of the two-wide tree (ptc_upload_scene checks the depth)

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < __builtin_inff(); }

__device__ __forceinline__ void slab_fast(const f3 bmin, const f3 bmax, const f3 oo, const f3 inv, float& t_near,
                                          float& t_far)
{
  const float ax = (bmin.x - oo.x) * inv.x, bx = (bmax.x - oo.x) * inv.x;
  const float ay = (bmin.y - oo.y) * inv.y, by = (bmax.y - oo.y) * inv.y;
  const float az = (bmin.z - oo.z) * inv.z, bz = (bmax.z - oo.z) * inv.z;
  t_near = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
  t_far = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
}

// Slab interval of a box FOR CULLING ONLY (never for a decision the reference takes), valid also when a direction
// component is zero or so small that its reciprocal is not finite.  On such an axis the ray keeps its coordinate:
// the interval is everything when the origin lies within the box's extent (boundary included, plus a margin far
// beyond rounding: a triangle test can accept a ray that runs along the box face) and nothing otherwise.  The
// products of slab_fast are 0 * inf = NaN exactly in the case that matters -- origin on a box plane -- and fminf /
// fmaxf then pick the other operand, which moved such a box to t = +inf: rays through mesh vertices, along
// triangle edges or down a box face lost their hit (found by the adversarial rays of
// tests/test_gpu_schedules.py::test_benchmark_size_rays_against_oracle).
__device__ __forceinline__ void slab_cull(const f3 bmin, const f3 bmax, const f3 oo, const f3 inv, float& t_near, float& t_far)
{
  const float kInf = __builtin_inff();
  auto axis = [&](float lo_b, float hi_b, float o, float r, float& lo, float& hi) {
    if (finite_f(r)) {
      const float x = (lo_b - o) * r, y = (hi_b - o) * r;
      lo = fminf(x, y);
      hi = fmaxf(x, y);
    } else {
      const float m = 1e-4f * (fabsf(lo_b) + fabsf(hi_b) + fabsf(o)) + 1e-30f;
      const bool inside = o >= lo_b - m && o <= hi_b + m;
      lo = inside ? -kInf : kInf;
      hi = inside ? kInf : -kInf;
    }
  };
  float lx, hx, ly, hy, lz, hz;
  axis(bmin.x, bmax.x, oo.x, inv.x, lx, hx);
  axis(bmin.y, bmax.y, oo.y, inv.y, ly, hy);
  axis(bmin.z, bmax.z, oo.z, inv.z, lz, hz);
  t_near = fmaxf(fmaxf(lx, ly), lz);
  t_far = fminf(fminf(hx, hy), hz);
}

// the reference's test (ray_aabb) that also hands back its two extremes
__device__ __forceinline__ bool slab_exact(const f3 bmin, const f3 bmax, const f3 o, const f3 d, float& t_near,
                                           float& t_far)
{
  const f3 t0 = (bmin - o) / d;
  const f3 t1 = (bmax - o) / d;
  const f3 rmin = min3(t0, t1);
  const f3 rmax = max3(t0, t1);
  t_far = sel_min(sel_min(rmax.x, rmax.y), rmax.z);
  t_near = sel_max(sel_max(rmin.x, rmin.y), rmin.z);
  return t_far >= t_near;
}

// Decision of an INNER node's box, equal to the reference's.  The shortcut's extremes differ from the exact
// ones by at most ~3 ulp each (one rounding of 1/d, one of the product, against one of the quotient).
__device__ __forceinline__ bool box_pass_inner(const f3 bmin, const f3 bmax, const f3 oo, const f3 od, const f3 inv,
                                               const bool exact_only, float& t_near, float& t_far)
{
  if (!exact_only) {
    slab_fast(bmin, bmax, oo, inv, t_near, t_far);
    const float gap = t_far - t_near;
    const float tol = 4e-7f * (fabsf(t_far) + fabsf(t_near)) + 1e-30f;
    if (gap > tol) return true;
    if (gap < -tol) return false;
  }
  return slab_exact(bmin, bmax, oo, od, t_near, t_far);
}

// May this child be skipped although its box test passed?  limit = |M^-1 d| * (closest t so far): the same
// distance measured along the object-space ray; pad_t = how far the world-space rounding of the reference's triangles
// (world_rounding_pad) can move a hit along it.  NaN compares false -> never skipped.
__device__ __forceinline__ bool box_culled(const float t_near, const float t_far, const float limit, const float pad_t)
{
  return (t_near - pad_t > limit * 1.001f + 1e-3f * (t_far - t_near)) || (t_far + pad_t < -1e-3f * fabsf(t_near));
}

// kAny: the any-hit form (scene_occluded below).  The limit stays at scale * best_t (the caller's t_max) for the whole walk, a
// triangle is accepted for !(t < t_min) && !(t > t_max), and the first accepted triangle ends the walk: best_k names it,
// best_t is left alone.
template <bool kCount, bool kAny = false>
__device__ __forceinline__ void mesh_closest_wide(const Ray& ray, const DScene& sc, const DMeshView& mv, const DObject* obj,
                                                  const uint32_t tri_base, float& best_t, int& best_k, uint32_t* stack,
                                                  uint32_t& flags, Tally& tally)
{
  if (mv.bvh_node_count == 0u) return;
  // inverse_transform_ray (transform.hpp:51-58); scale = length before the re-normalisation
  const f3 v = xform_vector(obj->inv_m, ray.d);
  const float scale = ieee_sqrt(dot(v, v));
  const f3 od = v * (1.0f / scale);
  const f3 oo = xform_point(obj->inv_m, ray.o);
  const f3 inv = mk3(1.0f / od.x, 1.0f / od.y, 1.0f / od.z);
  const bool exact_only = !(finite_f(inv.x) && finite_f(inv.y) && finite_f(inv.z));
  float limit = scale * best_t;
  const float ext = fmaxf(fmaxf(fmaxf(fabsf(mv.root_min[0]), fabsf(mv.root_max[0])), fmaxf(fabsf(mv.root_min[1]), fabsf(mv.root_max[1]))),
                          fmaxf(fabsf(mv.root_min[2]), fabsf(mv.root_max[2])));
  const float pad_t = world_rounding_pad(obj, ray.o, ext) * fmaxf(fmaxf(fabsf(inv.x), fabsf(inv.y)), fabsf(inv.z));

  uint32_t cur = mv.root_ref;
  if (!(cur & kLeafBit)) {
    float tn, tf;
    if (kCount) ++tally.boxes;
    if (!box_pass_inner(ld3(mv.root_min), ld3(mv.root_max), oo, od, inv, exact_only, tn, tf)) return;
    if (exact_only) slab_cull(ld3(mv.root_min), ld3(mv.root_max), oo, inv, tn, tf);
    if (box_culled(tn, tf, limit, pad_t)) return;
  }
  const float4* tris = sc.tris + kTriVec4 * (size_t)tri_base;
  int sp = 0;
  for (;;) {
    if (cur & kLeafBit) {
      // ray_triangle_intersection_test (intersections.cuh:49-85) on the precomputed world-space edges
      const uint32_t k = cur & ~kLeafBit;
      const float4 ta = tris[kTriVec4 * k], tb = tris[kTriVec4 * k + 1u], tc = tris[kTriVec4 * k + 2u];
      if (kCount) ++tally.tris;
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
            if (kAny) {
              if (!(t < ray.tmin) && !(t > best_t)) {
                best_k = (int)k;
                return;
              }
            } else if (!(t < ray.tmin) && (t < best_t || (t == best_t && (int)k > best_k))) {
              best_t = t;
              best_k = (int)k;
              limit = scale * t;
            }
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
    if (kCount) { tally.boxes += 2u; ++tally.nodes; }
    // Both children through the same code.  An inner child's decision must equal the reference's: the
    // shortcut decides unless the slab extremes are closer than its rounding error (then: exact test).
    // A leaf child's box is not part of the reference's decision: its triangle is skipped only when the ray misses
    // the box by a margin far beyond rounding IN SPACE -- the box is grown by 1e-5 of its coordinates (~100 ulp)
    // before the test.  (A margin relative to t does not do: 1/d magnifies one ulp of distance from the box to
    // any t when a direction component is tiny, while the triangle test's own tolerance is relative to the
    // coordinates; found with direction components of 1e-30.)
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
        // a direction component without a finite reciprocal: decisions as above (inner: the reference's own test;
        // leaf: visit), culling bounds from the form that is safe for such rays
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
}

// ray_scene_intersection_test with the fast mesh traversal.  Spheres and the per-object world-box test
// are the reference's code; a mesh winner's normal / side / point are filled in once at the end.
template <bool kCount>
__device__ __forceinline__ bool ray_scene_wide(Ray ray, const DScene& sc, Hit& rec, uint32_t* stack, uint32_t& flags,
                                               Tally& tally)
{
  bool hit = false;
  int win_tri = -1;
  for (uint32_t i = 0; i < sc.object_count; ++i) {
    const DObject* obj = sc.objects + i;
    if (!ray_aabb(ray.o, ray.d, ld3(obj->bmin), ld3(obj->bmax))) continue;
    if (obj->type == 0u) {
      Ray tr;
      inverse_transform_ray(obj->inv_m, ray, tr.o, tr.d);
      tr.tmin = ray.tmin;
      tr.tmax = ray.tmax;
      const float4 sp = sc.spheres[obj->index];
      if (ray_sphere(tr, xyz(sp), sp.w, rec)) {
        rec.p = xform_point(obj->m, rec.p);
        rec.t = length(rec.p - ray.o);
        rec.n = xform_normal(obj->inv_m, rec.n);
        rec.mat = sc.object_material[i];
        ray.tmax = rec.t;
        hit = true;
        win_tri = -1;
      }
    } else {
      float t = ray.tmax;
      int k = -1;
      const uint32_t base = sc.object_tri_base[i];
      mesh_closest_wide<kCount>(ray, sc, sc.mesh_views[sc.object_mesh[i]], obj, base, t, k, stack, flags, tally);
      if (k >= 0) {
        ray.tmax = t;
        rec.t = t;
        rec.mat = sc.object_material[i];
        hit = true;
        win_tri = (int)(base + (uint32_t)k);
      }
    }
  }
  if (win_tri >= 0) {
    const float4 tc = sc.tris[kTriVec4 * (size_t)win_tri + 2u];
    const f3 outward = mk3(tc.y, tc.z, tc.w);
    rec.p = ray_at(ray, rec.t);
    rec.side = dot(ray.d, outward) < 0.0f ? 0u : 1u;
    rec.n = rec.side == 0u ? outward : -outward;
  }
  return hit;
}

// occluded(ray) := the reference's ray_scene_intersection_test (path_tracer.cu:110-128) reports a hit (DESIGN section 5e).
// Objects in list order, each one from the caller's t_max (the OR-over-groups argument: every object is a group of its own):
// the world box by ray_aabb first, a sphere in object space against the world-space t_max, a mesh by mesh_closest_wide's any-hit
// form.  The first object that reports a hit ends the walk.  The closest-hit form started at best_t = t_max, best_k = -1 accepts
// the same set of triangles (t < best_t, or t == best_t and k > -1) and culls MORE (its limit shrinks), so "the any-hit walk names
// a triangle" == "the closest-hit walk finds one" == the reference's answer for the object (section 5e: no order appears in it).
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
    } else {
      float t = ray.tmax;
      int k = -1;
      Tally tally;
      mesh_closest_wide<false, true>(ray, sc, sc.mesh_views[sc.object_mesh[i]], obj, sc.object_tri_base[i], t, k, stack, flags, tally);
      if (k >= 0) return true;
    }
  }
  return false;
}

// ------------------------------------------------------------------------------------------------
// shading (path_tracer.cu:29-34, 130-201; distributions.cuh:6-19)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ f3 background(const f3 dir)
{
  const f3 u = normalize(dir);
  const float t = 0.5f * (u.y + 1.0f);
  return mk3(0.5f, 0.7f, 1.0f) * (1.0f - t) + mk3(1.0f, 1.0f, 1.0f) * t;  // glm::lerp = x*(1-a) + y*a
}

// What a path that leaves the scene in direction `dir` (not normalised) sees.  Without kEnv: background(), and `env` is not read --
// the instances are what they were.  kEnv (ptc_set_environment, an extension; DESIGN section 5j): the context's octahedral map,
// env_rules::lookup (pt_env.hpp) -- four 16-byte loads issued together, two lerps per component, nothing normalised.
template <bool kEnv>
__device__ __forceinline__ f3 sky(const f3 dir, const DEnv env)
{
  if constexpr (kEnv) {
    f3 v;
    env_rules::lookup(env.texels, env.n, dir.x, dir.y, dir.z, v.x, v.y, v.z);
    return v;
  } else {
    return background(dir);
  }
}

__device__ __forceinline__ f3 random_on_unit_sphere(Minstd& rng)
{
  const float phi = 2.f * 3.14159265358979323846264338327950288f * rng.uniform();
  const float cos_theta = 2.f * rng.uniform() - 1.f;
  const float sin_theta = ieee_sqrt(1.0f - cos_theta * cos_theta);
  float s, c;
  det_sincos(phi, s, c);
  return mk3(c * sin_theta, s * sin_theta, cos_theta);
}

__device__ __forceinline__ float schlick(float cosine, float ref_idx)
{
  float r0 = (1.0f - ref_idx) / (1.0f + ref_idx);
  r0 = r0 * r0;
  const float x = 1.0f - cosine;
  const float x2 = x * x;
  const float x4 = x2 * x2;
  return r0 + (1.0f - r0) * (x4 * x);
}

// Emissive material (ptc_material type 3, an extension: the reference has no emitters).  A path whose closest hit is an
// emitter ends there with throughput * emission, written as the miss's throughput * sky; no draw is made for it.
__device__ __forceinline__ bool is_emitter(const DMaterial& m) { return m.type == 3; }
__device__ __forceinline__ f3 emit_color(const f3 color, const DMaterial& m) { return color * mk3(m.p[0], m.p[1], m.p[2]); }

// Russian roulette (ptc_set_param "roulette", an extension; DESIGN section 5h) for a path that would go on: c is the throughput
// that came INTO the bounce (before evaluate_material), index the path's slot (streaming) or pixel (megakernel).  True: the path
// ends here with the sample (0, 0, 0) and makes no material draw.  False: it goes on, c divided by q when q < 1 (the largest
// component becomes exactly 1); q >= 1 draws nothing and divides nothing.  The draw is the roulette stream's alone:
// seed(path_seed(index, iteration) ^ kRouletteSeedXor), discard(bounce), one uniform().  One binary32 operation per line item.
__device__ __forceinline__ bool roulette_ends(f3& c, const uint32_t index, const uint32_t iteration, const uint32_t bounce)
{
  const float q = sel_max(sel_max(c.x, c.y), c.z);
  if (q >= 1.0f) return false;
  Minstd rng;
  rng.seed(path_seed(index, iteration) ^ kRouletteSeedXor);
  rng.discard(bounce);
  const float u = rng.uniform();
  if (!(u < q)) return true;  // (q == 0 as well)
  c = mk3(c.x / q, c.y / q, c.z / q);
  return false;
}

// evaluate_material, path_tracer.cu:138-201.  tmin_flag: ray.t_min is 1e-5 from now on (dielectric).
__device__ __forceinline__ void evaluate_material(f3& ro, f3& rd, bool& tmin_flag, const f3 hp, const f3 hn,
                                                  const uint32_t side, const DMaterial m, Minstd& rng, f3& color)
{
  ro = hp - hn * (1e-4f * sign_of(dot(rd, hn)));
  if (m.type == 0) {
    f3 dir = normalize(hn + random_on_unit_sphere(rng));
    if (fabs((double)dir.x) < 1e-8 && fabs((double)dir.y) < 1e-8 && fabs((double)dir.z) < 1e-8) dir = hn;
    rd = dir;
    color = color * mk3(m.p[0], m.p[1], m.p[2]);
  } else if (m.type == 1) {
    const f3 reflected = rd - (hn * dot(hn, rd)) * 2.0f;
    const f3 dir = reflected + random_on_unit_sphere(rng) * m.p[3];
    rd = dir;
    if (dot(dir, hn) > 0.0f) color = color * mk3(m.p[0], m.p[1], m.p[2]);
    else color = mk3(0.0f, 0.0f, 0.0f);
  } else {
    const float ior = m.p[0];
    const float ratio = side == 0u ? (1.0f / ior) : ior;
    const f3 unit = normalize(rd);
    const float cos_theta = sel_min(dot(-unit, hn), 1.0f);
    const float sin_theta = ieee_sqrt(1.0f - cos_theta * cos_theta);
    const bool cannot_refract = ratio * sin_theta > 1.0f;
    f3 dir;
    if (cannot_refract || schlick(cos_theta, ratio) > rng.uniform()) {
      dir = unit - (hn * dot(hn, unit)) * 2.0f;
    } else {
      const float dv = dot(hn, unit);
      const float k = 1.0f - ratio * ratio * (1.0f - dv * dv);
      dir = (k >= 0.0f) ? (unit * ratio - hn * (ratio * dv + ieee_sqrt(k))) : mk3(0.0f, 0.0f, 0.0f);
    }
    ro = hp;
    rd = dir;
    tmin_flag = true;
  }
}

// evaluate_material + the sky of a miss, for a wavefront whose lanes hold DIFFERENT kinds of work (round 4).  From the
// second bounce on the 64 paths of a wavefront have scattered: in the Cornell-box scenes most wavefronts hold diffuse,
// metal and glass hits and a path that left the box, and a `switch` over the kinds executes its four bodies one after
// the other -- 530 VALU instructions where a diffuse-only wavefront needs 205 (profiles/r04_config2_counters.txt).
// The bodies are made of the same few expensive pieces -- two draws, normalize, sqrt(1 - c^2), the sine / cosine -- on
// different operands.  This form runs every piece ONCE, each lane with the operands of its own kind, in an order that
// every kind can follow:
//     draws (all hits; the second one diffuse and metal)
//     A  unit = normalize(rd)                                   glass, miss
//     B  sin = sqrt(1 - cos^2), cos = 2 u2 - 1 | min(-unit.n, 1)  diffuse, metal | glass
//     .  sine / cosine of phi, the point on the unit sphere     diffuse, metal
//     C  sqrt(|n + r|^2) | sqrt(k)                              diffuse (then 1 / it) | glass that refracts
//     the kinds' own few operations
// A lane executes exactly the operations of its kind's body in evaluate_material / background, on the same operands:
// the same bits (the frames tests compare this kernel with k_shade's plain form and with the oracle).
// kind: 0 diffuse, 1 metal, 2 dielectric (Material::type), 3 miss, 4 emissive (kEmit instances only: material type 3, which
// the caller maps to kKindEmit -- its material's type would read as "miss" here), anything else: nothing to do.  An emissive
// hit makes no draw and touches neither ray nor tmin_flag: the path ends with color * emission (emit_color).
// kEnv (DESIGN section 5j): a miss takes the environment, sky<true>(rd, env), which wants no normalised direction: kind 3 then shares
// nothing with the other kinds but its branch.
constexpr uint32_t kKindMiss = 3u, kKindEmit = 4u, kKindNone = 5u;  // (kKindNone: a path roulette has ended, section 5h)
template <bool kEmit = false, bool kEnv = false>
__device__ __forceinline__ void shade_kinds(const uint32_t kind, f3& ro, f3& rd, bool& tmin_flag, const f3 hp, const f3 hn,
                                            const uint32_t side, const DMaterial m, const uint32_t slot, const uint32_t iteration,
                                            const uint32_t bounce, f3& color, const DEnv env = DEnv{nullptr, 0u, 0u})
{
  float u1 = 0.0f, u2 = 0.0f;
  if (kind <= 2u) {
    Minstd rng;
    rng.seed(path_seed(slot, iteration));  // re-seeded from the global slot index, then discard(bounce) (path_tracer.cu:300-301)
    rng.discard(bounce);
    u1 = rng.uniform();
    if (kind <= 1u) u2 = rng.uniform();
  }
  if (kind <= 1u) ro = hp - hn * (1e-4f * sign_of(dot(rd, hn)));
  f3 unit = rd;
  if (kind == 2u || (!kEnv && kind == 3u)) unit = normalize(rd);
  float cos_theta = 0.0f, sin_theta = 0.0f;
  if (kind <= 2u) {
    cos_theta = kind <= 1u ? 2.f * u2 - 1.f : sel_min(dot(-unit, hn), 1.0f);
    sin_theta = ieee_sqrt(1.0f - cos_theta * cos_theta);
  }
  f3 r = mk3(0.f, 0.f, 0.f);  // random_on_unit_sphere
  if (kind <= 1u) {
    const float phi = 2.f * 3.14159265358979323846264338327950288f * u1;
    float sn, cs;
    det_sincos(phi, sn, cs);
    r = mk3(cs * sin_theta, sn * sin_theta, cos_theta);
  }
  const f3 v = hn + r;  // diffuse
  float root_of = dot(v, v);
  float ratio = 1.0f, dv = 0.0f, k = 0.0f;
  bool reflects = false;
  if (kind == 2u) {
    const float ior = m.p[0];
    ratio = side == 0u ? (1.0f / ior) : ior;
    const bool cannot_refract = ratio * sin_theta > 1.0f;
    reflects = cannot_refract || schlick(cos_theta, ratio) > u1;  // (the draw is the path's first either way)
    dv = dot(hn, unit);
    k = 1.0f - ratio * ratio * (1.0f - dv * dv);
    root_of = k;
  }
  float root = 0.0f;
  if (kind == 0u || (kind == 2u && !reflects)) root = ieee_sqrt(root_of);
  if (kind == 0u) {
    f3 dir = v * (1.0f / root);
    if (fabs((double)dir.x) < 1e-8 && fabs((double)dir.y) < 1e-8 && fabs((double)dir.z) < 1e-8) dir = hn;
    rd = dir;
    color = color * mk3(m.p[0], m.p[1], m.p[2]);
  } else if (kind == 1u) {
    const f3 reflected = rd - (hn * dot(hn, rd)) * 2.0f;
    const f3 dir = reflected + r * m.p[3];
    rd = dir;
    if (dot(dir, hn) > 0.0f) color = color * mk3(m.p[0], m.p[1], m.p[2]);
    else color = mk3(0.0f, 0.0f, 0.0f);
  } else if (kind == 2u) {
    f3 dir;
    if (reflects) dir = unit - (hn * dot(hn, unit)) * 2.0f;
    else dir = (k >= 0.0f) ? (unit * ratio - hn * (ratio * dv + root)) : mk3(0.0f, 0.0f, 0.0f);
    ro = hp;
    rd = dir;
    tmin_flag = true;
  } else if (kind == 3u) {
    if constexpr (kEnv) {
      color = color * sky<true>(rd, env);
    } else {
      const float t = 0.5f * (unit.y + 1.0f);  // background(), path_tracer.cu:29-34
      color = color * (mk3(0.5f, 0.7f, 1.0f) * (1.0f - t) + mk3(1.0f, 1.0f, 1.0f) * t);
    }
  } else if (kEmit && kind == kKindEmit) {
    color = emit_color(color, m);
  }
}

// final_gather, path_tracer.cu:203-219
__device__ __forceinline__ float running_mean(uint32_t iteration, float old_v, float new_v)
{
  const float sc = (float)(iteration + 1u);
  return iteration == 0u ? new_v : (old_v * (sc - 1.0f) + new_v) / sc;
}
__device__ __forceinline__ void accumulate_color(float4* color4, uint32_t local_pixel, uint32_t iteration, f3 c)
{
  float4 old = iteration == 0u ? make_float4(0.f, 0.f, 0.f, 0.f) : ldnt(&color4[local_pixel]);
  old.x = running_mean(iteration, old.x, c.x);
  old.y = running_mean(iteration, old.y, c.y);
  old.z = running_mean(iteration, old.z, c.z);
  old.w = 0.0f;
  stnt(&color4[local_pixel], old);
}
__device__ __forceinline__ void accumulate_nd(float4* nd4, uint32_t local_pixel, uint32_t iteration, f3 n, float depth)
{
  float4 old = iteration == 0u ? make_float4(0.f, 0.f, 0.f, 0.f) : ldnt(&nd4[local_pixel]);
  old.x = running_mean(iteration, old.x, n.x);
  old.y = running_mean(iteration, old.y, n.y);
  old.z = running_mean(iteration, old.z, n.z);
  old.w = running_mean(iteration, old.w, depth);
  stnt(&nd4[local_pixel], old);
}

// generate_ray, ray_gen.cu:34-61 (frame invariants hoisted into DCamera)
__device__ __forceinline__ void generate_ray(const DCamera& cam, float fx, float fy, f3& o, f3& d)
{
  const float u = fx / (float)(cam.width - 1u);
  const float v = ((float)cam.height - fy) / (float)(cam.height - 1u);
  const float dx = cam.llx + cam.vw * u;
  const float dy = cam.lly + cam.vh * v;
  o = cam.origin;
  d = normalize(xform_vector(cam.cam, mk3(dx, dy, -1.0f)));
}

// The primary sample of a pixel (raygen_kernel, ray_gen.cu:11-32; path_tracing_mega_kernel, path_tracer.cu:233-240): the path's
// stream seeded, its first two draws jitter the pixel, the ray through that point with a primary ray's range.  rng is left behind
// the two draws (the megakernel goes on drawing from it).
// kLens (ptc_set_lens with a radius > 0, an extension: the reference's camera is a pinhole; DESIGN section 5i): the thin lens.  The
// path stream and the jitter are the pinhole's; a point on the lens disk comes from a stream of its own, seed(path_seed(pixel,
// iteration) ^ kLensSeedXor), two draws; the ray leaves that point towards the point the pinhole ray has at camera-space depth
// `focus`.  One binary32 operation per line item, in section 5i's order.  Without kLens nothing of it is compiled and `lens` is
// not read: the pinhole instances are what they were.
template <bool kLens = false>
__device__ __forceinline__ void primary_ray(const DCamera& cam, const uint32_t pixel, const uint32_t iteration, Minstd& rng, Ray& ray,
                                            const DLens lens = DLens{0.0f, 0.0f})
{
  const uint32_t x = pixel % cam.width, y = pixel / cam.width;
  rng.seed(path_seed(pixel, iteration));
  const float fx = (float)x + rng.uniform();
  const float fy = (float)y + rng.uniform();
  if constexpr (kLens) {
    const float u = fx / (float)(cam.width - 1u);  // generate_ray's dx, dy
    const float v = ((float)cam.height - fy) / (float)(cam.height - 1u);
    const float dx = cam.llx + cam.vw * u;
    const float dy = cam.lly + cam.vh * v;
    Minstd lens_rng;
    lens_rng.seed(path_seed(pixel, iteration) ^ kLensSeedXor);
    const float u1 = lens_rng.uniform();
    const float u2 = lens_rng.uniform();
    const float rho = lens.radius * ieee_sqrt(u1);
    const float phi = 2.f * 3.14159265358979323846264338327950288f * u2;
    float sn, cs;
    det_sincos(phi, sn, cs);
    const float lx = rho * cs;
    const float ly = rho * sn;
    const float px = dx * lens.focus;  // the point in focus: (px, py, -focus)
    const float py = dy * lens.focus;
    ray.o = xform_point(cam.cam, mk3(lx, ly, 0.0f));
    ray.d = normalize(xform_vector(cam.cam, mk3(px - lx, py - ly, -lens.focus)));
  } else {
    generate_ray(cam, fx, fy, ray.o, ray.d);
  }
  ray.tmin = 1e-4f;
  ray.tmax = FLT_MAX;
}

// A batch kernel's view of ONE frame of the batch (DBatchInfo): the frame's part of every per-slot array, `offset` slots in.
__device__ __forceinline__ void offset_frame(DPaths& p, const size_t offset)
{
  p.o4 += offset;
  p.d4 += offset;
  p.t2 += offset;
}
__device__ __forceinline__ void offset_frame(DHits& h, const size_t offset)
{
  h.tp += offset;
  h.nm += offset;
}
__device__ __forceinline__ void offset_frame(DFrame& f, const size_t offset)
{
  f.color4 += offset;
  f.nd4 += offset;
}

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// "filter_rays": may this ray hit one of the mesh objects [filt_begin, filt_end) of the traversal launch that follows?
// No, if it SURELY misses the world boxes of all of them (the same test with the same margin by which that launch skips
// an instance, traverse4m_walk::begin_object) or every box starts beyond the closest hit so far (tmax; a mesh hit needs
// t <= t_max).  A degenerate direction is the traversal launch's business (yes).
__device__ __forceinline__ bool may_hit_boxes(const DObject* objects, uint32_t filt_begin, uint32_t filt_end, const f3 o, const f3 d,
                                              const float tmax)
{
  const f3 winv = mk3(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
  bool may_hit = !finite_f(winv.x + winv.y + winv.z);
  for (uint32_t i = filt_begin; i < filt_end && !may_hit; ++i) {
    const DObject* ob = objects + i;
    const f3 a0 = (ld3(ob->bmin) - o) * winv, a1 = (ld3(ob->bmax) - o) * winv;
    const float wn = fmaxf(fmaxf(fminf(a0.x, a1.x), fminf(a0.y, a1.y)), fminf(a0.z, a1.z));
    const float wf = fminf(fminf(fmaxf(a0.x, a1.x), fmaxf(a0.y, a1.y)), fmaxf(a0.z, a1.z));
    const bool surely_missed = finite_f(wn) && finite_f(wf) && (wn - wf) > 4e-6f * (fabsf(wf) + fabsf(wn));
    // (with the margin of the reciprocals, and only for a box in front of the origin)
    const bool beyond = finite_f(wn) && wn > 0.0f && wn * (1.0f - 8e-6f) > tmax;
    may_hit = !(surely_missed || beyond);
  }
  return may_hit;
}
// ... and the rays go on the launch's work list (batch-global slots, DeviceCounters::list_count per frame) IN SLOT ORDER.
// The order does not matter for the results (they are written per slot) but it decides what the traversal launch costs:
// its wavefronts take the list in batches from cursors that move through it, so at any moment an XCD works on
// neighbouring list entries.  With the entries in slot order those are neighbouring pixels and the part of the tree
// they walk stays in the XCD's L2; with workgroups appending in the order they happened to finish (one atomicAdd each,
// tried first) the fabric reads of bounce 0's launch were 13.6 GB per 20 frames instead of 2.1 GB (L2 hit rate 0.54
// instead of 0.89; profiles/r03_worklist_order.txt).
// So a workgroup's place in the list is the exclusive prefix of the counts of the workgroups before it, by the
// decoupled look-back of k_shade_fused on the same descriptors (a launch of its own epoch) -- and for the same reason as
// there a workgroup's tile is its TICKET, not its block index (list_tile).  A workgroup of 256 threads lists up to
// kListPer x 256 slots (thread t: slots tile_first + j * 256 + t, bit j of may_mask); the last tile writes the frame's
// total.  Every thread of the workgroup must call this.
constexpr int kListPer = 4;
// slots per thread of a tile of the kernel that ends a bounce (pt_shade_tile.inc) and the tile sizes that follow from it
#ifndef PT_FUSE_K
#define PT_FUSE_K 2
#endif
constexpr int kFuseK = PT_FUSE_K;
constexpr uint32_t kFuseTile = 256u * kFuseK;      // k_shade_fused: a 256-thread workgroup's tile
constexpr uint32_t kServiceTile = 64u * kFuseK;    // k_persist: a service wavefront's tile
struct DTileScan {
  unsigned long long* desc;  // this frame's descriptors
  uint32_t epoch;
};
__device__ __forceinline__ uint32_t tile_lookback(const unsigned long long* desc, uint32_t tile, uint32_t epoch, uint32_t* flags);
constexpr unsigned long long kDescAggregate = 1ull << 32, kDescPrefix = 2ull << 32;

// the tile of this workgroup: tickets of the frame's counter, handed out in the order the workgroups start.  Exactly
// `tiles` workgroups of the frame call this (the others have left, see k_shade_fused).
__device__ __forceinline__ uint32_t list_tile(DeviceCounters* counters, uint32_t tiles)
{
  __shared__ uint32_t s_list_tile;
  if (threadIdx.x == 0u) {
    const uint32_t t = __hip_atomic_fetch_add(&counters->shade_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every tile of the frame is taken once the last ticket is out: the next launch starts from zero
    if (t + 1u == tiles) __hip_atomic_store(&counters->shade_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_list_tile = t;
  }
  __syncthreads();
  return s_list_tile;
}

__device__ __forceinline__ void list_rays(uint32_t may_mask, uint32_t* worklist, DeviceCounters* counters, size_t frame_base,
                                          uint32_t tile, uint32_t tiles, const DTileScan& scan)
{
  __shared__ uint32_t s_list_cnt[kListPer * 4];
  __shared__ uint32_t s_list_base;
  const uint32_t wave = threadIdx.x >> 6;
  uint32_t rank[kListPer];
#pragma unroll
  for (int j = 0; j < kListPer; ++j) {
    const uint64_t m = __ballot((may_mask >> j & 1u) != 0u);
    rank[j] = rank_below(m);
    if ((threadIdx.x & 63u) == 0u) s_list_cnt[j * 4 + (int)wave] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (wave == 0u) {
    uint32_t agg = 0u;
#pragma unroll
    for (int k = 0; k < kListPer * 4; ++k) agg += s_list_cnt[k];
    const unsigned long long tag = (unsigned long long)scan.epoch << 34;
    if (threadIdx.x == 0u)
      __hip_atomic_store(&scan.desc[tile], tag | (tile == 0u ? kDescPrefix : kDescAggregate) | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t excl = 0u;
    if (tile != 0u) {
      excl = tile_lookback(scan.desc, tile, scan.epoch, &counters->flags);
      if (threadIdx.x == 0u)
        __hip_atomic_store(&scan.desc[tile], tag | kDescPrefix | (excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0u) {
      s_list_base = excl;
      if (tile + 1u == tiles) counters->list_count = excl + agg;
    }
  }
  __syncthreads();
  uint32_t at = s_list_base;
  const uint32_t tile_first = tile * (256u * (uint32_t)kListPer);
#pragma unroll
  for (int j = 0; j < kListPer; ++j) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t c = s_list_cnt[j * 4 + w];
      if ((uint32_t)w == wave && (may_mask >> j & 1u))
        worklist[frame_base + at + rank[j]] = (uint32_t)frame_base + tile_first + (uint32_t)j * 256u + threadIdx.x;
      at += c;
    }
  }
}

__device__ __forceinline__ Ray load_ray(const DPaths& paths, uint32_t s)
{
  const float4 o = ldnt(&paths.o4[s]);
  const float4 d = ldnt(&paths.d4[s]);
  Ray r;
  r.o = xyz(o);
  r.d = xyz(d);
  r.tmin = (__float_as_uint(o.w) >> 31) ? 1e-5f : 1e-4f;
  r.tmax = FLT_MAX;
  return r;
}

// ... and the first throughput component, which rides in the direction's fourth word (DPaths): one load of d4 for both
__device__ __forceinline__ Ray load_ray(const DPaths& paths, uint32_t s, float& through_x)
{
  const float4 o = ldnt(&paths.o4[s]);
  const float4 d = ldnt(&paths.d4[s]);
  Ray r;
  r.o = xyz(o);
  r.d = xyz(d);
  r.tmin = (__float_as_uint(o.w) >> 31) ? 1e-5f : 1e-4f;
  r.tmax = FLT_MAX;
  through_x = d.w;
  return r;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, kWave);
  return v;
}

// exclusive prefix of `tile` (survivors of tiles [0, tile)), by the calling wavefront; every lane returns it
__device__ __forceinline__ uint32_t tile_lookback(const unsigned long long* desc, uint32_t tile, uint32_t epoch, uint32_t* flags)
{
  uint32_t excl = 0u;
  const int lane = (int)lane_id();
  int pos = (int)tile - 1;
  uint32_t spins = 0u;
  while (pos >= 0) {
    const int idx = pos - lane;  // lane 0 = the nearest predecessor
    for (;;) {
      unsigned long long d = 0ull;
      if (idx >= 0) d = __hip_atomic_load(&desc[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool valid = idx >= 0;
      const bool ready = !valid || (uint32_t)(d >> 34) == epoch;
      const bool is_prefix = valid && ready && (d & kDescPrefix) != 0ull;
      const uint64_t rdy = __ballot(ready), pm = __ballot(is_prefix);
      if (pm != 0ull) {
        const int p = __ffsll((unsigned long long)pm) - 1;  // nearest predecessor that knows its inclusive prefix
        const uint64_t need = (p == 63) ? ~0ull : ((1ull << (p + 1)) - 1ull);
        if ((rdy & need) == need) return excl + wave_sum(lane <= p ? (uint32_t)d : 0u);
      } else if (rdy == ~0ull) {
        excl += wave_sum(valid ? (uint32_t)d : 0u);
        break;  // 64 aggregates and no prefix among them: look further back
      }
      __builtin_amdgcn_s_sleep(2);
      if (++spins > (1u << 20)) {  // (about a second) a predecessor that never ran: see the kernel's header
        if (lane == 0) atomicOr(flags, kFlagDispatchOrder);
        return excl;
      }
    }
    pos -= kWave;
  }
  return excl;
}

// ------------------------------------------------------------------------------------------------
// sphere segments
// ------------------------------------------------------------------------------------------------
#ifndef PT_SPHERE_SKIP
#define PT_SPHERE_SKIP 0
#endif
#ifndef PT_SPHERE_LANES
#define PT_SPHERE_LANES 1
#endif
#ifndef PT_SHADE_KINDS
#define PT_SHADE_KINDS 1
#endif
#ifndef PT_FOLD_TAIL
#define PT_FOLD_TAIL 0
#endif
#ifndef PT_SPHERE_LANES_LEADING
#define PT_SPHERE_LANES_LEADING 0
#endif
// Sphere objects [obj_begin, obj_end) in the reference's order (ray_object_intersection_test, path_tracer.cu:78-100)
// for one ray whose closest hit so far is ray.tmax (FLT_MAX: none).  A sphere that is hit replaces `rec`, shrinks
// ray.tmax and sets `changed`.  Used by k_spheres (a run in front of a mesh, a scene without a mesh) and by
// the kernel that ends the bounce (k_shade_fused / k_tail_count: the run behind the last mesh).
// transform_point (transform.hpp:37-42) divides by w.  For an affine matrix w is exactly 1 whatever the (finite) point --
// (0 x + 0 y) + (0 z + 1) -- and x / 1 is x: when every lane of the wavefront has w == 1 the three IEEE divisions (ten
// instructions each) are skipped; the result has the same bits.  Any lane with another w (a projective matrix, a
// non-finite coordinate) sends the wavefront through the divisions.
__device__ __forceinline__ f3 xform_point_w1(const m4& m, f3 p)
{
  const f4 v = mul(m, p.x, p.y, p.z, 1.0f);
  if (__builtin_expect(__ballot(v.w != 1.0f) == 0ull, 1)) return mk3(v.x, v.y, v.z);
  return mk3(v.x, v.y, v.z) / v.w;
}

// kShareDir (k_spheres only: it has the registers to spare; in k_shade_fused the three extra live values cost more than
// they save, profiles/r03_sphere_math.txt): inverse_transform_ray's direction, normalize(M^-1 (d, 0)), is the same for
// every object whose M^-1 has the identity as its upper 3 x 3 (a translated sphere: every sphere of the Cornell box) --
// (1 dx + 0 dy) + (0 dz + t 0) is dx exactly when the components of d are finite and none is a zero (whose sign the sum
// could change) -- so such a wavefront normalises its direction once for all of them.
// Select approximately, verify exactly (round 4): before the reference's own sequence for a sphere object -- world box
// with six divisions, inverse transform with a normalisation, the quadratic with an IEEE square root and two divisions
// (path_tracer.cu:84-96, intersections.cuh:7-41) -- a dozen approximate operations on the WORLD-space ball around the
// object (DScene::sphere_ball) decide whether that sequence can possibly accept a hit.  true = it surely cannot:
//   * the ray's line passes the ball at more than its radius (the reference's discriminant would be negative), or
//   * the ball lies behind the origin (both roots negative: below t_min), or
//   * the ball starts beyond the closest hit so far: the reference compares the OBJECT-space root with the world-space
//     t_max (transform.hpp:51-58 copies the range unscaled), and an object-space distance is at least the world-space
//     one divided by the matrix's largest stretch.
// Everything is held against the ray with margins far beyond the rounding of either side (relative 1e-4 where the
// arithmetic is good to 1e-6), so a sphere the reference would accept is never skipped; what is not skipped takes the
// reference's sequence unchanged, in list order -- ties, the unscaled-t quirk and the box test included.
__device__ __forceinline__ bool sphere_surely_missed(const float4 ball, const float inv_stretch, const f3 o, const f3 d, const float a,
                                                     const float tmax)
{
  const float R = ball.w;
  const f3 oc = mk3(o.x - ball.x, o.y - ball.y, o.z - ball.z);
  const float oc2 = __builtin_fmaf(oc.x, oc.x, __builtin_fmaf(oc.y, oc.y, oc.z * oc.z));
  const float b = __builtin_fmaf(d.x, oc.x, __builtin_fmaf(d.y, oc.y, d.z * oc.z));  // d . oc (d not normalised)
  const float r2 = R * R;
  const float cc = oc2 - r2;                       // > 0: the origin is outside the ball
  const float scale2 = a * (oc2 + r2);             // the size of the terms the discriminant is made of
  const float disc = __builtin_fmaf(b, b, -(a * cc));
  const float margin = 1e-4f * __builtin_fmaf(b, b, scale2);
  const bool no_ball = !(R >= 0.0f) || !(margin < __builtin_inff());  // no ball for this object, or nothing can be said
  const bool line_misses = disc < -margin;
  const bool outside = cc > 1e-4f * (oc2 + r2);
  const bool behind = outside && b > 0.0f && b * b > 1e-8f * scale2;
  // distance (world units) to the ball along the ray, from below; an object-space root is at least that / stretch
  const float inv_len = __builtin_amdgcn_rsqf(a);
  const float bh = b * inv_len;
  const float dd = __builtin_fmaf(bh, bh, -cc);
  const float entry = -bh - __builtin_amdgcn_sqrtf(fmaxf(dd, 0.0f));  // (v_sqrt_f32, 1 ulp: margins below)
  const float lower = (entry - 1e-4f * (fabsf(bh) + R)) * inv_stretch * 0.9999f;
  const bool beyond = outside && dd > 0.0f && lower > tmax;
  return !no_ball && (line_misses || behind || beyond);
}

template <bool kShareDir = false>
__device__ __forceinline__ void sphere_segment(const DScene& sc, uint32_t obj_begin, uint32_t obj_end, Ray& ray, Hit& rec,
                                               bool& changed)
{
  const float ray_a = __builtin_fmaf(ray.d.x, ray.d.x, __builtin_fmaf(ray.d.y, ray.d.y, ray.d.z * ray.d.z));
  // 1/d by the hardware reciprocal: decides the world-box test of almost every ray without the reference's six
  // divisions per object (below)
  const f3 winv = mk3(__builtin_amdgcn_rcpf(ray.d.x), __builtin_amdgcn_rcpf(ray.d.y), __builtin_amdgcn_rcpf(ray.d.z));
  const bool winv_ok = finite_f(winv.x + winv.y + winv.z);
  const bool d_plain = kShareDir && finite_f(ray.d.x + ray.d.y + ray.d.z) && ray.d.x != 0.0f && ray.d.y != 0.0f && ray.d.z != 0.0f;
  bool have_nd = false;
  f3 nd = mk3(0.f, 0.f, 0.f);
  float nd_a = 0.0f;
  for (uint32_t i = obj_begin; i < obj_end; ++i) {
    const DObject* obj = sc.objects + i;
    if (obj->type != 0u) continue;
    if (PT_SPHERE_SKIP) {
      // (wave-uniform loads; the sequence below runs only when some lane of the wavefront cannot be ruled out)
      const float4 ball = sc.sphere_ball[(size_t)kSphereTab * i];
      const float inv_stretch = sc.sphere_ball[(size_t)kSphereTab * i + 1u].x;
      if (sphere_surely_missed(ball, inv_stretch, ray.o, ray.d, ray_a, ray.tmax)) continue;
    }
    {
      // ray_aabb_intersection_test (intersections.cuh:87-103) decides by the sign of min(far) - max(near).  With
      // reciprocals each slab value is within 3 ulp of the reference's quotient, so a gap beyond 2e-6 of the two
      // extremes has the reference's sign; only a ray that grazes the box within that margin (or has a zero /
      // non-finite direction component) takes the divisions.
      const f3 bmin = ld3(obj->bmin), bmax = ld3(obj->bmax);
      const f3 a0 = (bmin - ray.o) * winv, a1 = (bmax - ray.o) * winv;
      const float wn = fmaxf(fmaxf(fminf(a0.x, a1.x), fminf(a0.y, a1.y)), fminf(a0.z, a1.z));
      const float wf = fminf(fminf(fmaxf(a0.x, a1.x), fmaxf(a0.y, a1.y)), fmaxf(a0.z, a1.z));
      const float gap = wf - wn, margin = 2e-6f * (fabsf(wf) + fabsf(wn)) + 1e-30f;
      const bool box_ok = !(bmin.x > bmax.x || bmin.y > bmax.y || bmin.z > bmax.z);
      bool pass = gap > margin;
      const bool unsure = !box_ok || !winv_ok || !(gap > margin || gap < -margin);
      if (__builtin_expect(unsure, 0)) pass = ray_aabb(ray.o, ray.d, bmin, bmax);
      if (!pass) continue;
    }
    Ray tr;
    tr.o = xform_point_w1(obj->inv_m, ray.o);  // inverse_transform_ray, transform.hpp:51-58
    const m4& im = obj->inv_m;
    const bool identity3 = kShareDir && im.c[0][0] == 1.0f && im.c[1][1] == 1.0f && im.c[2][2] == 1.0f && im.c[0][1] == 0.0f &&
                           im.c[0][2] == 0.0f && im.c[1][0] == 0.0f && im.c[1][2] == 0.0f && im.c[2][0] == 0.0f &&
                           im.c[2][1] == 0.0f;  // (wave-uniform: scalar loads and compares)
    float a;
    if (kShareDir && identity3 && __ballot(!d_plain) == 0ull) {
      if (!have_nd) {
        nd = normalize(ray.d);
        nd_a = dot(nd, nd);
        have_nd = true;
      }
      tr.d = nd;
      a = nd_a;
    } else {
      tr.d = normalize(xform_vector(obj->inv_m, ray.d));
      a = dot(tr.d, tr.d);
    }
    tr.tmin = ray.tmin;
    tr.tmax = ray.tmax;
    const float4 sp = sc.spheres[obj->index];
    if (ray_sphere_a(tr, a, xyz(sp), sp.w, rec)) {
      rec.p = xform_point_w1(obj->m, rec.p);
      rec.t = length(rec.p - ray.o);
      rec.n = xform_normal(obj->inv_m, rec.n);
      rec.mat = sc.object_material[i];
      ray.tmax = rec.t;
      changed = true;
    }
  }
}
// ---- a run of SIMPLE sphere objects, candidates per lane (round 4) -------------------------------------------------
// ---- a run of translated spheres as a fold with the hit record's normal deferred (round 4; k_spheres) ----
// In front of a mesh the spheres are typically a room's walls: every ray is inside every one of them, every wall is hit,
// and which one wins is decided only by distance -- there is nothing to rule out, so sphere_segment pays the whole
// sequence of path_tracer.cu:84-96 + intersections.cuh:7-41 for every object (226 VALU instructions per ray and sphere
// on the Cornell box's walls, behind four dependent vector loads of the object's data: 1.15 ms per 29.5 M rays at 39 % of the VALU
// issue rate and 1.8 TB/s -- bound by neither, by its chains of dependent operations; profiles/r04_config2_counters.txt).  When every
// object of the run is "simple" (DScene::fold_run: both matrices pure translations, 3 x 3 part 1.0f / +-0.0f) the same
// operations on the same operands come much cheaper:
//   * transform_point's row (1 x + e y) + (e' z + t 1), e, e' zeros of either sign, IS x + t: the products with the
//     zeros are zeros, they vanish in the sums, one rounding remains -- unless x is -0.0f (with t a zero the zeros'
//     signs then decide the sign of the result; the fold does not look at t), or a coordinate is not finite (0 * inf).
//     w is (0 x + 0 y) + (0 z + 1) = 1 and nothing is divided.  3 instructions instead of 28, for the ray's origin, and
//     again for the hit point.
//   * transform_normal's row (1 nx + e ny) + (e' nz + e'' 0) IS nx, unless nx is -0.0f.
//   * what the NEXT object needs of an accepted hit is its distance (t_max: length(p_world - o)) -- the normal
//     ((p - centre) / radius: three divisions; the side; the transform) is needed of the LAST accepted hit only: the fold
//     keeps p - centre, the radius and the material of the hit it holds, and finishes the record once, behind the loop.
// A lane that meets one of the exceptions (-0.0f where it matters, a non-finite coordinate, a direction with a zero
// component: inverse_transform_ray's normalised direction is then not the same for every object) sends its wavefront
// through sphere_segment with the ray as it came.  Same bits as sphere_segment in every case (tests/test_gpu_spheres.py).
typedef __attribute__((address_space(4))) const float cfloat;
__device__ __forceinline__ bool neg_zero(const float x) { return __float_as_uint(x) == 0x80000000u; }
__device__ __forceinline__ void sphere_fold(const DScene& sc, const uint32_t obj_begin, const uint32_t obj_end, Ray& ray, Hit& rec, bool& changed)
{
  const bool plain = finite_f(ray.d.x + ray.d.y + ray.d.z) && ray.d.x != 0.0f && ray.d.y != 0.0f && ray.d.z != 0.0f &&
                     finite_f(ray.o.x + ray.o.y + ray.o.z) && !neg_zero(ray.o.x) && !neg_zero(ray.o.y) && !neg_zero(ray.o.z);
  if (__builtin_expect(__ballot(!plain) != 0ull, 0)) {
    sphere_segment<true>(sc, obj_begin, obj_end, ray, rec, changed);
    return;
  }
  const float tmax_in = ray.tmax;
  const f3 winv = mk3(__builtin_amdgcn_rcpf(ray.d.x), __builtin_amdgcn_rcpf(ray.d.y), __builtin_amdgcn_rcpf(ray.d.z));
  const bool winv_ok = finite_f(winv.x + winv.y + winv.z);
  const f3 nd = normalize(ray.d);  // inverse_transform_ray's direction, the same for every object of the run
  const float a = dot(nd, nd);
  bool odd = false;
  f3 pc = mk3(0.f, 0.f, 0.f);      // of the hit the fold holds: p - centre (object space), the radius, the material
  float held_r = 1.0f;
  uint32_t held_mat = 0u;
  const bool tmin_pos = ray.tmin > 0.0f;
  for (uint32_t i = obj_begin; i < obj_end; ++i) {
    // what differs between the objects of such a run, from the table the host packed (DScene::sphere_ball rows 2..6),
    // through the constant address space: scalar loads (the object array itself is read with vector loads -- the
    // compiler cannot know that the kernel's stores do not touch it)
    const cfloat* q = (const cfloat*)reinterpret_cast<const float*>(sc.sphere_ball + (size_t)kSphereTab * i + 2u);
    const f3 bmin = mk3(q[0], q[1], q[2]), bmax = mk3(q[4], q[5], q[6]);
    const f3 itr = mk3(q[3], q[7], q[11]);         // the inverse matrix' translation column
    const f3 center = mk3(q[8], q[9], q[10]);
    const f3 ftr = mk3(q[12], q[13], q[14]);       // the matrix' translation column
    const float radius = q[15];
    const uint32_t material = __float_as_uint(q[16]);
    {  // the object's world box (path_tracer.cu:84).  An origin strictly inside the box: every axis has one slab
       // bound behind the origin and one in front of it, whatever the (non-zero) direction -- near < 0 < far, the
       // reference passes; a room's walls are all of this kind, and a wavefront of such rays skips the slab arithmetic
      const bool inside = ray.o.x > bmin.x && ray.o.x < bmax.x && ray.o.y > bmin.y && ray.o.y < bmax.y && ray.o.z > bmin.z && ray.o.z < bmax.z;
      if (__ballot(!inside) != 0ull) {
        // as in sphere_segment
        const f3 a0 = (bmin - ray.o) * winv, a1 = (bmax - ray.o) * winv;
        const float wn = fmaxf(fmaxf(fminf(a0.x, a1.x), fminf(a0.y, a1.y)), fminf(a0.z, a1.z));
        const float wf = fminf(fminf(fmaxf(a0.x, a1.x), fmaxf(a0.y, a1.y)), fmaxf(a0.z, a1.z));
        const float gap = wf - wn, margin = 2e-6f * (fabsf(wf) + fabsf(wn)) + 1e-30f;
        const bool box_ok = !(bmin.x > bmax.x || bmin.y > bmax.y || bmin.z > bmax.z);
        bool pass = gap > margin;
        const bool unsure = !box_ok || !winv_ok || !(gap > margin || gap < -margin);
        if (__builtin_expect(unsure, 0)) pass = ray_aabb(ray.o, ray.d, bmin, bmax);
        if (!pass && !inside) continue;
      }
    }
    Ray tr;
    tr.o = ray.o + itr;
    tr.d = nd;
    // ray_sphere_intersection_test, intersections.cuh:7-41, up to the accepted root
    const f3 oc = tr.o - center;
    const float b = 2.0f * dot(tr.d, oc);
    const float c = dot(oc, oc) - radius * radius;
    const float disc = b * b - 4.0f * a * c;
    if (disc < 0.0f) continue;
    const float sq = ieee_sqrt(disc);
    // t1 = (-b - sq) / (2 a), 2 a > 0: a negative numerator gives a quotient that is negative or -0 and fails
    // t1 >= t_min (> 0) without being divided; a wavefront of rays inside their spheres never divides for t1
    const float n1 = -b - sq;
    const bool t1_out = n1 < 0.0f && tmin_pos && a > 0.0f;
    float t1 = -1.0f;
    if (__ballot(!t1_out) != 0ull) {
      asm volatile("" ::: "memory");  // (keeps the division inside the branch: the compiler would divide and select)
      t1 = n1 / (2.0f * a);
    }
    float t;
    if (!t1_out && t1 >= ray.tmin && t1 <= ray.tmax) {
      t = t1;
    } else {
      const float t2 = (-b + sq) / (2.0f * a);
      if (t2 >= ray.tmin && t2 <= ray.tmax) t = t2;
      else continue;
    }
    const f3 p = ray_at(tr, t);
    pc = p - center;
    held_r = radius;
    held_mat = material;
    rec.p = p + ftr;
    rec.t = length(rec.p - ray.o);
    odd = odd || neg_zero(p.x) || neg_zero(p.y) || neg_zero(p.z) || !finite_f(rec.t);  // (a non-finite p gives a non-finite length)
    ray.tmax = rec.t;
    changed = true;
  }
  if (changed) {
    const f3 outward = pc / held_r;
    rec.side = dot(nd, outward) < 0.0f ? 0u : 1u;
    const f3 n = rec.side == 0u ? outward : -outward;
    odd = odd || !finite_f(n.x + n.y + n.z) || neg_zero(n.x) || neg_zero(n.y) || neg_zero(n.z);
    rec.n = n;
    rec.mat = held_mat;
  }
  if (__builtin_expect(__ballot(odd) != 0ull, 0)) {
    ray.tmax = tmax_in;
    changed = false;
    sphere_segment<true>(sc, obj_begin, obj_end, ray, rec, changed);
  }
}

// sphere_segment walks the run object by object, and the wavefront pays the reference's whole sequence for an object
// whenever ANY lane cannot rule it out -- with 64 lanes that is almost every object: the Cornell box's five wall spheres
// are all "hit" by every ray inside it, and k_spheres ran eight full sequences per ray (645 us a launch, config 2).
// Here every lane first collects ITS candidates, for up to kSlots rays at once (k_shade_fused holds four), with the
// approximate arithmetic of sphere_surely_missed extended to bounds on the root the reference would accept:
//   lo  a lower bound of that root (world distance: a simple object does not stretch),
//   hi  an upper bound of it when the sphere is surely hit beyond t_min (else +inf).
// In list order an object is a candidate unless it is surely missed or lo exceeds `cap`, the smallest hi of the
// surely-hit objects BEFORE it (and the closest hit carried in): when its turn comes the reference's t_max is below its
// root whichever of the earlier objects were accepted, so the reference rejects it too.  (Objects AFTER it never
// matter for it: the reference walks the list in order.)  Then the lanes take their candidates one per iteration, lowest
// list index first and slot by slot, each lane with the data of ITS object (five float4 from DScene::sphere_ball) and
// the reference's operations spelled with the literal matrix entries of a translation -- same operands, same order,
// same bits.  The loop runs as often as the busiest lane has candidates: one to three times where sphere_segment paid
// for eight objects.
// mul(m, x, y, z, w) (pt_math.hpp) with the matrix's translation column taken from `tcol` (per lane), everything else from
// `m` (the run's common entries: wave-uniform)
__device__ __forceinline__ f4 mul_tcol(const m4& m, const f3 tcol, float x, float y, float z, float w)
{
  f4 r;
  r.x = (m.c[0][0] * x + m.c[1][0] * y) + (m.c[2][0] * z + tcol.x * w);
  r.y = (m.c[0][1] * x + m.c[1][1] * y) + (m.c[2][1] * z + tcol.y * w);
  r.z = (m.c[0][2] * x + m.c[1][2] * y) + (m.c[2][2] * z + tcol.z * w);
  r.w = (m.c[0][3] * x + m.c[1][3] * y) + (m.c[2][3] * z + m.c[3][3] * w);
  return r;
}

// The reference's sequence for one sphere object of a simple run (path_tracer.cu:84-96, intersections.cuh:7-41): the same
// operations on the same operands as sphere_segment, with the object's own numbers (q0..q3, see DScene::sphere_ball)
// in vector registers and the entries all objects of the run share in `first` (the run's first object, scalar).
__device__ __forceinline__ bool sphere_exact_simple(const DObject* first, const float4 q0, const float4 q1, const float4 q2, const float4 q3,
                                                    const f3 ro, const f3 rd, const float tmin, const float tmax, Hit& rec)
{
  {
    // the object's world box first (path_tracer.cu:84), as in sphere_segment: reciprocals, the reference's divisions
    // only for a ray that grazes it
    const f3 bmin = xyz(q0), bmax = xyz(q1);
    const f3 winv = mk3(__builtin_amdgcn_rcpf(rd.x), __builtin_amdgcn_rcpf(rd.y), __builtin_amdgcn_rcpf(rd.z));
    const f3 a0 = (bmin - ro) * winv, a1 = (bmax - ro) * winv;
    const float wn = fmaxf(fmaxf(fminf(a0.x, a1.x), fminf(a0.y, a1.y)), fminf(a0.z, a1.z));
    const float wf = fminf(fminf(fmaxf(a0.x, a1.x), fmaxf(a0.y, a1.y)), fmaxf(a0.z, a1.z));
    const float gap = wf - wn, margin = 2e-6f * (fabsf(wf) + fabsf(wn)) + 1e-30f;
    const bool box_ok = !(bmin.x > bmax.x || bmin.y > bmax.y || bmin.z > bmax.z);
    bool pass = gap > margin;
    const bool unsure = !box_ok || !finite_f(winv.x + winv.y + winv.z) || !(gap > margin || gap < -margin);
    if (__builtin_expect(unsure, 0)) pass = ray_aabb(ro, rd, bmin, bmax);
    if (!pass) return false;
  }
  const f3 ti = mk3(q0.w, q1.w, q2.w);
  // inverse_transform_ray (transform.hpp:51-58)
  Ray tr;
  const f4 ov = mul_tcol(first->inv_m, ti, ro.x, ro.y, ro.z, 1.0f);
  tr.o = mk3(ov.x, ov.y, ov.z);
  if (__builtin_expect(ov.w != 1.0f, 0)) tr.o = tr.o / ov.w;  // (x / 1 is x: the division transform_point always makes, skipped)
  const f4 dv = mul_tcol(first->inv_m, ti, rd.x, rd.y, rd.z, 0.0f);
  tr.d = normalize(mk3(dv.x, dv.y, dv.z));
  tr.tmin = tmin;
  tr.tmax = tmax;
  if (!ray_sphere_a(tr, dot(tr.d, tr.d), xyz(q2), q3.w, rec)) return false;
  // path_tracer.cu:92-96: point to world, t = distance, normal by transpose(inv_m)
  const f4 pv = mul_tcol(first->m, xyz(q3), rec.p.x, rec.p.y, rec.p.z, 1.0f);
  rec.p = mk3(pv.x, pv.y, pv.z);
  if (__builtin_expect(pv.w != 1.0f, 0)) rec.p = rec.p / pv.w;
  rec.t = length(rec.p - ro);
  rec.n = xform_normal(first->inv_m, rec.n);  // (no entry of the translation column in it)
  return true;
}

// the candidates of one ray among the objects of the run: bit k = object obj_begin + k.
// Bounds: with oc = origin - centre and u the unit direction, the roots are -u.oc -+ sqrt((u.oc)^2 - (|oc|^2 - r^2)).
// The radicand is a difference of terms up to 1e6 (the Cornell box's walls are spheres of radius 1000): every use of it
// carries m = 1e-5 of those terms (forty times what float arithmetic loses there) on the side that keeps the bound a
// bound -- the reference's own float result lies inside [lo, hi] as well.  The cap is the smallest hi of ALL surely-hit
// objects, not only of the earlier ones: the reference's answer is the closest accepted root (ties: the later object),
// it is at most that cap, and an object whose root lies beyond the cap cannot be the answer nor decide between others
// that could (what it may be accepted for in the reference's walk is overwritten by the object that sets the cap).
// kAllCaps false (k_shade_fused: four rays' worth of state and no registers for eight more bounds): the cap an object is
// held against is the one of the objects before it -- the reference's walk at its plainest, nothing to argue.
template <bool kAllCaps>
__device__ __forceinline__ uint32_t sphere_candidates(const DScene& sc, const uint32_t obj_begin, const uint32_t obj_end, const float4 o4,
                                                      const float4 d4, const float closest)
{
  const f3 o = xyz(o4), d = xyz(d4);
  const float tmin = (__float_as_uint(o4.w) >> 31) ? 1e-5f : 1e-4f;
  const float a = __builtin_fmaf(d.x, d.x, __builtin_fmaf(d.y, d.y, d.z * d.z));
  const float inv_len = __builtin_amdgcn_rsqf(a);
  float cap = closest >= 0.0f ? closest * 1.0001f : FLT_MAX;
  uint32_t cand = 0u;
  float lo_of[kAllCaps ? 8 : 1];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (kAllCaps) lo_of[k] = __builtin_inff();
    const uint32_t i = obj_begin + (uint32_t)k;
    if (i < obj_end) {  // (wave-uniform: the balls come through scalar loads)
      const float4 ball = sc.sphere_ball[(size_t)kSphereTab * i];
      const float R = ball.w;
      const f3 oc = mk3(o.x - ball.x, o.y - ball.y, o.z - ball.z);
      const float oc2 = __builtin_fmaf(oc.x, oc.x, __builtin_fmaf(oc.y, oc.y, oc.z * oc.z));
      const float bh = __builtin_fmaf(d.x, oc.x, __builtin_fmaf(d.y, oc.y, d.z * oc.z)) * inv_len;
      const float r2 = R * R;
      const float dd = __builtin_fmaf(bh, bh, -(oc2 - r2));
      const float m = 1e-5f * (__builtin_fmaf(bh, bh, oc2) + r2);
      // the inner ball (sphere_ball_of): what is hit for sure, and the bounds from the other side
      const float Rin = sc.sphere_ball[(size_t)kSphereTab * i + 1u].z;
      const float dd_in = __builtin_fmaf(bh, bh, -(oc2 - Rin * Rin));
      const float sq_up = __builtin_amdgcn_sqrtf(fmaxf(dd + m, 0.0f)), sq_dn = __builtin_amdgcn_sqrtf(fmaxf(dd_in - m, 0.0f));
      const float e = 1e-5f * (fabsf(bh) + sq_up + R) + 1e-6f;
      const bool near_bad = -bh - sq_dn < tmin - e;   // the nearer root is surely below t_min: only the farther one counts
      const bool near_ok = -bh - sq_up > tmin + e;    // ... surely at or above it: it is the one
      const bool missed = dd < -m || -bh + sq_up < tmin - e;
      const bool sure = dd_in > m && (near_ok || (near_bad && -bh + sq_dn > tmin + e));
      const float lo = near_bad ? -bh + sq_dn - e : -bh - sq_up - e;
      const float hi = near_ok ? -bh - sq_dn + e : -bh + sq_up + e;
      const bool known = m < __builtin_inff();        // (anything non-finite: a candidate, and no bound from it)
      const float lo_k = !known ? -__builtin_inff() : (missed ? __builtin_inff() : lo);
      if (kAllCaps) lo_of[k] = lo_k;
      else cand |= lo_k <= cap ? 1u << k : 0u;
      cap = (known && sure) ? fminf(cap, hi * 1.0001f) : cap;
    }
  }
  if (kAllCaps) {
#pragma unroll
    for (int k = 0; k < 8; ++k) cand |= lo_of[k] <= cap ? 1u << k : 0u;
  }
  return cand;
}

// (component by component: a conditional expression on the float4 STRUCT is compiled as a choice between two addresses
// in scratch memory)
__device__ __forceinline__ float4 sel4(const bool c, const float4 a, const float4 b)
{
  return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// o4 / d4: the rays as the path arrays hold them; tp / nm: the hit records (tp.x < 0: none yet), updated in place.
// valid: bit j = slot j holds a ray.  Returns the slots whose record changed.  (Every array index below is a literal:
// a loop over the slots, even a fully unrolled one, left the arrays in scratch memory.)
template <int kSlots>
__device__ __forceinline__ uint32_t sphere_run_lanes(const DScene& sc, const uint32_t obj_begin, const uint32_t obj_end, const float4 (&o4)[kSlots],
                                                     const float4 (&d4)[kSlots], float4 (&tp)[kSlots], float4 (&nm)[kSlots], const uint32_t valid)
{
  static_assert(kSlots >= 1 && kSlots <= 4, "slots");
  uint32_t cand = 0u;
  constexpr bool kAllCaps = kSlots == 1;
  if (valid & 1u) cand |= sphere_candidates<kAllCaps>(sc, obj_begin, obj_end, o4[0], d4[0], tp[0].x);
  if constexpr (kSlots > 1) { if (valid & 2u) cand |= sphere_candidates<kAllCaps>(sc, obj_begin, obj_end, o4[1], d4[1], tp[1].x) << 8; }
  if constexpr (kSlots > 2) { if (valid & 4u) cand |= sphere_candidates<kAllCaps>(sc, obj_begin, obj_end, o4[2], d4[2], tp[2].x) << 16; }
  if constexpr (kSlots > 3) { if (valid & 8u) cand |= sphere_candidates<kAllCaps>(sc, obj_begin, obj_end, o4[3], d4[3], tp[3].x) << 24; }
  uint32_t changed = 0u;
  while (__ballot(cand != 0u) != 0ull) {
    if (cand != 0u) {
      const int bit = __ffs((int)cand) - 1;
      cand &= cand - 1u;
      const int j = bit >> 3;
      const uint32_t i = obj_begin + (uint32_t)(bit & 7);
      const float4* q = sc.sphere_ball + (size_t)kSphereTab * i + 2u;
      const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
      float4 ro4 = o4[0], rd4 = d4[0];
      float tcur = tp[0].x;
      if constexpr (kSlots > 1) { ro4 = sel4(j == 1, o4[1], ro4); rd4 = sel4(j == 1, d4[1], rd4); tcur = j == 1 ? tp[1].x : tcur; }
      if constexpr (kSlots > 2) { ro4 = sel4(j == 2, o4[2], ro4); rd4 = sel4(j == 2, d4[2], rd4); tcur = j == 2 ? tp[2].x : tcur; }
      if constexpr (kSlots > 3) { ro4 = sel4(j == 3, o4[3], ro4); rd4 = sel4(j == 3, d4[3], rd4); tcur = j == 3 ? tp[3].x : tcur; }
      const float tmin = (__float_as_uint(ro4.w) >> 31) ? 1e-5f : 1e-4f;
      Hit rec;
      if (sphere_exact_simple(sc.objects + obj_begin, q0, q1, q2, q3, xyz(ro4), xyz(rd4), tmin, tcur >= 0.0f ? tcur : FLT_MAX, rec)) {
        const uint32_t mat = __float_as_uint(q[4].x);
        const float4 ntp = make_float4(rec.t, rec.p.x, rec.p.y, rec.p.z);
        const float4 nnm = make_float4(rec.n.x, rec.n.y, rec.n.z, __uint_as_float(mat | (rec.side << 31)));
        tp[0] = sel4(j == 0, ntp, tp[0]);
        nm[0] = sel4(j == 0, nnm, nm[0]);
        if constexpr (kSlots > 1) { tp[1] = sel4(j == 1, ntp, tp[1]); nm[1] = sel4(j == 1, nnm, nm[1]); }
        if constexpr (kSlots > 2) { tp[2] = sel4(j == 2, ntp, tp[2]); nm[2] = sel4(j == 2, nnm, nm[2]); }
        if constexpr (kSlots > 3) { tp[3] = sel4(j == 3, ntp, tp[3]); nm[3] = sel4(j == 3, nnm, nm[3]); }
        changed |= 1u << j;
      }
    }
  }
  return changed;
}

__device__ __forceinline__ void store_hit(const DHits& hits, uint32_t slot, const Hit& rec)
{
  stnt(&hits.tp[slot], make_float4(rec.t, rec.p.x, rec.p.y, rec.p.z));
  stnt(&hits.nm[slot], make_float4(rec.n.x, rec.n.y, rec.n.z, __uint_as_float(rec.mat | (rec.side << 31))));
}

