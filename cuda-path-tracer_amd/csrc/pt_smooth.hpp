// pt_smooth.hpp -- smooth shading in the megakernel (ptc_set_vertex_normals, ptc_set_param "smooth_normals"): the
// shading normal of a triangle hit from the three vertex normals and the hit's barycentrics, and the host's area-weighted vertex
// normals of a mesh.  Host-callable; every float line is one IEEE binary32 operation of the order written down in section 5n
// (-ffp-contract=off, correctly rounded divide and square root); tests/smooth_ref.py restates it in numpy.
#pragma once

#include "pt_math.hpp"

#include <float.h>

namespace pt {
namespace smooth {

// m = (n0 w + n1 u) + n2 v per component, w = (1 - u) - v: u, v are ray_triangle's own, so u belongs to vertex 1 and v to vertex 2
PT_HD f3 interpolate(const f3 n0, const f3 n1, const f3 n2, const float u, const float v)
{
  const float t = 1.0f - u;
  const float w = t - v;
  const f3 a = n0 * w;
  const f3 b = n1 * u;
  const f3 c = n2 * v;
  return (a + b) + c;
}

// The shading normal at a closest hit on a triangle of an object whose inverse matrix is inv_m: n0 .. n2 the vertex normals (object
// space, any length), u, v the accepted test's barycentrics, g the geometric normal facing the ray, d the ray direction.  True: ns
// is the interpolated normal, mapped as a sphere's is (xform_normal), normalised and turned to g's side.  False, the fall-back: ns =
// g -- the mapped normal has no length to divide by (zero, not finite, a square past FLT_MAX), it lies in the triangle's plane
// (c == 0) or is a NaN, or it faces away from the ray.
PT_HD bool shading_normal(const f3 n0, const f3 n1, const f3 n2, const float u, const float v, const f3 g, const f3 d, const m4& inv_m, f3& ns)
{
  ns = g;
  const f3 m = interpolate(n0, n1, n2, u, v);
  const f3 a = xform_normal(inv_m, m);
  const float l2 = dot(a, a);
  if (!(l2 > 0.0f && l2 <= FLT_MAX)) return false;
  f3 s = normalize(a);
  const float c = dot(s, g);
  if (c < 0.0f) s = -s;
  if (!(c < 0.0f || c > 0.0f)) return false;  // 0 of either sign, or a NaN
  if (!(dot(d, s) < 0.0f)) return false;
  ns = s;
  return true;
}

// Area-weighted vertex normals of one mesh, on the host: triangles in index order, c = cross(p1 - p0, p2 - p0) added to the sums of
// corners 0, 1, 2 in that order; then every sum s with 0 < dot(s, s) <= FLT_MAX becomes normalize(s), any other (zero, not finite,
// an unused vertex) becomes (0, 0, 0).  The caller has checked the indices.
inline void vertex_normals(const float* positions, const uint32_t vertex_count, const uint32_t* indices, const uint32_t index_count, float* out)
{
  for (size_t k = 0; k < 3u * (size_t)vertex_count; ++k) out[k] = 0.0f;
  auto at = [](const float* p, uint32_t i) { return mk3(p[3u * (size_t)i], p[3u * (size_t)i + 1u], p[3u * (size_t)i + 2u]); };
  for (uint32_t t = 0; t + 2u < index_count; t += 3u) {
    const f3 p0 = at(positions, indices[t]);
    const f3 e1 = at(positions, indices[t + 1u]) - p0;
    const f3 e2 = at(positions, indices[t + 2u]) - p0;
    const f3 c = cross(e1, e2);
    for (uint32_t k = 0; k < 3u; ++k) {
      float* s = out + 3u * (size_t)indices[t + k];
      s[0] = s[0] + c.x;
      s[1] = s[1] + c.y;
      s[2] = s[2] + c.z;
    }
  }
  for (uint32_t i = 0; i < vertex_count; ++i) {
    const f3 s = at(out, i);
    const float l2 = dot(s, s);
    const f3 n = l2 > 0.0f && l2 <= FLT_MAX ? normalize(s) : mk3(0.0f, 0.0f, 0.0f);
    out[3u * (size_t)i] = n.x;
    out[3u * (size_t)i + 1u] = n.y;
    out[3u * (size_t)i + 2u] = n.z;
  }
}

}  // namespace smooth
}  // namespace pt
