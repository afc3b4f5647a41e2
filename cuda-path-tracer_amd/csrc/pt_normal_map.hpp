// pt_normal_map.hpp -- normal maps in the megakernel (ptc_set_normal_maps, ptc_set_param "normal_maps"): the
// tangent-space normal a texture of the pool gives at a triangle hit, turned into the world about the base normal, and the host's
// decode table.  Host-callable; every float line is one IEEE binary32 operation of the order written down in section 5q
// (-ffp-contract=off, correctly rounded divide and square root); tests/normal_map_ref.py restates it in numpy.
#pragma once

#include "pt_math.hpp"
#include "pt_texture.hpp"

#include <float.h>
#include <stdint.h>

namespace pt {
namespace nmap {

// what the rule did at a hit (ptc_hit_shading_normal's and ptc_check_normal_map's outcome byte; 0 a miss, 1 no rule applied)
constexpr uint32_t kMiss = 0u, kNone = 1u, kBent = 2u, kFlat = 3u, kKept = 4u;

// The decode table, on the host: max((k - 128) / 127, -1) -- byte 128 is exactly 0, byte 255 exactly 1, bytes 0 and 1 are -1
inline void decode_table(float* out)
{
  for (uint32_t k = 0; k < texmap::kTableEntries; ++k) {
    const float c = ((float)k - 128.0f) / 127.0f;
    out[k] = c < -1.0f ? -1.0f : c;
  }
}

// step 2: texmap::lookup's steps 2 .. 7 with `table` (256 floats) whatever the record's encoding says; its filter and wrap hold
PT_HD bool lookup(const uint32_t* texels, texmap::Record rec, const float* table, const float s, const float t, f3& c)
{
  rec.flags &= ~1u;
  return texmap::lookup(texels, rec, table, s, t, c);
}

PT_HD bool has_length(const float l2) { return l2 > 0.0f && l2 <= FLT_MAX; }

// steps 3 .. 8 on the texel c: p0 .. p2 the corners' object-space positions, st0 .. st2 their coordinate pairs, m the object's
// matrix, b the base normal, g the geometric normal facing the ray, d the ray direction.  n = b unless the outcome is kBent.
PT_HD uint32_t bend(const f3 c, const f3 p0, const f3 p1, const f3 p2, const float* st0, const float* st1, const float* st2, const m4& m,
                    const f3 b, const f3 g, const f3 d, f3& n)
{
  n = b;
  const float x = c.x, y = c.y, z = c.z;
  if (x == 0.0f && y == 0.0f && z > 0.0f) return kFlat;
  const f3 e1 = p1 - p0;
  const f3 e2 = p2 - p0;
  const float ds1 = st1[0] - st0[0];
  const float ds2 = st2[0] - st0[0];
  const float dt1 = st1[1] - st0[1];
  const float dt2 = st2[1] - st0[1];
  const float da = ds1 * dt2;
  const float db = ds2 * dt1;
  const float det = da - db;
  if (!(det > 0.0f || det < 0.0f)) return kKept;
  f3 t_o = e1 * dt2 - e2 * dt1;
  f3 b_o = e2 * ds1 - e1 * ds2;
  if (det < 0.0f) {
    t_o = -t_o;
    b_o = -b_o;
  }
  const f3 t_w = xform_vector(m, t_o);
  const f3 b_w = xform_vector(m, b_o);
  const float k = dot(t_w, b);
  const f3 tp = t_w - b * k;
  if (!has_length(dot(tp, tp))) return kKept;
  const f3 t = normalize(tp);
  const f3 cr = cross(b, t);
  const f3 bt = dot(cr, b_w) < 0.0f ? -cr : cr;
  const f3 a = (t * x + bt * y) + b * z;
  if (!has_length(dot(a, a))) return kKept;
  const f3 s = normalize(a);
  if (!(dot(s, g) > 0.0f)) return kKept;
  if (!(dot(d, s) < 0.0f)) return kKept;
  n = s;
  return kBent;
}

// steps 1 .. 8 at a triangle hit with u, v the accepted test's
PT_HD uint32_t shade(const uint32_t* texels, const texmap::Record rec, const float* table, const f3 p0, const f3 p1, const f3 p2, const float* st0,
                     const float* st1, const float* st2, const float u, const float v, const m4& m, const f3 b, const f3 g, const f3 d, f3& n)
{
  const float s = texmap::interpolate(st0[0], st1[0], st2[0], u, v);
  const float t = texmap::interpolate(st0[1], st1[1], st2[1], u, v);
  f3 c;
  n = b;
  if (!nmap::lookup(texels, rec, table, s, t, c)) return kKept;
  return bend(c, p0, p1, p2, st0, st1, st2, m, b, g, d, n);
}

}  // namespace nmap
}  // namespace pt
