// pt_texture.hpp -- image textures in the megakernel (ptc_set_textures, ptc_set_texcoords, ptc_set_param "textures"; DESIGN section
// 5o): the interpolated coordinate of a triangle hit, the texel lookup (wrap, filter, decode) and the albedo it gives, and the host's
// decode tables.  Host-callable; every float line is one IEEE binary32 operation of the order written down in section 5o
// (-ffp-contract=off); tests/texture_ref.py restates it in numpy.
#pragma once

#include "pt_math.hpp"

#include <float.h>
#include <math.h>
#include <stdint.h>

namespace pt {
namespace texmap {

// ptc_texture_desc's enums, and how a record's flags word packs them
constexpr uint32_t kLinear = 0u, kSrgb = 1u;
constexpr uint32_t kNearest = 0u, kBilinear = 1u;
constexpr uint32_t kRepeat = 0u, kClamp = 1u;
constexpr uint32_t kMaxSide = 4096u;
constexpr uint32_t kTableEntries = 256u;  // per encoding; the device table is the linear one followed by the sRGB one
PT_HD uint32_t pack_flags(const uint32_t encoding, const uint32_t filter, const uint32_t wrap) { return encoding | (filter << 1) | (wrap << 2); }

// One texture of the pool: where its texels start (in texels: a texel is one 32-bit word, r in the low byte, then g, b, a), its
// sides, its flags.  Row 0 is t = 0.
struct Record {
  uint32_t offset, width, height, flags;
};

// step 1, per component: (a0 w + a1 u) + a2 v with w = (1 - u) - v -- smooth::interpolate's order
PT_HD float interpolate(const float a0, const float a1, const float a2, const float u, const float v)
{
  const float t = 1.0f - u;
  const float w = t - v;
  const float a = a0 * w;
  const float b = a1 * u;
  const float c = a2 * v;
  const float ab = a + b;
  return ab + c;
}

// step 2: the lookup's refusal -- a NaN or an infinity (FLT_MAX itself is looked up)
PT_HD bool finite(const float s, const float t) { return __builtin_fabsf(s) <= FLT_MAX && __builtin_fabsf(t) <= FLT_MAX; }

// step 3: the coordinate in texels, 0 <= g <= n
PT_HD float texel_coordinate(const float x, const uint32_t n, const uint32_t wrap)
{
  float f;
  if (wrap == kRepeat) {
    const float fl = __builtin_floorf(x);
    f = x - fl;
    if (f >= 1.0f) f = 0.0f;  // a tiny negative x: x - (-1) rounds to 1
  } else {
    f = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
  }
  return f * (float)n;
}

// step 4
PT_HD int nearest_index(const float g, const uint32_t n)
{
  const int i = (int)__builtin_floorf(g);
  return i > (int)n - 1 ? (int)n - 1 : i;
}

// step 5: i0, i1 and the weight of i1
PT_HD void bilinear_indices(const float g, const uint32_t n, const uint32_t wrap, int& i0, int& i1, float& a)
{
  const float h = g - 0.5f;
  const float fl = __builtin_floorf(h);
  a = h - fl;
  i0 = (int)fl;
  i1 = i0 + 1;
  const int last = (int)n - 1;
  if (wrap == kRepeat) {
    if (i0 < 0) i0 += (int)n;
    else if (i0 > last) i0 -= (int)n;
    if (i1 < 0) i1 += (int)n;
    else if (i1 > last) i1 -= (int)n;
  } else {
    i0 = i0 < 0 ? 0 : (i0 > last ? last : i0);
    i1 = i1 < 0 ? 0 : (i1 > last ? last : i1);
  }
}

// env_rules::mix's form
PT_HD float mix(const float x, const float y, const float a) { return x * (1.0f - a) + y * a; }

// steps 2 .. 7: the texture's colour at (s, t).  texels: the pool; table: 2 x 256 floats, linear then sRGB.  False: the coordinate is
// refused, rgb = 0 and nothing was loaded.
PT_HD bool lookup(const uint32_t* texels, const Record rec, const float* table, const float s, const float t, f3& rgb)
{
  rgb = mk3(0.0f, 0.0f, 0.0f);
  if (!finite(s, t)) return false;
  const uint32_t wrap = (rec.flags >> 2) & 1u;
  const float* tab = table + ((rec.flags & 1u) ? kTableEntries : 0u);
  const uint32_t* base = texels + rec.offset;
  const float gs = texel_coordinate(s, rec.width, wrap);
  const float gt = texel_coordinate(t, rec.height, wrap);
  if (((rec.flags >> 1) & 1u) == kNearest) {
    const int i = nearest_index(gs, rec.width), j = nearest_index(gt, rec.height);
    const uint32_t c = base[(size_t)j * rec.width + (size_t)i];
    rgb = mk3(tab[c & 255u], tab[(c >> 8) & 255u], tab[(c >> 16) & 255u]);
    return true;
  }
  int i0, i1, j0, j1;
  float as, at;
  bilinear_indices(gs, rec.width, wrap, i0, i1, as);
  bilinear_indices(gt, rec.height, wrap, j0, j1, at);
  const uint32_t* row0 = base + (size_t)j0 * rec.width;
  const uint32_t* row1 = base + (size_t)j1 * rec.width;
  const uint32_t c00 = row0[i0], c10 = row0[i1], c01 = row1[i0], c11 = row1[i1];  // the four loads together, ahead of their first use
  float out[3];
  for (uint32_t k = 0; k < 3u; ++k) {
    const uint32_t sh = 8u * k;
    const float v00 = tab[(c00 >> sh) & 255u], v10 = tab[(c10 >> sh) & 255u], v01 = tab[(c01 >> sh) & 255u], v11 = tab[(c11 >> sh) & 255u];
    out[k] = mix(mix(v00, v10, as), mix(v01, v11, as), at);
  }
  rgb = mk3(out[0], out[1], out[2]);
  return true;
}

// steps 1 .. 8 at a triangle hit: st0 .. st2 the corners' pairs, u, v the accepted test's, p the material's colour.  True: albedo =
// texel x p; false, the fall-back: albedo = p and no texel was loaded.
PT_HD bool albedo(const uint32_t* texels, const Record rec, const float* table, const float* st0, const float* st1, const float* st2,
                  const float u, const float v, const f3 p, f3& out)
{
  const float s = interpolate(st0[0], st1[0], st2[0], u, v);
  const float t = interpolate(st0[1], st1[1], st2[1], u, v);
  f3 c;
  out = p;
  if (!lookup(texels, rec, table, s, t, c)) return false;
  out = c * p;
  return true;
}

// The decode table of one encoding, on the host: linear k / 255 in binary32 (one division); sRGB the piecewise curve in double,
// rounded once
inline void decode_table(const uint32_t encoding, float* out)
{
  for (uint32_t k = 0; k < kTableEntries; ++k) {
    if (encoding == kLinear) {
      out[k] = (float)k / 255.0f;
    } else {
      const double c = (double)k / 255.0;
      out[k] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
    }
  }
}

}  // namespace texmap
}  // namespace pt
