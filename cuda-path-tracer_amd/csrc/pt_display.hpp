// pt_display.hpp -- the display transform (ptc_set_display, an extension: the reference shows clamp + gamma only):
// the metering of a frame into a 256-bin log-luminance histogram, the level a trimmed mean of that histogram gives, and the tone curve
// of a channel, stated once for the device (pt_display.hip: k_meter, k_meter_level, k_tonemap) and the host (ptc_check_display_meter,
// ptc_check_display_map; tests/display_ref.py restates it in numpy).
// Every line of the float arithmetic is one binary32 operation (-ffp-contract=off, IEEE divide); the histogram and the level are
// integers.  No log2f anywhere: a bin is the exponent and the top three mantissa bits of the luminance.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef PT_DISPLAY_HD
#if defined(__HIPCC__)
#define PT_DISPLAY_HD __host__ __device__ __forceinline__
#else
#define PT_DISPLAY_HD inline
#endif
#endif

namespace pt {
namespace display_rules {

constexpr uint32_t kBins = 256u;
constexpr uint32_t kBinBase = 888u;       // bits(2^-16) >> 20: bin 0 starts at 2^-16, eight bins an octave, bin 128 at 1.0
constexpr int kBelow = -1, kRejected = -2;  // bin_of's other two answers
constexpr float kCap = 1048576.0f;        // 2^20: what an exposed channel is cut to before the curve (an infinity lands here)
constexpr int kCurveClamp = 0, kCurveReinhard = 1, kCurveAces = 2;

PT_DISPLAY_HD uint32_t bits_of(const float f)
{
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}
PT_DISPLAY_HD float float_of(const uint32_t u)
{
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}

// Where a pixel is counted: its bin 0 .. 255, kBelow (a luminance under 2^-16: +0, -0, denormals) or kRejected (a luminance that is
// negative or not finite: a NaN in any channel, an infinity, a sum that overflows).
PT_DISPLAY_HD int bin_of(const float r, const float g, const float b)
{
  const float yr = 0.2126f * r;
  const float yg = 0.7152f * g;
  const float yb = 0.0722f * b;
  const float s = yr + yg;
  const float y = s + yb;
  if (!(y >= 0.0f) || !(y <= 3.402823466e+38f)) return kRejected;
  if (y < 1.52587890625e-05f) return kBelow;  // 2^-16
  const uint32_t k = (bits_of(y) >> 20) - kBinBase;
  return (int)(k < kBins - 1u ? k : kBins - 1u);
}

// The trimmed mean of a histogram, in 64-bit integers.  N = the samples; the first N low / 1000 and the last N (1000 - high) / 1000 of
// them, in ascending bin order, are left out; m = the mean bin of the others, rounded to nearest (halves up).  -1: nothing was counted.
// cum = the samples in bins below k, h = bin k's: kept() is how many of bin k's stay.
PT_DISPLAY_HD uint64_t kept(const uint64_t cum, const uint64_t h, const uint64_t lo, const uint64_t hi)
{
  const uint64_t a = cum > lo ? cum : lo;
  const uint64_t e = cum + h < hi ? cum + h : hi;
  return e > a ? e - a : 0u;
}
PT_DISPLAY_HD uint64_t skip_low(const uint64_t n, const uint32_t low_permille) { return n * low_permille / 1000u; }
PT_DISPLAY_HD uint64_t skip_high(const uint64_t n, const uint32_t high_permille) { return n * (1000u - high_permille) / 1000u; }
PT_DISPLAY_HD int mean_bin(const uint64_t K, const uint64_t S) { return K ? (int)((2u * S + K) / (2u * K)) : -1; }

// the lower edge of bin m, exactly
PT_DISPLAY_HD float level_of(const int m) { return float_of(((uint32_t)m + kBinBase) << 20); }

// the factor every channel is multiplied by: (key / level) * exposure, or the exposure alone where nothing was metered (m < 0)
PT_DISPLAY_HD float scale_of(const int m, const float key, const float exposure)
{
  if (m < 0) return exposure;
  const float q = key / level_of(m);
  return q * exposure;
}

inline int level_bin(const uint32_t* hist, const uint32_t low_permille, const uint32_t high_permille, uint64_t* counted)
{
  uint64_t n = 0;
  for (uint32_t k = 0; k < kBins; ++k) n += hist[k];
  if (counted) *counted = n;
  const uint64_t lo = skip_low(n, low_permille), hi = n - skip_high(n, high_permille);
  uint64_t cum = 0, K = 0, S = 0;
  for (uint32_t k = 0; k < kBins; ++k) {
    const uint64_t t = kept(cum, hist[k], lo, hi);
    K += t;
    S += (uint64_t)k * t;
    cum += hist[k];
  }
  return mean_bin(K, S);
}

// One channel through exposure and curve; w2 = white * white (Reinhard's, computed once on the host in binary32).  The result is what
// k_preview's lines encode: gamma 1 / 2.2, clamp to [0, 1], * 255.99f.
PT_DISPLAY_HD float map_channel(const float c, const float scale, const int curve, const float w2)
{
  const float e = c * scale;
  float x = e > 0.0f ? e : 0.0f;  // (a NaN, a negative: 0)
  x = x < kCap ? x : kCap;
  if (curve == kCurveReinhard) {
    const float q = x / w2;
    const float p = 1.0f + q;
    const float n = x * p;
    const float d = 1.0f + x;
    return n / d;
  }
  if (curve == kCurveAces) {  // Narkowicz's fit
    const float a = 2.51f * x;
    const float b = a + 0.03f;
    const float num = x * b;
    const float c2 = 2.43f * x;
    const float d = c2 + 0.59f;
    const float f = x * d;
    const float den = f + 0.14f;
    return num / den;
  }
  return x;
}

}  // namespace display_rules
}  // namespace pt
