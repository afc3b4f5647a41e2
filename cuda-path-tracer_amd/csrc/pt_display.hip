// pt_display.hip -- the display transform on the device (ptc_set_display): k_meter / k_meter_packed count a frame's
// pixels into a 256-bin log-luminance histogram, k_meter_level turns the histogram into the exposure factor, k_tonemap /
// k_tonemap_packed apply that factor and the tone curve and encode with k_preview's lines (pt_post.hip, which stays as it is).
// Three launches in stream order and nothing else between them: no workgroup waits for another.  The rule itself -- bins, trimming,
// curves, one binary32 operation a line -- is pt_display.hpp's, which the host compiles as well (ptc_check_display_*).
// Part of libptcore.so.
#include "pt_device.hpp"
#include "pt_display.hpp"

namespace pt {

using namespace display_rules;

// A wavefront's own histogram in LDS (4 x 256 words a workgroup): neighbouring pixels share bins, so one histogram a workgroup would
// have its four wavefronts queue on the same words.  Integer adds commute: the histogram is the same bits whatever the order.
struct MeterBlock {
  uint32_t h[kMeterBlock / kWave][kBins];
};
static_assert(kBins == (uint32_t)kMeterBlock, "the fold at the end of k_meter: one thread a bin");

__device__ __forceinline__ void meter_begin(MeterBlock& s)
{
#pragma unroll
  for (int w = 0; w < kMeterBlock / kWave; ++w) s.h[w][threadIdx.x] = 0u;
  __syncthreads();
}

__device__ __forceinline__ void meter_pixel(MeterBlock& s, const float r, const float g, const float b, uint32_t& below, uint32_t& rejected)
{
  const int bin = bin_of(r, g, b);
  if (bin >= 0) atomicAdd(&s.h[threadIdx.x / (uint32_t)kWave][bin], 1u);
  below += bin == kBelow ? 1u : 0u;
  rejected += bin == kRejected ? 1u : 0u;
}

// the four histograms folded, one global add per bin that counted anything; the two side counts through a wave reduction, one add each
// a wavefront
__device__ __forceinline__ void meter_end(MeterBlock& s, uint32_t below, uint32_t rejected, DMeter* acc)
{
  __syncthreads();
  uint32_t total = 0u;
#pragma unroll
  for (int w = 0; w < kMeterBlock / kWave; ++w) total += s.h[w][threadIdx.x];
  if (total) atomicAdd(&acc->hist[threadIdx.x], total);
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    below += __shfl_down(below, d, kWave);
    rejected += __shfl_down(rejected, d, kWave);
  }
  if ((threadIdx.x & (uint32_t)(kWave - 1)) == 0u) {
    if (below) atomicAdd(&acc->below, below);
    if (rejected) atomicAdd(&acc->rejected, rejected);
  }
}

// grid-stride over the pixels (the grid is capped at kMeterMaxBlocks workgroups, launch_meter); a pixel is one 16-byte load
__global__ __launch_bounds__(kMeterBlock) void k_meter(const float4* __restrict__ src, uint32_t pix_count, DMeter* acc)
{
  __shared__ MeterBlock s;
  meter_begin(s);
  uint32_t below = 0u, rejected = 0u;
  const uint64_t stride = (uint64_t)gridDim.x * (uint32_t)kMeterBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * (uint32_t)kMeterBlock + threadIdx.x; i < pix_count; i += stride) {
    const float4 v = src[i];
    meter_pixel(s, v.x, v.y, v.z, below, rejected);
  }
  meter_end(s, below, rejected, acc);
}

// ... of a packed frame, three floats a pixel (the gathered frame of a multi-GPU run, a caller's RGB buffer)
__global__ __launch_bounds__(kMeterBlock) void k_meter_packed(const float* __restrict__ src, uint32_t pix_count, DMeter* acc)
{
  __shared__ MeterBlock s;
  meter_begin(s);
  uint32_t below = 0u, rejected = 0u;
  const uint64_t stride = (uint64_t)gridDim.x * (uint32_t)kMeterBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * (uint32_t)kMeterBlock + threadIdx.x; i < pix_count; i += stride)
    meter_pixel(s, src[3u * i], src[3u * i + 1u], src[3u * i + 2u], below, rejected);
  meter_end(s, below, rejected, acc);
}

// One wavefront: lane l holds bins 4 l .. 4 l + 3.  The samples below a lane's bins are an exclusive scan over the wavefront (64-bit:
// a frame may hold up to 2^32 - 1 pixels); every bin then keeps what display_rules::kept says, and the two sums are a wave reduction.
// The result -- the histogram with it -- goes to `out`, and the accumulation words are left zero for the next k_meter.
__global__ __launch_bounds__(kWave) void k_meter_level(DMeter* acc, DExposure* out, uint32_t pix_count, uint32_t low_permille,
                                                       uint32_t high_permille, float key, float exposure)
{
  const uint32_t lane = threadIdx.x;
  uint32_t h[4];
  unsigned long long mine = 0u;
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    h[j] = acc->hist[4u * lane + j];
    out->hist[4u * lane + j] = h[j];
    acc->hist[4u * lane + j] = 0u;
    mine += h[j];
  }
  unsigned long long incl = mine;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned long long up = __shfl_up(incl, d, kWave);
    if ((int)lane >= d) incl += up;
  }
  const unsigned long long n = __shfl(incl, kWave - 1, kWave);
  const uint64_t lo = skip_low(n, low_permille), hi = n - skip_high(n, high_permille);
  uint64_t cum = incl - mine;
  unsigned long long K = 0u, S = 0u;
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    const uint64_t t = kept(cum, h[j], lo, hi);
    K += t;
    S += (uint64_t)(4u * lane + j) * t;
    cum += h[j];
  }
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    K += __shfl_down(K, d, kWave);
    S += __shfl_down(S, d, kWave);
  }
  if (lane == 0u) {
    const int m = mean_bin(K, S);
    out->pixels = pix_count;
    out->counted = (uint32_t)n;
    out->below = acc->below;
    out->rejected = acc->rejected;
    out->level_bin = m;
    out->level = m < 0 ? 0.0f : level_of(m);
    out->scale = scale_of(m, key, exposure);
    acc->below = 0u;
    acc->rejected = 0u;
  }
}

// k_preview's lines (pt_post.hip), on a channel that went through the curve
__device__ __forceinline__ uint32_t encode_rgba(const float r, const float g, const float b)
{
  const float e = 1.f / 2.2f;
  const float cr = powf(r, e), cg = powf(g, e), cb = powf(b, e);
  auto to255 = [](float x) -> uint32_t { return (uint32_t)(unsigned char)(sel_min(sel_max(x, 0.f), 1.f) * 255.99f); };
  return to255(cr) | (to255(cg) << 8) | (to255(cb) << 16) | (255u << 24);
}

__device__ __forceinline__ void tonemap_pixel(const uint32_t i, float r, float g, float b, const float scale, const int curve, const float w2,
                                              uint32_t* rgba, float* mapped)
{
  r = map_channel(r, scale, curve, w2);
  g = map_channel(g, scale, curve, w2);
  b = map_channel(b, scale, curve, w2);
  if (rgba) rgba[i] = encode_rgba(r, g, b);
  if (mapped) {
    mapped[3u * (size_t)i] = r;
    mapped[3u * (size_t)i + 1u] = g;
    mapped[3u * (size_t)i + 2u] = b;
  }
}

// One thread a pixel.  metered != null: the factor k_meter_level left there; else `scale` (manual metering: the exposure).
__global__ __launch_bounds__(256) void k_tonemap(const float4* __restrict__ src, uint32_t pix_count, const DExposure* metered, float scale,
                                                 int curve, float w2, uint32_t* rgba, float* mapped)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= pix_count) return;
  if (metered) scale = metered->scale;
  const float4 v = src[i];
  tonemap_pixel(i, v.x, v.y, v.z, scale, curve, w2, rgba, mapped);
}

__global__ __launch_bounds__(256) void k_tonemap_packed(const float* __restrict__ src, uint32_t pix_count, const DExposure* metered, float scale,
                                                        int curve, float w2, uint32_t* rgba, float* mapped)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= pix_count) return;
  if (metered) scale = metered->scale;
  tonemap_pixel(i, src[3u * (size_t)i], src[3u * (size_t)i + 1u], src[3u * (size_t)i + 2u], scale, curve, w2, rgba, mapped);
}

// ------------------------------------------------------------------------------------------------
// launchers (src4 or src3: exactly one is not null)
// ------------------------------------------------------------------------------------------------
static inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

void launch_meter(hipStream_t s, const float4* src4, const float* src3, uint32_t pix_count, DMeter* acc)
{
  const uint32_t blocks = div_up(pix_count, (uint32_t)kMeterBlock);
  const dim3 grid(blocks < kMeterMaxBlocks ? blocks : kMeterMaxBlocks), block(kMeterBlock);
  if (src4) hipLaunchKernelGGL(k_meter, grid, block, 0, s, src4, pix_count, acc);
  else hipLaunchKernelGGL(k_meter_packed, grid, block, 0, s, src3, pix_count, acc);
}
void launch_meter_level(hipStream_t s, DMeter* acc, DExposure* out, uint32_t pix_count, uint32_t low_permille, uint32_t high_permille,
                        float key, float exposure)
{
  hipLaunchKernelGGL(k_meter_level, dim3(1), dim3(kWave), 0, s, acc, out, pix_count, low_permille, high_permille, key, exposure);
}
void launch_tonemap(hipStream_t s, const float4* src4, const float* src3, uint32_t pix_count, const DExposure* metered, float scale,
                    int curve, float w2, uint32_t* rgba, float* mapped)
{
  const dim3 grid(div_up(pix_count, 256u)), block(256);
  if (src4) hipLaunchKernelGGL(k_tonemap, grid, block, 0, s, src4, pix_count, metered, scale, curve, w2, rgba, mapped);
  else hipLaunchKernelGGL(k_tonemap_packed, grid, block, 0, s, src3, pix_count, metered, scale, curve, w2, rgba, mapped);
}

}  // namespace pt
