// pt_denoise_variance.hip -- the variance-guided A-Trous mode (ptc_set_param "denoise_variance", ptc_denoise_variance; DESIGN section
// 5s): k_variance_estimate, the per-pixel spatial variance of the plane the passes filter; k_variance_prefilter, its 3 x 3 Gaussian and
// the count of pixels on the floor; k_denoise_var_lds<step> and k_denoise_var, the passes whose colour weight that variance steers and
// which carry it along -- in a translation unit of its own so that every other code object stays what it was.  The rule is
// pt_denoise_variance.hpp's; the tap-coordinate contract, the staging scheme and the workgroup order are k_denoise_lds' (pt_post.hip).
// Part of libptcore.so.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_denoise_variance.hpp"
#include <float.h>

namespace pt {

#include "pt_kernels_common.inc"

// ---- the estimate ----
// One workgroup of four wavefronts per 32 x 8 pixel tile, one thread per pixel; the tile with its 3-pixel halo, 38 x 14 pixels of
// colour, normal and position (36 bytes each, 19 KB), is staged in LDS once and both sweeps of the 7 x 7 window run from it.  Why
// 32 x 8 and not a wavefront's 8 x 8: the halo ratio (staged / output pixels) is 2.08 against 3.06 -- 16 x 16 would give 1.89, but a
// wavefront's 64 lanes then span four rows of 16, and a ds_read_b128's 16-lane groups take lanes from two rows whose 16-byte slots
// collide two ways at a row stride of 22; with 32 pixels a row each 32-lane half of a wavefront reads one contiguous run, which no
// group of ds_read_b128 or ds_read_b32 conflicts on.  Window coordinates are clamped to the image (a plain clamp: the estimate is
// new and owes the reference's off-by-one taps nothing), so every position is den_pos' own.
constexpr int kEstW = 32, kEstH = 8, kEstHalo = dvar::kVarRadius;
constexpr int kEstRow = kEstW + 2 * kEstHalo, kEstRows = kEstH + 2 * kEstHalo, kEstPoints = kEstRow * kEstRows;
__global__ __launch_bounds__(256) void k_variance_estimate(uint32_t width, uint32_t height, const float4* color, const float4* nd,
                                                           const float4* pos, float* variance, float n_phi, float p_phi)
{
#pragma clang fp contract(fast)
  __shared__ float4 s_a[kEstPoints];  // colour.rgb, normal.x
  __shared__ float4 s_b[kEstPoints];  // normal.yz, position.xy
  __shared__ float s_c[kEstPoints];   // position.z
  const int W = (int)width, H = (int)height;
  const uint32_t tiles_x = (width + kEstW - 1u) / kEstW;
  const int tx = (int)(blockIdx.x % tiles_x), ty = (int)(blockIdx.x / tiles_x);
  const int x0 = tx * kEstW - kEstHalo, y0 = ty * kEstH - kEstHalo;
  constexpr int kRounds = (kEstPoints + 255) / 256;  // all the global loads of a thread in flight before the first is used
  float4 c[kRounds], g[kRounds], q[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int k = min(r * 256 + (int)threadIdx.x, kEstPoints - 1);
    int u = x0 + k % kEstRow, v = y0 + k / kEstRow;
    u = u < 0 ? 0 : (u > W - 1 ? W - 1 : u);
    v = v < 0 ? 0 : (v > H - 1 ? H - 1 : v);
    const uint32_t ti = (uint32_t)u + (uint32_t)v * width;
    c[r] = color[ti];
    g[r] = nd[ti];
    q[r] = pos[ti];
  }
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int k = r * 256 + (int)threadIdx.x;
    if (k < kEstPoints) {
      s_a[k] = make_float4(c[r].x, c[r].y, c[r].z, g[r].x);
      s_b[k] = make_float4(g[r].y, g[r].z, q[r].x, q[r].y);
      s_c[k] = q[r].z;
    }
  }
  __syncthreads();
  const int i = (int)(threadIdx.x & 31u), j = (int)(threadIdx.x >> 5);
  const int x = tx * kEstW + i, y = ty * kEstH + j;
  if (x >= W || y >= H) return;  // (a frame whose sides are no multiple of the tile: the last column and row of tiles)
  const int centre = (j + kEstHalo) * kEstRow + i + kEstHalo;
  const float4 ca = s_a[centre], cb = s_b[centre];
  const f3 cval = mk3(ca.x, ca.y, ca.z), nval = mk3(ca.w, cb.x, cb.y), pval = mk3(cb.z, cb.w, s_c[centre]);
  const float kn = dvar::term_scale(n_phi), kp = dvar::term_scale(p_phi);
  // sweep 1: the weighted mean
  dvar::MeanSum ms{mk3(0.f, 0.f, 0.f), 0.0f};
#pragma unroll 1
  for (int dy = -kEstHalo; dy <= kEstHalo; ++dy) {
    const int row = centre + dy * kEstRow;
#pragma unroll
    for (int dx = -kEstHalo; dx <= kEstHalo; ++dx) {
      const float4 ta = s_a[row + dx], tb = s_b[row + dx];
      const float tz = s_c[row + dx];
      const float gq = dvar::estimate_weight(nval, mk3(ta.w, tb.x, tb.y), pval, mk3(tb.z, tb.w, tz), kn, kp);
      dvar::mean_tap(ms, gq, cval, mk3(ta.x, ta.y, ta.z));
    }
  }
  const f3 mean = dvar::mean_of(ms, cval);
  // sweep 2: the weighted squared distance from it (the weights again: 49 of them do not fit a thread's registers)
  float acc = 0.0f;
#pragma unroll 1
  for (int dy = -kEstHalo; dy <= kEstHalo; ++dy) {
    const int row = centre + dy * kEstRow;
#pragma unroll
    for (int dx = -kEstHalo; dx <= kEstHalo; ++dx) {
      const float4 ta = s_a[row + dx], tb = s_b[row + dx];
      const float tz = s_c[row + dx];
      const float gq = dvar::estimate_weight(nval, mk3(ta.w, tb.x, tb.y), pval, mk3(tb.z, tb.w, tz), kn, kp);
      dvar::variance_tap(acc, gq, mk3(ta.x, ta.y, ta.z), mean);
    }
  }
  variance[(uint32_t)x + (uint32_t)y * width] = dvar::variance_of(acc, ms.g);
}

// the nine variances around (x, y), coordinates clamped to the image, into v[3 (dy + 1) + dx + 1]
__device__ __forceinline__ void variance_3x3(const float* variance, const int W, const int H, const int x, const int y, float v[9])
{
  const int xl = x > 0 ? x - 1 : 0, xr = x < W - 1 ? x + 1 : W - 1;
  const int yu = y > 0 ? y - 1 : 0, yd = y < H - 1 ? y + 1 : H - 1;
  const uint32_t r0 = (uint32_t)yu * (uint32_t)W, r1 = (uint32_t)y * (uint32_t)W, r2 = (uint32_t)yd * (uint32_t)W;
  v[0] = variance[r0 + (uint32_t)xl];
  v[1] = variance[r0 + (uint32_t)x];
  v[2] = variance[r0 + (uint32_t)xr];
  v[3] = variance[r1 + (uint32_t)xl];
  v[4] = variance[r1 + (uint32_t)x];
  v[5] = variance[r1 + (uint32_t)xr];
  v[6] = variance[r2 + (uint32_t)xl];
  v[7] = variance[r2 + (uint32_t)x];
  v[8] = variance[r2 + (uint32_t)xr];
}

// The prefiltered plane of a variance plane, as the first pass sees it (prefiltered may be null: ptc_denoise wants the counters alone,
// its passes prefilter for themselves), and the stage's counters, k_denoise_albedo's way: kLightStatLines lines of kLoopStatWords words,
// word 0 += pixels, word 1 += pixels whose prefiltered variance is below dvar::kVarianceFloor; one add per wavefront and word, the
// workgroups dealt over the lines (all 32,400 wavefronts of a 1080p frame adding to one address cost more than the estimate).
__global__ __launch_bounds__(256) void k_variance_prefilter(uint32_t width, uint32_t height, const float* variance, float* prefiltered,
                                                            unsigned long long* stats)
{
  const uint32_t index = blockIdx.x * 256u + threadIdx.x;
  const bool inside = index < width * height;
  uint32_t n_floor = 0u;
  if (inside) {
    float v[9];
    variance_3x3(variance, (int)width, (int)height, (int)(index % width), (int)(index / width), v);
    const float p = dvar::prefilter(v);
    if (prefiltered) prefiltered[index] = p;
    n_floor = dvar::floored(p) ? 1u : 0u;
  }
  const uint32_t s_pixels = wave_sum(inside ? 1u : 0u), s_floor = wave_sum(n_floor);
  if ((threadIdx.x & (kWave - 1u)) == 0u) {
    unsigned long long* line = stats + kLoopStatWords * (blockIdx.x % kLightStatLines);
    if (s_pixels) atomicAdd(&line[0], (unsigned long long)s_pixels);
    if (s_floor) atomicAdd(&line[1], (unsigned long long)s_floor);
  }
}

// ---- the passes ----
// A guided pass with its taps through L1 / L2: "denoise_variant" 1, a step above 32 (the staged tile outgrows 64 KB of LDS) and a step
// that is no power of two; the cross-check of k_denoise_var_lds, as k_denoise is k_denoise_lds'.  kInterior as in denoise_pixel.
template <bool kInterior>
__device__ __forceinline__ void denoise_var_pixel(const DCamera& cam, const uint32_t pix_count, const float4* color, const float* variance,
                                                  const float4* nd, const float4* pos, float4* out, float* variance_out,
                                                  const int step_width, const DDenoiseVar& prm, const int x, const int y)
{
#pragma clang fp contract(fast)
  const uint32_t W = cam.width, H = cam.height;
  const uint32_t index = (uint32_t)x + (uint32_t)y * W;
  const f3 cval = xyz(color[index]);
  const f3 nval = xyz(nd[index]);
  const f3 pval = xyz(pos[index]);
  float v9[9];
  variance_3x3(variance, (int)W, (int)H, x, y, v9);
  const float step2 = (float)(step_width * step_width);
  const float kc = dvar::colour_scale(prm.sigma, dvar::prefilter(v9));
  const float kn = dvar::term_scale(step2 * prm.n_phi), kp = dvar::term_scale(prm.p_phi);
  dvar::PassSum ps{mk3(0.f, 0.f, 0.f), 0.0f, 0.0f};
#pragma unroll 1
  for (int dy = -2; dy <= 2; ++dy) {
    int v = y + dy * step_width;
    if (!kInterior) v = v < 0 ? 0 : (v > (int)H ? (int)H : v);
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      int u = x + dx * step_width;
      if (!kInterior) u = u < 0 ? 0 : (u > (int)W ? (int)W : u);
      uint32_t ti = (uint32_t)u + (uint32_t)v * W;
      if (!kInterior && ti >= pix_count) ti = pix_count - 1u;
      const f3 ctemp = xyz(color[ti]);
      const float4 ndt = nd[ti];
      const float vq = variance[ti];
      f3 ptmp;
      if (!kInterior && (u == (int)W || v == (int)H)) {  // the reference's off-by-one taps keep their own view ray
        f3 to, td;
        generate_ray(cam, (float)u + 0.5f, (float)v + 0.5f, to, td);
        ptmp = to + td * ndt.w;
      } else {
        ptmp = xyz(pos[ti]);
      }
      const f3 diff = cval - ctemp;
      const float dc = diff.x * diff.x + diff.y * diff.y + diff.z * diff.z;
      const float weight = dvar::pass_weight(dc, dvar::dist2(nval, xyz(ndt)), dvar::dist2(pval, ptmp), kc, kn, kp);
      dvar::pass_tap(ps, weight * dvar::kernel_weight(dx, dy), diff, vq);
    }
  }
  f3 c_out;
  float v_out;
  dvar::pass_result(ps, cval, c_out, v_out);
  out[index] = make_float4(c_out.x, c_out.y, c_out.z, 0.0f);
  variance_out[index] = v_out;
}

__global__ __launch_bounds__(256) void k_denoise_var(DCamera cam, uint32_t pix_count, const float4* color, const float* variance,
                                                     const float4* nd, const float4* pos, float4* out, float* variance_out,
                                                     int step_width, DDenoiseVar prm)
{
  const int W = (int)cam.width, H = (int)cam.height;
  const uint32_t tiles_x = ((uint32_t)W + 15u) / 16u;
  const int x0 = (int)(blockIdx.x % tiles_x) * 16, y0 = (int)(blockIdx.x / tiles_x) * 16;
  const int x = x0 + (int)(threadIdx.x & 15u), y = y0 + (int)(threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const int reach = 2 * step_width;
  const bool interior = x0 - reach >= 0 && y0 - reach >= 0 && x0 + 15 + reach < W && y0 + 15 + reach < H;
  if (interior) denoise_var_pixel<true>(cam, pix_count, color, variance, nd, pos, out, variance_out, step_width, prm, x, y);
  else denoise_var_pixel<false>(cam, pix_count, color, variance, nd, pos, out, variance_out, step_width, prm, x, y);
}

// The guided pass with its taps staged in LDS (the default): k_denoise_lds' scheme -- one residue class of rows per workgroup, dense
// horizontally, the step a template parameter, the reference's clamp applied once when a pixel is staged, one contiguous eighth of the
// tiles per XCD -- with a tenth float per staged pixel, the tap's variance, read by the tap's index.  The staged record stays three
// planes: two float4 and, where k_denoise_lds has a float (position.z), a float2 (position.z, variance): 40 bytes a pixel, 61,440 at
// step 32.  One ds_read_b64 of a 32-lane half covers 256 consecutive bytes, all 64 banks once, so the tenth float costs no LDS
// instruction and no conflict (a fourth plane of floats would have cost a ds_read_b32 a tap).
// The variance the centre's prefilter reads comes from the scalar plane itself, nine 4-byte loads a pixel whose rows are coalesced
// across the wavefront: the rows at +-1 pixel are not in the staged tile above step 1.  (The alternative, the .w lane of the float4
// ping-pong planes, would make them nine 16-byte loads, would put a non-zero .w into the result buffer the views read, and the first
// pass's input -- the accumulated colour or the irradiance plane -- has no such lane to read.)
constexpr int kDenVarW = 64, kDenVarRows = 4, kDenVarHalo = 2;
template <int kStep>
__global__ __launch_bounds__(256) void k_denoise_var_lds(DCamera cam, uint32_t pix_count, const float4* color, const float* variance,
                                                         const float4* nd, const float4* pos, float4* out, float* variance_out,
                                                         DDenoiseVar prm)
{
#pragma clang fp contract(fast)
  extern __shared__ float4 s_dyn[];
  constexpr int step = kStep;
  const int W = (int)cam.width, H = (int)cam.height;
  constexpr int row_len = kDenVarW + 2 * kDenVarHalo * step, rows = kDenVarRows + 2 * kDenVarHalo, points = row_len * rows;
  float4* s_a = s_dyn;                                         // colour.rgb, normal.x
  float4* s_b = s_dyn + points;                                // normal.yz, position.xy
  float2* s_c = reinterpret_cast<float2*>(s_dyn + 2 * points);  // position.z, variance
  const uint32_t tiles_x = ((uint32_t)W + kDenVarW - 1u) / kDenVarW;
  const uint32_t lattice_rows = ((uint32_t)H + (uint32_t)step - 1u) / (uint32_t)step;
  const uint32_t tiles_y = (lattice_rows + kDenVarRows - 1u) / kDenVarRows;
  const uint32_t total = tiles_x * tiles_y * (uint32_t)step, per_xcd = (total + 7u) / 8u;
  uint32_t b = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
  if ((blockIdx.x >> 3) >= per_xcd || b >= total) return;
  const int tx = (int)(b % tiles_x);
  b /= tiles_x;
  const int ty = (int)(b % tiles_y), ry = (int)(b / tiles_y);
  const int x0 = tx * kDenVarW - kDenVarHalo * step;  // first staged column
  // the centre's nine variances: issued ahead of the staging loads, used after the barrier
  const int i = (int)(threadIdx.x & 63u), j = (int)(threadIdx.x >> 6);
  const int x = tx * kDenVarW + i, y = (ty * kDenVarRows + j) * step + ry;
  const bool inside = x < W && y < H;
  float v9[9];
  if (inside) variance_3x3(variance, W, H, x, y, v9);
  constexpr int kRounds = 3;
  for (int base = 0; base < points; base += 256 * kRounds) {
    float4 c[kRounds], g[kRounds], q[kRounds];
    float vr[kRounds];
    int uu[kRounds], vv[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int k = min(base + r * 256 + (int)threadIdx.x, points - 1);
      const int li = k % row_len, lj = k / row_len;
      int u = x0 + li;
      int v = (ty * kDenVarRows + lj - kDenVarHalo) * step + ry;
      u = u < 0 ? 0 : (u > W ? W : u);
      v = v < 0 ? 0 : (v > H ? H : v);
      uint32_t ti = (uint32_t)u + (uint32_t)v * (uint32_t)W;
      if (ti >= pix_count) ti = pix_count - 1u;
      uu[r] = u;
      vv[r] = v;
      c[r] = color[ti];
      g[r] = nd[ti];
      q[r] = pos[ti];
      vr[r] = variance[ti];
    }
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int k = base + r * 256 + (int)threadIdx.x;
      f3 p = xyz(q[r]);
      if (uu[r] == W || vv[r] == H) {  // the reference's off-by-one taps keep their own view ray
        f3 to, td;
        generate_ray(cam, (float)uu[r] + 0.5f, (float)vv[r] + 0.5f, to, td);
        p = to + td * g[r].w;
      }
      if (k < points) {
        s_a[k] = make_float4(c[r].x, c[r].y, c[r].z, g[r].x);
        s_b[k] = make_float4(g[r].y, g[r].z, p.x, p.y);
        s_c[k] = make_float2(p.z, vr[r]);
      }
    }
  }
  __syncthreads();
  if (!inside) return;
  const int centre = (j + kDenVarHalo) * row_len + i + kDenVarHalo * step;
  const float4 ca = s_a[centre], cb = s_b[centre];
  const f3 cval = mk3(ca.x, ca.y, ca.z), nval = mk3(ca.w, cb.x, cb.y), pval = mk3(cb.z, cb.w, s_c[centre].x);
  const float step2 = (float)(step * step);
  // one reciprocal a pixel, not a tap: the colour term's scale from the prefiltered variance
  const float kc = dvar::colour_scale(prm.sigma, dvar::prefilter(v9));
  const float kn = dvar::term_scale(step2 * prm.n_phi), kp = dvar::term_scale(prm.p_phi);
  const float kernel[3] = {3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
  dvar::PassSum ps{mk3(0.f, 0.f, 0.f), 0.0f, 0.0f};
#pragma unroll 1
  for (int dy = -2; dy <= 2; ++dy) {
    const int ady = dy < 0 ? -dy : dy;
    const float w_by_adx[3] = {kernel[0], kernel[ady < 1 ? ady : 1], kernel[ady]};
    const int row = centre + dy * row_len;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int t = row + dx * step;
      const float4 ta = s_a[t], tb = s_b[t];
      const float2 tc = s_c[t];
      const f3 diff = mk3(cval.x - ta.x, cval.y - ta.y, cval.z - ta.z);
      const float nx = nval.x - ta.w, ny = nval.y - tb.x, nz = nval.z - tb.y;
      const float px = pval.x - tb.z, py = pval.y - tb.w, pz = pval.z - tc.x;
      const float dc = diff.x * diff.x + diff.y * diff.y + diff.z * diff.z, dn = nx * nx + ny * ny + nz * nz,
                  dp = px * px + py * py + pz * pz;
      const float weight = dvar::pass_weight(dc, dn, dp, kc, kn, kp);
      dvar::pass_tap(ps, weight * w_by_adx[dx < 0 ? -dx : dx], diff, tc.y);
    }
  }
  f3 c_out;
  float v_out;
  dvar::pass_result(ps, cval, c_out, v_out);
  const uint32_t index = (uint32_t)x + (uint32_t)y * (uint32_t)W;
  out[index] = make_float4(c_out.x, c_out.y, c_out.z, 0.0f);
  variance_out[index] = v_out;
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static inline uint32_t div_up_var(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

void launch_variance_estimate(hipStream_t s, uint32_t width, uint32_t height, const float4* color, const float4* nd, const float4* pos,
                              float* variance, float n_phi, float p_phi)
{
  const dim3 grid(div_up_var(width, (uint32_t)kEstW) * div_up_var(height, (uint32_t)kEstH)), block(256);
  hipLaunchKernelGGL(k_variance_estimate, grid, block, 0, s, width, height, color, nd, pos, variance, n_phi, p_phi);
}

void launch_variance_prefilter(hipStream_t s, uint32_t width, uint32_t height, const float* variance, float* prefiltered,
                               unsigned long long* stats)
{
  hipLaunchKernelGGL(k_variance_prefilter, dim3(div_up_var(width * height, 256u)), dim3(256), 0, s, width, height, variance, prefiltered, stats);
}

void launch_denoise_var_pass(hipStream_t s, const DCamera& cam, uint32_t pix_count, const float4* color, const float* variance,
                             const float4* nd, const float4* pos, float4* out, float* variance_out, int step_width, DDenoiseVar params)
{
  if (params.variant == 1 || step_width > 32 || (step_width & (step_width - 1)) != 0) {  // taps through L1 / L2
    const uint32_t tiles = div_up_var(cam.width, 16u) * div_up_var(cam.height, 16u);
    hipLaunchKernelGGL(k_denoise_var, dim3(tiles), dim3(256), 0, s, cam, pix_count, color, variance, nd, pos, out, variance_out, step_width,
                       params);
    return;
  }
  const uint32_t st = (uint32_t)step_width;
  const uint32_t total = div_up_var(cam.width, (uint32_t)kDenVarW) * div_up_var(div_up_var(cam.height, st), (uint32_t)kDenVarRows) * st;
  const dim3 grid(div_up_var(total, 8u) * 8u), block(256);  // one contiguous eighth of the tiles per XCD (see k_denoise_lds)
  const size_t lds = (size_t)(kDenVarW + 2 * kDenVarHalo * step_width) * (size_t)(kDenVarRows + 2 * kDenVarHalo) * 40u;
#define PT_VAR_PASS(S) \
  hipLaunchKernelGGL(k_denoise_var_lds<S>, grid, block, lds, s, cam, pix_count, color, variance, nd, pos, out, variance_out, params)
  switch (step_width) {
  case 1: PT_VAR_PASS(1); break;
  case 2: PT_VAR_PASS(2); break;
  case 4: PT_VAR_PASS(4); break;
  case 8: PT_VAR_PASS(8); break;
  case 16: PT_VAR_PASS(16); break;
  default: PT_VAR_PASS(32); break;
  }
#undef PT_VAR_PASS
}

}  // namespace pt
