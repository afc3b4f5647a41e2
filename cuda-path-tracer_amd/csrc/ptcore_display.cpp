// ptcore_display.cpp -- the display transform on the host: ptc_set_display / ptc_get_display and their refusals,
// show_display (what ptc_present_rgba8 and ptc_gather_present_rgba8 launch under a display that is not the reference's),
// ptc_get_exposure_info, ptc_tonemap_buffer (the same launches on a caller's buffer), and the rule on the host with no GPU
// (ptc_check_display_meter, ptc_check_display_map: pt_display.hpp's functions, the ones the kernels call).  Part of libptcore.so
// (ptcore_ctx.hpp).
#include "ptcore_ctx.hpp"
#include "pt_display.hpp"

using namespace pt;
using namespace ptcd;

static_assert(PTC_CURVE_CLAMP == display_rules::kCurveClamp && PTC_CURVE_REINHARD == display_rules::kCurveReinhard &&
                  PTC_CURVE_ACES == display_rules::kCurveAces,
              "pt_display.hpp restates ptc_curve");
static_assert(sizeof(((ptc_exposure_info*)nullptr)->histogram) == sizeof(((DExposure*)nullptr)->hist) &&
                  sizeof(((DMeter*)nullptr)->hist) == display_rules::kBins * sizeof(uint32_t),
              "256 bins on the device, on the host and in the ABI");

namespace {

// Why ptc_set_display refuses d, naming the field; empty: it does not.
std::string display_refusal(const ptc_display_params& d)
{
  const auto positive = [](const char* name, float v) {
    return std::isfinite(v) && v > 0.0f ? std::string() : std::string(name) + " must be finite and > 0, got " + std::to_string(v);
  };
  if (d.curve < PTC_CURVE_CLAMP || d.curve > PTC_CURVE_ACES) return "curve must be 0 (clamp), 1 (reinhard) or 2 (aces), got " + std::to_string(d.curve);
  if (d.metering != 0 && d.metering != 1) return "metering must be 0 or 1, got " + std::to_string(d.metering);
  for (const std::string& s : {positive("exposure", d.exposure), positive("key", d.key), positive("white", d.white)})
    if (!s.empty()) return s;
  if (d.high_permille > 1000u) return "high_permille must be at most 1000, got " + std::to_string(d.high_permille);
  if (d.low_permille >= d.high_permille)
    return "low_permille must be below high_permille, got " + std::to_string(d.low_permille) + " and " + std::to_string(d.high_permille);
  return std::string();
}

void info_of(const DExposure& e, ptc_exposure_info* out)
{
  out->pixels = e.pixels;
  out->counted = e.counted;
  out->below = e.below;
  out->rejected = e.rejected;
  out->level_bin = e.level_bin;
  out->level = e.level;
  out->scale = e.scale;
  std::memcpy(out->histogram, e.hist, sizeof e.hist);
}

// what a call under manual metering reports: nothing counted, the exposure as the factor
DExposure manual_exposure(uint32_t n, float exposure)
{
  DExposure e{};
  e.pixels = n;
  e.level_bin = -1;
  e.scale = exposure;
  return e;
}

// the context's accumulation words and result block, allocated (and the words zeroed) by the first call that shows anything
int display_state(ptc_ctx* ctx)
{
  if (ctx->meter_dev) return PTC_OK;
  void* p = nullptr;
  HIP_TRY(ctx, hipMalloc(&p, sizeof(DMeter) + sizeof(DExposure)));
  if (hipMemset(p, 0, sizeof(DMeter) + sizeof(DExposure)) != hipSuccess) {
    (void)hipFree(p);
    return fail(ctx, PTC_ERR_HIP, "hipMemset(display state) failed");
  }
  ctx->meter_dev = static_cast<DMeter*>(p);
  ctx->exposure_dev = reinterpret_cast<DExposure*>(static_cast<char*>(p) + sizeof(DMeter));
  return PTC_OK;
}

}  // namespace

namespace ptcd {

bool reference_display(const ptc_display_params& d) { return d.curve == PTC_CURVE_CLAMP && d.metering == 0 && d.exposure == 1.0f; }

int show_display(ptc_ctx* ctx, const float4* src4, const float* src3, uint32_t n, uint32_t* rgba, float* mapped, DExposure* shown)
{
  const ptc_display_params& d = ctx->display;
  const float w2 = d.white * d.white;
  if (d.metering) {
    if (int rc = display_state(ctx)) return rc;
    launch_meter(ctx->stream, src4, src3, n, ctx->meter_dev);
    launch_meter_level(ctx->stream, ctx->meter_dev, ctx->exposure_dev, n, d.low_permille, d.high_permille, d.key, d.exposure);
    launch_tonemap(ctx->stream, src4, src3, n, ctx->exposure_dev, 0.0f, d.curve, w2, rgba, mapped);
    if (int rc = check_last(ctx, "display")) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(shown, ctx->exposure_dev, sizeof(DExposure), hipMemcpyDeviceToHost, ctx->stream));
    return PTC_OK;
  }
  launch_tonemap(ctx->stream, src4, src3, n, nullptr, d.exposure, d.curve, w2, rgba, mapped);
  *shown = manual_exposure(n, d.exposure);
  return check_last(ctx, "display");
}

}  // namespace ptcd

extern "C" {

// Checked values only: a refusal leaves the context's display as it was.  Nothing on the device depends on the display until a
// present, so no queued frame needs flushing.
int ptc_set_display(ptc_ctx* ctx, const ptc_display_params* display)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!display) return fail(ctx, PTC_ERR_INVALID, "display is NULL");
  const std::string why = display_refusal(*display);
  if (!why.empty()) return fail(ctx, PTC_ERR_INVALID, why);
  ctx->display = *display;
  return PTC_OK;
}

int ptc_get_display(ptc_ctx* ctx, ptc_display_params* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  *out = ctx->display;
  return PTC_OK;
}

int ptc_get_exposure_info(ptc_ctx* ctx, ptc_exposure_info* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (!ctx->shown_known) return fail(ctx, PTC_ERR_INVALID, "no present has gone through the display transform");
  info_of(ctx->shown, out);
  return PTC_OK;
}

int ptc_tonemap_buffer(ptc_ctx* ctx, const void* src, int channels, uint32_t pix_count, int src_on_device, void* rgba_out, float* mapped_out,
                       int out_on_device, ptc_exposure_info* info)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!src || !rgba_out) return fail(ctx, PTC_ERR_INVALID, "src or rgba_out is NULL");
  if (channels != 3 && channels != 4) return fail(ctx, PTC_ERR_INVALID, "channels must be 3 or 4");
  if (pix_count == 0u || pix_count > 0x7fffffffu) return fail(ctx, PTC_ERR_INVALID, "pix_count must be in [1, 2^31)");
  if (src_on_device && channels == 4 && (reinterpret_cast<uintptr_t>(src) & 15u) != 0u)
    return fail(ctx, PTC_ERR_INVALID, "a device src of 4 channels must be 16-byte aligned");
  if (int rc = bind_device(ctx)) return rc;
  struct Pool {
    std::vector<void*> p;
    ~Pool() { free_pool(p); }
  } pool;
  const size_t P = pix_count;
  const float* in = static_cast<const float*>(src);
  if (!src_on_device) {
    float* dev = nullptr;
    if (int rc = dev_alloc(ctx, pool.p, &dev, P * (size_t)channels)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(dev, src, P * (size_t)channels * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    in = dev;
  }
  uint32_t* rgba = static_cast<uint32_t*>(rgba_out);
  float* mapped = mapped_out;
  if (!out_on_device) {
    if (int rc = dev_alloc(ctx, pool.p, &rgba, P)) return rc;
    if (mapped_out)
      if (int rc = dev_alloc(ctx, pool.p, &mapped, P * 3u)) return rc;
  }
  const float4* src4 = channels == 4 ? reinterpret_cast<const float4*>(in) : nullptr;
  const float* src3 = channels == 3 ? in : nullptr;
  DExposure shown{};
  if (int rc = show_display(ctx, src4, src3, pix_count, rgba, mapped, &shown)) {
    (void)hipStreamSynchronize(ctx->stream);  // (`shown` and the pool outlive what was enqueued)
    return rc;
  }
  hipError_t e = hipSuccess;
  if (!out_on_device) {
    e = hipMemcpyAsync(rgba_out, rgba, P * 4u, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && mapped_out) e = hipMemcpyAsync(mapped_out, mapped, P * 3u * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  }
  const hipError_t waited = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = waited;
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("tonemap buffer: ") + hipGetErrorString(e));
  if (info) info_of(shown, info);
  return PTC_OK;
}

int ptc_check_display_params(const ptc_display_params* params, char* why, uint32_t capacity)
{
  if (!params) return PTC_ERR_INVALID;
  const std::string refusal = display_refusal(*params);
  if (why && capacity) std::snprintf(why, capacity, "%s", refusal.c_str());
  return refusal.empty() ? PTC_OK : PTC_ERR_INVALID;
}

// The metering of pt_display.hpp on the host, as k_meter and k_meter_level run it: no GPU, no context.  ptc_set_display's refusals,
// without a message.
int ptc_check_display_meter(const ptc_display_params* params, const float* rgb, int channels, uint32_t count, ptc_exposure_info* info_out)
{
  if (!params || !info_out || (channels != 3 && channels != 4) || (count != 0u && !rgb)) return PTC_ERR_INVALID;
  if (!display_refusal(*params).empty()) return PTC_ERR_INVALID;
  if (!params->metering) {
    info_of(manual_exposure(count, params->exposure), info_out);
    return PTC_OK;
  }
  DExposure e{};
  e.pixels = count;
  for (uint32_t i = 0; i < count; ++i) {
    const float* p = rgb + (size_t)i * (size_t)channels;
    const int bin = display_rules::bin_of(p[0], p[1], p[2]);
    if (bin >= 0) e.hist[bin] += 1u;
    else if (bin == display_rules::kBelow) e.below += 1u;
    else e.rejected += 1u;
  }
  uint64_t counted = 0;
  e.level_bin = display_rules::level_bin(e.hist, params->low_permille, params->high_permille, &counted);
  e.counted = (uint32_t)counted;
  e.level = e.level_bin < 0 ? 0.0f : display_rules::level_of(e.level_bin);
  e.scale = display_rules::scale_of(e.level_bin, params->key, params->exposure);
  info_of(e, info_out);
  return PTC_OK;
}

// ... and the curve, as k_tonemap runs it, under a scale of the caller's
int ptc_check_display_map(const ptc_display_params* params, float scale, const float* rgb, int channels, uint32_t count, float* mapped_out)
{
  if (!params || (channels != 3 && channels != 4) || (count != 0u && (!rgb || !mapped_out))) return PTC_ERR_INVALID;
  if (!display_refusal(*params).empty()) return PTC_ERR_INVALID;
  const float w2 = params->white * params->white;
  for (uint32_t i = 0; i < count; ++i)
    for (uint32_t c = 0; c < 3u; ++c)
      mapped_out[3u * (size_t)i + c] = display_rules::map_channel(rgb[(size_t)i * (size_t)channels + c], scale, params->curve, w2);
  return PTC_OK;
}

}  // extern "C"
