// path_tracer.hpp -- C++ host mirror of the reference's `class PathTracer`
// (/root/reference/src/lib/path_tracer.hpp:60-99) over the C ABI of libptcore.so (include/ptcore.h).
// Same public methods and mutable fields, so a caller written against the reference class (its CLI,
// cli/cli.cpp:86-105, or its GUI) compiles against this one.  Header-only; errors become exceptions
// (the reference exits the process: cuda_utils/cuda_check.cpp:7-23).
#pragma once

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ptcore.h"
#include "png_image.hpp"
#include "scene_description.hpp"

namespace hip_pt {

struct UResolution {  // resolution.hpp:13-22
  unsigned int width = 0;
  unsigned int height = 0;
};

enum class DisplayBufferType { final, color, normal, depth };  // path_tracer.hpp:19
enum class GPUMethod { megakernel, streaming };                // path_tracer.hpp:57

struct EdgeAvoidingATrousDenoiser {  // denoising/edge_avoiding_a_trous_denoiser.hpp:7-12
  int filter_size = 10;
  float color_weight = 0.45f;
  float normal_weight = 0.30f;
  float position_weight = 0.25f;
};

struct uchar4 {
  unsigned char x, y, z, w;
};

class PathTracer {
public:
  int max_iterations = 1;
  GPUMethod current_gpu_method = GPUMethod::streaming;
  bool direct_light = false;  // a light sample at every diffuse hit (megakernel method only; ptc_set_param "direct_light")
  // an environment sample at every diffuse hit (megakernel method only; ptc_set_param "environment_light")
  bool environment_light = false;
  // the balance heuristic between light samples and the path's own ray (megakernel method only; ptc_set_param "mis")
  bool mis = false;
  // smooth shading (megakernel method only; ptc_set_param "smooth_normals"): triangle hits are shaded with the
  // interpolated vertex normal.  Set before create_buffers it also makes create_buffers compute and set the scene's vertex normals
  // (compute_vertex_normals); vertex normals of the caller's own go through set_vertex_normals after create_buffers.
  bool smooth_normals = false;
  // image textures (megakernel method only; ptc_set_param "textures"): a triangle hit on a diffuse or metal material
  // with a texture bound takes its colour from the texel at the interpolated coordinate.  Textures and coordinates go through
  // set_textures and set_texcoords after create_buffers; without either the flag changes nothing.
  bool textures = false;
  // normal maps (megakernel method only; ptc_set_param "normal_maps"): a triangle hit on a diffuse or metal material
  // with a normal map bound shades with the map's normal.  The binding goes through set_normal_maps after set_textures; without
  // textures, coordinates or a binding the flag changes nothing.  Independent of `textures`.
  bool normal_maps = false;
  // the denoiser's albedo factorisation (ptc_set_param "denoise_albedo"): denoise filters the colour divided by the
  // first-hit albedo and multiplies it back, so that a texture's detail passes the filter.  Both methods.
  bool denoise_albedo = false;
  // the variance-guided passes (ptc_set_param "denoise_variance"): denoise estimates a per-pixel variance of the plane
  // it filters and divides the colour distance by denoise_variance_sigma x that, not by the constant color_weight.  Both methods.
  bool denoise_variance = false;
  float denoise_variance_sigma = 16.0f;  // finite and > 0 (ptc_set_denoise_variance)
  int roulette = 0;  // Russian roulette at every bounce >= this but the last, 0 = off (both methods; ptc_set_param "roulette", [0, 64])
  // the thin lens (ptc_set_lens): aperture radius (0 = the pinhole, the default) and the distance of the plane in
  // focus, world units; both methods
  struct Lens {
    float radius = 0.0f, focus_distance = 1.0f;
    bool operator!=(const Lens& o) const { return radius != o.radius || focus_distance != o.focus_distance; }
  } lens;
  // environment lighting (ptc_set_environment): an octahedral HDR map (hdr_image.hpp: load_environment makes one
  // from an equirectangular .hdr), or null = the reference's gradient, the default; both methods.  Pushed when the pointer changes.
  std::shared_ptr<const EnvironmentMap> environment;
  // the display transform (ptc_set_display): exposure (manual or metered), a tone curve and the reference's
  // encoding, where send_to_preview shows radiance (final, color).  The default is the reference display.  Pushed by send_to_preview.
  ptc_display_params display{PTC_CURVE_CLAMP, 0, 1.0f, 0.18f, 4.0f, 50u, 950u};
  EdgeAvoidingATrousDenoiser atrous_denoiser{};
  int max_bounces = 50;  // reference: compile-time constant, path_tracer.cu:27

  explicit PathTracer(int device = 0)
  {
    ptc_config cfg{device, max_bounces, PTC_METHOD_STREAMING, 0};
    if (ptc_create(&cfg, &ctx_) < 0) throw std::runtime_error(std::string("ptc_create: ") + ptc_last_error(nullptr));
  }
  ~PathTracer() { ptc_destroy(ctx_); }
  PathTracer(const PathTracer&) = delete;
  PathTracer& operator=(const PathTracer&) = delete;

  void restart() { check(ptc_restart(ctx_), "restart"); }
  [[nodiscard]] int iteration() const noexcept { return ptc_iteration(ctx_); }
  void resize_image(UResolution r) { check(ptc_resize(ctx_, r.width, r.height), "resize_image"); }

  void create_buffers(UResolution r, const SceneDescription& scene)
  {
    const FlatScene flat = scene.build_scene();
    ptc_scene_desc d{};
    d.objects = flat.objects.data();
    d.object_count = (uint32_t)flat.objects.size();
    d.object_material_indices = flat.object_material_indices.data();
    d.spheres = flat.spheres.data();
    d.sphere_count = (uint32_t)flat.spheres.size();
    d.materials = flat.materials.data();
    d.material_count = (uint32_t)flat.materials.size();
    d.positions = flat.positions.data();
    d.vertex_count = (uint32_t)(flat.positions.size() / 3);
    d.indices = flat.indices.data();
    d.index_count = (uint32_t)flat.indices.size();
    check(ptc_upload_scene(ctx_, &d), "create_buffers");
    if (smooth_normals && !flat.indices.empty()) set_vertex_normals(compute_vertex_normals(flat));  // (a new scene starts without normals)
    // what the scene file says about textures (a new scene starts without): the materials' pictures, read here (png_image.hpp flips
    // the rows), and the mesh's per-corner coordinates
    if (!flat.textures.empty()) {
      std::vector<PngImage> pictures;
      std::vector<ptc_texture_desc> descs;
      for (const TextureSource& src : flat.textures) pictures.push_back(read_png(src.file));
      for (size_t i = 0; i < pictures.size(); ++i)
        descs.push_back(ptc_texture_desc{pictures[i].rgba.data(), (uint32_t)pictures[i].width, (uint32_t)pictures[i].height, flat.textures[i].encoding,
                                         flat.textures[i].filter, flat.textures[i].wrap});
      set_textures(descs, flat.material_texture);
      if (!flat.material_normal_map.empty()) set_normal_maps(flat.material_normal_map);
    }
    if (!flat.texcoords.empty()) set_texcoords(flat.texcoords);
    resize_image(r);
  }

  // area-weighted vertex normals of the scene's mesh (ptc_compute_vertex_normals; host only): three floats per vertex
  [[nodiscard]] static std::vector<float> compute_vertex_normals(const FlatScene& flat)
  {
    std::vector<float> normals(flat.positions.size(), 0.0f);
    if (ptc_compute_vertex_normals(flat.positions.data(), (uint32_t)(flat.positions.size() / 3), flat.indices.data(), (uint32_t)flat.indices.size(),
                                   normals.data()) < 0)
      throw std::runtime_error(std::string("compute_vertex_normals: ") + ptc_last_error(nullptr));
    return normals;
  }
  // the uploaded scene's vertex normals (ptc_set_vertex_normals): three floats per vertex of the scene; an empty vector removes them
  void set_vertex_normals(const std::vector<float>& normals)
  {
    check(ptc_set_vertex_normals(ctx_, normals.empty() ? nullptr : normals.data(), (uint32_t)(normals.size() / 3)), "vertex_normals");
  }
  [[nodiscard]] ptc_smooth_loop_stats smooth_loop_stats() const
  {
    ptc_smooth_loop_stats s{};
    check(ptc_get_smooth_loop_stats(ctx_, &s), "smooth_loop_stats");
    return s;
  }
  // the uploaded scene's textures and, per material, -1 or the texture bound to it (ptc_set_textures); no textures removes them
  void set_textures(const std::vector<ptc_texture_desc>& textures_in, const std::vector<int32_t>& material_texture)
  {
    check(ptc_set_textures(ctx_, textures_in.empty() ? nullptr : textures_in.data(), (uint32_t)textures_in.size(), material_texture.data(),
                           (uint32_t)material_texture.size()),
          "textures");
  }
  // the uploaded scene's texture coordinates (ptc_set_texcoords): two floats per triangle corner, parallel to the scene's indices; an
  // empty vector removes them
  void set_texcoords(const std::vector<float>& st)
  {
    check(ptc_set_texcoords(ctx_, st.empty() ? nullptr : st.data(), (uint32_t)(st.size() / 2)), "texcoords");
  }
  // per material of the uploaded scene -1 or the texture that is its normal map (ptc_set_normal_maps), after set_textures, which drops
  // the binding; an empty vector removes it
  void set_normal_maps(const std::vector<int32_t>& material_normal_map)
  {
    check(ptc_set_normal_maps(ctx_, material_normal_map.empty() ? nullptr : material_normal_map.data(), (uint32_t)material_normal_map.size()),
          "normal_maps");
  }
  [[nodiscard]] ptc_normal_map_loop_stats normal_map_loop_stats() const
  {
    ptc_normal_map_loop_stats s{};
    check(ptc_get_normal_map_loop_stats(ctx_, &s), "normal_map_loop_stats");
    return s;
  }
  // the normal the loop would shade with at the closest hit, from what is set (ptc_hit_shading_normal): rays 8 floats each; per ray
  // three floats and an outcome byte (0 miss, 1 no map applied, 2 bent, 3 flat, 4 kept)
  struct HitShadingNormal {
    std::vector<float> normal;
    std::vector<uint8_t> outcome;
  };
  [[nodiscard]] HitShadingNormal hit_shading_normal(const std::vector<float>& rays)
  {
    push_fields();
    const uint32_t n = (uint32_t)(rays.size() / 8);
    HitShadingNormal out{std::vector<float>(3u * (size_t)n), std::vector<uint8_t>(n)};
    check(ptc_hit_shading_normal(ctx_, rays.data(), n, out.normal.data(), out.outcome.data()), "hit_shading_normal");
    return out;
  }
  // host only: the normal maps' decode table (ptc_normal_map_decode_table), 256 floats
  [[nodiscard]] static std::vector<float> normal_map_decode_table()
  {
    std::vector<float> table(256);
    if (ptc_normal_map_decode_table(table.data()) < 0) throw std::runtime_error(std::string("normal_map_decode_table: ") + ptc_last_error(nullptr));
    return table;
  }
  [[nodiscard]] ptc_texture_loop_stats texture_loop_stats() const
  {
    ptc_texture_loop_stats s{};
    check(ptc_get_texture_loop_stats(ctx_, &s), "texture_loop_stats");
    return s;
  }
  // the lookup of one of the scene's textures on the device (ptc_sample_texture): st two floats a pair -> three floats a pair
  [[nodiscard]] std::vector<float> sample_texture(uint32_t texture, const std::vector<float>& st)
  {
    push_fields();
    std::vector<float> rgb(3u * (st.size() / 2));
    check(ptc_sample_texture(ctx_, texture, st.data(), (uint32_t)(st.size() / 2), rgb.data(), nullptr), "sample_texture");
    return rgb;
  }
  // the closest hit's texture coordinate and albedo (ptc_hit_surface): rays 8 floats each; per ray (s, t) and three floats
  struct HitSurface {
    std::vector<float> st, albedo;
  };
  [[nodiscard]] HitSurface hit_surface(const std::vector<float>& rays)
  {
    push_fields();
    const uint32_t n = (uint32_t)(rays.size() / 8);
    HitSurface out{std::vector<float>(2u * (size_t)n), std::vector<float>(3u * (size_t)n)};
    check(ptc_hit_surface(ctx_, rays.data(), n, out.st.data(), out.albedo.data()), "hit_surface");
    return out;
  }
  // the closest hit's primitive and attributes (ptc_hit_attributes): rays 8 floats each; per ray object, triangle, (u, v), normal
  struct HitAttributes {
    std::vector<uint32_t> object, triangle;
    std::vector<float> uv, normal;
  };
  [[nodiscard]] HitAttributes hit_attributes(const std::vector<float>& rays)
  {
    push_fields();
    const uint32_t n = (uint32_t)(rays.size() / 8);
    HitAttributes out{std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<float>(2u * (size_t)n), std::vector<float>(3u * (size_t)n)};
    check(ptc_hit_attributes(ctx_, rays.data(), n, out.object.data(), out.triangle.data(), out.uv.data(), out.normal.data()), "hit_attributes");
    return out;
  }

  void path_trace(const Camera& camera, UResolution)
  {
    push_fields();
    const ptc_camera c = camera.to_c();
    check(ptc_trace(ctx_, &c), "path_trace");
  }
  void denoise(UResolution)
  {
    push_fields();
    check(ptc_denoise(ctx_), "denoise");
  }
  // the albedo stage alone (ptc_denoise_albedo), whatever denoise_albedo says: per pixel three floats of albedo, three of irradiance and
  // the eight of the pixel-centre ray the kernel walked
  struct DenoiseAlbedo {
    std::vector<float> albedo, irradiance, rays;
  };
  [[nodiscard]] DenoiseAlbedo denoise_albedo_planes(UResolution resolution)
  {
    push_fields();
    const size_t n = (size_t)resolution.width * resolution.height;
    DenoiseAlbedo out{std::vector<float>(3u * n), std::vector<float>(3u * n), std::vector<float>(8u * n)};
    check(ptc_denoise_albedo(ctx_, out.albedo.data(), out.irradiance.data(), out.rays.data()), "denoise_albedo");
    return out;
  }
  // the estimate stage alone (ptc_denoise_variance), whatever denoise_variance says: per pixel the variance and its 3 x 3 Gaussian
  struct DenoiseVariance {
    std::vector<float> variance, prefiltered;
  };
  [[nodiscard]] DenoiseVariance denoise_variance_planes(UResolution resolution)
  {
    push_fields();
    const size_t n = (size_t)resolution.width * resolution.height;
    DenoiseVariance out{std::vector<float>(n), std::vector<float>(n)};
    check(ptc_denoise_variance(ctx_, out.variance.data(), out.prefiltered.data()), "denoise_variance");
    return out;
  }
  [[nodiscard]] ptc_denoise_variance_stats denoise_variance_stats() const
  {
    ptc_denoise_variance_stats s{};
    check(ptc_get_denoise_variance_stats(ctx_, &s), "denoise_variance_stats");
    return s;
  }
  // the whole mode on the host from caller planes (ptc_check_denoise_variance; no GPU): colour and normal 3 floats a pixel, depth one
  static void check_denoise_variance(const std::vector<float>& colour, const std::vector<float>& normal, const std::vector<float>& depth,
                                     const ptc_camera& camera, UResolution resolution, const ptc_denoiser_params& weights, float sigma,
                                     std::vector<float>& variance_out, std::vector<float>& result_out)
  {
    const size_t n = (size_t)resolution.width * resolution.height;
    if (colour.size() != 3u * n || normal.size() != 3u * n || depth.size() != n) throw std::runtime_error("check_denoise_variance: plane sizes");
    variance_out.assign(n, 0.0f);
    result_out.assign(3u * n, 0.0f);
    if (ptc_check_denoise_variance(colour.data(), normal.data(), depth.data(), &camera, resolution.width, resolution.height, &weights, sigma,
                                   variance_out.data(), result_out.data()) != PTC_OK)
      throw std::runtime_error("check_denoise_variance: refused");
  }
  [[nodiscard]] ptc_denoise_albedo_stats denoise_albedo_stats() const
  {
    ptc_denoise_albedo_stats s{};
    check(ptc_get_denoise_albedo_stats(ctx_, &s), "denoise_albedo_stats");
    return s;
  }
  // dst: device (or managed) pointer like the reference's PBO when dst_is_device, else host memory
  void send_to_preview(uchar4* dst, UResolution, DisplayBufferType type = DisplayBufferType::final,
                       bool dst_is_device = false) const
  {
    check(ptc_set_display(ctx_, &display), "display");
    check(ptc_present_rgba8(ctx_, dst, dst_is_device ? 1 : 0, static_cast<int>(type)), "send_to_preview");
  }
  // of the last send_to_preview that went through the display transform (ptc_get_exposure_info)
  [[nodiscard]] ptc_exposure_info exposure_info() const
  {
    ptc_exposure_info info{};
    check(ptc_get_exposure_info(ctx_, &info), "exposure_info");
    return info;
  }
  void synchronize() { check(ptc_synchronize(ctx_), "synchronize"); }
  [[nodiscard]] ptc_stats stats() const
  {
    ptc_stats s{};
    check(ptc_get_stats(ctx_, &s), "stats");
    return s;
  }
  ptc_ctx* handle() { return ctx_; }

private:
  void push_fields()
  {
    check(ptc_set_max_iterations(ctx_, max_iterations), "max_iterations");
    check(ptc_set_method(ctx_, current_gpu_method == GPUMethod::megakernel ? PTC_METHOD_MEGAKERNEL : PTC_METHOD_STREAMING), "method");
    if (direct_light != direct_light_pushed_) {  // (ptc_set_param flushes queued frames: only on a change)
      check(ptc_set_param(ctx_, "direct_light", direct_light ? 1 : 0), "direct_light");
      direct_light_pushed_ = direct_light;
    }
    if (environment_light != environment_light_pushed_) {
      check(ptc_set_param(ctx_, "environment_light", environment_light ? 1 : 0), "environment_light");
      environment_light_pushed_ = environment_light;
    }
    if (mis != mis_pushed_) {
      check(ptc_set_param(ctx_, "mis", mis ? 1 : 0), "mis");
      mis_pushed_ = mis;
    }
    if (smooth_normals != smooth_normals_pushed_) {
      check(ptc_set_param(ctx_, "smooth_normals", smooth_normals ? 1 : 0), "smooth_normals");
      smooth_normals_pushed_ = smooth_normals;
    }
    if (textures != textures_pushed_) {
      check(ptc_set_param(ctx_, "textures", textures ? 1 : 0), "textures");
      textures_pushed_ = textures;
    }
    if (normal_maps != normal_maps_pushed_) {
      check(ptc_set_param(ctx_, "normal_maps", normal_maps ? 1 : 0), "normal_maps");
      normal_maps_pushed_ = normal_maps;
    }
    if (denoise_albedo != denoise_albedo_pushed_) {
      check(ptc_set_param(ctx_, "denoise_albedo", denoise_albedo ? 1 : 0), "denoise_albedo");
      denoise_albedo_pushed_ = denoise_albedo;
    }
    if (denoise_variance != denoise_variance_pushed_) {
      check(ptc_set_param(ctx_, "denoise_variance", denoise_variance ? 1 : 0), "denoise_variance");
      denoise_variance_pushed_ = denoise_variance;
    }
    if (denoise_variance_sigma != denoise_variance_sigma_pushed_) {
      check(ptc_set_denoise_variance(ctx_, denoise_variance_sigma), "denoise_variance_sigma");
      denoise_variance_sigma_pushed_ = denoise_variance_sigma;
    }
    if (roulette != roulette_pushed_) {
      check(ptc_set_param(ctx_, "roulette", roulette), "roulette");
      roulette_pushed_ = roulette;
    }
    if (lens != lens_pushed_) {  // (ptc_set_lens flushes queued frames too)
      check(ptc_set_lens(ctx_, lens.radius, lens.focus_distance), "lens");
      lens_pushed_ = lens;
    }
    if (environment != environment_pushed_) {  // (ptc_set_environment flushes queued frames too)
      check(ptc_set_environment(ctx_, environment ? environment->rgb.data() : nullptr, environment ? environment->size : 0u), "environment");
      environment_pushed_ = environment;
    }
    check(ptc_set_max_bounces(ctx_, max_bounces), "max_bounces");
    const ptc_denoiser_params p{atrous_denoiser.filter_size, atrous_denoiser.color_weight, atrous_denoiser.normal_weight,
                                atrous_denoiser.position_weight};
    check(ptc_set_denoiser_params(ctx_, &p), "denoiser");
  }
  void check(int rc, const char* what) const
  {
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + ptc_last_error(ctx_));
  }
  ptc_ctx* ctx_ = nullptr;
  bool direct_light_pushed_ = false;
  bool environment_light_pushed_ = false;
  bool mis_pushed_ = false;
  bool smooth_normals_pushed_ = false;
  bool textures_pushed_ = false;
  bool normal_maps_pushed_ = false;
  bool denoise_albedo_pushed_ = false;
  bool denoise_variance_pushed_ = false;
  float denoise_variance_sigma_pushed_ = 16.0f;
  int roulette_pushed_ = 0;
  Lens lens_pushed_{};
  std::shared_ptr<const EnvironmentMap> environment_pushed_;
};

}  // namespace hip_pt
