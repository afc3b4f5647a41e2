// pt_megakernel.inc -- the megakernel's loop, the whole path in one thread: mega_path, and k_megakernel around it.  Included (inside
// namespace pt, after pt_kernels_common.inc and with pt_light_sample.hpp in front) by pt_kernels.hip, which instantiates the plain
// instances beside the closest-hit kernels as ever, and by pt_mega_direct.hip, which instantiates the kRoulette ones and
// k_megakernel_direct, and by pt_mega_mis.hip, which instantiates k_megakernel_mis (kMis, DESIGN section 5l), and by pt_mega_smooth.hip,
// which instantiates k_megakernel_smooth (kSmooth, section 5n), and by pt_mega_tex.hip, which instantiates k_megakernel_tex (kTex,
// section 5o): the code object that holds the traversal kernels stays the one it was (DESIGN section 5h).
// path_tracing_mega_kernel, path_tracer.cu:227-269: the whole path in one thread, one RNG stream per
// pixel (a different image from streaming mode at the same seed -- a property of the reference).
// kEmit: the scene has an emissive material (the host's choice; without one the instance is the reference's loop as it was).
// kRoulette: Russian roulette from bounce `roulette` on, the last bounce excepted (DESIGN section 5h; the host picks the instance
// when some bounce plays): after the emitter check and before evaluate_material, on the roulette stream of the pixel.  A path that
// ends there leaves colour 0 and makes no draw.
// kDirect (with kEmit; DESIGN section 5g): one light sample (section 5f, pt_light_sample.hpp) and one shadow ray at every diffuse
// hit, a per-path radiance sum and the emission gate that keeps a lamp from being counted twice -- and nothing else.  The shadow
// ray takes the per-thread any-hit walk (scene_occluded) on the thread's own LDS stack, which is free while it runs.  The light
// samples draw from a stream of their own (path_seed(pixel, iteration) ^ kLightSeedXor, draws 3b .. 3b + 2 at bounce b), so every
// material draw, every closest hit, the normal and depth planes and rays_total are those of the plain loop at the same iteration:
// only the colour differs.  A path roulette ends takes no light sample at that hit and adds nothing to the three loop counters; a
// survivor's light sample is weighted with the divided colour.  tests/direct_loop_ref.py restates the loop in numpy.
// stats (kDirect): kLightStatLines lines of kLoopStatWords 64-bit words; word 0 += diffuse hits, word 1 += shadow rays traced,
// word 2 += unoccluded ones.  stack: the calling thread's column of the workgroup's LDS stack.
// kLens (DESIGN section 5i): the primary ray is the thin lens's, primary_ray<true> with `lens`; rng is left where the pinhole leaves it,
// so every material draw is the pinhole render's.  The lens instances (k_megakernel_lens, k_megakernel_direct_lens) live in
// pt_mega_direct.hip.
// kEnv (ptc_set_environment, DESIGN section 5j): a miss takes the environment, sky<true>(ray.d, env), at every bounce and whatever
// count_emission says, as the gradient does; the environment is no lamp and draws no light sample.  An environment instance serves
// pinhole and lens alike -- lens.radius > 0 decides per launch, kLens is not read -- and is built with kEmit and kRoulette on (a scene
// without emitters meets no emitter; `roulette` >= max_bounces plays at no bounce: the same bits): k_megakernel_env<kDirect>,
// pt_mega_direct.hip.
// kEnvLight (with kEnv and kDirect; ptc_set_param "environment_light", DESIGN section 5k): the environment is a light as well.  Every
// diffuse hit draws one environment sample (env_light::sample_point, pt_env_light.hpp; the stream path_seed(pixel, iteration) ^
// kEnvLightSeedXor, draws 4b .. 4b + 3 at bounce b) behind the lamp's, with a shadow ray of its own on the same LDS stack, and a miss
// counts the environment only when the vertex before it drew no environment sample -- section 5g's gate in a flag of its own,
// count_env.  The lamps are a run-time choice here: lt.records null (a wave-uniform kernel argument) is a frame without "direct_light"
// or without a lamp table, which draws no lamp sample and counts every emitter.  stats words 3 .. 5 += diffuse hits that drew an
// environment sample, its shadow rays, the unoccluded ones.  k_megakernel_env_light, pt_mega_direct.hip.
// kMis (with kEnvLight; ptc_set_param "mis", DESIGN section 5l; k_megakernel_mis, pt_mega_mis.hip): the balance heuristic between each
// light sample and the path's own continuation ray at diffuse vertices.  One more float of path state, bsdf_pdf -- the cosine lobe's
// density of the direction evaluate_material drew, read only while count_emission or count_env is false.  A lamp's and the
// environment's sample are weighted against the lobe's density of their direction (not at the last bounce, which has no continuation
// ray); an emitter hit and a miss behind a diffuse vertex count with the lobe's weight against the light sampler's density of that
// hit instead of 0: mis.inv_pdf_m[material], loaded beside the material, and env_light::density, whose load stands in front of the
// sky's texel loads.  Here the environment light is a run-time choice as well (el.table null: none) and so is the environment
// (env.texels null: the gradient).  Every draw, every closest hit and shadow ray and the six counters are those of the loop without it.
// stats words 6 and 7 += emitter hits and misses behind a diffuse vertex that were weighted.
// kSmooth (with kEnvLight; ptc_set_param "smooth_normals" in a scene with vertex normals, DESIGN section 5n; k_megakernel_smooth,
// pt_mega_smooth.hip): at a triangle hit the shading normal hn is smooth::shading_normal's (pt_smooth.hpp) of the winner's three
// vertex normals -- the closest hit reports the winner, ray_scene<.., true> -- and takes rec.n's place in the normal plane, in
// evaluate_material, in the light samples and in bsdf_pdf; rec.n stays geometric (side, the lamp-side cosine of an emitter hit).  A
// light sample whose direction lies behind the geometry (dot(w, rec.n) <= 0) counts as not sampled, and a diffuse or metal triangle
// hit whose new direction does (dot(ray.d, rec.n) <= 0) ends the path with colour 0 behind its light samples.  Every light is a
// run-time choice as under kMis, with or without it, and a frame that samples none deposits colour alone.  stats words 8 .. 11 +=
// shading normals formed, fall-backs, absorbed continuations, culled light samples.
// kTex (with kEnvLight; ptc_set_param "textures" in a scene with textures and texture coordinates, DESIGN section 5o; k_megakernel_tex,
// pt_mega_tex.hip): at a triangle hit on a diffuse or metal material with a texture bound, after the emitter check and roulette and
// immediately before evaluate_material, the material is copied and texmap::albedo's (pt_texture.hpp) colour -- the texel at the
// winner's interpolated corner coordinates times p[0..2] -- replaces p[0..2] in the copy; everything downstream takes it from there.
// Every light is a run-time choice as under kSmooth, with kSmooth or without.  stats words 12, 13 += lookups, fall-backs.
template <bool kEmit, bool kRoulette, bool kDirect, bool kLens = false, bool kEnv = false, bool kEnvLight = false, bool kMis = false,
          bool kSmooth = false, bool kTex = false>
__device__ __forceinline__ void mega_path(const DScene& sc, const DLights& lt, const DCamera& cam, const uint32_t iteration, const DBand band,
                                          const uint32_t pix_count, const int max_bounces, const DFrame fb, DeviceCounters* counters,
                                          unsigned long long* stats, const int roulette, uint32_t* stack,
                                          const DLens lens = DLens{0.0f, 0.0f}, const DEnv env = DEnv{nullptr, 0u, 0u},
                                          const DEnvLight el = DEnvLight{nullptr}, const DMis mis = DMis{nullptr},
                                          const DSmooth sm = DSmooth{nullptr, nullptr},
                                          const DTex tx = DTex{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr})
{
  constexpr bool kDyn = kSmooth || kTex;  // every light and the environment are run-time choices
  static_assert(!kTex || kEnvLight, "the textured instances sample lamps and environment by run-time choice");
  static_assert(!kSmooth || kEnvLight, "the smooth instances sample lamps and environment by run-time choice");
  static_assert(!kEnvLight || (kEnv && kDirect), "the environment-light instance has an environment and a radiance sum");
  static_assert(!kMis || kEnvLight, "the multiple-importance instance samples lamps and environment by run-time choice");
  static_assert(kEmit || !kDirect, "direct lighting: launched only for a scene with a lamp table, so with an emissive material");
  const uint32_t s = blockIdx.x * kWave + threadIdx.x;
  uint32_t rays = 0u, flags = 0u;
  uint32_t n_diffuse = 0u, n_shadow = 0u, n_clear = 0u;
  uint32_t e_diffuse = 0u, e_shadow = 0u, e_clear = 0u;
  [[maybe_unused]] uint32_t m_emit = 0u, m_miss = 0u;
  [[maybe_unused]] uint32_t s_formed = 0u, s_fallback = 0u, s_absorbed = 0u, s_culled = 0u;
  [[maybe_unused]] uint32_t t_lookup = 0u, t_fallback = 0u;
  const bool lamps = !kEnvLight || lt.records != nullptr;
  const bool env_lamp = !(kMis || kDyn) || el.table != nullptr;  // (kEnvLight) the environment is sampled
  if (s < pix_count) {
    const uint32_t pixel = band_pixel(band, s);
    Minstd rng;
    Ray ray;
    if constexpr (kEnv) {
      if (lens.radius > 0.0f) primary_ray<true>(cam, pixel, iteration, rng, ray, lens);
      else primary_ray<false>(cam, pixel, iteration, rng, ray);
    } else {
      primary_ray<kLens>(cam, pixel, iteration, rng, ray, lens);
    }
    f3 color = mk3(1.0f, 1.0f, 1.0f);
    f3 radiance = mk3(0.0f, 0.0f, 0.0f);
    bool count_emission = true;  // the last vertex drew no light sample (the camera, metal, glass): a lamp hit from it counts
    bool count_env = true;       // (kEnvLight) ... no environment sample: a miss from it counts the environment
    [[maybe_unused]] float bsdf_pdf = 0.0f;  // (kMis) the lobe's density of ray.d, behind a diffuse vertex
    f3 normal = -ray.d;
    float depth = 1e6f;
    for (int i = 0; i < max_bounces; ++i) {
      Hit rec;
      rec.t = 0.0f;
      rec.p = rec.n = mk3(0.f, 0.f, 0.f);
      rec.mat = 0u;
      rec.side = 0u;
      ++rays;
      Tally tally;
      [[maybe_unused]] HitAttr at;
      if (!ray_scene<false, kDyn>(ray, sc, rec, stack, flags, tally, kDyn ? &at : nullptr)) {
        if constexpr (kMis) {
          if (!count_env) {  // behind an environment sample: the lobe's share of the sky it reached (the entry's load first)
            ++m_miss;
            const float p_e = env_light::density(el.table, env.n, ray.d);
            const f3 seen = color * sky<true>(ray.d, env);
            color = seen * mis::balance(bsdf_pdf, p_e);
          } else {
            color = env.texels ? color * sky<true>(ray.d, env) : color * sky<false>(ray.d, env);
          }
          break;
        }
        if constexpr (kDyn) {  // the environment itself by env.texels
          if (!count_env) color = mk3(0.0f, 0.0f, 0.0f);
          else color = env.texels ? color * sky<true>(ray.d, env) : color * sky<false>(ray.d, env);
          break;
        }
        if (kEnvLight && !count_env) color = mk3(0.0f, 0.0f, 0.0f);  // the environment sample of the vertex before has counted it
        else color = color * sky<kEnv>(ray.d, env);
        break;
      }
      f3 hn = rec.n;  // the shading normal: the geometric one but at a triangle hit under kSmooth
      [[maybe_unused]] bool tri = false;
      if constexpr (kSmooth) {
        if (at.first != kNoChild) {
          tri = true;
          const uint32_t mesh = sc.object_mesh[at.object];
          const uint32_t* idx = sc.mesh_views[mesh].indices + at.first;
          const float* vn = sm.normals + 3u * (size_t)sm.mesh_first_vertex[mesh];
          const f3 n0 = ld3(vn + 3u * (size_t)idx[0]), n1 = ld3(vn + 3u * (size_t)idx[1]), n2 = ld3(vn + 3u * (size_t)idx[2]);
          if (smooth::shading_normal(n0, n1, n2, at.u, at.v, rec.n, ray.d, sc.objects[at.object].inv_m, hn)) ++s_formed;
          else ++s_fallback;
        }
      }
      if (i == 0) {
        normal = hn;
        depth = rec.t;
      }
      bool tmin_flag = ray.tmin != 1e-4f;
      const DMaterial& mat = sc.materials[rec.mat];
      [[maybe_unused]] float inv_pdf_m = 0.0f;
      if constexpr (kMis) {
        if (lamps) inv_pdf_m = mis.inv_pdf_m[rec.mat];
        if (is_emitter(mat)) {  // behind a diffuse vertex: the lobe's share of the lamp it reached, against the lamp sampler's density there
          if (count_emission) {
            color = emit_color(color, mat);
          } else {
            ++m_emit;
            const float cos_l = __builtin_fabsf(dot(rec.n, ray.d));
            const float t2 = rec.t * rec.t;
            const float p_l = mis::lamp_density(t2, cos_l, inv_pdf_m);
            color = emit_color(color, mat) * mis::balance(bsdf_pdf, p_l);
          }
          break;
        }
      }
      if (kEmit && is_emitter(mat)) {  // the path ends at the emitter: no draw; after a diffuse vertex its light sample has counted the lamp
        color = !kDirect || count_emission ? emit_color(color, mat) : mk3(0.0f, 0.0f, 0.0f);
        break;
      }
      if (kRoulette && i >= roulette && i != max_bounces - 1 && roulette_ends(color, pixel, iteration, (uint32_t)i)) {
        color = mk3(0.0f, 0.0f, 0.0f);  // the path ends by chance: the sample is (radiance +) 0, no draw, no light sample
        break;
      }
      if constexpr (kTex) {
        DMaterial tmat = mat;
        if (at.first != kNoChild && mat.type <= 1) {
          const int32_t ti = tx.material_texture[rec.mat];
          if (ti >= 0) {
            const uint32_t mesh = sc.object_mesh[at.object];
            const float* st = tx.st + 2u * ((size_t)tx.mesh_first_index[mesh] + at.first);
            f3 alb;
            if (texmap::albedo(tx.texels, tx.records[ti], tx.table, st, st + 2, st + 4, at.u, at.v, mk3(mat.p[0], mat.p[1], mat.p[2]), alb)) ++t_lookup;
            else ++t_fallback;
            tmat.p[0] = alb.x;
            tmat.p[1] = alb.y;
            tmat.p[2] = alb.z;
          }
        }
        evaluate_material(ray.o, ray.d, tmin_flag, rec.p, hn, rec.side, tmat, rng, color);
      } else {
        evaluate_material(ray.o, ray.d, tmin_flag, rec.p, hn, rec.side, mat, rng, color);
      }
      ray.tmin = tmin_flag ? 1e-5f : 1e-4f;
      if constexpr (kDirect) {
        if (lamps) count_emission = mat.type != 0;
        if constexpr (kEnvLight) {
          if (env_lamp) count_env = mat.type != 0;
        }
        if (mat.type == 0) {  // diffuse: colour is throughput x albedo now; one light sample at the hit, about the unflipped normal
          [[maybe_unused]] env_light::Sample es;  // (kEnvLight) the environment's sample: drawn first, its loads ahead of the lamp's shadow ray
          [[maybe_unused]] const bool weigh = kMis && i != max_bounces - 1;  // the last bounce has no continuation ray to weigh against
          if constexpr (kMis) bsdf_pdf = mis::lobe_density(dot(hn, ray.d));
          if constexpr (kMis) {
            es.sampled = false;
            if (env_lamp) {
              ++e_diffuse;
              env_light::Terms et;
              es = env_light::sample_point(el.table, env.texels, env.n, hn, pixel, iteration, 4u * (uint32_t)i, et);
              if (weigh) es.contrib = es.contrib * mis::balance(env_light::env_density(et.jac), mis::lobe_density(et.cos_r));
            }
          } else if constexpr (kEnvLight) {
            if constexpr (kDyn) es.sampled = false;
            if (env_lamp) {
              ++e_diffuse;
              es = env_light::sample_point(el.table, env.texels, env.n, hn, pixel, iteration, 4u * (uint32_t)i);
            }
          }
          if constexpr (kSmooth) {
            if (tri && es.sampled && dot(es.w, rec.n) <= 0.0f) {  // behind the geometry: not sampled
              es.sampled = false;
              ++s_culled;
            }
          }
          if (lamps) {
            ++n_diffuse;
            [[maybe_unused]] LightTerms lterms;
            LightSample ls;
            if constexpr (kMis) {
              ls = light_sample_point(lt, rec.p, hn, pixel, iteration, 3u * (uint32_t)i, lterms);
              if (weigh)
                ls.contrib = ls.contrib * mis::balance(mis::lamp_density(lterms.d2, lterms.cos_l, lterms.inv_pdf), mis::lobe_density(lterms.cos_r));
            } else {
              ls = light_sample_point(lt, rec.p, hn, pixel, iteration, 3u * (uint32_t)i);
            }
            if constexpr (kSmooth) {
              if (tri && ls.sampled && dot(ls.w, rec.n) <= 0.0f) {
                ls.sampled = false;
                ++s_culled;
              }
            }
            if (ls.sampled) {
              ++n_shadow;
              Ray shadow;
              shadow.o = rec.p;
              shadow.tmin = 1e-4f;
              shadow.d = ls.w;
              shadow.tmax = ls.tmax;
              if (!scene_occluded(shadow, sc, stack, flags)) {
                ++n_clear;
                radiance = radiance + color * ls.contrib;
              }
            }
          }
          if constexpr (kEnvLight) {
            if (es.sampled) {  // ... and its shadow ray behind the lamp's
              ++e_shadow;
              Ray shadow;
              shadow.o = rec.p;
              shadow.tmin = 1e-4f;
              shadow.d = es.w;
              shadow.tmax = es.tmax;
              if (!scene_occluded(shadow, sc, stack, flags)) {
                ++e_clear;
                radiance = radiance + color * es.contrib;
              }
            }
          }
        }
      }
      if constexpr (kSmooth) {
        if (tri && mat.type != 2 && dot(ray.d, rec.n) <= 0.0f) {  // the new direction enters the geometry: absorbed
          ++s_absorbed;
          color = mk3(0.0f, 0.0f, 0.0f);
          break;
        }
      }
    }
    if constexpr (kDyn) accumulate_color(fb.color4, s, iteration, lamps || env_lamp ? radiance + color : color);
    else accumulate_color(fb.color4, s, iteration, kDirect ? radiance + color : color);
    accumulate_nd(fb.nd4, s, iteration, normal, depth);
    if (flags) atomicOr(&counters->flags, flags);
  }
  // one atomic per counter and wavefront; the three loop counters spread over lines (adds to one line serialise in L2)
  uint32_t sum = rays, sd = n_diffuse, ss = n_shadow, sv = n_clear, ed = e_diffuse, es = e_shadow, ev = e_clear;
  [[maybe_unused]] uint32_t me = m_emit, mm = m_miss;
  [[maybe_unused]] uint32_t qf = s_formed, qb = s_fallback, qa = s_absorbed, qc = s_culled;
  [[maybe_unused]] uint32_t tl = t_lookup, tf = t_fallback;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    if constexpr (kDirect) {
      sd += __shfl_down(sd, off, 64);
      ss += __shfl_down(ss, off, 64);
      sv += __shfl_down(sv, off, 64);
    }
    if constexpr (kEnvLight) {
      ed += __shfl_down(ed, off, 64);
      es += __shfl_down(es, off, 64);
      ev += __shfl_down(ev, off, 64);
    }
    if constexpr (kMis) {
      me += __shfl_down(me, off, 64);
      mm += __shfl_down(mm, off, 64);
    }
    if constexpr (kSmooth) {
      qf += __shfl_down(qf, off, 64);
      qb += __shfl_down(qb, off, 64);
      qa += __shfl_down(qa, off, 64);
      qc += __shfl_down(qc, off, 64);
    }
    if constexpr (kTex) {
      tl += __shfl_down(tl, off, 64);
      tf += __shfl_down(tf, off, 64);
    }
  }
  if (threadIdx.x == 0u) {
    if (sum) atomicAdd(&counters->rays_total, (unsigned long long)sum);
    if constexpr (kDirect) {
      unsigned long long* line = stats + kLoopStatWords * (blockIdx.x % kLightStatLines);
      if (sd) atomicAdd(&line[0], (unsigned long long)sd);
      if (ss) atomicAdd(&line[1], (unsigned long long)ss);
      if (sv) atomicAdd(&line[2], (unsigned long long)sv);
      if constexpr (kEnvLight) {
        if (ed) atomicAdd(&line[3], (unsigned long long)ed);
        if (es) atomicAdd(&line[4], (unsigned long long)es);
        if (ev) atomicAdd(&line[5], (unsigned long long)ev);
      }
      if constexpr (kMis) {
        if (me) atomicAdd(&line[6], (unsigned long long)me);
        if (mm) atomicAdd(&line[7], (unsigned long long)mm);
      }
      if constexpr (kSmooth) {
        if (qf) atomicAdd(&line[8], (unsigned long long)qf);
        if (qb) atomicAdd(&line[9], (unsigned long long)qb);
        if (qa) atomicAdd(&line[10], (unsigned long long)qa);
        if (qc) atomicAdd(&line[11], (unsigned long long)qc);
      }
      if constexpr (kTex) {
        if (tl) atomicAdd(&line[12], (unsigned long long)tl);
        if (tf) atomicAdd(&line[13], (unsigned long long)tf);
      }
    }
  }
}

// the plain loop (instances: pt_kernels.hip; the ones that play roulette: pt_mega_direct.hip)
template <bool kEmit, bool kRoulette = false>
__global__ __launch_bounds__(kWave) void k_megakernel(DScene sc, DCamera cam, uint32_t iteration, DBand band,
                                                      uint32_t pix_count, int max_bounces, DFrame fb,
                                                      DeviceCounters* counters, int roulette)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kEmit, kRoulette, false>(sc, DLights{}, cam, iteration, band, pix_count, max_bounces, fb, counters, nullptr, roulette,
                                     s_stack + threadIdx.x);
}

// ... under a thin lens (DESIGN section 5i; instances: pt_mega_direct.hip)
template <bool kEmit, bool kRoulette>
__global__ __launch_bounds__(kWave) void k_megakernel_lens(DScene sc, DCamera cam, uint32_t iteration, DBand band,
                                                           uint32_t pix_count, int max_bounces, DFrame fb,
                                                           DeviceCounters* counters, int roulette, DLens lens)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kEmit, kRoulette, false, true>(sc, DLights{}, cam, iteration, band, pix_count, max_bounces, fb, counters, nullptr, roulette,
                                           s_stack + threadIdx.x, lens);
}
