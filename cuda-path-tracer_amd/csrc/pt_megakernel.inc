// pt_megakernel.inc -- the megakernel's loop, the whole path in one thread (path_tracing_mega_kernel, path_tracer.cu:227-269; one RNG
// stream per pixel: a different image from streaming mode at the same seed, a property of the reference): mega_path, the two plain
// kernels around it, and what every unit's launcher shares.  Included inside namespace pt, after pt_kernels_common.inc and with
// pt_light_sample.hpp and pt_env_light.hpp in front, by the six units that hold its 26 instances: pt_kernels.hip (the plain loop
// without roulette, beside the closest-hit kernels as ever), pt_mega_direct.hip, pt_mega_mis.hip, pt_mega_smooth.hip,
// pt_mega_tex.hip and pt_mega_nmap.hip -- a unit per feature, so that the code objects of the features before it stay the ones they
// were (DESIGN section 5h).  Which instance a frame launches: pt_mega_rules.hpp.
//
// The options of the loop, one bit of kF each: what the option adds; its DESIGN section, where the reasons are; the 64-bit words of a
// loop-counter line it adds to (`stats`: kLightStatLines lines of kLoopStatWords words, one add per wavefront); the kernels built with it.
//   kMegaEmit      a path ends at an emissive material and takes its colour, without a draw; off, the loop is the reference's.
//                  5d; -; k_megakernel<true, ..>, k_megakernel_lens<true, ..> and every kernel below (no emitter: the same bits)
//   kMegaRoulette  Russian roulette from bounce `roulette` on, the last bounce excepted: behind the emitter check, before
//                  evaluate_material, on the pixel's roulette stream.  A path it ends leaves colour 0, draws, samples and counts nothing.
//                  5h; -; k_megakernel<.., true>, k_megakernel_lens<.., true>, k_megakernel_direct<true>, k_megakernel_direct_lens<true>
//                  and every kernel from kMegaEnv on (`roulette` INT_MAX plays at no bounce: the same bits)
//   kMegaDirect    (with kMegaEmit) at every diffuse hit one light sample (5f, pt_light_sample.hpp; stream path_seed(pixel, iteration) ^
//                  kLightSeedXor, draws 3b .. 3b + 2 at bounce b) and one shadow ray (scene_occluded on the thread's own LDS stack, free
//                  while it runs), a per-path radiance sum, and the gate count_emission that keeps a lamp from counting twice.  Draws,
//                  closest hits, normal, depth and rays_total stay the plain loop's; tests/direct_loop_ref.py restates it in numpy.
//                  5g; words 0 .. 2 diffuse hits, shadow rays, unoccluded ones; k_megakernel_direct<..>, k_megakernel_direct_lens<..>,
//                  k_megakernel_env<true> and every kernel from kMegaEnvLight on
//   kMegaLens      the primary ray is the thin lens's, primary_ray<true> with `lens`; rng is left where the pinhole leaves it.
//                  5i; -; k_megakernel_lens<..>, k_megakernel_direct_lens<..>
//   kMegaEnv       a miss takes the environment, sky<true>(ray.d, env), at every bounce, as the gradient does: the environment is no
//                  lamp.  Pinhole or lens by lens.radius > 0 per launch; kMegaLens is not read.
//                  5j; -; k_megakernel_env<..> and every kernel below
//   kMegaEnvLight  (with kMegaEnv and kMegaDirect) the environment is a light too: behind the lamp's sample one environment sample
//                  (env_light::sample_point, pt_env_light.hpp; stream ^ kEnvLightSeedXor, draws 4b .. 4b + 3) with a shadow ray of its
//                  own, and 5g's gate in a flag of its own, count_env, for the miss behind it.  The lamps become a run-time choice:
//                  lt.records null (wave-uniform) draws no lamp sample and counts every emitter.
//                  5k; words 3 .. 5 hits that drew an environment sample, its shadow rays, unoccluded ones; k_megakernel_env_light and
//                  every kernel below
//   kMegaMis       (with kMegaEnvLight) the balance heuristic at diffuse vertices (pt_mis.hpp).  One more float of path state,
//                  bsdf_pdf, the lobe's density of the direction drawn, read only while a gate is closed.  A light sample is weighed
//                  against the lobe's density of its direction (not at the last bounce: no continuation ray); an emitter hit or a miss
//                  behind a diffuse vertex counts with the lobe's weight against the sampler's density there -- mis.inv_pdf_m[material],
//                  loaded beside the material, and env_light::density, loaded ahead of the sky's texels -- instead of 0.  The
//                  environment light (el.table) and the environment (env.texels) become run-time choices as well.  Draws, hits,
//                  shadow rays and words 0 .. 5 stay those of the loop without it.
//                  5l; words 6, 7 emitter hits, misses that were weighed; k_megakernel_mis, k_megakernel_smooth<true>, k_megakernel_tex<true, ..>
//   kMegaSmooth    (with kMegaEnvLight) at a triangle hit -- ray_scene<.., true> reports the winner -- the shading normal hn is
//                  smooth::shading_normal's (pt_smooth.hpp) and takes rec.n's place in the normal plane, evaluate_material, the light
//                  samples and bsdf_pdf; rec.n stays geometric (side, an emitter's cosine).  A light sample that points behind the
//                  geometry counts as not sampled; a diffuse or metal hit whose new direction does ends the path with colour 0 behind
//                  its light samples.  Every light is a run-time choice as under kMegaMis, with it or without.
//                  5n; words 8 .. 11 normals formed, fall-backs, absorbed continuations, culled light samples; k_megakernel_smooth<..>,
//                  k_megakernel_tex<.., true>
//   kMegaTex       (with kMegaEnvLight) at a triangle hit on a diffuse or metal material with a texture bound, immediately before
//                  evaluate_material, texmap::albedo's colour (pt_texture.hpp: the texel at the interpolated corner coordinates times
//                  p[0..2]) replaces p[0..2] in a copy of the material.  Every light is a run-time choice as under kMegaSmooth.
//                  5o; words 12, 13 lookups, fall-backs; k_megakernel_tex<..>, k_megakernel_nmap<..>
//   kMegaNmap      (with kMegaTex) at the same place and on the same hits, for a material with a normal map bound (nm.material_normal_map),
//                  nmap::shade's normal (pt_normal_map.hpp: the map's texel in the tangent frame of the corners' coordinates, about hn)
//                  replaces hn from there on -- evaluate_material, the light samples, bsdf_pdf; the normal plane has hn as it was.  Where
//                  it bent the normal, kMegaSmooth's culls and its absorption apply as at a triangle under kMegaSmooth.  The albedo fetch
//                  becomes a run-time choice, tx.material_texture.
//                  5q; words 14, 15 bent normals, fall-backs (a flat texel counts in neither); k_megakernel_nmap<..>
constexpr uint32_t kMegaEmit = 1u, kMegaRoulette = 2u, kMegaDirect = 4u, kMegaLens = 8u, kMegaEnv = 16u, kMegaEnvLight = 32u, kMegaMis = 64u,
                   kMegaSmooth = 128u, kMegaTex = 256u, kMegaNmap = 512u;
// what every instance with an environment is built with: emitters and roulette compiled in, pinhole or lens by lens.radius
constexpr uint32_t kMegaEnvBase = kMegaEmit | kMegaRoulette | kMegaEnv;
// ... and every instance that samples the environment: the lamps' samples by lt.records
constexpr uint32_t kMegaEnvLit = kMegaEnvBase | kMegaDirect | kMegaEnvLight;

// stack: the calling thread's column of the workgroup's LDS stack
template <uint32_t kF>
__device__ __forceinline__ void mega_path(const DScene& sc, const DLights& lt, const DCamera& cam, const uint32_t iteration, const DBand band,
                                          const uint32_t pix_count, const int max_bounces, const DFrame fb, DeviceCounters* counters,
                                          unsigned long long* stats, const int roulette, uint32_t* stack,
                                          const DLens lens = DLens{0.0f, 0.0f}, const DEnv env = DEnv{nullptr, 0u, 0u},
                                          const DEnvLight el = DEnvLight{nullptr}, const DMis mis = DMis{nullptr},
                                          const DSmooth sm = DSmooth{nullptr, nullptr},
                                          const DTex tx = DTex{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
                                          const DNmap nm = DNmap{nullptr, nullptr})
{
  constexpr bool kEmit = kF & kMegaEmit, kRoulette = kF & kMegaRoulette, kDirect = kF & kMegaDirect, kLens = kF & kMegaLens, kEnv = kF & kMegaEnv,
                 kEnvLight = kF & kMegaEnvLight, kMis = kF & kMegaMis, kSmooth = kF & kMegaSmooth, kTex = kF & kMegaTex, kNmap = kF & kMegaNmap;
  constexpr bool kDyn = kSmooth || kTex;  // every light and the environment are run-time choices
  static_assert(!kNmap || kTex, "the normal-mapped instances read the textured instances' pool and coordinates");
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
  [[maybe_unused]] uint32_t b_bent = 0u, b_kept = 0u;
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
      f3 hn = rec.n;  // the shading normal: the geometric one but at a triangle hit under kSmooth, and behind a bent hit under kNmap
      [[maybe_unused]] bool tri = false;
      [[maybe_unused]] bool bent = false;  // (kNmap) the normal map replaced hn at this hit
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
          int32_t ti;
          if constexpr (kNmap) {  // the map first: every load of the hit ahead of the first use, the flat test ahead of the tangents
            ti = tx.material_texture ? tx.material_texture[rec.mat] : -1;
            const int32_t ni = nm.material_normal_map[rec.mat];
            if (ni >= 0) {
              const uint32_t mesh = sc.object_mesh[at.object];
              const float* stp = tx.st + 2u * ((size_t)tx.mesh_first_index[mesh] + at.first);
              const uint32_t* idx = sc.mesh_views[mesh].indices + at.first;
              const float* pos = sc.mesh_views[mesh].positions;
              const texmap::Record nrec = tx.records[ni];
              const float stc[6] = {stp[0], stp[1], stp[2], stp[3], stp[4], stp[5]};
              const f3 p0 = ld3(pos + 3u * (size_t)idx[0]), p1 = ld3(pos + 3u * (size_t)idx[1]), p2 = ld3(pos + 3u * (size_t)idx[2]);
              f3 nn;
              const uint32_t how = nmap::shade(tx.texels, nrec, nm.table, p0, p1, p2, stc, stc + 2, stc + 4, at.u, at.v, sc.objects[at.object].m, hn,
                                               rec.n, ray.d, nn);
              if (how == nmap::kBent) {
                bent = true;
                hn = nn;
                ++b_bent;
              } else if (how == nmap::kKept) {
                ++b_kept;
              }
            }
          } else {
            ti = tx.material_texture[rec.mat];
          }
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
          if constexpr (kSmooth || kNmap) {
            if ((kSmooth ? tri : bent) && es.sampled && dot(es.w, rec.n) <= 0.0f) {  // behind the geometry: not sampled
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
            if constexpr (kSmooth || kNmap) {
              if ((kSmooth ? tri : bent) && ls.sampled && dot(ls.w, rec.n) <= 0.0f) {
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
      if constexpr (kSmooth || kNmap) {
        if ((kSmooth ? tri : bent) && mat.type != 2 && dot(ray.d, rec.n) <= 0.0f) {  // the new direction enters the geometry: absorbed
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
  [[maybe_unused]] uint32_t bb = b_bent, bk = b_kept;
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
    if constexpr (kSmooth || kNmap) {
      qf += __shfl_down(qf, off, 64);
      qb += __shfl_down(qb, off, 64);
      qa += __shfl_down(qa, off, 64);
      qc += __shfl_down(qc, off, 64);
    }
    if constexpr (kTex) {
      tl += __shfl_down(tl, off, 64);
      tf += __shfl_down(tf, off, 64);
    }
    if constexpr (kNmap) {
      bb += __shfl_down(bb, off, 64);
      bk += __shfl_down(bk, off, 64);
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
      if constexpr (kSmooth || kNmap) {
        if (qf) atomicAdd(&line[8], (unsigned long long)qf);
        if (qb) atomicAdd(&line[9], (unsigned long long)qb);
        if (qa) atomicAdd(&line[10], (unsigned long long)qa);
        if (qc) atomicAdd(&line[11], (unsigned long long)qc);
      }
      if constexpr (kTex) {
        if (tl) atomicAdd(&line[12], (unsigned long long)tl);
        if (tf) atomicAdd(&line[13], (unsigned long long)tf);
      }
      if constexpr (kNmap) {
        if (bb) atomicAdd(&line[14], (unsigned long long)bb);
        if (bk) atomicAdd(&line[15], (unsigned long long)bk);
      }
    }
  }
}

// the plain loop (instances: <.., false> pt_kernels.hip; the ones that play roulette: pt_mega_direct.hip)
template <bool kEmit, bool kRoulette = false>
__global__ __launch_bounds__(kWave) void k_megakernel(DScene sc, DCamera cam, uint32_t iteration, DBand band,
                                                      uint32_t pix_count, int max_bounces, DFrame fb,
                                                      DeviceCounters* counters, int roulette)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<(kEmit ? kMegaEmit : 0u) | (kRoulette ? kMegaRoulette : 0u)>(sc, DLights{}, cam, iteration, band, pix_count, max_bounces, fb, counters,
                                                                         nullptr, roulette, s_stack + threadIdx.x);
}

// ... under a thin lens (DESIGN section 5i; instances: pt_mega_direct.hip)
template <bool kEmit, bool kRoulette>
__global__ __launch_bounds__(kWave) void k_megakernel_lens(DScene sc, DCamera cam, uint32_t iteration, DBand band,
                                                           uint32_t pix_count, int max_bounces, DFrame fb,
                                                           DeviceCounters* counters, int roulette, DLens lens)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<(kEmit ? kMegaEmit : 0u) | (kRoulette ? kMegaRoulette : 0u) | kMegaLens>(sc, DLights{}, cam, iteration, band, pix_count, max_bounces, fb,
                                                                                     counters, nullptr, roulette, s_stack + threadIdx.x, lens);
}

// ---- the host's side: what the six units' launchers share.  A unit's launcher (launch_mega_*, below launch_megakernel in
// pt_kernels.hip) gets the frame and the instance the rule chose, picks that kernel among its own by the instance's template
// arguments and launches it through one of these: one thread per pixel of the band, a wavefront per workgroup.
void launch_mega_plain(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in);   // pt_kernels.hip
void launch_mega_direct(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in);  // pt_mega_direct.hip
void launch_mega_mis(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in);     // pt_mega_mis.hip
void launch_mega_smooth(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in);  // pt_mega_smooth.hip
void launch_mega_tex(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in);     // pt_mega_tex.hip
void launch_mega_nmap(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in);    // pt_mega_nmap.hip
template <typename K, typename... A>
void mega_go(K kernel, hipStream_t s, const MegaFrame& f, const A&... args)
{
  hipLaunchKernelGGL(kernel, dim3((f.pix_count + kWave - 1u) / kWave), dim3(kWave), 0, s, args...);
}
// the parameters of the two plain kernels (no lamp table, no loop counters), then `more`
template <typename K, typename... A>
void mega_go_plain(K kernel, hipStream_t s, const MegaFrame& f, const A&... more)
{
  mega_go(kernel, s, f, f.scene, f.cam, f.iteration, f.band, f.pix_count, f.max_bounces, f.fb, f.counters, f.roulette, more...);
}
// ... of every other kernel, then `more`
template <typename K, typename... A>
void mega_go_lit(K kernel, hipStream_t s, const MegaFrame& f, const A&... more)
{
  mega_go(kernel, s, f, f.scene, f.lights, f.cam, f.iteration, f.band, f.pix_count, f.max_bounces, f.fb, f.counters, f.stats, f.roulette, more...);
}
