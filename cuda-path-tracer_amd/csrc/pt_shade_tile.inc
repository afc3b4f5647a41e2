// pt_shade_tile.inc -- one TILE of the kernel that ends a bounce (k_shade_fused, pt_shade.hip): trailing sphere run +
// material + stable compaction + final gather for kFuseK x 64 x kGroupWaves consecutive slots of one frame.  Included (inside
// namespace pt, after pt_kernels_common.inc) by pt_shade.hip, whose kernel gives a 256-thread workgroup a tile, and by
// pt_persist.hip, whose persistent launch (k_persist, round 5) gives one to a single SERVICE wavefront.  In front of the tile: the
// end of a bounce for ONE path (goes_on, bounce_outcome, pack_survivor), which k_tail_count and k_shade (pt_shade.hip) share with it.
//   kGroupWaves  wavefronts of the group that owns the tile: 4 (blockDim 256) or 1 (blockDim 64)
//   kCoherent    the tile's inputs were written, and its outputs are read, by OTHER wavefronts of the SAME launch (k_persist):
//                every handed-over byte is then stored write-through (sc1) and loaded past the L1, the per-frame counters are updated by agent-scope atomics, and the caller drains its
//                stores (s_waitcnt vmcnt(0)) before it signs the tile off (MI355X_MICROARCH.md, inter-workgroup visibility)
// Slots per thread of a tile: 2 (round 4; 4 until then).  With four the kernel needs 128 registers and spills 18 of them at four
// wavefronts per SIMD; with two it needs 88, spills nothing and runs five (profiles/r04_config2_counters.txt).
#ifndef PT_SHADE_WAVES
#define PT_SHADE_WAVES 4
#endif
// (kFuseK, kFuseTile, kServiceTile: pt_kernels_common.inc -- the persistent launch's feed counts tiles too)
static_assert(kFuseTile <= 256u * kListPer, "k_raygen / k_spheres scan their work lists on k_shade_fused's tile descriptors");
// Hand-over loads and stores of a kCoherent tile.  Loads: non-temporal global loads (ldnt) -- they go past the L1, which is
// all a reader needs (tools/micro/coherence_probe.hip: a re-read line rewritten by another wavefront's sc1 stores comes back
// fresh through sc1, sc0 sc1 and nt loads alike, stale through plain ones; profiles/r05_coherence_probe.txt) and the
// compiler keeps track of them.  The first build used buffer loads with the sc1 bit (__builtin_amdgcn_raw_buffer_load_b128,
// aux 16): a service wavefront that had read a hit record's line in one bounce got the SAME bytes again in the next -- stale.
// Stores: write-through global stores (sc1), hand-issued; the caller's s_waitcnt vmcnt(0) before its sign-off drains them.
template <bool kCoherent>
__device__ __forceinline__ float4 ld_in(const float4* base, uint32_t index)
{
  return ldnt(&base[index]);
}
template <bool kCoherent>
__device__ __forceinline__ float2 ld_in(const float2* base, uint32_t index)
{
  return ldnt(&base[index]);
}
template <bool kCoherent>
__device__ __forceinline__ void st_out(float2* base, uint32_t index, const float2 v)
{
  if (kCoherent) {
    v2f w;
    w.x = v.x;
    w.y = v.y;
    asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(&base[index]), "v"(w) : "memory");
  } else {
    stnt(&base[index], v);
  }
}
template <bool kCoherent>
__device__ __forceinline__ void st_out(float4* base, uint32_t index, const float4 v)
{
  if (kCoherent) {
    v4f w;
    w.x = v.x;
    w.y = v.y;
    w.z = v.z;
    w.w = v.w;
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(&base[index]), "v"(w) : "memory");
  } else {
    stnt(&base[index], v);
  }
}

// ---- the end of a bounce for one path, stated once for the streaming forms (k_tail_count, k_shade, shade_tile) ----
// "This hit goes on": the path's closest hit is not an emitter (kEmit; mat_word: the hit record's material word, the side bit
// ignored), and roulette (kRoulette: a bounce that plays; index: the path's global slot) does not end it.  through(): the
// throughput that came into the bounce, asked for only when roulette plays (a caller that has to load it loads it then); c: that
// throughput, divided for a path that goes on (roulette_ends).  `ended`: roulette ended it; false with a false result: an emitter
// did.  What the compaction counts (k_tail_count) and what the material step does (k_shade, which hands both answers to
// bounce_outcome) must agree: both ask here, with or without roulette.  (shade_tile's phase 1 makes the same two checks in
// place, as it did: asked here, every form tried gave its roulette instances of k_shade_fused other instructions --
// profiles/loops_refactor.txt, A.)
template <bool kEmit, bool kRoulette, class Through>
__device__ __forceinline__ bool goes_on(const DScene& sc, const uint32_t mat_word, Through&& through, f3& c, const uint32_t index,
                                        const uint32_t iteration, const uint32_t bounce, bool& ended)
{
  ended = false;
  if (kEmit && is_emitter(sc.materials[mat_word & 0x7fffffffu])) return false;
  if (kRoulette) {
    c = through();
    ended = roulette_ends(c, index, iteration, bounce);
  }
  return !ended;
}

// material_kernel (path_tracer.cu:292-315) and the final gather of a path that ends here, for one slot, in the plain form (one
// `if` per outcome; shade_tile's default is shade_kinds, the same operations for a wavefront of mixed outcomes).  hit, tp, nm: the
// closest hit; emits: it is an emitter; ended: roulette has ended the path (both: goes_on's answers); color: the throughput,
// already divided for a roulette survivor.
// True: the path survives with its new ray in ro, rd, tmin_flag and its throughput in color.  False: it ended and its sample is
// in `fb` (staged: acc_iteration 0) -- miss: throughput * sky; emitter: throughput * emission, no draw; roulette: 0, no draw;
// the last bounce: the raw throughput.  env (DESIGN section 5j): null, or the environment that is the sky of a miss, sky<true> -- the
// caller's constant, decided where this is inlined.  (Not a template parameter: as a template this function gave k_shade's four
// instances other instructions.)
__device__ __forceinline__ bool bounce_outcome(const DScene& sc, const DFrame& fb, const uint32_t local_pixel, const uint32_t acc_iteration,
                                               const int bounce, const int last_bounce, const uint32_t slot, const uint32_t iteration,
                                               const bool hit, const float4 tp, const float4 nm, const bool emits, const bool ended,
                                               f3& ro, f3& rd, bool& tmin_flag, f3& color, const DEnv* env = nullptr)
{
  if (!hit) {
    // miss: throughput *= sky; the path ends (path_tracer.cu:304-307, 283-289)
    color = color * (env ? sky<true>(rd, *env) : background(rd));
    if (bounce == 0) accumulate_nd(fb.nd4, local_pixel, acc_iteration, -rd, 1e6f);  // raygen defaults, ray_gen.cu:26-28
    accumulate_color(fb.color4, local_pixel, acc_iteration, color);
    return false;
  }
  const f3 hn = xyz(nm);
  if (bounce == 0) accumulate_nd(fb.nd4, local_pixel, acc_iteration, hn, tp.x);  // path_tracer.cu:308-311
  const uint32_t ms = __float_as_uint(nm.w);
  const DMaterial m = sc.materials[ms & 0x7fffffffu];
  if (emits) {
    color = emit_color(color, m);  // the path ends at the emitter: no draw
  } else if (ended) {
    color = mk3(0.0f, 0.0f, 0.0f);
  } else {
    // RNG re-seeded from the global slot index, then discard(bounce) (path_tracer.cu:300-301)
    Minstd rng;
    rng.seed(path_seed(slot, iteration));
    rng.discard((uint32_t)bounce);
    evaluate_material(ro, rd, tmin_flag, mk3(tp.y, tp.z, tp.w), hn, ms >> 31, m, rng, color);
  }
  if (last_bounce || emits || ended) {
    accumulate_color(fb.color4, local_pixel, acc_iteration, color);  // capped paths deposit raw throughput
    return false;
  }
  return true;
}

// a survivor as the path arrays hold it (DPaths): o4 = origin, pixel | tmin_flag << 31; d4 = direction, throughput.x; t2 = throughput.yz
__device__ __forceinline__ void pack_survivor(const f3 ro, const f3 rd, const f3 color, const uint32_t pixel, const bool tmin_flag, float4& o4,
                                              float4& d4, float2& t2)
{
  o4 = make_float4(ro.x, ro.y, ro.z, __uint_as_float(pixel | (tmin_flag ? 0x80000000u : 0u)));
  d4 = make_float4(rd.x, rd.y, rd.z, color.x);
  t2 = make_float2(color.y, color.z);
}

// Every pointer is the frame's own (frame offset applied by the caller); `fo` is that offset in slots (work-list entries are
// batch-global); n_all = live[bounce] of the frame, n = what is walked (the list's length at bounce 0 of a finishing raygen,
// else n_all), tiles = tiles of n; s_cnt: kFuseK * kGroupWaves words and s_excl: one word of the group's LDS.
// kEmit: the scene has an emissive material (ptc_material type 3; the host picks the instance).  A path whose closest hit is
// an emitter ends at this bounce, so the survivor ballot of phase 1 needs the hit's material: the hit record's nm is then
// loaded in phase 1 (phase 2 finds it in registers) and the material's type read from the table.  Without emitters nm
// waits for phase 2 as before, and the instance is the one that ran before emitters existed.
// kRoulette: the bounce plays Russian roulette ("roulette", DESIGN section 5h; the host picks the instance for the bounces that
// play, never the last one).  A path that would go on may end by chance, so the survivor ballot of phase 1 needs the decision:
// the throughput that came into the bounce (d4.w, t2) is loaded with the ray, the roulette stream's draw is made in phase 1 and
// a survivor's division is applied to the registers phase 2 reads its throughput from; a path that ends is remembered for phase
// 2, which gives it no material draw and the sample (0, 0, 0).  The count still goes out after one round trip.
// kEnv: the frame has an environment (ptc_set_environment, DESIGN section 5j; the host picks the instance): a miss multiplies the
// throughput by the map's value in the ray's direction (`env`) where the gradient stands otherwise.  Only colour differs.
template <bool kSpheres, bool kFirst, int kGroupWaves, bool kCoherent, bool kNext = false, bool kEmit = false, bool kRoulette = false, bool kEnv = false>
__device__ __forceinline__ void shade_tile(const DScene& sc, const uint32_t obj_begin, const uint32_t obj_end, const DPaths in, const DPaths out,
                                           const DHits hits, const int staged, const int bounce, const int last_bounce, const uint32_t* slot_base,
                                           unsigned long long* tile_desc, const uint32_t epoch, const DFrame fb, const DBand band,
                                           DeviceCounters* counters, uint8_t* octs, const uint32_t iteration, const uint32_t* list, const size_t fo,
                                           const uint32_t tile, const uint32_t tiles, const uint32_t n, const uint32_t n_all, uint32_t* s_cnt,
                                           uint32_t* s_excl, const DNextRun* next = nullptr, const DEnv env = DEnv{nullptr, 0u, 0u})
{
  static_assert(!kEnv || !kCoherent, "environment: the per-bounce launches (k_persist is not taught it)");
  static_assert(!kNext || (!kCoherent && !kFirst), "prefold: the per-bounce launches, behind a bounce that had a closest-hit launch");
  static_assert(!kRoulette || !kCoherent, "roulette: the per-bounce launches (k_persist is not taught it)");
  constexpr uint32_t kThreads = 64u * (uint32_t)kGroupWaves, kTile = kThreads * (uint32_t)kFuseK;
  const uint32_t acc_iteration = staged ? 0u : iteration;
  const uint32_t wave = threadIdx.x >> 6;
  // ---- phase 1: rays and hits of the tile; the closest hit is final after the trailing sphere run ----
  float4 o4[kFuseK], d4[kFuseK], tp[kFuseK], nm[kFuseK];
  float2 t2[kFuseK];  // (throughput: d4.w, t2.x, t2.y -- DPaths)
  uint32_t have_nm = 0u, hit_mask = 0u, ended_mask = 0u;
  uint32_t slot_of[kFuseK];  // position tile * kFuseTile + j * 256 + thread of the walk -> slot (the same unless `list`)
#pragma unroll
  for (int j = 0; j < kFuseK; ++j) {
    const uint32_t at = tile * kTile + (uint32_t)j * kThreads + threadIdx.x;
    slot_of[j] = at < n ? (list ? list[at] - (uint32_t)fo : at) : n_all;
  }
#pragma unroll
  for (int j = 0; j < kFuseK; ++j) {
    const uint32_t s = slot_of[j];
    tp[j] = make_float4(-1.0f, 0.f, 0.f, 0.f);
    nm[j] = o4[j] = d4[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kRoulette) t2[j] = make_float2(0.f, 0.f);
    if (s < n_all) {
      o4[j] = ld_in<kCoherent>(in.o4, s);
      d4[j] = ld_in<kCoherent>(in.d4, s);
      if (!kFirst) tp[j] = ld_in<kCoherent>(hits.tp, s);
      if (kRoulette) t2[j] = bounce != 0 ? ld_in<kCoherent>(in.t2, s) : make_float2(1.0f, 1.0f);
    }
  }
  // the sphere run that ends the object list: every lane with its own candidates, all its slots at once, when the run
  // allows it (sphere_run_lanes); object by object otherwise
  const bool lanes_run = kSpheres && PT_SPHERE_LANES && sc.lanes_run != 0u;
  if (kSpheres && lanes_run) {
    static_assert(kFuseK <= 4, "sphere_run_lanes: at most four slots");
    uint32_t valid = 0u;
#pragma unroll
    for (int j = 0; j < kFuseK; ++j) valid |= slot_of[j] < n_all ? 1u << j : 0u;
    have_nm |= sphere_run_lanes<kFuseK>(sc, obj_begin, obj_end, o4, d4, tp, nm, valid);
  }
#pragma unroll
  for (int j = 0; j < kFuseK; ++j) {
    const uint32_t s = slot_of[j];
    if (kSpheres && !lanes_run && s < n_all) {
      Ray ray;
      ray.o = xyz(o4[j]);
      ray.d = xyz(d4[j]);
      ray.tmin = (__float_as_uint(o4[j].w) >> 31) ? 1e-5f : 1e-4f;
      ray.tmax = tp[j].x >= 0.0f ? tp[j].x : FLT_MAX;
      Hit rec;
      bool changed = false;
      if (PT_FOLD_TAIL && sc.fold_run != 0u) sphere_fold(sc, obj_begin, obj_end, ray, rec, changed);
      else sphere_segment(sc, obj_begin, obj_end, ray, rec, changed);
      if (changed) {  // the record stays in registers: its only reader is this thread, a few lines down
        tp[j] = make_float4(rec.t, rec.p.x, rec.p.y, rec.p.z);
        nm[j] = make_float4(rec.n.x, rec.n.y, rec.n.z, __uint_as_float(rec.mat | (rec.side << 31)));
        have_nm |= 1u << j;
      }
    }
    const bool hit = s < n_all && tp[j].x >= 0.0f;
    hit_mask |= hit ? 1u << j : 0u;
    bool goes_on = hit;  // (goes_on()'s two checks, in place: see there)
    if (kEmit && hit) {  // (kFirst: a hit is the sphere run's, its record is in registers)
      if (!kFirst && !(have_nm >> j & 1u)) {
        nm[j] = ld_in<kCoherent>(hits.nm, s);
        have_nm |= 1u << j;
      }
      goes_on = !is_emitter(sc.materials[__float_as_uint(nm[j].w) & 0x7fffffffu]);
    }
    if (kRoulette && goes_on) {  // (exactly the paths the ballot below counts: the host picks a kRoulette instance for no last bounce)
      f3 c = mk3(bounce == 0 ? 1.0f : d4[j].w, t2[j].x, t2[j].y);
      if (roulette_ends(c, (slot_base ? *slot_base : 0u) + s, iteration, (uint32_t)bounce)) {
        goes_on = false;
        ended_mask |= 1u << j;
      } else {  // (q >= 1: the same bits)
        d4[j].w = c.x;
        t2[j] = make_float2(c.y, c.z);
      }
    }
    const uint64_t live = __ballot(goes_on && !last_bounce);
    if ((threadIdx.x & 63u) == 0u) s_cnt[j * kGroupWaves + (int)wave] = (uint32_t)__popcll(live);
  }
  // what phase 2 still needs from memory, requested before anybody waits for anything
#pragma unroll
  for (int j = 0; j < kFuseK; ++j) {
    const uint32_t s = slot_of[j];
    if (!kRoulette) {  // (a roulette instance has it already)
      t2[j] = make_float2(0.f, 0.f);
      if (s < n_all && bounce != 0) t2[j] = ld_in<kCoherent>(in.t2, s);  // (bounce 0: throughput 1, k_raygen does not write it)
    }
    if (!kFirst && (hit_mask >> j & 1u) && !(have_nm >> j & 1u)) nm[j] = ld_in<kCoherent>(hits.nm, s);
  }
  if (kGroupWaves > 1) __syncthreads();
  // ---- the tile's survivor count goes out (one round trip after the workgroup started) ----
  uint32_t agg = 0u;
#pragma unroll
  for (int k = 0; k < kFuseK * kGroupWaves; ++k) agg += s_cnt[k];
  const unsigned long long tag = (unsigned long long)epoch << 34;
  if (threadIdx.x == 0u)
    __hip_atomic_store(&tile_desc[tile], tag | (tile == 0u ? kDescPrefix : kDescAggregate) | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  // ---- phase 2: material_kernel per slot, in place: the new ray and throughput of a survivor take the registers of the
  // old ones (nothing is written yet: where to is known only after the look-back, which by then has had the whole of
  // this phase to resolve); paths that end go into the framebuffer ----
  uint32_t surv_mask = 0u;
#pragma unroll
  for (int j = 0; j < kFuseK; ++j) {
    const uint32_t s = slot_of[j];
    f3 ro = xyz(o4[j]), rd = xyz(d4[j]), color = bounce == 0 ? mk3(1.0f, 1.0f, 1.0f) : mk3(d4[j].w, t2[j].x, t2[j].y);
    uint32_t pixbits = __float_as_uint(o4[j].w);
    if (s < n_all) {
      const uint32_t pixel = pixbits & 0x7fffffffu;
      const uint32_t local_pixel = band_local(band, pixel);
      bool tmin_flag = (pixbits >> 31) != 0u;
#if PT_SHADE_KINDS
      const bool is_hit = (hit_mask >> j & 1u) != 0u;
      const f3 hn = xyz(nm[j]);
      const uint32_t ms = __float_as_uint(nm[j].w);
      DMaterial m{(int32_t)kKindMiss, {0.f, 0.f, 0.f, 0.f}};  // (a hit's type is 0..2, or 3 in a kEmit instance: validate_scene)
      if (is_hit) m = sc.materials[ms & 0x7fffffffu];
      const bool emits = kEmit && is_hit && is_emitter(m);  // (phase 1 counted it out)
      const bool ended = kRoulette && (ended_mask >> j & 1u) != 0u;  // (roulette, phase 1: no draw, the sample is 0)
      if (bounce == 0) {
        if (is_hit) accumulate_nd(fb.nd4, local_pixel, acc_iteration, hn, tp[j].x);  // path_tracer.cu:308-311
        else accumulate_nd(fb.nd4, local_pixel, acc_iteration, -rd, 1e6f);           // raygen defaults, ray_gen.cu:26-28
      }
      const uint32_t slot = (slot_base ? *slot_base : 0u) + s;
      shade_kinds<kEmit, kEnv>(ended ? kKindNone : emits ? kKindEmit : (uint32_t)m.type, ro, rd, tmin_flag, mk3(tp[j].y, tp[j].z, tp[j].w), hn, ms >> 31, m,
                               slot, iteration, (uint32_t)bounce, color, env);
      if (ended) color = mk3(0.0f, 0.0f, 0.0f);
      if (!is_hit || last_bounce || emits || ended) {
        // a miss ends the path with throughput * sky (path_tracer.cu:304-307, 283-289), an emitter with throughput * emission;
        // capped paths deposit raw throughput
        accumulate_color(fb.color4, local_pixel, acc_iteration, color);
      } else {
        surv_mask |= 1u << j;  // (pack_survivor, in place: called here it costs every instance 18 instructions and more)
        o4[j] = make_float4(ro.x, ro.y, ro.z, __uint_as_float(pixel | (tmin_flag ? 0x80000000u : 0u)));
        d4[j] = make_float4(rd.x, rd.y, rd.z, color.x);
        t2[j] = make_float2(color.y, color.z);
      }
#else
      const bool is_hit = (hit_mask >> j & 1u) != 0u;  // (emits, ended: what phase 1 counted by)
      const bool emits = kEmit && is_hit && is_emitter(sc.materials[__float_as_uint(nm[j].w) & 0x7fffffffu]);
      if (bounce_outcome(sc, fb, local_pixel, acc_iteration, bounce, last_bounce, (slot_base ? *slot_base : 0u) + s, iteration, is_hit, tp[j], nm[j],
                         emits, kRoulette && (ended_mask >> j & 1u) != 0u, ro, rd, tmin_flag, color, kEnv ? &env : nullptr)) {
        surv_mask |= 1u << j;
        pack_survivor(ro, rd, color, pixel, tmin_flag, o4[j], d4[j], t2[j]);
      }
#endif
    }
  }

  // ---- the tile's offset comes in ----
  if (wave == 0u) {
    uint32_t excl = 0u;
    if (tile != 0u) {
      excl = tile_lookback(tile_desc, tile, epoch, &counters->flags);
      if (threadIdx.x == 0u)
        __hip_atomic_store(&tile_desc[tile], tag | kDescPrefix | (excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0u) {
      *s_excl = excl;
      if (tile + 1u == tiles) {  // the last tile knows the frame's total (k_scan's epilogue)
        if (kCoherent) {  // (other wavefronts of this launch, on other XCDs, read and update these words)
          __hip_atomic_store(&counters->live[bounce + 1], last_bounce ? 0u : excl + agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          atomicAdd(&counters->rays_total, (unsigned long long)n_all);
          atomicAdd(&counters->paths[bounce], (unsigned long long)n_all);
        } else {
          counters->live[bounce + 1] = last_bounce ? 0u : excl + agg;
          counters->rays_total += n_all;
          counters->paths[bounce] += n_all;
        }
      }
    }
  }
  if (kGroupWaves > 1) __syncthreads();

  // ---- survivors to their stable place: tile offset + sub-blocks before + wavefronts before + lanes before ----
  uint32_t base = *s_excl;
#pragma unroll
  for (int j = 0; j < kFuseK; ++j) {
    uint32_t before = 0u, in_sub = 0u;
#pragma unroll
    for (int w = 0; w < kGroupWaves; ++w) {
      const uint32_t c = s_cnt[j * kGroupWaves + w];
      before += (uint32_t)w < wave ? c : 0u;
      in_sub += c;
    }
    const bool survives = (surv_mask >> j & 1u) != 0u;
    const uint64_t live = __ballot(survives);
    if (survives) {
      const uint32_t dst = base + before + rank_below(live);
      st_out<kCoherent>(out.o4, dst, o4[j]);
      st_out<kCoherent>(out.d4, dst, d4[j]);
      st_out<kCoherent>(out.t2, dst, t2[j]);
      if (octs) octs[dst] = (uint8_t)((d4[j].x < 0.0f ? 1u : 0u) | (d4[j].y < 0.0f ? 2u : 0u) | (d4[j].z < 0.0f ? 4u : 0u));
      if (kNext) {
        // "prefold": k_spheres<first, filter> of the NEXT bounce for this survivor, whose ray is at hand (pt_shade.hip: same
        // calls on the same operands -- load_ray's view of the ray just stored, sphere_fold or sphere_segment<true>, the miss
        // record a first launch writes, may_hit_boxes with the range the run has left)
        Ray ray;
        ray.o = xyz(o4[j]);
        ray.d = xyz(d4[j]);
        ray.tmin = (__float_as_uint(o4[j].w) >> 31) ? 1e-5f : 1e-4f;
        ray.tmax = FLT_MAX;
        Hit rec;
        bool changed = false;
        if (next->fold_run != 0u) sphere_fold(sc, next->begin, next->end, ray, rec, changed);
        else sphere_segment<true>(sc, next->begin, next->end, ray, rec, changed);
        if (changed) store_hit(next->hits, dst, rec);
        else stnt(&next->hits.tp[dst], make_float4(-1.0f, 0.f, 0.f, 0.f));
        next->flags[dst] = may_hit_boxes(sc.objects, next->filt_begin, next->filt_end, ray.o, ray.d, ray.tmax) ? (uint8_t)1 : (uint8_t)0;
      }
    }
    base += in_sub;
  }
}
