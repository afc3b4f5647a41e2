// pt_shade_end.inc -- the kernels that end a bounce of the streaming loop: k_shade<kEmit, kRoulette> (the three-kernel form's last) and
// k_shade_fused<kSpheres, kFirst, kNext, kEmit, kRoulette> (the default).  Included (inside namespace pt, after pt_kernels_common.inc
// and pt_shade_tile.inc) by pt_shade.hip with PT_SHADE_ENV 0, which defines them under those names as ever, and by pt_env.hip with
// PT_SHADE_ENV 1: the environment's instances (ptc_set_environment, DESIGN section 5j) k_shade_env and k_shade_fused_env, which take a
// trailing DEnv and hand it to bounce_outcome / shade_tile<.., kEnv = true>; everything else is the same text.  (An include and
// not a device function both kernels call, as pt_raygen.inc: the instances without an environment are to stay the ones they were.)
#if PT_SHADE_ENV
#define PT_SHADE_NAME(name) name##_env
#define PT_SHADE_ENV_PARAM , DEnv env
#define PT_SHADE_ENV_ARG , env
#define PT_SHADE_ENV_PTR , &env
#else
#define PT_SHADE_NAME(name) name
#define PT_SHADE_ENV_PARAM
#define PT_SHADE_ENV_ARG
#define PT_SHADE_ENV_PTR
#endif

// material_kernel (path_tracer.cu:292-315) + the stable compaction scatter + the final gather of
// every path that ends at this bounce.
// staged: `fb` is the slot's staging buffer (one sample per frame of the batch, plain stores); k_accumulate then
// folds the staged samples into the real framebuffer in iteration order.  Otherwise the running mean goes
// straight into `fb`.  kEmit, kRoulette: as k_tail_count's (the chunk offsets count the paths that go on).
template <bool kEmit = false, bool kRoulette = false>
__global__ __launch_bounds__(256) void PT_SHADE_NAME(k_shade)(DScene sc, DPaths in, DPaths out, DHits hits, int staged, int bounce,
                                               int last_bounce, const uint32_t* slot_base, const uint32_t* chunk_offsets,
                                               DFrame fb, DBand band, DeviceCounters* counters, uint8_t* octs, DBatchInfo bi PT_SHADE_ENV_PARAM)
{
  const uint32_t frame = blockIdx.y;  // see DBatchInfo
  const uint32_t iteration = bi.iteration[frame];
  const uint32_t acc_iteration = staged ? 0u : iteration;
  if (octs) octs += (size_t)frame * bi.stride;
  offset_frame(in, (size_t)frame * bi.stride);
  offset_frame(out, (size_t)frame * bi.stride);
  offset_frame(hits, (size_t)frame * bi.stride);
  chunk_offsets += (size_t)frame * bi.chunk_stride;
  if (staged) offset_frame(fb, (size_t)frame * bi.stride);
  counters += frame;
  const uint32_t n = counters->live[bounce];
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (blockIdx.x * 256u >= n) return;
  const bool active = s < n;
  bool survives = false;
  f3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 0), color = mk3(0, 0, 0);
  uint32_t pixel = 0u;
  bool tmin_flag = false;
  if (active) {
    const float4 o4 = ldnt(&in.o4[s]);
    const float4 d4 = ldnt(&in.d4[s]);
    const float2 t2 = bounce == 0 ? make_float2(1.0f, 1.0f) : ldnt(&in.t2[s]);  // (throughput: d4.w, t2 -- DPaths; k_raygen writes neither)
    const float4 tp = ldnt(&hits.tp[s]);
    ro = xyz(o4);
    rd = xyz(d4);
    color = mk3(bounce == 0 ? 1.0f : d4.w, t2.x, t2.y);
    pixel = __float_as_uint(o4.w) & 0x7fffffffu;
    tmin_flag = (__float_as_uint(o4.w) >> 31) != 0u;
    const uint32_t slot = (slot_base ? *slot_base : 0u) + s;
    const bool hit = !(tp.x < 0.0f);
    float4 nm = make_float4(0.f, 0.f, 0.f, 0.f);
    bool emits = false, ended = false;
    if (hit) {
      nm = ldnt(&hits.nm[s]);
      // the decision k_tail_count has counted by: an emitter ends the path; roulette ends it with the sample (0, 0, 0) and no draw,
      // or lets it go on with its throughput divided (section 5h; the host picks a kRoulette instance for no last bounce)
      const bool on = goes_on<kEmit, kRoulette>(sc, __float_as_uint(nm.w), [&] { return color; }, color, slot, iteration, (uint32_t)bounce, ended);
      emits = !on && !ended;
    }
    survives = bounce_outcome(sc, fb, band_local(band, pixel), acc_iteration, bounce, last_bounce, slot, iteration, hit, tp, nm, emits, ended,
                              ro, rd, tmin_flag, color PT_SHADE_ENV_PTR);
  }
  const uint64_t live = __ballot(survives);
  if (survives) {
    const uint32_t dst = chunk_offsets[s / kChunk] + rank_below(live);
    float4 o4, d4;
    float2 t2;
    pack_survivor(ro, rd, color, pixel, tmin_flag, o4, d4, t2);
    stnt(&out.o4[dst], o4);
    stnt(&out.d4[dst], d4);
    stnt(&out.t2[dst], t2);
    // direction octant of the new ray, for the coherence sort of the next bounce (k_sort_octant)
    if (octs) octs[dst] = (uint8_t)((rd.x < 0.0f ? 1u : 0u) | (rd.y < 0.0f ? 2u : 0u) | (rd.z < 0.0f ? 4u : 0u));
  }
}

// ------------------------------------------------------------------------------------------------
// the end of a bounce in ONE pass: trailing sphere run + material + stable compaction + final gather
// ------------------------------------------------------------------------------------------------
// k_tail_count -> k_scan -> k_shade read every ray and hit record twice and put a one-workgroup scan between two
// full-width launches.  This kernel does the three jobs in one pass over the slots (path_tracer.cu:292-315 material_kernel,
// :454-457 stable_partition, :317-330 final gather; :78-100 for the sphere run that ends the object list):
//   * a workgroup owns a TILE of 256 x kFuseK consecutive slots (every thread kFuseK of them, 256 apart: coalesced),
//     loads ray + hit, finishes the closest hit (the trailing spheres), and knows from "is there a hit" alone which of
//     its paths survive -- so the tile's survivor count is published after ONE round trip to memory;
//   * the stable offset of the tile = survivors of all tiles before it, found by decoupled look-back over the tile
//     descriptors (aggregate / inclusive prefix, Merrill & Garland): a wavefront reads up to 64 predecessors at once;
//   * tiles are taken in TICKET order (one agent-scope atomic per workgroup on the frame's counter line; blocks are
//     numbered frame-fastest, so neighbouring workgroups of a batch take their tickets on different lines), not in
//     blockIdx order: whoever waits for a tile's descriptor waits for a workgroup that is RUNNING (it has its ticket),
//     whatever else holds the chip's wavefront slots.  Block order is 1-3 % faster (the ticket's round trip sits in
//     front of a workgroup's first load) and is NOT safe: with several streams' kernels on the chip, workgroups of
//     one kernel fill an XCD spinning for a predecessor that waits for a slot on an XCD filled by another kernel's
//     spinners -- seen once in 67 GPU tests x several runs (ten one-frame launches on ten streams), caught by the
//     bounded wait below.  The wait stays bounded all the same: a workgroup that has waited about a second sets
//     kFlagDispatchOrder and ptc_get_stats reports an error instead of an image;
//   * descriptors carry the launch's epoch, so nothing has to be cleared between launches.
// Same arithmetic and same slot order as the three kernels it replaces: images are bit-identical (tests).
// Slots per thread: 2 (round 4; 4 until then).  With four the kernel needs 128 registers and spills 18 of them at four
// wavefronts per SIMD; with two it needs 88, spills nothing and runs five: config 2 +2.2 %, config 3 +0.6 ... 1.2 %;
// one slot (eight wavefronts): -4 ... -6 % (profiles/r04_config2_counters.txt).  Six wavefronts (80 registers) spill 53.
template <bool kSpheres, bool kFirst, bool kNext = false, bool kEmit = false, bool kRoulette = false>
// (occupancy bounds re-measured on the final build: at least 5 or 6 wavefronts per SIMD forces spills, -8 % / -13 % end
// to end; 1 to 3 compile to the same 124 registers)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PT_SHADE_WAVES, 8))) void PT_SHADE_NAME(k_shade_fused)(DScene sc, uint32_t obj_begin, uint32_t obj_end, DPaths in, DPaths out, DHits hits,
                                                     int staged, int bounce, int last_bounce, const uint32_t* slot_base,
                                                     unsigned long long* tile_desc, uint32_t tile_stride, uint32_t epoch, DFrame fb,
                                                     DBand band, DeviceCounters* counters, uint8_t* octs, DBatchInfo bi, const uint32_t* list,
                                                     DNextRun next PT_SHADE_ENV_PARAM)
{
  __shared__ uint32_t s_excl, s_tile;
  __shared__ uint32_t s_cnt[kFuseK * 4];
  const uint32_t frame = blockIdx.x % bi.count;  // frame-fastest: neighbouring blocks take their tickets on different lines
  const uint32_t iteration = bi.iteration[frame];
  const size_t fo = (size_t)frame * bi.stride;
  if (octs) octs += fo;
  in.o4 += fo;  // (written out, not offset_frame: with it the kFirst instances order two scalar adds differently)
  in.d4 += fo;
  in.t2 += fo;
  out.o4 += fo;
  out.d4 += fo;
  out.t2 += fo;
  hits.tp += fo;
  hits.nm += fo;
  tile_desc += (size_t)frame * tile_stride;
  if (staged) {
    fb.color4 += fo;
    fb.nd4 += fo;
  }
  counters += frame;
  // list ("filter_rays", bounce 0 of a scene whose whole object list is the bounce's one listed traversal launch): the
  // rays that are not on the launch's work list have been finished by k_raygen, which knew that they hit nothing; this
  // kernel then walks the list (slot order: the survivors land where they would have) instead of all slots
  const uint32_t n_all = counters->live[bounce];
  const uint32_t n = list ? counters->list_count : n_all;
  if (list) list += fo;
  const uint32_t tiles = (n + kFuseTile - 1u) / kFuseTile;
  // The grid is sized for a frame of all-live slots; the workgroups the frame has no tile for leave without a ticket:
  // exactly `tiles` tickets are taken per frame.  (Dispatching the empty workgroups costs little: a launch sized by the
  // last batch's live counts, whose workgroups came back for more tiles when there were too few, was slower -- the
  // loop cost 24 spilled registers -- profiles/r03_shade_breakdown.txt.)
  if (blockIdx.x / bi.count >= tiles) {
    if (tiles == 0u && blockIdx.x / bi.count == 0u && threadIdx.x == 0u) {  // nothing alive: nothing follows
      counters->live[bounce + 1] = 0u;
      counters->rays_total += n_all;  // (not zero when k_raygen has finished every ray of the frame, see `list`)
      counters->paths[bounce] += n_all;
    }
    return;
  }
  if (threadIdx.x == 0u) {
    const uint32_t t = __hip_atomic_fetch_add(&counters->shade_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every tile of the frame is taken once the last ticket is out: the next launch starts from zero
    if (t + 1u == tiles) __hip_atomic_store(&counters->shade_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_tile = t;
  }
  __syncthreads();
  const uint32_t tile = s_tile;

  // (the tile itself: pt_shade_tile.inc, shared with the persistent launch's service wavefronts)
  if (kNext) {  // (the next bounce's records and bytes of this frame)
    offset_frame(next.hits, fo);
    next.flags += fo;
  }
  shade_tile<kSpheres, kFirst, 4, false, kNext, kEmit, kRoulette, PT_SHADE_ENV != 0>(sc, obj_begin, obj_end, in, out, hits, staged, bounce, last_bounce, slot_base, tile_desc, epoch, fb, band,
                                                counters, octs, iteration, list, fo, tile, tiles, n, n_all, s_cnt, &s_excl, &next PT_SHADE_ENV_ARG);
}

#undef PT_SHADE_NAME
#undef PT_SHADE_ENV_PARAM
#undef PT_SHADE_ENV_ARG
#undef PT_SHADE_ENV_PTR
