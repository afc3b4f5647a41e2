// pt_shade.hip -- ray generation and the end of a bounce (see pt_kernels.hip for the map of the path): k_raygen, k_spheres,
// k_tail_count / k_scan / k_shade (the three-kernel form), k_shade_fused (default), k_sort_octant, k_accumulate.

#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
static_assert(pt::beam_rules::kLeaf == pt::kLeafBit, "pt_beam_rules.hpp restates the leaf bit of the four-wide node (pt_device.hpp)");
static_assert((uint32_t)pt::beam_rules::kEntries == pt::kBeamEntries, "pt_beam_rules.hpp restates the entries per tile (pt_device.hpp)");
static_assert(pt::feed_rules::kBatch == (uint32_t)pt::kWave, "a feed batch is one wavefront's worth of rays");
#include <float.h>
#include "pt_launch_flags.hpp"

namespace pt {

#include "pt_kernels_common.inc"
#include "pt_shade_tile.inc"  // the end of a bounce per path (goes_on, bounce_outcome, pack_survivor) and per tile (shade_tile)

// k_raygen<kFilter, kFinish>, k_raygen_next and their thin-lens forms k_raygen_lens<kFilter, kFinish>, k_raygen_next_lens:
// pt_raygen.inc, one text for both
#define PT_RAYGEN_LENS 0
#include "pt_raygen.inc"
#undef PT_RAYGEN_LENS
#define PT_RAYGEN_LENS 1
#include "pt_raygen.inc"
#undef PT_RAYGEN_LENS

// ptc_generate_rays: the primary ray of every slot of the band at one iteration, as the frame's ray generation builds it (primary_ray
// and nothing else), 8 floats per slot: origin, t_min, direction, t_max -- the layout ptc_intersect_rays takes.
template <bool kLens>
__global__ __launch_bounds__(256) void k_generate_rays(DCamera cam, uint32_t iteration, DBand band, uint32_t pix_count, DLens lens, float4* rays)
{
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= pix_count) return;
  Minstd rng;
  Ray ray;
  primary_ray<kLens>(cam, band_pixel(band, s), iteration, rng, ray, lens);
  rays[2u * (size_t)s] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.tmin);
  rays[2u * (size_t)s + 1u] = make_float4(ray.d.x, ray.d.y, ray.d.z, ray.tmax);
}

// A run of sphere objects that does not end the object list (the spheres in front of a mesh), continuing from /
// handing on the closest hit in the hit record.  (The run that ENDS the list -- or is the whole list -- is part of
// the kernel that ends the bounce.)  (Taking the sphere runs into the traversal kernel instead was tried in round 2: inlined or as a
// call, their temporaries pushed loop-carried state of the walk into scratch, with reloads inside its hot loop.)
// kFilter: the launch is followed by a traversal launch over the mesh objects [filt_begin, filt_end).  A ray that SURELY
// misses the world boxes of all of them (the same test with the same margin by which that launch skips an instance,
// traverse4m_walk::begin_object), or whose boxes all start beyond the closest hit so far, has nothing to do there: only
// the others are put on the work list (batch-global slots, DeviceCounters::list_count per frame; their order is
// irrelevant -- results are written per slot), and the traversal launch fetches its rays through that list.  In the
// Cornell-box scenes most rays of most bounces never come near the meshes.
template <bool kFirst, bool kFilter>
// (at least six wavefronts per SIMD: 80 registers, 3-14 spilled, against 92 and five wavefronts: config 2 +2.7 %; seven: +1.7 %,
// eight (49-62 spilled): +1.1 %; profiles/r04_config2_counters.txt)
#ifndef PT_SPHERES_WAVES
#define PT_SPHERES_WAVES 6
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PT_SPHERES_WAVES, 8))) void k_spheres(DScene sc, uint32_t obj_begin, uint32_t obj_end, DPaths paths, DHits hits,
                                                 int bounce, DeviceCounters* counters, DBatchInfo bi, uint32_t filt_begin,
                                                 uint32_t filt_end, uint32_t* worklist, DTileScan scan, uint32_t tile_stride)
{
  const uint32_t frame = blockIdx.x % bi.count;  // see DBatchInfo; frame-fastest as in k_raygen
  offset_frame(paths, (size_t)frame * bi.stride);
  offset_frame(hits, (size_t)frame * bi.stride);
  counters += frame;
  scan.desc += (size_t)frame * tile_stride;
  const uint32_t n = counters->live[bounce];
  const uint32_t tiles = (n + 256u * kListPer - 1u) / (256u * kListPer);
  if (blockIdx.x / bi.count >= tiles) {
    if (kFilter && tiles == 0u && blockIdx.x / bi.count == 0u && threadIdx.x == 0u) counters->list_count = 0u;  // nothing alive: an empty list
    return;
  }
  const uint32_t tile = kFilter ? list_tile(counters, tiles) : blockIdx.x / bi.count;
  const uint32_t block_first = tile * (256u * kListPer);  // a workgroup tests kListPer x 256 consecutive slots
  uint32_t may_mask = 0u;
  // (sphere_run_lanes is for the run that ends the list: here, in front of a mesh, the spheres are typically the walls of a
  // room -- every ray hits every one of them, there is little to rule out, and sphere_segment shares the inverse
  // transform's normalised direction among them: measured 907 us against 1114 for the per-lane form, config 2)
  const bool lanes_run = PT_SPHERE_LANES_LEADING && sc.lanes_run != 0u;
  const bool fold_run = sc.fold_run != 0u;
#pragma unroll 1
  for (int j = 0; j < kListPer; ++j) {
    const uint32_t s = block_first + (uint32_t)j * 256u + threadIdx.x;
    if (s >= n) continue;
    Ray ray = load_ray(paths, s);
    if (!kFirst) {
      const float carried = ldnt(&hits.tp[s]).x;
      if (carried >= 0.0f) ray.tmax = carried;
    }
    Hit rec;
    bool changed = false;
    if (lanes_run) {
      const float4 ro4[1] = {ldnt(&paths.o4[s])}, rd4[1] = {ldnt(&paths.d4[s])};
      float4 rtp[1] = {make_float4(ray.tmax < FLT_MAX ? ray.tmax : -1.0f, 0.f, 0.f, 0.f)}, rnm[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
      changed = sphere_run_lanes<1>(sc, obj_begin, obj_end, ro4, rd4, rtp, rnm, 1u) != 0u;
      if (changed) {
        stnt(&hits.tp[s], rtp[0]);
        stnt(&hits.nm[s], rnm[0]);
        ray.tmax = rtp[0].x;
      }
    } else {
      if (fold_run) sphere_fold(sc, obj_begin, obj_end, ray, rec, changed);
      else sphere_segment<true>(sc, obj_begin, obj_end, ray, rec, changed);
      if (changed) store_hit(hits, s, rec);
    }
    if (!changed && kFirst) stnt(&hits.tp[s], make_float4(-1.0f, 0.f, 0.f, 0.f));
    if (kFilter && may_hit_boxes(sc.objects, filt_begin, filt_end, ray.o, ray.d, ray.tmax)) may_mask |= 1u << j;
  }
  if (kFilter) list_rays(may_mask, worklist, counters, (size_t)frame * bi.stride, tile, tiles, scan);
}

// "prefold": the work list of a bounce whose leading sphere run the shade kernel of the bounce before has walked for every
// survivor (shade_tile<.., kNext>): k_spheres<.., kFilter>'s list -- the flagged slots in slot order, the frame's count in
// DeviceCounters::list_count -- from the bytes that kernel left, one per slot.  A compaction of its own rather than list_rays: a
// workgroup takes 4096 consecutive slots, every thread sixteen of them in ONE 16-byte load (the first form, list_rays' 1024-slot
// tiles with a byte per load, spent 234 us per launch on 28,800 workgroups' chains of ticket, load, look-back and store: as
// long as the k_traverse4m launch behind it took to walk its rays' first nodes).  Tiles by ticket and look-back over the
// slot's descriptors as everywhere (a launch of its own epoch).
constexpr uint32_t kFlagsPer = 16u, kFlagsTile = 256u * kFlagsPer;
__global__ __launch_bounds__(256) void k_list_flags(const uint8_t* flags, int bounce, DeviceCounters* counters, DBatchInfo bi, uint32_t* worklist,
                                                    DTileScan scan, uint32_t tile_stride)
{
  __shared__ uint32_t s_wave[4];
  __shared__ uint32_t s_base, s_tile;
  const uint32_t frame = blockIdx.x % bi.count;
  const size_t fo = (size_t)frame * bi.stride;
  flags += fo;
  counters += frame;
  scan.desc += (size_t)frame * tile_stride;
  const uint32_t n = counters->live[bounce];
  const uint32_t tiles = (n + kFlagsTile - 1u) / kFlagsTile;
  if (blockIdx.x / bi.count >= tiles) {
    if (tiles == 0u && blockIdx.x / bi.count == 0u && threadIdx.x == 0u) counters->list_count = 0u;  // nothing alive: an empty list
    return;
  }
  if (threadIdx.x == 0u) {
    const uint32_t t = __hip_atomic_fetch_add(&counters->shade_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t + 1u == tiles) __hip_atomic_store(&counters->shade_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_tile = t;
  }
  __syncthreads();
  const uint32_t tile = s_tile;
  const uint32_t first = tile * kFlagsTile + threadIdx.x * kFlagsPer;  // this thread's sixteen slots: first .. first + 15
  // (the flag array is a frame's stride long and the stride a multiple of 16? not necessarily: a thread whose sixteen bytes
  // cross the live count reads them one by one)
  uint32_t bits = 0u;
  if (first + kFlagsPer <= n && ((reinterpret_cast<uintptr_t>(flags + first) & 15u) == 0u)) {
    const uint4 w = *reinterpret_cast<const uint4*>(flags + first);
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) bits |= ((ww[q] >> (8 * k)) & 0xffu) != 0u ? 1u << (4 * q + k) : 0u;
  } else {
    for (uint32_t k = 0u; k < kFlagsPer; ++k)
      if (first + k < n && flags[first + k] != 0u) bits |= 1u << k;
  }
  const uint32_t mine = (uint32_t)__popc(bits);
  // exclusive prefix within the wavefront, then across the workgroup's four
  uint32_t incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
    if ((int)(threadIdx.x & 63u) >= off) incl += up;
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 63u) s_wave[wave] = incl;
  __syncthreads();
  uint32_t before = 0u, agg = 0u;
#pragma unroll
  for (uint32_t w = 0u; w < 4u; ++w) {
    before += w < wave ? s_wave[w] : 0u;
    agg += s_wave[w];
  }
  if (wave == 0u) {
    const unsigned long long tag = (unsigned long long)scan.epoch << 34;
    if (threadIdx.x == 0u)
      __hip_atomic_store(&scan.desc[tile], tag | (tile == 0u ? kDescPrefix : kDescAggregate) | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t excl = 0u;
    if (tile != 0u) {
      excl = tile_lookback(scan.desc, tile, scan.epoch, &counters->flags);
      if (threadIdx.x == 0u)
        __hip_atomic_store(&scan.desc[tile], tag | kDescPrefix | (excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0u) {
      s_base = excl;
      if (tile + 1u == tiles) counters->list_count = excl + agg;
    }
  }
  __syncthreads();
  uint32_t at = s_base + before + (incl - mine);
  while (bits != 0u) {
    const uint32_t k = (uint32_t)__ffs((int)bits) - 1u;
    bits &= bits - 1u;
    worklist[fo + at++] = (uint32_t)fo + first + k;
  }
}

// The end of a bounce's closest-hit stage: the sphere run that ends the object list (if any) and the live count of
// every 64-slot chunk (ballot / popcount of "the hit record holds a hit"), for the compaction scan.
// kSpheres: objects [obj_begin, obj_end) are tested; kFirst: nothing has written the hit record in this bounce yet.
// kEmit: the scene has an emissive material; a hit on one ends the path (k_shade) and is not counted live.
// kRoulette: the bounce plays Russian roulette: a hit that would go on makes the roulette decision here, from
// the throughput that came into the bounce, and is not counted live when it ends.  Both are goes_on (pt_shade_tile.inc), which
// k_shade asks as well.
// 256-thread workgroups: one wavefront per SIMD fits beside the other stream's persistent traversal wavefronts as soon
// as one of those has left (1024-thread workgroups wait until four per SIMD have: measured 15 % slower end to end,
// together with a scan fused in behind a "last workgroup" sign-off).
template <bool kSpheres, bool kFirst, bool kEmit = false, bool kRoulette = false>
__global__ __launch_bounds__(256) void k_tail_count(DScene sc, uint32_t obj_begin, uint32_t obj_end, DPaths paths, DHits hits,
                                                    int bounce, uint32_t* chunk_counts, DeviceCounters* counters, DBatchInfo bi,
                                                    const uint32_t* slot_base)
{
  const uint32_t frame = blockIdx.y;  // see DBatchInfo
  offset_frame(paths, (size_t)frame * bi.stride);
  offset_frame(hits, (size_t)frame * bi.stride);
  chunk_counts += (size_t)frame * bi.chunk_stride;
  counters += frame;
  const uint32_t n = counters->live[bounce];
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  // a wavefront beyond the live range owns no chunk: k_scan reads ceil(n / 64) entries, and in a batch the next
  // entries belong to the next frame
  if ((s & ~63u) >= n) return;
  bool hit = false;
  if (s < n) {
    float t_so_far = -1.0f;
    if (!kFirst) t_so_far = ldnt(&hits.tp[s]).x;
    hit = t_so_far >= 0.0f;
    float through_x = 1.0f;  // (kRoulette: d4.w, from the sphere run's own load of the ray when there is one)
    uint32_t mat_word = 0u;
    bool have_word = false;  // the hit is the sphere run's: its material is at hand
    if (kSpheres) {
      Ray ray = kRoulette ? load_ray(paths, s, through_x) : load_ray(paths, s);
      if (hit) ray.tmax = t_so_far;
      Hit rec;
      bool changed = false;
      sphere_segment(sc, obj_begin, obj_end, ray, rec, changed);
      if (changed) {
        store_hit(hits, s, rec);
        hit = have_word = true;
        mat_word = rec.mat;
      } else if (kFirst) {
        stnt(&hits.tp[s], make_float4(-1.0f, 0.f, 0.f, 0.f));
      }
    }
    if ((kEmit || kRoulette) && hit) {  // (the host picks a kRoulette instance for no last bounce: every hit that goes on plays)
      if (kEmit && !have_word) mat_word = __float_as_uint(ldnt(&hits.nm[s]).w);
      const auto through = [&]() -> f3 {  // (loaded for a hit that plays only)
        const float2 t2 = bounce == 0 ? make_float2(1.0f, 1.0f) : ldnt(&paths.t2[s]);
        if (!kSpheres) through_x = ldnt(&paths.d4[s]).w;
        return mk3(bounce == 0 ? 1.0f : through_x, t2.x, t2.y);
      };
      f3 c;
      bool ended;
      hit = goes_on<kEmit, kRoulette>(sc, mat_word, through, c, (slot_base ? *slot_base : 0u) + s, bi.iteration[frame], (uint32_t)bounce, ended);
    }
  }
  const uint64_t live = __ballot(hit);  // (kEmit, kRoulette: hits that go on)
  if ((threadIdx.x & 63u) == 0u) chunk_counts[s / kChunk] = (uint32_t)__popcll(live);
}

// Exclusive scan of the per-chunk live counts (one workgroup; <= ~32k chunks at 1080p).
// Writes live[bounce+1] (0 after the last bounce: nothing survives the cap) and the ray counter.
__global__ __launch_bounds__(1024) void k_scan(int bounce, int last_bounce, const uint32_t* chunk_counts,
                                               uint32_t* chunk_offsets, DeviceCounters* counters, DBatchInfo bi)
{
  __shared__ uint32_t s_wave[16];
  __shared__ uint32_t s_carry;
  const uint32_t frame = blockIdx.x;  // one workgroup per frame of the batch
  chunk_counts += (size_t)frame * bi.chunk_stride;
  chunk_offsets += (size_t)frame * bi.chunk_stride;
  counters += frame;
  const uint32_t n = counters->live[bounce];
  const uint32_t chunks = (n + kChunk - 1u) / kChunk;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0u) s_carry = 0u;
  __syncthreads();
  for (uint32_t base = 0; base < chunks; base += 1024u) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < chunks ? chunk_counts[i] : 0u;
    // inclusive scan inside the wavefront
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off, 64);
      if (lane >= (uint32_t)off) x += y;
    }
    if (lane == 63u) s_wave[wave] = x;
    __syncthreads();
    uint32_t wave_prefix = 0u;
    for (uint32_t w = 0; w < wave; ++w) wave_prefix += s_wave[w];
    const uint32_t carry = s_carry;
    if (i < chunks) chunk_offsets[i] = carry + wave_prefix + x - v;
    __syncthreads();
    if (threadIdx.x == 1023u) s_carry = carry + wave_prefix + x;
    __syncthreads();
  }
  if (threadIdx.x == 0u) {
    counters->live[bounce + 1] = last_bounce ? 0u : s_carry;
    counters->rays_total += n;
    counters->paths[bounce] += n;
  }
}

// k_shade<kEmit, kRoulette> and k_shade_fused<kSpheres, kFirst, kNext, kEmit, kRoulette>: pt_shade_end.inc, one text for these and for the
// environment's instances (k_shade_env, k_shade_fused_env: pt_env.hip)
#define PT_SHADE_ENV 0
#include "pt_shade_end.inc"
#undef PT_SHADE_ENV

// Ray sorting ("ray_sort", BASELINE.json's ray-sorted wavefront; the reference keeps a sort_by_key by material
// commented out, path_tracer.cu:439-446).  The slots -- and with them the random numbers, which are keyed on the
// compacted slot index -- are NOT permuted: what is sorted is the ORDER in which the persistent traversal lanes pick
// their rays up.  Within every block of 4096 consecutive slots (neighbouring pixels: neighbouring ray origins) the
// rays are grouped by direction octant, stably, into an index array the ray feed reads through; a wavefront's 64 rays
// then start close together AND head the same way.  Results cannot change; what it buys is measured in DESIGN.md.
constexpr uint32_t kSortBlock = 4096u;
__global__ __launch_bounds__(1024) void k_sort_octant(const uint8_t* octs, uint32_t* order, int bounce, DeviceCounters* counters,
                                                      DBatchInfo bi)
{
  __shared__ uint32_t s_cnt[8][4][16];  // [octant][round][wavefront]
  __shared__ uint32_t s_base[8][4][16];
  const uint32_t frame = blockIdx.y;
  const uint32_t n = counters[frame].live[bounce];
  const uint32_t block0 = blockIdx.x * kSortBlock;
  if (block0 >= n) return;
  const size_t fbase = (size_t)frame * bi.stride;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t oct[4], rank[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t s = block0 + (uint32_t)r * 1024u + threadIdx.x;
    oct[r] = s < n ? (uint32_t)octs[fbase + s] : 8u;
#pragma unroll
    for (uint32_t o = 0; o < 8u; ++o) {
      const uint64_t m = __ballot(oct[r] == o);
      if (oct[r] == o) rank[r] = rank_below(m);
      if (lane == 0u) s_cnt[o][r][wave] = (uint32_t)__popcll(m);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0u) {  // 512 counters: exclusive scan in (octant, round, wavefront) order
    uint32_t run = 0u;
    for (int o = 0; o < 8; ++o)
      for (int r = 0; r < 4; ++r)
        for (int w = 0; w < 16; ++w) {
          s_base[o][r][w] = run;
          run += s_cnt[o][r][w];
        }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t s = block0 + (uint32_t)r * 1024u + threadIdx.x;
    if (oct[r] < 8u) order[fbase + block0 + s_base[oct[r]][r][wave] + rank[r]] = (uint32_t)fbase + s;
  }
}


// final_gather (path_tracer.cu:203-219) of the batch's staged samples into the accumulated framebuffers, in
// iteration order (running means do not commute)
__global__ __launch_bounds__(256) void k_accumulate(DFrame stage, DFrame fb, uint32_t pix_count, DBatchInfo bi)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= pix_count) return;
  // The running means of a pixel stay in registers over the frames of the batch (one read and one write of the
  // framebuffer per batch; the same operations in the same order as a fold frame by frame), and the staged samples are
  // requested eight frames at a time: one after the other, a thread of a 32-frame batch sat through 32 dependent round
  // trips and the kernel moved 2.3 TB/s.
  const uint32_t first = bi.iteration[0];
  float4 col = make_float4(0.f, 0.f, 0.f, 0.f), nd = make_float4(0.f, 0.f, 0.f, 0.f);
  if (first != 0u) {
    col = ldnt(&fb.color4[i]);
    nd = ldnt(&fb.nd4[i]);
  }
  constexpr uint32_t kAhead = 8u;
  for (uint32_t f0 = 0; f0 < bi.count; f0 += kAhead) {
    float4 c[kAhead], g[kAhead];
#pragma unroll
    for (uint32_t k = 0; k < kAhead; ++k) {
      const uint32_t f = min(f0 + k, bi.count - 1u);
      c[k] = ldnt(&stage.color4[(size_t)f * bi.stride + i]);
      g[k] = ldnt(&stage.nd4[(size_t)f * bi.stride + i]);
    }
#pragma unroll
    for (uint32_t k = 0; k < kAhead; ++k) {
      if (f0 + k >= bi.count) break;
      const uint32_t it = bi.iteration[f0 + k];
      col.x = running_mean(it, col.x, c[k].x);
      col.y = running_mean(it, col.y, c[k].y);
      col.z = running_mean(it, col.z, c[k].z);
      nd.x = running_mean(it, nd.x, g[k].x);
      nd.y = running_mean(it, nd.y, g[k].y);
      nd.z = running_mean(it, nd.z, g[k].z);
      nd.w = running_mean(it, nd.w, g[k].w);
    }
  }
  col.w = 0.0f;
  stnt(&fb.color4[i], col);
  stnt(&fb.nd4[i], nd);
}


// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// (div_up, with_flags: pt_launch_flags.hpp)

void launch_raygen(hipStream_t s, const DCameras& cams, const DBatchInfo& bi, DBand band, uint32_t pix_count,
                   DPaths paths, DeviceCounters* counters, const DObject* objects, uint32_t filt_begin, uint32_t filt_end,
                   uint32_t* worklist, DHits hits, unsigned long long* tile_desc, uint32_t tile_stride, uint32_t epoch,
                   bool finish_misses, DFrame fb, bool staged, DLens lens, DEnv env)
{
  const dim3 grid(div_up(pix_count, 256u * kListPer) * bi.count), block(256);
  const DTileScan scan{tile_desc, epoch};
  // an environment: ray generation meets the sky only where it finishes the unlisted rays itself
  if (env.texels && finish_misses && worklist && filt_begin < filt_end && tile_desc)
    return launch_raygen_env(s, cams, bi, band, pix_count, paths, counters, objects, filt_begin, filt_end, worklist, hits, tile_desc, tile_stride,
                             epoch, fb, staged, lens, env);
  if (lens.radius > 0.0f) {  // the thin lens: the same three choices, the lens instances
    const bool filter = worklist && filt_begin < filt_end && tile_desc;
    with_flags(
        [&](auto kFilter, auto kFinish) {
          if constexpr (decltype(kFilter)::value || !decltype(kFinish)::value)
            hipLaunchKernelGGL((k_raygen_lens<decltype(kFilter)::value, decltype(kFinish)::value>), grid, block, 0, s, cams, bi, band, pix_count, paths,
                               counters, objects, filter ? filt_begin : 0u, filter ? filt_end : 0u, worklist, hits, scan, tile_stride, fb,
                               decltype(kFinish)::value && staged ? 1 : 0, lens);
        },
        filter, filter && finish_misses);
    return;
  }
  if (worklist && filt_begin < filt_end && tile_desc) {
    if (finish_misses)
      hipLaunchKernelGGL((k_raygen<true, true>), grid, block, 0, s, cams, bi, band, pix_count, paths, counters, objects, filt_begin,
                         filt_end, worklist, hits, scan, tile_stride, fb, staged ? 1 : 0);
    else
      hipLaunchKernelGGL((k_raygen<true, false>), grid, block, 0, s, cams, bi, band, pix_count, paths, counters, objects, filt_begin,
                         filt_end, worklist, hits, scan, tile_stride, fb, 0);
  } else {
    hipLaunchKernelGGL((k_raygen<false, false>), grid, block, 0, s, cams, bi, band, pix_count, paths, counters, objects, 0u, 0u, worklist,
                       hits, scan, tile_stride, fb, 0);
  }
}
void launch_raygen_next(hipStream_t s, const DScene& scene, const DCameras& cams, const DBatchInfo& bi, DBand band, uint32_t pix_count, DPaths paths,
                        DeviceCounters* counters, const DNextRun& next, DLens lens)
{
  const dim3 grid(div_up(pix_count, 256u * kListPer) * bi.count), block(256);
  if (lens.radius > 0.0f) hipLaunchKernelGGL(k_raygen_next_lens, grid, block, 0, s, scene, cams, bi, band, pix_count, paths, counters, next, lens);
  else hipLaunchKernelGGL(k_raygen_next, grid, block, 0, s, scene, cams, bi, band, pix_count, paths, counters, next);
}
void launch_generate_rays(hipStream_t s, const DCamera& cam, uint32_t iteration, DBand band, uint32_t pix_count, DLens lens, float4* rays)
{
  const dim3 grid(div_up(pix_count, 256u)), block(256);
  if (lens.radius > 0.0f) hipLaunchKernelGGL(k_generate_rays<true>, grid, block, 0, s, cam, iteration, band, pix_count, lens, rays);
  else hipLaunchKernelGGL(k_generate_rays<false>, grid, block, 0, s, cam, iteration, band, pix_count, lens, rays);
}
void launch_spheres(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, bool first, DPaths paths, DHits hits,
                    uint32_t max_paths, int bounce, DeviceCounters* counters, const DBatchInfo& bi, uint32_t filt_begin,
                    uint32_t filt_end, uint32_t* worklist, unsigned long long* tile_desc, uint32_t tile_stride, uint32_t epoch)
{
  const dim3 grid(div_up(max_paths, 256u * kListPer) * bi.count), block(256);
  const DTileScan scan{tile_desc, epoch};
  with_flags(
      [&](auto kFirst, auto kFilter) {
        hipLaunchKernelGGL((k_spheres<decltype(kFirst)::value, decltype(kFilter)::value>), grid, block, 0, s, scene, obj_begin, obj_end, paths, hits,
                           bounce, counters, bi, filt_begin, filt_end, worklist, scan, tile_stride);
      },
      first, worklist && filt_begin < filt_end && tile_desc);
}
void launch_list_flags(hipStream_t s, const uint8_t* flags, uint32_t max_paths, int bounce, DeviceCounters* counters, const DBatchInfo& bi,
                       uint32_t* worklist, unsigned long long* tile_desc, uint32_t tile_stride, uint32_t epoch)
{
  const dim3 grid(div_up(max_paths, kFlagsTile) * bi.count), block(256);
  const DTileScan scan{tile_desc, epoch};
  hipLaunchKernelGGL(k_list_flags, grid, block, 0, s, flags, bounce, counters, bi, worklist, scan, tile_stride);
}
void launch_tail_count(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, bool first, DPaths paths,
                       DHits hits, uint32_t max_paths, int bounce, uint32_t* chunk_counts, DeviceCounters* counters,
                       const DBatchInfo& bi, bool emitters, bool roulette, const uint32_t* slot_base)
{
  const dim3 grid(div_up(max_paths, 256u), bi.count), block(256);
  // spheres: there is a run to test; without one some closest-hit launch has written every record of the bounce (so: not first)
  const bool spheres = obj_begin < obj_end;
  with_flags(
      [&](auto kSpheres, auto kFirst, auto kEmit, auto kRoulette) {
        if constexpr (decltype(kSpheres)::value || !decltype(kFirst)::value)
          hipLaunchKernelGGL((k_tail_count<decltype(kSpheres)::value, decltype(kFirst)::value, decltype(kEmit)::value, decltype(kRoulette)::value>),
                             grid, block, 0, s, scene, spheres ? obj_begin : 0u, spheres ? obj_end : 0u, paths, hits, bounce, chunk_counts,
                             counters, bi, slot_base);
      },
      spheres, spheres && first, emitters, roulette);  // (roulette: a bounce that plays)
}
void launch_scan(hipStream_t s, int bounce, bool last_bounce, const uint32_t* chunk_counts, uint32_t* chunk_offsets,
                 DeviceCounters* counters, const DBatchInfo& bi)
{
  hipLaunchKernelGGL(k_scan, dim3(bi.count), dim3(1024), 0, s, bounce, last_bounce ? 1 : 0, chunk_counts, chunk_offsets,
                     counters, bi);
}
void launch_shade(hipStream_t s, const DScene& scene, DPaths in, DPaths out, DHits hits, uint32_t max_paths,
                  bool staged, int bounce, bool last_bounce, const uint32_t* slot_base,
                  const uint32_t* chunk_offsets, DFrame fb, DBand band, DeviceCounters* counters, uint8_t* octs,
                  const DBatchInfo& bi, bool emitters, bool roulette, DEnv env)
{
  if (env.texels)  // an environment: its instances, built with kEmit on (pt_env.hip)
    return launch_shade_env(s, scene, in, out, hits, max_paths, staged, bounce, last_bounce, slot_base, chunk_offsets, fb, band, counters, octs, bi,
                            roulette, env);
  with_flags(
      [&](auto kEmit, auto kRoulette) {
        hipLaunchKernelGGL((k_shade<decltype(kEmit)::value, decltype(kRoulette)::value>), dim3(div_up(max_paths, 256u), bi.count), dim3(256), 0, s,
                           scene, in, out, hits, staged ? 1 : 0, bounce, last_bounce ? 1 : 0, slot_base, chunk_offsets, fb, band, counters, octs, bi);
      },
      emitters, roulette);  // (roulette: a bounce that plays)
}
void launch_shade_fused(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, bool first, DPaths in, DPaths out,
                        DHits hits, uint32_t max_paths, bool staged, int bounce, bool last_bounce, const uint32_t* slot_base,
                        unsigned long long* tile_desc, uint32_t tile_stride, uint32_t epoch, DFrame fb, DBand band,
                        DeviceCounters* counters, uint8_t* octs, const DBatchInfo& bi, const uint32_t* list, const DNextRun* next,
                        bool emitters, bool roulette, DEnv env)
{
  if (env.texels)  // an environment: its instances, built with kEmit on (pt_env.hip)
    return launch_shade_fused_env(s, scene, obj_begin, obj_end, first, in, out, hits, max_paths, staged, bounce, last_bounce, slot_base, tile_desc,
                                  tile_stride, epoch, fb, band, counters, octs, bi, list, next, roulette, env);
  const dim3 grid(div_up(max_paths, kFuseTile) * bi.count), block(256);
  const DNextRun none{};
  // prefold: the next bounce's leading sphere run rides along; spheres: a run ends the object list (without one, and first: a
  // scene without objects, every ray misses; not first: some closest-hit launch has written every record of the bounce).
  // emitters: the scene has an emissive material; roulette: a bounce that plays (the caller asks for none at
  // the last bounce) -- the same six instances again with kEmit, and those twelve with kRoulette.
  const bool prefold = next && !first && !last_bounce;
  with_flags(
      [&](auto kSpheres, auto kFirst, auto kNext, auto kEmit, auto kRoulette) {
        if constexpr (!(decltype(kFirst)::value && decltype(kNext)::value))
          hipLaunchKernelGGL((k_shade_fused<decltype(kSpheres)::value, decltype(kFirst)::value, decltype(kNext)::value, decltype(kEmit)::value,
                                            decltype(kRoulette)::value>),
                             grid, block, 0, s, scene, obj_begin, obj_end, in, out, hits, staged ? 1 : 0, bounce, last_bounce ? 1 : 0, slot_base,
                             tile_desc, tile_stride, epoch, fb, band, counters, octs, bi, list, next ? *next : none);
      },
      obj_begin < obj_end, first && !prefold, prefold, emitters, roulette);
}
uint32_t shade_tiles_per_frame(uint32_t max_paths) { return div_up(max_paths, kFuseTile); }
void launch_sort_octant(hipStream_t s, const uint8_t* octs, uint32_t* order, uint32_t max_paths, int bounce,
                        DeviceCounters* counters, const DBatchInfo& bi)
{
  hipLaunchKernelGGL(k_sort_octant, dim3(div_up(max_paths, kSortBlock), bi.count), dim3(1024), 0, s, octs, order, bounce, counters, bi);
}
void launch_accumulate(hipStream_t s, DFrame stage, DFrame fb, uint32_t pix_count, const DBatchInfo& bi)
{
  hipLaunchKernelGGL(k_accumulate, dim3(div_up(pix_count, 256u)), dim3(256), 0, s, stage, fb, pix_count, bi);
}
}  // namespace pt
