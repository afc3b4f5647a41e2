// ptcore_checks.cpp -- host-side checks of the rules the kernels share with the host (ptc_check_beam, ptc_check_beam_frustum, ptc_check_feed,
// ptc_check_traversal_layout, ptc_check_rng, ptc_check_light_sample), ptc_debug_beam_entries, ptc_debug_sphere_lanes, ptc_selftest_math, ptc_selftest_rng, and
// ptc_generate_rays (the frame's primary rays as ray generation builds them).  Part of libptcore.so (ptcore_ctx.hpp).
#include "ptcore_ctx.hpp"
#include "pt_mega_rules.hpp"
#include "pt_rng.hpp"
#include "pt_light_sample.hpp"
#include "pt_demodulate.hpp"
#include "pt_denoise_variance.hpp"

using namespace pt;
using namespace ptcd;

extern "C" {

// Entry points for primary rays (pt_beam_rules.hpp) checked on the host: for a mesh, an object matrix, a camera and a
// resolution, every tile's entries as k_beam computes them (same functions), then for sample rays of the tile -- the
// corners and the centre of the jitter range of every `stride`-th pixel -- the closest hit of a plain walk over the
// four-wide quantised tree started at the ROOT against the same walk started at the tile's ENTRIES: triangle and t must
// agree.  Returns the number of rays that disagree (0 = sound), or a negative status; stats (may be NULL): tiles, tiles
// without entries, entries in total, rays checked, rays that hit.
int ptc_check_beam(const float* positions, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count, const float* object_m16,
                   const ptc_camera* camera, uint32_t width, uint32_t height, uint32_t stride, uint64_t* stats5, float* entries_out)
{
  if (!positions || !indices || !camera || index_count == 0u || index_count % 3u || width < 2u || height < 2u || stride == 0u) return PTC_ERR_INVALID;
  std::vector<ptc_bvh_node> nodes((size_t)index_count / 3u * 2u);
  uint32_t depth = 0;
  const int rc = build_bvh(positions, vertex_count, indices, index_count, nodes.data(), &depth);
  if (rc < 0) return rc;
  WideAccel wide;
  if (int r = build_wide(nodes.data(), (uint32_t)rc, wide)) return r;
  Wide4Accel w4;
  if (int r = build_wide4(nodes.data(), (uint32_t)rc, w4)) return r;
  m4 m{};
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) m.c[c][r] = object_m16 ? object_m16[4 * c + r] : (c == r ? 1.0f : 0.0f);
  const m4 inv_m = inverse(m);
  const DCamera cam = make_camera(*camera, width, height);
  auto gen = [&](float fx, float fy, f3& o, f3& d) {  // generate_ray (pt_kernels.hip), the same operations
    const float u = fx / (float)(cam.width - 1u);
    const float v = ((float)cam.height - fy) / (float)(cam.height - 1u);
    const float dx = cam.llx + cam.vw * u;
    const float dy = cam.lly + cam.vh * v;
    o = cam.origin;
    d = normalize(xform_vector(cam.cam, mk3(dx, dy, -1.0f)));
  };
  const uint32_t* nq = w4.nodes_q.data();
  const uint32_t n4 = (uint32_t)(w4.nodes_q.size() / 16u);
  const f3 root_lo = mk3(wide.root_min[0], wide.root_min[1], wide.root_min[2]), root_hi = mk3(wide.root_max[0], wide.root_max[1], wide.root_max[2]);
  // closest hit of the plain walk from a set of start references (boxes tested first)
  struct HitRec { bool hit; uint32_t rank; float t; };
  auto slab = [](const f3 lo, const f3 hi, const f3 o, const f3 inv, float tmax) {
    float tn = 0.0f, tf = tmax;
    const float lo_[3] = {lo.x, lo.y, lo.z}, hi_[3] = {hi.x, hi.y, hi.z}, o_[3] = {o.x, o.y, o.z}, i_[3] = {inv.x, inv.y, inv.z};
    for (int a = 0; a < 3; ++a) {
      const float t0 = (lo_[a] - o_[a]) * i_[a], t1 = (hi_[a] - o_[a]) * i_[a];
      tn = std::max(tn, std::min(t0, t1));
      tf = std::min(tf, std::max(t0, t1));
    }
    return tn <= tf * 1.000001f + 1e-6f;
  };
  auto walk = [&](const f3 o, const f3 d, const f3* lo4, const f3* hi4, const uint32_t* ref4, int n) {
    HitRec best{false, 0u, 3.0e38f};
    const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    std::vector<uint32_t> stack;
    for (int k = 0; k < n; ++k)
      if (slab(lo4[k], hi4[k], o, inv, best.t)) stack.push_back(ref4[k]);
    while (!stack.empty()) {
      const uint32_t ref = stack.back();
      stack.pop_back();
      if (ref & kLeafBit) {
        const uint32_t rank = ref & ~kLeafBit;
        if (rank >= wide.tri_order.size()) continue;  // the dummy
        const uint32_t tri = wide.tri_order[rank];
        const f3 p0 = mk3(positions[3 * indices[3 * tri]], positions[3 * indices[3 * tri] + 1], positions[3 * indices[3 * tri] + 2]);
        const f3 p1 = mk3(positions[3 * indices[3 * tri + 1]], positions[3 * indices[3 * tri + 1] + 1], positions[3 * indices[3 * tri + 1] + 2]);
        const f3 p2 = mk3(positions[3 * indices[3 * tri + 2]], positions[3 * indices[3 * tri + 2] + 1], positions[3 * indices[3 * tri + 2] + 2]);
        const f3 e1 = p1 - p0, e2 = p2 - p0, h = cross(d, e2);
        const float a = dot(e1, h);
        if (a > -1e-12f && a < 1e-12f) continue;
        const float f = 1.0f / a;
        const f3 sv = o - p0;
        const float u = f * dot(sv, h);
        if (u < 0.0f || u > 1.0f) continue;
        const f3 q = cross(sv, e1);
        const float v = f * dot(d, q);
        if (v < 0.0f || u + v > 1.0f) continue;
        const float t = f * dot(e2, q);
        if (t < 1e-4f) continue;
        if (t < best.t || (t == best.t && rank > best.rank)) best = HitRec{true, rank, t};
        continue;
      }
      if (ref >= n4) return HitRec{true, 0xffffffffu, -1.0f};  // a reference out of range: reported as a disagreement
      const uint32_t* q = nq + 16u * (size_t)ref;
      for (int c = 0; c < 4; ++c) {
        f3 lo, hi;
        if (!beam_rules::child_box(q, c, lo, hi)) continue;
        if (slab(lo, hi, o, inv, best.t)) stack.push_back(q[12 + c]);
      }
    }
    return best;
  };
  uint64_t tiles = 0, empty = 0, entries = 0, rays = 0, hits = 0;
  int bad = 0;
  const uint32_t tiles_x = (width + kBeamTile - 1u) / kBeamTile, tiles_y = (height + kBeamTile - 1u) / kBeamTile;
  const uint32_t root_ref4[1] = {w4.root_ref};
  for (uint32_t ty = 0; ty < tiles_y; ++ty)
    for (uint32_t tx = 0; tx < tiles_x; ++tx) {
      const float x0 = (float)(tx * kBeamTile) - 0.05f, x1 = (float)((tx + 1u) * kBeamTile) + 0.05f;
      const float y0 = (float)(ty * kBeamTile) - 0.05f, y1 = (float)((ty + 1u) * kBeamTile) + 0.05f;
      const beam_rules::Frustum fr = beam_rules::tile_frustum(cam.cam, cam.origin, cam.llx, cam.lly, cam.vw, cam.vh, cam.width, cam.height, inv_m, x0, x1, y0, y1);
      f3 lo4[4], hi4[4];
      uint32_t ref4[4];
      const int n = beam_rules::tile_entries(nq, n4, w4.root_ref, root_lo, root_hi, fr, lo4, hi4, ref4);
      if (entries_out) {  // as k_beam stores them: {box min, reference bits} {box max, 0}; unused: an inside-out box
        float* e = entries_out + ((size_t)ty * tiles_x + tx) * 32u;
        for (int k = 0; k < 4; ++k) {
          const float inf = __builtin_inff();
          uint32_t ref = k < n ? ref4[k] : kNoChild;
          float refbits;
          std::memcpy(&refbits, &ref, 4);
          const float rec[8] = {k < n ? lo4[k].x : inf, k < n ? lo4[k].y : inf, k < n ? lo4[k].z : inf, refbits,
                                k < n ? hi4[k].x : -inf, k < n ? hi4[k].y : -inf, k < n ? hi4[k].z : -inf, 0.0f};
          std::memcpy(e + 8 * k, rec, sizeof rec);
        }
      }
      ++tiles;
      empty += n == 0;
      entries += (uint64_t)n;
      for (int k = 0; k < n; ++k)
        if (!(ref4[k] & kLeafBit) && ref4[k] >= n4) ++bad;
      for (uint32_t py = ty * kBeamTile; py < std::min(height, (ty + 1u) * kBeamTile); py += stride)
        for (uint32_t px = tx * kBeamTile; px < std::min(width, (tx + 1u) * kBeamTile); px += stride) {
          const float jit[5][2] = {{0.0f, 0.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}, {1.0f, 1.0f}, {0.5f, 0.5f}};  // (uniform_real can round to 1)
          for (const auto& j : jit) {
            f3 ro, rd;
            gen((float)px + j[0], (float)py + j[1], ro, rd);
            const f3 oo = xform_point(inv_m, ro), od = xform_vector(inv_m, rd);
            const HitRec a = walk(oo, od, &root_lo, &root_hi, root_ref4, 1);
            const HitRec b = walk(oo, od, lo4, hi4, ref4, n);
            ++rays;
            hits += a.hit;
            if (a.hit != b.hit || (a.hit && (a.rank != b.rank || a.t != b.t))) ++bad;
          }
        }
    }
  if (stats5) {
    stats5[0] = tiles;
    stats5[1] = empty;
    stats5[2] = entries;
    stats5[3] = rays;
    stats5[4] = hits;
  }
  return bad;
}

// The tile frustums of ptc_check_beam / k_beam by themselves (pt_beam_rules.hpp: tile_frustum, the same call), without a mesh: per
// tile 16 floats {eye.xyz, usable (1 or 0), n[0].xyz, n[1].xyz, n[2].xyz, n[3].xyz} into frusta_out [tiles][16], and the binary32
// constants the rule read into consts39 (may be NULL): the camera matrix (16, column-major), its origin (3), vw, vh, llx, lly, and the
// object's inverse matrix (16).  Returns the number of tiles or a negative status.
int ptc_check_beam_frustum(const float* object_m16, const ptc_camera* camera, uint32_t width, uint32_t height, float* frusta_out,
                           uint64_t capacity_floats, float* consts39)
{
  if (!camera || !frusta_out || width < 2u || height < 2u) return PTC_ERR_INVALID;
  const uint32_t tiles_x = (width + kBeamTile - 1u) / kBeamTile, tiles_y = (height + kBeamTile - 1u) / kBeamTile;
  if ((uint64_t)tiles_x * tiles_y > 0x7fffffffull || capacity_floats < (uint64_t)tiles_x * tiles_y * 16u) return PTC_ERR_INVALID;
  m4 m{};
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) m.c[c][r] = object_m16 ? object_m16[4 * c + r] : (c == r ? 1.0f : 0.0f);
  const m4 inv_m = inverse(m);
  const DCamera cam = make_camera(*camera, width, height);
  if (consts39) {
    std::memcpy(consts39, cam.cam.c, 16 * sizeof(float));
    const float rest[7] = {cam.origin.x, cam.origin.y, cam.origin.z, cam.vw, cam.vh, cam.llx, cam.lly};
    std::memcpy(consts39 + 16, rest, sizeof rest);
    std::memcpy(consts39 + 23, inv_m.c, 16 * sizeof(float));
  }
  for (uint32_t ty = 0; ty < tiles_y; ++ty)
    for (uint32_t tx = 0; tx < tiles_x; ++tx) {
      const float x0 = (float)(tx * kBeamTile) - 0.05f, x1 = (float)((tx + 1u) * kBeamTile) + 0.05f;
      const float y0 = (float)(ty * kBeamTile) - 0.05f, y1 = (float)((ty + 1u) * kBeamTile) + 0.05f;
      const beam_rules::Frustum fr = beam_rules::tile_frustum(cam.cam, cam.origin, cam.llx, cam.lly, cam.vw, cam.vh, cam.width, cam.height, inv_m, x0, x1, y0, y1);
      float* e = frusta_out + ((size_t)ty * tiles_x + tx) * 16u;
      const float rec[16] = {fr.eye.x, fr.eye.y, fr.eye.z, fr.usable ? 1.0f : 0.0f, fr.n[0].x, fr.n[0].y, fr.n[0].z, fr.n[1].x, fr.n[1].y, fr.n[1].z,
                             fr.n[2].x, fr.n[2].y, fr.n[2].z, fr.n[3].x, fr.n[3].y, fr.n[3].z};
      std::memcpy(e, rec, sizeof rec);
    }
  return (int)(tiles_x * tiles_y);
}

// The ray feed of the persistent traversal launches (BatchFeed; pt_feed_rules.hpp) checked on the host: a frame of n rays,
// its eight regions, each dealt as static_eighths / 8 static batches of 64 followed by dynamic batches of dyn_batch (64 or
// 128) rays.  Every ray of the frame must be handed out exactly once, every batch must be contiguous in the frame's order
// and inside the frame.  Returns the number of violations (0 = sound) or a negative status.
int ptc_check_feed(uint32_t n, uint32_t static_eighths, uint32_t dyn_batch)
{
  if (static_eighths > 8u || (dyn_batch != 64u && dyn_batch != 128u) || n > (1u << 28)) return PTC_ERR_INVALID;
  std::vector<uint8_t> seen(n, 0);
  int bad = 0;
  auto hand_out = [&](uint32_t begin, uint32_t end) {
    if (end > n || begin >= end) { ++bad; return; }
    for (uint32_t q = begin; q < end; ++q) {
      if (seen[q]) ++bad;
      seen[q] = 1;
    }
  };
  const uint32_t rs = feed_rules::region_size_of(n);
  uint64_t total = 0;
  for (uint32_t r = 0; r < 8u; ++r) {
    const uint32_t len = feed_rules::region_len_of(n, rs, r);
    total += len;
    const uint32_t stat = feed_rules::static_batches_of(len, static_eighths);
    if ((uint64_t)stat * 64u > len) { ++bad; continue; }
    for (uint32_t k = 0; k < stat; ++k) {  // BatchFeed::acquire, static part: full batches
      const uint32_t begin = feed_rules::pos_of(rs, r, k * 64u);
      hand_out(begin, begin + 64u);
    }
    for (uint32_t b = stat * 64u; b < len; b += dyn_batch) {  // ... dynamic part: the cursor advances by dyn_batch
      const uint32_t begin = feed_rules::pos_of(rs, r, b);
      const uint32_t count = std::min(len, b + dyn_batch) - b;
      hand_out(begin, begin + count);
      // a batch of two must be contiguous: its second half where the map puts it
      if (count > 64u && feed_rules::pos_of(rs, r, b + 64u) != begin + 64u) ++bad;
    }
  }
  if (total != n) ++bad;
  for (uint32_t q = 0; q < n; ++q)
    if (!seen[q]) ++bad;
  return bad;
}

// frame_plan (ptcore_ctx.hpp), the sizing rule ptc_resize follows, for the resolutions ptc_resize accepts.
int ptc_check_frame_plan(uint32_t width, uint32_t height, int frames_in_flight, int frames_auto, int batch_frames, int prefold,
                         ptc_frame_plan* out)
{
  if (!out || width < 2u || height < 2u || (uint64_t)width * height > 0x7fffffffull) return PTC_ERR_INVALID;
  *out = frame_plan(width, height, frames_in_flight, frames_auto != 0, batch_frames, prefold != 0);
  return PTC_OK;
}

// mega_rules::instance (pt_mega_rules.hpp), the rule launch_megakernel follows, with roulette_frame's reading of `plays`.
int ptc_check_megakernel_instance(int direct, int env, int env_lit, int smooth, int textured, int weigh, int lens, int plays, int emitters,
                                  int roulette, int max_bounces, char* name_out, uint32_t name_capacity, int* roulette_out)
{
  return ptc_check_megakernel_instance2(direct, env, env_lit, smooth, textured, weigh, lens, plays, emitters, 0, roulette, max_bounces, name_out,
                                        name_capacity, roulette_out);
}

// ... with the tenth fact
int ptc_check_megakernel_instance2(int direct, int env, int env_lit, int smooth, int textured, int weigh, int lens, int plays, int emitters,
                                   int bent, int roulette, int max_bounces, char* name_out, uint32_t name_capacity, int* roulette_out)
{
  if (!name_out || !roulette_out) return PTC_ERR_INVALID;
  mega_rules::Facts f;
  f.bent = bent != 0;
  f.direct = direct != 0;
  f.env = env != 0;
  f.env_lit = env_lit != 0;
  f.smooth = smooth != 0;
  f.textured = textured != 0;
  f.weigh = weigh != 0;
  f.lens = lens != 0;
  f.plays = plays < 0 ? roulette_frame(roulette, max_bounces) : plays != 0;
  f.emitters = emitters != 0;
  if (!mega_rules::instance_name(mega_rules::instance(f), name_out, name_capacity)) return PTC_ERR_INVALID;
  *roulette_out = mega_rules::roulette_argument(f.plays, roulette);
  return PTC_OK;
}

// Test hook: the entries k_beam computes on the GPU for the uploaded scene's first traversal launch (its mesh object) and
// `camera` at the context's resolution, [tiles][4][8 floats] as ptc_check_beam lays them out.
int ptc_debug_beam_entries(ptc_ctx* ctx, const ptc_camera* camera, float* entries_out, uint64_t capacity_floats)
{
  if (!ctx || !camera || !entries_out) return PTC_ERR_INVALID;
  if (!ctx->has_scene || !ctx->pix_capacity || ctx->launches.empty()) return fail(ctx, PTC_ERR_INVALID, "no scene / frame / mesh launch");
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  const uint32_t tx = (ctx->width + kBeamTile - 1u) / kBeamTile, ty = (ctx->height + kBeamTile - 1u) / kBeamTile;
  const size_t floats = (size_t)tx * ty * 32u;
  if (capacity_floats < floats) return fail(ctx, PTC_ERR_INVALID, "entries_out too small");
  float4* dev = nullptr;
  HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&dev), floats * sizeof(float)));
  DCameras cams{};
  cams.c[0] = make_camera(*camera, ctx->width, ctx->height);
  const uint8_t cam_of[1] = {0};
  DScene scene = ctx->scene;
  const uint32_t mesh_obj = ctx->launches[0].mesh;
  scene.cur = ctx->mesh_views[ctx->object_mesh[mesh_obj]];
  launch_beam(ctx->stream, scene, mesh_obj, cams, cam_of, 1u, tx, ty, ctx->mesh_nodes4[ctx->object_mesh[mesh_obj]], dev);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(entries_out, dev, floats * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("beam entries: ") + hipGetErrorString(e));
  return PTC_OK;
}

// Test hook: the per-lane form of a sphere run (sphere_run_lanes<slots>) on the uploaded scene's trailing run, fed with the caller's
// rays the way ptc_intersect_rays feeds the traversal launches -- t_min as the path state's flag, t_max as the closest hit carried
// in, a record nothing has written yet a miss.
int ptc_debug_sphere_lanes(ptc_ctx* ctx, const float* rays, uint32_t n, int slots, float* hit_t, float* hit_normal, uint32_t* hit_material,
                           uint8_t* hit_side, uint8_t* candidates)
{
  if (!ctx || !rays || !hit_t || !hit_normal || !hit_material || !hit_side) return PTC_ERR_INVALID;
  if (!ctx->has_scene) return fail(ctx, PTC_ERR_NO_SCENE, "no scene uploaded");
  if (!lanes_run_of(ctx, ctx->tail_begin, ctx->tail_end))
    return fail(ctx, PTC_ERR_INVALID, "the trailing sphere run does not take the per-lane form");
  if (n > 0x7fffffffu) return fail(ctx, PTC_ERR_INVALID, "too many rays");
  for (uint32_t i = 0; i < n; ++i) {
    const float* r = rays + 8u * (size_t)i;
    if (!((r[3] == 1e-4f || r[3] == 1e-5f) && r[7] >= 0.0f)) return fail(ctx, PTC_ERR_INVALID, "t_min must be 1e-4 or 1e-5, t_max >= 0");
    if (!std::isfinite(r[0] + r[1] + r[2]) || !std::isfinite(r[4] + r[5] + r[6])) return fail(ctx, PTC_ERR_INVALID, "origin and direction must be finite");
  }
  constexpr uint32_t kUntouched = 0x7fffffffu;  // material field of a record the run has not written: a miss
  float untouched_bits;
  std::memcpy(&untouched_bits, &kUntouched, 4);
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  std::vector<void*> pool;
  float4 *ro = nullptr, *rd = nullptr, *d_tp = nullptr, *d_nm = nullptr;
  uint8_t* d_cand = nullptr;
  const size_t cap = n ? n : 1u;
  int rc = dev_alloc(ctx, pool, &ro, cap);
  if (!rc) rc = dev_alloc(ctx, pool, &rd, cap);
  if (!rc) rc = dev_alloc(ctx, pool, &d_tp, cap);
  if (!rc) rc = dev_alloc(ctx, pool, &d_nm, cap);
  if (!rc && candidates) rc = dev_alloc(ctx, pool, &d_cand, cap);
  if (rc) {
    free_pool(pool);
    return rc;
  }
  std::vector<float4> ho(n), hd(n), tp(n), nm(n);
  for (uint32_t i = 0; i < n; ++i) {
    const float* r = rays + 8u * (size_t)i;
    const uint32_t flag = r[3] == 1e-5f ? 0x80000000u : 0u;
    float w;
    std::memcpy(&w, &flag, 4);
    ho[i] = make_float4(r[0], r[1], r[2], w);
    hd[i] = make_float4(r[4], r[5], r[6], 0.0f);
    // "none yet" as the kernels that call the per-lane form say it (a negative t).  With one ray per lane a cap of +inf -- a closest
    // hit of FLT_MAX times the form's 1.0001 -- would admit the unset bounds of the slots BEYOND the run as candidates, objects
    // that are not there: no distance comes near that, and the hook keeps it out
    tp[i] = make_float4(r[7] < 3.0e38f ? r[7] : -1.0f, 0.0f, 0.0f, 0.0f);
    nm[i] = make_float4(0.0f, 0.0f, 0.0f, untouched_bits);
  }
  hipError_t e = hipSuccess;
  bool known = true;
  if (n) {
    e = hipMemcpyAsync(ro, ho.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(rd, hd.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tp, tp.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_nm, nm.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
      known = launch_debug_sphere_lanes(ctx->stream, ctx->scene, ctx->tail_begin, ctx->tail_end, slots, ro, rd, d_tp, d_nm, n, d_cand);
      e = hipGetLastError();
    }
    if (e == hipSuccess && known) e = hipMemcpyAsync(tp.data(), d_tp, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && known) e = hipMemcpyAsync(nm.data(), d_nm, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && known && candidates) e = hipMemcpyAsync(candidates, d_cand, n, hipMemcpyDeviceToHost, ctx->stream);
  } else {
    known = launch_debug_sphere_lanes(ctx->stream, ctx->scene, 0u, 0u, slots, nullptr, nullptr, nullptr, nullptr, 0u, nullptr);
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  free_pool(pool);
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("sphere lanes: ") + hipGetErrorString(e));
  if (!known) return fail(ctx, PTC_ERR_INVALID, "slots must be 1 or the fused kernel's slots per lane");
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t ms;
    std::memcpy(&ms, &nm[i].w, 4);
    const bool miss = (ms & 0x7fffffffu) == kUntouched;
    hit_t[i] = miss ? -1.0f : tp[i].x;
    hit_normal[3u * i] = nm[i].x;
    hit_normal[3u * i + 1u] = nm[i].y;
    hit_normal[3u * i + 2u] = nm[i].z;
    hit_material[i] = miss ? 0u : (ms & 0x7fffffffu);
    hit_side[i] = miss ? (uint8_t)0 : (uint8_t)(ms >> 31);
  }
  return PTC_OK;
}

int ptc_check_traversal_layout(const ptc_bvh_node* nodes, uint32_t node_count, uint64_t* checked_boxes)
{
  if (!nodes || node_count == 0u) return PTC_ERR_INVALID;
  Wide4Accel w4;
  if (int rc = build_wide4(nodes, node_count, w4)) return rc;
  // the reference tree: leaf of every depth-first rank, parents, and every node's range of leaf ranks
  std::vector<uint32_t> leaf_of_rank, parent(node_count, 0xffffffffu), first_rank(node_count, 0u), last_rank(node_count, 0u);
  {
    std::vector<uint32_t> stack{0u};
    while (!stack.empty()) {
      const uint32_t i = stack.back();
      stack.pop_back();
      if (nodes[i].primitive_count != 0u) {
        first_rank[i] = last_rank[i] = (uint32_t)leaf_of_rank.size();
        leaf_of_rank.push_back(i);
      } else {
        const uint32_t l = nodes[i].first_child_or_primitive;
        if (l + 1u >= node_count) return PTC_ERR_BVH;
        parent[l] = parent[l + 1u] = i;
        stack.push_back(l + 1u);
        stack.push_back(l);
      }
    }
    for (uint32_t i = node_count; i-- > 0u;)  // children come after their parent in the reference's array
      if (nodes[i].primitive_count == 0u) {
        first_rank[i] = first_rank[nodes[i].first_child_or_primitive];
        last_rank[i] = last_rank[nodes[i].first_child_or_primitive + 1u];
      }
  }
  std::unordered_map<uint64_t, uint32_t> node_of_range;
  node_of_range.reserve(node_count * 2u);
  for (uint32_t i = 0; i < node_count; ++i) node_of_range[((uint64_t)first_rank[i] << 32) | last_rank[i]] = i;

  int bad = 0;
  uint64_t boxes = 0;
  const uint32_t triangles = (uint32_t)leaf_of_rank.size();
  std::vector<uint32_t> seen(triangles, 0u);
  if (w4.root_ref & pt::kLeafBit) {
    if (triangles != 1u || (w4.root_ref & ~pt::kLeafBit) != 0u) ++bad;
    else seen[0] = 1u;
  } else {
    const uint32_t n4 = (uint32_t)(w4.nodes_q.size() / 16u);
    // rank range of every four-wide node: children are in depth-first order and nodes in depth-first preorder,
    // so a child node has a larger index than its parent
    std::vector<uint32_t> first4(n4, 0u), last4(n4, 0u);
    for (uint32_t n = n4; n-- > 0u;) {
      const uint32_t* q = &w4.nodes_q[(size_t)n * 16u];
      bool any = false;
      for (int c = 0; c < 4; ++c) {
        const uint32_t ref = q[12 + c];
        if (ref == w4.dummy_ref) {  // unused slot: must carry the inside-out box on every axis
          for (int ax = 0; ax < 3; ++ax)
            if (((q[4 + ax] >> (8 * c)) & 0xffu) != 255u || ((q[7 + ax] >> (8 * c)) & 0xffu) != 0u) ++bad;
          continue;
        }
        uint32_t a, b;
        if (ref & pt::kLeafBit) {
          a = b = ref & ~pt::kLeafBit;
        } else {
          if (ref <= n || ref >= n4) return PTC_ERR_BVH;
          a = first4[ref];
          b = last4[ref];
        }
        if (!any) first4[n] = a;
        else if (a != last4[n] + 1u) ++bad;  // the children tile their parent's leaves in order
        last4[n] = b;
        any = true;
      }
      if (!any) ++bad;
    }
    if (w4.root_ref >= n4 || first4[w4.root_ref] != 0u || last4[w4.root_ref] + 1u != triangles) ++bad;
    for (uint32_t n = 0; n < n4 && w4.root_ref < n4; ++n) {
      const uint32_t* q = &w4.nodes_q[(size_t)n * 16u];
      float origin[3];
      std::memcpy(origin, q, 12);
      for (int c = 0; c < 4; ++c) {
        const uint32_t ref = q[12 + c];
        if (ref == w4.dummy_ref) continue;
        uint32_t a, b;
        if (ref & pt::kLeafBit) {
          a = b = ref & ~pt::kLeafBit;
          if (a < triangles) ++seen[a];
        } else {
          a = first4[ref];
          b = last4[ref];
        }
        const auto it = node_of_range.find(((uint64_t)a << 32) | b);
        if (it == node_of_range.end()) {  // the child does not stand for a node of the reference tree
          ++bad;
          continue;
        }
        const ptc_bvh_node& x = nodes[it->second];
        for (int ax = 0; ax < 3; ++ax) {
          const uint32_t step_bits = q[ax == 0 ? 3 : 9 + ax];
          if (step_bits & 0x807fffffu) ++bad;  // a power of two
          const double step = std::ldexp(1.0, (int)(step_bits >> 23) - 127);
          const double lo = (double)origin[ax] + (double)((q[4 + ax] >> (8 * c)) & 0xffu) * step;
          const double hi = (double)origin[ax] + (double)((q[7 + ax] >> (8 * c)) & 0xffu) * step;
          if (lo > (double)x.aabb_min[ax] || hi < (double)x.aabb_max[ax]) ++bad;
        }
        ++boxes;
      }
    }
  }
  for (uint32_t r = 0; r < triangles; ++r) {
    if (seen[r] != 1u) ++bad;  // every triangle is a child of exactly one four-wide node
    const uint32_t leaf = leaf_of_rank[r];
    if (parent[leaf] != 0xffffffffu) {
      const float4 p0 = w4.leaf_parent[2u * (size_t)r], p1 = w4.leaf_parent[2u * (size_t)r + 1u];
      const ptc_bvh_node& p = nodes[parent[leaf]];
      if (p0.x != p.aabb_min[0] || p0.y != p.aabb_min[1] || p0.z != p.aabb_min[2] || p1.x != p.aabb_max[0] ||
          p1.y != p.aabb_max[1] || p1.z != p.aabb_max[2])
        ++bad;
    }
  }
  if (checked_boxes) *checked_boxes = boxes;
  return bad;
}

int ptc_selftest_math(ptc_ctx* ctx, const float* a, const float* b, uint32_t n, float* out_div, float* out_sqrt,
                      float* out_sin, float* out_cos)
{
  if (!ctx || !a || !b || !out_div || !out_sqrt || !out_sin || !out_cos) return PTC_ERR_INVALID;
  if (n == 0) return PTC_OK;
  if (int rc = bind_device(ctx)) return rc;
  std::vector<void*> pool;
  float* d[6] = {};
  for (auto& p : d)
    if (int rc = dev_alloc(ctx, pool, &p, n)) {
      free_pool(pool);
      return rc;
    }
  hipError_t e = hipMemcpyAsync(d[0], a, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d[1], b, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_selftest(ctx->stream, d[0], d[1], n, d[2], d[3], d[4], d[5]);
    e = hipGetLastError();
  }
  float* outs[4] = {out_div, out_sqrt, out_sin, out_cos};
  for (int k = 0; k < 4 && e == hipSuccess; ++k)
    e = hipMemcpyAsync(outs[k], d[2 + k], n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  free_pool(pool);
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("selftest: ") + hipGetErrorString(e));
  return PTC_OK;
}

// The per-path generator (pt_rng.hpp) on the host: out[6 i ..] as k_selftest_rng writes it
int ptc_check_rng(const uint32_t* seeds, const uint32_t* discards, uint32_t n, uint32_t* out)
{
  if (n == 0) return PTC_OK;
  if (!seeds || !discards || !out) return PTC_ERR_INVALID;
  for (uint32_t i = 0; i < n; ++i) selftest_rng_one(seeds[i], discards[i], out + 6u * (size_t)i);
  return PTC_OK;
}

// The environment's lookup and apron (pt_env.hpp) on the host, as ptc_set_environment + ptc_sample_environment run
// them: no GPU, no context.  The same refusals as ptc_set_environment's, without a message.
int ptc_check_environment(const float* rgb, uint32_t n, const float* dirs, uint32_t count, float* rgb_out)
{
  if (!rgb || n < env_rules::kMinSize || n > env_rules::kMaxSize) return PTC_ERR_INVALID;
  if (count != 0u && (!dirs || !rgb_out)) return PTC_ERR_INVALID;
  for (size_t k = 0; k < 3u * (size_t)n * n; ++k)
    if (!(rgb[k] >= 0.0f) || !std::isfinite(rgb[k])) return PTC_ERR_INVALID;
  std::vector<float4> e((size_t)(n + 2u) * (n + 2u));
  env_rules::apron(rgb, n, e.data());
  for (uint32_t i = 0; i < count; ++i)
    env_rules::lookup(e.data(), n, dirs[3u * (size_t)i], dirs[3u * (size_t)i + 1u], dirs[3u * (size_t)i + 2u], rgb_out[3u * (size_t)i],
                      rgb_out[3u * (size_t)i + 1u], rgb_out[3u * (size_t)i + 2u]);
  return PTC_OK;
}

// the apron alone: E as ptc_set_environment uploads it, 4 (n + 2)^2 floats
int ptc_check_environment_apron(const float* rgb, uint32_t n, float* texels_out)
{
  if (!rgb || !texels_out || n < env_rules::kMinSize || n > env_rules::kMaxSize) return PTC_ERR_INVALID;
  env_rules::apron(rgb, n, reinterpret_cast<float4*>(texels_out));
  return PTC_OK;
}

// The environment's alias table (pt_env_light.hpp) on the host, as the first call that needs it builds it: no GPU, no
// context.  ptc_check_environment's refusals.
int ptc_check_environment_light_table(const float* rgb, uint32_t n, void* entries_out, double* total_weight, uint64_t* positive_squares)
{
  if (!rgb || !total_weight || !positive_squares || n < env_rules::kMinSize || n > env_rules::kMaxSize) return PTC_ERR_INVALID;
  for (size_t k = 0; k < 3u * (size_t)n * n; ++k)
    if (!(rgb[k] >= 0.0f) || !std::isfinite(rgb[k])) return PTC_ERR_INVALID;
  std::vector<float4> e((size_t)(n + 2u) * (n + 2u));
  env_rules::apron(rgb, n, e.data());
  std::vector<env_light::Entry> entries;
  *total_weight = env_light::build_table(e.data(), n, entries, positive_squares);
  if (entries_out) {
    if (entries.empty()) std::memset(entries_out, 0, (size_t)n * n * sizeof(env_light::Entry));
    else std::memcpy(entries_out, entries.data(), entries.size() * sizeof(env_light::Entry));
  }
  return PTC_OK;
}

// The shading normal of a triangle hit (pt_smooth.hpp) on the host: the header the megakernel's smooth instances run
int ptc_check_shading_normal(const float* n0, const float* n1, const float* n2, const float* u, const float* v, const float* g, const float* d,
                             const float* m16, uint32_t count, float* ns_out, uint8_t* fallback_out)
{
  if (!m16 || (count != 0u && (!n0 || !n1 || !n2 || !u || !v || !g || !d || !ns_out))) return PTC_ERR_INVALID;
  m4 inv;
  ptc_object o{};
  const float box[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (int rc = make_object(1u, 0u, m16, nullptr, box, &o)) return rc;  // the inverse a scene's object carries
  std::memcpy(&inv, o.inv_m, sizeof inv);
  auto at = [](const float* p, uint32_t i) { return mk3(p[3u * (size_t)i], p[3u * (size_t)i + 1u], p[3u * (size_t)i + 2u]); };
  for (uint32_t i = 0; i < count; ++i) {
    f3 ns;
    const bool formed = smooth::shading_normal(at(n0, i), at(n1, i), at(n2, i), u[i], v[i], at(g, i), at(d, i), inv, ns);
    ns_out[3u * (size_t)i] = ns.x;
    ns_out[3u * (size_t)i + 1u] = ns.y;
    ns_out[3u * (size_t)i + 2u] = ns.z;
    if (fallback_out) fallback_out[i] = formed ? (uint8_t)0 : (uint8_t)1;
  }
  return PTC_OK;
}

// The texture lookup (pt_texture.hpp) on the host: the header the textured kernels run on the device, on the
// caller's own texels (a byte quadruple is the word the pool holds, r in the low byte)
int ptc_check_texture_lookup(const ptc_texture_desc* desc, const float* st, uint32_t n, float* rgb_out, uint8_t* rejected_out)
{
  if (!desc || (n != 0u && (!st || !rgb_out))) return fail(nullptr, PTC_ERR_INVALID, "texture lookup: an array is NULL");
  const std::string why = texture_refusal(*desc);
  if (!why.empty()) return fail(nullptr, PTC_ERR_INVALID, "the texture " + why);
  const size_t count = (size_t)desc->width * desc->height;
  std::vector<uint32_t> words(count);
  for (size_t i = 0; i < count; ++i)
    words[i] = (uint32_t)desc->rgba8[4u * i] | ((uint32_t)desc->rgba8[4u * i + 1u] << 8) | ((uint32_t)desc->rgba8[4u * i + 2u] << 16) |
               ((uint32_t)desc->rgba8[4u * i + 3u] << 24);
  float table[2u * texmap::kTableEntries];
  texmap::decode_table(texmap::kLinear, table);
  texmap::decode_table(texmap::kSrgb, table + texmap::kTableEntries);
  const texmap::Record rec{0u, desc->width, desc->height, texmap::pack_flags(desc->encoding, desc->filter, desc->wrap)};
  for (uint32_t i = 0; i < n; ++i) {
    f3 c;
    const bool ok = texmap::lookup(words.data(), rec, table, st[2u * (size_t)i], st[2u * (size_t)i + 1u], c);
    rgb_out[3u * (size_t)i] = c.x;
    rgb_out[3u * (size_t)i + 1u] = c.y;
    rgb_out[3u * (size_t)i + 2u] = c.z;
    if (rejected_out) rejected_out[i] = ok ? (uint8_t)0 : (uint8_t)1;
  }
  return PTC_OK;
}

// The denoiser's albedo rule (pt_demodulate.hpp) on the host, a channel at a time: the header k_denoise_albedo and
// k_remodulate run on the device
int ptc_check_demodulate(const float* colour, const float* albedo, uint32_t n, float* irradiance_out, float* effective_out)
{
  if (n != 0u && (!colour || !albedo || !irradiance_out || !effective_out)) return fail(nullptr, PTC_ERR_INVALID, "demodulate: an array is NULL");
  for (uint32_t i = 0; i < n; ++i) {
    const float e = demod::effective_albedo(albedo[i]);
    effective_out[i] = e;
    irradiance_out[i] = demod::demodulate(colour[i], e);
  }
  return PTC_OK;
}

// The whole "denoise_variance" mode on the host from the caller's planes: tap positions as k_denoise_positions and
// the off-by-one taps make them, the estimate, then the guided passes with their ping-pong -- every per-tap number from
// pt_denoise_variance.hpp, the header the kernels compile.  colour, normal: 3 floats a pixel; depth: one; variance_out (may be NULL):
// the estimate, one float a pixel; result_out (may be NULL): 3 floats a pixel, untouched when filter_size < 1 (no pass, no result).
int ptc_check_denoise_variance(const float* colour, const float* normal, const float* depth, const ptc_camera* camera, uint32_t width,
                               uint32_t height, const ptc_denoiser_params* weights, float sigma, float* variance_out, float* result_out)
{
  if (!colour || !normal || !depth || !camera || !weights) return fail(nullptr, PTC_ERR_INVALID, "denoise_variance: an array is NULL");
  if (width < 2u || height < 2u || (uint64_t)width * height > 0x7fffffffull) return fail(nullptr, PTC_ERR_INVALID, "denoise_variance: bad size");
  if (!std::isfinite(sigma) || !(sigma > 0.0f)) return fail(nullptr, PTC_ERR_INVALID, "denoise_variance: sigma must be finite and > 0");
  const int W = (int)width, H = (int)height;
  const uint32_t P = width * height;
  const DCamera cam = make_camera(*camera, width, height);
  auto view_point = [&](int u, int v, float d) {  // generate_ray (pt_kernels_common.inc) at the pixel centre, the same operations
    const float fu = ((float)u + 0.5f) / (float)(cam.width - 1u);
    const float fv = ((float)cam.height - ((float)v + 0.5f)) / (float)(cam.height - 1u);
    const f3 dir = normalize(xform_vector(cam.cam, mk3(cam.llx + cam.vw * fu, cam.lly + cam.vh * fv, -1.0f)));
    return cam.origin + dir * d;
  };
  auto at3 = [](const std::vector<float>& a, uint32_t i) { return mk3(a[3u * i], a[3u * i + 1u], a[3u * i + 2u]); };
  const std::vector<float> nrm(normal, normal + 3u * (size_t)P);
  std::vector<float> pos(3u * (size_t)P);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const uint32_t i = (uint32_t)x + (uint32_t)y * width;
      const f3 p = view_point(x, y, depth[i]);
      pos[3u * i] = p.x, pos[3u * i + 1u] = p.y, pos[3u * i + 2u] = p.z;
    }
  std::vector<float> c(colour, colour + 3u * (size_t)P), c2(3u * (size_t)P), var(P), var2(P);
  // ---- the estimate
  {
    const float kn = dvar::term_scale(weights->normal_weight), kp = dvar::term_scale(weights->position_weight);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const uint32_t i = (uint32_t)x + (uint32_t)y * width;
        const f3 cp = at3(c, i), np = at3(nrm, i), xp = at3(pos, i);
        dvar::MeanSum ms{mk3(0.f, 0.f, 0.f), 0.0f};
        auto window = [&](auto&& tap) {
          for (int dy = -dvar::kVarRadius; dy <= dvar::kVarRadius; ++dy)
            for (int dx = -dvar::kVarRadius; dx <= dvar::kVarRadius; ++dx) {
              const uint32_t q = (uint32_t)std::clamp(x + dx, 0, W - 1) + (uint32_t)std::clamp(y + dy, 0, H - 1) * width;
              tap(dvar::estimate_weight(np, at3(nrm, q), xp, at3(pos, q), kn, kp), at3(c, q));
            }
        };
        window([&](float g, f3 cq) { dvar::mean_tap(ms, g, cp, cq); });
        const f3 m = dvar::mean_of(ms, cp);
        float acc = 0.0f;
        window([&](float g, f3 cq) { dvar::variance_tap(acc, g, cq, m); });
        var[i] = dvar::variance_of(acc, ms.g);
      }
  }
  if (variance_out) std::copy(var.begin(), var.end(), variance_out);
  // ---- the passes: (colour, variance) ping-pong; the last pass's output is the result
  const float kp = dvar::term_scale(weights->position_weight);
  int passes = 0;
  for (int64_t step = 1; step <= (int64_t)weights->filter_size; step *= 2, ++passes) {
    const float kn = dvar::term_scale((float)(step * step) * weights->normal_weight);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const uint32_t i = (uint32_t)x + (uint32_t)y * width;
        float v9[9];
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx)
            v9[3 * (dy + 1) + dx + 1] = var[(uint32_t)std::clamp(x + dx, 0, W - 1) + (uint32_t)std::clamp(y + dy, 0, H - 1) * width];
        const float kc = dvar::colour_scale(sigma, dvar::prefilter(v9));
        const f3 cp = at3(c, i), np = at3(nrm, i), xp = at3(pos, i);
        dvar::PassSum ps{mk3(0.f, 0.f, 0.f), 0.0f, 0.0f};
        for (int dy = -2; dy <= 2; ++dy)
          for (int dx = -2; dx <= 2; ++dx) {
            // the passes' tap-coordinate contract (k_denoise_lds): inclusive clamp, the last element past the end, own view ray
            const int u = (int)std::clamp<int64_t>(x + dx * step, 0, W), v = (int)std::clamp<int64_t>(y + dy * step, 0, H);
            const uint32_t ti = std::min((uint32_t)u + (uint32_t)v * width, P - 1u);
            const f3 xq = (u == W || v == H) ? view_point(u, v, depth[ti]) : at3(pos, ti);
            const f3 diff = cp - at3(c, ti);
            const float dc = dvar::dist2(cp, at3(c, ti));
            const float w = dvar::pass_weight(dc, dvar::dist2(np, at3(nrm, ti)), dvar::dist2(xp, xq), kc, kn, kp);
            dvar::pass_tap(ps, w * dvar::kernel_weight(dx, dy), diff, var[ti]);
          }
        f3 co;
        float vo;
        dvar::pass_result(ps, cp, co, vo);
        c2[3u * i] = co.x, c2[3u * i + 1u] = co.y, c2[3u * i + 2u] = co.z;
        var2[i] = vo;
      }
    c.swap(c2);
    var.swap(var2);
  }
  if (result_out && passes > 0) std::copy(c.begin(), c.end(), result_out);
  return PTC_OK;
}

// The normal map's rule (pt_normal_map.hpp) on the host: steps 1 .. 8 on the caller's own texels
int ptc_check_normal_map(const ptc_texture_desc* desc, const float* p0, const float* p1, const float* p2, const float* st0, const float* st1,
                         const float* st2, const float* u, const float* v, const float* m16, const float* b, const float* g, const float* d,
                         uint32_t count, float* normal_out, uint8_t* outcome_out)
{
  if (!desc || !m16 || (count != 0u && (!p0 || !p1 || !p2 || !st0 || !st1 || !st2 || !u || !v || !b || !g || !d || !normal_out || !outcome_out)))
    return fail(nullptr, PTC_ERR_INVALID, "normal map: an array is NULL");
  const std::string why = texture_refusal(*desc);
  if (!why.empty()) return fail(nullptr, PTC_ERR_INVALID, "the texture " + why);
  const size_t texels = (size_t)desc->width * desc->height;
  std::vector<uint32_t> words(texels);
  for (size_t i = 0; i < texels; ++i)
    words[i] = (uint32_t)desc->rgba8[4u * i] | ((uint32_t)desc->rgba8[4u * i + 1u] << 8) | ((uint32_t)desc->rgba8[4u * i + 2u] << 16) |
               ((uint32_t)desc->rgba8[4u * i + 3u] << 24);
  float table[texmap::kTableEntries];
  nmap::decode_table(table);
  const texmap::Record rec{0u, desc->width, desc->height, texmap::pack_flags(desc->encoding, desc->filter, desc->wrap)};
  m4 m;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) m.c[c][r] = m16[4 * c + r];
  auto at3 = [](const float* a, uint32_t i) { return mk3(a[3u * (size_t)i], a[3u * (size_t)i + 1u], a[3u * (size_t)i + 2u]); };
  for (uint32_t i = 0; i < count; ++i) {
    f3 n;
    const uint32_t how = nmap::shade(words.data(), rec, table, at3(p0, i), at3(p1, i), at3(p2, i), st0 + 2u * (size_t)i, st1 + 2u * (size_t)i,
                                     st2 + 2u * (size_t)i, u[i], v[i], m, at3(b, i), at3(g, i), at3(d, i), n);
    normal_out[3u * (size_t)i] = n.x;
    normal_out[3u * (size_t)i + 1u] = n.y;
    normal_out[3u * (size_t)i + 2u] = n.z;
    outcome_out[i] = (uint8_t)how;
  }
  return PTC_OK;
}

// ... and the sample (env_light::sample_draws) on the caller's points, normals and draws, written out as ptc_environment_light writes
// a sample whose shadow ray is free
int ptc_check_environment_light(const float* rgb, uint32_t n, const float* points, const float* normals, const uint32_t* v, const float* u,
                                uint32_t count, float* radiance, float* shadow_rays, uint8_t* sampled)
{
  if (!rgb || n < env_rules::kMinSize || n > env_rules::kMaxSize) return PTC_ERR_INVALID;
  if (count != 0u && (!points || !normals || !v || !u || !radiance)) return PTC_ERR_INVALID;
  for (uint32_t i = 0; i < count; ++i)
    if (v[i] < 1u || v[i] > 0x7ffffffeu) return PTC_ERR_INVALID;  // a raw value of the generator
  for (size_t k = 0; k < 3u * (size_t)n * n; ++k)
    if (!(rgb[k] >= 0.0f) || !std::isfinite(rgb[k])) return PTC_ERR_INVALID;
  std::vector<float4> e((size_t)(n + 2u) * (n + 2u));
  env_rules::apron(rgb, n, e.data());
  std::vector<env_light::Entry> entries;
  const bool table = env_light::build_table(e.data(), n, entries, nullptr) > 0.0;
  for (uint32_t i = 0; i < count; ++i) {
    env_light::Sample s{};
    if (table)
      s = env_light::sample_draws(reinterpret_cast<const uint4*>(entries.data()), e.data(), n,
                                  mk3(normals[3u * (size_t)i], normals[3u * (size_t)i + 1u], normals[3u * (size_t)i + 2u]), v[i], u[3u * (size_t)i],
                                  u[3u * (size_t)i + 1u], u[3u * (size_t)i + 2u]);
    radiance[3u * (size_t)i] = s.contrib.x;
    radiance[3u * (size_t)i + 1u] = s.contrib.y;
    radiance[3u * (size_t)i + 2u] = s.contrib.z;
    if (sampled) sampled[i] = s.sampled ? (uint8_t)1 : (uint8_t)0;
    if (shadow_rays) {
      float* r = shadow_rays + 8u * (size_t)i;
      std::memcpy(r, points + 3u * (size_t)i, 3u * sizeof(float));
      r[3] = 1e-4f;
      r[4] = s.sampled ? s.w.x : 0.0f;
      r[5] = s.sampled ? s.w.y : 0.0f;
      r[6] = s.sampled ? s.w.z : 0.0f;
      r[7] = s.sampled ? s.tmax : 0.0f;
    }
  }
  return PTC_OK;
}

// ... and the sample's density (env_light::density) in `count` caller-given unit directions, as
// ptc_environment_light_pdf returns it; a map of weight 0: zeros
int ptc_check_environment_light_pdf(const float* rgb, uint32_t n, const float* dirs, uint32_t count, float* pdf_out)
{
  if (!rgb || n < env_rules::kMinSize || n > env_rules::kMaxSize) return PTC_ERR_INVALID;
  if (count != 0u && (!dirs || !pdf_out)) return PTC_ERR_INVALID;
  for (size_t k = 0; k < 3u * (size_t)n * n; ++k)
    if (!(rgb[k] >= 0.0f) || !std::isfinite(rgb[k])) return PTC_ERR_INVALID;
  std::vector<float4> e((size_t)(n + 2u) * (n + 2u));
  env_rules::apron(rgb, n, e.data());
  std::vector<env_light::Entry> entries;
  const bool table = env_light::build_table(e.data(), n, entries, nullptr) > 0.0;
  for (uint32_t i = 0; i < count; ++i)
    pdf_out[i] = table ? env_light::density(reinterpret_cast<const uint4*>(entries.data()), n,
                                            mk3(dirs[3u * (size_t)i], dirs[3u * (size_t)i + 1u], dirs[3u * (size_t)i + 2u]))
                       : 0.0f;
  return PTC_OK;
}

// The light sample of section 5f (pt_light_sample.hpp: the header k_light_sample and the megakernel's lit instances run) on the host, against
// the lamp table of `scene` and the caller's draws: no GPU, no context.  Written out as ptc_direct_light writes a sample whose shadow
// ray is free; a scene without lamps or of total weight 0: zeros.
int ptc_check_light_sample(const ptc_scene_desc* scene, const float* points, const float* normals, const uint32_t* v, const float* u,
                           uint32_t count, uint32_t* lamp, float* shadow_rays, float* contribution, uint8_t* sampled)
{
  if (!scene) return fail(nullptr, PTC_ERR_INVALID, "scene is NULL");
  if (count != 0u && (!points || !normals || !v || !u)) return fail(nullptr, PTC_ERR_INVALID, "points, normals or draws are NULL");
  for (uint32_t i = 0; i < count; ++i)
    if (v[i] < 1u || v[i] > 0x7ffffffeu) return fail(nullptr, PTC_ERR_INVALID, "a raw draw is 1 .. 2^31 - 2");
  std::vector<ptc_light> lights;
  std::vector<uint32_t> thresholds;
  ptc_light_info li{};
  uint32_t last = 0u;
  if (int rc = checked_light_table(scene, lights, &li, &last, &thresholds)) return rc;
  static_assert(sizeof(ptc_light) == 4 * sizeof(float4), "a lamp record is four float4");
  const DLights lt{reinterpret_cast<const float4*>(lights.data()), thresholds.data(), li.lights, last,
                   reinterpret_cast<const DObject*>(scene->objects), reinterpret_cast<const float4*>(scene->spheres),
                   reinterpret_cast<const DMaterial*>(scene->materials)};
  for (uint32_t i = 0; i < count; ++i) {
    LightSample s{};
    uint32_t k = 0u;
    if (!thresholds.empty()) {
      LightTerms terms;
      k = light_pick(lt, v[i]);
      s = light_sample_draws(lt, mk3(points[3u * (size_t)i], points[3u * (size_t)i + 1u], points[3u * (size_t)i + 2u]),
                             mk3(normals[3u * (size_t)i], normals[3u * (size_t)i + 1u], normals[3u * (size_t)i + 2u]), v[i], u[2u * (size_t)i],
                             u[2u * (size_t)i + 1u], terms);
    }
    if (lamp) lamp[i] = k;
    if (sampled) sampled[i] = s.sampled ? (uint8_t)1 : (uint8_t)0;
    if (contribution) {
      contribution[3u * (size_t)i] = s.contrib.x;
      contribution[3u * (size_t)i + 1u] = s.contrib.y;
      contribution[3u * (size_t)i + 2u] = s.contrib.z;
    }
    if (shadow_rays) {
      float* r = shadow_rays + 8u * (size_t)i;
      std::memcpy(r, points + 3u * (size_t)i, 3u * sizeof(float));
      r[3] = 1e-4f;
      r[4] = s.sampled ? s.w.x : 0.0f;
      r[5] = s.sampled ? s.w.y : 0.0f;
      r[6] = s.sampled ? s.w.z : 0.0f;
      r[7] = s.sampled ? s.tmax : 0.0f;
    }
  }
  return PTC_OK;
}

// ... and on the device
int ptc_selftest_rng(ptc_ctx* ctx, const uint32_t* seeds, const uint32_t* discards, uint32_t n, uint32_t* out)
{
  if (!ctx || !seeds || !discards || !out) return PTC_ERR_INVALID;
  if (n == 0) return PTC_OK;
  if (int rc = bind_device(ctx)) return rc;
  std::vector<void*> pool;
  uint32_t *d_seeds = nullptr, *d_discards = nullptr, *d_out = nullptr;
  int rc = dev_alloc(ctx, pool, &d_seeds, n);
  if (!rc) rc = dev_alloc(ctx, pool, &d_discards, n);
  if (!rc) rc = dev_alloc(ctx, pool, &d_out, (size_t)n * 6u);
  if (rc) {
    free_pool(pool);
    return rc;
  }
  hipError_t e = hipMemcpyAsync(d_seeds, seeds, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_discards, discards, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_selftest_rng(ctx->stream, d_seeds, d_discards, n, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * 6u * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  free_pool(pool);
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("selftest_rng: ") + hipGetErrorString(e));
  return PTC_OK;
}

/* diagnostic (tools/debug): the persistent launch's state block of slot `slot`, after a synchronisation */
int ptc_debug_persist(ptc_ctx* ctx, int slot, void* dst, uint64_t bytes)
{
  if (!ctx || !dst || slot < 0 || slot >= (int)ctx->slots.size() || !ctx->slots[(size_t)slot].persist) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(dst, ctx->slots[(size_t)slot].persist, std::min<uint64_t>(bytes, sizeof(DPersist)), hipMemcpyDeviceToHost));
  return PTC_OK;
}

}  // extern "C"


extern "C" {
// The primary rays of `iteration` for every slot of the context, in slot order, under the context's lens: the
// device function the frame's ray generation runs, and nothing else.  Moves neither ptc_stats nor the iteration counter.
int ptc_generate_rays(ptc_ctx* ctx, const ptc_camera* camera, uint32_t iteration, float* rays_out, uint64_t capacity_floats)
{
  if (!ctx || !camera || !rays_out) return PTC_ERR_INVALID;
  if (!ctx->pix_capacity || !ctx->pix_count) return fail(ctx, PTC_ERR_INVALID, "ptc_resize first");
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  const size_t floats = (size_t)ctx->pix_count * 8u;
  if (capacity_floats < floats) return fail(ctx, PTC_ERR_INVALID, "rays_out too small: " + std::to_string(floats) + " floats needed");
  float4* dev = nullptr;
  HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&dev), floats * sizeof(float)));
  launch_generate_rays(ctx->stream, make_camera(*camera, ctx->width, ctx->height), iteration, ctx->band, ctx->pix_count,
                       ctx->lens.radius > 0.0f ? ctx->lens : DLens{0.0f, 0.0f}, dev);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(rays_out, dev, floats * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("generate rays: ") + hipGetErrorString(e));
  return PTC_OK;
}
}  // extern "C"
