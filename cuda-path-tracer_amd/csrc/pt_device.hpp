// pt_device.hpp -- device-visible types of the render core and the launch interface between the
// C ABI (ptcore.cpp) and the HIP kernels (pt_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/ptcore.h"
#include "pt_math.hpp"
#include "pt_env.hpp"
#include "pt_smooth.hpp"
#include "pt_texture.hpp"
#include "pt_normal_map.hpp"

namespace pt {

constexpr int kWave = 64;            // gfx950 wavefront
constexpr int kChunk = 64;           // paths per compaction chunk = one wavefront
constexpr int kStackDepth = 64;      // traversal stack entries per ray (LDS, [depth][lane])
constexpr int kMaxBounces = 64;      // == PTC_MAX_BOUNCES_CAP
// Ray-fetch cursor sets of the persistent traversal launches.  k_raygen zeroes them at the start of a frame and the
// last wavefront of every traversal launch zeroes the set it used (launch_epilogue), so launch n of a slot's stream
// takes set n % kWorkSlots whatever the number of launches per frame (objects x bounces is unbounded).
constexpr int kWorkSlots = 4;
// Traversal stack entries per lane the four-wide walk keeps in LDS (6 KiB per wavefront at 24); deeper entries go to
// DScene::spill.  ONE constant for the kernels' LDS arrays and the host's DScene::lds_cap / spill sizing: a build with
// -DPT_T4_LDS=16 against a host that assumed 24 wrote past its stack (round-2 A/B fault).
#ifndef PT_T4_LDS
#define PT_T4_LDS 24
#endif
constexpr int kLds4 = PT_T4_LDS;
static_assert(kLds4 >= 4 && kLds4 <= kStackDepth, "PT_T4_LDS out of range");

// error bits in DeviceCounters::flags
constexpr uint32_t kFlagStackOverflow = 1u;
constexpr uint32_t kFlagDispatchOrder = 2u;  // k_shade_fused gave up waiting for a predecessor tile (bounded look-back wait)
constexpr uint32_t kFlagPersistStall = 4u;   // k_persist: a wavefront waited for work (or for the redo lock) beyond the bound and gave up

// Same 160-byte layout as ptc_object / the reference's GPUObject (scene.hpp:16-22)
struct DObject {
  uint32_t type;
  uint32_t index;
  m4 m;
  m4 inv_m;
  float bmin[3];
  float bmax[3];
};
static_assert(sizeof(DObject) == 160, "object layout");

// The reference meets a mesh's triangles in WORLD space, at vertices fl(M v), while the walks cull with the OBJECT-space
// boxes along the ray fl(M^-1 o) + t M^-1 d.  Against exact arithmetic a vertex is off by at most 4u (|M| |v| + |t_M|)
// per component and the object-space origin by 4u (|M^-1| |o| + |t_M^-1|) (u = 2^-24, no contraction); mapped into object
// space, a hit the reference finds lies within the returned distance (twice that bound) of its leaf's box, per axis.
// The walks grow the boxes they may skip by it.  Near the origin it is a few 1e-6; a mesh 1e5 from the origin needs
// about 0.02, more than the walks' relative margins (found by a displaced sphere at (1e5, 0, 0): the walk culled the
// reference's winner, tests/test_gpu_mesh_limits.py).  extent = largest |object-space coordinate| of the mesh.
__device__ __forceinline__ float world_rounding_pad(const DObject* obj, const f3 ro, const float extent)
{
  float rm = 0.0f, ri = 0.0f, tm = 0.0f, ti = 0.0f;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    rm = fmaxf(rm, fabsf(obj->m.c[0][r]) + fabsf(obj->m.c[1][r]) + fabsf(obj->m.c[2][r]));
    ri = fmaxf(ri, fabsf(obj->inv_m.c[0][r]) + fabsf(obj->inv_m.c[1][r]) + fabsf(obj->inv_m.c[2][r]));
    tm = fmaxf(tm, fabsf(obj->m.c[3][r]));
    ti = fmaxf(ti, fabsf(obj->inv_m.c[3][r]));
  }
  const float o = fmaxf(fmaxf(fabsf(ro.x), fabsf(ro.y)), fabsf(ro.z));
  return 4.7683716e-7f * (ri * (rm * extent + tm + o) + ti);  // 8u
}

struct DMaterial {
  int32_t type;
  float p[4];
};
static_assert(sizeof(DMaterial) == 20, "material layout");

// Read-only scene in HBM.
//   bvh: two float4 per node: {min.xyz, bits(first_child_or_primitive)}, {max.xyz, bits(primitive_count)}
//   wide: the same tree re-laid for the fast traversal (k_trace_wide): one 64-byte record per INNER node
//         holding both children's boxes,
//           w0 = {lmin.xyz, lmax.x}  w1 = {lmax.yz, rmin.xy}  w2 = {rmin.z, rmax.xyz}  w3 = {bits lref, bits rref, -, -}
//         ref = index of the child's record, or kLeafBit | rank of the child's triangle in depth-first
//         (left-first) leaf order -- the order in which the reference's traversal reaches the leaves.
//   tris: per MESH OBJECT (instance), world-space triangles in that depth-first order, kTriVec4 (= 4) float4 each,
//         three of them used:
//           {p0.xyz, e1.x} {e1.yz, e2.xy} {e2.z, n.xyz}   with p = transform_point(M, position),
//           e1 = p1 - p0, e2 = p2 - p0, n = normalize(cross(e1, e2))   (exactly what the reference
//           recomputes per test, path_tracer.cu:57-59, intersections.cuh:45-46,54-55)
//   bvh4q: the same tree collapsed to four children per node for the persistent traversal, 64 bytes per node
//         (half a cache line, four 16-byte loads): dwords 0-2 origin xyz (f32); dword 3 and dwords 10, 11 = the three
//         power-of-two grid steps x, y, z as floats; dwords 4-9 = child planes as 8-bit grid
//         coordinates, component-major (lo_x[4] lo_y[4] lo_z[4] hi_x[4] hi_y[4] hi_z[4], child c in byte c), rounded
//         outwards: a quantised child box contains the exact one, which is all a conservative walk needs;
//         dwords 12-15 = refs[4].  ref = node index or kLeafBit | depth-first triangle rank; an unused slot has an
//         inside-out box (lower planes 255, upper planes 0) and refers to the dummy triangle (DScene::dummy_ref).
//         Nodes in depth-first preorder.
//   leaf_parent: per triangle (depth-first rank) the box of the leaf's parent in the REFERENCE tree, 2 float4.
//         Why it suffices for exactness: boxes nest exactly (parent = componentwise min/max of children) and
//         IEEE subtraction/division are monotonic, so whenever a node passes the reference's box test all its
//         ancestors pass too; a triangle is reachable in the reference iff its parent's box passes.
// float4s per triangle record of DScene::tris: the 48 bytes described above padded to 64, so that a record never
// straddles two 64-byte segments of a cache line (measured +2 % rays/s against 48-byte records; 3 = unpadded)
#ifndef PT_TRI_VEC4
#define PT_TRI_VEC4 4
#endif
constexpr uint32_t kTriVec4 = PT_TRI_VEC4;
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t kNoChild = 0xffffffffu;

// The acceleration data of ONE mesh (reference tree + the traversal layouts derived from it).  DScene::cur is the
// mesh of the object a traversal launch walks (the host sets it per launch); kernels that loop over all objects of
// the scene look the mesh up per object (DScene::mesh_views[DScene::object_mesh[i]]).
struct DMeshView {
  const float* positions;
  const uint32_t* indices;
  const float4* bvh;
  const float4* wide;              // 4 float4 per inner node
  const float4* leaf_parent;       // 2 float4 per triangle
  const uint4* bvh4q;              // the four-wide nodes in 64 bytes (Wide4Accel::nodes_q), 4 x uint4 per node
  uint32_t bvh4_root;
  uint32_t dummy_ref;              // reference in the unused child slots of a four-wide node (an inside-out box, a triangle no ray hits)
  float root_min[3];               // box of the root (tested before descending, like any inner node)
  float root_max[3];
  uint32_t root_ref;               // record 0, or kLeafBit for a single-triangle mesh
  uint32_t bvh_node_count;
};

// Which pixels of the frame this context renders.  Contiguous (nranks == 1): pixel = pix_begin + s.
// Interleaved (multi-GPU, load-balanced): the frame is cut into blocks of `block_rows` rows dealt round-robin to
// `nranks` contexts; local row lr is row ((lr / block_rows) * nranks + rank) * block_rows + lr % block_rows.
struct DBand {
  uint32_t pix_begin, width, rank, nranks, block_rows;
};
PT_HD uint32_t band_pixel(const DBand& b, uint32_t s)
{
  if (b.nranks <= 1u) return b.pix_begin + s;
  const uint32_t lr = s / b.width, x = s - lr * b.width;
  const uint32_t y = ((lr / b.block_rows) * b.nranks + b.rank) * b.block_rows + lr % b.block_rows;
  return y * b.width + x;
}
PT_HD uint32_t band_local(const DBand& b, uint32_t pixel)
{
  if (b.nranks <= 1u) return pixel - b.pix_begin;
  const uint32_t y = pixel / b.width, x = pixel - y * b.width;
  const uint32_t lr = ((y / b.block_rows) / b.nranks) * b.block_rows + y % b.block_rows;
  return lr * b.width + x;
}

// Entry points for primary rays ("beam", round 4): per distinct camera of a batch and per tile of kBeamTile x kBeamTile
// pixels, the (at most four) deepest nodes of the launch's four-wide tree that the tile's frustum overlaps, each with its
// box in the object's space: 2 float4 per entry {box min, reference bits} {box max, 0}, 4 entries per tile (unused:
// an inside-out box).  A primary ray tests the four boxes of its tile like the children of one node and starts its walk
// there instead of at the root (k_beam writes them, k_traverse4<.., kBeam> reads them).
constexpr uint32_t kBeamTile = 8u;
constexpr uint32_t kBeamEntries = 4u;
struct DBeam {
  const float4* entries;        // null: off
  uint32_t tiles_x, tiles;      // tiles per row, tiles per camera
  uint32_t width;               // of the frame, pixels
  DBand band;                   // which pixel a slot of bounce 0 holds (band_pixel)
  uint8_t beam_of[32];          // frame of the batch -> camera of the batch (frames with the same camera share one)
};
constexpr uint32_t kSphereTab = 8u;  // float4 per object in DScene::sphere_ball
struct DScene {
  const DObject* objects;
  const uint32_t* object_material;
  const float4* spheres;  // center.xyz, radius
  const DMaterial* materials;
  DMeshView cur;                   // the mesh of this launch's object (mesh 0 unless the host says otherwise)
  const DMeshView* mesh_views;     // all meshes of the scene ...
  const uint32_t* object_mesh;     // ... and which one each object instantiates (0 for spheres)
  const float4* tris;              // kTriVec4 float4 per instance triangle
  const uint32_t* object_tri_base; // per object: first triangle of its instance in `tris` (meshes only)
  uint32_t* slow_stack;            // global traversal stack of the launch's exact redo (redo_slow_rays), [kStackDepth][kWave]
  uint2* spill;                    // traversal stack entries beyond the LDS part, [entry][persistent thread]
  uint32_t spill_stride;           // number of persistent threads
  uint32_t spill_cap;              // entries per thread in `spill`
  uint32_t lds_cap;                // entries per lane kept in LDS before `spill` (kLds4; fewer only in tests)
  uint32_t force_slow;             // test hook: hand EVERY ray to the exact redo (redo_slow_rays)
  uint32_t static_eighths;         // persistent traversal: share (x/8) of each image region dealt without atomics
  uint32_t refill_lanes;           // persistent traversal: fetch new rays once this many lanes of a wavefront are idle
  uint32_t split_idle;             // ... and once the launch has no rays left: split busy lanes' stacks among idle ones when
                                   // at least this many lanes are idle (0: never)
  uint32_t object_count;
  // per object kSphereTab float4, for spheres: [0] the world-space ball that contains the transformed sphere {centre.xyz,
  // radius (rounded up)} -- radius < 0: no ball (a projective matrix; a mesh object): never skipped; [1] {1 / largest
  // stretch of the object's matrix (rounded down), 1 if "simple" (both matrices pure translations spelled 1.0f / +0.0f),
  // radius of the INNER ball of a simple object (inside what the reference's float sequence can hit; sphere_ball_of), 0};
  // [2..6] what a lane needs of a simple object: {box min, inverse translation x}, {box max, .. y},
  // {sphere centre, .. z}, {translation, sphere radius}, {material bits, 0, 0, 0} (sphere_run_lanes).
  const float4* sphere_ball;
  uint32_t lanes_run;              // set per launch by the host: the launch's sphere run may take sphere_run_lanes
  uint32_t fold_run;               // ... every object of the launch's sphere run is a "simple" sphere: k_spheres may take sphere_fold
  DBeam beam;                      // set per launch by the host (bounce 0's first traversal launch, or off)
};

// Camera constants prepared on the host once per frame (GPUCamera, camera.hpp:10-15, plus the
// per-frame invariants of generate_ray, ray_gen.cu:37-47, hoisted out of the per-pixel code).
struct DCamera {
  m4 cam;            // translate(position) * mat4_cast(rotation)
  f3 origin;         // (cam * (0,0,0,1)).xyz
  float vw, vh;      // viewport width / height
  float llx, lly;    // lower-left corner x, y  ( = -(vw/2), -(vh/2) )
  uint32_t width, height;
};

// The thin lens (ptc_set_lens): aperture radius and focus distance in world units, context-wide.  radius 0 is the
// pinhole: the host launches the pinhole instances and nothing reads this.  Not part of DCamera: DCameras is kMaxBatch cameras by
// value and the kernel-argument block has no room for 32 copies of a frame-wide constant.
struct DLens {
  float radius, focus;
};

// The environment (ptc_set_environment): the context's octahedral HDR map with its apron, (n + 2) x (n + 2) texels
// {r, g, b, 0}, row-major (pt_env.hpp).  A kernel argument of the environment instances alone; texels null: no environment, the
// host launches the gradient's instances and nothing reads this.
struct DEnv {
  const float4* texels;
  uint32_t n, pad;
};

// Live-path state, 40 B/path in three arrays (round 5; 48 until then: a float4 of its own for the throughput, two words unused --
// the kernels that end a bounce are HBM-bound and read and write every word of it):
//   o4 = origin.xyz, bits(pixel | tmin_flag<<31)   tmin_flag: t_min is 1e-5 (after a dielectric) instead of 1e-4
//   d4 = direction.xyz, throughput.r               (the closest-hit kernels load o4 and d4 and ignore d4.w; k_raygen leaves it 0:
//   t2 = throughput.gb                              bounce 0 starts from throughput 1 without reading either)
struct DPaths {
  float4* o4;
  float4* d4;
  float2* t2;
};

// Closest-hit record written by the trace kernel (32 B/path):
//   tp = t (or -1 on miss), point.xyz ;  nm = normal.xyz, bits(material | side<<31)
// (point is stored because for spheres the reference keeps the TRANSFORMED object-space hit point,
//  path_tracer.cu:93, which is not origin + direction * t)
struct DHits {
  float4* tp;
  float4* nm;
};

// Accumulated framebuffers (running means): color4 = rgb,-  ;  nd4 = normal.xyz, depth
struct DFrame {
  float4* color4;
  float4* nd4;
};

struct DeviceCounters {
  uint32_t live[kMaxBounces + 1];  // live paths entering bounce b of the current frame
  uint32_t listed_now[kMaxBounces + 1];  // rays on the work list of bounce b's (last) listed traversal launch; with live[]: what the host sizes later launches by
  uint32_t flags;
  uint32_t slow_count;             // rays set aside for the exact redo by the running traversal launch
  uint32_t waves_done;             // wavefronts of the running traversal launch that have signed off
  uint32_t shade_ticket;           // k_shade_fused: next tile of this frame to be taken (zero between launches)
  uint32_t list_count;             // rays k_raygen / k_spheres<.., kFilter> have put on the next traversal launch's work list (written by the list's last tile)
  unsigned long long rays_total;
  unsigned long long paths[kMaxBounces];      // sum of live[b] over frames since the last profile reset
  unsigned long long box_tests[kMaxBounces];  // instrumented runs only
  unsigned long long tri_tests[kMaxBounces];
  uint32_t max_box_tests[kMaxBounces];        // longest single traversal (box tests of one ray), instrumented runs
  unsigned long long listed_rays[kMaxBounces];  // rays the traversal launches fetched through a work list (frame 0's block: whole batch)
  unsigned long long slow_rays[kMaxBounces];  // rays redone exactly (redo_slow_rays)
  unsigned long long node_visits[kMaxBounces];  // BVH node records fetched by the closest-hit kernels, instrumented runs
  // ray-fetch cursors of the persistent traversal launches, one per image region, each on its own 128-byte
  // line (cursors sharing a line serialise in L2: measured ~30 atomics/us for the whole line)
  uint32_t work[kWorkSlots][8][32];
};

// Several iterations ("frames") traced by the same launches: every per-frame array of a slot is one allocation
// with frame f at element offset f * stride (chunk arrays: f * chunk_stride; counters: f), and the kernels of
// one bounce cover all frames of the batch (blockIdx.y = frame; the persistent traversal kernel feeds its lanes
// from all of them).  One launch then carries count times the rays, so the latency tail of a bounce (a few
// long rays) is paid once per batch instead of once per frame.
constexpr int kMaxBatch = 32;
struct DBatchInfo {
  uint32_t stride, chunk_stride, count, pad;
  uint32_t iteration[kMaxBatch];
};
struct DCameras {
  DCamera c[kMaxBatch];
};

// "prefold" (round 5, review item 4): the kernel that ends bounce b has a survivor's NEXT ray in registers; when the next bounce
// opens with a sphere run in front of a mesh (a room's walls: config 2) it tests that run there and then -- the hit record of
// bounce b + 1 goes straight to the survivor's new slot (a second set of hit records: other tiles still read this bounce's),
// one byte says whether the ray may reach the mesh launch's boxes -- and bounce b + 1 starts with k_list_flags (the work list
// from those bytes) instead of k_spheres' pass over every ray.
struct DNextRun {
  uint32_t begin, end;            // the sphere run in front of the next bounce's first traversal launch (objects)
  uint32_t filt_begin, filt_end;  // the mesh objects of that launch (may_hit_boxes)
  uint32_t fold_run;              // the run may take sphere_fold (every object a translated sphere)
  uint32_t pad;
  DHits hits;                     // the NEXT bounce's hit records
  uint8_t* flags;                 // per new slot: 1 = the ray goes on the traversal launch's work list
};

// ---- the bounce-spanning persistent launch (k_persist, round 5) ------------------------------------
// One launch per batch carries the traversal of bounces >= 1 and the shade passes of ALL bounces: of every five wavefronts
// four walk rays (traverse4_walk<.., kPersist>) and one shades tiles (shade_tile<.., 1, true>).  Frame f moves through
//   S(0) -> T(1) -> S(1) -> T(2) -> ... -> S(max_bounces - 1) -> done          (R(b): the exact redo, between T(b) and S(b))
// on its own; what a frame is in is one 64-bit word (phase code << 32 | count: rays of a T phase, tiles of an S phase)
// that the wavefront finishing the phase's last piece of work rewrites, and everybody else polls.  All of it through
// agent-scope atomics; the payload (hit records, path state) is stored write-through and loaded past the L1 (sc1).
constexpr uint32_t kPersistSlotBits = 26u;  // a lane's ray: position in the batch (frame * stride + slot) | frame << 26
constexpr uint32_t kPersistSlotMask = (1u << kPersistSlotBits) - 1u;
constexpr uint32_t kPersistDyn = 128u;      // rays per cursor add (fixed: a cursor then only ever stands on multiples of it)
constexpr uint32_t kPhaseT = 0u, kPhaseRedo = 1u, kPhaseRedoing = 2u, kPhaseS = 3u, kPhaseDone = 0xffffffffu;  // code = bounce << 3 | kind
constexpr uint32_t kPhaseKindBits = 3u, kPhaseKindMask = 7u;
struct DPersistFrame {       // every hot word on a 128-byte line of its own
  uint32_t cursor[8][32];    // [region][0]: bounce << 26 | rays of the frame's current T phase handed out from that region
  uint32_t t_done[32];       // [0]: bounce << 26 | rays of the current T phase whose results are in memory
  uint32_t s_ticket[32];     // [0]: bounce << 26 | next tile of the current S phase
  uint32_t s_done[32];       // [0]: tiles of the current S phase finished
};
struct DPersist {
  unsigned long long state[kMaxBatch];  // two lines, read by everybody
  uint32_t started, frames_done, redo_lock, error;
  uint32_t pad[28];
  DPersistFrame f[kMaxBatch];
  uint32_t dbg[kMaxBatch][16][8];   // PT_PERSIST_DEBUG builds: per frame and bounce {n, rays fetched, rays finalized, tiles, tiles done, live out, .., ..}
};
struct DPersistArgs {
  DPersist* st;
  DPaths paths[2];           // bounce b reads paths[b & 1] and writes paths[(b & 1) ^ 1]
  int max_bounces;
  uint32_t service_every;    // one wavefront in this many (by arrival) is a service wavefront
  uint32_t help_tiles;       // tiles a walking wavefront shades when it finds no rays to hand out, before it looks for rays again
  uint32_t tail_begin, tail_end;  // the sphere run that ends the object list (k_shade_fused's obj_begin / obj_end)
  int staged;
  const uint32_t* slot_base;
  unsigned long long* tile_desc;
  uint32_t tile_stride, epoch0;   // bounce b's shade pass carries epoch0 + b
  DFrame stage;
  DBand band;
  const uint32_t* list0;     // bounce 0: the work list k_raygen left when it finished the other primaries itself, or null
  uint32_t* slow_list;       // per frame at f * stride (DeviceCounters::slow_count of that frame)
};

struct DDenoise {
  float c_phi, n_phi, p_phi;
  int variant;  // 0: taps staged in LDS per sub-lattice (k_denoise_lds, default); 1: taps through L1 / L2 (k_denoise)
};

// a guided pass of "denoise_variance" (DESIGN section 5s): no colour weight -- sigma x the prefiltered variance takes its place
struct DDenoiseVar {
  float n_phi, p_phi, sigma;
  int variant;  // as DDenoise's: 0 k_denoise_var_lds, 1 k_denoise_var
};

// The reference BVH built on the device (pt_bvh_gpu.hip): the same tree as build_bvh (pt_bvh.cpp), node for node.
// d_packed: 2 * (2T-1) float4 ({min, first}, {max, count}: DScene::bvh); d_nodes (may be null): the same nodes in the
// reference's 32-byte layout; level_base (may be null): first node of every depth, plus the node count at the end.
// Synchronises the stream (one readback per tree level).
int build_bvh_device(hipStream_t stream, const float* d_positions, const uint32_t* d_indices, uint32_t index_count,
                     float4* d_packed, ptc_bvh_node* d_nodes, uint32_t* node_count, uint32_t* max_depth,
                     std::vector<uint32_t>* level_base);

// The traversal layouts of pt_scene_host.cpp (WideAccel, Wide4Accel, the leaf order) built on the device from a
// reference tree whose nodes are stored depth by depth (level_base as above).  The arrays are hipMalloc'ed and belong
// to the caller.
struct DeviceLayouts {
  uint32_t* nodes_q = nullptr;     // DScene::bvh4q
  float4* leaf_parent = nullptr;   // DScene::leaf_parent (+ the dummy's entry)
  uint32_t* tri_order = nullptr;   // depth-first rank -> triangle of the mesh
  float4* wide = nullptr;          // DScene::wide
  uint32_t wide4_nodes = 0, wide4_depth = 0, triangles = 0, inner_nodes = 0;
  uint32_t root_ref4 = 0, root_ref2 = 0, dummy_ref = 0;
  float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0};
};
int build_layouts_device(hipStream_t stream, const float4* d_bvh, uint32_t count, const std::vector<uint32_t>& level_base,
                         DeviceLayouts* out);
// world-space triangle records of one instance in depth-first order (DScene::tris), kTriVec4 float4 per triangle
void launch_instance_triangles(hipStream_t stream, const m4& m, const float* d_positions, const uint32_t* d_indices,
                               const uint32_t* d_tri_order, uint32_t triangles, float4* d_out);

// ---- launch interface (implemented in pt_kernels.hip) ----
// filt_begin < filt_end and worklist != null: the bounce's first launch is a traversal launch over the mesh objects
// [filt_begin, filt_end); raygen lists the rays that may hit them (in slot order: a look-back scan on the descriptors
// tile_desc -- k_shade_fused's, tile_stride per frame -- under a launch epoch of its own) and writes the miss record of
// the others into `hits`.  finish_misses (that launch walks the scene's whole object list, so an unlisted ray hits
// nothing): the unlisted rays end in raygen -- sky into fb (the shade kernels' frame: staged, or the framebuffers) -- and
// bounce 0's launch_shade_fused gets list = worklist
void launch_raygen(hipStream_t s, const DCameras& cams, const DBatchInfo& bi, DBand band, uint32_t pix_count,
                   DPaths paths, DeviceCounters* counters, const DObject* objects = nullptr, uint32_t filt_begin = 0u,
                   uint32_t filt_end = 0u, uint32_t* worklist = nullptr, DHits hits = DHits{nullptr, nullptr},
                   unsigned long long* tile_desc = nullptr, uint32_t tile_stride = 0u, uint32_t epoch = 0u,
                   bool finish_misses = false, DFrame fb = DFrame{nullptr, nullptr}, bool staged = false, DLens lens = DLens{0.0f, 0.0f},
                   DEnv env = DEnv{nullptr, 0u, 0u});
// variant 0: reference-order traversal (k_trace); 1: culled near-first traversal over the wide layout (k_trace_wide)
void launch_trace(hipStream_t s, const DScene& scene, DPaths paths, DHits hits, uint32_t max_paths, int bounce,
                  DeviceCounters* counters, bool count_tests, int variant);
// variant 3 (default): per bounce, the object list is walked in the reference's order; the closest hit so far
// travels from launch to launch in the hit record:
//   launch_traverse   one mesh object: persistent wavefronts, each lane fetches the next ray when its own is done;
//                     rays it sets aside (degenerate direction, winner grazing its parent box) are redone exactly by
//                     the last wavefront of the same launch
//   launch_spheres    a run of spheres in FRONT of a mesh (objects [obj_begin, obj_end))
//   launch_tail_count the end of the stage: the run of spheres that ends the object list (may be empty, may be the
//                     whole list) and the live count of every 64-slot chunk from the hit records; also after launch_trace
//   launch_scan       exclusive scan of those counts (compaction offsets, live[bounce + 1])
// first: nothing has written the hit records in this bounce yet
// filt_begin < filt_end and worklist != null: also builds the work list of the traversal launch that follows over the mesh
// objects [filt_begin, filt_end) (rays that surely miss all their world boxes are left out); that launch then gets
// order = worklist, listed = true.  (tile_desc, tile_stride, epoch: as for launch_raygen)
void launch_spheres(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, bool first, DPaths paths, DHits hits,
                    uint32_t max_paths, int bounce, DeviceCounters* counters, const DBatchInfo& bi, uint32_t filt_begin = 0u,
                    uint32_t filt_end = 0u, uint32_t* worklist = nullptr, unsigned long long* tile_desc = nullptr,
                    uint32_t tile_stride = 0u, uint32_t epoch = 0u);
// a run [obj_begin, obj_end) of mesh objects of the SAME mesh in one launch (k_traverse4m): variant 3 only
void launch_traverse_run(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, bool first, DPaths paths,
                         DHits hits, int bounce, int work_slot, DeviceCounters* counters, bool count_tests, uint32_t waves,
                         uint32_t* slow_list, const uint32_t* order, const DBatchInfo& bi, bool listed = false);
// the entry points of `nbeam` cameras (cams.c[cam_of[b]]) for the mesh object obj_index, into `out` (DBeam::entries)
void launch_beam(hipStream_t s, const DScene& scene, uint32_t obj_index, const DCameras& cams, const uint8_t* cam_of, uint32_t nbeam,
                 uint32_t tiles_x, uint32_t tiles_y, uint32_t node_count4, float4* out);
void launch_traverse(hipStream_t s, const DScene& scene, uint32_t obj_index, bool first, DPaths paths, DHits hits,
                     int bounce, int work_slot, DeviceCounters* counters, bool count_tests, uint32_t waves,
                     uint32_t* slow_list, const uint32_t* order, int variant, const DBatchInfo& bi, bool listed = false);
// coherence sort of the pick-up order (never of the slots): octs = direction octant per slot (written by launch_shade
// when given), order = per block of 4096 slots the slots grouped by octant; launch_traverse reads its rays through it
void launch_sort_octant(hipStream_t s, const uint8_t* octs, uint32_t* order, uint32_t max_paths, int bounce,
                        DeviceCounters* counters, const DBatchInfo& bi);
void launch_tail_count(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, bool first, DPaths paths,
                       DHits hits, uint32_t max_paths, int bounce, uint32_t* chunk_counts, DeviceCounters* counters,
                       const DBatchInfo& bi, bool emitters = false, bool roulette = false, const uint32_t* slot_base = nullptr);
void launch_scan(hipStream_t s, int bounce, bool last_bounce, const uint32_t* chunk_counts, uint32_t* chunk_offsets,
                 DeviceCounters* counters, const DBatchInfo& bi);
// roulette (launch_tail_count, launch_shade, launch_shade_fused): the bounce plays Russian roulette; the caller
// decides that and never asks for it at the last bounce -- the kRoulette instances do not look at last_bounce for it
void launch_shade(hipStream_t s, const DScene& scene, DPaths in, DPaths out, DHits hits, uint32_t max_paths,
                  bool staged, int bounce, bool last_bounce, const uint32_t* slot_base,
                  const uint32_t* chunk_offsets, DFrame fb, DBand band, DeviceCounters* counters, uint8_t* octs,
                  const DBatchInfo& bi, bool emitters = false, bool roulette = false, DEnv env = DEnv{nullptr, 0u, 0u});
// the end of a bounce in one pass (k_shade_fused): trailing sphere run [obj_begin, obj_end) + material + stable compaction +
// final gather.  tile_desc: shade_tiles_per_frame(max_paths) descriptors per frame of the batch (tile_stride apart), zero
// at allocation, cleared again only when the epochs start over; epoch: a number no earlier launch of this lap has used (1 .. 2^30 - 1).
// list: bounce 0 after launch_raygen(finish_misses): the work list of the bounce's one traversal launch -- the kernel
// walks it (DeviceCounters::list_count entries per frame) instead of all slots
void launch_shade_fused(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, bool first, DPaths in, DPaths out,
                        DHits hits, uint32_t max_paths, bool staged, int bounce, bool last_bounce, const uint32_t* slot_base,
                        unsigned long long* tile_desc, uint32_t tile_stride, uint32_t epoch, DFrame fb, DBand band,
                        DeviceCounters* counters, uint8_t* octs, const DBatchInfo& bi, const uint32_t* list = nullptr,
                        const DNextRun* next = nullptr, bool emitters = false, bool roulette = false, DEnv env = DEnv{nullptr, 0u, 0u});
// The environment (ptc_set_environment; pt_env.hip).  env.texels != null: launch_raygen (where it finishes the
// unlisted rays), launch_shade and launch_shade_fused hand over to these, the environment's instances of the same kernels, built with
// kEmit on; launch_env_sample: the lookup on `count` directions (three floats each, device memory), three floats out each
void launch_raygen_env(hipStream_t s, const DCameras& cams, const DBatchInfo& bi, DBand band, uint32_t pix_count, DPaths paths,
                       DeviceCounters* counters, const DObject* objects, uint32_t filt_begin, uint32_t filt_end, uint32_t* worklist, DHits hits,
                       unsigned long long* tile_desc, uint32_t tile_stride, uint32_t epoch, DFrame fb, bool staged, DLens lens, DEnv env);
void launch_shade_env(hipStream_t s, const DScene& scene, DPaths in, DPaths out, DHits hits, uint32_t max_paths, bool staged, int bounce,
                      bool last_bounce, const uint32_t* slot_base, const uint32_t* chunk_offsets, DFrame fb, DBand band, DeviceCounters* counters,
                      uint8_t* octs, const DBatchInfo& bi, bool roulette, DEnv env);
void launch_shade_fused_env(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, bool first, DPaths in, DPaths out, DHits hits,
                            uint32_t max_paths, bool staged, int bounce, bool last_bounce, const uint32_t* slot_base, unsigned long long* tile_desc,
                            uint32_t tile_stride, uint32_t epoch, DFrame fb, DBand band, DeviceCounters* counters, uint8_t* octs,
                            const DBatchInfo& bi, const uint32_t* list, const DNextRun* next, bool roulette, DEnv env);
void launch_env_sample(hipStream_t s, DEnv env, const float* dirs, uint32_t count, float* out);
// "prefold" at bounce 0: ray generation that also walks the sphere run in front of bounce 0's first mesh launch (next.hits: the
// CURRENT bounce's records here) and leaves the bytes for launch_list_flags
void launch_raygen_next(hipStream_t s, const DScene& scene, const DCameras& cams, const DBatchInfo& bi, DBand band, uint32_t pix_count, DPaths paths,
                        DeviceCounters* counters, const DNextRun& next, DLens lens = DLens{0.0f, 0.0f});
// the primary rays of one iteration for every slot of the band, 8 floats per slot (origin, t_min, direction, t_max): primary_ray and
// nothing else (ptc_generate_rays; k_generate_rays, pt_shade.hip)
void launch_generate_rays(hipStream_t s, const DCamera& cam, uint32_t iteration, DBand band, uint32_t pix_count, DLens lens, float4* rays);
// "prefold": the work list of a bounce whose leading sphere run the previous bounce's shade kernel has already walked, from the
// bytes it left (k_list_flags; tile_desc / epoch as for launch_spheres)
void launch_list_flags(hipStream_t s, const uint8_t* flags, uint32_t max_paths, int bounce, DeviceCounters* counters, const DBatchInfo& bi,
                       uint32_t* worklist, unsigned long long* tile_desc, uint32_t tile_stride, uint32_t epoch);
uint32_t shade_tiles_per_frame(uint32_t max_paths);
void launch_accumulate(hipStream_t s, DFrame stage, DFrame fb, uint32_t pix_count, const DBatchInfo& bi);
// the bounce-spanning persistent launch (pt_kernels.hip, k_persist): state set-up (k_persist_init) + the launch, `waves` wavefronts;
// spheres: the object list ends in a sphere run (pa.tail_begin / tail_end); listed0: bounce 0's shade pass walks pa.list0
void launch_persist(hipStream_t s, const DScene& scene, uint32_t obj_index, DHits hits, DeviceCounters* counters, const DBatchInfo& bi,
                    const DPersistArgs& pa, uint32_t waves, bool spheres, bool listed0, bool emitters = false);
uint32_t persist_tiles_per_frame(uint32_t max_paths);
// ---- the megakernel's launch (DESIGN sections 5g .. 5o) ----------------------------------------------------------------------
// What the options of the loop (mega_path, pt_megakernel.inc) read beside the scene.  Each is a kernel argument of the instances
// that know the option alone, kept out of DScene and DMeshView, which every other kernel takes by value; each has an "off" value
// -- a null first member, radius 0 -- and an instance that takes run-time choices reads the option from it.
// The lamp table (section 5f): records = 4 float4 per lamp primitive (ptc_light), thresholds = per record the first of the
// generator's 2^31 - 2 states that belongs to a later record (build_light_table), as a dense array.  records null: no lamp samples.
struct DLights {
  const float4* records;
  const uint32_t* thresholds;
  uint32_t count, last;        // records; last record with a weight > 0
  const DObject* objects;      // DScene's arrays: a sphere lamp reads its object's matrix and its sphere, every lamp its material
  const float4* spheres;
  const DMaterial* materials;
};
// The environment as a light (section 5k; pt_env_light.hpp).  table: the alias table of DEnv's map, n x n entries of 16 bytes
// (env_light::Entry), the context's own allocation beside the map; null: no environment samples (no map, or a map of weight 0).
struct DEnvLight {
  const uint4* table;
};
// Multiple importance sampling (section 5l; pt_mis.hpp).  inv_pdf_m: per material of the scene the inv_pdf every lamp record of that
// material carries, (float)(W / lum), 0 for a material that is no lamp or has lum 0; the scene's allocation beside the lamp table,
// null without one.
struct DMis {
  const float* inv_pdf_m;
};
// Smooth shading (section 5n; pt_smooth.hpp).  normals: three floats per vertex of the whole scene, object space, the scene's own
// allocation; mesh_first_vertex: per mesh where its vertices start in it.  normals null: the geometric normal.
struct DSmooth {
  const float* normals;
  const uint32_t* mesh_first_vertex;
};
// Image textures (section 5o; pt_texture.hpp).  texels: every texture's texels back to back, one allocation of the scene's pool;
// records: one per texture; material_texture: per material -1 or a texture; table: the two decode tables; st: two floats per
// triangle corner of the whole scene, parallel to its indices; mesh_first_index: per mesh where its corners start in it.  A null
// member: not set.
struct DTex {
  const uint32_t* texels;
  const texmap::Record* records;
  const int32_t* material_texture;
  const float* table;
  const float* st;
  const uint32_t* mesh_first_index;
};
// Normal maps (section 5q; pt_normal_map.hpp).  material_normal_map: per material -1 or a texture of DTex's pool; table: the normal
// maps' decode table, 256 floats.  They read DTex's texels, records, st and mesh_first_index.  material_normal_map null: no maps.
struct DNmap {
  const int32_t* material_normal_map;
  const float* table;
};
// The loop counters: kLightStatLines lines of kLoopStatWords 64-bit words (a 128-byte line each), one add per wavefront and word
// (the words: mega_path's table).  Not part of DeviceCounters, whose layout the feed depends on.
constexpr uint32_t kLoopStatWords = 16u;
// One frame of the megakernel: everything a launch takes.  ptc_trace builds it in one place (mega_frame, ptcore_trace.cpp), where
// every "off" value is written once; launch_megakernel (pt_kernels.hip) reads the frame's facts back from those values, asks the
// instance rule (pt_mega_rules.hpp) for the kernel, and the unit that holds that kernel launches it.  roulette: the kernel's argument
// as the rule decides it (mega_rules::roulette_argument); stats: the loop counters, null for a frame that counts nothing; emitters,
// weigh: the two facts no member carries (the scene has an emissive material; the balance heuristic applies).
struct MegaFrame {
  DScene scene;
  DLights lights;
  DCamera cam;
  uint32_t iteration;
  DBand band;
  uint32_t pix_count;
  int max_bounces;
  DFrame fb;
  DeviceCounters* counters;
  unsigned long long* stats;
  int roulette;
  DLens lens;
  DEnv env;
  DEnvLight el;
  DMis mis;
  DSmooth sm;
  DTex tx;
  DNmap nm;
  bool emitters, weigh;
};
void launch_megakernel(hipStream_t s, const MegaFrame& f);
void launch_preview(hipStream_t s, const float4* buf, uint32_t pix_count, int mode, uint32_t* rgba);
void launch_pack(hipStream_t s, const float4* buf, uint32_t pix_count, int which, float* dst);
// the bands of one multi-GPU gather launch (k_gather_bands): up to kGatherBands sources per launch
constexpr int kGatherBands = 16;
struct DGatherBands {
  struct Src {
    const float* src;
    DBand band;
    uint32_t pix_count;
  } src[kGatherBands];
};
void launch_gather_bands(hipStream_t s, const DGatherBands& bands, uint32_t count, uint32_t max_pix, int channels,
                         uint32_t frame_pixels, float* frame);
void launch_preview_packed(hipStream_t s, const float* buf, uint32_t pix_count, int channels, int mode, uint32_t* rgba);
// The display transform (ptc_set_display; pt_display.hip).  DMeter: the words k_meter adds into, zero between
// calls (k_meter_level leaves them so).  DExposure: what k_meter_level makes of them -- the histogram as counted, the mean bin of
// its trimmed middle (-1: nothing counted), that bin's lower edge and the factor k_tonemap multiplies every channel by.
// src4 (a float4 a pixel, 16-byte aligned) or src3 (three floats a pixel): exactly one is not null.  launch_meter's grid is capped at
// kMeterMaxBlocks workgroups of kMeterBlock threads, which stride over the rest.  launch_tonemap: metered null = `scale` as given;
// rgba or mapped (three floats a pixel) may be null.
constexpr int kMeterBlock = 256;
constexpr uint32_t kMeterMaxBlocks = 2048u;
struct DMeter {
  uint32_t hist[256];
  uint32_t below, rejected;
};
struct DExposure {
  uint32_t hist[256];
  uint32_t pixels, counted, below, rejected;
  int32_t level_bin;
  float level, scale;
};
void launch_meter(hipStream_t s, const float4* src4, const float* src3, uint32_t pix_count, DMeter* acc);
void launch_meter_level(hipStream_t s, DMeter* acc, DExposure* out, uint32_t pix_count, uint32_t low_permille, uint32_t high_permille,
                        float key, float exposure);
void launch_tonemap(hipStream_t s, const float4* src4, const float* src3, uint32_t pix_count, const DExposure* metered, float scale,
                    int curve, float w2, uint32_t* rgba, float* mapped);
void launch_denoise_positions(hipStream_t s, const DCamera& cam, uint32_t pix_count, const float4* nd, float4* pos);
void launch_denoise_pass(hipStream_t s, const DCamera& cam, uint32_t pix_count, const float4* color, const float4* nd,
                         const float4* pos, float4* out, int step_width, DDenoise params);
void launch_intersect(hipStream_t s, const DScene& scene, const float4* rays_o, const float4* rays_d, uint32_t n,
                      DHits hits, DeviceCounters* counters, int variant);
// occlusion queries (pt_occlude.hip): rays_o = origin.xyz, bits(t_min flag << 31); rays_d = direction.xyz, t_max; occluded = one byte
// per ray, zeroed by the caller, set to 1 by the kernels and never read-modify-written.
//   launch_occlude_spheres  the sphere objects of [obj_begin, obj_end) for every ray not flagged yet
//   launch_occlude          one mesh object: k_traverse4's persistent wavefronts, stopping at the first accepted triangle; counters:
//                           one block with live[0] = rays (the feed), its slow_rays[0] counts the rays redone exactly
void launch_occlude_spheres(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, const float4* rays_o,
                            const float4* rays_d, uint32_t n, uint8_t* occluded);
void launch_occlude(hipStream_t s, const DScene& scene, uint32_t obj_index, const float4* rays_o, const float4* rays_d,
                    uint8_t* occluded, int work_slot, DeviceCounters* counters, uint32_t waves, uint32_t* slow_list, const DBatchInfo& bi);
// direct-light queries (pt_light.hip) on the lamp table, DLights
constexpr uint32_t kLightSeedXor = 0x4c495445u;  // xor-ed into path_seed(point, sample_index): no render path xors its seed
// Russian roulette (ptc_set_param "roulette"): xor-ed into path_seed(slot or pixel, iteration); discard(bounce), one draw
constexpr uint32_t kRouletteSeedXor = 0x52524c54u;
// the thin lens (ptc_set_lens): xor-ed into path_seed(pixel, iteration); two draws, the point on the lens disk
constexpr uint32_t kLensSeedXor = 0x4c454e53u;
// the environment as a light (ptc_environment_light, "environment_light"): xor-ed into path_seed(point or pixel,
// sample_index or iteration); four draws a sample (the render loop: discard(4 * bounce))
constexpr uint32_t kEnvLightSeedXor = 0x454e564cu;
constexpr uint32_t kLightStatLines = 64u;        // the resolve kernel's two counters, spread over this many 128-byte lines
//   launch_light_sample   one thread per point: the shadow ray in the path-state layout occlude_on_device takes (o4 = p, tmin_word;
//                         d4 = w, t_max) and contrib = {unshadowed contribution rgb, 1 if sampled else 0}; a culled sample: t_max 0
//                         tmin_word: 0 (the any-hit kernels' flag word) or the bits of 1e-4f (launch_intersect's plain t_min)
//   launch_light_resolve  radiance = sampled and not occluded ? contribution : 0; visible, rays (8 floats per point) may be null;
//                         occluded: one byte per point, or (null) closest_tp: launch_intersect's records, hit iff .x >= 0;
//                         stats: kLightStatLines lines of 32 words, word 0 += sampled, word 1 += visible
void launch_light_sample(hipStream_t s, const DLights& lights, const float* points, const float* normals, uint32_t n, uint32_t sample_index,
                         uint32_t tmin_word, float4* o4, float4* d4, float4* contrib);
void launch_light_resolve(hipStream_t s, const float4* o4, const float4* d4, const float4* contrib, const uint8_t* occluded,
                          const float4* closest_tp, uint32_t n, float* radiance, float* rays, uint8_t* visible, uint32_t* stats);
//   launch_env_light_sample  launch_light_sample's shape (pt_env.hip): one thread per point, one environment sample each; the shadow
//                            ray is {p, tmin_word; w, FLT_MAX}, a culled sample's t_max 0.  launch_light_resolve takes it from there
void launch_env_light_sample(hipStream_t s, DEnv env, DEnvLight el, const float* points, const float* normals, uint32_t n, uint32_t sample_index,
                             uint32_t tmin_word, float4* o4, float4* d4, float4* contrib);
// ptc_hit_attributes' kernel (pt_mega_smooth.hip): one thread per ray, the reference's walk (ray_scene) on the thread's LDS stack.
// rays: two float4 a ray, {origin, t_min} {direction, t_max}; per ray the winner's object and triangle (0xffffffff: a miss / a
// sphere), u, v, and the shading normal (sm.normals null: the geometric one); flags |= kFlagStackOverflow
void launch_hit_attributes(hipStream_t s, const DScene& scene, DSmooth sm, const float4* rays, uint32_t n, uint32_t* object_out,
                           uint32_t* triangle_out, float2* uv_out, float* normal_out, uint32_t* flags);
// ptc_sample_texture's kernel (pt_mega_tex.hip): one thread per coordinate pair, texmap::lookup on one record of the pool; rgb 3
// floats a pair (zeros where the rule refuses the pair), rejected (may be null) one byte a pair
void launch_texture_sample(hipStream_t s, DTex tx, uint32_t texture, const float* st, uint32_t n, float* rgb, uint8_t* rejected);
// ptc_hit_surface's kernel (pt_mega_tex.hip): k_hit_attributes' walk; per ray the interpolated s, t (tx.st null, a sphere, a miss:
// zeros) and the albedo the loop would use at the hit (a miss: zeros); flags |= kFlagStackOverflow
void launch_hit_surface(hipStream_t s, const DScene& scene, DTex tx, const float4* rays, uint32_t n, float2* st_out, float* albedo_out,
                        uint32_t* flags);
// ptc_hit_shading_normal's kernel (pt_mega_nmap.hip): k_hit_surface's walk; per ray the normal the loop would hand evaluate_material
// at the closest hit from what is set (sm.normals, nm.material_normal_map; either may be null) and what the rule did there
// (nmap::kMiss .. kKept); flags |= kFlagStackOverflow
void launch_hit_shading_normal(hipStream_t s, const DScene& scene, DSmooth sm, DTex tx, DNmap nm, const float4* rays, uint32_t n,
                               float* normal_out, uint8_t* outcome_out, uint32_t* flags);
// "denoise_albedo" (pt_denoise_albedo.hip).  launch_denoise_albedo: one wavefront per 8 x 8 pixel tile of cam's frame;
// per pixel the first-hit albedo under tx (k_hit_surface's at a diffuse or metal hit, else ones) and the colour demodulated by it, a
// float4 each; rays (may be null) 2 float4 a pixel: the pixel-centre ray it walked; stats: kLightStatLines lines of kLoopStatWords
// words, 0 .. 3 += pixels, surface hits, texel lookups, floored channels; flags |= kFlagStackOverflow.  launch_remodulate: front =
// front x the effective albedo of that plane, in place
void launch_denoise_albedo(hipStream_t s, const DScene& scene, DTex tx, const DCamera& cam, const float4* color, float4* albedo,
                           float4* irradiance, float4* rays, unsigned long long* stats, uint32_t* flags);
void launch_remodulate(hipStream_t s, uint32_t pix_count, const float4* albedo, float4* front);
// "denoise_variance" (pt_denoise_variance.hip).  launch_variance_estimate: per pixel the weighted variance of `color`
// over its 7 x 7 window (normal and position weights, centred form), one float a pixel.  launch_variance_prefilter: the 3 x 3
// Gaussian of a variance plane (prefiltered may be null: the counters alone); stats: kLightStatLines lines of kLoopStatWords words, 0 and 1 += pixels, pixels below the floor.  launch_denoise_var_pass: one guided pass at
// step_width -- colour and variance in, colour and variance out (neither pair may alias); the LDS kernel for the steps 1 .. 32 that are
// powers of two under variant 0, else the through-cache kernel.
void launch_variance_estimate(hipStream_t s, uint32_t width, uint32_t height, const float4* color, const float4* nd, const float4* pos,
                              float* variance, float n_phi, float p_phi);
void launch_variance_prefilter(hipStream_t s, uint32_t width, uint32_t height, const float* variance, float* prefiltered,
                               unsigned long long* stats);
void launch_denoise_var_pass(hipStream_t s, const DCamera& cam, uint32_t pix_count, const float4* color, const float* variance,
                             const float4* nd, const float4* pos, float4* out, float* variance_out, int step_width, DDenoiseVar params);
// ptc_environment_light_pdf's kernel (pt_env.hip): one thread per unit direction, env_light::density
void launch_env_light_pdf(hipStream_t s, DEnvLight el, uint32_t n, const float* dirs, uint32_t count, float* pdf);
void launch_selftest(hipStream_t s, const float* a, const float* b, uint32_t n, float* out_div, float* out_sqrt,
                     float* out_sin, float* out_cos);
void launch_selftest_rng(hipStream_t s, const uint32_t* seeds, const uint32_t* discards, uint32_t n, uint32_t* out);
// test hook (ptc_debug_sphere_lanes): sphere_run_lanes<slots> on the run [obj_begin, obj_end), rays and records in the path-state
// layout, cand (may be null) one byte per ray; false (nothing launched): slots is neither 1 nor the fused kernel's slots per lane
bool launch_debug_sphere_lanes(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, int slots, const float4* rays_o4,
                               const float4* rays_d4, float4* hit_tp, float4* hit_nm, uint32_t n, uint8_t* cand);

}  // namespace pt
