/*
 * ptcore.h -- C ABI of libptcore.so, the MI355X (gfx950) path-tracing core.
 *
 * This is the drop-in boundary for the render core of LesleyLai/cuda-path-tracer: one `ptc_ctx`
 * replaces one `class PathTracer` (reference src/lib/path_tracer.hpp:60-99) together with the
 * device-side `Scene` it owns (src/lib/scene.hpp:25-67).  Each entry point names the reference
 * interface it replaces.  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - every function returns PTC_OK (0) or a negative ptc_status; nothing calls exit()
 *     (the reference's CUDA_CHECK / panic abort the process: cuda_utils/cuda_check.cpp:7-23,
 *     prelude.cpp:5-10);  ptc_last_error() gives the message of the last failure.
 *   - one context = one GPU = one host thread at a time (same as the reference, which is
 *     single-threaded on the default stream).
 *   - matrices are column-major float[16] (glm layout): m[4*col + row].
 *   - framebuffers are row-major, row 0 = top of the view, flat index = x + y*width
 *     (cuda_utils/indices.cuh:20-26).
 *   - there is NO CPU fallback: every call that needs the GPU fails with PTC_ERR_NO_DEVICE /
 *     PTC_ERR_HIP when no gfx950 device is usable.
 */
#ifndef PTCORE_H
#define PTCORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTC_ABI_VERSION 3

typedef enum ptc_status {
  PTC_OK = 0,
  PTC_ERR_INVALID = -1,       /* bad argument / bad call order */
  PTC_ERR_NO_DEVICE = -2,     /* no usable HIP device */
  PTC_ERR_HIP = -3,           /* a HIP runtime call or kernel failed */
  PTC_ERR_OOM = -4,
  PTC_ERR_BVH = -5,           /* BVH build failed (empty SAH side: bvh.cpp:84-85) */
  PTC_ERR_STACK = -6,         /* traversal stack overflow (reference: UB beyond depth 24, static_stack.hpp:21-25) */
  PTC_ERR_NO_SCENE = -7
} ptc_status;

/* GPUMethod, path_tracer.hpp:57 */
typedef enum ptc_method { PTC_METHOD_MEGAKERNEL = 0, PTC_METHOD_STREAMING = 1 } ptc_method;

/* DisplayBufferType, path_tracer.hpp:19 */
typedef enum ptc_display { PTC_DISPLAY_FINAL = 0, PTC_DISPLAY_COLOR = 1, PTC_DISPLAY_NORMAL = 2, PTC_DISPLAY_DEPTH = 3 } ptc_display;

/* which accumulated framebuffer ptc_download reads */
typedef enum ptc_buffer { PTC_BUF_COLOR = 0, PTC_BUF_NORMAL = 1, PTC_BUF_DEPTH = 2, PTC_BUF_FINAL = 3 } ptc_buffer;

/* ObjectType + GPUObject, scene.hpp:14-22.  Same 160-byte layout as the reference. */
typedef struct ptc_object {
  uint32_t type;      /* 0 sphere, 1 mesh */
  uint32_t index;     /* sphere index; 0 for meshes (scene_description.cpp:42) */
  float m[16];        /* Transform::m_ */
  float inv_m[16];    /* Transform::inverse_m_ */
  float aabb_min[3];  /* world-space AABB */
  float aabb_max[3];
} ptc_object;

/* Sphere, sphere.hpp:8-11 */
typedef struct ptc_sphere { float center[3]; float radius; } ptc_sphere;

/* Material, material.hpp:19-38 (20 bytes).  type 0 Diffuse {albedo rgb}, 1 Metal {albedo rgb, fuzz},
 * 2 Dielectric {refraction_index},
 *   Defined behaviour -- the reference's bits, pinned by tests/test_gpu_materials.py -- for any finite albedo (0, above 1,
 *   products that become denormal or overflow included) and fuzz (above 1 included) and any finite refraction index > 0;
 *   nothing is clamped.  Other values of types 0-2 (index 0 or negative, NaN / inf in a record) are not refused: they give
 *   the reference's NaN, in the same pixels, and no more is promised for them.
 * 3 Emissive {emitted radiance rgb, p[3] reserved: 0} -- an extension (the reference has no emitters; parity unpinned by
 *   construction, like ptc_mesh_range).  Each component finite and >= 0, else ptc_upload_scene fails with PTC_ERR_INVALID.
 *   A path whose closest hit is emissive ends at that bounce with colour * emission (binary32, per component, as a miss
 *   ends with colour * sky), makes no draw there and is not a survivor: it leaves the compaction like a miss, so the
 *   slots -- and the random numbers -- of the paths behind it, live[] and ptc_stats.last_live count only the paths that
 *   go on.  Two-sided (the side bit is ignored); at bounce 0 normal / depth are the hit's.  Streaming and megakernel
 *   alike, every schedule parameter included (scenes whose table holds a type 3 run instances of the shade kernels built
 *   for it; other scenes run exactly the code they ran before). */
typedef struct ptc_material { int32_t type; float p[4]; } ptc_material;

/* BVHNode, accelerators/bvh.hpp:17-28 (32 bytes).  leaf <=> primitive_count != 0; for a leaf
 * first_child_or_primitive is the offset of its triangle in the index array (multiple of 3); for an
 * inner node it is the left child, the right child is +1. */
typedef struct ptc_bvh_node {
  float aabb_min[3];
  float aabb_max[3];
  uint32_t first_child_or_primitive;
  uint32_t primitive_count;
} ptc_bvh_node;

/* One mesh of a scene that has several (an extension: the reference keeps ONE mesh per scene whatever the scene
 * file holds, scene_description.cpp:42,95 -- SURVEY section 8 f2).  Ranges into ptc_scene_desc's positions / indices /
 * bvh arrays; the indices of a mesh count from ITS first vertex, its BVH nodes from ITS first node (each mesh as
 * bvh_from_mesh would return it on its own). */
typedef struct ptc_mesh_range {
  uint32_t first_vertex, vertex_count;
  uint32_t first_index, index_count;
  uint32_t first_bvh_node, bvh_node_count; /* bvh_node_count 0: built by ptc_upload_scene */
} ptc_mesh_range;

/* The flat arrays SceneDescription::build_scene() uploads with six cudaMemcpy calls
 * (scene_description.cpp:54-114).  Host pointers; copied during ptc_upload_scene. */
typedef struct ptc_scene_desc {
  const ptc_object* objects;
  uint32_t object_count;
  const uint32_t* object_material_indices; /* object_count entries */
  const ptc_sphere* spheres;
  uint32_t sphere_count;
  const ptc_material* materials;
  uint32_t material_count;
  /* 3 floats per vertex.  Every vertex that a triangle uses must be finite: a NaN or infinite coordinate in one fails
   * ptc_upload_scene with PTC_ERR_INVALID and a message that names the mesh and the vertex, before anything is built
   * or uploaded (the scene uploaded before stays).  A vertex no triangle uses may hold anything. */
  const float* positions;
  uint32_t vertex_count;
  const uint32_t* indices;                 /* 3 per triangle */
  uint32_t index_count;
  /* optional: NULL -> built by ptc_upload_scene.  A caller's tree must keep, besides the ranges (children after their
   * parent, leaf triangles inside the index array, min <= max), four rules the traversal layouts rely on: every node
   * but the root is the child of exactly one node; a leaf's offset is a multiple of 3; a leaf's box contains its
   * triangle's three vertices; a child's box lies inside its parent's.  Exact float comparisons; a tree that breaks
   * one fails with PTC_ERR_INVALID and a message that names the node (every caller tree is checked before the
   * first BVH is built on the device).  Depth <= 62, else PTC_ERR_STACK. */
  const ptc_bvh_node* bvh;
  uint32_t bvh_node_count;
  /* optional mesh table (NULL: the arrays above are the scene's one mesh, every mesh object instantiates it and
   * ptc_object::index is ignored, like the reference).  With a table, a mesh object's `index` names its mesh. */
  const ptc_mesh_range* meshes;
  uint32_t mesh_count;
} ptc_scene_desc;

/* Camera, camera.hpp:17-23 */
typedef struct ptc_camera {
  float position[3];
  float rotation_wxyz[4]; /* glm::quat, default {1,0,0,0} */
  float vfov;             /* radians */
} ptc_camera;

/* EdgeAvoidingATrousDenoiser's public fields, denoising/edge_avoiding_a_trous_denoiser.hpp:9-12 */
typedef struct ptc_denoiser_params {
  int32_t filter_size;   /* default 10 */
  float color_weight;    /* default 0.45 */
  float normal_weight;   /* default 0.30 */
  float position_weight; /* default 0.25 */
} ptc_denoiser_params;

typedef struct ptc_config {
  int32_t device;       /* HIP device ordinal (the reference never selects one: cli.cpp:71-78) */
  int32_t max_bounces;  /* reference: compile-time 50 (path_tracer.cu:27); <=0 -> 50 */
  int32_t method;       /* ptc_method; default streaming (path_tracer.hpp:64) */
  int32_t reserved;
} ptc_config;

#define PTC_MAX_BOUNCES_CAP 64

typedef struct ptc_stats {
  uint64_t rays_total;                       /* closest-hit queries since ptc_restart / create */
  uint64_t frames;                           /* ptc_trace calls that rendered since then */
  uint32_t last_live[PTC_MAX_BOUNCES_CAP];   /* live paths entering each bounce of the last streaming frame */
  uint32_t bvh_node_count;
  uint32_t bvh_max_depth;
  uint32_t triangle_count;
  uint32_t stack_capacity;                   /* traversal stack entries available per ray */
} ptc_stats;

/* Measurement support (no reference equivalent; the reference only has a wall-clock Stopwatch, cli.cpp:27-60).
 * Per bounce index, summed over every streaming frame traced since ptc_reset_profile:
 *   paths      live paths that entered the bounce (= closest-hit queries = rays)
 *   node_visits BVH node records fetched by the closest-hit kernel (counting runs; one four-child 64-byte record
 *              in the default kernel, one two-child record in variant 1, one 32-byte node in variant 0)
 *   trace_ms   duration of the closest-hit kernel, from HIP events recorded on the context's stream
 *              around each launch (only while events are enabled)
 *   box_tests  ray/AABB tests of BVH nodes, tri_tests  ray/triangle tests (only while counting is
 *              enabled: an instrumented, slower kernel variant -- never time it) */
typedef struct ptc_profile {
  uint64_t paths[PTC_MAX_BOUNCES_CAP];
  uint64_t box_tests[PTC_MAX_BOUNCES_CAP];
  uint64_t tri_tests[PTC_MAX_BOUNCES_CAP];
  double trace_ms[PTC_MAX_BOUNCES_CAP];
  uint32_t trace_launches[PTC_MAX_BOUNCES_CAP];
  uint32_t max_box_tests[PTC_MAX_BOUNCES_CAP]; /* longest single traversal seen (counting runs) */
  uint64_t listed_rays[PTC_MAX_BOUNCES_CAP]; /* rays the traversal launches fetched through a work list ("filter_rays"); 0: they walked all live rays */
  uint64_t slow_rays[PTC_MAX_BOUNCES_CAP];   /* rays redone with exact box decisions at the end of a traversal launch (always counted) */
  uint64_t node_visits[PTC_MAX_BOUNCES_CAP]; /* BVH node records fetched (counting runs): SURVEY 8(d)'s N_node */
  double denoise_ms;                         /* summed duration of the A-Trous passes (HIP events, while events are enabled) */
  uint32_t denoise_passes;
  uint32_t persist_launches;                 /* batches whose bounces >= 1 and shade passes ran as ONE persistent launch ("persist", k_persist) */
} ptc_profile;

typedef struct ptc_ctx ptc_ctx;

/* ---- lifetime ---- */
int ptc_abi_version(void);
int ptc_device_count(int* count);                                   /* cli.cpp:72-73 cudaGetDeviceCount */
int ptc_create(const ptc_config* config, ptc_ctx** out);            /* PathTracer::PathTracer(), path_tracer.cu:387 */
void ptc_destroy(ptc_ctx* ctx);                                     /* ~PathTracer (cuda::Buffer dtors, cuda_buffer.hpp:20) */
const char* ptc_last_error(const ptc_ctx* ctx);                     /* ctx may be NULL: last ptc_create failure */

/* Use an externally owned HIP stream (hipStream_t as void*), e.g. torch's current stream, for all
 * kernels of this context.  NULL restores the context's own stream. */
int ptc_set_stream(ptc_ctx* ctx, void* hip_stream);

/* ---- scene + buffers ---- */
/* Upload half of PathTracer::create_buffers (path_tracer.cu:559-564) = SceneDescription::build_scene's
 * device uploads.  An empty mesh (index_count == 0) is accepted (the reference panics, bvh.cpp:200).  Every refusal that
 * depends on the caller's arrays alone leaves the previously uploaded scene in place. */
int ptc_upload_scene(ptc_ctx* ctx, const ptc_scene_desc* scene);
/* PathTracer::resize_image (path_tracer.cu:527-545): (re)allocates all per-pixel buffers, restarts. */
int ptc_resize(ptc_ctx* ctx, uint32_t width, uint32_t height);
/* Render only image rows [row_begin,row_end) of the width x height frame (multi-GPU row bands;
 * no reference equivalent).  Must follow ptc_resize.  Default: all rows. */
int ptc_set_rows(ptc_ctx* ctx, uint32_t row_begin, uint32_t row_end);
/* Load-balanced multi-GPU partition: the frame is cut into blocks of block_rows rows dealt round-robin to
 * nranks contexts; this context renders the blocks rank, rank+nranks, ...  Its framebuffers (ptc_download,
 * ptc_present_rgba8) hold those rows packed in order.  Slot numbering is per context ("local"), so the noise
 * pattern differs from the single-context image; contiguous bands (ptc_set_rows) keep the exact option. */
int ptc_set_interleave(ptc_ctx* ctx, uint32_t rank, uint32_t nranks, uint32_t block_rows);
int ptc_restart(ptc_ctx* ctx);                                      /* PathTracer::restart, path_tracer.cu:522-525 */
int ptc_iteration(const ptc_ctx* ctx);                              /* PathTracer::iteration(), path_tracer.hpp:88 */
int ptc_set_iteration(ptc_ctx* ctx, int iteration);                 /* test hook: continue from a given sample index */

/* public mutable fields of PathTracer (path_tracer.hpp:62-66) */
int ptc_set_max_iterations(ptc_ctx* ctx, int max_iterations);       /* PathTracer::max_iterations (default 1) */
int ptc_set_method(ptc_ctx* ctx, int method);                       /* PathTracer::current_gpu_method */
int ptc_set_max_bounces(ptc_ctx* ctx, int max_bounces);             /* static max_bounces = 50, path_tracer.cu:27 */
int ptc_set_denoiser_params(ptc_ctx* ctx, const ptc_denoiser_params* p); /* PathTracer::atrous_denoiser */
/* Closest-hit kernel variant (speed only; all return the same hits, bit for bit -- same box decisions, same
 * tie rule; 0 and 1 exist to cross-check the default on the GPU):
 *   3 (default) = persistent wavefronts whose lanes fetch the next ray as soon as their own is finished, over the
 *                 tree collapsed to four children per 64-byte quantised node; box decisions only conservative, the
 *                 winning triangle re-checked against its parent's box with the reference's arithmetic
 *                 (sufficient: see DESIGN.md "nesting"); objects walked as sphere / mesh segments; the only
 *                 variant that traces several iterations per launch ("batch_frames")
 *   1           = culled near-first traversal with exact box decisions, one wavefront per 64 fixed paths (the
 *                 walk the default uses for the few rays it sets aside)
 *   0           = traversal in the reference's own order (path_tracer.cu:36-76: depth-first, left first, no
 *                 t culling) */
int ptc_set_trace_variant(ptc_ctx* ctx, int variant);
/* Knobs by name.  Three kinds (round-3 review: "they are ABI now -- mark which are stable"):
 *   STABLE   part of the interface: meaning and default are kept, an application may rely on them
 *              frames_in_flight, batch_frames, slot_offset, traverse_waves
 *   SCHEDULE choose between implementations that return the SAME bits; kept for A/B measurements and as cross-checks of
 *            each other, defaults may move with the hardware, a name may go when its alternative goes
 *              fused_shade, filter_rays, merge_instances, sphere_lanes, sphere_fold, beam, ray_sort, denoise_variant, bvh_build_on_device,
 *              layout_on_device, split_idle, refill_lanes, static_eighths, small_waves, small_rays_per_lane, min_waves
 *   TEST     hooks for the parity tests only: debug_lds_entries, debug_force_slow, debug_shade_epoch
 * None of them changes a result, with one exception that is the point of it: slot_offset keys the material RNG
 * (multi-GPU).  Unknown names return PTC_ERR_INVALID.  Known names:
 *   "frames_in_flight" consecutive iterations in flight at once, folded into the framebuffer in iteration order
 *                      (default: 64, fewer when their path state would exceed 24 GiB; 1 = strictly serial on
 *                      the context's stream; 1..256; set before ptc_resize)
 *   "batch_frames"     iterations traced by the same launches (default 32; 1..32; before ptc_resize).  ptc_trace
 *                      queues an iteration and enqueues the batch when it is full or when any other call
 *                      looks at the context; frames_in_flight / batch_frames batches run on separate streams.
 *                      The library asks the HIP runtime for 24 hardware queues (GPU_MAX_HW_QUEUES, default 4:
 *                      streams on one queue serialise) when it is loaded before the runtime starts; an
 *                      application that initialises HIP first should export GPU_MAX_HW_QUEUES=24 itself
 *   "merge_instances"  1 (default): consecutive mesh objects that instantiate the same mesh are walked by one traversal
 *                      launch per bounce (a lane keeps its ray and takes the instances in turn); 0: one launch each
 *   "bvh_build_on_device"  1 (default): a scene without BVH gets the reference BVH from the GPU builder
 *                      (ptc_build_bvh_device); 0: from the threaded host builder.  Same nodes either way
 *   "layout_on_device" 1 (default): the traversal layouts (collapsed four-wide tree, leaf order, per-instance
 *                      triangle records) are derived on the GPU; 0: on the host.  Same bytes either way
 *                      (ptc_download_layout); a caller's BVH that is not numbered depth by depth goes to the host
 *   "fused_shade"      1 (default): the end of a bounce -- trailing sphere run, material, stable compaction, final gather -- is
 *                      ONE kernel (tiles by ticket, decoupled look-back; a bounded wait reports PTC_ERR_HIP from ptc_get_stats
 *                      instead of ever hanging); 0: three kernels (count, scan, shade)
 *   "filter_rays"      1 (default): the kernel in front of a mesh launch (a sphere run; ray generation at bounce 0) also lists the
 *                      rays that may hit one of the launch's world boxes at all -- in slot order, by the look-back scan of
 *                      "fused_shade" -- and the launch walks only those (ptc_profile::listed_rays).  When bounce 0's launch
 *                      covers the scene's whole mesh part (only the sphere run that ends the object list follows), a primary ray
 *                      that is not listed hits nothing: its path ends in ray generation and the bounce's shade kernel walks the
 *                      list.  Images, live counts and ray totals are those of 0: every live ray is fetched by the launch
 *   "traverse_waves"   most persistent wavefronts a traversal launch may use (default 5120 = the number that is
 *                      resident at 5 per SIMD; before ptc_upload_scene).  A launch uses one wavefront per 3072
 *                      primary rays it carries, at least 1024
 *   A batch of a single iteration (an interactive front-end that presents or denoises after every iteration, the
 *   stepwise calls) runs in one of eight extra one-frame slots with streams of their own, so that viewer-style
 *   use keeps eight frames in flight as well (config 5, 1 spp + denoise per 1080p frame: 1.6 ms)
 *   "ray_sort"         1: from the second bounce on, the persistent traversal lanes pick their rays up grouped by
 *                      direction octant within blocks of 4096 neighbouring slots (an index array built by a small
 *                      kernel per bounce; the slots themselves, and so the random numbers, stay where they are).
 *                      Default 0: measured on the benchmark scene it does not pay for itself.  Before
 *                      ptc_resize
 *   "denoise_variant"  0 (default): the A-Trous passes stage their taps in LDS, one sub-lattice of the dilated filter per
 *                      workgroup; 1: taps through L1 / L2 (round-1 kernel, kept as a cross-check).  Same results up to
 *                      summation order (both within 1e-5 of the oracle)
 *   "denoise_albedo"   DENOISING (default 0; an extension): 1 = ptc_denoise filters irradiance, not colour.  Per
 *                      pixel the first-hit albedo of the pixel-centre view ray (k_denoise_albedo: at a diffuse or metal hit what
 *                      ptc_hit_surface reports there -- with the texel only while "textures" is 1 and textures and coordinates
 *                      are set --, at glass, an emitter and on a miss (1, 1, 1)); per channel e = albedo > 1/64 ? albedo : 1/64 (a NaN
 *                      takes 1/64); the passes run on colour / e with the same normals, positions, weights and "denoise_variant",
 *                      and their result x e is the final buffer (k_remodulate).  ptc_profile's denoise_passes and denoise_ms count
 *                      the passes as before; the stage's own time and counters: ptc_get_denoise_albedo_stats.  A filter_size < 1
 *                      runs no stage.  Two float4 planes per pixel, allocated by the first call that needs them and released with
 *                      the frame.  0 launches exactly what was launched before the parameter existed.  Any time
 *   "denoise_variance" DENOISING (default 0; an extension): 1 = ptc_denoise steers the colour weight by a per-pixel
 *                      variance instead of the constant color_weight.  An estimate stage (k_variance_estimate) takes, per pixel, the
 *                      variance of the plane the passes filter -- the accumulated colour, or the irradiance under "denoise_albedo" 1
 *                      -- over its 7 x 7 window (coordinates clamped to the image; tap weights exp(-(|dn|^2 / normal_weight +
 *                      |dx|^2 / position_weight)); centred: the weighted mean first, then the weighted squared distance from it, summed
 *                      over the channels).  A pass at step s keeps the 5 x 5 taps, their kernel weights, their coordinate contract and
 *                      the normal and position terms of the plain pass; its colour term is |dc|^2 / (sigma x v + 2^-53), v the 3 x 3
 *                      Gaussian (1 2 1; 2 4 2; 1 2 1) / 16 of the current variance plane around the centre pixel at one-pixel spacing;
 *                      it writes c' = sum w c / sum w and v' = sum w^2 v / (sum w)^2, and v' travels with c' through the ping-pong.
 *                      color_weight is not read.  sigma: ptc_set_denoise_variance.  The passes count into ptc_profile's
 *                      denoise_passes and denoise_ms as the plain ones do; the stage's own time and counters:
 *                      ptc_get_denoise_variance_stats.  "denoise_variant" picks the passes' kernel as before.  A filter_size < 1 runs
 *                      no stage.  Two float planes per pixel, allocated by the first call that needs them and released with the
 *                      frame.  0 launches exactly what was launched before the parameter existed.  Any time
 *   "slot_offset"     added to every compacted slot index before the material RNG is seeded (path_tracer.cu:300).  A
 *                      rank of a multi-GPU run that numbers its paths locally (ptc_set_interleave) sets rank * (pixels of
 *                      the largest share) so that no two ranks draw the same random streams; 0 (default) = the reference
 *   "beam"             1 (default): when a bounce-0 traversal launch walks one mesh object, a small kernel first computes, per
 *                      8 x 8-pixel tile and distinct camera of the batch, the deepest nodes of that object's tree the tile's
 *                      frustum overlaps (at most four, with their boxes), and the primary rays start there instead of at the
 *                      root; 0: at the root.  Before ptc_resize
 *   "sphere_lanes"     1 (default): in the kernel that ends a bounce, a sphere run that ends the object list and consists of
 *                      at most eight spheres whose matrices are pure translations is tested candidate by candidate, every
 *                      lane with the spheres IT cannot rule out ("select approximately, verify exactly": approximate bounds
 *                      on the root the reference would accept, then the reference's own sequence for each candidate);
 *                      0: object by object for the whole wavefront.  Any time
 *   "sphere_fold"      1 (default): a sphere run IN FRONT of a mesh whose objects are all translated spheres (a room's
 *                      walls) is walked with the matrix products that are sums with zeros written as those sums, and the hit
 *                      record's normal finished once, for the hit that remains, instead of for every accepted hit on the way
 *                      (same operations on the same operands; a wavefront with a ray on one of the exceptions -- a -0.0f
 *                      coordinate against a zero translation, a zero direction component, anything non-finite -- takes the
 *                      plain form); 0: the plain form.  Any time
 *   "min_waves"        fewest persistent wavefronts of a traversal launch (default 1024)
 *   "split_idle"       once a traversal launch has handed out its last ray: idle lanes of a persistent wavefront that
 *                      trigger work splitting (an idle lane takes over the bottom of a busy lane's traversal stack
 *                      with a copy of its ray; default 8, 0 = never).  Cuts the latency tail of every launch
 *   "refill_lanes"     idle lanes of a persistent wavefront that trigger the next ray fetch (default 32; 20 until round 4)
 *   "static_eighths"   share of a launch's rays dealt to the wavefronts statically (default 4 = 4/8; 3 until round 4)
 *   "small_waves", "small_rays_per_lane"  a traversal launch with fewer than small_rays_per_lane (default 4) rays per lane of
 *                      "traverse_waves" wavefronts uses at most small_waves (default 3072) of them
 *   "run_waves"        SCHEDULE (round 5; default 3072): most wavefronts of a launch that walks a run of instances of one mesh
 *                      (k_traverse4m) when the context has two or more batch slots: the other batch's HBM-bound kernels get on the
 *                      chip beside it (config 2: +6 % against 5120)
 *   "persist"          SCHEDULE (round 5; default 0): 1 = a batch of at least "persist_min_frames" (2) frames whose launch plan is one
 *                      mesh object per bounce with nothing in front of it (fused shade, staged samples, no ray sorting, not instrumented)
 *                      runs bounce 0's traversal as ever and then ONE launch for the traversal of bounces >= 1 and every shade pass
 *                      (k_persist: one wavefront in "persist_service_every" (5) shades tiles, the others walk; a walking wavefront
 *                      without rays shades "persist_help_tiles" (8) tiles before it looks again).  Bit-identical (tests/test_gpu_persist.py),
 *                      measured 0.58 x the per-bounce launches: off.  Its waits are bounded: a launch that gives up
 *                      makes ptc_get_stats fail with PTC_ERR_HIP instead of hanging.  Any time (queued frames are flushed first)
 *   "prefold"          SCHEDULE (round 5; default 1): when a bounce opens with a sphere run in front of a mesh launch that lists its rays (a
 *                      room's walls), the kernel that ends the bounce BEFORE walks that run for its survivors -- and ray generation for
 *                      the primary rays -- into a second set of hit records, and the bounce starts with the work list (k_list_flags)
 *                      instead of k_spheres.  Bit-identical; config 2 +8-9 %.  0: every bounce runs k_spheres.  Before ptc_resize
 *                      (33 more bytes per pixel and frame in flight)
 *   "direct_light"     RENDERING (default 0; an extension): 1 = ptc_trace under PTC_METHOD_MEGAKERNEL draws one light
 *                      sample (ptc_direct_light's, from a random stream of its own) with a shadow ray at every diffuse hit, sums the
 *                      samples' radiance along the path, and counts an emissive hit only when the vertex before it drew no sample
 *                      (the camera, metal, glass).  The expectation of every pixel is unchanged, its variance is lower wherever a lamp is
 *                      small; normal, depth and ptc_stats.rays_total (closest-hit queries) are bit for bit those of 0.  A scene without
 *                      lamps, or of total lamp weight 0, renders bit for bit as with 0; a scene with an emissive sphere that cannot be
 *                      sampled (ptc_light_table) makes ptc_trace fail with PTC_ERR_INVALID, naming the object.  Under
 *                      PTC_METHOD_STREAMING ptc_trace and ptc_trace_begin fail with PTC_ERR_INVALID while it is 1, before anything is
 *                      queued: the streaming loop does not render direct light.  Counters: ptc_get_direct_loop_stats.  Any time
 *   "environment_light" RENDERING (default 0; an extension): 1 = under PTC_METHOD_MEGAKERNEL, in a frame whose
 *                      environment (ptc_set_environment) has weight > 0, every hit on a diffuse material draws one environment sample
 *                      (ptc_environment_light's, from path_seed(pixel, iteration) ^ 0x454e564c, draws 4 b .. 4 b + 3 at bounce b) with a
 *                      shadow ray of its own, and a miss counts the environment only when the vertex before it drew no such sample (the
 *                      camera, metal, glass).  Independent of "direct_light": with both, a diffuse hit draws the lamp's sample, then the
 *                      environment's.  The expectation of every pixel is that of 0; normal, depth, rays_total, the lamps' stream and
 *                      ptc_get_direct_loop_stats are bit for bit those of the same render with 0: only colour differs.  Without an
 *                      environment, or under a map of weight 0, it renders bit for bit as with 0.  The alias table (16 n n bytes on the
 *                      device) is built by the first ptc_trace that needs it: PTC_ERR_OOM from there, the environment stays.  Under
 *                      PTC_METHOD_STREAMING ptc_trace and ptc_trace_begin fail with PTC_ERR_INVALID while it is 1, before anything is
 *                      queued.  Counters: ptc_get_environment_light_loop_stats.  Any time (queued frames are flushed first)
 *   "mis"              RENDERING (default 0; an extension): 1 = under PTC_METHOD_MEGAKERNEL, in a frame that samples the
 *                      lamps ("direct_light" with a lamp table of weight > 0), the environment ("environment_light" with a map of weight
 *                      > 0) or both, every light sample at a diffuse hit is combined with the path's own continuation ray by the balance
 *                      heuristic: the sample is weighted p_light / (p_light + cos_r / pi), and a lamp the continuation ray hits or a sky it
 *                      reaches counts with cos / pi / (cos / pi + p_light) instead of 0 (p_light: the sampler's solid-angle density of
 *                      that direction; ptc_light_material_pdf, ptc_environment_light_pdf).  Diffuse vertices only, and not at the last
 *                      bounce, whose light samples keep weight 1: the expectation of every pixel is that of 0.  Normal, depth,
 *                      rays_total, every stream and ptc_get_direct_loop_stats / ptc_get_environment_light_loop_stats are bit for bit
 *                      those of the same render with 0: only colour differs.  A frame that samples neither light renders bit for bit
 *                      as with 0.  Under PTC_METHOD_STREAMING ptc_trace and ptc_trace_begin fail with PTC_ERR_INVALID while it is 1,
 *                      before anything is queued.  Counters: ptc_get_mis_loop_stats.  Any time (queued frames are flushed first)
 *   "smooth_normals"   RENDERING (default 0; an extension): 1 = under PTC_METHOD_MEGAKERNEL, in a scene with vertex normals
 *                      (ptc_set_vertex_normals), a triangle hit is shaded with the interpolated vertex normal: the normal plane, the
 *                      material's lobes and the light samples take it, the geometric normal keeps `side` and the lamp-side terms.  A
 *                      light sample or a diffuse / metal continuation that lies behind the geometry counts as 0.  Every other
 *                      parameter combines with it.  Without vertex normals a frame launches what it launched with 0.  Under
 *                      PTC_METHOD_STREAMING ptc_trace and ptc_trace_begin fail with PTC_ERR_INVALID while it is 1, before anything is
 *                      queued.  Counters: ptc_get_smooth_loop_stats.  Any time (queued frames are flushed first)
 *   "textures"         RENDERING (default 0; an extension): 1 = under PTC_METHOD_MEGAKERNEL, in a scene with textures
 *                      (ptc_set_textures) and texture coordinates (ptc_set_texcoords), a triangle hit on a diffuse or metal material
 *                      with a texture bound takes its colour from the texel at the interpolated coordinate, times the material's
 *                      p[0..2].  Glass and emissive materials and spheres keep p.  Normal, depth and the ray count are those of the
 *                      same render with 0.  Every other parameter combines with it.  Without textures or without coordinates a
 *                      frame launches what it launched with 0.  Under PTC_METHOD_STREAMING ptc_trace and ptc_trace_begin fail with
 *                      PTC_ERR_INVALID while it is 1, before anything is queued.  Counters: ptc_get_texture_loop_stats.  Any time
 *                      (queued frames are flushed first)
 *   "normal_maps"      RENDERING (default 0; an extension): 1 = under PTC_METHOD_MEGAKERNEL, in a scene with textures,
 *                      texture coordinates and a normal-map binding (ptc_set_normal_maps), a triangle hit on a diffuse or metal material
 *                      with a map bound is shaded with the map's normal -- its material, its light samples and "mis" see it; the normal
 *                      and depth planes are those of the same render with 0 (the paths behind the hit differ).  Independent of "textures";
 *                      every other parameter combines with it.  Without textures, coordinates or a bound map a frame launches what it
 *                      launched with 0.  Under PTC_METHOD_STREAMING ptc_trace and ptc_trace_begin fail with PTC_ERR_INVALID while it is
 *                      1, before anything is queued.  Counters: ptc_get_normal_map_loop_stats.  Any time (queued frames are flushed first)
 *   "roulette"         RENDERING (default 0 = off; an extension): k in [1, 64] = Russian roulette at every bounce b >= k
 *                      except the last one, under both methods (and "direct_light").  A path whose closest hit exists and is no emitter
 *                      takes q = the largest component of the throughput that came into the bounce; q >= 1 changes nothing (no draw); else
 *                      one draw u from a random stream of its own (path_seed(slot or pixel, iteration) ^ 0x52524c54, discard(b)): u < q
 *                      divides the throughput by q and the bounce goes on as ever, otherwise the path ends with the sample (0, 0, 0) and
 *                      no material draw.  The expectation of every pixel is unchanged (the variance may rise); bounce 0 never plays, so
 *                      normal and depth are bit for bit those of 0; ptc_stats.rays_total and the live counts fall.  0, and any
 *                      k >= max_bounces - 1, launch exactly what was launched before the parameter existed.  A frame with a bounce that
 *                      plays is not eligible for "persist" (k_persist is not taught roulette): it renders through the per-bounce
 *                      launches, with the same bits.  Any time (queued frames are flushed first)
 *   "pair_batches"     SCHEDULE (round 5; default 0): 1 = a full batch is held until the next one is full (or anything else looks at
 *                      the context); the two are enqueued bounce by bounce on two slots and their traversal launches take turns.
 *                      Bit-identical, measured 6-7 % slower than the default (profiles/r05_pair_batches.txt): off.  Any time
 *   "debug_lds_entries" test hook: keep only this many of the 24 per-lane traversal stack entries in LDS, so that small
 *                      scenes exercise the global overflow area (1..24; before ptc_upload_scene)
 *   "debug_shade_epoch" test hook: the look-back launches on every frame slot's tile descriptors count on from this value
 *                      (0..2^30 - 1; the next launch takes value + 1, and after 2^30 - 1 the epochs start at 1 again, behind a
 *                      clear of the descriptors), so that a test reaches the wrap without 2^30 launches.  Any time, also after
 *                      ptc_resize; synchronises the frames in flight, as slot_offset does, and clears the descriptors
 *   "debug_force_slow" test hook: route every ray through the exact redo at the end of the traversal launch */
int ptc_set_param(ptc_ctx* ctx, const char* name, int value);

/* The thin lens (an extension: the reference's camera is a pinhole).  Two context-wide values in world units: the
 * aperture radius (default 0 = the pinhole: exactly what was launched before the lens existed) and the distance of the plane in
 * focus (default 1; read only under a radius > 0).  Under a radius > 0 the primary ray of a pixel leaves a point of the lens disk
 * -- uniform on the disk, two draws of a random stream of its own (path_seed(pixel, iteration) ^ 0x4c454e53) -- towards the point
 * the pinhole ray has at camera-space depth focus_distance; the jitter and every material draw are the pinhole render's.  Both render
 * methods and every parameter that renders a pinhole frame ("direct_light", "roulette", emitters, rows / interleave); a lens frame
 * gets no entry points ("beam"), and ptc_denoise's positions stay the pinhole ray's x depth (approximate under a lens).
 * PTC_ERR_INVALID, with the offending value in ptc_last_error and the lens left as it was: a NaN or infinite value, a negative
 * radius, a radius > 0 with focus_distance <= 0.  Any time (queued frames are flushed first: a batch renders with one lens). */
int ptc_set_lens(ptc_ctx* ctx, float lens_radius, float focus_distance);
int ptc_get_lens(ptc_ctx* ctx, float* lens_radius, float* focus_distance);

/* Environment lighting (an extension: the reference's sky is a fixed gradient).  A context-wide octahedral HDR map:
 * rgb = 3 n n floats in host memory, texel M[j][i] at rgb + 3 (j n + i), row j along z, column i along x, +y up, 2 <= n <= 4096, every
 * component finite and >= 0.  With a map set, every path that leaves the scene -- in both render methods, under every parameter --
 * ends with throughput x the map's value in its direction (a clamped bilinear fetch, continuous over the sphere; the rule, one binary32
 * operation at a time, is DESIGN section 5j's) where the gradient stands otherwise: only colour differs from the gradient's render --
 * normal, depth, live counts and rays_total are the same.  "direct_light" counts the environment at every miss and draws no light
 * sample for it.  rgb == NULL or n == 0 removes the map: exactly what was launched before it existed.  The map survives
 * ptc_upload_scene and ptc_resize.  Any time (queued frames are flushed first: a batch renders under one environment).  A frame with
 * an environment takes the per-bounce launches under "persist" 1 (the same bits).
 * PTC_ERR_INVALID (n out of range; a NaN, infinite or negative component: ptc_last_error names the texel and the component),
 * PTC_ERR_OOM (the device allocation); after any refusal the environment that was set stays in place. */
int ptc_set_environment(ptc_ctx* ctx, const float* rgb, uint32_t n);
/* *n = the size of the map that is set, 0 without one */
int ptc_get_environment(ptc_ctx* ctx, uint32_t* n);
/* The device function a miss calls, on `count` directions of the caller's (host arrays: 3 floats in, 3 floats out each; a direction
 * need not be normalised; a zero, NaN or infinite one gives 0).  PTC_ERR_INVALID without an environment.  Moves no statistics. */
int ptc_sample_environment(ptc_ctx* ctx, const float* dirs, uint32_t count, float* rgb_out);
/* Host only, no context: an equirectangular image (rgb: 3 width height floats, row 0 up, the image's centre the direction -z) to the
 * octahedral map ptc_set_environment takes (out: 3 n n floats).  Per octahedral texel centre the direction d in binary64; the image
 * sampled bilinearly, wrapping in u and clamping in v, at u = atan2(d.x, -d.z) / 2 pi + 0.5, v = acos(d.y) / pi; times scale; rounded
 * to binary32.  A point sample per texel (no filtering).  PTC_ERR_INVALID: a NULL, a zero size, n outside [2,4096], a scale that is
 * negative or not finite. */
int ptc_environment_from_equirect(const float* rgb, uint32_t width, uint32_t height, uint32_t n, float scale, float* out);

/* ---- the hot path ---- */
/* PathTracer::path_trace (path_tracer.cu:389-477): one sample per pixel, accumulated as a running
 * mean; no-op once iteration() >= max_iterations.  Asynchronous on the context's stream. */
int ptc_trace(ptc_ctx* ctx, const ptc_camera* camera);

/* The same frame in three steps, for callers that must exchange live-path counts between bounces
 * (multi-GPU row bands keep the reference's global slot numbering this way):
 *   ptc_trace_begin   = generate_rays (ray_gen.cu:63-79)
 *   ptc_trace_bounce  = intersection_kernel + material_kernel + stable_partition for bounce b
 *                       (path_tracer.cu:423-457); slot_base_dev (device pointer to ONE uint32, or
 *                       NULL for 0) is added to every local slot index before RNG seeding
 *   ptc_trace_end     = final_gathering_kernel (path_tracer.cu:460-470) + ++iteration
 * (ptc_trace_begin at iteration() == INT_MAX fails with PTC_ERR_INVALID: the counter is an int, and ptc_trace_end would overflow it)
 * ptc_live_count_dev returns the device address of the uint32 holding the number of live paths
 * entering bounce b of the current frame (valid after bounce b-1 was enqueued). */
int ptc_trace_begin(ptc_ctx* ctx, const ptc_camera* camera);
int ptc_trace_bounce(ptc_ctx* ctx, int bounce, const uint32_t* slot_base_dev);
int ptc_trace_end(ptc_ctx* ctx);
int ptc_live_count_dev(ptc_ctx* ctx, int bounce, const uint32_t** dev_ptr);
/* Enqueue a copy of that counter into a caller-owned device uint32, e.g. a torch tensor that is then all-gathered
 * over RCCL.  Only inside ptc_trace_begin .. ptc_trace_end.  Ordering: the copy runs on the frame's own stream and
 * the context's stream (ptc_set_stream, e.g. torch's current stream) is made to wait for it, so work the caller
 * enqueues there afterwards sees the value; ptc_trace_bounce in turn makes the frame's stream wait for everything
 * enqueued on the context's stream so far before it reads slot_base_dev.  No host synchronisation. */
int ptc_copy_live_count(ptc_ctx* ctx, int bounce, void* dst_dev);
/* The same value on the host (synchronises the frame's stream): the per-bounce read-back the reference does
 * after every thrust::stable_partition (path_tracer.cu:457). */
int ptc_read_live_count(ptc_ctx* ctx, int bounce, uint32_t* host_out);

/* PathTracer::denoise (path_tracer.cu:479-485) */
int ptc_denoise(ptc_ctx* ctx);

/* The albedo stage of "denoise_albedo" alone, whatever the parameter says: k_denoise_albedo on the accumulated
 * colour and the last traced camera, returned to host arrays, each of which may be NULL -- albedo_out 3 floats per pixel (the plane
 * as the parameter's text describes it), irradiance_out 3 floats per pixel (colour / e per channel), rays_out 8 floats per pixel (the
 * pixel-centre rays the kernel walked, in ptc_intersect_rays' layout: origin, t_min 1e-4, direction, t_max infinity; pinhole rays under
 * a lens too).  Pixels in row order.  The final buffer is not touched.  ptc_denoise's refusals: PTC_ERR_INVALID without a traced frame
 * and for a context that does not own the whole frame (ptc_set_rows, ptc_set_interleave).  Synchronises. */
int ptc_denoise_albedo(ptc_ctx* ctx, float* albedo_out, float* irradiance_out, float* rays_out);
/* pixels, surface_hits (pixels whose first hit is diffuse or metal), texel_lookups (those that took a texel) and floored (channels
 * whose albedo took the floor 1/64) of the last call that ran k_denoise_albedo -- ptc_denoise under "denoise_albedo" 1 with a
 * filter_size >= 1, or ptc_denoise_albedo; zeros before the first.  stage_ms: the summed duration of the stage's launches
 * (k_denoise_albedo and k_remodulate) since ptc_restart, while events are enabled (ptc_set_profiling).  Synchronises. */
typedef struct ptc_denoise_albedo_stats {
  uint64_t pixels, surface_hits, texel_lookups, floored;
  double stage_ms;
} ptc_denoise_albedo_stats;
int ptc_get_denoise_albedo_stats(ptc_ctx* ctx, ptc_denoise_albedo_stats* out);
/* The rule of section 5r on the host (no GPU, no context), a channel at a time: effective_out[i] = albedo[i] > 1/64 ? albedo[i] : 1/64
 * and irradiance_out[i] = colour[i] / effective_out[i], one binary32 operation each -- the header the kernels run.  n values in every
 * array.  PTC_ERR_INVALID: a NULL with n > 0. */
int ptc_check_demodulate(const float* colour, const float* albedo, uint32_t n, float* irradiance_out, float* effective_out);

/* sigma of "denoise_variance" (default 16, the choice of its sweep): the prefiltered variance is multiplied by it under the colour distance,
 * so two pixels of equal variance under pure noise have a mean exponent of -2 / sigma.  PTC_ERR_INVALID for a value that is not
 * finite or is <= 0; the value set before stays.  Any time. */
int ptc_set_denoise_variance(ptc_ctx* ctx, float sigma);
int ptc_get_denoise_variance(ptc_ctx* ctx, float* sigma);
/* The estimate stage of "denoise_variance" alone, whatever that parameter says, on the plane ptc_denoise would filter now (the
 * irradiance while "denoise_albedo" is 1, else the accumulated colour) with the weights set now, returned to host arrays, each of
 * which may be NULL -- variance_out one float per pixel (the estimate), prefiltered_out one float per pixel (its 3 x 3 Gaussian, what
 * the first pass divides by).  Pixels in row order.  The final buffer is not touched.  ptc_denoise's refusals: PTC_ERR_INVALID without
 * a traced frame and for a context that does not own the whole frame (ptc_set_rows, ptc_set_interleave).  Synchronises. */
int ptc_denoise_variance(ptc_ctx* ctx, float* variance_out, float* prefiltered_out);
/* pixels and floored (pixels whose first prefiltered variance is below the floor 2^-53) of the last call that ran the estimate stage
 * -- ptc_denoise under "denoise_variance" 1 with a filter_size >= 1, or ptc_denoise_variance; zeros before the first.  stage_ms: the
 * summed duration of the stage's launches (k_variance_estimate and k_variance_prefilter) since ptc_restart, while events are enabled
 * (ptc_set_profiling).  Synchronises. */
typedef struct ptc_denoise_variance_stats {
  uint64_t pixels, floored;
  double stage_ms;
} ptc_denoise_variance_stats;
int ptc_get_denoise_variance_stats(ptc_ctx* ctx, ptc_denoise_variance_stats* out);
/* The whole mode on the host (no GPU, no context) from the caller's planes, with the per-tap functions of the header the kernels
 * compile: colour and normal 3 floats per pixel, depth one, pixels in row order; the view rays of `camera` at width x height (both
 * >= 2); weights: filter_size, normal_weight and position_weight are read, color_weight is not.  variance_out (may be NULL): the
 * estimate, one float per pixel.  result_out (may be NULL): the last pass's colour, 3 floats per pixel; untouched when filter_size < 1.
 * PTC_ERR_INVALID: a NULL input, a bad size, a sigma that ptc_set_denoise_variance would refuse. */
int ptc_check_denoise_variance(const float* colour, const float* normal, const float* depth, const ptc_camera* camera, uint32_t width,
                               uint32_t height, const ptc_denoiser_params* weights, float sigma, float* variance_out, float* result_out);

/* PathTracer::send_to_preview (path_tracer.cu:487-520): tonemap to RGBA8 (4 bytes/pixel, rows of
 * this context only).  dst is a device pointer if dst_is_device != 0 (the reference always writes a
 * device/managed pointer), else host memory.  Synchronises like the reference. */
int ptc_present_rgba8(ptc_ctx* ctx, void* dst, int dst_is_device, int display_type);

/* Copy an accumulated float framebuffer (rows of this context only) as packed floats: 3 per pixel
 * for COLOR/NORMAL/FINAL (glm::vec3 layout of dev_color_buffer_ etc., path_tracer.hpp:73-81),
 * 1 per pixel for DEPTH.  Synchronises. */
int ptc_download(ptc_ctx* ctx, int which, void* dst, int dst_is_device);

/* ---- several GPUs: one process and one context per GPU, the frame's rows dealt to the ranks ---- */
/* (No reference equivalent: the reference is single-GPU.  SURVEY section 8e: the scene is replicated, every rank
 * traces its rows (ptc_set_interleave / ptc_set_rows) without talking to anyone, and radiance moves only at present
 * time, from every rank straight to the root over xGMI.)
 * The transport is HIP inter-process memory: a rank exports the device buffer that holds its packed rows
 * (ptc_band_export, once), the root maps the peers' buffers (ptc_band_import, once; the handle's geometry is checked
 * against the root's frame) and, whenever a frame is presented (ptc_gather_frame / ptc_gather_present_rgba8), ONE
 * kernel on the root reads every band where it lies -- the peers' over xGMI, all links at once -- and writes it into
 * row order; nothing is staged.  ptc_gather_last_us reports how long that launch took on the root.  The handles
 * and the "my rows are ready" signal travel over whatever channel the application has between its processes --
 * shared memory in hip_pt --gpus N (host/main.cpp), torch.distributed in bench.py and the tests:
 *     every rank but the root:  ptc_band_publish(ctx, which);   then signal / barrier
 *     the root, after that:     ptc_gather_frame(ctx, which, dst, dst_is_device)
 * Works the same when the ranks share one GPU (how it is tested on a one-GPU box). */
typedef struct ptc_band_handle {
  uint8_t ipc_mem[64];     /* hipIpcMemHandle_t of the rank's band buffer (3 floats per pixel of the band) */
  uint32_t pix_count;      /* pixels the rank renders */
  uint32_t pix_begin;      /* DBand of the rank: where its packed pixel s sits in the frame */
  uint32_t width;
  uint32_t rank, nranks, block_rows;
  uint32_t reserved[2];
} ptc_band_handle;
int ptc_band_export(ptc_ctx* ctx, ptc_band_handle* out);
int ptc_band_import(ptc_ctx* root, uint32_t rank, const ptc_band_handle* handle);
/* Pack this rank's rows of buffer `which` (ptc_buffer) into its exported band buffer and wait until they are there. */
int ptc_band_publish(ptc_ctx* ctx, int which);
/* Root: its own rows + the rows every imported rank has published -> the whole frame in row order, packed like
 * ptc_download (3 floats per pixel, 1 for PTC_BUF_DEPTH).  dst holds width*height pixels.  Synchronises. */
int ptc_gather_frame(ptc_ctx* root, int which, void* dst, int dst_is_device);
/* Root: PathTracer::send_to_preview of the gathered frame (width*height RGBA8).  display_type as ptc_present_rgba8;
 * PTC_DISPLAY_FINAL gathers the accumulated colour (a denoised buffer exists only for a context that owns the whole
 * frame). */
int ptc_gather_present_rgba8(ptc_ctx* root, void* dst, int dst_is_device, int display_type);
/* Root: device time of the most recent gather (the root's own pack excluded: from the first to the last band landing
 * in row order), in microseconds.  Waits for that gather. */
int ptc_gather_last_us(ptc_ctx* root, float* microseconds);

/* ---- the display transform (an extension: the reference shows clamp + gamma only) ---- */
/* Context-wide, applied where radiance is shown: ptc_present_rgba8 and ptc_gather_present_rgba8 under PTC_DISPLAY_FINAL and
 * PTC_DISPLAY_COLOR (the normal and depth views are never touched).  Three steps: meter (optional) -- a 256-bin log-luminance
 * histogram of the shown buffer, on the device, whose trimmed mean gives an exposure factor; curve -- every channel times that factor,
 * then through the tone curve; encode -- send_to_preview's lines, unchanged (gamma 1 / 2.2, clamp, * 255.99f, alpha 255).
 * The rule, in binary32 and integers (DESIGN section 5m states it operation by operation; tests/display_ref.py restates it):
 *   meter   Y = (0.2126f r + 0.7152f g) + 0.0722f b.  Y negative or not finite (a NaN in any channel): `rejected`.  Y < 2^-16 (zeros,
 *           denormals): `below`.  Else bin = min((bits(Y) >> 20) - 888, 255): eight bins an octave from 2^-16, bin 128 at 1.0.
 *   level   N = the counted samples; the first N low_permille / 1000 and the last N (1000 - high_permille) / 1000 of them in bin order
 *           are left out (floored); K, S = the count and the bin sum of the others; level_bin = (2 S + K) / (2 K);
 *           level = that bin's lower edge; scale = (key / level) * exposure.  N == 0: level_bin -1, level 0, scale = exposure.
 *           metering 0: scale = exposure, and nothing is metered.
 *   curve   e = c * scale; x = e > 0 ? e : 0 (a NaN or a negative shows black); x = min(x, 2^20);
 *           CLAMP y = x;  REINHARD y = (x (1 + x / white^2)) / (1 + x);  ACES y = (x (2.51 x + 0.03)) / (x (2.43 x + 0.59) + 0.14).
 * The reference display -- curve CLAMP, metering 0, exposure 1.0f, the default -- launches exactly what was launched before the
 * display existed (the other fields are not read). */
typedef enum ptc_curve { PTC_CURVE_CLAMP = 0, PTC_CURVE_REINHARD = 1, PTC_CURVE_ACES = 2 } ptc_curve;
typedef struct ptc_display_params {   /* (ptc_display is the enum of the views) */
  int32_t curve;                      /* ptc_curve */
  int32_t metering;                   /* 0 manual, 1 histogram */
  float exposure;                     /* linear factor; finite and > 0; default 1 */
  float key;                          /* what the metered level is mapped to; finite and > 0; default 0.18f */
  float white;                        /* Reinhard's white point; finite and > 0; default 4 */
  uint32_t low_permille, high_permille; /* the trimmed mean keeps the ranks between them; low < high <= 1000; defaults 50, 950 */
} ptc_display_params;
typedef struct ptc_exposure_info {
  uint32_t pixels;                    /* pixels shown */
  uint32_t counted, below, rejected;  /* pixels = counted + below + rejected under metering 1; all three 0 under metering 0 */
  int32_t level_bin;                  /* -1: nothing was counted, or metering 0 */
  float level;                        /* lower edge of level_bin; 0 where level_bin is -1 */
  float scale;                        /* the factor every channel was multiplied by */
  uint32_t histogram[256];
} ptc_exposure_info;
/* Any time; the display survives ptc_upload_scene and ptc_resize.  PTC_ERR_INVALID, with the offending field named in ptc_last_error
 * and the display that was set left in place: a NaN, infinite or non-positive exposure, key or white; permilles out of order; an
 * unknown curve; a metering other than 0 or 1. */
int ptc_set_display(ptc_ctx* ctx, const ptc_display_params* display);
int ptc_get_display(ptc_ctx* ctx, ptc_display_params* out);
/* Of the most recent present (ptc_present_rgba8, ptc_gather_present_rgba8) that went through the display transform.
 * ptc_present_rgba8 meters the rows of this context -- a non-root rank's own present meters only its rows --,
 * ptc_gather_present_rgba8 the whole gathered frame on the root.  PTC_ERR_INVALID before any such present. */
int ptc_get_exposure_info(ptc_ctx* ctx, ptc_exposure_info* out);
/* The same kernels on a caller's buffer under the context's display (the reference display included): src = pix_count pixels of
 * `channels` floats, 3 (packed) or 4 (the fourth is ignored; a device pointer must be 16-byte aligned), in device memory if
 * src_on_device != 0; rgba_out (4 bytes a pixel) and mapped_out (optional: the channels after the curve, 3 floats a pixel) in
 * device memory if out_on_device != 0; info (optional, host memory).  Needs neither a scene nor a frame, moves no render statistics
 * and leaves ptc_get_exposure_info's answer alone.  Synchronises. */
int ptc_tonemap_buffer(ptc_ctx* ctx, const void* src, int channels, uint32_t pix_count, int src_on_device, void* rgba_out, float* mapped_out,
                       int out_on_device, ptc_exposure_info* info);
/* The rule on the host, no GPU and no context (pt_display.hpp compiled for the host): the metering of count pixels of `channels`
 * (3 or 4) floats under params, and the curve of params on every pixel under a given scale (mapped_out: 3 floats a pixel).
 * PTC_ERR_INVALID: a NULL, channels, params ptc_set_display would refuse. */
/* ptc_set_display's decision on params: PTC_OK, or PTC_ERR_INVALID with the refusal's text -- it names the field -- in why (may be
 * NULL; capacity bytes, always terminated). */
int ptc_check_display_params(const ptc_display_params* params, char* why, uint32_t capacity);
int ptc_check_display_meter(const ptc_display_params* params, const float* rgb, int channels, uint32_t count, ptc_exposure_info* info_out);
int ptc_check_display_map(const ptc_display_params* params, float scale, const float* rgb, int channels, uint32_t count, float* mapped_out);

int ptc_synchronize(ptc_ctx* ctx);                                  /* cudaDeviceSynchronize at cli.cpp:100 */
int ptc_get_stats(ptc_ctx* ctx, ptc_stats* out);                    /* synchronises */
int ptc_set_profiling(ptc_ctx* ctx, int time_trace_kernel, int count_tests);
int ptc_reset_profile(ptc_ctx* ctx);
int ptc_get_profile(ptc_ctx* ctx, ptc_profile* out);                /* synchronises */

/* ---- pieces exposed for parity tests and for host-side callers ---- */
/* intersection_kernel alone (path_tracer.cu:271-290) on caller-supplied rays (host arrays of
 * 8 floats: origin, t_min, direction, t_max = struct Ray, ray.hpp:8-20).  Outputs (host):
 * hit_t[n] (t, or -1 on miss), hit_normal[3n], hit_material[n], hit_side[n]. */
int ptc_intersect_rays(ptc_ctx* ctx, const float* rays, uint32_t n, float* hit_t, float* hit_normal,
                       uint32_t* hit_material, uint8_t* hit_side);

/* The primary rays of `iteration` for every slot of the context in slot order -- all pixels, or this context's under ptc_set_rows /
 * ptc_set_interleave -- as the frame's ray generation builds them for `camera` under the context's lens (ptc_set_lens): the same
 * device function.  rays_out (host): 8 floats per ray, origin, t_min, direction, t_max -- what ptc_intersect_rays,
 * ptc_occluded_rays and ptc_direct_light's shadow rays take; capacity_floats >= 8 x the context's pixels.  After ptc_resize;
 * synchronises; moves neither ptc_stats nor the iteration counter. */
int ptc_generate_rays(ptc_ctx* ctx, const ptc_camera* camera, uint32_t iteration, float* rays_out, uint64_t capacity_floats);

/* Occlusion queries (an extension: the reference has no any-hit query).  occluded[i] = 1 iff ray_scene_intersection_test
 * (path_tracer.cu:110-128) reports a hit for ray i, else 0 -- the reference's own arithmetic and corners: world box by
 * ray_aabb first, spheres in object space against the carried t_max, triangles accept t_min <= t <= t_max, a triangle counts
 * only if every inner ancestor's box passes.  Emissive surfaces occlude like any other.  Rays as for ptc_intersect_rays (host,
 * 8 floats each); occluded: n bytes (host).  Rays with t_min 1e-4f or 1e-5f and t_max >= 0 under trace variant 3 take the
 * any-hit kernels (k_occlude_spheres, k_occlude4: the walk stops at the first hit); any other ray, or trace variant 0 / 1,
 * sends the whole call through the exact closest-hit kernel of ptc_intersect_rays (the reference-order one when a t_max is
 * NaN: the reference's test rejects on t > t_max, so it accepts).  Moves neither ptc_stats nor ptc_profile. */
int ptc_occluded_rays(ptc_ctx* ctx, const float* rays, uint32_t n, uint8_t* occluded);
/* Since ptc_reset_profile / create: rays asked, rays found occluded, rays the any-hit launches redid with exact box decisions,
 * device time of the kernels (HIP events; only while ptc_set_profiling has timing on, else 0), kernel launches. */
typedef struct ptc_occlusion_stats {
  uint64_t rays, occluded, redone;
  double kernel_ms;
  uint32_t launches;
} ptc_occlusion_stats;
int ptc_get_occlusion_stats(ptc_ctx* ctx, ptc_occlusion_stats* out);

/* Direct-light queries (an extension: the reference has no emitters).
 * The lamp table of a scene: one record per primitive of every object whose material is emissive (type 3) -- emissive objects
 * in object-list order, the triangles of a mesh object in index order, two instances of one mesh as two sets of records. */
typedef struct ptc_light {           /* one lamp primitive, 64 bytes, world space */
  float p0[3], e1[3], e2[3], n[3];   /* triangle: transform_point(M, v0), p1 - p0, p2 - p0, normalize(cross(e1, e2)) -- the operations of
                                        DScene::tris;  sphere: p0 = transform_point(M, centre), e1[0] = world radius = length of M's
                                        column 0 (binary32, glm order) * radius, the rest 0 */
  float cdf;                         /* (float)(sum of the weights up to and including this record / W); the last record with a
                                        weight > 0 and every record behind it: exactly 1.0f.  Informational: no sample reads it */
  float inv_pdf;                     /* 1 / (area density of a sample on this primitive) = (float)(W / lum), 0 when lum == 0 */
  uint32_t object;                   /* index into ptc_scene_desc::objects */
  uint32_t kind_material;            /* material index | kind << 31  (kind 0 triangle, 1 sphere) */
} ptc_light;
/* weight of a record = area * lum in binary64 from the record's own binary32 fields: area = 0.5 |e1 x e2| or 4 pi R^2,
 * lum = max(r, g, b) of the material's emission; W = the weights summed in table order.  A sample picks its record from the RAW
 * first draw v of its stream (1 .. 2^31 - 2), in integers: with n = v - 1 in [0, N), N = 2^31 - 2,
 *   k = min(#{j : T_j <= n}, last record with a weight > 0),
 * T_k = round(run_k / W * N) in binary64 from the same running sums, then raised to at least T_(k-1) + 1 for a record of weight > 0 and
 * capped so that the records of weight > 0 behind it keep a state each; a record of weight 0 has T_k = T_(k-1), the last record with
 * a weight > 0 and every record behind it N.  Record k so owns T_k - T_(k-1) of the N states: none for a weight of 0, at least one for
 * any weight > 0, and within 1 + m of its share w_k / W * N (m = the records of weight > 0 whose share is below one state).  More than N
 * records of weight > 0: PTC_ERR_INVALID.  (The binary32 cdf is no part of this: near 1 it has a step of 2^-24, under which a small
 * lamp beside a large one was never picked, or many times too often.) */
typedef struct ptc_light_info {
  uint32_t lights, sphere_lights, triangle_lights, emissive_objects;
  double total_area, total_weight;
} ptc_light_info;
/* Host-side, no GPU needed: the table of `scene` into out[capacity]; info may be NULL.  Returns the number of records (0: no
 * lamps) or a negative ptc_status: PTC_ERR_INVALID for NULL arguments, a scene ptc_upload_scene would refuse, a capacity that
 * is too small, and an emissive SPHERE whose matrix is no similarity -- a sphere lamp is sampled uniformly in object space,
 * which is uniform in area only if the columns of the upper 3 x 3 are pairwise orthogonal and of equal length (both to 1e-5
 * relative) and the bottom row is (0, 0, 0, 1); the message (ptc_last_error(NULL)) names the object.  Mesh lamps take any
 * matrix.  Such a scene still uploads and renders; only this call and ptc_direct_light refuse it. */
int ptc_light_table(const ptc_scene_desc* scene, ptc_light* out, uint32_t capacity, ptc_light_info* info);
int ptc_get_light_info(ptc_ctx* ctx, ptc_light_info* out);    /* of the uploaded scene (zeros while its lamps cannot be sampled) */

/* radiance[3i..] = radiance leaving a white Lambertian surface at points[i] with unit normal normals[i] by ONE light sample:
 *   Le * cos_r * cos_l * inv_pdf / (pi * d^2) if the shadow ray is free, else 0
 * with w = (q - p) / d, cos_r = dot(n, w) (<= 0: no sample), cos_l = |dot(n_l, w)| (lamps are two-sided, as in the path
 * tracer; a sphere lamp's far side is hidden by the lamp itself -- the shadow ray decides, not a special case).
 * Shadow ray: origin p, t_min 1e-4f, direction w, t_max = d * 0.999f (the any-hit walk's fast domain).
 * Draws: Minstd seeded from path_seed(i, sample_index) xor 0x4c495445 (no render path xors its seed); the raw first draw picks the lamp, u1, u2
 * the point (triangle: b1 = 1 - sqrt(u1), b2 = u2 * sqrt(u1), q = p0 + b1 e1 + b2 e2; sphere: z = 1 - 2 u1,
 * r = sqrt(max(0, 1 - z^2)), phi = 2 pi u2 through det_sincos, q = transform_point(M, c + R * dir), n_l = normalize(q - world
 * centre)).  The binary32 operation order: DESIGN section 5f.
 * A sample with cos_r <= 0, d == 0 (or not finite), a picked lamp of weight 0, or no lamps: radiance 0, visible 0,
 * ray = {p, 1e-4f, 0, 0, 0, 0}.
 * shadow_rays (8 floats per point, as ptc_intersect_rays takes them) and visible (1 byte per point) may be NULL.
 * on_device != 0: every pointer is a device pointer (a torch tensor); the call synchronises like ptc_download.
 * Under trace variant 0 / 1 the generated rays go through the exact closest-hit kernel, as in ptc_occluded_rays.
 * A scene without lamps (or of total weight 0) gives zeros and launches nothing; a scene with an emissive sphere that cannot
 * be sampled (ptc_light_table) fails with PTC_ERR_INVALID.
 * Finite points and unit normals are the contract; moves neither ptc_stats nor ptc_profile nor ptc_occlusion_stats. */
int ptc_direct_light(ptc_ctx* ctx, const float* points, const float* normals, uint32_t n, uint32_t sample_index,
                     float* radiance, float* shadow_rays, uint8_t* visible, int on_device);
/* Since ptc_reset_profile / create: points asked, samples that produced a shadow ray (points - culled), samples that arrived,
 * device time of the kernels -- k_light_sample, the occlusion launches, k_light_resolve -- (HIP events; only while
 * ptc_set_profiling has timing on, else 0), kernel launches. */
typedef struct ptc_direct_stats {
  uint64_t points, sampled, unoccluded;
  double kernel_ms;
  uint32_t launches;
} ptc_direct_stats;
int ptc_get_direct_stats(ptc_ctx* ctx, ptc_direct_stats* out);

/* The direct-lit megakernel ("direct_light" 1) since ptc_restart: hits on a diffuse material (each one draws a
 * light sample), shadow rays traced (the samples that were not culled) and the shadow rays that arrived (their contribution was
 * added).  Synchronises.  Zeros while nothing direct-lit has been traced since ptc_restart.  Moves none of ptc_stats, ptc_profile,
 * ptc_occlusion_stats and ptc_direct_stats, and nothing moves it but ptc_trace and ptc_restart. */
typedef struct ptc_direct_loop_stats {
  uint64_t diffuse_hits, shadow_rays, unoccluded;
} ptc_direct_loop_stats;
int ptc_get_direct_loop_stats(ptc_ctx* ctx, ptc_direct_loop_stats* out);

/* The environment as a light (an extension).  radiance[3i..] = radiance leaving a white Lambertian surface at
 * points[i] with unit normal normals[i] by ONE sample of the context's environment (ptc_set_environment):
 *   L(w) * cos_r * 4 f |w|_1^3 / pi if the shadow ray is free, else 0
 * The distribution is piecewise constant over the n x n texel squares of the octahedral unit square, proportional to the largest
 * channel of the lookup's integral over the square times |w_c|_1^3 at its centre (the solid angle: d omega = 4 |w|_1^3 ds_x ds_z);
 * an alias table of one 16-byte entry per square, {q, alias, f, f of the alias} with f = 1 / (P n^2), built in binary64 on the host.
 * Draws: Minstd seeded from path_seed(i, sample_index) xor 0x454e564c; a raw value v picks the entry ((v - 1) n^2) >> 31, u1 < q keeps
 * its square (else the alias), u2, u3 the point in the square; the point is decoded to the unit direction w (the inverse of the lookup's
 * octahedral map), cos_r = dot(n, w) (<= 0: no sample), L = the lookup a miss makes.  The binary32 operation order: DESIGN section 5k.
 * Shadow ray: origin p, t_min 1e-4f, direction w, t_max FLT_MAX.  A culled sample: radiance 0, visible 0, ray = {p, 1e-4f, 0, 0, 0, 0}.
 * Arrays, on_device, the trace variants and the statistics it leaves alone: as ptc_direct_light.  The table (16 n n bytes on the device)
 * is built by the first call that needs it and kept until the map changes: PTC_ERR_OOM if it cannot be allocated (the environment
 * stays).  PTC_ERR_INVALID without an environment; a map of weight 0 gives zeros and launches nothing. */
int ptc_environment_light(ptc_ctx* ctx, const float* points, const float* normals, uint32_t n, uint32_t sample_index,
                          float* radiance, float* shadow_rays, uint8_t* visible, int on_device);
/* ptc_direct_stats' five fields for ptc_environment_light since ptc_reset_profile / create (the kernels: k_env_light_sample, the
 * occlusion launches, k_light_resolve). */
typedef ptc_direct_stats ptc_environment_light_stats;
int ptc_get_environment_light_stats(ptc_ctx* ctx, ptc_environment_light_stats* out);
/* The megakernel under "environment_light" 1 since ptc_restart: hits on a diffuse material that drew an environment sample, its shadow
 * rays traced (the samples that were not culled) and those that arrived.  Synchronises.  Moves nothing else, ptc_get_direct_loop_stats
 * included, and nothing moves it but ptc_trace and ptc_restart. */
typedef struct ptc_environment_light_loop_stats {
  uint64_t diffuse_hits, shadow_rays, unoccluded;
} ptc_environment_light_loop_stats;
int ptc_get_environment_light_loop_stats(ptc_ctx* ctx, ptc_environment_light_loop_stats* out);

/* Multiple importance sampling ("mis", an extension).
 * The environment sample's density with respect to solid angle in `count` UNIT directions dirs[3i..] (the density is that of the
 * direction as given; nothing is normalised): 1 / (4 f |w|_1^3) with f = 1 / (P n^2) of the texel square the direction falls in
 * (s = q 0.5 + 0.5 per axis of the lookup's octahedral point q, i = min(floor(s n), n - 1), k = j n + i), read from the square's own
 * entry of the alias table; 0 in a square of weight 0 and for a zero, NaN or infinite direction.  For ptc_environment_light's sample in
 * direction w it is the reciprocal of the factor 4 f |w|_1^3 of that sample.  on_device: dirs and pdf_out are device pointers.  The
 * table is built by the first call that needs it, as ptc_environment_light does.  PTC_ERR_INVALID without an environment; a map of weight 0
 * gives zeros and launches nothing.  Moves no statistics. */
int ptc_environment_light_pdf(ptc_ctx* ctx, const float* dirs, uint32_t count, float* pdf_out, int on_device);
/* Per material of `scene` the inv_pdf every lamp record (ptc_light_table) of that material carries, (float)(W / lum): the reciprocal
 * of the lamp sampler's density per unit area on that material's surfaces.  0 for a material that is not emissive, for lum == 0 and in
 * a scene whose lamp table has weight 0.  Host only, no GPU, no context.  -> the number of materials, or PTC_ERR_INVALID (a NULL, a
 * capacity below material_count, ptc_light_table's refusals). */
int ptc_light_material_pdf(const ptc_scene_desc* scene, float* out, uint32_t capacity);
/* The megakernel under "mis" 1 since ptc_restart: emitter hits and misses behind a diffuse vertex that counted with the continuation
 * ray's weight.  Synchronises.  Moves nothing else, and nothing moves it but ptc_trace and ptc_restart. */
typedef struct ptc_mis_loop_stats {
  uint64_t weighted_emitter_hits, weighted_misses;
} ptc_mis_loop_stats;
int ptc_get_mis_loop_stats(ptc_ctx* ctx, ptc_mis_loop_stats* out);

/* Smooth shading ("smooth_normals", an extension: the reference shades every triangle with its face normal).
 *
 * ptc_set_vertex_normals: three floats per vertex, parallel to the uploaded scene's `positions` and covering the whole scene -- a mesh
 * of a mesh table finds its normals at first_vertex, as its positions do.  Object space; they need not be unit length.  NULL / 0
 * removes them.  PTC_ERR_NO_SCENE without a scene, PTC_ERR_INVALID (with a message) when vertex_count differs from the scene's or
 * exactly one of the two arguments is NULL / 0; a refusal leaves what was set in place.  The device copy belongs to the scene:
 * ptc_upload_scene releases it with the scene, and a new scene starts without normals; ptc_resize and the context's settings do not
 * touch it.  Queued frames are traced first. */
int ptc_set_vertex_normals(ptc_ctx* ctx, const float* normals, uint32_t vertex_count);
/* 1 and *vertex_count (may be NULL) = the scene's vertex count while normals are set; 0 and *vertex_count = 0 when none are. */
int ptc_get_vertex_normals(const ptc_ctx* ctx, uint32_t* vertex_count);
/* Area-weighted vertex normals of ONE mesh, on the host (no GPU, no context): triangles in index order, c = cross(p1 - p0, p2 - p0)
 * added to the sums of corners 0, 1, 2 in that order, binary32, nothing contracted; then every sum s with 0 < dot(s, s) <= FLT_MAX
 * becomes normalize(s) and every other one -- zero, not finite, a vertex no triangle uses -- (0, 0, 0).  The order is serial and
 * fixed (tests/smooth_ref.py restates it bit for bit); there is no device version, whose float atomics would make the sums depend on
 * scheduling.  normals_out: 3 vertex_count floats.  PTC_ERR_INVALID: a NULL, index_count no multiple of 3, an index out of range. */
int ptc_compute_vertex_normals(const float* positions, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count, float* normals_out);
/* The closest hit's primitive and its attributes, for callers that interpolate attributes of their own.  rays: 8 floats a ray, as for
 * ptc_intersect_rays.  Per ray: object_out = the object's index, 0xffffffff on a miss; triangle_out = the triangle of its mesh (the
 * offset of its first index / 3), 0xffffffff for a sphere and on a miss; uv_out = the accepted triangle test's u, v (vertex 1's and
 * vertex 2's weights; 0, 0 otherwise); normal_out (3 floats) = the shading normal of section 5n where vertex normals are set and a
 * triangle was hit, else the geometric normal facing the ray, zeros on a miss.  Host pointers.  One thread per ray walks the
 * reference's tree in the reference's order (an equal t is accepted: within a mesh the triangle visited last wins, across objects the
 * later one): it names the winner the render loops' own walks find, and makes no claim about speed. */
int ptc_hit_attributes(ptc_ctx* ctx, const float* rays, uint32_t n, uint32_t* object_out, uint32_t* triangle_out, float* uv_out, float* normal_out);
/* The megakernel under "smooth_normals" 1 with vertex normals set, since ptc_restart: triangle hits whose shading normal was the
 * interpolated one, those that fell back to the geometric normal, paths ended because the new direction entered the geometry, light
 * samples culled because theirs did.  Synchronises.  Moves nothing else, and nothing moves it but ptc_trace and ptc_restart. */
typedef struct ptc_smooth_loop_stats {
  uint64_t shading_normals, fallbacks, absorbed, culled_light_samples;
} ptc_smooth_loop_stats;
int ptc_get_smooth_loop_stats(ptc_ctx* ctx, ptc_smooth_loop_stats* out);

/* Image textures ("textures", an extension: the reference's materials have one constant colour).
 *
 * A texture: width x height texels of four bytes, r g b a (alpha is carried and ignored), row 0 first, and row 0 is t = 0 -- the
 * BOTTOM of the picture in OBJ's convention: a file reader flips rows, the core never does.  Each side 1 .. 4096.  encoding: how a
 * byte becomes a float (ptc_texture_decode_table); filter and wrap: the lookup's (section 5o), wrap on both axes. */
enum { PTC_TEXTURE_LINEAR = 0, PTC_TEXTURE_SRGB = 1 };
enum { PTC_TEXTURE_NEAREST = 0, PTC_TEXTURE_BILINEAR = 1 };
enum { PTC_TEXTURE_REPEAT = 0, PTC_TEXTURE_CLAMP = 1 };
typedef struct ptc_texture_desc {
  const uint8_t* rgba8;
  uint32_t width, height;
  uint32_t encoding;
  uint32_t filter;
  uint32_t wrap;
} ptc_texture_desc;
/* ptc_set_textures: the scene's textures and, per material of the uploaded scene, -1 or the texture bound to it
 * (material_texture[m], material_count entries).  textures NULL / texture_count 0 removes everything (material_texture is not read).
 * PTC_ERR_NO_SCENE without a scene; PTC_ERR_INVALID (with a message) for a material_count other than the scene's, a binding out of
 * range, a side outside 1 .. 4096, a NULL texel pointer, an enum value out of range, a pool above 1 GiB; a refusal leaves what was
 * set in place.  The texels are copied: one device allocation of the scene's holds every texture back to back.  The copy belongs
 * to the scene: ptc_upload_scene releases it with the scene, and a new scene starts without textures; ptc_resize and the
 * context's settings do not touch it.  A binding on a glass or an emissive material is accepted and ignored.  Queued frames are
 * traced first. */
int ptc_set_textures(ptc_ctx* ctx, const ptc_texture_desc* textures, uint32_t texture_count, const int32_t* material_texture,
                     uint32_t material_count);
/* 1, *texture_count and *texel_count (the pool's texels; either may be NULL) while textures are set; 0 and zeros when none are. */
int ptc_get_textures(const ptc_ctx* ctx, uint32_t* texture_count, uint64_t* texel_count);
/* ptc_set_texcoords: two floats (s, t) per triangle CORNER, parallel to the uploaded scene's `indices` and covering the whole scene --
 * a mesh of a mesh table finds its corners at first_index, as its indices do.  Per corner and not per vertex: a seam needs no split
 * vertices, and positions, indices and BVH stay the caller's.  Any float is accepted (a hit whose interpolated coordinate is not
 * finite keeps the material's colour).  NULL / 0 removes them.  Refusals and lifetime as ptc_set_vertex_normals', with index_count
 * in vertex_count's place. */
int ptc_set_texcoords(ptc_ctx* ctx, const float* st, uint32_t index_count);
/* 1 and *index_count (may be NULL) = the scene's index count while coordinates are set; 0 and *index_count = 0 when none are. */
int ptc_get_texcoords(const ptc_ctx* ctx, uint32_t* index_count);
/* The decode table of an encoding, on the host (no GPU, no context): out[k] for a byte k.  Linear: (float)k / 255.0f, one binary32
 * division.  sRGB: the piecewise sRGB curve (c / 12.92 up to 0.04045, ((c + 0.055) / 1.055)^2.4 above) evaluated in double and
 * rounded once.  The device decodes by loading from a copy of these tables.  PTC_ERR_INVALID: a NULL, an unknown encoding. */
int ptc_texture_decode_table(uint32_t encoding, float* out256);
/* The lookup of section 5o (steps 2 .. 7) on the device, without rendering: k_texture_sample, one thread per pair.  texture: an index
 * into what ptc_set_textures set; st: 2 n floats; rgb_out: 3 n floats, zeros where the rule refuses the pair (a NaN or an infinity);
 * rejected_out (may be NULL): one byte a pair, 1 where it did.  Host pointers.  PTC_ERR_INVALID without textures or for an index
 * out of range. */
int ptc_sample_texture(ptc_ctx* ctx, uint32_t texture, const float* st, uint32_t n, float* rgb_out, uint8_t* rejected_out);
/* Per ray (8 floats, as for ptc_intersect_rays) at the closest hit: st_out (2 floats) = the interpolated texture coordinate of a
 * triangle hit while coordinates are set (zeros for a sphere, on a miss and without coordinates); albedo_out (3 floats) = the colour
 * the megakernel's loop would shade with there under "textures" 1 -- texel x p[0..2] where the rule applies (textures and coordinates
 * set, a triangle, a diffuse or metal material with a binding, a finite coordinate), else the material's p[0..2]; zeros on a miss.
 * ptc_hit_attributes' walk, one thread per ray; host pointers. */
int ptc_hit_surface(ptc_ctx* ctx, const float* rays, uint32_t n, float* st_out, float* albedo_out);
/* The megakernel under "textures" 1 with textures and coordinates set, since ptc_restart: texel lookups made (one per textured hit
 * that reached evaluate_material, whatever the filter), and hits that fell back to the material's colour because the interpolated
 * coordinate was not finite.  Synchronises.  Moves nothing else, and nothing moves it but ptc_trace and ptc_restart. */
typedef struct ptc_texture_loop_stats {
  uint64_t lookups, fallbacks;
} ptc_texture_loop_stats;
int ptc_get_texture_loop_stats(ptc_ctx* ctx, ptc_texture_loop_stats* out);

/* Normal maps ("normal_maps", an extension): a texture of the pool read as a tangent-space normal at a triangle hit
 * on a diffuse or metal material, in the frame the corners' texture coordinates span, about the hit's base normal (the interpolated
 * vertex normal under "smooth_normals", else the geometric one).
 *
 * ptc_set_normal_maps: per material of the uploaded scene -1 or an index into the pool ptc_set_textures set (material_count
 * entries).  NULL / 0 removes the binding.  PTC_ERR_NO_SCENE without a scene; PTC_ERR_INVALID (with a message) without textures, for a
 * material_count other than the scene's, for an index out of range; a refusal leaves what was set.  The binding belongs to the scene
 * as the textures do, and a successful ptc_set_textures removes it: its indices named the old pool.  A texture bound as a normal map
 * is decoded with ptc_normal_map_decode_table's table whatever its encoding says; its filter and wrap hold.  A binding on a glass or
 * an emissive material is accepted and ignored.  Queued frames are traced first. */
int ptc_set_normal_maps(ptc_ctx* ctx, const int32_t* material_normal_map, uint32_t material_count);
/* 1 and *bound_materials (may be NULL) = the materials with a map while a binding is set; 0 and 0 when none is. */
int ptc_get_normal_maps(const ptc_ctx* ctx, uint32_t* bound_materials);
/* The normal maps' decode table, on the host (no GPU, no context): out[k] = max(((float)k - 128.0f) / 127.0f, -1.0f) -- byte 128 is
 * exactly 0, byte 255 exactly 1, bytes 0 and 1 are -1.  PTC_ERR_INVALID: a NULL. */
int ptc_normal_map_decode_table(float* out256);
/* Per ray (8 floats, as for ptc_intersect_rays) at the closest hit: normal_out (3 floats) = the normal the megakernel's loop would hand
 * its material there from what is SET (vertex normals if set, the normal map if bound, textures and coordinates set), whatever the
 * parameters say -- as ptc_hit_surface reports; outcome_out (one byte): 0 a miss (normal zeros), 1 no map applied (a sphere, an unbound
 * material, glass, an emitter, nothing set), 2 bent, 3 flat (the texel is (0, 0, > 0): the base normal's bits), 4 kept (the rule fell
 * back to the base normal).  ptc_hit_attributes' walk, one thread per ray; host pointers. */
int ptc_hit_shading_normal(ptc_ctx* ctx, const float* rays, uint32_t n, float* normal_out, uint8_t* outcome_out);
/* The megakernel under "normal_maps" 1 with a binding, textures and coordinates set, since ptc_restart: hits whose normal the map
 * replaced, and hits where the rule fell back to the base normal; a flat texel counts in neither.  Synchronises. */
typedef struct ptc_normal_map_loop_stats {
  uint64_t bent, kept;
} ptc_normal_map_loop_stats;
int ptc_get_normal_map_loop_stats(ptc_ctx* ctx, ptc_normal_map_loop_stats* out);

/* Where the time of the last ptc_upload_scene went (milliseconds of host wall clock; the "Initialization" stage of
 * the reference's Stopwatch, cli.cpp): */
typedef struct ptc_upload_times {
  float bvh_build_ms;   /* the reference BVH (0 when the caller brought one) */
  float layout_ms;      /* collapsed / quantised traversal trees derived from it */
  float triangles_ms;   /* per-instance world-space triangle records */
  float copy_ms;        /* hipMalloc + host-to-device copies (includes packing the reference nodes) */
  float total_ms;
  uint32_t bvh_on_device; /* 1: the reference BVH was built by the GPU builder */
  uint32_t layout_on_device; /* 1: the traversal trees and triangle records were derived on the GPU */
} ptc_upload_times;
int ptc_get_upload_times(const ptc_ctx* ctx, ptc_upload_times* out);
/* The device-resident traversal data of the uploaded scene, for inspection and tests: which = 0 four-wide nodes
 * (64 B each), 1 parent boxes per triangle rank, 2 per-instance triangle records (64 B each), 3 two-child records, 4 the reference
 * nodes as two float4.  *bytes (may be NULL) gets the size; host may be NULL to ask for the size only. */
int ptc_download_layout(ptc_ctx* ctx, int which, void* host, uint64_t capacity, uint64_t* bytes);

/* bvh_from_mesh (accelerators/bvh.cpp:211-253), host-side, no GPU needed.  nodes must hold
 * index_count/3*2-1 entries.  Returns the node count (>0) or a negative ptc_status: PTC_ERR_INVALID for an index out of
 * range or a NaN or infinite coordinate in a vertex that a triangle uses (unused vertices may hold anything; the
 * reference's builder indexes out of bounds or panics on such a mesh), PTC_ERR_BVH for a node of more than 4 coincident centroids. */
int ptc_build_bvh(const float* positions, uint32_t vertex_count, const uint32_t* indices,
                  uint32_t index_count, ptc_bvh_node* nodes, uint32_t* max_depth);
/* The same tree built by the context's GPU (pt_bvh_gpu.hip: all nodes of a depth split at once; the decisions are
 * the host builder's, from one source) -- node for node what ptc_build_bvh returns.  This is what ptc_upload_scene
 * runs when the scene brings no BVH (param "bvh_build_on_device", default 1; 0 = the host builder).  The same
 * refusals, too: a vertex in use that is not finite is PTC_ERR_INVALID here as well (the message names the vertex), checked
 * on the host before anything goes to the device. */
int ptc_build_bvh_device(ptc_ctx* ctx, const float* positions, uint32_t vertex_count, const uint32_t* indices,
                         uint32_t index_count, ptc_bvh_node* nodes, uint32_t* max_depth);

/* Per-object part of SceneDescription::build_scene (scene_description.cpp:17-52): fills inv_m
 * (glm::inverse) and the world AABB.  sphere / mesh_aabb6 (min xyz, max xyz) as the type needs. */
int ptc_make_object(uint32_t type, uint32_t index, const float* m16, const ptc_sphere* sphere,
                    const float* mesh_aabb6, ptc_object* out);

/* Host-side check of the traversal layouts derived from a reference BVH (no GPU needed): builds the collapsed
 * four-wide tree with its 64-byte quantised nodes and verifies, in double precision, that every quantised child
 * box contains the exact box of the reference node it stands for, that every reference leaf is reachable exactly
 * once, and that each triangle's recorded parent box is its reference parent's.  Returns the number of
 * violations (0 = sound), or a negative ptc_status; *checked_boxes (may be NULL) gets the number of child boxes
 * looked at. */
int ptc_check_traversal_layout(const ptc_bvh_node* nodes, uint32_t node_count, uint64_t* checked_boxes);
/* The ray feed of the persistent traversal launches, checked on the host (no GPU; test hook): a frame of n rays dealt in
 * eight regions, static_eighths / 8 of every region as static batches of 64, the rest as dynamic batches of dyn_batch (64
 * or 128) rays, with the region geometry the kernels use (csrc/pt_feed_rules.hpp).  Returns the number of rays handed out
 * twice or never and of batches that are not contiguous or leave the frame (0 = sound), or a negative ptc_status. */
int ptc_check_feed(uint32_t n, uint32_t static_eighths, uint32_t dyn_batch);
/* The sizing rule of ptc_resize, on the host (no GPU, no context; test hook): what a context whose parameters are
 * frames_in_flight (frames_auto != 0: the caller has not set it, and the in-flight state is capped at 24 GiB), batch_frames and
 * prefold would allocate for a width x height frame -- frames in flight, frames per batch, batch slots, single-frame slots, and
 * whether samples are staged (0: one frame in flight, shaded straight into the framebuffers).  PTC_ERR_INVALID for a NULL out
 * and for a resolution ptc_resize refuses. */
typedef struct ptc_frame_plan {
  int32_t frames, batch, big_slots, single_slots, staged;
} ptc_frame_plan;
int ptc_check_frame_plan(uint32_t width, uint32_t height, int frames_in_flight, int frames_auto, int batch_frames, int prefold,
                         ptc_frame_plan* out);
/* The instance rule of the megakernel, on the host (no GPU, no context; test hook; csrc/pt_mega_rules.hpp): which of its 22
 * kernels ptc_trace launches for a frame with these nine facts (0 or not 0 each) -- direct: "direct_light" and a lamp table of
 * weight > 0; env: an environment; env_lit: "environment_light", an environment and a table of weight > 0; smooth:
 * "smooth_normals" and vertex normals; textured: "textures", textures and texture coordinates; weigh: "mis" and (direct or
 * env_lit); lens: a lens radius > 0; plays: some bounce plays roulette, or < 0 for ptc_trace's own reading of `roulette` under
 * `max_bounces`; emitters: the scene has an emissive material -- and the roulette argument the kernel gets: `roulette` where a
 * bounce plays, else INT_MAX.  name_out: the kernel as a profile prints it, e.g. "k_megakernel_tex<true, false>".
 * PTC_ERR_INVALID for a NULL out and for a name_capacity the name does not fit in (40 bytes hold every name). */
int ptc_check_megakernel_instance(int direct, int env, int env_lit, int smooth, int textured, int weigh, int lens, int plays, int emitters,
                                  int roulette, int max_bounces, char* name_out, uint32_t name_capacity, int* roulette_out);
/* ... with the tenth fact, bent: "normal_maps", textures, texture coordinates and a normal-map binding (section 5q) -- the rule over
 * all 26 kernels; with bent 0 it answers as ptc_check_megakernel_instance does. */
int ptc_check_megakernel_instance2(int direct, int env, int env_lit, int smooth, int textured, int weigh, int lens, int plays, int emitters,
                                   int bent, int roulette, int max_bounces, char* name_out, uint32_t name_capacity, int* roulette_out);
/* Entry points for primary rays ("beam"), checked on the host (no GPU): for every 8 x 8-pixel tile of a width x height
 * frame of `camera`, the entries k_beam computes for the mesh under the object matrix object_m16 (NULL: identity;
 * column-major), and for sample rays of the tile (corners and centre of the jitter range of every stride-th pixel) the
 * closest hit of a walk from the tree's root against the same walk from the tile's entries.  Returns the number of rays
 * that disagree (0 = sound) or a negative status; stats5 (may be NULL): tiles, tiles without entries, entries, rays, hits;
 * entries_out (may be NULL): the entries themselves, [tiles][4][8 floats] = {box min, reference bits} {box max, 0}. */
int ptc_check_beam(const float* positions, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count, const float* object_m16,
                   const ptc_camera* camera, uint32_t width, uint32_t height, uint32_t stride, uint64_t* stats5, float* entries_out);
/* Host only, no GPU: the tile frustums ptc_check_beam and k_beam cull with, by themselves (the same shared rule, no mesh).  Per tile
 * 16 floats into frusta_out [tiles][16]: eye.xyz, usable (1 or 0), then the normals of the left, right, top and bottom plane; into
 * consts39 (may be NULL) the binary32 constants the rule read: camera matrix (16, column-major), its origin (3), viewport width and
 * height, lower-left x and y, the object's inverse matrix (16).  Returns the number of tiles or a negative status. */
int ptc_check_beam_frustum(const float* object_m16, const ptc_camera* camera, uint32_t width, uint32_t height, float* frusta_out,
                           uint64_t capacity_floats, float* consts39);
/* Test hook: the same entries as k_beam computes them on the GPU for the uploaded scene's first traversal launch. */
int ptc_debug_beam_entries(ptc_ctx* ctx, const ptc_camera* camera, float* entries_out, uint64_t capacity_floats);
/* Test hook: the per-lane form of a sphere run (csrc/pt_kernels_common.inc: sphere_run_lanes, what the kernels that end a bounce
 * run for a trailing run of up to eight translated spheres) on the uploaded scene's trailing sphere run, for the caller's rays.
 * rays, n and the four outputs as for ptc_intersect_rays, except that origins and directions must be finite, every t_min 1e-4 or
 * 1e-5 and every t_max >= 0 (the closest hit carried in; 3e38 and more: none).  slots: 1 (every bound of the run held against the smallest cap) or the number of rays a lane of the
 * fused shade kernel holds (2; an object is held against the caps of the objects before it) -- consecutive rays are laid into a
 * lane's slots as that kernel lays a tile's: ray g * 256 * slots + j * 256 + t is slot j of thread t of workgroup g.  candidates
 * (may be NULL): one byte per ray, bit k set when object k of the run is a candidate of that ray (sphere_candidates).
 * PTC_ERR_INVALID when the scene's trailing run does not take the per-lane form (none, more than eight objects, two classes of
 * matrices, a member that is no translated sphere, "sphere_lanes" 0), for another slots and for a ray outside that domain. */
int ptc_debug_sphere_lanes(ptc_ctx* ctx, const float* rays, uint32_t n, int slots, float* hit_t, float* hit_normal, uint32_t* hit_material,
                           uint8_t* hit_side, uint8_t* candidates);
/* TEST / diagnostic: the state block (DPersist, pt_device.hpp) of slot `slot`'s persistent launch ("persist"), copied after a
 * device synchronisation; its per-phase counters are filled in by -DPT_PERSIST_DEBUG builds only (tools/debug/persist_diff.py).
 * No reference equivalent. */
int ptc_debug_persist(ptc_ctx* ctx, int slot, void* dst, uint64_t bytes);

/* Device self-test of the arithmetic contract the parity tests rely on: evaluates IEEE divide,
 * sqrt and the deterministic sin/cos on the GPU for n inputs (host arrays in, host arrays out). */
int ptc_selftest_math(ptc_ctx* ctx, const float* a, const float* b, uint32_t n, float* out_div,
                      float* out_sqrt, float* out_sin, float* out_cos);
/* Device self-test of the per-path generator (csrc/pt_rng.hpp: thrust::default_random_engine + uniform_real_distribution<float>,
 * whose bits every frame depends on).  Per element i (host arrays in and out): seed(seeds[i]), discard(discards[i]), two raw values,
 * then two uniform draws; out[6 i ..] = the state after the seed, the state after the discard, the raw values, the bit
 * patterns of the draws. */
int ptc_selftest_rng(ptc_ctx* ctx, const uint32_t* seeds, const uint32_t* discards, uint32_t n, uint32_t* out);
/* The same header run on the host (no GPU; test hook): the same six words per element. */
int ptc_check_rng(const uint32_t* seeds, const uint32_t* discards, uint32_t n, uint32_t* out);
/* The environment's lookup (csrc/pt_env.hpp, the header ptc_sample_environment runs on the device) on the host: the map rgb of size n
 * (ptc_set_environment's layout and refusals) in `count` directions.  No GPU, no context; test hook. */
int ptc_check_environment(const float* rgb, uint32_t n, const float* dirs, uint32_t count, float* rgb_out);
/* ... and the map as ptc_set_environment uploads it: (n + 2) x (n + 2) texels of four floats {r, g, b, 0}, the apron filled in. */
int ptc_check_environment_apron(const float* rgb, uint32_t n, float* texels_out);
/* The environment's alias table (csrc/pt_env_light.hpp) as the first call that needs it builds it, on the host: no
 * GPU, no context; test hook.  entries_out (may be NULL): n n entries of 16 bytes {float q, uint32 alias, float f, float f of the
 * alias}, in table order k = j n + i; zeros for a map of weight 0.  *total_weight = W, *positive_squares = the squares of weight > 0. */
int ptc_check_environment_light_table(const float* rgb, uint32_t n, void* entries_out, double* total_weight, uint64_t* positive_squares);
/* The shading normal of section 5n (csrc/pt_smooth.hpp, the header the megakernel's smooth instances run on the device) on the host: no
 * GPU, no context; test hook.  Per case i the vertex normals n0, n1, n2 (3 floats each), the barycentrics u, v, the geometric normal g
 * facing the ray and the ray direction d (3 floats each), all under the object matrix m16 (column-major; its inverse as ptc_make_object
 * computes it).  ns_out: 3 floats a case; fallback_out (may be NULL): 1 where the rule fell back to g. */
int ptc_check_shading_normal(const float* n0, const float* n1, const float* n2, const float* u, const float* v, const float* g, const float* d,
                             const float* m16, uint32_t count, float* ns_out, uint8_t* fallback_out);
/* The texture lookup of section 5o (csrc/pt_texture.hpp, the header the textured kernels run on the device; steps 2 .. 7) on the
 * host: no GPU, no context; the host twin of ptc_sample_texture.  desc: one texture; st: 2 n floats; rgb_out: 3 n floats;
 * rejected_out (may be NULL): one byte a pair.  PTC_ERR_INVALID: a NULL, a texture ptc_set_textures would refuse. */
int ptc_check_texture_lookup(const ptc_texture_desc* desc, const float* st, uint32_t n, float* rgb_out, uint8_t* rejected_out);
/* The normal map's rule of section 5q (csrc/pt_normal_map.hpp, the header the normal-mapped kernels run on the device) on the host: no
 * GPU, no context.  desc: the map (its encoding is not read).  Per case i: the corners' object-space positions p0, p1, p2 (3 floats
 * each), their coordinate pairs st0, st1, st2 (2 floats each), the hit's u, v, the base normal b, the geometric normal g facing the ray
 * and the ray direction d (3 floats each), all under the object matrix m16 (column-major).  normal_out: 3 floats a case; outcome_out:
 * one byte a case, 2 bent, 3 flat, 4 kept.  PTC_ERR_INVALID: a NULL, a texture ptc_set_textures would refuse. */
int ptc_check_normal_map(const ptc_texture_desc* desc, const float* p0, const float* p1, const float* p2, const float* st0, const float* st1,
                         const float* st2, const float* u, const float* v, const float* m16, const float* b, const float* g, const float* d,
                         uint32_t count, float* normal_out, uint8_t* outcome_out);
/* ... and the sample on `count` caller-given points, normals and draws (v[i]: a raw value 1 .. 2^31 - 2; u + 3 i: u1, u2, u3), written as
 * ptc_environment_light writes a sample whose shadow ray is free: radiance 3 floats, shadow_rays 8 floats (may be NULL), sampled one
 * byte (may be NULL) per point.  PTC_ERR_INVALID: a NULL, n out of range, a bad component, a v out of range. */
int ptc_check_environment_light(const float* rgb, uint32_t n, const float* points, const float* normals, const uint32_t* v, const float* u,
                                uint32_t count, float* radiance, float* shadow_rays, uint8_t* sampled);
/* ... and the sample's density in `count` caller-given unit directions, as ptc_environment_light_pdf returns it (zeros for a map of
 * weight 0).  PTC_ERR_INVALID: a NULL, n out of range, a bad component. */
int ptc_check_environment_light_pdf(const float* rgb, uint32_t n, const float* dirs, uint32_t count, float* pdf_out);
/* The light sample of ptc_direct_light (csrc/pt_light_sample.hpp, the header k_light_sample and the megakernel's lit instances run on the
 * device) on the host, against the lamp table of `scene` (ptc_light_table's refusals): no GPU, no context; test hook.  Per point i the
 * point and its unit normal (3 floats each) and the three draws given explicitly: v[i] raw (1 .. 2^31 - 2; it picks the lamp), u + 2 i:
 * u1, u2.  Out, each may be NULL: lamp (the record picked), shadow_rays (8 floats, as ptc_direct_light returns them), contribution (3
 * floats, unshadowed), sampled (one byte).  A scene without lamps or of total weight 0: zeros.  PTC_ERR_INVALID: a NULL input, a v out of
 * range. */
int ptc_check_light_sample(const ptc_scene_desc* scene, const float* points, const float* normals, const uint32_t* v, const float* u,
                           uint32_t count, uint32_t* lamp, float* shadow_rays, float* contribution, uint8_t* sampled);

#ifdef __cplusplus
}
#endif
#endif /* PTCORE_H */
