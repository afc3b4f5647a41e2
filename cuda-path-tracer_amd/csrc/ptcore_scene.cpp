// ptcore_scene.cpp -- ptc_upload_scene as a sequence of stages: validation and the other refusals that
// need the caller's arrays alone; per mesh the reference BVH (reference_bvh: caller's, device-built or host-built); everything
// else the host can work out (stage_host: lamp table, sphere table, object -> mesh, triangle bases, launch table); the
// release of the old scene; uploads and per mesh the traversal layouts (mesh_layouts: device or host side); the instance
// triangles; and ONE commit (one assignment of the context's ptc_scene_state), after the last step that can fail.  Also
// ptc_build_bvh*, ptc_light_table, ptc_make_object.  Part of libptcore.so (ptcore_ctx.hpp).
#include "ptcore_ctx.hpp"
#include "pt_layout_rules.hpp"

#include <cmath>

using namespace pt;
using namespace ptcd;

namespace {

// One mesh of a scene description: the caller's arrays as bvh_from_mesh would see that mesh on its own.
struct MeshSlice {
  const float* positions = nullptr;
  uint32_t vertex_count = 0;
  const uint32_t* indices = nullptr;
  uint32_t index_count = 0;
  const ptc_bvh_node* caller_bvh = nullptr;
  uint32_t caller_nodes = 0;
};

// The meshes of a scene.  The reference keeps ONE mesh whatever the scene file says (scene_description.cpp:42,95), which is
// what a description without a mesh table means here; with a table (ptc_mesh_range) every mesh object instantiates the
// mesh its `index` names.
uint32_t mesh_count_of(const ptc_scene_desc* s) { return s->meshes ? s->mesh_count : (s->index_count ? 1u : 0u); }
uint32_t mesh_of_object(const ptc_scene_desc* s, const ptc_object& o) { return s->meshes ? o.index : 0u; }
MeshSlice mesh_slice(const ptc_scene_desc* s, uint32_t m)
{
  if (!s->meshes) return {s->positions, s->vertex_count, s->indices, s->index_count, s->bvh, s->bvh ? s->bvh_node_count : 0u};
  const ptc_mesh_range& r = s->meshes[m];
  const ptc_bvh_node* bvh = s->bvh && r.bvh_node_count ? s->bvh + r.first_bvh_node : nullptr;
  return {s->positions + 3u * (size_t)r.first_vertex, r.vertex_count, s->indices + r.first_index, r.index_count, bvh, bvh ? r.bvh_node_count : 0u};
}

// position of the first index that names no vertex, or -1
int64_t first_index_out_of_range(const uint32_t* indices, uint32_t index_count, uint32_t vertex_count)
{
  for (uint32_t i = 0; i < index_count; ++i)
    if (indices[i] >= vertex_count) return i;
  return -1;
}

// Matrices are column-major: m[4 * col + row].  is_affine: the last row is (0, 0, 0, 1).  all_linear: does `pred(entry, on
// the diagonal)` hold for every entry outside the translation column?
bool is_affine(const float* m) { return m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f; }
template <typename Pred>
bool all_linear(Pred pred)
{
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r)
      if (!(c == 3 && r < 3) && !pred(4 * c + r, c == r)) return false;
  return true;
}
// "simple": both matrices are a pure translation -- diagonal 1.0f, everything else outside the translation column a
// zero of either sign (a cofactor inverse leaves -0.0f in a checkerboard).  The reference's matrix arithmetic then has
// the same operands for every such object of a run except the translation, and a lane can fetch what differs for
// itself (sphere_run_lanes): box, inverse translation, sphere, translation, material
bool is_simple(const ptc_object& o)
{
  auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
  bool simple = all_linear([&](int k, bool diagonal) {
    for (const float* mat : {o.m, o.inv_m})
      if (diagonal ? bits(mat[k]) != 0x3f800000u : (bits(mat[k]) & 0x7fffffffu) != 0u) return false;
    return true;
  });
  for (int r = 0; r < 3; ++r) simple = simple && std::isfinite(o.m[12 + r]) && std::isfinite(o.inv_m[12 + r]);
  return simple;
}
// one sphere class: the same bits in both matrices outside the translation columns
bool same_linear(const ptc_object& a, const ptc_object& b)
{
  return all_linear([&](int k, bool) { return std::memcmp(&a.m[k], &b.m[k], 4) == 0 && std::memcmp(&a.inv_m[k], &b.inv_m[k], 4) == 0; });
}

// The world-space ball around a sphere object (DScene::sphere_ball), in double precision with the roundings of the
// float copies charged to the radius: centre = M (c, 1), radius = r * (largest singular value of M's 3 x 3 part).
// A matrix whose last row is not (0, 0, 0, 1), anything non-finite, a mesh object: radius -1 (no ball, never skipped).
static void sphere_ball_of(const ptc_object& o, const ptc_sphere* spheres, uint32_t sphere_count, uint32_t material, float4* out)
{
  out[0] = make_float4(0.f, 0.f, 0.f, -1.0f);
  for (uint32_t k = 1; k < kSphereTab; ++k) out[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (o.type != 0u || o.index >= sphere_count) return;
  const float* m = o.m;
  if (!is_affine(m)) return;
  const ptc_sphere& sp = spheres[o.index];
  double a[3][3];  // a[row][col]
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) a[r][c] = (double)m[4 * c + r];
  // largest eigenvalue of A^T A by power iteration from three starts (symmetric positive semi-definite 3 x 3), then
  // bounded from above by the Frobenius norm and pushed up by 1e-6 relative: an upper bound is all that is needed
  double g[3][3];
  double frob2 = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      g[i][j] = 0.0;
      for (int k = 0; k < 3; ++k) g[i][j] += a[k][i] * a[k][j];
      frob2 += a[i][j] * a[i][j];
    }
  if (!std::isfinite(frob2) || frob2 <= 0.0) return;
  double lam = 0.0;
  for (int start = 0; start < 3; ++start) {
    double v[3] = {start == 0 ? 1.0 : 0.3, start == 1 ? 1.0 : 0.2, start == 2 ? 1.0 : 0.1};
    double l = 0.0;
    for (int it = 0; it < 200; ++it) {
      double w[3];
      for (int i = 0; i < 3; ++i) w[i] = g[i][0] * v[0] + g[i][1] * v[1] + g[i][2] * v[2];
      const double n = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
      if (!(n > 0.0)) break;
      for (int i = 0; i < 3; ++i) v[i] = w[i] / n;
      l = n;
    }
    lam = std::max(lam, l);
  }
  // power iteration approaches the eigenvalue from below: the Gershgorin bound of G is a true upper bound; take the
  // smaller of it and the Frobenius norm, but never less than the iterate
  double gersh = 0.0;
  for (int i = 0; i < 3; ++i) gersh = std::max(gersh, std::fabs(g[i][0]) + std::fabs(g[i][1]) + std::fabs(g[i][2]));
  // (only proven bounds: the iterate approaches from below and is no bound, however close -- round 4 took "iterate plus
  // 1 %" when that was smaller, which an anisotropic matrix with a slowly converging iteration could undercut)
  double lam_up = std::min(gersh, frob2);
  lam_up = std::max(lam_up, lam);
  const double sigma = std::sqrt(lam_up) * (1.0 + 1e-6);
  const double cx = a[0][0] * sp.center[0] + a[0][1] * sp.center[1] + a[0][2] * sp.center[2] + (double)m[12];
  const double cy = a[1][0] * sp.center[0] + a[1][1] * sp.center[1] + a[1][2] * sp.center[2] + (double)m[13];
  const double cz = a[2][0] * sp.center[0] + a[2][1] * sp.center[1] + a[2][2] * sp.center[2] + (double)m[14];
  const double rad = std::fabs((double)sp.radius) * sigma;
  if (!std::isfinite(cx + cy + cz + rad)) return;
  const float fx = (float)cx, fy = (float)cy, fz = (float)cz;
  // What separates the ball the kernels compute with from the sphere the reference's float sequence sees, as a length:
  // the rounding of the centre to float (slack); the one rounding of `origin + inverse translation` in inverse_transform_ray,
  // which is relative to the OBJECT-space origin and so carries 2^-24 of the sphere's own centre; and the rounding of the hit
  // point back in world space (2^-24 of its coordinates), which moves the distance the reference records against the root.
  // The OUTER ball (radius + that) contains what the reference can hit: it decides "missed" and the lower bounds; the INNER
  // ball (radius - that, row 1 .z) lies inside it: "surely hit" and the upper bounds come from it (round 4 took the outer
  // radius for both, which is the wrong way round for the latter -- a small sphere far from the origin).
  const double slack = std::fabs(cx - fx) + std::fabs(cy - fy) + std::fabs(cz - fz);
  const double coord = std::fabs(cx) + std::fabs(cy) + std::fabs(cz) + std::fabs((double)sp.center[0]) + std::fabs((double)sp.center[1]) +
                       std::fabs((double)sp.center[2]) + 3.0 * rad;
  const double cerr = slack + coord * (1.0 / 4194304.0);  // 2^-22
  float fr = (float)((rad + cerr) * (1.0 + 1e-6));
  fr = std::nextafter(fr, INFINITY);
  float fin = (float)(std::max(0.0, std::fabs((double)sp.radius) * (1.0 - 1e-6) - cerr) * (1.0 - 1e-6));
  // "Surely hit" also means that the reference's test of the object's STORED box passes first (path_tracer.cu:84), and the C ABI
  // takes that box as given: the inner ball must lie inside it.  No inner ball for a radius that is not positive (the reference's
  // own box of a negative radius has min > max: the object is never hit) or a box that is empty on an axis; otherwise no larger
  // than the distance from the centre to the nearest face (a caller's clipped box).  Before this bound a ray through such an
  // object was a "sure hit" that capped the list, and a sphere behind it, later in the list, was never tested.
  double face = (double)INFINITY;
  const double centre[3] = {cx, cy, cz};
  for (int ax = 0; ax < 3; ++ax)
    face = std::min(face, std::min(centre[ax] - (double)o.aabb_min[ax], (double)o.aabb_max[ax] - centre[ax]));
  if (!(sp.radius > 0.0f) || !(face > 0.0)) fin = 0.0f;  // (a NaN bound: none)
  else fin = std::min(fin, (float)std::max(0.0, face * (1.0 - 1e-6) - cerr));
  fin = fin > 0.0f ? std::nextafter(fin, 0.0f) : 0.0f;
  float inv_sigma = (float)((1.0 / sigma) * (1.0 - 1e-6));
  inv_sigma = std::nextafter(inv_sigma, 0.0f);
  out[0] = make_float4(fx, fy, fz, fr);
  const bool simple = is_simple(o);
  out[1] = make_float4(inv_sigma, simple ? 1.0f : 0.0f, simple ? fin : 0.0f, 0.f);  // (.z: a simple object does not stretch)
  float mat_f;
  std::memcpy(&mat_f, &material, 4);
  out[2] = make_float4(o.aabb_min[0], o.aabb_min[1], o.aabb_min[2], o.inv_m[12]);
  out[3] = make_float4(o.aabb_max[0], o.aabb_max[1], o.aabb_max[2], o.inv_m[13]);
  out[4] = make_float4(sp.center[0], sp.center[1], sp.center[2], o.inv_m[14]);
  out[5] = make_float4(o.m[12], o.m[13], o.m[14], sp.radius);
  out[6] = make_float4(mat_f, 0.f, 0.f, 0.f);
}

// DScene::sphere_ball of every object, and per object 0 or the class of a simple sphere object (ptc_ctx::sphere_class):
// classes are numbered from 1 in the order of their first object
void sphere_table(const ptc_scene_desc* s, std::vector<float4>& balls, std::vector<uint32_t>& sphere_class)
{
  balls.resize((size_t)s->object_count * kSphereTab);
  sphere_class.assign(s->object_count, 0u);
  std::vector<uint32_t> class_first;  // first object of every class
  for (uint32_t i = 0; i < s->object_count; ++i) {
    sphere_ball_of(s->objects[i], s->spheres, s->sphere_count, s->object_material_indices[i], &balls[(size_t)kSphereTab * i]);
    if (balls[(size_t)kSphereTab * i + 1u].y == 0.0f) continue;
    uint32_t k = 0;
    while (k < class_first.size() && !same_linear(s->objects[class_first[k]], s->objects[i])) ++k;
    if (k == class_first.size()) class_first.push_back(i);
    sphere_class[i] = k + 1u;
  }
}

int validate_scene(ptc_ctx* ctx, const ptc_scene_desc* s)
{
  if (s->object_count && (!s->objects || !s->object_material_indices)) return fail(ctx, PTC_ERR_INVALID, "objects missing");
  if (s->sphere_count && !s->spheres) return fail(ctx, PTC_ERR_INVALID, "spheres missing");
  if (s->material_count && !s->materials) return fail(ctx, PTC_ERR_INVALID, "materials missing");
  if (s->index_count % 3u) return fail(ctx, PTC_ERR_INVALID, "index_count is not a multiple of 3");
  if (s->object_count > 0xffffu) return fail(ctx, PTC_ERR_INVALID, "more than 65535 objects");
  if (s->index_count && (!s->indices || !s->positions)) return fail(ctx, PTC_ERR_INVALID, "mesh arrays missing");
  if (s->meshes && s->mesh_count > 0xffffu) return fail(ctx, PTC_ERR_INVALID, "more than 65535 meshes");
  for (uint32_t m = 0; m < mesh_count_of(s); ++m) {
    if (s->meshes) {
      const ptc_mesh_range& r = s->meshes[m];
      if ((uint64_t)r.first_vertex + r.vertex_count > s->vertex_count || (uint64_t)r.first_index + r.index_count > s->index_count ||
          r.index_count % 3u)
        return fail(ctx, PTC_ERR_INVALID, "mesh range outside the vertex / index arrays");
      if (r.bvh_node_count && (!s->bvh || (uint64_t)r.first_bvh_node + r.bvh_node_count > s->bvh_node_count))
        return fail(ctx, PTC_ERR_INVALID, "mesh range outside the BVH array");
    }
    const MeshSlice mesh = mesh_slice(s, m);
    if (first_index_out_of_range(mesh.indices, mesh.index_count, mesh.vertex_count) >= 0)
      return fail(ctx, PTC_ERR_INVALID, "vertex index out of range");
  }
  for (uint32_t i = 0; i < s->object_count; ++i) {
    const ptc_object& o = s->objects[i];
    if (o.type > 1u) return fail(ctx, PTC_ERR_INVALID, "unknown object type");
    if (o.type == 0u && o.index >= s->sphere_count) return fail(ctx, PTC_ERR_INVALID, "sphere index out of range");
    if (o.type == 1u && s->meshes && o.index >= s->mesh_count) return fail(ctx, PTC_ERR_INVALID, "mesh index out of range");
    if (s->object_material_indices[i] >= s->material_count) return fail(ctx, PTC_ERR_INVALID, "material index out of range");
  }
  for (uint32_t i = 0; i < s->material_count; ++i) {
    const ptc_material& m = s->materials[i];
    if (m.type < 0 || m.type > 3) return fail(ctx, PTC_ERR_INVALID, "unknown material type");
    if (m.type == 3) {  // emissive (an extension): radiance rgb finite and >= 0, p[3] reserved
      for (int k = 0; k < 3; ++k)
        if (!(std::isfinite(m.p[k]) && m.p[k] >= 0.0f))
          return fail(ctx, PTC_ERR_INVALID, "material " + std::to_string(i) + ": emission must be finite and >= 0");
      if (m.p[3] != 0.0f) return fail(ctx, PTC_ERR_INVALID, "material " + std::to_string(i) + ": p[3] of an emissive material must be 0");
    }
  }
  return PTC_OK;
}

// A caller's tree (ptc_scene_desc::bvh).  Besides the ranges, the rules the traversal layouts rely on and the reference's
// walk never needs (include/ptcore.h): every node but the root is the child of exactly one node, a
// leaf's offset is a multiple of 3, a leaf's box holds its triangle's vertices, a child's box lies inside its parent's.
// Exact float comparisons, O(count); the indices were checked against the vertex count before (validate_scene).
int validate_bvh(ptc_ctx* ctx, const MeshSlice& mesh)
{
  const ptc_bvh_node* nodes = mesh.caller_bvh;
  const uint32_t count = mesh.caller_nodes, index_count = mesh.index_count;
  auto bad = [&](uint32_t i, const std::string& what) { return fail(ctx, PTC_ERR_INVALID, "BVH node " + std::to_string(i) + ": " + what); };
  std::vector<uint8_t> parents(count, 0u);
  for (uint32_t i = 0; i < count; ++i) {
    const ptc_bvh_node& n = nodes[i];
    for (int k = 0; k < 3; ++k)
      if (!(n.aabb_min[k] <= n.aabb_max[k])) return bad(i, "empty or NaN box");
    const uint32_t f = n.first_child_or_primitive;
    if (n.primitive_count != 0u) {
      if ((uint64_t)f + 2u >= index_count) return bad(i, "leaf out of range");
      if (f % 3u) return bad(i, "leaf offset is not a multiple of 3");
      for (uint32_t v = 0; v < 3u; ++v) {
        const float* p = mesh.positions + 3u * (size_t)mesh.indices[f + v];
        for (int k = 0; k < 3; ++k)
          if (!(n.aabb_min[k] <= p[k] && p[k] <= n.aabb_max[k])) return bad(i, "leaf box does not contain its triangle");
      }
    } else {
      if ((uint64_t)f + 1u >= count || f <= i) return bad(i, "child out of range");
      for (uint32_t c = f; c <= f + 1u; ++c) {
        if (parents[c]++) return bad(c, "child of more than one node");
        for (int k = 0; k < 3; ++k)
          if (!(n.aabb_min[k] <= nodes[c].aabb_min[k] && nodes[c].aabb_max[k] <= n.aabb_max[k]))
            return bad(c, "box not inside its parent's (node " + std::to_string(i) + ")");
      }
    }
  }
  for (uint32_t i = 1; i < count; ++i)
    if (!parents[i]) return bad(i, "no node's child");
  return PTC_OK;
}

// depth of a tree numbered children-after-parents; level_base (optional) gets the first node of every depth plus the
// node count when the nodes are stored depth by depth (the reference's breadth-first numbering), else it is left empty
uint32_t bvh_depth_of(const ptc_bvh_node* nodes, uint32_t count, std::vector<uint32_t>* level_base = nullptr)
{
  std::vector<uint32_t> depth(count, 0u);
  uint32_t deepest = 0;
  bool by_level = true;
  if (level_base) level_base->assign(1, 0u);
  for (uint32_t i = 0; i < count; ++i) {
    if (depth[i] < deepest) by_level = false;
    if (depth[i] > deepest && level_base) level_base->push_back(i);
    deepest = std::max(deepest, depth[i]);
    if (nodes[i].primitive_count == 0u) {
      depth[nodes[i].first_child_or_primitive] = depth[i] + 1;
      depth[nodes[i].first_child_or_primitive + 1] = depth[i] + 1;
    }
  }
  if (level_base) {
    level_base->push_back(count);
    if (!by_level || level_base->size() != (size_t)deepest + 2u) level_base->clear();
  }
  return deepest;
}

}  // namespace

namespace ptcd {

// The lamp table (include/ptcore.h: ptc_light) from the caller's arrays -- not from DScene::tris, which is in
// tree order and may exist only on the device.  Records in binary32 with the operations of the instance triangles
// (layout_rules::instance_triangle); weights, their running sum and the cdf in binary64, from the records' own fields.
// thresholds (may be null): what a sample picks its lamp by (light_pick, pt_light_sample.hpp) -- per record T_k, the first of the
// generator's N = 2^31 - 2 states n = v - 1 that belongs to a later record: round(run_k / W * N) from the same running sums, raised so
// that every record of weight > 0 owns a state, capped so that the live records behind it still get one each; a record of weight 0
// repeats its predecessor's (it owns nothing), the last live record and everything behind it get N.  Record k so owns
// T_k - T_(k-1) states, within 1 + m of its share w_k / W * N (m = the live records whose share is below one state).  Empty for a
// table of weight 0.
int build_light_table(const ptc_scene_desc* s, std::vector<ptc_light>& out, ptc_light_info* info, uint32_t* last, std::string* err,
                      std::vector<uint32_t>* thresholds)
{
  out.clear();
  if (thresholds) thresholds->clear();
  ptc_light_info li{};
  std::vector<double> weight;
  std::vector<float> lum_of;
  for (uint32_t i = 0; i < s->object_count; ++i) {
    const ptc_object& o = s->objects[i];
    const uint32_t mi = s->object_material_indices[i];
    const ptc_material& mat = s->materials[mi];
    if (mat.type != 3) continue;
    ++li.emissive_objects;
    const float lum = std::max(std::max(mat.p[0], mat.p[1]), mat.p[2]);
    m4 m;
    std::memcpy(&m, o.m, sizeof m);
    auto push = [&](ptc_light& l, uint32_t kind, double area) {
      l.cdf = 0.0f;
      l.inv_pdf = 0.0f;
      l.object = i;
      l.kind_material = mi | kind << 31;
      out.push_back(l);
      weight.push_back(area * (double)lum);
      lum_of.push_back(lum);
      li.total_area += area;
    };
    if (o.type == 0u) {
      // uniform on the object-space sphere is uniform in area on its image only under a similarity
      double len[3], c[3][3];
      for (int k = 0; k < 3; ++k) {
        for (int r = 0; r < 3; ++r) c[k][r] = (double)o.m[4 * k + r];
        len[k] = std::sqrt(c[k][0] * c[k][0] + c[k][1] * c[k][1] + c[k][2] * c[k][2]);
      }
      bool ok = is_affine(o.m) && std::isfinite(len[0] + len[1] + len[2]) && len[0] > 0.0;
      for (int a = 0; a < 3 && ok; ++a)
        for (int b = a + 1; b < 3; ++b) {
          const double dt = c[a][0] * c[b][0] + c[a][1] * c[b][1] + c[a][2] * c[b][2];
          ok = ok && std::fabs(dt) <= 1e-5 * len[a] * len[b] && std::fabs(len[a] - len[b]) <= 1e-5 * std::max(len[a], len[b]);
        }
      if (!ok) {
        *err = "object " + std::to_string(i) + ": an emissive sphere whose matrix is not a similarity (rotation x uniform scale + translation) cannot be sampled";
        out.clear();
        return PTC_ERR_INVALID;
      }
      const ptc_sphere& sp = s->spheres[o.index];
      const f3 centre = xform_point(m, mk3(sp.center[0], sp.center[1], sp.center[2]));
      const float radius = length(mk3(o.m[0], o.m[1], o.m[2])) * sp.radius;
      ptc_light l{};
      l.p0[0] = centre.x, l.p0[1] = centre.y, l.p0[2] = centre.z;
      l.e1[0] = radius;
      push(l, 1u, 4.0 * 3.14159265358979323846 * (double)radius * (double)radius);
      ++li.sphere_lights;
    } else {
      const MeshSlice mesh = mesh_slice(s, mesh_of_object(s, o));
      for (uint32_t t = 0; t + 2u < mesh.index_count; t += 3u) {
        const float *q0 = mesh.positions + 3u * (size_t)mesh.indices[t], *q1 = mesh.positions + 3u * (size_t)mesh.indices[t + 1u],
                    *q2 = mesh.positions + 3u * (size_t)mesh.indices[t + 2u];
        float4 rec[kTriVec4];
        layout_rules::instance_triangle(m, mk3(q0[0], q0[1], q0[2]), mk3(q1[0], q1[1], q1[2]), mk3(q2[0], q2[1], q2[2]), rec);
        ptc_light l{};
        std::memcpy(l.p0, rec, 12u * sizeof(float));
        const double e1[3] = {l.e1[0], l.e1[1], l.e1[2]}, e2[3] = {l.e2[0], l.e2[1], l.e2[2]};
        const double cx = e1[1] * e2[2] - e2[1] * e1[2], cy = e1[2] * e2[0] - e2[2] * e1[0], cz = e1[0] * e2[1] - e2[0] * e1[1];
        push(l, 0u, 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz));
        ++li.triangle_lights;
      }
    }
    if (out.size() > 0x7fffffffu) {
      *err = "more than 2^31 - 1 lamp primitives";
      out.clear();
      return PTC_ERR_INVALID;
    }
  }
  li.lights = (uint32_t)out.size();
  double W = 0.0;
  uint32_t last_live = 0u;
  uint64_t live = 0u;
  for (size_t k = 0; k < out.size(); ++k) {
    if (!std::isfinite(weight[k])) {
      *err = "lamp primitive " + std::to_string(k) + " (object " + std::to_string(out[k].object) + ") has no finite area";
      out.clear();
      return PTC_ERR_INVALID;
    }
    W += weight[k];
    if (weight[k] > 0.0) last_live = (uint32_t)k, ++live;
  }
  constexpr uint64_t kStates = 0x7ffffffeull;  // N: the values v - 1 of a raw draw
  if (live > kStates) {
    *err = "more than 2^31 - 2 lamp primitives of weight > 0: a sample's draw has no state for each";
    out.clear();
    return PTC_ERR_INVALID;
  }
  li.total_weight = W;
  if (W > 0.0) {
    if (thresholds) thresholds->resize(out.size());
    double run = 0.0;
    uint64_t prev = 0u, behind = live;  // T_(k-1); live records from k on
    for (size_t k = 0; k < out.size(); ++k) {
      run += weight[k];
      out[k].cdf = k >= last_live ? 1.0f : (float)(run / W);
      out[k].inv_pdf = lum_of[k] == 0.0f ? 0.0f : (float)(W / (double)lum_of[k]);
      if (k >= last_live) {
        prev = kStates;
      } else if (weight[k] > 0.0) {
        --behind;
        const uint64_t ideal = (uint64_t)std::floor(run / W * (double)kStates + 0.5);
        prev = std::min(std::max(ideal, prev + 1u), kStates - behind);
      }
      if (thresholds) (*thresholds)[k] = (uint32_t)prev;
    }
  }
  if (info) *info = li;
  if (last) *last = last_live;
  return PTC_OK;
}

// Per material the inv_pdf every lamp record of that material carries (multiple importance sampling): (float)(W / lum)
// with build_light_table's lum and W = its total weight; 0 for a material that is not emissive, for lum == 0 and for a table of weight 0.
void light_material_pdf(const ptc_scene_desc* s, double total_weight, std::vector<float>& out)
{
  out.assign(s->material_count, 0.0f);
  if (!(total_weight > 0.0)) return;
  for (uint32_t m = 0; m < s->material_count; ++m) {
    const ptc_material& mat = s->materials[m];
    if (mat.type != 3) continue;
    const float lum = std::max(std::max(mat.p[0], mat.p[1]), mat.p[2]);
    out[m] = lum == 0.0f ? 0.0f : (float)(total_weight / (double)lum);
  }
}

int checked_light_table(const ptc_scene_desc* s, std::vector<ptc_light>& out, ptc_light_info* info, uint32_t* last,
                        std::vector<uint32_t>* thresholds)
{
  if (int rc = validate_scene(nullptr, s)) return rc;
  std::string err;
  if (int rc = build_light_table(s, out, info, last, &err, thresholds)) return fail(nullptr, rc, err);
  return PTC_OK;
}

// What ptc_set_textures and ptc_check_texture_lookup refuse in one texture ("" : nothing)
std::string texture_refusal(const ptc_texture_desc& t)
{
  if (t.width < 1u || t.width > texmap::kMaxSide || t.height < 1u || t.height > texmap::kMaxSide)
    return "is " + std::to_string(t.width) + " x " + std::to_string(t.height) + ": each side must be in [1,4096]";
  if (!t.rgba8) return "has a NULL texel pointer";
  if (t.encoding > PTC_TEXTURE_SRGB) return "has encoding " + std::to_string(t.encoding) + ": 0 (linear) or 1 (sRGB)";
  if (t.filter > PTC_TEXTURE_BILINEAR) return "has filter " + std::to_string(t.filter) + ": 0 (nearest) or 1 (bilinear)";
  if (t.wrap > PTC_TEXTURE_CLAMP) return "has wrap " + std::to_string(t.wrap) + ": 0 (repeat) or 1 (clamp)";
  return "";
}

}  // namespace ptcd

namespace {

const char kBvhFailed[] = "BVH build failed (empty SAH side: coincident centroids?)";

// The reference BVH of a mesh built on the device; the caller has checked the indices and the vertices in use.  nodes_host
// gets the 2T-1 nodes in the reference's layout; *packed_out (when asked for) keeps the device copy in DScene::bvh's layout,
// owned by the caller.
int bvh_on_device(ptc_ctx* ctx, const MeshSlice& mesh, ptc_bvh_node* nodes_host, uint32_t* max_depth, float4** packed_out,
                  std::vector<uint32_t>* level_base = nullptr)
{
  const uint32_t T = mesh.index_count / 3u;
  if (T == 0u) return fail(ctx, PTC_ERR_BVH, "empty mesh");
  std::vector<void*> pool;
  const float* d_pos = nullptr;
  const uint32_t* d_idx = nullptr;
  float4* d_packed = nullptr;
  ptc_bvh_node* d_nodes = nullptr;
  const size_t count = 2u * (size_t)T - 1u;
  int rc = upload(ctx, pool, &d_pos, mesh.positions, (size_t)mesh.vertex_count * 3u);
  if (!rc) rc = upload(ctx, pool, &d_idx, mesh.indices, (size_t)T * 3u);
  if (!rc) rc = dev_alloc(ctx, pool, &d_packed, 2u * count);
  if (!rc && nodes_host) rc = dev_alloc(ctx, pool, &d_nodes, count);
  uint32_t built = 0u;
  if (!rc) {
    rc = build_bvh_device(ctx->stream, d_pos, d_idx, T * 3u, d_packed, d_nodes, &built, max_depth, level_base);
    if (rc) fail(ctx, rc, rc == PTC_ERR_BVH ? kBvhFailed : "device BVH build failed");
  }
  if (!rc && nodes_host && hipMemcpy(nodes_host, d_nodes, count * sizeof(ptc_bvh_node), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(ctx, PTC_ERR_HIP, "device BVH download failed");
  for (void* p : pool)
    if (p != d_packed || rc || !packed_out) (void)hipFree(p);
  if (!rc && packed_out) *packed_out = d_packed;
  return rc ? rc : (int)built;
}

// one mesh of the scene on its way to the device
struct MeshWork {
  MeshSlice in;
  // reference BVH (reference_bvh)
  std::vector<ptc_bvh_node> built;   // host copy of a BVH built here (only when something on the host needs it)
  const ptc_bvh_node* nodes = nullptr;  // the host's copy, the caller's or `built`; null when only the device holds the tree
  std::vector<uint32_t> level_base;  // first node of every depth + the node count, when the nodes are stored depth by depth
  float4* dev_packed = nullptr;      // the device builder's output, already in DMeshView::bvh's layout
  uint32_t node_count = 0, depth = 0, triangles = 0;
  bool layouts_on_device = false;
  // traversal layouts (mesh_layouts), whichever side built them
  DMeshView view{};
  const uint32_t* tri_order_dev = nullptr;  // depth-first rank -> triangle: on the device ...
  std::vector<uint32_t> tri_order_host;     // ... or on the host
  uint32_t w4_depth = 0, w4_nodes = 0;
  ~MeshWork() { if (dev_packed) (void)hipFree(dev_packed); }
};

// An upload in progress: the scene state it builds beside the context (ptc_scene_state: assigned to the context as a whole,
// at the end; freed with this struct if it never gets there), the host's staging of arrays that go to the device only
// (stage_host), and the clock behind upload_times: lap(field) charges the time since the last lap to that field.
struct NewScene : ptc_scene_state {
  std::vector<ptc_light> lights;
  std::vector<uint32_t> thresholds;  // the records' selection thresholds (build_light_table); empty: nothing to sample
  std::vector<float> material_pdf; // per material the records' inv_pdf (light_material_pdf); uploaded with the lamp table
  std::vector<float4> balls;       // DScene::sphere_ball
  std::vector<uint32_t> tri_base;  // DScene::object_tri_base
  std::vector<uint32_t> first_vertex;  // per mesh: where its vertices start in the scene's arrays (vertex normals, section 5n)
  std::vector<uint32_t> first_index;   // per mesh: where its corners start in the scene's indices (texture coordinates, section 5o)
  size_t tri_records = 0;          // records of DScene::tris
  std::chrono::steady_clock::time_point start = std::chrono::steady_clock::now(), last = start;
  void lap(float& into)
  {
    const auto now = std::chrono::steady_clock::now();
    into += std::chrono::duration<float, std::milli>(now - last).count();
    last = now;
  }
  ~NewScene() { free_pool(scene_allocs); }
};

// The reference BVH of one mesh (scene_description.cpp:99-101): the caller's tree, else the device builder's, else the host
// builder's -- and with it which side derives the layouts.
int reference_bvh(ptc_ctx* ctx, MeshWork& w, NewScene& n)
{
  if (w.in.index_count == 0u) return PTC_OK;  // (the reference panics on an empty mesh, bvh.cpp:200; here: a mesh nobody can hit)
  if (w.in.caller_bvh) {
    w.nodes = w.in.caller_bvh;
    w.node_count = w.in.caller_nodes;
    w.depth = bvh_depth_of(w.nodes, w.node_count, &w.level_base);
    n.lap(n.upload_times.copy_ms);
  } else {
    const bool host_copy = !ctx->bvh_on_device || !ctx->layout_on_device;
    if (host_copy) w.built.resize((size_t)w.in.index_count / 3u * 2u);
    int rc;
    if (ctx->bvh_on_device) {
      rc = bvh_on_device(ctx, w.in, host_copy ? w.built.data() : nullptr, &w.depth, &w.dev_packed, &w.level_base);
      if (rc < 0) return rc;
      n.upload_times.bvh_on_device = 1u;
    } else {
      rc = build_bvh(w.in.positions, w.in.vertex_count, w.in.indices, w.in.index_count, w.built.data(), &w.depth);
      if (rc < 0) return fail(ctx, rc, kBvhFailed);
      (void)bvh_depth_of(w.built.data(), (uint32_t)rc, &w.level_base);
    }
    w.nodes = host_copy ? w.built.data() : nullptr;
    w.node_count = (uint32_t)rc;
    n.lap(n.upload_times.bvh_build_ms);
  }
  w.triangles = w.node_count ? (w.node_count + 1u) / 2u : 0u;
  // depth-first traversal pushes two children per inner node popped: stack need = depth + 1
  if (w.node_count && w.depth + 2u > (uint32_t)kStackDepth)
    return fail(ctx, PTC_ERR_STACK, "BVH depth " + std::to_string(w.depth) + " exceeds the traversal stack");
  // the layouts come from the device when the nodes are stored depth by depth (the reference's breadth-first order:
  // always, unless the caller brought a tree numbered some other way)
  w.layouts_on_device = ctx->layout_on_device && w.node_count != 0u && !w.level_base.empty();
  if (!w.layouts_on_device && w.node_count != 0u && !w.nodes) return fail(ctx, PTC_ERR_INVALID, "internal: no host copy of the BVH");
  return PTC_OK;
}

// Launches of the persistent pipeline (ptc_ctx::TraceLaunch) from the objects' types and, per object, the nodes of the mesh
// it instantiates.  A mesh object without nodes (empty mesh) is no launch; the sphere code skips non-sphere objects, so
// the runs on both sides of it merge.
std::vector<ptc_ctx::TraceLaunch> launch_table(const ptc_object* objects, const std::vector<uint32_t>& object_nodes,
                                               uint32_t* tail_begin, uint32_t* tail_end)
{
  std::vector<ptc_ctx::TraceLaunch> launches;
  const uint32_t count = (uint32_t)object_nodes.size();
  uint32_t run_begin = 0;  // objects [run_begin, i) come after the last mesh launch ...
  bool any = false;        // ... and hold a sphere
  for (uint32_t i = 0; i < count; ++i)
    if (objects[i].type == 0u) {
      any = true;
    } else if (object_nodes[i]) {
      launches.push_back({i, any ? run_begin : 0u, any ? i : 0u});
      run_begin = i + 1u;
      any = false;
    }
  *tail_begin = any ? run_begin : 0u;
  *tail_end = any ? count : 0u;
  return launches;
}

// Everything of the new scene that the host works out alone, from the description and the meshes' node counts; the old
// scene is still in place, and the one refusal here leaves it there.
int stage_host(ptc_ctx* ctx, const ptc_scene_desc* s, const std::vector<MeshWork>& meshes, NewScene& n)
{
  // the lamp table (direct-light queries).  An emissive sphere that cannot be sampled is no reason to
  // refuse the scene: it renders as ever, only ptc_direct_light refuses
  if (build_light_table(s, n.lights, &n.light_info, &n.light_last, &n.light_error, &n.thresholds) != PTC_OK) {
    n.light_info = ptc_light_info{};
    n.thresholds.clear();
  }
  if (!n.thresholds.empty()) light_material_pdf(s, n.light_info.total_weight, n.material_pdf);
  for (uint32_t i = 0; i < s->material_count; ++i) n.has_emitters |= s->materials[i].type == 3;
  sphere_table(s, n.balls, n.sphere_class);
  // per mesh OBJECT (instance): its mesh and the first of its world-space triangle records, which end with one all-zero
  // record (the dummy triangle of the four-wide tree's unused slots)
  n.object_mesh.assign(s->object_count, 0u);
  n.tri_base.assign(s->object_count, 0u);
  std::vector<uint32_t> object_nodes(s->object_count, 0u);
  for (uint32_t i = 0; i < s->object_count; ++i) {
    if (s->objects[i].type != 1u) continue;
    const uint32_t m = mesh_of_object(s, s->objects[i]);
    n.object_mesh[i] = m;
    n.tri_base[i] = (uint32_t)n.tri_records;
    if (m < meshes.size()) {
      n.tri_records += (size_t)meshes[m].triangles + 1u;
      object_nodes[i] = meshes[m].node_count;
    }
    if (n.tri_records > 0x7fffffffull) return fail(ctx, PTC_ERR_OOM, "too many instance triangles");
  }
  n.launches = launch_table(s->objects, object_nodes, &n.tail_begin, &n.tail_end);
  n.vertex_count = s->vertex_count;
  for (uint32_t m = 0; m < meshes.size(); ++m) n.first_vertex.push_back(s->meshes ? s->meshes[m].first_vertex : 0u);
  n.index_count = s->index_count;
  n.material_count = s->material_count;
  for (uint32_t m = 0; m < meshes.size(); ++m) n.first_index.push_back(s->meshes ? s->meshes[m].first_index : 0u);
  for (const MeshWork& w : meshes) {
    n.bvh_nodes += w.node_count;
    n.bvh_depth = std::max(n.bvh_depth, w.depth);
    n.triangles += w.in.index_count / 3u;
  }
  DScene& d = n.scene;
  d.object_count = s->object_count;
  d.refill_lanes = ctx->refill_lanes;
  d.split_idle = ctx->split_idle;
  d.static_eighths = ctx->static_eighths;
  d.force_slow = (uint32_t)ctx->force_slow;
  d.spill_stride = ctx->traverse_waves * kWave;  // (the overflow areas themselves belong to the frame slots, batch_begin)
  d.lds_cap = std::min<uint32_t>(ctx->lds_entries, (uint32_t)kLds4);
  return PTC_OK;
}

// the arrays every scene has: lamp records, the reference's four tables, the sphere table
int upload_tables(ptc_ctx* ctx, const ptc_scene_desc* s, NewScene& n)
{
  std::vector<void*>& pool = n.scene_allocs;
  DScene& d = n.scene;
  if (!n.thresholds.empty()) {
    static_assert(sizeof(ptc_light) == 4 * sizeof(float4), "a lamp record is four float4");
    if (int rc = upload(ctx, pool, &n.light_records, reinterpret_cast<const float4*>(n.lights.data()), 4u * n.lights.size())) return rc;
    if (int rc = upload(ctx, pool, &n.light_thresholds, n.thresholds.data(), n.thresholds.size())) return rc;
    if (int rc = upload(ctx, pool, &n.light_material_pdf, n.material_pdf.data(), n.material_pdf.size())) return rc;
  }
  const DObject* objects = nullptr;
  if (int rc = upload(ctx, pool, &objects, reinterpret_cast<const DObject*>(s->objects), s->object_count)) return rc;
  d.objects = objects;
  if (int rc = upload(ctx, pool, &d.object_material, s->object_material_indices, s->object_count)) return rc;
  if (int rc = upload(ctx, pool, &d.spheres, reinterpret_cast<const float4*>(s->spheres), s->sphere_count)) return rc;
  const DMaterial* mats = nullptr;
  if (int rc = upload(ctx, pool, &mats, reinterpret_cast<const DMaterial*>(s->materials), s->material_count)) return rc;
  d.materials = mats;
  return upload(ctx, pool, &d.sphere_ball, n.balls.data(), n.balls.size());
}

// the arrays of the reference layout of one mesh: positions, indices, nodes as two float4 {min.xyz, first}, {max.xyz, count}
int mesh_arrays(ptc_ctx* ctx, NewScene& n, MeshWork& w)
{
  std::vector<void*>& pool = n.scene_allocs;
  DMeshView& v = w.view;
  if (int rc = upload(ctx, pool, &v.positions, w.in.positions, (size_t)w.in.vertex_count * 3u)) return rc;
  if (int rc = upload(ctx, pool, &v.indices, w.in.indices, w.in.index_count)) return rc;
  v.bvh_node_count = w.node_count;
  if (w.dev_packed) {
    pool.push_back(w.dev_packed);
    v.bvh = w.dev_packed;
    w.dev_packed = nullptr;
    return PTC_OK;
  }
  std::vector<float4> packed((size_t)w.node_count * 2u);
  for (uint32_t i = 0; i < w.node_count; ++i) {
    const ptc_bvh_node& node = w.nodes[i];
    float fbits, cbits;
    std::memcpy(&fbits, &node.first_child_or_primitive, 4);
    std::memcpy(&cbits, &node.primitive_count, 4);
    packed[2u * i] = make_float4(node.aabb_min[0], node.aabb_min[1], node.aabb_min[2], fbits);
    packed[2u * i + 1u] = make_float4(node.aabb_max[0], node.aabb_max[1], node.aabb_max[2], cbits);
  }
  return upload(ctx, pool, &v.bvh, packed.data(), packed.size());
}

// The layouts of one mesh for the fast traversals (wide inner records, the four-wide quantised tree, the depth-first leaf
// order), derived on the device or on the host and uploaded -- the same bytes; the leaf order stays where it was made.
// Either side leaves the arrays in the mesh's view and the numbers in one DeviceLayouts.
int mesh_layouts(ptc_ctx* ctx, NewScene& n, MeshWork& w)
{
  std::vector<void*>& pool = n.scene_allocs;
  DeviceLayouts lay;
  DMeshView& v = w.view;
  if (w.layouts_on_device) {
    const int rc = build_layouts_device(ctx->stream, w.view.bvh, w.node_count, w.level_base, &lay);
    for (void* q : {(void*)lay.nodes_q, (void*)lay.leaf_parent, (void*)lay.tri_order, (void*)lay.wide})
      if (q) pool.push_back(q);
    if (rc) return fail(ctx, rc, "traversal layouts failed on the device");
    v.wide = lay.wide;
    v.leaf_parent = lay.leaf_parent;
    v.bvh4q = reinterpret_cast<const uint4*>(lay.nodes_q);
    w.tri_order_dev = lay.tri_order;
    n.upload_times.layout_on_device = 1u;
    n.lap(n.upload_times.layout_ms);
  } else {
    WideAccel wa;
    if (int rc = build_wide(w.nodes, w.node_count, wa)) return fail(ctx, rc, "wide BVH layout failed");
    Wide4Accel w4;
    if (int rc = build_wide4(w.nodes, w.node_count, w4)) return fail(ctx, rc, "four-wide BVH layout failed");
    n.lap(n.upload_times.layout_ms);
    const uint32_t* nodes_q = nullptr;
    if (int rc = upload(ctx, pool, &v.wide, wa.wide.data(), wa.wide.size())) return rc;
    if (int rc = upload(ctx, pool, &v.leaf_parent, w4.leaf_parent.data(), w4.leaf_parent.size())) return rc;
    if (int rc = upload(ctx, pool, &nodes_q, w4.nodes_q.data(), w4.nodes_q.size())) return rc;
    v.bvh4q = reinterpret_cast<const uint4*>(nodes_q);
    lay.root_ref4 = w4.root_ref, lay.dummy_ref = w4.dummy_ref, lay.root_ref2 = wa.root_ref;
    std::memcpy(lay.root_min, wa.root_min, sizeof lay.root_min);
    std::memcpy(lay.root_max, wa.root_max, sizeof lay.root_max);
    lay.wide4_depth = w4.depth, lay.wide4_nodes = w4.node_count;
    w.tri_order_host = std::move(wa.tri_order);
    n.lap(n.upload_times.copy_ms);
  }
  v.bvh4_root = lay.root_ref4;
  v.dummy_ref = lay.dummy_ref;
  v.root_ref = lay.root_ref2;
  std::memcpy(v.root_min, lay.root_min, sizeof v.root_min);
  std::memcpy(v.root_max, lay.root_max, sizeof v.root_max);
  w.w4_depth = lay.wide4_depth;
  w.w4_nodes = lay.wide4_nodes;
  return PTC_OK;
}

// DScene::tris: per mesh object the world-space triangle records of its instance in depth-first order, from the side that
// holds the leaf order; and DScene::object_tri_base
int instance_triangles(ptc_ctx* ctx, const ptc_scene_desc* s, const std::vector<MeshWork>& meshes, NewScene& n)
{
  float4* tris = nullptr;
  if (int rc = dev_alloc(ctx, n.scene_allocs, &tris, n.tri_records * kTriVec4)) return rc;
  if (n.tri_records) HIP_TRY(ctx, hipMemsetAsync(tris, 0, n.tri_records * kTriVec4 * sizeof(float4), ctx->stream));
  std::vector<float4> host_tris;
  for (uint32_t i = 0; i < s->object_count; ++i) {
    if (s->objects[i].type != 1u || n.object_mesh[i] >= meshes.size()) continue;
    const MeshWork& w = meshes[n.object_mesh[i]];
    if (w.triangles == 0u) continue;
    m4 m;
    std::memcpy(&m, s->objects[i].m, sizeof m);
    float4* dst = tris + (size_t)n.tri_base[i] * kTriVec4;
    if (w.tri_order_dev) {
      launch_instance_triangles(ctx->stream, m, w.view.positions, w.view.indices, w.tri_order_dev, w.triangles, dst);
    } else {
      host_tris.assign((size_t)w.triangles * kTriVec4, make_float4(0.f, 0.f, 0.f, 0.f));
      build_instance_triangles(m, w.in.positions, w.in.indices, w.tri_order_host, host_tris.data());
      HIP_TRY(ctx, hipMemcpyAsync(dst, host_tris.data(), host_tris.size() * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  n.scene.tris = tris;
  n.layout_counts[2] = (uint64_t)n.tri_records * 16u * kTriVec4;  // bytes of tris, all instances (ptc_download_layout)
  return upload(ctx, n.scene_allocs, &n.scene.object_tri_base, n.tri_base.data(), n.tri_base.size());
}

// what the scene holds over all its meshes: their views (host and device), the object -> mesh table, the sizes of mesh 0's
// arrays (ptc_download_layout) and the stack need of the four-wide walk
int mesh_tables(ptc_ctx* ctx, const std::vector<MeshWork>& meshes, NewScene& n)
{
  DScene& d = n.scene;
  for (const MeshWork& w : meshes) {
    n.mesh_views.push_back(w.view);
    n.mesh_nodes4.push_back(w.w4_nodes);
    if (!w.node_count) continue;
    // up to three entries per level; whatever exceeds the LDS part goes to the per-thread overflow area (DScene::spill)
    const uint32_t need4 = 3u * w.w4_depth + 2u > d.lds_cap ? 3u * w.w4_depth + 2u - d.lds_cap : 0u;
    d.spill_cap = std::max(d.spill_cap, need4);
  }
  if (int rc = upload(ctx, n.scene_allocs, &d.mesh_views, n.mesh_views.data(), n.mesh_views.size())) return rc;
  if (int rc = upload(ctx, n.scene_allocs, &d.object_mesh, n.object_mesh.data(), n.object_mesh.size())) return rc;
  if (int rc = upload(ctx, n.scene_allocs, &n.mesh_first_vertex, n.first_vertex.data(), n.first_vertex.size())) return rc;
  if (int rc = upload(ctx, n.scene_allocs, &n.mesh_first_index, n.first_index.data(), n.first_index.size())) return rc;
  if (meshes.empty()) return PTC_OK;
  d.cur = n.mesh_views[0];
  const uint64_t t0 = meshes[0].triangles, n0 = meshes[0].node_count;
  n.layout_counts[0] = (uint64_t)meshes[0].w4_nodes * 64u;  // bvh4q
  n.layout_counts[1] = n0 ? (t0 + 1u) * 32u : 0u;           // leaf_parent
  n.layout_counts[3] = n0 ? (t0 - 1u) * 64u : 0u;           // wide
  n.layout_counts[4] = n0 * 32u;                            // bvh
  return PTC_OK;
}

}  // namespace

// gives one array of the scene's pool back (the textures' and the normal maps' replaced arrays)
template <typename T>
static void drop_scene_array(ptc_ctx* ctx, T*& p)
{
  if (!p) return;
  auto& pool = ctx->scene_allocs;
  pool.erase(std::remove(pool.begin(), pool.end(), (void*)p), pool.end());
  (void)hipFree(p);
  p = nullptr;
}

extern "C" {

int ptc_upload_scene(ptc_ctx* ctx, const ptc_scene_desc* s)
{
  if (!ctx || !s) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = validate_scene(ctx, s)) return rc;
  NewScene n;
  std::vector<MeshWork> meshes(mesh_count_of(s));
  for (uint32_t m = 0; m < meshes.size(); ++m) meshes[m].in = mesh_slice(s, m);

  // ---- what can refuse the scene while the old one is intact, in this order: a vertex in use that is not finite (the rule:
  // pt_host.hpp); every caller tree, before any device work; per mesh its reference BVH; the host's own preparation
  for (uint32_t m = 0; m < meshes.size(); ++m) {
    const MeshSlice& in = meshes[m].in;
    const int64_t v = first_non_finite_vertex(in.positions, in.vertex_count, in.indices, in.index_count);
    if (v >= 0)
      return fail(ctx, PTC_ERR_INVALID, "mesh " + std::to_string(m) + ": vertex " + std::to_string(v) + " has a NaN or infinite coordinate");
  }
  for (const MeshWork& w : meshes)
    if (w.in.index_count != 0u && w.in.caller_bvh)
      if (int rc = validate_bvh(ctx, w.in)) return rc;
  for (MeshWork& w : meshes)
    if (int rc = reference_bvh(ctx, w, n)) return rc;
  if (int rc = stage_host(ctx, s, meshes, n)) return rc;

  // ---- the old scene goes, before the new one's allocations.  Iterations queued or in flight were asked for against it:
  // trace them first.  From here to the commit the context holds no scene, and a failure leaves it so (~NewScene)
  if (int rc = sync_frames(ctx)) return rc;
  free_pool(ctx->scene_allocs);
  static_cast<ptc_scene_state&>(*ctx) = ptc_scene_state{};
  ++ctx->scene_serial;

  if (int rc = upload_tables(ctx, s, n)) return rc;
  n.lap(n.upload_times.copy_ms);
  for (MeshWork& w : meshes) {
    if (int rc = mesh_arrays(ctx, n, w)) return rc;
    n.lap(n.upload_times.copy_ms);
    if (int rc = mesh_layouts(ctx, n, w)) return rc;
  }
  if (int rc = instance_triangles(ctx, s, meshes, n)) return rc;
  n.lap(n.upload_times.triangles_ms);
  if (int rc = mesh_tables(ctx, meshes, n)) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, PTC_ERR_HIP, "scene upload failed");
  n.lap(n.upload_times.copy_ms);

  // ---- the commit: nothing above assigned a scene-describing field of the context, nothing below can fail
  n.upload_times.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - n.start).count();
  n.has_scene = true;
  std::swap(static_cast<ptc_scene_state&>(*ctx), static_cast<ptc_scene_state&>(n));
  return PTC_OK;
}

int ptc_build_bvh_device(ptc_ctx* ctx, const float* positions, uint32_t vertex_count, const uint32_t* indices,
                         uint32_t index_count, ptc_bvh_node* nodes, uint32_t* max_depth)
{
  if (!ctx || !positions || !indices || !nodes || index_count % 3u != 0u) return fail(ctx, PTC_ERR_INVALID, "bad arguments");
  if (int rc = bind_device(ctx)) return rc;
  if (first_index_out_of_range(indices, index_count, vertex_count) >= 0) return fail(ctx, PTC_ERR_INVALID, "vertex index out of range");
  if (const int64_t v = first_non_finite_vertex(positions, vertex_count, indices, index_count); v >= 0)
    return fail(ctx, PTC_ERR_INVALID, "vertex " + std::to_string(v) + " has a NaN or infinite coordinate");
  return bvh_on_device(ctx, {positions, vertex_count, indices, index_count, nullptr, 0u}, nodes, max_depth, nullptr);
}

int ptc_download_layout(ptc_ctx* ctx, int which, void* host, uint64_t capacity, uint64_t* bytes)
{
  if (!ctx || which < 0 || which > 4) return fail(ctx, PTC_ERR_INVALID, "layout: 0 bvh4q, 1 leaf_parent, 2 tris, 3 wide, 4 bvh");
  if (!ctx->has_scene) return fail(ctx, PTC_ERR_NO_SCENE, "no scene uploaded");
  if (int rc = bind_device(ctx)) return rc;
  const void* src[5] = {ctx->scene.cur.bvh4q, ctx->scene.cur.leaf_parent, ctx->scene.tris, ctx->scene.cur.wide, ctx->scene.cur.bvh};
  const uint64_t n = ctx->layout_counts[which];
  if (bytes) *bytes = n;
  if (!host) return PTC_OK;
  if (capacity < n) return fail(ctx, PTC_ERR_INVALID, "buffer too small");
  if (n) HIP_TRY(ctx, hipMemcpy(host, src[which], n, hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_get_upload_times(const ptc_ctx* ctx, ptc_upload_times* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  *out = ctx->upload_times;
  return PTC_OK;
}

int ptc_light_table(const ptc_scene_desc* scene, ptc_light* out, uint32_t capacity, ptc_light_info* info)
{
  if (!scene || !out) return fail(nullptr, PTC_ERR_INVALID, "scene or out is NULL");
  if (int rc = validate_scene(nullptr, scene)) return rc;
  std::vector<ptc_light> lights;
  ptc_light_info li{};
  std::string err;
  if (int rc = build_light_table(scene, lights, &li, nullptr, &err, nullptr)) return fail(nullptr, rc, err);
  if (lights.size() > capacity)
    return fail(nullptr, PTC_ERR_INVALID, "capacity " + std::to_string(capacity) + " is too small for " + std::to_string(lights.size()) + " lamp primitives");
  if (!lights.empty()) std::memcpy(out, lights.data(), lights.size() * sizeof(ptc_light));
  if (info) *info = li;
  return (int)lights.size();
}

int ptc_light_material_pdf(const ptc_scene_desc* scene, float* out, uint32_t capacity)
{
  if (!scene || !out) return fail(nullptr, PTC_ERR_INVALID, "scene or out is NULL");
  if (int rc = validate_scene(nullptr, scene)) return rc;
  std::vector<ptc_light> lights;
  ptc_light_info li{};
  std::string err;
  if (int rc = build_light_table(scene, lights, &li, nullptr, &err, nullptr)) return fail(nullptr, rc, err);
  if (scene->material_count > capacity)
    return fail(nullptr, PTC_ERR_INVALID, "capacity " + std::to_string(capacity) + " is too small for " + std::to_string(scene->material_count) + " materials");
  std::vector<float> pdf;
  light_material_pdf(scene, li.total_weight, pdf);
  if (!pdf.empty()) std::memcpy(out, pdf.data(), pdf.size() * sizeof(float));
  return (int)pdf.size();
}

int ptc_get_light_info(ptc_ctx* ctx, ptc_light_info* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (!ctx->has_scene) return fail(ctx, PTC_ERR_NO_SCENE, "no scene uploaded");
  *out = ctx->light_info;
  return PTC_OK;
}

// Vertex normals beside the scene.  Every refusal comes before anything is touched; the device array joins the
// scene's pool, so the scene's one release path (ptc_upload_scene: free_pool, then a value-initialised ptc_scene_state) takes it.
int ptc_set_vertex_normals(ptc_ctx* ctx, const float* normals, uint32_t vertex_count)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!ctx->has_scene) return fail(ctx, PTC_ERR_NO_SCENE, "no scene uploaded");
  if ((normals == nullptr) != (vertex_count == 0u)) return fail(ctx, PTC_ERR_INVALID, "vertex normals: NULL and 0 go together (they remove the normals)");
  if (normals && vertex_count != ctx->vertex_count)
    return fail(ctx, PTC_ERR_INVALID, "vertex normals: " + std::to_string(vertex_count) + " normals for a scene of " + std::to_string(ctx->vertex_count) +
                                          " vertices");
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;  // frames queued or in flight were asked for with what was set
  if (!normals) {
    ctx->normals_set = false;
    return PTC_OK;
  }
  if (!ctx->vertex_normals)
    if (int rc = dev_alloc(ctx, ctx->scene_allocs, &ctx->vertex_normals, 3u * (size_t)vertex_count)) return rc;
  HIP_TRY(ctx, hipMemcpy(ctx->vertex_normals, normals, 3u * (size_t)vertex_count * sizeof(float), hipMemcpyHostToDevice));
  ctx->normals_set = true;
  return PTC_OK;
}

int ptc_get_vertex_normals(const ptc_ctx* ctx, uint32_t* vertex_count)
{
  const bool set = ctx && ctx->has_scene && ctx->normals_set;
  if (vertex_count) *vertex_count = set ? ctx->vertex_count : 0u;
  return set ? 1 : 0;
}

// Texture coordinates beside the scene: ptc_set_vertex_normals' shape, two floats per corner.
int ptc_set_texcoords(ptc_ctx* ctx, const float* st, uint32_t index_count)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!ctx->has_scene) return fail(ctx, PTC_ERR_NO_SCENE, "no scene uploaded");
  if ((st == nullptr) != (index_count == 0u)) return fail(ctx, PTC_ERR_INVALID, "texture coordinates: NULL and 0 go together (they remove the coordinates)");
  if (st && index_count != ctx->index_count)
    return fail(ctx, PTC_ERR_INVALID, "texture coordinates: " + std::to_string(index_count) + " corners for a scene of " +
                                          std::to_string(ctx->index_count) + " indices");
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;  // frames queued or in flight were asked for with what was set
  if (!st) {
    ctx->texcoords_set = false;
    return PTC_OK;
  }
  if (!ctx->texcoords)
    if (int rc = dev_alloc(ctx, ctx->scene_allocs, &ctx->texcoords, 2u * (size_t)index_count)) return rc;
  HIP_TRY(ctx, hipMemcpy(ctx->texcoords, st, 2u * (size_t)index_count * sizeof(float), hipMemcpyHostToDevice));
  ctx->texcoords_set = true;
  return PTC_OK;
}

int ptc_get_texcoords(const ptc_ctx* ctx, uint32_t* index_count)
{
  const bool set = ctx && ctx->has_scene && ctx->texcoords_set;
  if (index_count) *index_count = set ? ctx->index_count : 0u;
  return set ? 1 : 0;
}

// Textures beside the scene.  Every refusal comes before anything is touched; the new pool, records and binding
// are uploaded beside the old ones and take their place in the scene's pool only when nothing can fail any more.
int ptc_set_textures(ptc_ctx* ctx, const ptc_texture_desc* textures, uint32_t texture_count, const int32_t* material_texture, uint32_t material_count)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!ctx->has_scene) return fail(ctx, PTC_ERR_NO_SCENE, "no scene uploaded");
  if ((textures == nullptr) != (texture_count == 0u)) return fail(ctx, PTC_ERR_INVALID, "textures: NULL and 0 go together (they remove the textures)");
  std::vector<texmap::Record> records;
  uint64_t texels = 0;
  if (textures) {
    if (material_count != ctx->material_count)
      return fail(ctx, PTC_ERR_INVALID, "textures: " + std::to_string(material_count) + " bindings for a scene of " + std::to_string(ctx->material_count) +
                                            " materials");
    if (material_count && !material_texture) return fail(ctx, PTC_ERR_INVALID, "textures: material_texture is NULL");
    for (uint32_t i = 0; i < texture_count; ++i) {
      const std::string why = texture_refusal(textures[i]);
      if (!why.empty()) return fail(ctx, PTC_ERR_INVALID, "texture " + std::to_string(i) + " " + why);
      records.push_back(texmap::Record{(uint32_t)texels, textures[i].width, textures[i].height,
                                        texmap::pack_flags(textures[i].encoding, textures[i].filter, textures[i].wrap)});
      texels += (uint64_t)textures[i].width * textures[i].height;
      if (texels * 4u > (1ull << 30)) return fail(ctx, PTC_ERR_INVALID, "textures: the pool exceeds 1 GiB at texture " + std::to_string(i));
    }
    for (uint32_t m = 0; m < material_count; ++m)
      if (material_texture[m] < -1 || material_texture[m] >= (int64_t)texture_count)
        return fail(ctx, PTC_ERR_INVALID, "textures: material " + std::to_string(m) + " is bound to texture " + std::to_string(material_texture[m]) +
                                              " of " + std::to_string(texture_count));
  }
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;  // frames queued or in flight were asked for with what was set
  auto drop = [&](auto*& p) { drop_scene_array(ctx, p); };
  if (!textures) {
    drop(ctx->tex_texels);
    drop(ctx->tex_records);
    drop(ctx->tex_material);
    drop(ctx->nmap_material);  // its indices named this pool
    ctx->nmap_bound = 0;
    ctx->nmaps_set = false;
    ctx->texture_count = 0;
    ctx->texel_count = 0;
    ctx->textures_set = false;
    return PTC_OK;
  }
  std::vector<void*> fresh;
  struct Guard {
    std::vector<void*>& p;
    ~Guard() { free_pool(p); }
  } guard{fresh};
  uint32_t* d_texels = nullptr;
  texmap::Record* d_records = nullptr;
  int32_t* d_material = nullptr;
  float* d_table = nullptr;
  if (int rc = dev_alloc(ctx, fresh, &d_texels, (size_t)texels)) return rc;
  if (int rc = dev_alloc(ctx, fresh, &d_records, records.size())) return rc;
  if (int rc = dev_alloc(ctx, fresh, &d_material, std::max<size_t>(material_count, 1u))) return rc;
  if (!ctx->tex_table)
    if (int rc = dev_alloc(ctx, fresh, &d_table, 2u * (size_t)texmap::kTableEntries)) return rc;
  for (uint32_t i = 0; i < texture_count; ++i)
    HIP_TRY(ctx, hipMemcpy(d_texels + records[i].offset, textures[i].rgba8, (size_t)records[i].width * records[i].height * 4u, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(d_records, records.data(), records.size() * sizeof(texmap::Record), hipMemcpyHostToDevice));
  if (material_count) HIP_TRY(ctx, hipMemcpy(d_material, material_texture, material_count * sizeof(int32_t), hipMemcpyHostToDevice));
  if (d_table) {
    float table[2u * texmap::kTableEntries];
    texmap::decode_table(texmap::kLinear, table);
    texmap::decode_table(texmap::kSrgb, table + texmap::kTableEntries);
    HIP_TRY(ctx, hipMemcpy(d_table, table, sizeof table, hipMemcpyHostToDevice));
  }
  // the commit: nothing below can fail
  drop(ctx->tex_texels);
  drop(ctx->tex_records);
  drop(ctx->tex_material);
  drop(ctx->nmap_material);  // its indices named the old pool
  ctx->nmap_bound = 0;
  ctx->nmaps_set = false;
  ctx->scene_allocs.insert(ctx->scene_allocs.end(), fresh.begin(), fresh.end());
  fresh.clear();
  ctx->tex_texels = d_texels;
  ctx->tex_records = d_records;
  ctx->tex_material = d_material;
  if (d_table) ctx->tex_table = d_table;
  ctx->texture_count = texture_count;
  ctx->texel_count = texels;
  ctx->textures_set = true;
  return PTC_OK;
}

int ptc_get_textures(const ptc_ctx* ctx, uint32_t* texture_count, uint64_t* texel_count)
{
  const bool set = ctx && ctx->has_scene && ctx->textures_set;
  if (texture_count) *texture_count = set ? ctx->texture_count : 0u;
  if (texel_count) *texel_count = set ? ctx->texel_count : 0u;
  return set ? 1 : 0;
}

// The normal-map binding beside the textures: ptc_set_textures' shape -- every refusal before anything is touched,
// the new binding uploaded beside the old one
int ptc_set_normal_maps(ptc_ctx* ctx, const int32_t* material_normal_map, uint32_t material_count)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!ctx->has_scene) return fail(ctx, PTC_ERR_NO_SCENE, "no scene uploaded");
  if ((material_normal_map == nullptr) != (material_count == 0u))
    return fail(ctx, PTC_ERR_INVALID, "normal maps: NULL and 0 go together (they remove the binding)");
  uint32_t bound = 0;
  if (material_normal_map) {
    if (!ctx->textures_set) return fail(ctx, PTC_ERR_INVALID, "normal maps: no textures are set (ptc_set_textures first)");
    if (material_count != ctx->material_count)
      return fail(ctx, PTC_ERR_INVALID, "normal maps: " + std::to_string(material_count) + " bindings for a scene of " +
                                            std::to_string(ctx->material_count) + " materials");
    for (uint32_t m = 0; m < material_count; ++m) {
      if (material_normal_map[m] < -1 || material_normal_map[m] >= (int64_t)ctx->texture_count)
        return fail(ctx, PTC_ERR_INVALID, "normal maps: material " + std::to_string(m) + " is bound to texture " +
                                              std::to_string(material_normal_map[m]) + " of " + std::to_string(ctx->texture_count));
      if (material_normal_map[m] >= 0) ++bound;
    }
  }
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;  // frames queued or in flight were asked for with what was set
  auto drop = [&](auto*& p) { drop_scene_array(ctx, p); };
  if (!material_normal_map) {
    drop(ctx->nmap_material);
    ctx->nmap_bound = 0;
    ctx->nmaps_set = false;
    return PTC_OK;
  }
  std::vector<void*> fresh;
  struct Guard {
    std::vector<void*>& p;
    ~Guard() { free_pool(p); }
  } guard{fresh};
  int32_t* d_material = nullptr;
  float* d_table = nullptr;
  if (int rc = dev_alloc(ctx, fresh, &d_material, (size_t)material_count)) return rc;
  if (!ctx->nmap_table)
    if (int rc = dev_alloc(ctx, fresh, &d_table, (size_t)texmap::kTableEntries)) return rc;
  HIP_TRY(ctx, hipMemcpy(d_material, material_normal_map, material_count * sizeof(int32_t), hipMemcpyHostToDevice));
  if (d_table) {
    float table[texmap::kTableEntries];
    nmap::decode_table(table);
    HIP_TRY(ctx, hipMemcpy(d_table, table, sizeof table, hipMemcpyHostToDevice));
  }
  // the commit: nothing below can fail
  drop(ctx->nmap_material);
  ctx->scene_allocs.insert(ctx->scene_allocs.end(), fresh.begin(), fresh.end());
  fresh.clear();
  ctx->nmap_material = d_material;
  if (d_table) ctx->nmap_table = d_table;
  ctx->nmap_bound = bound;
  ctx->nmaps_set = true;
  return PTC_OK;
}

int ptc_get_normal_maps(const ptc_ctx* ctx, uint32_t* bound_materials)
{
  const bool set = ctx && ctx->has_scene && ctx->nmaps_set;
  if (bound_materials) *bound_materials = set ? ctx->nmap_bound : 0u;
  return set ? 1 : 0;
}

int ptc_normal_map_decode_table(float* out256)
{
  if (!out256) return fail(nullptr, PTC_ERR_INVALID, "normal map decode table: out is NULL");
  nmap::decode_table(out256);
  return PTC_OK;
}

int ptc_texture_decode_table(uint32_t encoding, float* out256)
{
  if (!out256) return fail(nullptr, PTC_ERR_INVALID, "texture decode table: out is NULL");
  if (encoding > PTC_TEXTURE_SRGB) return fail(nullptr, PTC_ERR_INVALID, "texture decode table: encoding " + std::to_string(encoding) + " is neither 0 nor 1");
  texmap::decode_table(encoding, out256);
  return PTC_OK;
}

int ptc_compute_vertex_normals(const float* positions, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count, float* normals_out)
{
  if (!normals_out || (vertex_count && !positions) || (index_count && !indices)) return fail(nullptr, PTC_ERR_INVALID, "vertex normals: an array is NULL");
  if (index_count % 3u != 0u) return fail(nullptr, PTC_ERR_INVALID, "vertex normals: index_count is no multiple of 3");
  if (const int64_t i = first_index_out_of_range(indices, index_count, vertex_count); i >= 0)
    return fail(nullptr, PTC_ERR_INVALID, "vertex normals: index " + std::to_string(i) + " names no vertex");
  smooth::vertex_normals(positions, vertex_count, indices, index_count, normals_out);
  return PTC_OK;
}

int ptc_build_bvh(const float* positions, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                  ptc_bvh_node* nodes, uint32_t* max_depth)
{
  if (!positions || !indices || !nodes || index_count % 3u) return PTC_ERR_INVALID;
  return build_bvh(positions, vertex_count, indices, index_count, nodes, max_depth);
}

int ptc_make_object(uint32_t type, uint32_t index, const float* m16, const ptc_sphere* sphere, const float* mesh_aabb6,
                    ptc_object* out)
{
  return make_object(type, index, m16, sphere, mesh_aabb6, out);
}

}  // extern "C"

