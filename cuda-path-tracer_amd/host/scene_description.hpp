// scene_description.hpp -- C++ host mirror of the reference's SceneDescription and asset front-end
// (/root/reference/src/lib/scene_description.{hpp,cpp}, camera.hpp, material.hpp, mesh.hpp, sphere.hpp,
// assets/json_parser.cpp, assets/model_loader.cpp), reduced to what feeds the render core.  No glm, assimp or
// nlohmann: the few matrix functions, a small JSON reader and an OBJ reader are written out here.
#pragma once

#include <array>
#include <cstdint>
#include <map>
#include <string>
#include <variant>
#include <vector>

#include "../../include/ptcore.h"
#include "hdr_image.hpp"

namespace hip_pt {

using Mat4 = std::array<float, 16>;  // column-major like glm: m[4*col + row]

Mat4 identity();
Mat4 translate(float x, float y, float z);                         // glm::translate(vec3)
Mat4 scale(float x, float y, float z);                             // glm::scale(vec3)
Mat4 rotate(float angle_rad, float ax, float ay, float az);        // glm::rotate(angle, axis)
Mat4 look_at(const float from[3], const float at[3], const float up[3]);  // json_parser.cpp:57-70
Mat4 multiply(const Mat4& a, const Mat4& b);                       // glm mat4 * mat4

// a material's "texture" in a scene file (an extension): the picture (a PNG; file empty: none) and how it is looked
// up, ptc_texture_desc's enum values
struct TextureSource {
  std::string file;
  uint32_t encoding = PTC_TEXTURE_SRGB, filter = PTC_TEXTURE_BILINEAR, wrap = PTC_TEXTURE_REPEAT;
  bool operator==(const TextureSource& o) const { return file == o.file && encoding == o.encoding && filter == o.filter && wrap == o.wrap; }
};
// (normal_map: a material's "normal_map"; its encoding is not read)
struct DiffuseMateral { float albedo[3]; TextureSource texture{}; TextureSource normal_map{}; };                 // (sic) material.hpp:6-8
struct MetalMaterial { float albedo[3]; float fuzz; TextureSource texture{}; TextureSource normal_map{}; };      // material.hpp:10-13
struct DielectricMaterial { float refraction_index; };      // material.hpp:15-17
struct EmissiveMaterial { float emission[3]; };             // an extension (the reference has no emitters): ptc_material type 3
using Material = std::variant<DiffuseMateral, MetalMaterial, DielectricMaterial, EmissiveMaterial>;

struct Sphere { float center[3] = {0, 0, 0}; float radius = 0; };  // sphere.hpp:8-11

struct Mesh {  // mesh.hpp:9-18
  std::vector<float> positions;    // xyz per vertex
  std::vector<uint32_t> indices;
  // texture coordinates (an extension): one (s, t) pair per triangle CORNER, parallel to indices (a corner without
  // a `vt` has (0, 0)); empty: the file has no `vt` record
  std::vector<float> texcoords;
  float aabb_min[3] = {0, 0, 0}, aabb_max[3] = {0, 0, 0};
  [[nodiscard]] size_t triangle_count() const { return indices.size() / 3; }
};

struct Camera {  // camera.hpp:17-23
  float position[3] = {0, 0, 0};
  float rotation_wxyz[4] = {1, 0, 0, 0};
  float vfov = 1.57079632679f;
  // the thin lens (an extension: the reference's camera is a pinhole), PathTracer::lens's two values.  Not part
  // of ptc_camera: the lens is the context's (ptc_set_lens).  0 / 0: no lens, none given
  float lens_radius = 0.0f;
  float focus_distance = 0.0f;
  [[nodiscard]] ptc_camera to_c() const
  {
    return ptc_camera{{position[0], position[1], position[2]},
                      {rotation_wxyz[0], rotation_wxyz[1], rotation_wxyz[2], rotation_wxyz[3]}, vfov};
  }
};

// what build_scene() hands to ptc_upload_scene: the reference's six cudaMemcpy sources
struct FlatScene {
  std::vector<ptc_object> objects;
  std::vector<uint32_t> object_material_indices;
  std::vector<ptc_sphere> spheres;
  std::vector<ptc_material> materials;
  std::vector<float> positions;
  std::vector<uint32_t> indices;
  // image textures (an extension; PathTracer::create_buffers sets them): texcoords two floats per corner, parallel to
  // indices (empty: the mesh has none); textures: the distinct TextureSource of the materials; material_texture: per material -1 or
  // an index into it (empty: no material has one)
  std::vector<float> texcoords;
  std::vector<TextureSource> textures;
  std::vector<int32_t> material_texture;
  // normal maps (an extension): per material -1 or an index into `textures` (empty: no material has one); a map's
  // picture stands in `textures` once per (file, filter, wrap), also where it is some material's colour texture
  std::vector<int32_t> material_normal_map;
};

class SceneDescription {  // scene_description.hpp:27-49
public:
  std::string filename;
  Camera camera;
  int resolution[2] = {0, 0};
  int spp = 1;
  // environment lighting (an extension): the octahedral map PathTracer::environment takes, or null (the
  // reference's gradient); environment_source: the scene file's entry it came from (file: absolute; size 0: the picture's height)
  std::shared_ptr<const EnvironmentMap> environment;
  struct EnvironmentSource {
    std::string file;
    float scale = 1.0f;
    int size = 0;
    bool light = false;  // "light": true -- the scene asks for environment light sampling where the method renders it
  } environment_source;
  // smooth shading (an extension): the scene file's "smooth_normals": true -- shade every mesh with interpolated
  // vertex normals, computed from its triangles (the megakernel method renders them)
  bool smooth_normals = false;
  // image textures (an extension): the scene file's "textures": true; has_textures: a material carries a "texture"
  bool textures = false;
  [[nodiscard]] bool has_textures() const;
  // normal maps (an extension): the scene file's "normal_maps": true; has_normal_maps: a material carries a "normal_map"
  bool normal_maps = false;
  [[nodiscard]] bool has_normal_maps() const;

  void add_material(const std::string& name, Material material);
  void add_object(Sphere sphere, const Mat4& transform, const std::string& material_name);
  void add_object(const Mesh& mesh, const Mat4& transform, const std::string& material_name);
  [[nodiscard]] const Mesh* get_mesh(const std::string& name) const;
  const Mesh& add_mesh(std::string name, Mesh&& mesh);
  [[nodiscard]] FlatScene build_scene() const;  // scene_description.cpp:12-117

private:
  struct Object {
    bool is_mesh;
    Sphere sphere;
    Mat4 transform;
  };
  std::vector<Object> objects_;
  std::map<std::string, Material, std::less<>> material_map_;
  std::vector<std::string> objects_material_mapping_;
  std::map<std::string, Mesh, std::less<>> mesh_map_;
};

// assets/json_parser.cpp:174-224 (scene_from_json) and assets/model_loader.cpp:11-44 (load_obj)
// read_environment false: the "environment" key is checked and kept in environment_source, the picture is left to the caller
// (hip_pt, whose command line may name another picture: it reads the one that counts, once)
SceneDescription scene_from_json(const std::string& filename, bool read_environment = true);
Mesh load_obj(const std::string& filename);

// image.cpp:9-22: RGBA8 PNG (the reference calls stbi_write_png)
bool write_png(const std::string& filename, int width, int height, const void* rgba);

}  // namespace hip_pt
