// scene_flatten.h — the host-only half of preprocess: everything the device derives from a caller's phx_scene before the first HIP call.
//
// flatten_scene validates the scene (every caller-supplied index is checked here, and nowhere else), lays its triangles out in
// scene_t::triangles() order, bakes the materials and the light table with the fp32 operations bit parity with the oracle depends on, and
// classifies the scene for the shade kernels.  It makes no HIP call and touches no device: <hip/hip_runtime.h> is here for float2 / float4
// alone, so the translation unit also compiles with a plain host compiler (tests/native/host_flatten.cpp).  scene_commit.cpp commits the result.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/phx_xpu.h"
#include "kernels.h"

#include <string>
#include <vector>

namespace phx {

// What a geometry update (flatten_geometry, phx_dev_update_geometry) needs of the committed scene besides the moved scene itself, so that it
// reads no material, lobe, texel or environment image again.  Host memory only; flatten_scene fills it, the device keeps it beside its tables.
struct GeometryFingerprint {
  std::vector<uint32_t> prim_material;  // per primitive: material | smooth << 31
  std::vector<uint8_t> is_emitter;      // per material
  std::vector<DevLight> lights;         // first_tri, num_tris, material and the material's emission as committed (area and lpdf are geometry's)
  std::vector<double> light_power;      // PHX_LIGHT_SELECT_BY_POWER: per light, its weight in the selection table over its area
  double env_mean = 0.0;                // PHX_LIGHT_INCLUDE_ENVIRONMENT: G / (W H) of the environment image
  bool any_smooth = false, any_tex = false, any_mask = false, any_emit_tex = false;
};

struct FlatScene {
  // triangles in scene_t::triangles() order: mesh order x face-set order (scene.cpp:58-62, mesh.cpp:118-128)
  std::vector<float> abc;               // 9 floats per primitive
  std::vector<uint32_t> prim_material;  // material | smooth << 31
  std::vector<float> prim_normals;      // any_smooth: 9 floats per primitive (zero on flat faces)
  std::vector<float2> prim_uv;          // SC_TEX_LOBES: 3 corner UVs per primitive (lobes' images, masks and emitters' images read them)
  bool any_smooth = false;
  std::vector<DevLight> lights;         // one per emissive face set; its triangles are light_tris[first_tri ...] in face order
  std::vector<DevLightTri> light_tris;
  std::vector<float> light_cdf;         // PHX_LIGHTS_BY_AREA: per light triangle, the light's running area up to and including it over the light's area
  std::vector<float> light_pcdf;        // PHX_LIGHT_SELECT_BY_POWER: per light, the running selection probability up to and including it (the last is 1)
  std::vector<DevMaterial> materials;
  std::vector<uint32_t> lobe_tex;       // 8 per material: texture + 1 of baked lobe k
  std::vector<DevMatLite> mat_lite;     // diffuse_only == 2: the 32-byte table
  std::vector<uint8_t> mat_masked;      // per material: some lobe's factor is an image mask
  std::vector<uint32_t> mat_emit_tex;   // per material: the image on its emission + 1 (phx_material.emission_uv_texture), 0 = none
  bool any_emit_tex = false;            // some emitter has one: the scene has SC_TEX_LOBES whatever its lobes
  std::vector<DevTexture> textures;     // the texture table and every texel as RGB + 0: packed only when scene.any_tex & SC_TEX_ANY
  std::vector<float4> texels;
  uint32_t env_tex = 0, env_mapping = 0; float env_e[3] = {0.0f, 0.0f, 0.0f};  // the environment's image (texture + 1, 0 = none), mapping and emission
  // PHX_LIGHT_INCLUDE_ENVIRONMENT: the environment's direction tables, mcdf (H floats) then ccdf (H rows of W), and its interval p_env of the
  // selection table (light_pcdf then has lights.size() + 1 entries); w_env is the weight it entered the table with
  std::vector<float> env_cdf;
  float env_p = 0.0f; double env_w = 0.0;
  // every word of DevScene that needs no device: camera, film, environment, light count, any_tex, diffuse_only, any_per_hit, max_depth.
  // The pointers and the tree's words stay zero for the commit stage.
  DevScene scene{};
  GeometryFingerprint fingerprint;      // flatten_scene only
  float bounds[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // flatten_geometry only: the fp32 min / max of every vertex, lo.xyz hi.xyz
};

// The one statement of how a phx_camera becomes DevScene's camera fields (cam_m, zoom, stepx, stepy, ratio, width, height, aperture_radius,
// focal_distance), with the camera's refusals: flatten_scene and phx_dev_set_camera both read it.  PHX_ERR_ARG leaves `sc` untouched.
int flatten_camera(const phx_camera& c, DevScene& sc, std::string& err);

// PHX_OK, or PHX_ERR_ARG with the reason in `err`; `out` is meaningful only after PHX_OK
int flatten_scene(const phx_scene& s, const phx_options& opt, FlatScene& out, std::string& err);

// The geometry half alone, for a scene that is the committed one (`fp`: its fingerprint, `opt`: its options) with other vertex positions
// and normals: fills abc, prim_material, prim_normals, any_smooth, lights, light_tris, light_cdf, light_pcdf, env_p, env_w and bounds — by the code
// flatten_scene runs, so they are word for word flatten_scene's of the moved scene — and nothing else.  PHX_ERR_ARG, with the reason in
// `err`, when the triangle count, a primitive's material word, the number of lights, a light's triangle count or material, any_smooth or the texture
// classes differ from the fingerprint's, for a vertex that is not finite, and for geometry flatten_scene refuses.  The face index arrays
// are not compared: the triangles given are the triangles rendered.
int flatten_geometry(const phx_scene& s, const phx_options& opt, const GeometryFingerprint& fp, FlatScene& out, std::string& err);

}  // namespace phx
