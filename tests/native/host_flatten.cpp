// host_flatten.cpp — flatten_scene (csrc/scene_flatten.cpp) behind a C interface for tests/test_scene_flatten.py, compiled with a plain
// host compiler.  With -DHOST_FLATTEN_MAIN it is a stand-alone program instead, for a run under AddressSanitizer / UBSan: it flattens a
// good scene and one scene per out-of-range index family (the bad index sits at the LAST face, in exactly sized heap arrays, so that an
// unchecked index would read past an allocation) and prints each status.
#include "../../phosphorus_mk2_amd/csrc/scene_flatten.h"

#include <cstdio>

using namespace phx;

namespace {
struct Flat { FlatScene fs; std::string err; int rc = PHX_OK; };
}  // namespace

extern "C" {

void* hf_flatten(const phx_scene* s, const phx_options* opt) {
  Flat* f = new Flat();
  f->rc = flatten_scene(*s, *opt, f->fs, f->err);
  return f;
}
void hf_free(void* h) { delete static_cast<Flat*>(h); }
int hf_status(void* h) { return static_cast<Flat*>(h)->rc; }
const char* hf_error(void* h) { return static_cast<Flat*>(h)->err.c_str(); }

// array `which` -> its address, *bytes its size
const void* hf_array(void* h, int which, uint64_t* bytes) {
  const FlatScene& fs = static_cast<Flat*>(h)->fs;
  auto of = [&](const auto& v) -> const void* { *bytes = v.size() * sizeof(v[0]); return v.data(); };
  switch (which) {
    case 0: return of(fs.abc);
    case 1: return of(fs.prim_material);
    case 2: return of(fs.prim_normals);
    case 3: return of(fs.prim_uv);
    case 4: return of(fs.lights);
    case 5: return of(fs.light_tris);
    case 6: return of(fs.light_cdf);
    case 7: return of(fs.mat_lite);
    case 8: return of(fs.mat_masked);
    case 9: return of(fs.lobe_tex);
    case 10: return of(fs.textures);
    case 11: return of(fs.texels);
    default: *bytes = 0; return nullptr;
  }
}

uint32_t hf_word(void* h, int which) {
  const FlatScene& fs = static_cast<Flat*>(h)->fs;
  switch (which) {
    case 0: return fs.any_smooth;
    case 1: return fs.scene.any_tex;
    case 2: return fs.scene.diffuse_only;
    case 3: return fs.scene.any_per_hit;
    case 4: return fs.scene.num_lights;
    case 5: return fs.env_tex;
    case 6: return (uint32_t)fs.materials.size();
    default: return 0xffffffffu;
  }
}

}  // extern "C"

#ifdef HOST_FLATTEN_MAIN
namespace {

// a textured, smooth floor quad (per-vertex normals and UVs) under an emissive quad; every array a heap allocation of its exact size
struct TestScene {
  std::vector<float> v0, n0, uv0, v1, texels;
  std::vector<uint32_t> f0, f1, set0, set1;
  std::vector<uint8_t> smooth0;
  std::vector<phx_face_set> sets0, sets1;
  std::vector<phx_mesh> meshes;
  std::vector<phx_material> mats;
  std::vector<phx_texture> texs;
  phx_scene s{};
  TestScene() {
    v0 = {-1, 0, -1, 1, 0, -1, 1, 0, -3, -1, 0, -3};
    n0 = {0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0};
    uv0 = {0, 0, 1, 0, 1, 1, 0, 1};
    f0 = {0, 1, 2, 0, 2, 3};
    smooth0 = {1, 1};
    set0 = {0, 1};
    v1 = {-0.5f, 1, -1.5f, -0.5f, 1, -2.5f, 0.5f, 1, -2.5f, 0.5f, 1, -1.5f};
    f1 = {0, 1, 2, 0, 2, 3};
    set1 = {0, 1};
    texels = {0.5f, 0.25f, 0.125f, 1, 1, 1};
    mats.assign(2, phx_material{});
    mats[0].num_lobes = 1; mats[0].lobes[0].type = PHX_LOBE_DIFFUSE;
    for (int c = 0; c < 3; ++c) { mats[0].lobes[0].weight[c] = 0.7f; mats[0].lobes[0].pre_weight[c] = 1.0f; mats[1].emission[c] = 4.0f; }
    mats[0].lobes[0].texture = 1;
    mats[1].is_emitter = 1;
    texs.assign(1, phx_texture{});
    link();
  }
  void link() {  // after any array changed
    sets0.assign(1, phx_face_set{}); sets0[0].material = 0; sets0[0].num_faces = (uint32_t)set0.size(); sets0[0].faces = set0.data();
    sets1.assign(1, phx_face_set{}); sets1[0].material = 1; sets1[0].num_faces = (uint32_t)set1.size(); sets1[0].faces = set1.data();
    meshes.assign(2, phx_mesh{});
    phx_mesh& a = meshes[0];
    a.vertices = v0.data(); a.num_vertices = (uint32_t)v0.size() / 3; a.normals = n0.data(); a.num_normals = (uint32_t)n0.size() / 3;
    a.faces = f0.data(); a.num_faces = (uint32_t)f0.size() / 3; a.smooth = smooth0.data();
    a.flags = PHX_MESH_NORMALS_PER_VERTEX | PHX_MESH_UV_PER_VERTEX; a.num_sets = 1; a.sets = sets0.data(); a.uvs = uv0.data(); a.num_uvs = (uint32_t)uv0.size() / 2;
    phx_mesh& b = meshes[1];
    b.vertices = v1.data(); b.num_vertices = (uint32_t)v1.size() / 3; b.faces = f1.data(); b.num_faces = (uint32_t)f1.size() / 3;
    b.flags = a.flags; b.num_sets = 1; b.sets = sets1.data();
    texs[0].width = 2; texs[0].height = 1; texs[0].texels = texels.data();
    s.num_meshes = 2; s.meshes = meshes.data(); s.num_materials = (uint32_t)mats.size(); s.materials = mats.data();
    s.num_textures = 1; s.textures = texs.data(); s.environment_material = -1;
    s.camera.fov = 1.9f; s.camera.film_width = s.camera.film_height = 8;
    for (int i = 0; i < 4; ++i) s.camera.to_world[5 * i] = 1.0f;
  }
};

int run(const char* name, const TestScene& t, int want, const char* fragment) {
  phx_options opt{};
  FlatScene fs; std::string err;
  const int rc = flatten_scene(t.s, opt, fs, err);
  const bool ok = rc == want && (want == PHX_OK ? fs.prim_material.size() == 4 && fs.lights.size() == 1 : err.find(fragment) != std::string::npos);
  std::printf("%s %d %s\n", name, rc, ok ? "as-expected" : err.c_str());
  return ok ? 0 : 1;
}

template <typename T> void cut(std::vector<T>& v, size_t n) { v = std::vector<T>(v.begin(), v.begin() + n); }  // a new allocation of exactly n

}  // namespace

int main() {
  int bad = 0;
  { TestScene t; bad += run("good", t, PHX_OK, ""); }
  { TestScene t; t.set0.back() = 2; bad += run("face", t, PHX_ERR_ARG, "face index out of range"); }
  { TestScene t; t.f0.back() = 4; bad += run("vertex", t, PHX_ERR_ARG, "vertex index out of range"); }
  { TestScene t; cut(t.n0, 9); t.link(); bad += run("normal", t, PHX_ERR_ARG, "normal index out of range"); }
  { TestScene t; cut(t.uv0, 6); t.link(); bad += run("uv", t, PHX_ERR_ARG, "uv index out of range"); }
  { TestScene t; t.sets1[0].material = 2; bad += run("material", t, PHX_ERR_ARG, "face set material out of range"); }
  return bad;
}
#endif
