// stage_hooks.cpp — the stage-level entry points that read the preprocessed scene: phx_dev_trace, the BSDF, texture, lobe-weight, environment
// and light hooks.  Each runs one kernel of film_hooks.hip / trace.hip on arrays the caller hands in: the tests compare single stages of the
// pipeline with the reference through them, and no frame launches them.
//
// A hook checks its own arguments, stages its arrays (device_internal.h: Staging) and runs its launch; stage_hook() is what they share.
#include "device_internal.h"

using namespace phx;

namespace {

// A stage hook: no exception leaves it, and it needs a preprocessed scene.  `body` does the hook's own argument checks, stages its arrays and runs its launch.
template <typename F>
int stage_hook(phx_device* d, const char* name, F&& body) {
  return guarded([&]() -> int {
    if (!d || !d->preprocessed) return fail(PHX_ERR_STATE, std::string(name) + " before preprocess");
    Staging s{d};
    return body(s);
  });
}

}  // namespace

extern "C" {

int phx_dev_trace(phx_device* d, uint32_t n, const float* o, const float* dir, const float* tmax, int shadow,
                  float* t, float* u, float* v, uint32_t* prim, uint8_t* hit) {
  return stage_hook(d, "trace", [&](Staging& s) -> int {
    if (n == 0) return PHX_OK;
    std::vector<float4> ro(n), rd(n), hh(n);
    for (uint32_t i = 0; i < n; ++i) { ro[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], 0.0f); rd[i] = make_float4(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2], tmax[i]); }
    const float4 *a = s.in(ro.data(), n), *b = s.in(rd.data(), n); float4* c = s.out(hh.data(), n);
    if (const int rc = s.run([&] { launch_trace_rays(d->stream, d->scene, n, a, b, c, shadow); })) return rc;
    for (uint32_t i = 0; i < n; ++i) {  // k_trace_rays stores the primitive id (scene_t::triangles() order) in w, 0xffffffff on a miss
      const uint32_t tri = bits_of(hh[i].w);
      if (t) t[i] = hh[i].x;
      if (u) u[i] = hh[i].y;
      if (v) v[i] = hh[i].z;
      if (prim) prim[i] = tri;
      if (hit) hit[i] = tri != 0xffffffffu;
    }
    return PHX_OK;
  });
}

int phx_dev_bsdf_f(phx_device* d, uint32_t material, uint32_t n, const float* n3, const float* wi3, const float* wo3, float* f3) {
  return stage_hook(d, "bsdf_f", [&](Staging& s) -> int {
    if (material >= d->tables.num_materials) return fail(PHX_ERR_ARG, "material out of range");
    if (d->tables.mat_masked[material]) return fail(PHX_ERR_ARG, "bsdf_f: the material has image-masked lobes, whose weights need the hit's (s, t) (see phx_dev_lobe_weights)");
    if (n == 0) return PHX_OK;
    const size_t n3s = 3 * (size_t)n;
    const float *a = s.in(n3, n3s), *b = s.in(wi3, n3s), *c = s.in(wo3, n3s); float* f = s.out(f3, n3s);
    return s.run([&] { launch_bsdf_f(d->stream, d->tables.d_materials.p + material, n, a, b, c, f); });
  });
}

int phx_dev_bsdf_sample(phx_device* d, uint32_t material, uint32_t n, const float* n3, const float* wi3, const float* u2,
                        float* wo3, float* f3, float* pdf, uint32_t* flags) {
  return stage_hook(d, "bsdf_sample", [&](Staging& s) -> int {
    if (material >= d->tables.num_materials) return fail(PHX_ERR_ARG, "material out of range");
    if (d->tables.mat_masked[material]) return fail(PHX_ERR_ARG, "bsdf_sample: the material has image-masked lobes, whose weights need the hit's (s, t) (see phx_dev_lobe_weights)");
    if (n == 0) return PHX_OK;
    const size_t n3s = 3 * (size_t)n;
    const float *a = s.in(n3, n3s), *b = s.in(wi3, n3s), *c = s.in(u2, 2 * (size_t)n);
    float *wo = s.out(wo3, n3s), *f = s.out(f3, n3s), *p = s.out(pdf, n); uint32_t* fl = s.out(flags, n);
    return s.run([&] { launch_bsdf_sample(d->stream, d->tables.d_materials.p + material, n, a, b, c, wo, f, p, fl); });
  });
}

int phx_dev_texture_lookup(phx_device* d, uint32_t texture, uint32_t n, const float* st, float* rgb) {
  return stage_hook(d, "texture_lookup", [&](Staging& s) -> int {
    if (texture >= d->tables.num_textures) return fail(PHX_ERR_ARG, "texture out of range (textures are kept only for scenes with a textured lobe)");
    if (n == 0) return PHX_OK;
    if (!st || !rgb) return fail(PHX_ERR_ARG, "texture_lookup: null argument");
    const float* a = s.in(st, 2 * (size_t)n); float* o = s.out(rgb, 3 * (size_t)n);
    return s.run([&] { launch_texture_lookup(d->stream, d->tables.d_textures.p, d->tables.d_texels.p, texture, n, a, o); });
  });
}

int phx_dev_lobe_weights(phx_device* d, uint32_t material, uint32_t n, const float* n3, const float* wi3, const float* st, float* w, uint32_t* kept) {
  return stage_hook(d, "lobe_weights", [&](Staging& s) -> int {
    if (material >= d->tables.num_materials) return fail(PHX_ERR_ARG, "material out of range");
    if (n == 0) return PHX_OK;
    const bool tex = (d->scene.any_tex & SC_TEX_LOBES) != 0;  // the scene's lobes read images: st is needed
    if (!n3 || !wi3 || !w || !kept || (tex && !st)) return fail(PHX_ERR_ARG, "lobe_weights: null argument");
    const float *a = s.in(n3, 3 * (size_t)n), *b = s.in(wi3, 3 * (size_t)n), *c = tex ? s.in(st, 2 * (size_t)n) : nullptr;
    float* o = s.out(w, 3 * PHX_MAX_LOBES * (size_t)n); uint32_t* k = s.out(kept, n);
    return s.run([&] {
      launch_lobe_weights(d->stream, d->tables.d_materials.p + material, tex ? d->tables.d_textures.p : nullptr, d->tables.d_texels.p, tex ? d->tables.d_lobe_tex.p + 8 * (size_t)material : nullptr,
                          n, a, b, c, o, k);
    });
  });
}

int phx_dev_environment_lookup(phx_device* d, uint32_t n, const float* dirs, float* rgb) {
  return stage_hook(d, "environment_lookup", [&](Staging& s) -> int {
    if (!d->tables.env_tex) return fail(PHX_ERR_ARG, "environment_lookup: the scene's environment has no image");
    if (n == 0) return PHX_OK;
    if (!dirs || !rgb) return fail(PHX_ERR_ARG, "environment_lookup: null argument");
    const float* a = s.in(dirs, 3 * (size_t)n); float* o = s.out(rgb, 3 * (size_t)n);
    return s.run([&] { launch_environment_lookup(d->stream, d->tables.d_textures.p, d->tables.d_texels.p, d->tables.env_tex - 1u, d->tables.env_mapping, d->tables.env_e[0], d->tables.env_e[1], d->tables.env_e[2], n, a, o); });
  });
}

int phx_dev_light_sample(phx_device* d, uint32_t n, const float* u3, uint32_t* light, uint32_t* tri, float* bary, float* P, float* pdf) {
  return stage_hook(d, "light_sample", [&](Staging& s) -> int {
    if (n == 0) return PHX_OK;
    if (!u3 || !light || !tri || !bary || !P || !pdf) return fail(PHX_ERR_ARG, "light_sample: null argument");
    const float* a = s.in(u3, 3 * (size_t)n);
    uint32_t *ol = s.out(light, n), *ot = s.out(tri, n); float *ob = s.out(bary, 2 * (size_t)n), *oP = s.out(P, 3 * (size_t)n), *op = s.out(pdf, n);
    return s.run([&] { launch_light_sample(d->stream, d->scene, n, a, ol, ot, ob, oP, op); });
  });
}

int phx_dev_light_emission(phx_device* d, uint32_t n, const float* u3, float* st, float* e) {
  return stage_hook(d, "light_emission", [&](Staging& s) -> int {
    if (n == 0) return PHX_OK;
    if (!u3 || !st || !e) return fail(PHX_ERR_ARG, "light_emission: null argument");
    const float* a = s.in(u3, 3 * (size_t)n);
    float *os = s.out(st, 2 * (size_t)n), *oe = s.out(e, 3 * (size_t)n);
    return s.run([&] { launch_light_emission(d->stream, d->scene, n, a, os, oe); });
  });
}

int phx_dev_environment_sample(phx_device* d, uint32_t n, const float* u3, uint32_t* light, uint32_t* texel, float* st, float* dir, float* pdf, float* e) {
  return stage_hook(d, "environment_sample", [&](Staging& s) -> int {
    if (!(d->scene.any_tex & SC_LIGHTS_ENV)) return fail(PHX_ERR_ARG, "environment_sample: the scene does not sample its environment (light_sampling without PHX_LIGHT_INCLUDE_ENVIRONMENT)");
    if (n == 0) return PHX_OK;
    if (!u3 || !light || !texel || !st || !dir || !pdf || !e) return fail(PHX_ERR_ARG, "environment_sample: null argument");
    const float* a = s.in(u3, 3 * (size_t)n);
    uint32_t *ol = s.out(light, n), *ot = s.out(texel, 2 * (size_t)n);
    float *os = s.out(st, 2 * (size_t)n), *od = s.out(dir, 3 * (size_t)n), *op = s.out(pdf, n), *oe = s.out(e, 3 * (size_t)n);
    return s.run([&] { launch_environment_sample(d->stream, d->scene, d->tables.env_e[0], d->tables.env_e[1], d->tables.env_e[2], n, a, ol, ot, os, od, op, oe); });
  });
}

}  // extern "C"
