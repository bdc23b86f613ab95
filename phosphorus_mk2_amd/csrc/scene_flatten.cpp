// scene_flatten.cpp — phx_scene -> FlatScene (scene_flatten.h): validation, primitive-order arrays, baked materials and lights.
// Host code only: no HIP call, no device, no global state.
#include "scene_flatten.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace phx {
namespace {

// microfacet_t::roughness_to_alpha + precompute (src/bsdf/params.hpp:86-99), with the device's logf_
float roughness_to_alpha(float roughness) {
  roughness = std::max(roughness, (float)1e-5);
  float x = logf_(roughness);
  return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}

// -> false: more than 8 lobes or an unknown closure id (fac_mode, textures and masks were validated by the caller)
bool bake_material(const phx_material& m, float sheen_L5, DevMaterial& out, uint32_t* lobe_tex /* 8: texture + 1 per baked lobe */) {
  std::memset(&out, 0, sizeof(out));
  for (int k = 0; k < PHX_MAX_LOBES; ++k) lobe_tex[k] = 0;
  out.is_emitter = m.is_emitter; out.ex = m.emission[0]; out.ey = m.emission[1]; out.ez = m.emission[2];
  out.sheen_L5 = sheen_L5;
  if (m.num_lobes > PHX_MAX_LOBES) return false;
  uint32_t k = 0;
  for (uint32_t i = 0; i < m.num_lobes; ++i) {
    const phx_lobe& s = m.lobes[i];
    DevLobe& l = out.lobes[k];
    l.type = s.type; l.wx = s.weight[0]; l.wy = s.weight[1]; l.wz = s.weight[2];
    // the device lobe holds the mode byte alone; an image mode has no ior and keeps its mask's texture + 1 in that word's bits
    const uint32_t mode = PHX_FAC_MODE(s.fac_mode);
    l.fac_mode = mode; l.fac_ior = mode >= PHX_FAC_TEX_B ? float_of_bits(PHX_FAC_TEXTURE(s.fac_mode)) : s.fac_ior;
    l.px = s.pre_weight[0]; l.py = s.pre_weight[1]; l.pz = s.pre_weight[2];
    if (mode != PHX_FAC_NONE) out.per_hit = 1;
    if (s.texture) { out.tex_lobes |= 1u << k; lobe_tex[k] = s.texture; }
    switch (s.type) {
      case PHX_LOBE_DIFFUSE: l.flags = B_REFLECT | B_DIFFUSE; break;
      case PHX_LOBE_OREN_NAYAR: {  // oren_nayar_t::precompute, params.hpp:36-43
        l.flags = B_REFLECT | B_DIFFUSE;
        const float sg = (float)((double)s.alpha * (kPiD / (double)180.0f));
        const float s2 = sg * sg;
        l.a = 1.0f - (s2 / (2.0f * (s2 + 0.33f)));
        l.b = 0.45f * s2 / (s2 + 0.09f);
        break;
      }
      case PHX_LOBE_REFLECTION: l.flags = B_REFLECT | B_SPECULAR; l.eta = s.eta; break;
      case PHX_LOBE_REFRACTION: l.flags = B_TRANSMIT | B_SPECULAR; l.eta = s.eta; break;
      case PHX_LOBE_MICROFACET:
        l.flags = s.refract ? B_TRANSMIT : B_REFLECT;  // src/bsdf.hpp:70-72
        l.eta = s.eta; l.refract = s.refract;
        l.xalpha = std::min(1.0f, std::max(0.0001f, roughness_to_alpha(s.xalpha)));
        l.yalpha = std::min(1.0f, std::max(0.0001f, roughness_to_alpha(s.yalpha)));
        break;
      case PHX_LOBE_SHEEN: l.flags = B_REFLECT | B_GLOSSY; l.r = s.r; break;
      case PHX_LOBE_TRANSPARENT: l.flags = B_TRANSMIT; break;  // src/material.cpp:98-103
      case PHX_LOBE_EMISSIVE: case PHX_LOBE_BACKGROUND: continue;  // not lobes (material.cpp:240-245)
      default: return false;
    }
    ++k;
  }
  out.num_lobes = k;
  return true;
}

// PHX_LIGHT_SELECT_BY_POWER, the rule of include/phx_xpu.h: the selection table pcdf and every light's lpdf = (1 / area) * p_l.  The weights,
// their sums and the running table are binary64 in the order written (the file is compiled without contraction); pcdf, p_l and lpdf are fp32.
// PHX_LIGHT_INCLUDE_ENVIRONMENT (w_env != nullptr): the environment is one more entry behind the mesh lights, with that weight; its interval
// of the table goes to out.env_p.
// A light's weight is its area times `power[l]` (light_power_factors: what the materials and images contribute, kept with the committed scene so
// that a geometry update rebuilds the table without reading either).
void light_power_table(const std::vector<double>& power, FlatScene& out, const double* w_env = nullptr) {
  const size_t nm = out.lights.size(), nl = nm + (w_env ? 1u : 0u);  // mesh lights, table entries
  std::vector<double> w(nl);
  bool finite = true; size_t npos = 0; double wsum = 0.0;
  for (size_t l = 0; l < nl; ++l) {
    if (l == nm) {
      w[l] = *w_env;
      if (!std::isfinite(w[l])) finite = false;
      if (w[l] > 0.0) ++npos;
      wsum += w[l];
      break;
    }
    w[l] = (double)out.lights[l].area * power[l];
    if (!std::isfinite(w[l])) finite = false;
    if (w[l] > 0.0) ++npos;
    wsum += w[l];
  }
  const bool uniform = !finite || npos == 0;  // a black or broken scene: uniform selection through the same table
  const double phi = PHX_LIGHT_POWER_FLOOR;
  std::vector<double> acc(nl);
  double run = 0.0;
  for (size_t l = 0; l < nl; ++l) {
    const double q = uniform ? 1.0 / (double)nl : (w[l] > 0.0 ? (1.0 - phi) * w[l] / wsum + phi / (double)npos : 0.0);
    run += q; acc[l] = run;
  }
  out.light_pcdf.resize(nl);
  for (size_t l = 0; l < nl; ++l) out.light_pcdf[l] = (float)(acc[l] / acc[nl - 1]);
  for (size_t l = 0; l < nm; ++l) {
    const float p = out.light_pcdf[l] - (l ? out.light_pcdf[l - 1] : 0.0f);
    out.lights[l].lpdf = (1.0f / out.lights[l].area) * p;
  }
  if (w_env) out.env_p = out.light_pcdf[nm] - out.light_pcdf[nm - 1];  // (a scene has at least one mesh light)
}

// per mesh light: (0.2126 |e_r| m_r + 0.7152 |e_g| m_g) + 0.0722 |e_b| m_b, m the channel means of the image on its emission (1 without one)
std::vector<double> light_power_factors(const phx_scene& s, const std::vector<DevLight>& lights) {
  std::vector<double> power(lights.size()), img(3 * (size_t)s.num_textures, -1.0);  // img: an image's channel means, computed at its first use
  for (size_t l = 0; l < lights.size(); ++l) {
    const DevLight& L = lights[l];
    double m[3] = {1.0, 1.0, 1.0};
    if (const uint32_t t = s.materials[L.material].emission_uv_texture) {
      double* mt = &img[3 * (size_t)(t - 1u)];
      if (mt[0] < 0.0 || mt[0] != mt[0]) {  // (a NaN mean is recomputed: it stays NaN)
        const phx_texture& T = s.textures[t - 1u];
        const size_t nt = (size_t)T.width * T.height;
        double sum[3] = {0.0, 0.0, 0.0};
        for (size_t k = 0; k < nt; ++k) for (int c = 0; c < 3; ++c) sum[c] += std::fabs((double)T.texels[3 * k + c]);
        for (int c = 0; c < 3; ++c) mt[c] = sum[c] / (double)nt;
      }
      for (int c = 0; c < 3; ++c) m[c] = mt[c];
    }
    const double er = std::fabs((double)L.ex), eg = std::fabs((double)L.ey), eb = std::fabs((double)L.ez);
    power[l] = (0.2126 * er * m[0] + 0.7152 * eg * m[1]) + 0.0722 * eb * m[2];
  }
  return power;
}

// PHX_LIGHT_INCLUDE_ENVIRONMENT, the rule of include/phx_xpu.h: the importance g of every texel of the environment image T, the direction
// tables out.env_cdf (mcdf, then ccdf row by row) and the environment's weight in the selection table, out.env_w.  One pass over the image,
// one row of g at a time; a black or broken image (G zero or not finite) gets the tables of the uniform sphere in a second pass.
void environment_tables(const phx_scene& s, FlatScene& out) {
  const phx_material& m = s.materials[s.environment_material];
  const phx_texture& T = s.textures[m.emission_texture - 1u];
  const int W = (int)T.width, H = (int)T.height;
  const double e[3] = {std::fabs((double)m.emission[0]), std::fabs((double)m.emission[1]), std::fabs((double)m.emission[2])};
  auto y_at = [&](int i, int j) {
    const float* c = T.texels + 3 * ((size_t)j * (size_t)W + (size_t)i);
    return (0.2126 * (e[0] * std::fabs((double)c[0])) + 0.7152 * (e[1] * std::fabs((double)c[1]))) + 0.0722 * (e[2] * std::fabs((double)c[2]));
  };
  auto yhat = [&](int i, int j) {
    double v = y_at(i, j);
    if (T.filter == PHX_TEX_CLOSEST) return v;
    for (int dj = -1; dj <= 1; ++dj)
      for (int di = -1; di <= 1; ++di) {
        bool outside = false;
        const int x = tex_wrap(i + di, W, T.swrap, outside), y = tex_wrap(j + dj, H, T.twrap, outside);
        const double n = outside ? 0.0 : y_at(x, y);
        if (n > v) v = n;
      }
    return v;
  };
  out.env_cdf.assign((size_t)H + (size_t)H * (size_t)W, 1.0f);
  std::vector<double> g((size_t)W), rowsum((size_t)H);
  auto build = [&](bool sphere) {  // -> G
    double G = 0.0;
    for (int j = 0; j < H; ++j) {
      const double sj = std::sin((kPiD * ((double)j + 0.5)) / (double)H);
      double rs = 0.0;
      for (int i = 0; i < W; ++i) {
        g[(size_t)i] = sphere ? sj : yhat(i, j) * sj;
        G += g[(size_t)i]; rs += g[(size_t)i];
      }
      rowsum[(size_t)j] = rs;
      float* row = out.env_cdf.data() + (size_t)H + (size_t)j * (size_t)W;
      double run = 0.0;
      for (int i = 0; i < W; ++i) { run += g[(size_t)i]; row[i] = rs > 0.0 && std::isfinite(rs) ? (float)(run / rs) : 1.0f; }
    }
    double run = 0.0;
    for (int j = 0; j < H; ++j) { run += rowsum[(size_t)j]; out.env_cdf[(size_t)j] = (float)(run / G); }
    out.env_cdf[(size_t)H - 1] = 1.0f;
    return G;
  };
  const double G = build(false);
  if (!(G > 0.0) || !std::isfinite(G)) build(true);
  out.fingerprint.env_mean = G / ((double)W * (double)H);
}
// the environment's weight in the selection table: the image's share env_mean = G / (W H) (environment_tables) times the area of the sphere
// around the geometry's bounds — the one part of the environment's entry that moves with the geometry
double environment_weight(const std::vector<float>& abc, double env_mean) {
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (size_t k = 0; k < abc.size(); ++k) { lo[k % 3] = std::min(lo[k % 3], abc[k]); hi[k % 3] = std::max(hi[k % 3], abc[k]); }
  const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
  const double R = 0.5 * std::sqrt((dx * dx + dy * dy) + dz * dz);
  return ((((4.0 * kPiD) * R) * R) * env_mean) * (kPiD / 2.0);
}

// Which image lookups the scene's materials ask for, with their refusals: any_tex (some lobe reads an image at the hit's UV — a colour
// texture or a mask — or some emitter's emission does), any_mask, any_emit_tex.  flatten_scene classifies the scene by them; flatten_geometry
// refuses a scene whose classes are not the committed one's.
int texture_classes(const phx_scene& s, bool& any_tex, bool& any_mask, bool& any_emit_tex, std::string& err) {
  auto refuse = [&err](std::string why) { err = std::move(why); return (int)PHX_ERR_ARG; };
  auto material = [](uint32_t i) { return "material " + std::to_string(i); };
  any_tex = any_mask = any_emit_tex = false;
  for (uint32_t i = 0; i < s.num_materials; ++i) {
    const phx_material& m = s.materials[i];
    for (uint32_t k = 0; k < m.num_lobes && k < PHX_MAX_LOBES; ++k) {
      const bool emits = m.is_emitter || (int32_t)i == s.environment_material || m.lobes[k].type == PHX_LOBE_EMISSIVE || m.lobes[k].type == PHX_LOBE_BACKGROUND;
      // an image mask on the closure's mix factor (fac_mode: mode byte + the mask's texture): the same rules as a colour texture
      const uint32_t mode = PHX_FAC_MODE(m.lobes[k].fac_mode), mask = PHX_FAC_TEXTURE(m.lobes[k].fac_mode);
      if (mode > PHX_FAC_TEX_A) return refuse(material(i) + ": unknown fac_mode");
      if (mode < PHX_FAC_TEX_B && mask) return refuse(material(i) + ": fac_mode names a mask texture but its mode is not PHX_FAC_TEX_*");
      if (mode >= PHX_FAC_TEX_B) {
        if (mask == 0 || mask > s.num_textures) return refuse(material(i) + ": mask texture index out of range");
        if (emits) return refuse(material(i) + ": masks on emitters / the environment are not supported");
        any_tex = any_mask = true;
      }
      const uint32_t t = m.lobes[k].texture;
      if (!t) continue;
      if (t > s.num_textures) return refuse(material(i) + ": lobe texture index out of range");
      if (emits) return refuse(material(i) + ": textures on emitters / the environment are not supported");
      any_tex = true;
    }
    // an environment map: only on the environment material (a surface emitter's image is emission_uv_texture, below)
    if (m.emission_mapping > PHX_ENV_LATLONG_Z_UP) return refuse(material(i) + ": unknown emission_mapping");
    if (m.emission_texture) {
      if ((int32_t)i != s.environment_material) return refuse(material(i) + ": emission_texture is allowed only on the environment material");
      if (m.emission_texture > s.num_textures) return refuse(material(i) + ": emission_texture index out of range");
    }
    // an image on a surface emitter's emission, read at mesh UVs (at hits and at next-event estimation's light samples)
    if (m.emission_uv_texture) {
      if ((int32_t)i == s.environment_material) return refuse(material(i) + ": emission_uv_texture is not allowed on the environment material (its image is emission_texture)");
      if (!m.is_emitter) return refuse(material(i) + ": emission_uv_texture is allowed only on emitters");
      if (m.emission_uv_texture > s.num_textures) return refuse(material(i) + ": emission_uv_texture index out of range");
      any_tex = any_emit_tex = true;
    }
  }
  return PHX_OK;
}

// The geometry half of flattening: the triangles in scene_t::triangles() order with their material words, the vertex normals of a scene
// with smooth faces, the corner UVs (with_uv), and per emissive face set a light with its triangles, its area and — by_area — its area CDF.
// is_emitter: per material.  `out` has been reset and out.any_smooth is set.
int walk_geometry(const phx_scene& s, const std::vector<uint8_t>& is_emitter, bool with_uv, bool lights_by_area, FlatScene& out, std::string& err) {
  auto refuse = [&err](std::string why) { err = std::move(why); return (int)PHX_ERR_ARG; };
  for (uint32_t mi = 0; mi < s.num_meshes; ++mi) {
    const phx_mesh& m = s.meshes[mi];
    if (!m.vertices || !m.faces || (m.num_sets && !m.sets) || (with_uv && m.num_uvs && !m.uvs)) return refuse("mesh with null arrays");
    for (uint32_t si = 0; si < m.num_sets; ++si) {
      const phx_face_set& fs = m.sets[si];
      if (fs.material >= is_emitter.size()) return refuse("face set material out of range");
      const bool emitter = is_emitter[fs.material] != 0;
      DevLight L{(uint32_t)out.light_tris.size(), 0, 0.0f, fs.material, 0.0f, 0.0f, 0.0f, 0.0f};
      for (uint32_t k = 0; k < fs.num_faces; ++k) {
        const uint32_t f = fs.faces[k];
        if (f >= m.num_faces) return refuse("face index out of range");
        const uint32_t ia = m.faces[3 * f], ib = m.faces[3 * f + 1], ic = m.faces[3 * f + 2];
        if (ia >= m.num_vertices || ib >= m.num_vertices || ic >= m.num_vertices) return refuse("vertex index out of range");
        const uint32_t prim = (uint32_t)out.prim_material.size();
        const float* a = m.vertices + 3 * (size_t)ia; const float* b = m.vertices + 3 * (size_t)ib; const float* c = m.vertices + 3 * (size_t)ic;
        out.abc.insert(out.abc.end(), a, a + 3); out.abc.insert(out.abc.end(), b, b + 3); out.abc.insert(out.abc.end(), c, c + 3);
        const bool smooth = m.smooth && m.smooth[f];
        out.prim_material.push_back(fs.material | (smooth ? 0x80000000u : 0u));
        if (out.any_smooth) {
          uint32_t na = ia, nb = ib, nc = ic;
          if (!(m.flags & PHX_MESH_NORMALS_PER_VERTEX)) { na = 3 * f; nb = 3 * f + 1; nc = 3 * f + 2; }  // mesh.cpp:188-192
          float nn[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
          if (smooth) {
            if (!m.normals || na >= m.num_normals || nb >= m.num_normals || nc >= m.num_normals) return refuse("normal index out of range");
            std::memcpy(nn, m.normals + 3 * (size_t)na, 12); std::memcpy(nn + 3, m.normals + 3 * (size_t)nb, 12); std::memcpy(nn + 6, m.normals + 3 * (size_t)nc, 12);
          }
          out.prim_normals.insert(out.prim_normals.end(), nn, nn + 9);
        }
        if (with_uv) {  // mesh_t::shading_parameters (mesh.cpp:239-257): UV indices per vertex or per face corner, like the normals; no UVs: (0, 0)
          float2 uv[3] = {make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)};
          if (m.num_uvs) {
            const bool per_vertex = (m.flags & PHX_MESH_UV_PER_VERTEX) != 0;
            const uint32_t ui[3] = {per_vertex ? ia : 3 * f, per_vertex ? ib : 3 * f + 1, per_vertex ? ic : 3 * f + 2};
            for (int c = 0; c < 3; ++c) {
              if (ui[c] >= m.num_uvs) return refuse("uv index out of range");
              uv[c] = make_float2(m.uvs[2 * (size_t)ui[c]], m.uvs[2 * (size_t)ui[c] + 1]);
            }
          }
          out.prim_uv.insert(out.prim_uv.end(), uv, uv + 3);
        }
        if (emitter) {  // mesh_t::preprocess -> light_t::make_area (mesh.cpp:108-116), area_light_t (light.cpp:10-45)
          const v3 ab(b[0] - a[0], b[1] - a[1], b[2] - a[2]), ac(c[0] - a[0], c[1] - a[1], c[2] - a[2]);
          const v3 gn = normalize_inplace(cross(ab, ac));  // the flat face's normal as k_shade's shading_normal would compute it per sample
          DevLightTri T{a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], gn.x, gn.y, gn.z, prim, smooth ? 1u : 0u, mi | (fs.material << 16), 3 * f};
          out.light_tris.push_back(T);
          L.area += 0.5f * length(cross(ab, ac));  // triangle_t::area, mesh.cpp:293-300; summed in face order (light.cpp:36-39)
          L.num_tris++;
          if (lights_by_area) out.light_cdf.push_back(L.area);  // acc_i
        }
      }
      if (emitter && L.num_tris) {
        out.lights.push_back(L);
        for (uint32_t k = 0; k < (lights_by_area ? L.num_tris : 0u); ++k) out.light_cdf[L.first_tri + k] = out.light_cdf[L.first_tri + k] / L.area;  // cdf[i] = acc_i / area; the last is 1
      }
    }
  }
  if (out.prim_material.empty()) return refuse("scene has no triangles");
  if (out.lights.empty()) return refuse("scene has no emissive face set (reference underflows nlights-1, SURVEY A-19)");
  return PHX_OK;
}

// Everything of the light table that hangs on geometry, from the lights walk_geometry left (areas, CDFs) and the committed scene's
// fingerprint (emissions, power factors, the environment's share): per light the pick pdf and the emission of its material, as k_shade
// evaluated them per sample until round 2; then the selection table under PHX_LIGHT_SELECT_BY_POWER, with the environment's entry.
void light_tables(FlatScene& out, const GeometryFingerprint& fp, bool lights_by_power, bool lights_env) {
  const float nlf = (float)out.lights.size();
  for (size_t l = 0; l < out.lights.size(); ++l) {
    DevLight& L = out.lights[l];
    L.lpdf = (1.0f / L.area) / nlf;
    L.ex = fp.lights[l].ex; L.ey = fp.lights[l].ey; L.ez = fp.lights[l].ez;
  }
  if (lights_env) { out.env_w = environment_weight(out.abc, fp.env_mean); light_power_table(fp.light_power, out, &out.env_w); }
  else if (lights_by_power) light_power_table(fp.light_power, out);
}

void scan_smooth(const phx_scene& s, FlatScene& out) {
  for (uint32_t mi = 0; mi < s.num_meshes; ++mi) {
    const phx_mesh& m = s.meshes[mi];
    for (uint32_t f = 0; f < m.num_faces; ++f) if (m.smooth && m.smooth[f]) out.any_smooth = true;
  }
}

}  // namespace

int flatten_camera(const phx_camera& c, DevScene& sc, std::string& err) {
  auto refuse = [&err](std::string why) { err = std::move(why); return (int)PHX_ERR_ARG; };
  // (camera_t's constructor leaves focal_distance uninitialised, entities/camera.hpp:31-36: it means something only behind a lens)
  if (!(std::fabs(c.aperture_radius) <= FLT_MAX) || (c.aperture_radius != 0.0f && !(std::fabs(c.focal_distance) <= FLT_MAX)))
    return refuse("camera: aperture radius / focal distance not finite");
  if (c.film_width == 0 || c.film_height == 0 || c.film_width > 65535 || c.film_height > 65535)
    return refuse("film size out of range");
  std::memcpy(sc.cam_m, c.to_world, sizeof(sc.cam_m));
  sc.zoom = 1.12f * std::tan(c.fov * 0.5f);  // camera.hpp:113
  sc.stepx = 1.0f / (float)c.film_width; sc.stepy = 1.0f / (float)c.film_height;
  sc.ratio = (float)c.film_width / (float)c.film_height;
  sc.width = c.film_width; sc.height = c.film_height;
  sc.aperture_radius = c.aperture_radius; sc.focal_distance = c.focal_distance;  // thin lens iff aperture_radius != 0 (camera_t::is_pinhole)
  return PHX_OK;
}

int flatten_scene(const phx_scene& s, const phx_options& opt, FlatScene& out, std::string& err) {
  auto refuse = [&err](std::string why) { err = std::move(why); return (int)PHX_ERR_ARG; };
  if (!s.meshes || !s.materials || s.num_materials == 0) return refuse("scene without meshes/materials");
  {  // the camera's refusals come here, its fields at the end, where `out` has been reset: one function states both
    DevScene checked{};
    if (const int rc = flatten_camera(s.camera, checked, err)) return rc;
  }
  if (s.environment_material >= (int32_t)s.num_materials) return refuse("environment material out of range");
  // the packed word: the triangle pick in the low byte, the light's selection above it, the environment's bit above that.  Valid: 0, 1, 0x101 and 0x301
  if (PHX_LIGHT_SAMPLING_MODE(opt.light_sampling) > PHX_LIGHTS_BY_AREA) return refuse("unknown light_sampling");
  if (PHX_LIGHT_SELECTION(opt.light_sampling) & ~(uint32_t)(PHX_LIGHT_SELECT_BY_POWER | PHX_LIGHT_INCLUDE_ENVIRONMENT))
    return refuse("unknown light_sampling: bits above PHX_LIGHT_INCLUDE_ENVIRONMENT");
  const bool lights_by_area = PHX_LIGHT_SAMPLING_MODE(opt.light_sampling) == PHX_LIGHTS_BY_AREA;
  const bool lights_by_power = (opt.light_sampling & PHX_LIGHT_SELECT_BY_POWER) != 0;
  const bool lights_env = PHX_LIGHT_ENVIRONMENT(opt.light_sampling) != 0;
  if (lights_by_power && !lights_by_area) return refuse("light_sampling: PHX_LIGHT_SELECT_BY_POWER needs PHX_LIGHTS_BY_AREA");
  if (lights_env && !lights_by_power) return refuse("light_sampling: PHX_LIGHT_INCLUDE_ENVIRONMENT needs PHX_LIGHT_SELECT_BY_POWER");

  // image textures: the table must be well formed whether or not a lobe uses it; a lobe's texture must exist, and only surface closures of
  // non-emitting materials may carry one (an emitter's image is on its emission: emission_uv_texture)
  if (s.num_textures && !s.textures) return refuse("scene with textures but a null texture table");
  uint64_t total_texels = 0;
  for (uint32_t t = 0; t < s.num_textures; ++t) {
    const phx_texture& T = s.textures[t];
    const std::string texture = "texture " + std::to_string(t);
    if (T.width == 0 || T.height == 0) return refuse(texture + " has zero size");
    if (T.width > 65536u || T.height > 65536u || (uint64_t)T.width * T.height > (1ull << 26))
      return refuse(texture + " too large (at most 65536 x 65536 and 2^26 texels)");
    if (!T.texels) return refuse(texture + " without texels");
    if (T.filter > PHX_TEX_CLOSEST || T.swrap > PHX_WRAP_BLACK || T.twrap > PHX_WRAP_BLACK) return refuse(texture + " with an unknown filter or wrap mode");
    total_texels += (uint64_t)T.width * T.height;
  }
  if (total_texels > (1ull << 30)) return refuse("textures too large (at most 2^30 texels in all)");
  bool any_tex = false, any_mask = false, any_emit_tex = false;
  if (const int rc = texture_classes(s, any_tex, any_mask, any_emit_tex, err)) return rc;
  // a constant sky is served by cosine-weighted BSDF sampling; the refusal also keeps the option out of every kernel without the image lookup
  if (lights_env && (s.environment_material < 0 || !s.materials[s.environment_material].emission_texture))
    return refuse("light_sampling: PHX_LIGHT_INCLUDE_ENVIRONMENT needs an environment material with an emission_texture");

  out = FlatScene{};
  GeometryFingerprint& fp = out.fingerprint;
  fp.is_emitter.resize(s.num_materials);
  for (uint32_t i = 0; i < s.num_materials; ++i) fp.is_emitter[i] = s.materials[i].is_emitter != 0;
  scan_smooth(s, out);
  if (const int rc = walk_geometry(s, fp.is_emitter, any_tex, lights_by_area, out, err)) return rc;

  // sheen_L5: the first sheen lobe of the material table (bsdf.h)
  float L5 = 0.0f; bool have = false;
  for (uint32_t i = 0; i < s.num_materials && !have; ++i)
    for (uint32_t k = 0; k < s.materials[i].num_lobes && k < PHX_MAX_LOBES; ++k)
      if (s.materials[i].lobes[k].type == PHX_LOBE_SHEEN) { L5 = sheen_L(0.5f, s.materials[i].lobes[k].r); have = true; break; }
  std::vector<DevMaterial>& mats = out.materials;
  mats.resize(s.num_materials);
  out.lobe_tex.resize(8 * (size_t)s.num_materials);
  for (uint32_t i = 0; i < s.num_materials; ++i)
    if (!bake_material(s.materials[i], L5, mats[i], out.lobe_tex.data() + 8 * (size_t)i)) return refuse("material with an unknown closure id");
  out.mat_masked.assign(s.num_materials, 0);
  out.any_emit_tex = any_emit_tex;
  out.mat_emit_tex.resize(s.num_materials);
  for (uint32_t i = 0; i < s.num_materials; ++i) out.mat_emit_tex[i] = s.materials[i].emission_uv_texture;
  for (uint32_t i = 0; i < s.num_materials; ++i)
    for (uint32_t k = 0; k < mats[i].num_lobes; ++k) if (mats[i].lobes[k].fac_mode >= PHX_FAC_TEX_B) out.mat_masked[i] = 1;

  // the lights' tables (light_tables), from the fingerprint a geometry update will read them from again
  fp.lights = out.lights;
  for (auto& L : fp.lights) { L.ex = mats[L.material].ex; L.ey = mats[L.material].ey; L.ez = mats[L.material].ez; }
  if (lights_by_power) fp.light_power = light_power_factors(s, fp.lights);
  if (lights_env) environment_tables(s, out);
  light_tables(out, fp, lights_by_power, lights_env);
  fp.prim_material = out.prim_material;
  fp.any_smooth = out.any_smooth; fp.any_tex = any_tex; fp.any_mask = any_mask; fp.any_emit_tex = any_emit_tex;

  // the environment's image, and every texture's texels as float4 (one 16-byte load per texel) behind a small table
  DevScene& sc = out.scene;
  sc.env_material = s.environment_material;
  out.env_tex = s.environment_material >= 0 ? s.materials[s.environment_material].emission_texture : 0u;  // texture + 1, 0 = none
  if (out.env_tex) {
    out.env_mapping = s.materials[s.environment_material].emission_mapping;
    for (int c = 0; c < 3; ++c) out.env_e[c] = s.materials[s.environment_material].emission[c];
  }
  sc.any_tex = (any_tex ? SC_TEX_LOBES : 0u) | (out.env_tex ? SC_TEX_ENV : 0u) | (any_mask ? SC_TEX_MASK : 0u) | (lights_by_area ? SC_LIGHTS_BY_AREA : 0u) |
               (lights_by_power ? SC_LIGHTS_BY_POWER : 0u) | (lights_env ? SC_LIGHTS_ENV : 0u);
  if (sc.any_tex & SC_TEX_ANY) {
    out.textures.resize(s.num_textures);
    out.texels.resize((size_t)total_texels);
    uint32_t off = 0;
    for (uint32_t t = 0; t < s.num_textures; ++t) {
      const phx_texture& T = s.textures[t];
      const uint32_t nt = T.width * T.height;
      out.textures[t] = DevTexture{off, T.width, T.height, T.filter | (T.swrap << 8) | (T.twrap << 16)};
      for (uint32_t k = 0; k < nt; ++k) out.texels[off + k] = make_float4(T.texels[3 * (size_t)k], T.texels[3 * (size_t)k + 1], T.texels[3 * (size_t)k + 2], 0.0f);
      off += nt;
    }
  }

  // which shade kernel the scene runs: textured lobes and environment maps are shaded by k_shade_g<.., TEX, ENV> only, and so is the pick by area
  sc.diffuse_only = sc.any_tex ? 0 : 1;
  for (auto& m : mats) {
    if (m.per_hit) sc.diffuse_only = 0, sc.any_per_hit = 1;
    for (uint32_t k = 0; k < m.num_lobes; ++k) if (m.lobes[k].type != L_DIFFUSE) sc.diffuse_only = 0;
  }
  bool single = sc.diffuse_only != 0;
  for (auto& m : mats) single = single && m.num_lobes <= 1;
  if (single) {  // at most one Lambert lobe everywhere (the soups, the Cornell box): a 32-byte material table for k_shade<2>
    sc.diffuse_only = 2;
    for (const DevMaterial& m : mats) {  // (a material without lobes has zero weights, whatever an emissive closure left in lobes[0])
      const DevLobe l = m.num_lobes ? m.lobes[0] : DevLobe{};
      out.mat_lite.push_back(DevMatLite{l.wx, l.wy, l.wz, m.num_lobes | (l.flags << 8), m.ex, m.ey, m.ez, 0u});
    }
  }

  sc.num_lights = (uint32_t)out.lights.size();
  sc.max_depth = opt.path_depth;
  return flatten_camera(s.camera, sc, err);  // (accepted above)
}

int flatten_geometry(const phx_scene& s, const phx_options& opt, const GeometryFingerprint& fp, FlatScene& out, std::string& err) {
  auto refuse = [&err](std::string why) { err = "update_geometry: " + std::move(why); return (int)PHX_ERR_ARG; };
  if (!s.meshes || !s.materials || s.num_materials != fp.is_emitter.size()) return refuse("the scene's material table is not the committed scene's");
  bool any_tex = false, any_mask = false, any_emit_tex = false;
  if (const int rc = texture_classes(s, any_tex, any_mask, any_emit_tex, err)) return rc;
  if (any_tex != fp.any_tex || any_mask != fp.any_mask || any_emit_tex != fp.any_emit_tex) return refuse("the texture classes (any_tex) differ from the committed scene's");
  out = FlatScene{};
  scan_smooth(s, out);
  if (out.any_smooth != fp.any_smooth) return refuse("any_smooth differs from the committed scene's");
  const bool lights_by_area = PHX_LIGHT_SAMPLING_MODE(opt.light_sampling) == PHX_LIGHTS_BY_AREA;
  if (const int rc = walk_geometry(s, fp.is_emitter, false, lights_by_area, out, err)) return rc;
  if (out.prim_material.size() != fp.prim_material.size())
    return refuse("the triangle count differs from the committed scene's (" + std::to_string(out.prim_material.size()) + " for " + std::to_string(fp.prim_material.size()) + ")");
  for (size_t p = 0; p < out.prim_material.size(); ++p)
    if (out.prim_material[p] != fp.prim_material[p]) return refuse("the material word of primitive " + std::to_string(p) + " differs from the committed scene's");
  if (out.lights.size() != fp.lights.size()) return refuse("the number of lights differs from the committed scene's");
  for (size_t l = 0; l < out.lights.size(); ++l) {
    if (out.lights[l].num_tris != fp.lights[l].num_tris) return refuse("the triangle count of light " + std::to_string(l) + " differs from the committed scene's");
    if (out.lights[l].material != fp.lights[l].material) return refuse("the material of light " + std::to_string(l) + " differs from the committed scene's");
  }
  // one pass over the vertices: the finiteness check and the geometry's bounds (fp32 min / max, what k_prim_bounds gives: the summary's)
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  const float* v = out.abc.data();
  for (size_t k = 0, n = out.abc.size() / 3; k < n; ++k, v += 3) {
    if (!(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]))) return refuse("vertex " + std::to_string(k % 3) + " of primitive " + std::to_string(k / 3) + " is not finite");
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
  }
  for (int a = 0; a < 3; ++a) { out.bounds[a] = lo[a]; out.bounds[3 + a] = hi[a]; }
  light_tables(out, fp, (opt.light_sampling & PHX_LIGHT_SELECT_BY_POWER) != 0, PHX_LIGHT_ENVIRONMENT(opt.light_sampling) != 0);
  return PHX_OK;
}

}  // namespace phx
