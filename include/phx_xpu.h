/*
 * phx_xpu.h — C ABI of the MI355X (gfx950) path-tracing device for phosphorus.
 *
 * This is the drop-in boundary: a shared library (libphx_hip.so) exporting exactly
 * what a `hip_t : xpu_t` backend of the reference needs.  The reference interface it
 * replaces is `struct xpu_t` (reference src/xpu.hpp:12-40):
 *
 *     virtual void preprocess(const scene_t&)            -> phx_dev_preprocess
 *     virtual void start(const scene_t&, frame_state_t&) -> phx_dev_start
 *     virtual void join()                                -> phx_dev_join
 *     static T* make(const parsed_options_t&)            -> phx_dev_make   (src/xpu/cpu.hpp:35, src/xpu/cuda.hpp:12)
 *     virtual ~xpu_t()                                   -> phx_dev_destroy
 *     static discover(const parsed_options_t&)           -> phx_discover   (src/xpu.cpp:7-9)
 *
 * Plain C types only: pointers + sizes, no C++/torch types, int status codes instead of the
 * reference's exceptions (std::runtime_error in utils/allocator.hpp:37-39 and kernels/cpu/spt.hpp:230).
 * All arrays passed to phx_dev_preprocess are copied; the caller may free them afterwards
 * (the reference device also rebuilds its own BVH in preprocess, src/xpu/cpu.cpp:35-44,219).
 */
#ifndef PHX_XPU_H
#define PHX_XPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------- */
enum {
  PHX_OK            = 0,
  PHX_ERR_ARG       = 1, /* bad argument / malformed scene */
  PHX_ERR_DEVICE    = 2, /* HIP error; see phx_last_error() */
  PHX_ERR_NO_DEVICE = 3, /* no gfx950 device visible */
  PHX_ERR_STATE     = 4, /* call order violated (start before preprocess, ...) */
  PHX_ERR_OOM       = 5  /* device arena exhausted ("Out of memory", utils/allocator.hpp:37) */
};

/* ---- ray / interaction flag bits (reference src/state.hpp:33-36) ------------------- */
enum { PHX_HIT = 1, PHX_MASKED = 2, PHX_SHADOW = 4, PHX_SPECULAR = 8 };

/* ---- closure ids (reference src/bsdf.hpp:14-24) and lobe flags (src/bsdf/params.hpp:12-16) */
enum {
  PHX_LOBE_EMISSIVE = 0, PHX_LOBE_DIFFUSE = 1, PHX_LOBE_OREN_NAYAR = 2, PHX_LOBE_REFLECTION = 4,
  PHX_LOBE_REFRACTION = 8, PHX_LOBE_MICROFACET = 16, PHX_LOBE_SHEEN = 32, PHX_LOBE_BACKGROUND = 64,
  PHX_LOBE_TRANSPARENT = 128
};
enum { PHX_BSDF_DIFFUSE = 1, PHX_BSDF_GLOSSY = 2, PHX_BSDF_SPECULAR = 4, PHX_BSDF_REFLECT = 8, PHX_BSDF_TRANSMIT = 16 };
#define PHX_MAX_LOBES 8 /* bsdf_t::MaxLobes, src/bsdf.hpp:9 */

/* ---- options: parsed_options_t (reference src/options.hpp:6-43) + device knobs ------- */
typedef struct phx_options {
  uint32_t samples_per_pixel; /* default 16 */
  uint32_t paths_per_sample;  /* default 16; only scales the film by 1/pps (src/xpu/cpu.cpp:191) */
  uint32_t path_depth;        /* default 9 */
  uint32_t single_threaded;   /* honoured by CPU devices only */
  uint32_t host_only;         /* --no-gpu: phx_discover returns 0 devices */
  uint32_t render_normals;
  uint32_t verbose;
  /* device additions (0 = auto) */
  int32_t  device_ordinal;    /* HIP device index; -1 = current device */
  uint32_t samples_in_flight; /* samples of one pixel carried per wavefront pass */
  uint32_t tiles_per_batch;   /* tiles pulled from the queue per pass */
  uint32_t bvh_builder;       /* PHX_BVH_AUTO (default), PHX_BVH_DEVICE_LBVH or PHX_BVH_HOST_SAH: where preprocess builds the tree */
  uint32_t light_sampling;    /* PHX_LIGHTS_REFERENCE (default) or PHX_LIGHTS_BY_AREA: how next-event estimation picks a triangle of the chosen light; | PHX_LIGHT_SELECT_BY_POWER [| PHX_LIGHT_INCLUDE_ENVIRONMENT] */
  uint32_t reserved[4];
} phx_options;
/* AUTO = the device builder (LBVH over extended Morton codes + the optimal 8-wide collapse) for every scene with at least 64
 * triangles: 1 M triangles in 12 ms and 10 M in 40 ms against 0.6 s / 7 s of the host's binned-SAH builder, and since round 3 its
 * trees trace as fast or faster on every scene measured (profiles/r03_z_emc_probe.log).  cpu_t::preprocess rebuilds its accelerator
 * on every call (src/xpu/cpu.cpp:35-44), so the build time is part of the interface's cost.  HOST_SAH stays selectable, and AUTO falls back to it
 * when the device build fails (phx_stats.bvh_built_on_device = 0); an explicit DEVICE_LBVH request fails with PHX_ERR_DEVICE instead. */
enum { PHX_BVH_AUTO = 0, PHX_BVH_DEVICE_LBVH = 1, PHX_BVH_HOST_SAH = 2 };
/* light_sampling.  Next-event estimation chooses a light uniformly (l = floor(pick * nlights), clamped) and a triangle inside it from the
 * draw lu, and reports the density lpdf = (1 / area of the light's face set) / nlights.  Any other value is PHX_ERR_ARG at phx_dev_preprocess.
 *   PHX_LIGHTS_REFERENCE: the triangle by index, ti = floor(lu * num_tris) (clamped), remapped = min(lu * num_tris - ti, 1 - FLT_EPSILON), as
 *     light.cpp:55-67 does with its search commented out (light.cpp:30-53).  The reported density is the true one only when every triangle of
 *     the light has the same area (SURVEY A-12; tests/integrator64.py: uniform_triangle_pick).  Bit for bit the reference's films.
 *   PHX_LIGHTS_BY_AREA: the triangle by area, all in fp32.  Per light, in the face order of its face set,
 *       acc_i = acc_{i-1} + area_i        (the running sum whose last value is the light's area)
 *       cdf[i] = acc_i / area             (the last entry is area / area = 1)
 *     ti is the smallest i with lu < cdf[i], or num_tris - 1 when there is none (binary search on the monotone table);
 *       lo = ti ? cdf[ti - 1] : 0         remapped = min((lu - lo) / (cdf[ti] - lo), 1 - FLT_EPSILON)
 *     and everything behind the pick is unchanged: triangle_t::sample(remapped, lv), P, lpdf, which is now the true density.  A triangle
 *     of zero area has cdf[i] == lo and is never chosen.  A light of one triangle, or of two whose fp32 areas are bit-equal (cdf = {0.5, 1}),
 *     is sampled bit for bit as under PHX_LIGHTS_REFERENCE; three or more equal triangles are not (3 * a rounds).  The scene is shaded by
 *     k_shade_g (phx_stats.shade_general = 1) whatever its closures.  Lights are chosen uniformly unless PHX_LIGHT_SELECT_BY_POWER (below,
 *     DESIGN 14) is set in the same word. */
enum { PHX_LIGHTS_REFERENCE = 0, PHX_LIGHTS_BY_AREA = 1 };
/* The word is packed like phx_lobe.fac_mode: the low byte is the triangle pick above, bit 8 chooses how a LIGHT is selected.  The valid
 * words are 0, 1, 0x101 (PHX_LIGHTS_BY_AREA | PHX_LIGHT_SELECT_BY_POWER) and 0x301 (below); every other word, 0x100 among them (selection by power needs the
 * unbiased triangle pick), is PHX_ERR_ARG at phx_dev_preprocess.
 *   PHX_LIGHT_SELECT_BY_POWER: a light by its power instead of uniformly.  Lights stay in the light table's order (mesh x face-set order);
 *   all host arithmetic below is binary64, without contraction, in the order written.
 *     weight   m_l = the per-channel mean of |texel| over ALL texels of the image named by the material's emission_uv_texture, summed
 *              sequentially in row-major texel order and divided by W * H; (1, 1, 1) without an image.  With area_l and e the fp32 values of the
 *              light's record widened to double,
 *                w_l = area_l * ((0.2126 |e_r| m_r + 0.7152 |e_g| m_g) + 0.0722 |e_b| m_b)
 *              The image mean stands for the light's true power: it ignores which part of the image the UVs show, and only ever affects variance.
 *     totals   n+ = the number of lights with w_l > 0;  Wsum = sum of w_l, sequentially in light order.
 *     fallback if any w_l is not finite, or n+ = 0: q_l = 1 / nlights (uniform selection through the same table; the scene is black or broken).
 *     floor    q_l = w_l > 0 ? (1 - phi) w_l / Wsum + phi / n+ : 0, phi = PHX_LIGHT_POWER_FLOOR = 1/8.  Every lamp that emits anything keeps
 *              q_l >= 1 / (8 n+), so the estimator's second moment is at most 8 x uniform selection's and 8/7 x pure power selection's, and a
 *              24-bit draw realises such a probability to a relative 2^-24 * 8 n+.  A black lamp is never sampled.
 *     table    acc_l = acc_{l-1} + q_l;  pcdf[l] = fp32(acc_l / acc_last): monotone, the last entry 1.0f exactly.
 *     pick     l = the smallest index with pick < pcdf[l], or nlights - 1 when there is none (binary search);  lo = l ? pcdf[l - 1] : 0;
 *              p_l = pcdf[l] - lo in fp32, and the light's density lpdf = (1.0f / area_l) * p_l in fp32, evaluated at preprocess.  `pick` is used
 *              for nothing else; a light with p_l = 0 cannot be chosen.
 *   Everything behind the pick is PHX_LIGHTS_BY_AREA's: the triangle by the area CDF, triangle_t::sample, P, the emission.  A scene with ONE
 *   light has pcdf = {1}, l = 0 and lpdf = 1.0f / area: bit for bit what PHX_LIGHTS_BY_AREA alone renders. */
enum { PHX_LIGHT_SELECT_BY_POWER = 0x100 };
/* Bit 9 of the same word: next-event estimation samples the ENVIRONMENT IMAGE too.  The only new valid word is 0x301
 * (PHX_LIGHTS_BY_AREA | PHX_LIGHT_SELECT_BY_POWER | PHX_LIGHT_INCLUDE_ENVIRONMENT): the valid words are 0, 1, 0x101 and 0x301, and every other one
 * (0x200, 0x201, 0x300 among them) is PHX_ERR_ARG at phx_dev_preprocess, as is 0x301 on a scene whose environment material has no
 * emission_texture (a constant sky is served by cosine-weighted BSDF sampling already).  The scene still needs an emissive face set.
 * With the bit clear nothing changes.  All host arithmetic below is binary64, without contraction, in the order written; device tables are fp32.
 *   importance T = the environment image (W x H), e = the environment material's emission, Y(c) = (0.2126 c_r + 0.7152 c_g) + 0.0722 c_b.
 *              Per texel (column i, row j) y_ij = Y(|e| * |texel_ij|) (per channel), and
 *                g_ij = yhat_ij * sin((pi * (j + 0.5)) / H)
 *              with yhat_ij = y_ij under PHX_TEX_CLOSEST.  Under PHX_TEX_LINEAR yhat_ij starts as y_ij and is replaced by every y of the 3 x 3
 *              neighbourhood of (i, j) that compares greater (rows j - 1 .. j + 1, in each columns i - 1 .. i + 1), the neighbours taken through
 *              the image's own wrap modes; one outside the image under PHX_WRAP_BLACK counts 0.  So g > 0 wherever the bilinear lookup can be
 *              non-zero inside the texel: the sampled density is positive wherever the integrand is.
 *              G = the sum of g_ij, sequentially in row-major order;  rowsum_j = the sum of g_ij over i, sequentially.
 *   weight     the environment is ONE MORE ENTRY of PHX_LIGHT_SELECT_BY_POWER's table, behind the nlights mesh lights, with
 *                w_env = (((4 pi) * R) * R) * (G / (W * H)) * (pi / 2)
 *              R = 0.5 * sqrt(dx*dx + dy*dy + dz*dz) of the scene's bounding box (fp32 min / max of every triangle corner, the extents
 *              subtracted after widening to double).  sum g / (W H) approximates (1 / pi) * integral of yhat sin(theta) dtheta dphi / (2 pi),
 *              so w_env is 4 pi R^2 x the solid-angle-weighted mean luminance: an area light's A * Y against pi R^2 * integral of L d omega
 *              with the common pi divided out.  Like m_l it only ever affects variance.  n+, Wsum, the fallback, the floor, pcdf and p_l are
 *              the rule above applied to nlights + 1 entries; pcdf has nlights + 1 entries, the last 1.0f.  The mesh lights keep
 *              lpdf = (1.0f / area_l) * p_l, and p_env = pcdf[nlights] - pcdf[nlights - 1] in fp32.  A black image has w_env = 0 and is never chosen.
 *   directions mcdf[j] = fp32((rowsum_0 + ... + rowsum_j) / G), the last entry set to 1.0f;  ccdf[j][i] = fp32((g_0j + ... + g_ij) / rowsum_j), a
 *              row of zero sum all 1.0f (it has mcdf[j] == mcdf[j - 1] and is never chosen).  Both are monotone.  If G is zero or not finite
 *              (a black or broken image: w_env is then 0, or not finite and the whole table uniform) the two tables are built from
 *              g_ij = sin((pi * (j + 0.5)) / H) instead: uniform over the sphere.
 *   sample     when the pick returns l == nlights: j = the smallest index with lu < mcdf[j], else H - 1;  lo = j ? mcdf[j - 1] : 0;
 *              P_row = mcdf[j] - lo;  ru = min((lu - lo) / P_row, 1 - FLT_EPSILON);  i, P_col and rv likewise from lv in ccdf[j].  Binary searches
 *              of at most 17 steps with clamped indices: a NaN draw ends at the last index, no draw reads outside a table.  All fp32:
 *                s = (i + rv) / W    t = (j + ru) / H    phi = (s - 0.5f) * 2 pi    lambda = (0.5f - t) * pi      (2 pi, pi: the nearest floats)
 *                PHX_ENV_LATLONG_Y_UP: d = (-cos(lambda) sin(phi), sin(lambda), cos(lambda) cos(phi))
 *                PHX_ENV_LATLONG_Z_UP: d = ( cos(lambda) cos(phi), cos(lambda) sin(phi), sin(lambda))
 *              the inverses of phx_material.emission_texture's mapping, and
 *                pdf_omega = ((P_row * P_col) * (W * H)) / (2 pi^2 * sin(pi * t))          pdf = p_env * pdf_omega
 *              (W * H and 2 pi^2 rounded to fp32 once; sin(pi t) = cos(y), y = pi * (0.5 - t) in binary64, by the Taylor polynomial
 *              1 - y^2 (1/2! - y^2 (1/4! - ... - y^2 / 20!)) evaluated in binary64 from the inside out and rounded to fp32 once: no library
 *              function enters the density).  The estimator divides by the tables' own intervals, so it is unbiased to the draw's 24
 *              bits whatever rounding went into g.  If sin(pi t) <= 0, or pdf is not finite and positive, there is no shadow ray.
 *   estimate   le = the environment's e in direction d exactly as a miss computes it, f = bsdf_t::f(d, wo) with the sign of the cosine n.d it
 *              carries dropped (f * -1 where n.d < 0: |n.d|, as in the weight of a BSDF sample),
 *                contrib = beta * ((le * f) * (1.0f / pdf))
 *              with NO factor 4 (that is a quirk of the reference's area lights; it has no environment sampling) and without the mesh
 *              lights' n.d >= 0 gate: bsdf_t::f decides, so transmissive lobes keep their environment light.  The shadow ray starts at
 *              p + n * (n.d < 0 ? -1e-4f : 1e-4f), runs along d, tmax = FLT_MAX, and counts in rays_shadow; a sample whose f is zero in every
 *              channel (a direction below an opaque surface) issues none.
 *   miss       a path that misses adds the environment only at depth 0 or behind a specular bounce (the gate of surface emission):
 *              everywhere else next-event estimation has accounted for it.  The film's expectation is the one of 0x101; its variance is not.
 *   limits     no MIS; where a lobe's sampling pdf is one of DESIGN 4.11's quirks the two films' expectations differ by that documented bias. */
enum { PHX_LIGHT_INCLUDE_ENVIRONMENT = 0x200 };
#define PHX_LIGHT_SAMPLING_MODE(x) ((x) & 0xffu)    /* PHX_LIGHTS_* */
#define PHX_LIGHT_SELECTION(x) ((x) & ~0xffu)       /* 0 or PHX_LIGHT_SELECT_BY_POWER */
#define PHX_LIGHT_ENVIRONMENT(x) ((x) & 0x200u)     /* 0 or PHX_LIGHT_INCLUDE_ENVIRONMENT */
#define PHX_LIGHT_POWER_FLOOR 0.125

/* ---- scene: what the device reads through scene_t (src/scene.hpp:14-50) --------------- */

/* One closure of a flattened closure tree (the output contract of material_t::evaluate,
 * src/material.cpp:218-305,419-458, with constant inputs; shading normal = interpolated N). */
typedef struct phx_lobe {
  uint32_t type;      /* PHX_LOBE_* */
  float    weight[3]; /* accumulated colour weight */
  float    alpha;     /* OrenNayar: sigma (treated as degrees, src/bsdf/params.hpp:38) */
  float    eta;       /* Reflection / Refraction / Microfacet */
  float    xalpha;    /* Microfacet roughness inputs BEFORE precompute() (params.hpp:86-99) */
  float    yalpha;
  uint32_t refract;   /* Microfacet: 1 = transmissive */
  float    r;         /* Sheen roughness */
  /* Per-hit closure weight — the one hit-dependent input the reference's own node shaders produce: a mix_closure_node whose `fac`
   * is driven by fresnel_dielectric_node (Blender's glass node: plugins/blender/blender/shader.hpp:306-335,
   * src/shaders/fresnel_dielectric_node.osl:16-20, mix_closure_node.osl:20).  At every hit
   *   fac = fresnel_dielectric(dot(I, N), backfacing ? 1 / max(1e-5, fac_ior) : max(1e-5, fac_ior))      (src/shaders/fresnel.h)
   * and the closure's weight is (pre_weight * term) * weight with term = fac (PHX_FAC_MIX_B) or 1 - fac (PHX_FAC_MIX_A), in the
   * order material_t::eval_closure multiplies down the tree (src/material.cpp:218-305); a closure whose weight comes out all
   * zero is not there at that hit (OSL: closure * 0 is the null closure).  PHX_FAC_NONE: weight is the whole constant weight.
   *
   * Image mask (texture_node.Cout -> luminance_node.in, luminance_node.out -> mix_closure_node.fac: src/shaders/luminance_node.osl is the
   * node set's only colour -> float node): the low byte of fac_mode is the mode, PHX_FAC_TEX_B or PHX_FAC_TEX_A, and bits 8..31 name the
   * mask image, 1-based into phx_scene.textures (PHX_FAC_PACK(mode, k), PHX_FAC_MODE, PHX_FAC_TEXTURE).  At every surface hit with
   * interpolated mesh UV (s, t)
   *   c   = the phx_texture lookup of image k at (s, t), with the image's own filter and wrap modes
   *   fac = (c.r * 0.2126f + c.g * 0.7152f) + c.b * 0.0722f        (fp32, in this order, no contraction; NOT clamped)
   * and term = fac (PHX_FAC_TEX_B) or 1 - fac (PHX_FAC_TEX_A); the weight is (pre_weight * term) * (weight * colour texel), the colour
   * texel being 1 without `texture`, and a lobe whose weight comes out all zero is not there at that hit (it counts neither in the lobe
   * choice of bsdf_t::sample nor in bsdf_t::f).  A restatement, not pinned to OSL's object code.  fac_ior is ignored for the two image
   * modes; bits 8..31 must be zero for the other modes; one lobe has one factor (Fresnel or image), different lobes of one material may
   * differ.  Like `texture`, not allowed on the lobes of emitters or of the environment material; a mesh without UVs has (s, t) = (0, 0). */
  uint32_t fac_mode;
  float    fac_ior;
  float    pre_weight[3]; /* product of the constant weights ABOVE the hit-dependent factor in the closure tree */
  /* Image texture on the colour weight (texture_node.osl's Cout into the closure's Cs): 0 = none, k = phx_scene.textures[k - 1].  At every
   * surface hit the lobe's weight is weight * texel (one fp32 multiply per channel), looked up at the hit's interpolated mesh UV; the
   * per-hit factor above then applies to that product, (pre_weight * term) * (weight * texel), and a lobe whose weight comes out all
   * zero is not there at that hit.  Not allowed on the lobes of emitters or of the environment material. */
  uint32_t texture;
} phx_lobe;
enum { PHX_FAC_NONE = 0, PHX_FAC_MIX_B = 1, PHX_FAC_MIX_A = 2, PHX_FAC_TEX_B = 3, PHX_FAC_TEX_A = 4 };
#define PHX_FAC_MODE(x)       ((uint32_t)(x) & 0xffu)               /* the mode of a phx_lobe.fac_mode word */
#define PHX_FAC_TEXTURE(x)    ((uint32_t)(x) >> 8)                  /* its mask image: 0 = none, k = phx_scene.textures[k - 1] */
#define PHX_FAC_PACK(mode, k) (((uint32_t)(mode) & 0xffu) | ((uint32_t)(k) << 8))

typedef struct phx_material {
  uint32_t num_lobes;   /* 0 for pure emitters (diffuse_emitter_node.osl) */
  uint32_t is_emitter;  /* material_t::is_emitter, src/material.cpp:487 */
  float    emission[3]; /* weight of the emission()/background() closure: hits.e */
  /* Environment map (environment_node.osl's Cout = environment(filename, I) into background_node.Cs): 0 = none, k = phx_scene.textures[k - 1].
   * Allowed ONLY on phx_scene.environment_material (PHX_ERR_ARG elsewhere: a surface emitter's image is emission_uv_texture).  Where a path
   * misses every surface (camera rays included) with direction d = (x, y, z), it adds beta * e with e = emission * texel(s, t), one fp32
   * multiply per channel; the environment is sampled by next-event estimation only under PHX_LIGHT_INCLUDE_ENVIRONMENT.  (s, t) restates OpenImageIO's documented lat-long
   * convention (latlong_up "y" by default, or "z"), computed in binary64 from the fp32 components widened to double, operation by
   * operation in the order written (no contraction), each result rounded to fp32 once; INV_2PI and INV_PI are the doubles nearest
   * 1/(2 pi) and 1/pi:
   *   PHX_ENV_LATLONG_Y_UP: s = 0.5 + atan2(-x, z) * INV_2PI   t = 0.5 - atan2(y, sqrt(z*z + x*x)) * INV_PI
   *   PHX_ENV_LATLONG_Z_UP: s = 0.5 + atan2( y, x) * INV_2PI   t = 0.5 - atan2(z, sqrt(x*x + y*y)) * INV_PI
   * It is a restatement, not pinned to OpenImageIO's object code.  The texel is the phx_texture lookup with the texture's own filter and
   * wrap modes (OpenImageIO's lat-long wrap is swrap periodic, twrap clamp); no MIP maps, no blur.  A zero or non-finite d reads black. */
  uint32_t emission_texture;
  uint32_t emission_mapping; /* PHX_ENV_LATLONG_*; any other value is PHX_ERR_ARG */
  /* Textured surface emission (texture_node.Cout into diffuse_emitter_node.Cs): 0 = none, k = phx_scene.textures[k - 1].  Allowed on
   * is_emitter materials only, and not on phx_scene.environment_material; an index past the table is PHX_ERR_ARG too.  Wherever the
   * material's emission e is used it is e * texel(s, t): one fp32 multiply per channel (no contraction), the phx_texture lookup with the
   * image's own filter and wraps -- the expression emission_texture uses for the environment.
   *   at a hit (depth == 0, or behind a specular bounce): (s, t) is the hit's interpolated mesh UV, as for a textured lobe;
   *   at a light sample of next-event estimation: with (bu, bv) of triangle_t::sample, P = bu * a + bv * b + (1 - bu - bv) * c and
   *       st = (bu * uv_a + bv * uv_b) + (1 - bu - bv) * uv_c        (fp32, in this order)
   *     the UV of the sampled point itself.  A stated deviation (DESIGN: light_st_rotated): the reference reads the sample's (bu, bv) as
   *     Moeller-Trumbore barycentrics (st = w * uv0 + u * uv1 + v * uv2, mesh.cpp:178-181,256) although barycentric_to_point puts them on
   *     a and b (mesh.cpp:314-316), so it looks the image up at another point of the triangle than the one it lights from.
   * A mesh without UVs has (s, t) = (0, 0).  The lobes of an emitter still take no image.  The scene is shaded by the TEX kernels. */
  uint32_t emission_uv_texture;
  phx_lobe lobes[PHX_MAX_LOBES];
} phx_material;
enum { PHX_ENV_LATLONG_Y_UP = 0, PHX_ENV_LATLONG_Z_UP = 1 };

/* mesh_t::face_set_t, src/mesh.hpp:26-41 */
typedef struct phx_face_set {
  uint32_t        material;  /* index into phx_scene.materials */
  uint32_t        num_faces;
  const uint32_t* faces;     /* face indices (not multiplied by 3) */
} phx_face_set;

/* mesh_t, src/mesh.hpp:14-138; mesh id = index in phx_scene.meshes (src/scene.cpp:79-82) */
typedef struct phx_mesh {
  const float*    vertices;  /* xyz per vertex */
  uint32_t        num_vertices;
  const float*    normals;   /* xyz; per vertex, or per face-corner when !NORMALS_PER_VERTEX */
  uint32_t        num_normals;
  const uint32_t* faces;     /* 3 vertex indices per face */
  uint32_t        num_faces;
  const uint8_t*  smooth;    /* per face: 1 = interpolate normals, 0 = geometric normal (mesh.cpp:187-206) */
  uint32_t        flags;     /* PHX_MESH_* */
  uint32_t        num_sets;
  const phx_face_set* sets;
  /* texture coordinates (mesh_t::uvs), 2 floats (s, t) each; per vertex when PHX_MESH_UV_PER_VERTEX, per face corner (3 f + k) otherwise.
   * Read only when some lobe is textured; a mesh without UVs has st = (0, 0) at every hit (mesh.cpp:240-241). */
  const float*    uvs;
  uint32_t        num_uvs;
} phx_mesh;
enum { PHX_MESH_UV_PER_VERTEX = 1, PHX_MESH_NORMALS_PER_VERTEX = 2 }; /* mesh_t::flags_t, src/mesh.hpp:20-23 */

/* camera_t, src/entities/camera.hpp:10-39.  aperture_radius == 0: pinhole (camera_t::is_pinhole); otherwise the thin lens of
 * src/kernels/cpu/camera.hpp:140-147 with the disc mapping of src/math/simd/sampling.hpp:8-32 as the reference wrote it (SURVEY A-21:
 * raw samples, swapped select) and focal_distance the distance of the plane in focus.  Both must be finite. */
typedef struct phx_camera {
  float    to_world[16]; /* Imath::M44f x[i][j], row-vector convention v' = v * M */
  float    fov;
  float    focal_distance;
  float    aperture_radius;
  uint32_t film_width;
  uint32_t film_height;
} phx_camera;

/* An RGB image texture (texture_node.osl).  Texels are linear fp32 RGB, no colour transform.  Row 0 is the first scanline and holds
 * t in [0, 1/height) (OIIO's convention).  At (s, t): x = s*W - 0.5, y = t*H - 0.5 and PHX_TEX_LINEAR blends the four texels around
 * (floor(x), floor(y)) bilinearly; PHX_TEX_CLOSEST reads texel (floor(s*W), floor(t*H)).  Wrap modes per axis; under PHX_WRAP_BLACK a
 * texel outside the image reads as 0.  A non-finite coordinate, or |s*W| or |t*H| above 2^24, reads black.  No MIP maps, no bicubic. */
typedef struct phx_texture {
  uint32_t     width, height; /* 1 .. 65536 each, at most 2^26 texels */
  const float* texels;        /* width * height RGB triples, row-major, rows top to bottom */
  uint32_t     filter;        /* PHX_TEX_* */
  uint32_t     swrap, twrap;  /* PHX_WRAP_* */
  uint32_t     reserved[3];
} phx_texture;
enum { PHX_TEX_LINEAR = 0, PHX_TEX_CLOSEST = 1 };
enum { PHX_WRAP_PERIODIC = 0, PHX_WRAP_CLAMP = 1, PHX_WRAP_BLACK = 2 };

typedef struct phx_scene {
  uint32_t            num_meshes;
  const phx_mesh*     meshes;
  uint32_t            num_materials;
  const phx_material* materials;
  int32_t             environment_material; /* -1 = none (scene_t::environment, src/scene.cpp:126) */
  phx_camera          camera;
  uint32_t            num_textures;  /* phx_lobe.texture, the mask of phx_lobe.fac_mode, phx_material.emission_texture and emission_uv_texture index this table (1-based) */
  const phx_texture*  textures;
} phx_scene;

/* ---- frame: frame_state_t {sampler, tiles, film} (src/state.hpp:18-31) --------------- */
typedef struct phx_tile { uint32_t x, y, w, h; } phx_tile; /* job::tiles_t::tile_t, src/jobs/tiles.hpp:12-19 */

/* job::tiles_t::next (src/jobs/tiles.hpp:40-47): returns 1 and fills *out, or 0 when drained.
 * Called from the device's driver thread; must be thread safe (devices share one queue,
 * src/core.cpp:103-108). */
typedef int (*phx_next_tile_fn)(void* user, phx_tile* out);

/* film_t<>::add_tile (src/film.hpp:12-15): `buffer` is the tile's interleaved fp32
 * render_buffer_t (src/buffer.hpp:8-97): pixel (x,y) at buffer[y*ystride + x*xstride + c].
 * Called from the device's driver thread. */
typedef void (*phx_add_tile_fn)(void* user, int32_t x, int32_t y, int32_t w, int32_t h,
                                const float* buffer, uint32_t xstride, uint32_t ystride);

typedef struct phx_frame {
  void*            tiles_user;
  phx_next_tile_fn next_tile;
  void*            film_user;
  phx_add_tile_fn  add_tile;        /* may be NULL when device_film is set */
  uint64_t         sampler_seed;    /* seed of the counter-based sampler (replaces sampler_t's mt19937) */
  uint32_t         primary_components; /* components of channel "primary": 3 or 4 (3 are written, buffer.cpp:25-30) */
  uint32_t         normals_channel;    /* 1: append channel "normals" x3 (cpu.cpp:194-196) */
  /* optional: accumulate straight into a full-frame device-resident film (W*H*xstride fp32 in HBM,
   * e.g. a torch tensor's data_ptr) — used for the multi-GPU film reduce. */
  float*           device_film;
  /* optional: a full-frame HOST film (W*H*xstride fp32) the device fills tile by tile itself — the same
   * effect as an add_tile callback that copies into a frame buffer (film::file_t, src/film/file.cpp:27-41)
   * without a foreign-function call per tile. */
  float*           host_film;
  /* Per-pixel error estimate.  0: off, and nothing changes by a byte.  1: a channel "m2" of 3 floats (r, g, b) is appended to
   * every pixel behind "primary" and, when present, "normals": its offset is primary_components + (normals_channel ? 3 : 0), and xstride
   * grows by 3.  Any other value is PHX_ERR_ARG at phx_dev_start.  "primary" and "normals" are bit for bit what the frame without the
   * channel holds.  The channel is the centred second moment of the pixel's samples.  Per pixel and colour channel, for a pass that
   * carries samples s0 .. s0 + ns - 1 of the pixel (x_s the radiance of sample s, f_prev the pixel's fp32 "primary" value and m2_prev the
   * channel's value before the pass; the batch buffer is zeroed at the start of a batch), in binary64 without contraction:
   *     y_s  = fp32(x_s * inv)                    the very value the film adds; inv = 1.0f / (spp * pps)
   *     n    = s0;   mean = s0 ? (double)f_prev / (double)s0 : 0.0;   M2 = (double)m2_prev
   *     for each sample, in sample order:
   *         n   += 1;  r_n = 1.0 / (double)n      IEEE binary64 division
   *         d    = (double)y_s - mean
   *         mean = mean + d * r_n
   *         M2   = M2 + d * ((double)y_s - mean)
   *     m2_out = fp32(M2)
   * A frame of one pass holds the centred sum of squares to one fp32 rounding; a pixel whose samples are all equal holds +0.0 exactly, and
   * so does every pixel at spp == 1.  The film value is a sum of S = spp samples y_s, so the unbiased estimate of ITS variance is
   * m2 * S / (S - 1): no subtraction of squares ever happens.  A non-finite sample makes that pixel's m2 non-finite, and no other pixel's.
   * The channel is a statistic of ONE frame: nothing accumulates across frames. */
  uint32_t         moments_channel;
  uint32_t         reserved[1];
} phx_frame;

/* ---- adaptive sampling: a pixel stops taking samples once its own error estimate is small enough ---------- */
/* Off by default, and then nothing changes by a byte.  The setting belongs to the device object (phx_dev_set_adaptive) and applies to every
 * frame started afterwards.  A frame started while it is on must have moments_channel == 1 (PHX_ERR_ARG at phx_dev_start otherwise) and
 * carries one more channel, "samples": 1 float per pixel behind "m2", at offset primary_components + (normals_channel ? 3 : 0) + 3; xstride
 * grows by 1.  It holds (float)n, the samples the pixel took.  With spp = samples_per_pixel, tau = threshold, a = floor; all arithmetic
 * is binary64, without contraction, in the order written:
 *   rounds    the rounds end at e_0 = min(min_samples, spp) and e_{j+1} = min(e_j + step, spp).  A round is carried as one pass; only when
 *             samples_in_flight is set, or the path budget forces it, is it split into passes of at most that many samples, by the rule
 *             that splits a frame's spp without the setting, applied to the round.  Decisions happen at round ends only.
 *   decision  after a round that ends at n < spp, for every pixel still active, with f_c its fp32 "primary" and m2_c its fp32 "m2" per colour:
 *                 q = (double)n / (double)(n - 1)
 *                 g = ((double)a * (double)n) / (double)spp
 *                 per colour:  L = (double)m2_c * q;   b = (double)tau * (fabs((double)f_c) + g);   ok_c = L <= b * b
 *                 stop = ok_r && ok_g && ok_b          (a NaN compares false: such a pixel never stops)
 *             which is se(V_c) <= tau * (|V_c| + a) for the pixel's extrapolated final value V_c = f_c * spp / n, the standard error
 *             taken from the centred second moment.
 *   rescale   a pixel that stops is rescaled once:
 *                 k       = (double)spp / (double)n
 *                 primary = fp32((double)f_c * k)
 *                 m2      = fp32(((double)m2_c * k) * k)
 *                 samples = (float)n
 *             "normals" (and the fourth component of "primary") are never rescaled.
 *   the rest  a pixel that reaches spp is not touched: its "primary", "normals" and "m2" are what the same pass schedule writes without
 *             the setting, and its samples = (float)spp.
 *   variance  after the rescale the unbiased variance of ANY pixel's value is m2 * n / (n - 1), n its own "samples".
 * A pixel's path keys are (seed, film pixel, absolute sample index), so a pixel that stops after n samples holds exactly the first n samples
 * of the frame without the setting; its result depends on its own samples and this schedule alone, not on the batch, the tile order, the
 * tiling or the number of devices.  phx_stats.camera_samples is the sum of the channel.
 * Limits: the estimator is biased, as every variance-driven stopping rule is; a pixel whose first min_samples samples are all equal stops
 * (m2 = +0.0), even if a rare bright path would have reached it; the film jitter stays stratified for spp, not for n. */
typedef struct phx_adaptive {
  float    threshold;    /* tau: relative standard error at which a pixel stops; finite, >= 0 */
  float    floor;        /* a: absolute floor added to |value| in film units; finite, >= 0 */
  uint32_t min_samples;  /* samples every pixel takes before the first decision; >= 2 */
  uint32_t step;         /* samples per later round; >= 1 */
  uint32_t reserved[4];  /* must be 0 */
} phx_adaptive;

/* ---- film denoiser: an edge-avoiding a-trous filter whose yardstick is the film's own error estimate ------ */
/* A post-process of a finished film that has the channel "m2" (phx_frame.moments_channel): a pixel is averaged with neighbours that are the
 * same surface (the "normals" channel) and statistically the same value (their luminance differs by less than sigma_l standard deviations,
 * the deviation taken from m2).  Nothing calls it unless the host does; it reads no scene and changes no frame.
 * State, per pixel: the colour C[3] and the variance of the pixel's value V[3] as fp32; the normal N[3] as the film holds it (fp32, constant,
 * all zero where the camera ray missed); a flag `valid` (constant).  All arithmetic is binary64, without contraction, in the order written;
 * fp32 values are widened first, and a result is rounded to fp32 once, where fp32(...) says so.
 *   init      n     = (double) of the pixel's "samples" float, or (double)spp when samples_offset == 0
 *             valid = the 3 "primary" floats, the 3 "m2" floats and N are finite, every m2 >= 0, and n is finite and >= 2
 *             V_c   = fp32(m2_c * (n / (n - 1)))
 *             An invalid pixel is never a tap below and never part of the 3 x 3; its output floats are its input floats.
 *   iteration i = 0 .. iterations - 1, step s = 2^i: every valid pixel p reads the state the iteration started from and writes a second one.
 *             l_x   = (0.2126 * C_r + 0.7152 * C_g) + 0.0722 * C_b                          luminance of pixel x
 *             e_x   = (0.2126 * sqrt(V_r) + 0.7152 * sqrt(V_g)) + 0.0722 * sqrt(V_b)        its deviation, were the colours' noise fully correlated
 *             S_p   = (sum of (g * e_q) * e_q) / (sum of g)   over q = p + (dx, dy), dy = -1 .. 1 outer, dx = -1 .. 1 inner (ONE pixel apart,
 *                     whatever s), only q inside the film and valid;  g = k3[dy] * k3[dx], k3 = (1/4, 1/2, 1/4);  both sums start at 0.0
 *             sig   = sigma_l * sqrt(S_p)
 *             taps  q = p + s * (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner; a tap outside the film or invalid is skipped.
 *                     h   = k5[dy] * k5[dx],  k5 = (1/16, 1/4, 3/8, 1/4, 1/16)
 *                     centre tap (dx == dy == 0):  w = h   (9/64)
 *                     otherwise
 *                       w_n = 1                                        if N_p and N_q are both all-zero, or normals_offset == 0
 *                             else d = (Nx * Nx' + Ny * Ny') + Nz * Nz';  d = d > 0 ? d : 0;  d = d * d, normal_power_log2 times;  w_n = d
 *                       w_l = (l_q == l_p ? 1 : 0)                     if sig == 0
 *                             else u = fabs(l_q - l_p) / sig;  t = 1 - u * u;  w_l = u < 1 ? t * t : 0       (Tukey's biweight)
 *                       w   = (h * w_n) * w_l
 *                     W += w;   A_c += w * (C_q,c - C_p,c);   B_c += (w * w) * V_q,c          (W, A_c, B_c start at 0.0)
 *             result  C'_c = fp32(C_p,c + A_c / W);   V'_c = fp32(B_c / (W * W))              (W >= 9/64: the centre tap)
 *   output    every float of the pixel is film_in's, except, for a valid pixel when iterations >= 1:
 *             primary rgb = C;   m2 rgb = fp32(V_c * ((n - 1) / n)), so that the variance read from the output (m2 * n / (n - 1)) is V.
 *             iterations == 0 copies the film.
 * The delta form makes a constant neighbourhood exact; a film whose m2 is zero everywhere averages only pixels of EQUAL luminance.
 * Limits: V' treats the pixels as independent and ignores the blur's bias, so it understates the true error (tenfold and more);
 * the biweight rejects bright outliers, so the film's mean drops where the frame has fireflies; there is no depth or albedo guide: textures
 * and coplanar depth edges are protected by luminance alone; nothing is temporal here (what carries a film across a camera move is
 * phx_reproject); a multi-GPU film must be reduced before the call (a
 * rank's own film holds zeros in the pixels it does not own). */
typedef struct phx_denoise {
  uint32_t width, height;      /* 1 .. 65536 each */
  uint32_t xstride;            /* floats per pixel of both films; >= 6 */
  uint32_t normals_offset;     /* 0 = the film has no normals: w_n = 1 everywhere; else >= 3, normals_offset + 3 <= xstride */
  uint32_t m2_offset;          /* required: >= 3, m2_offset + 3 <= xstride */
  uint32_t samples_offset;     /* 0 = none: every pixel took spp samples; else >= 3, < xstride */
  uint32_t spp;                /* >= 2 */
  uint32_t iterations;         /* 0 .. 8; 0 copies the film */
  float    sigma_l;            /* finite, > 0 */
  uint32_t normal_power_log2;  /* 0 .. 10: w_n = (N.N')^(2^normal_power_log2); 7 is (N.N')^128 */
  uint32_t on_device;          /* 0: both pointers are host memory, 1: both are device memory (HBM) */
  uint32_t reserved[5];        /* must be 0 */
} phx_denoise;

/* ---- first-hit guide channels: what the camera rays of a frame met, as a film of 8 floats a pixel ------------------------ */
/* A pass of its own beside the frame (phx_dev_render_guides): camera rays are never stored, the ray of (seed, film pixel, absolute sample
 * index) is rebuilt from the pixel and jitter tables, so the pass revisits exactly the first hits a frame with the same seed shades.  It
 * launches none of the frame's kernels and changes no frame.  The film is W x H of the preprocessed scene's camera, the jitter table the one
 * of the device's phx_options.samples_per_pixel (spp), 1 <= samples = G <= spp.  All arithmetic is fp32 without contraction, in the order
 * written.  For pixel p and samples s = 0 .. G - 1, in this order:
 *   ray       (o, d) = the camera ray of key (sampler_seed, p, s), pinhole or lens, as the frame builds it
 *   hit       the closest hit along it, tmax = FLT_MAX, ties to the lowest primitive: the hit of phx_dev_trace and of the frame
 *   albedo    a miss, and a hit on an is_emitter material, contribute (1, 1, 1); any other hit the sum over the material's lobes, in lobe
 *             order and starting at (0, 0, 0), of the weight phx_dev_lobe_weights reports at that hit: weight * texel at the hit's
 *             interpolated (s, t) = (w * uv0 + u * uv1) + v * uv2, w = (1 - u) - v, and (pre_weight * term) * that for Fresnel and image-mask
 *             factors, with the shading normal the frame's "normals" channel holds for that sample and the view vector -d; a lobe that is
 *             not there at the hit adds nothing
 *   position  for a hit at distance t:  X_c = o_c + t * d_c  (one multiply, one add);  hits += 1
 *   sums      albedo_sum += albedo (every sample);  X_sum += X and t_sum += t (hits only); per component, in sample order, from 0
 * and the pixel's 8 floats are
 *   0-2 albedo    albedo_sum_c * (1.0f / (float)G)
 *   3   coverage  (float)hits * (1.0f / (float)G)
 *   4-6 position  X_sum_c / (float)hits, or 0 when hits == 0
 *   7   distance  t_sum / (float)hits, or 0 when hits == 0
 * Limits: a mirror's or a glass pane's albedo is its own lobe weight, not what it reflects or shows; emitters and the sky count as white,
 * so that demodulation leaves them alone; there are no normal maps; the guides of a multi-GPU frame are rendered whole by every rank. */
typedef struct phx_guides {
  uint64_t sampler_seed;       /* the frame's phx_frame.sampler_seed */
  uint32_t samples;            /* G: 1 .. samples_per_pixel of the device */
  uint32_t on_device;          /* 0: film is host memory, 1: device memory (HBM) */
  uint32_t reserved[4];        /* must be 0 */
} phx_guides;

/* The guides of phx_dev_denoise_guided: phx_denoise's rule with the changes below.  binary64 without contraction in the order written, fp32
 * values widened first, as there.  G_x are the 8 guide floats of pixel x (the layout above) at guides[x * xstride].
 *   valid     additionally requires the pixel's 8 guide floats to be finite.
 *   PHX_GUIDE_DEMODULATE   the filter runs on the film divided by the first hit's albedo, and multiplies it back:
 *             D_c   = max((double)albedo_c, (double)albedo_floor)
 *             init    C_c = fp32(primary_c / D_c);   V_c = fp32((m2_c * (n / (n - 1))) / (D_c * D_c))
 *             output  primary_c = fp32(C_c * D_c);   m2_c = fp32(((V_c * D_c) * D_c) * ((n - 1) / n))
 *             l_x, e_x, S_p and the biweight are those of the demodulated C and V.
 *   PHX_GUIDE_PLANE        (needs normals_offset != 0) a non-centre tap's weight is w = ((h * w_n) * w_l) * w_x with
 *             w_x = 1 if coverage_p == 0 and coverage_q == 0;  0 if exactly one of them is 0;  otherwise
 *             r   = (N_x * dX_x + N_y * dX_y) + N_z * dX_z      N = p's film normal, dX_c = position_q,c - position_p,c
 *             tol = (sigma_x * plane_scale) * distance_p;   u = fabs(r) / tol;   t = 1 - u * u;   w_x = u < 1 ? t * t : 0
 *             and w_x = (r == 0 ? 1 : 0) when tol == 0.  plane_scale is the world size of one pixel at unit distance
 *             (this camera's 1.12 * tan(fov / 2) / film_height, camera.hpp:113), so tol is sigma_x pixels' worth of surface at p's distance: q is kept when it lies on p's
 *             tangent plane to within that.
 * flags == 0 is phx_dev_denoise bit for bit, whatever the other fields hold (guides may then be NULL). */
enum { PHX_GUIDE_DEMODULATE = 1, PHX_GUIDE_PLANE = 2 };
typedef struct phx_denoise_guides {
  const float* guides;         /* width x height x xstride floats, in the films' memory space (phx_denoise.on_device); not NULL unless flags == 0 */
  uint32_t xstride;            /* floats per pixel of the guide film; >= 8 */
  uint32_t flags;              /* PHX_GUIDE_* */
  float    albedo_floor;       /* DEMODULATE: finite, > 0 */
  float    sigma_x;            /* PLANE: finite, > 0 */
  float    plane_scale;        /* PLANE: finite, > 0 */
  uint32_t reserved[4];        /* must be 0 */
} phx_denoise_guides;

/* ---- film accumulation across frames: pooling finished films of different seeds into one ----------------------------------- */
/* A pass of its own beside the frame (phx_dev_film_accumulate): it reads a finished film and the accumulator, launches none of the frame's
 * kernels and changes no frame.  `acc` is in and out: a film with the channels "primary", optionally "normals", "m2" and ALWAYS "samples",
 * the layout of an adaptive film, so that phx_dev_denoise and the variance identity below read it as it is.  `frame_film` is the finished
 * film of ONE frame with "m2", with or without "samples" (samples_offset_b == 0: every pixel took spp_b samples).  The two films have their
 * own strides and offsets (the fields ending in _a are acc's, in _b the frame film's) and live in the same memory space.
 * Per pixel and colour, in binary64, without contraction, in the order written, fp32 inputs widened first:
 *     n_a = (double)samples_a        n_b = samples_offset_b ? (double)samples_b : (double)spp_b
 *     n   = n_a + n_b
 *   a count (n_a or n_b) that is NaN, infinite or negative makes that pixel's primary rgb, m2 and samples NaN, and no other pixel's; its
 *   normals stay acc's.  This is tested first.  Otherwise
 *   n_b == 0:  the pixel of acc is not touched                  (a rank's unowned pixel, an empty frame)
 *   n_a == 0:  primary rgb, m2 := the frame's floats bit for bit; samples := fp32(n_b)      (accumulating into a zeroed film is the copy)
 *   otherwise
 *     Q_a = (m2_a * n_a) * n_a       Q_b = (m2_b * n_b) * n_b   centred sums of squares of the unit-scale samples: m2 = Q / n^2 for uniform
 *                                                               and for rescaled adaptive pixels alike (phx_adaptive, "variance")
 *     d   = V_b - V_a                                           V = the pixel's "primary"
 *     V   = fp32(V_a + (d * n_b) / n)
 *     Q   = (Q_a + Q_b) + ((d * d) * (n_a * n_b)) / n           Chan's rule: the term in d is what "add the m2s" forgets
 *     m2  = fp32((Q / n) / n)
 *     samples = fp32(n)                                         exact up to 2^24 samples a pixel; beyond, the count is rounded: a stated limit
 *   normals (when both films have them, and the pixel is touched: the two last cases): the frame's three floats if any of them != 0, else
 *             acc's: "the last sample with a hit wins", as k_film has it.  A fourth component of primary stays acc's, as does every float
 *             of acc's pixel outside the four channels.
 *   Non-finite colours propagate through the arithmetic above into that pixel alone.
 * After the call the unbiased variance of any pixel's value is m2 * n / (n - 1) with its own "samples": the identity the denoiser and
 * phx_adaptive already rely on.
 * The caller's part, which the call cannot check: the frames must come from different sampler_seeds (path keys and the jitter table both
 * depend on the seed: the same seed twice is the same samples twice); the frames must share paths_per_sample and the scene; the pooled
 * estimate treats all n samples as one sample set; a multi-GPU film must be reduced before it is accumulated (a rank's own film holds
 * zeros in the pixels it does not own).
 * summary (optional) is counted in the same launch from the floats acc's pixel holds AFTER the call: V_c its primary, m2_c, and
 * n = (double)samples.  The counters are integers, so the result is exact and independent of the order of the reduction:
 *     pixels     width * height
 *     invalid    pixels with a non-finite primary rgb, m2 or n, an m2_c < 0 or n < 2
 *     converged  valid pixels that meet the criterion of phx_adaptive at full exposure: per colour
 *                    L = m2_c * (n / (n - 1));   b = tau * (fabs(V_c) + floor);   ok_c = L <= b * b
 *                converged = ok_r && ok_g && ok_b        (tau = 0 is allowed: it counts the pixels with m2 == 0)
 *     samples    the sum over the valid pixels of (uint64_t)min(n, 2^53), truncated, modulo 2^64 */
typedef struct phx_accumulate {
  uint32_t width, height;      /* 1 .. 65536 each */
  uint32_t xstride_a;          /* floats per pixel of acc; 7 .. 24 */
  uint32_t normals_offset_a;   /* 0 = acc has no normals; else >= 3, normals_offset_a + 3 <= xstride_a */
  uint32_t m2_offset_a;        /* required: >= 3, m2_offset_a + 3 <= xstride_a */
  uint32_t samples_offset_a;   /* required: >= 3, < xstride_a */
  uint32_t xstride_b;          /* floats per pixel of frame_film; 6 .. 24 */
  uint32_t normals_offset_b;   /* 0 = the frame film has no normals; else as for acc */
  uint32_t m2_offset_b;        /* required, as for acc */
  uint32_t samples_offset_b;   /* 0 = none: every pixel took spp_b samples; else >= 3, < xstride_b */
  uint32_t spp_b;              /* >= 1 when samples_offset_b == 0; not read otherwise */
  uint32_t on_device;          /* 0: both films are host memory, 1: both are device memory (HBM) */
  float    tau;                /* the summary's threshold; finite, >= 0 */
  float    floor;              /* the summary's floor in film units; finite, >= 0 */
  uint32_t reserved[2];        /* must be 0 */
} phx_accumulate;
typedef struct phx_accumulate_summary {
  uint64_t pixels, invalid, converged, samples;
} phx_accumulate_summary;

/* ---- the tile map: an accumulator film -> one convergence record per tile, so that a frame can leave converged tiles out ----- */
/* A pass of its own beside the frame (phx_dev_film_tile_map): it reads an accumulator film (phx_accumulate's acc: "primary", "m2" and
 * "samples" are read, 7 floats a pixel; normals and every other float of a pixel are not), launches none of the frame's kernels and changes
 * no film.  It writes one phx_tile_record per tile of a grid over the film:
 *     tx = ceil(width / tile_width)      ty = ceil(height / tile_height)
 *     record j * tx + i covers x in [i * tile_width, min((i + 1) * tile_width, width)) and y in [j * tile_height, min((j + 1) * tile_height, height))
 *   rows run top to bottom and tiles left to right: for tile_width == tile_height this is the list phx_tiles_make(width, height, tile_size,
 *   0, 1) produces, in its order; the ragged edge tiles are the narrower ones.  record.tile is usable as a frame's tile as it is.
 * Per pixel, in binary64, without contraction, in the order written, fp32 inputs widened first; V_c its primary, m_c its m2, n = (double)samples:
 *     valid      all six floats finite, every m_c >= 0, n finite and n >= 2               (phx_accumulate's summary: not "invalid")
 *     starved    n finite and 0 <= n < 2, whatever the other floats hold.  A starved pixel is also invalid; it is counted separately
 *                because more samples cure it and never cure a NaN
 *   for a valid pixel, q = n / (n - 1), and per colour
 *     L = m_c * q;   den = fabs(V_c) + floor;   b = tau * den;   ok_c = L <= b * b
 *     converged = ok_r && ok_g && ok_b                                                    (phx_accumulate's summary criterion word for word)
 *     r_c = den > 0 ? sqrt(L) / den : (L == 0 ? 0 : +inf)
 *     r   = fp32(max(r_r, r_g, r_b))        the relative standard error, rounded to fp32 once; it may round to +inf
 * Per tile:
 *     invalid, starved, converged    the counts of those pixels
 *     samples    the sum over the valid pixels of (uint64_t)min(n, 2^53)
 *     worst      the largest r of the tile's valid pixels, +0.0f when there are none
 *   every quantity is an integer count or a maximum of non-negative non-NaN floats, so the result does not depend on the reduction's order.
 * A tile is OPEN when converged < w * h - invalid or starved > 0: a valid pixel still misses the criterion, or a pixel waits for samples.
 * summary (optional): the sums of the records' counts over all tiles (pixels = width * height), tiles = tx * ty, and open, the number of open
 * tiles.  Its first four fields equal phx_accumulate_summary of the same film, tau and floor. */
typedef struct phx_tile_map {
  uint32_t width, height;      /* 1 .. 65536 each */
  uint32_t xstride;            /* floats per pixel of acc; 7 .. 24 */
  uint32_t m2_offset;          /* required: >= 3, m2_offset + 3 <= xstride */
  uint32_t samples_offset;     /* required: >= 3, < xstride */
  uint32_t tile_width, tile_height; /* 4 .. 1024 each */
  uint32_t on_device;          /* 0: film and records are host memory, 1: both are device memory (HBM), 2: the film is device memory and the records host memory */
  float    tau;                /* the criterion's threshold; finite, >= 0 */
  float    floor;              /* the criterion's floor in film units; finite, >= 0 */
  uint32_t reserved[4];        /* must be 0 */
} phx_tile_map;
typedef struct phx_tile_record { /* 40 bytes */
  phx_tile tile;               /* x, y, w, h */
  uint32_t invalid, starved, converged;
  float    worst;
  uint64_t samples;
} phx_tile_record;
typedef struct phx_tile_map_summary {
  uint64_t pixels, invalid, converged, samples, tiles, open;
} phx_tile_map_summary;

/* ---- the display pass: a film's linear radiance -> an 8-bit sRGB image, with the exposure taken from the film itself -------- */
/* A pass of its own beside the frame (phx_dev_film_display): it reads a finished film of ANY layout (only the first three floats of a pixel,
 * "primary" rgb), launches none of the frame's kernels and changes no film.  The image is width x height pixels of 4 bytes, R, G, B, 255,
 * row-major, rows image_pitch bytes apart.  Pixel i is (x, y) = (i mod width, i div width).  Nothing in the rule is implementation-defined:
 * integer operations, fp32 arithmetic without contraction in the order written, two binary64 steps that are spelled out, and powf_ (the
 * library's own deterministic pow: a binary64 log and exp kernel of + - * / fma, rounded to fp32 once).
 * Histogram: made iff PHX_DISPLAY_AUTO_EXPOSURE is set, or summary is given, or histogram is given.
 *     a pixel is `invalid` when r, g or b is not finite.  Otherwise
 *     Y = fp32((0.2126 * r + 0.7152 * g) + 0.0722 * b)      in binary64, fp32 inputs widened first: the denoiser's weights in its order
 *     Y <= 0 counts as `unlit`.  Otherwise
 *     bin = clamp((bits(Y) >> 20) - 888, 0, 255)            8 bins an octave over [2^-16, 2^16), the ends open-ended, in integer operations
 *     counted = the sum of the bins = pixels - invalid - unlit
 *   The counts are 64-bit integers, exact in any order.  A bin is linear inside its octave and is read below as if it were logarithmic: bin
 *   k stands for 2^((2k + 1) / 16 - 16), the logarithmic middle of [2^(k / 8 - 16), 2^((k + 1) / 8 - 16)), so the estimate can be off by up
 *   to 0.09 stop.
 * Exposure (PHX_DISPLAY_AUTO_EXPOSURE; N = counted, C_k = h_0 + ... + h_(k-1)):
 *     N == 0:  scale := the struct's scale, from_histogram = 0       (a film with no lit pixel)
 *     otherwise, from_histogram = 1 and
 *     c_lo = (N * low_q16) >> 16        c_hi = (N * high_q16 + 65535) >> 16            ranks, 64-bit integers
 *     w_k  = the overlap of bin k's rank range [C_k, C_k + h_k) with [c_lo, c_hi)
 *     W = sum of w_k                    S = sum of w_k * (2k + 1)
 *     p = fp32((double)S / (double)(16 * W) - 16.0)                  the mean log2 luminance between the percentiles
 *     Ybar = powf_(2.0f, p)
 *     scale = fminf(fmaxf(key / Ybar, min_scale), max_scale)
 *   Without the flag scale := the struct's scale and from_histogram = 0.
 * Encode, per colour c of every pixel (an invalid pixel by the same rule: NaN -> 0, +inf -> white), fp32:
 *     x = scale * v_c;  if !(x > 0) then x = 0  (NaN, negatives, -0, -inf);  x = fminf(x, 65536.0f)
 *     PHX_TONE_CLAMP:     t = x
 *     PHX_TONE_REINHARD:  t = (x * (1 + x / (white * white))) / (1 + x)
 *     PHX_TONE_ACES:      t = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)
 *     t = fminf(t, 1.0f)
 *     e = t <= 0.0031308f ? 12.92f * t : 1.055f * powf_(t, 1.0f / 2.4f) - 0.055f                  the sRGB transfer function
 *     q = 255.0f * e + d       d = 0.5f, or under PHX_DISPLAY_DITHER d = (B[y & 3][x & 3] + 0.5f) / 16.0f with the 4 x 4 ordered matrix
 *                              B = {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}}
 *     code = (uint8_t)(int)q   q lies in [0, 256)
 * Out of scope: colour management beyond the sRGB curve, hue-preserving and local operators, temporal smoothing of the exposure (feed
 * summary.scale of one call back as the next one's scale, min_scale and max_scale), outputs of more than 8 bits. */
enum { PHX_DISPLAY_DITHER = 1, PHX_DISPLAY_AUTO_EXPOSURE = 2 };            /* phx_display.flags */
enum { PHX_TONE_CLAMP = 0, PHX_TONE_REINHARD = 1, PHX_TONE_ACES = 2 };     /* phx_display.tone */
typedef struct phx_display {
  uint32_t width, height;      /* 1 .. 65536 each */
  uint32_t xstride;            /* floats per film pixel; 3 .. 24.  Only the first three are read */
  uint32_t image_pitch;        /* bytes per image row; 0 = 4 * width, else a multiple of 4 and >= 4 * width.  Bytes past 4 * width of a row are never written */
  uint32_t on_device;          /* 0: film and image are host memory, 1: both are device memory (HBM), 2: the film is device memory, the image host memory (the preview) */
  uint32_t flags;              /* PHX_DISPLAY_*; other bits are refused */
  uint32_t tone;               /* PHX_TONE_* */
  float    scale;              /* the exposure multiplier; finite, > 0.  Under AUTO_EXPOSURE the fallback */
  float    white;              /* PHX_TONE_REINHARD only: finite, > 0 */
  float    key;                /* AUTO_EXPOSURE only: finite, > 0 */
  uint32_t low_q16;            /* AUTO_EXPOSURE only: the percentiles in units of 1 / 65536, low_q16 < high_q16 */
  uint32_t high_q16;           /* <= 65536 */
  float    min_scale;          /* AUTO_EXPOSURE only: finite, > 0 */
  float    max_scale;          /* finite, >= min_scale */
  uint32_t reserved[2];        /* must be 0 */
} phx_display;
typedef struct phx_display_summary {
  uint64_t pixels, invalid, unlit, counted;
  float    scale;              /* the multiplier the image was encoded with */
  uint32_t from_histogram;     /* 1: scale came from the histogram, 0: it is the struct's */
} phx_display_summary;

/* ---- reprojection: carrying an accumulator film from one camera of a static scene to another ------------------------------- */
/* A pass of its own beside the frame (phx_dev_film_reproject): it reads the accumulator under the old camera (acc_from), the guide films
 * (phx_guides) under the old and the new camera (guides_from, guides_to) and the two cameras; it writes EVERY float of acc_to, a film of
 * acc_from's layout.  It reads no scene, launches none of the frame's kernels and changes no frame.  The layout fields are those of
 * phx_accumulate's acc ("primary", "normals", "m2", "samples"; here the normals are required: the plane test reads them); both guide films
 * have 8 floats a pixel at xstride_g floats apart.  All four films are width x height pixels, row-major, in the same memory space.
 * All arithmetic is binary64, without contraction, in the order written; fp32 inputs are widened first; a result is rounded to fp32 once,
 * where fp32(...) says so.
 * Cameras (derived once, on the host, for `from` and `to` alike; M = to_world, row-vector convention, M[4 * i + j] = x[i][j]):
 *     O     = (M[12], M[13], M[14])                                      the origin; a lens camera is projected as the pinhole through O
 *     a b c = M[0] M[1] M[2];  d e f = M[4] M[5] M[6];  g h k = M[8] M[9] M[10]
 *     A = e * k - f * h;   B = f * g - d * k;   C = d * h - e * g;       det = (a * A + b * B) + c * C
 *     I     = | A / det   (c * h - b * k) / det   (b * f - c * e) / det |    the inverse of the upper 3 x 3: adjugate over determinant
 *             | B / det   (a * k - c * g) / det   (c * d - a * f) / det |
 *             | C / det   (b * g - a * h) / det   (a * e - b * d) / det |
 *     zoom  = 1.12 * tan((double)fov * 0.5)       ratio = W / H       W = (double)film_width, H = (double)film_height
 *   det == 0, or a non-finite det, O, I or zoom, or zoom == 0, is refused ("from" / "to"), as is a film size other than width x height.
 *   What is inverted is the camera ray of the frame (camera.hpp:113-139): camera-space direction (nx * ratio * zoom, ny * zoom, -1) through
 *   M.  The frame's own zoom and ratio are fp32; the difference cancels below, like everything that both projections share.
 *     project(K, X):   D = X - O_K (per component);   c_j = (D_x * I_0j + D_y * I_1j) + D_z * I_2j,  j = x, y, z
 *                      behind the camera unless c_z < 0 (a NaN is behind it).  t = -c_z
 *                      fx = ((c_x / t) / (ratio * zoom) + 0.5) * W;    fy = (0.5 - (c_y / t) / zoom) * H
 * Output pixel p = (x, y), G = its 8 floats of guides_to:
 *   no history      every float of acc_to's pixel := 0.  (phx_accumulate's n_a == 0 case then makes the next frame the copy there.)
 *   coverage_p > 0 is false (the sky, a NaN):  no history, counted as no_geometry.  Otherwise X = G's position and
 *     project(from, X), project(to, X); X behind either camera: no history (counted, like every case below, as disoccluded)
 *     sx = x + (fx_from - fx_to);   sy = y + (fy_from - fy_to)         motion, not position: under from == to, sx == x and sy == y exactly,
 *                                                                      wherever inside the pixel the mean hit position lies
 *     unless sx > -1 && sx < W && sy > -1 && sy < H (false for a NaN):  no history
 *     x0 = floor(sx);  y0 = floor(sy);  tx = sx - x0;  ty = sy - y0
 *   taps, in this order:  (x0, y0) w = (1 - tx) * (1 - ty);  (x0 + 1, y0) w = tx * (1 - ty);  (x0, y0 + 1) w = (1 - tx) * ty;
 *                         (x0 + 1, y0 + 1) w = tx * ty
 *     A tap q counts only if  w > 0;  q is inside the film;  acc_from's pixel q is valid by phx_denoise's definition with its own samples
 *     (primary rgb, m2 and N finite, every m2 >= 0, n finite and >= 2);  q's 8 floats of guides_from are finite;  coverage_q > 0;  and q
 *     is the same surface:  with dX = X - position_q (per component), N = q's normal in acc_from and
 *         tol = plane_scale_from * distance_q        plane_scale_from = zoom_from / H: a pixel's world size at unit distance
 *         r = (N_x * dX_x + N_y * dX_y) + N_z * dX_z;          fabs(r) <= sigma_plane * tol
 *         dd = (dX_x * dX_x + dX_y * dX_y) + dX_z * dX_z;      lim = sigma_dist * tol;   dd <= lim * lim
 *     (a NaN fails either test).  No tap counts: no history.
 *   result, over the taps that count, in tap order; every sum STARTS AT its first term (not at 0.0):
 *     Wsum = sum of w_i;   u_i = w_i / Wsum
 *     n   = sum of u_i * n_i;   V_c = sum of u_i * V_i,c;   m_c = sum of (u_i * u_i) * m2_i,c      the denoiser's B / W^2: taps as independent
 *     n_out = min(n, (double)max_history);   if n > n_out:  m_c = m_c * (n / n_out)     the history claims no more confidence than
 *                                                                                      max_history samples of the same spread
 *     primary rgb = fp32(V_c);   m2 = fp32(m_c);   samples = fp32(n_out)
 *     every other float of the pixel (the normals, a fourth component of primary, ...) is that of the counting tap of largest w, ties to
 *     the first in tap order.
 *   So one tap of weight 1 with n <= max_history is the copy of acc_from's pixel bit for bit (u = 1; 1 * v == v, -0 included), and a
 *   non-finite value of a pixel of acc_from or guides_from makes that pixel no tap and reaches no other pixel.
 * summary (optional), integers counted in the same launch, exact in any order:  pixels = width * height = reused + no_geometry +
 *   disoccluded;  samples = the sum over the reused pixels of (uint64_t) of the "samples" float written, truncated, modulo 2^64.
 * Limits: view-dependent shading (glossy, mirror, glass) is carried as if it were diffuse; the sky and whatever is seen through a specular
 * path get no history (the guides hold the FIRST hit); the lens is projected as a pinhole, so out-of-focus regions smear; m2 of a bilinear
 * mix treats the taps as independent and understates the variance of the result; objects do not move; nothing here clamps the history against
 * the new frame (phx_outlier_clamp, DESIGN 23, is a pass of its own for that); the film size cannot change with the camera; a multi-GPU film is reduced first. */
typedef struct phx_reproject {
  uint32_t   width, height;      /* 1 .. 65536 each */
  uint32_t   xstride_a;          /* floats per pixel of acc_from and acc_to; 10 .. 24 */
  uint32_t   normals_offset_a;   /* required: >= 3, normals_offset_a + 3 <= xstride_a */
  uint32_t   m2_offset_a;        /* required: >= 3, m2_offset_a + 3 <= xstride_a */
  uint32_t   samples_offset_a;   /* required: >= 3, < xstride_a */
  uint32_t   xstride_g;          /* floats per pixel of guides_from and guides_to; 8 .. 64 */
  uint32_t   on_device;          /* 0: the four films are host memory, 1: all are device memory (HBM) */
  phx_camera from, to;           /* film_width x film_height of both must be width x height */
  float      sigma_plane;        /* finite, > 0: the tangent-plane tolerance in pixels' worth of surface */
  float      sigma_dist;         /* finite, > 0: the distance tolerance, likewise */
  uint32_t   max_history;        /* >= 2: the most samples a reprojected pixel may claim */
  uint32_t   reserved[3];        /* must be 0 */
} phx_reproject;
typedef struct phx_reproject_summary {
  uint64_t pixels, reused, no_geometry, disoccluded, samples;
} phx_reproject_summary;

/* ---- the outlier clamp: pulling a film's pixels back to what a neighbourhood can justify ----------------------------------- */
/* A pass of its own beside the frame (phx_dev_film_outlier_clamp): film A is clamped, pixel by pixel and colour by colour, against bounds
 * taken from the neighbourhood of the same pixel in a reference film B, into film_out, a film of A's layout.  Two uses of the one rule:
 *   despeckle      B is A itself: a finished frame film against its own neighbourhood, before it is pooled or filtered
 *                  (PHX_OUTLIER_EXCLUDE_CENTRE | PHX_OUTLIER_UPPER_ONLY: a firefly does not vouch for itself, and nothing is brightened)
 *   history clamp  A is a reprojected accumulator (phx_reproject), B the first frame film under the new camera, before that frame is
 *                  pooled into A: the variance clipping of temporal filters.  It also bounds phx_reproject's "carried as if it were
 *                  diffuse" limit: a carried value cannot leave what the new frame's neighbourhood shows.
 * It reads no scene, launches none of the frame's kernels and changes no frame.  A has xstride_a floats a pixel, "primary" rgb first, "m2"
 * (3 floats) at m2_offset_a and "samples" (1 float) at samples_offset_a, each 0 = none; B has xstride_b floats a pixel, of which only the
 * first three, "primary" rgb, are read.  The films are width x height pixels, row-major, in the same memory space.
 * All arithmetic is binary64, without contraction, in the order written; fp32 inputs are widened first; a result is rounded to fp32 once,
 * where fp32(...) says so.  Pixel p = (x, y), A_c its colour c of A, n its samples float:
 *   skipped        A_r, A_g or A_b is not finite, or A has "samples" and n is not a finite number > 0:  every float of the pixel is A's.
 *                  (A pixel without history is all zero after phx_reproject, and stays so: phx_accumulate then starts it afresh.)
 *   taps           q = p + (dx, dy), dy = -r .. r outer, dx = -r .. r inner, r = radius; under PHX_OUTLIER_EXCLUDE_CENTRE without (0, 0).
 *                  A tap counts if q is inside the film and B_q's r, g and b are finite.
 *   luminance      l_q = (0.2126 * R + 0.7152 * G) + 0.0722 * B      of B_q: the denoiser's weights in its order
 *   trim           `trim` times: the counting tap of largest l_q is dropped, among equals the earlier one in tap order.  (A second
 *                  firefly in the window would otherwise widen the bounds that should catch the first.)
 *   k              the number of taps left.  k < min_taps: the pixel is untouched and counted as unbounded.
 *   bounds         per colour c, sums starting at 0.0 and running over the taps left in tap order:
 *                      mu = (sum of B_q,c) / k
 *                      s  = (sum of (B_q,c - mu) * (B_q,c - mu)) / k
 *                      w  = gamma * sqrt(s) + floor
 *                      hi = mu + w;   lo = mu - w
 *   clamp          A_c > hi:  A'_c = fp32(hi).   A_c < lo and PHX_OUTLIER_UPPER_ONLY is not set:  A'_c = fp32(lo).   Otherwise the float
 *                  keeps its bits.  The pixel is counted as clamped if any colour was, else as inside.
 *   m2             (when A has it)  v = m2_c.  If colour c was clamped and A_c != 0:  f = A'_c / A_c;  if 0 <= f < 1:  v = (v * f) * f, as
 *                  if every sample of the pixel had been scaled by f.
 *   samples cap    if clamped_history > 0, the pixel was clamped in any colour and n > clamped_history:  samples := fp32(clamped_history)
 *                  and, with n_out = (double)clamped_history, v = v * (n / n_out) for all three colours, as phx_reproject's cap does: a
 *                  history that had to be clamped claims no more confidence than clamped_history samples.  Counted as capped.
 *   rounding       m2_c = fp32(v) where either step applied to it; otherwise the float keeps its bits.  Every other float of the pixel
 *                  is A's.
 * So a constant film comes back bit for bit (s = 0, hi = lo = mu = the value: neither comparison holds), and with B = A, the centre
 * included, trim = 0 and floor = 0 no pixel is clamped once gamma >= sqrt(k - 1) (Samuelson's inequality; k <= 49).
 * summary (optional), integers counted in the same launch, exact in any order:  pixels = width * height = skipped + unbounded + inside +
 *   clamped;  capped counts the pixels whose samples were cut.
 * Aliasing: film_out may be film exactly (the same address) or share no byte with it; ref may be film exactly (then xstride_b must be
 *   xstride_a) or share no byte with it; film_out may be ref exactly or share no byte with it.  Any partial overlap is refused.  Where
 *   film_out shares bytes with ref the call works from a device copy of ref, made inside the call and released before it returns, so
 *   every bound is taken from B as it was before the call.
 * Limits: the clamp is BIASED: it removes the energy the outliers carried (a film whose fireflies hold 10 % of its mean comes back some
 *   10 % darker), and a true small highlight narrower than the window is cut like a firefly; the taps know no surface (no normals or
 *   guides in the window), so bounds taken across an edge are wide; colours are clamped one by one, so a clamped pixel can change hue;
 *   objects do not move; a multi-GPU film is reduced first. */
enum { PHX_OUTLIER_EXCLUDE_CENTRE = 1, PHX_OUTLIER_UPPER_ONLY = 2 };       /* phx_outlier_clamp.flags */
typedef struct phx_outlier_clamp {
  uint32_t width, height;      /* 1 .. 65536 each */
  uint32_t xstride_a;          /* floats per pixel of film and film_out; 3 .. 24 */
  uint32_t m2_offset_a;        /* 0 = A has no m2; else >= 3, m2_offset_a + 3 <= xstride_a */
  uint32_t samples_offset_a;   /* 0 = A has no samples; else >= 3, < xstride_a, outside m2 */
  uint32_t xstride_b;          /* floats per pixel of ref; 3 .. 24.  Only the first three are read */
  uint32_t on_device;          /* 0: the three films are host memory, 1: all are device memory (HBM) */
  uint32_t flags;              /* PHX_OUTLIER_*; other bits are refused */
  uint32_t radius;             /* 1 .. 3: the window is (2 * radius + 1) pixels square */
  uint32_t trim;               /* 0 .. 3: the brightest taps left out of the bounds */
  uint32_t min_taps;           /* 1 .. (2 * radius + 1)^2: fewer taps left bound nothing */
  float    gamma;              /* finite, >= 0: the bounds' half width in standard deviations of the taps */
  float    floor;              /* finite, >= 0: added to the half width, in film units */
  uint32_t clamped_history;    /* 0 = no cap; else the most samples a clamped pixel may claim (needs samples_offset_a) */
  uint32_t reserved[2];        /* must be 0 */
} phx_outlier_clamp;
typedef struct phx_outlier_clamp_summary {
  uint64_t pixels, skipped, unbounded, inside, clamped, capped;
} phx_outlier_clamp_summary;

/* ---- statistics ------------------------------------------------------------------------ */
/* The shade kernels (shade_general.hip: launch_shade picks one per launch from the scene's closures, images and lens and from the pass).
 * phx_stats::shade_kernels has bit (family * PHX_SHADE_PASSES + pass) set for every one the last frame launched. */
enum {
  PHX_SHADE_PASS_LATER   = 0, /* a later bounce */
  PHX_SHADE_PASS_CAMERA  = 1, /* the camera rays' pass, through a pinhole */
  PHX_SHADE_PASS_LENS    = 2, /* the camera rays' pass, through a lens (aperture_radius != 0) */
  PHX_SHADE_PASSES       = 3
};
enum {
  PHX_SHADE_FAMILY_LAMBERT1 = 0,  /* k_shade<2>: at most one Lambert lobe per material */
  PHX_SHADE_FAMILY_LAMBERT  = 1,  /* k_shade<1>: Lambert lobes only */
  PHX_SHADE_FAMILY_GENERAL  = 2,  /* k_shade_g: 2 + (PERHIT | TEX << 1 | ENV << 2), i.e. families 2 to 9 */
  PHX_SHADE_G_PERHIT        = 1,  /* ... some closure weight depends on the hit (glass) */
  PHX_SHADE_G_TEX           = 2,  /* ... some lobe reads an image */
  PHX_SHADE_G_ENV           = 4,  /* ... the environment has an image */
  PHX_SHADE_FAMILY_MASK     = 10, /* k_shade_g with image masks on closure mixes (PERHIT, TEX and MASK) */
  PHX_SHADE_FAMILY_MASK_ENV = 11, /* ... and an environment image */
  PHX_SHADE_FAMILIES        = 12,
  PHX_SHADE_KERNELS         = 36  /* PHX_SHADE_FAMILIES * PHX_SHADE_PASSES */
};
typedef struct phx_stats {
  uint64_t camera_samples;   /* primary rays generated */
  uint64_t rays_closest;     /* non-masked slots presented to closest-hit trace */
  uint64_t rays_shadow;      /* non-masked shadow rays traced */
  uint64_t rays_masked;      /* shadow rays masked before trace (src/kernels/cpu/spt.hpp:138-141) */
  uint64_t tiles;
  uint64_t trace_launches;   /* k_trace launches (each traces closest-hit + pending shadow rays) */
  double   trace_ms;         /* sum of HIP-event durations of the k_trace launches */
  double   closest_ms;       /* = trace_ms (kept for ABI stability) */
  double   shadow_ms;        /* 0: shadow rays are traced inside k_trace */
  double   shade_ms;         /* generate + shade/NEE + integrate + film kernels */
  double   frame_ms;         /* wall time start..join on the host */
  uint64_t bvh_nodes;
  uint64_t bvh_bytes;
  uint64_t triangles;
  double   preprocess_ms;    /* wall time of the last phx_dev_preprocess */
  double   bvh_build_ms;     /* of which: tree construction (host SAH, or device LBVH incl. its upload of the triangles) */
  /* the k_trace launch plan of the preprocessed scene (trace.hip: trace_plan) */
  uint64_t trace_block;      /* threads per k_trace workgroup: 256, 512 or 1024 */
  uint64_t trace_ntop;       /* top-of-tree elements staged in LDS by every workgroup */
  uint64_t trace_levels;     /* per-lane stack entries (= tree depth - 1, at least 2) */
  uint64_t trace_waves_per_cu; /* resident k_trace waves per compute unit with that LDS footprint */
  uint64_t bvh_depth;        /* levels of the 8-wide tree (<= 64) */
  uint64_t paths_in_flight;  /* paths carried per wavefront pass in the last frame (pixels of a batch x samples) */
  /* traversal work of the last frame — filled only by the instrumented build (make variant NAME=count EXTRA=-DPHX_COUNT=1),
   * 0 otherwise; [0] closest-hit rays, [1] shadow rays */
  uint64_t node_visits_lds[2]; /* nodelets read from the top of the tree staged in LDS */
  uint64_t node_visits_mem[2]; /* nodelets read through the vector L1 (4 x 16 B per lane) */
  uint64_t tri_tests[2];       /* triangle records read through the vector L1 (3 x 16 B per lane) and tested */
  uint64_t instrumented;       /* 1 if this library counts them */
  uint64_t wave_iters;         /* instrumented: k_trace loop iterations summed over waves */
  uint64_t node_block_execs;   /* instrumented: iterations in which at least one lane visited a node */
  uint64_t tri_block_execs;    /* instrumented: iterations in which at least one lane tested a triangle */
  uint64_t refills;            /* instrumented: refill rounds summed over waves */
  uint64_t idle_lane_iters;    /* instrumented: lanes without a ray at the node block, summed over iterations */
  uint64_t tri_pending_lane_iters; /* instrumented: lanes that sit out the node block because triangles of their last node are pending */
  uint64_t stack_pushes[8];    /* instrumented: pushes onto the per-lane stack of pending sibling groups, by the depth they land at (7 = 7 and deeper) */
  double   bvh_cost_model;     /* modelled traversal cost of the tree in use (the optimal collapse's objective; area units) */
  uint64_t trace_lds_levels;   /* ... of which this many live in LDS (deep trees: the rest spills to HBM) */
  uint64_t bvh_built_on_device; /* 1: the tree in use was built on the device */
  double   shade_kernel_ms;    /* of shade_ms: the shade/NEE/integrate launches alone (k_shade or k_shade_g), HIP events */
  uint64_t shade_launches;     /* how many of them */
  uint64_t shade_general;      /* 1: the scene has non-Lambert closures and runs k_shade_g; 0: k_shade (Lambert only) */
  double   primary_ms;         /* of trace_ms: the camera-ray launches (k_trace_primary: one packet walk per 64 rays), HIP events; closest_ms
                                  holds the k_trace launches alone */
  uint64_t primary_launches;   /* how many of them (one per pass) */
  uint64_t primary_packets;    /* instrumented: packets of 64 camera rays walked by k_trace_primary ... */
  uint64_t primary_fallbacks;  /* ... of which this many had rays in more than one direction octant and took the per-lane walk */
  uint64_t primary_node_tests; /* instrumented: node tests per packet (one test serves its 64 rays), summed */
  uint64_t primary_tri_tests;  /* instrumented: triangles a packet reached (each is tested by its 64 lanes), summed */
  uint64_t primary_tri_lanes_hit; /* instrumented: lanes whose closest hit a triangle test improved, summed */
  uint64_t device_bytes;       /* HBM this device object holds right now: tree, scene tables, ray / hit / shadow queues, path state, batch buffer */
  uint64_t tri_pairs_pending;  /* instrumented: pending (ray, triangle) pairs of a wave at its triangle-block executions, summed (each execution tests one per pending lane) */
  uint64_t tri_pairs_hist[8];  /* instrumented: those executions by the wave's pending pairs: <= 8, 16, 24, 32, 48, 64, 96, more */
  uint64_t trace_stack_packed; /* 1: k_trace keeps 5-byte stack entries in LDS (deep trees: more of the tree is staged), 0: 8-byte entries */
  uint64_t shade_kernels;      /* bit (family * 3 + pass) set for every shade kernel launched by the last frame (PHX_SHADE_FAMILY_*, PHX_SHADE_PASS_*) */
} phx_stats;

typedef struct phx_device phx_device; /* opaque */

/* ---- the xpu_t surface ----------------------------------------------------------------- */
/* xpu_t::discover (src/xpu.cpp:7-9): number of usable gfx950 devices (0 when options->host_only). */
int         phx_discover(const phx_options* options, int* num_devices);
/* T::make(const parsed_options_t&) (src/xpu/cpu.hpp:35).  NULL on failure (see phx_last_error). */
phx_device* phx_dev_make(const phx_options* options);
/* xpu_t::preprocess (src/xpu.hpp:20; cpu.cpp:219 -> details_t::reset :35): flatten + upload scene, build BVH.
 * A call refused before anything is uploaded (PHX_ERR_STATE, a malformed scene) keeps the previous scene renderable; one that fails later
 * (the device builder's fatal error, a tree too deep, out of memory) leaves the device WITHOUT a scene: phx_dev_start and the stage-level
 * entry points answer PHX_ERR_STATE until a phx_dev_preprocess succeeds. */
int         phx_dev_preprocess(phx_device* dev, const phx_scene* scene);
/* xpu_t::start (src/xpu.hpp:26; cpu.cpp:223-238): non-blocking; spawns the driver thread. */
int         phx_dev_start(phx_device* dev, const phx_frame* frame);
/* xpu_t::join (src/xpu.hpp:32; cpu.cpp:240): blocks; returns the frame's status. */
int         phx_dev_join(phx_device* dev);
/* ~xpu_t.  A frame that was started and not joined is JOINED here: destroy blocks until that frame has ended, and the frame's
 * next_tile / add_tile callbacks may still be called while it does — whatever they use must outlive this call.  The device's driver
 * thread (one per device, asleep between frames) ends with it; a device that is never destroyed leaves that thread asleep at exit. */
void        phx_dev_destroy(phx_device* dev);

/* last error message of the calling thread (a frame's error is handed to the thread that calls phx_dev_join) */
const char* phx_last_error(void);
int         phx_dev_get_stats(const phx_device* dev, phx_stats* out);
/* Adaptive sampling (phx_adaptive above) for every frame this device starts from now on; NULL turns it off, which is the default.  Needs no
 * scene.  PHX_ERR_STATE while a frame is started and not yet joined; PHX_ERR_ARG, with the field's name in the message, for a value outside
 * the ranges stated at the struct or a non-zero reserved word: the previous setting then stays in force. */
int         phx_dev_set_adaptive(phx_device* dev, const phx_adaptive* a /* NULL: off */);
/* Replaces the camera of the preprocessed scene and nothing else: no validation of the scene, no tree, no upload.  Every later
 * frame, guide pass and stage hook is what it would be on a device preprocessed with the same scene under this camera, bit for bit: the
 * kernels rebuild their camera rays from the camera's fields on each launch and pick the lens or pinhole instantiation then.
 * PHX_ERR_STATE without a preprocessed scene and while a frame is started and not joined; PHX_ERR_ARG for a camera phx_dev_preprocess would
 * refuse, with its text, and for a film_width or film_height other than the preprocessed scene's (the film, the tile plan and the pixel
 * tables are sized by them).  A refused call leaves the device as it was. */
int         phx_dev_set_camera(phx_device* dev, const phx_camera* camera);

/* ---- native tile queue: job::tiles_t (src/jobs/tiles.hpp:10-90) ----------------------- */
/* make(): row-major tile_size x tile_size tiles with edge remainders (tiles.hpp:49-89);
 * rank/world shard the queue for multi-GPU: tile (tx, ty) belongs to rank (tx + s*ty) % world, s the smallest odd
 * number >= 3 coprime to world (diagonals over the film: balanced whatever the row length). */
typedef struct phx_tiles phx_tiles;
phx_tiles*  phx_tiles_make(uint32_t width, uint32_t height, uint32_t tile_size, uint32_t rank, uint32_t world);
/* make_list(): a queue of the caller's own tiles in the caller's order (the open tiles of a tile map).  The list is copied;
 * count == 0 (tiles may then be NULL) gives a queue that is drained at once.  No geometry is checked here: the frame's own "tile outside
 * the film" check stays the only one.  NULL (PHX_ERR_ARG) for a null list with count > 0. */
phx_tiles*  phx_tiles_make_list(const phx_tile* tiles, uint32_t count);
int         phx_tiles_next(void* tiles /* phx_tiles* */, phx_tile* out); /* a phx_next_tile_fn */
uint32_t    phx_tiles_count(const phx_tiles* tiles);
void        phx_tiles_reset(phx_tiles* tiles);
void        phx_tiles_free(phx_tiles* tiles);

/* ---- stage-level entry points (used by the parity tests; all synchronous) ------------- */
/* Closest-hit (shadow==0) or any-hit (shadow==1) trace of n host rays against the device BVH:
 * the device equivalent of stream_mbvh_kernel_t::trace (kernels/cpu/stream_bvh_kernel.cpp:159).
 * o,d: xyz per ray; tmax per ray.  Outputs: t (hit distance, or tmax on miss), u,v, prim
 * (index into scene_t::triangles() order, 0xffffffff on miss; for any-hit 0/1-style hit flag in hit[]). */
int phx_dev_trace(phx_device* dev, uint32_t n, const float* o, const float* d, const float* tmax,
                  int shadow, float* t, float* u, float* v, uint32_t* prim, uint8_t* hit);

/* bsdf_t::f (src/bsdf.cpp:113-131) and bsdf_t::sample (:133-248) evaluated on the device for
 * material `material` with shading normal n[i]: KAT hooks.  Vectors are xyz per item.  They take no texture coordinates: a colour
 * texture is left out (the baked weight is used) and a material with image-masked lobes is PHX_ERR_ARG. */
int phx_dev_bsdf_f(phx_device* dev, uint32_t material, uint32_t n_items, const float* n,
                   const float* wi, const float* wo, float* f_out);
int phx_dev_bsdf_sample(phx_device* dev, uint32_t material, uint32_t n_items, const float* n,
                        const float* wi, const float* u2, float* wo_out, float* f_out,
                        float* pdf_out, uint32_t* flags_out);

/* The image lookup the shade kernel applies to a textured lobe, run on the device for texture `texture` (0-based index into
 * phx_scene.textures of the preprocessed scene) at n coordinates st (s, t per item): rgb per item.  A parity hook like phx_dev_bsdf_f.
 * The texture table is uploaded only when some lobe of the preprocessed scene is textured or masked, or its environment has an image: for any
 * other scene every call returns PHX_ERR_ARG, as does an index past the table. */
int phx_dev_texture_lookup(phx_device* dev, uint32_t texture, uint32_t n, const float* st, float* rgb);

/* The closure weights of a hit as the shade kernel resolves them: for every baked lobe of material `material` of the preprocessed scene (its
 * surface closures in table order; emission / background entries are not lobes) the weight at shading normal n[i], view direction wi[i]
 * (hits.wi) and texture coordinates st[i] — Fresnel factor, colour texture and image mask alike.  w receives PHX_MAX_LOBES x 3 floats per
 * item (zero past the material's lobes); bit k of kept[i] is set when lobe k is there at that hit.  st is not read (and may be NULL) for a
 * scene in which no lobe has a texture or a mask.  A parity hook.  PHX_ERR_STATE before preprocess, PHX_ERR_ARG for a material out of range. */
int phx_dev_lobe_weights(phx_device* dev, uint32_t material, uint32_t n_items, const float* n, const float* wi, const float* st,
                         float* w, uint32_t* kept);

/* The environment's e on a miss as the shade kernel computes it (phx_material.emission_texture: mapping, lookup and multiply), run on
 * the device for n directions dirs (x, y, z per item) against the preprocessed scene's environment: rgb per item.  A parity hook.
 * PHX_ERR_STATE before preprocess; PHX_ERR_ARG when the scene's environment has no image. */
int phx_dev_environment_lookup(phx_device* dev, uint32_t n, const float* dirs, float* rgb);

/* The light sample of next-event estimation as the shade kernel draws it, in the light_sampling mode the device was made with: for n triples
 * u3 (pick, lu, lv per item) the chosen light (index into the scene's emissive face sets in mesh x face-set order), the triangle inside it (face
 * order of the set), the barycentrics (bu, bv) of triangle_t::sample, the point P = bu * a + bv * b + (1 - bu - bv) * c and the light's lpdf.
 * A parity hook: it runs the device function k_shade_g runs.  PHX_ERR_STATE before preprocess. */
int phx_dev_light_sample(phx_device* dev, uint32_t n, const float* u3, uint32_t* light, uint32_t* tri, float* bary, float* P, float* pdf);

/* The emission next-event estimation uses at that light sample: for the same n triples u3 (pick, lu, lv per item) the (s, t) of the sampled
 * point by the rule of phx_material.emission_uv_texture (st, 2 floats per item) and the light's emission e times the texel there (e, 3 floats
 * per item).  A light whose material has no image returns its constant e and st = (0, 0).  A parity hook: it runs the device function
 * k_shade_g runs.  PHX_ERR_STATE before preprocess. */
int phx_dev_light_emission(phx_device* dev, uint32_t n, const float* u3, float* st, float* e);

/* The environment sample of next-event estimation under PHX_LIGHT_INCLUDE_ENVIRONMENT as the shade kernel draws it: for n triples u3 (pick, lu,
 * lv per item) the pick (light[k] == nlights marks an environment pick; for a mesh light every other output is zero), the texel (i, j: 2 words
 * per item), (s, t) (2 floats), the direction d (3 floats), pdf = p_env * pdf_omega (0 where the rule issues no shadow ray) and the environment's e
 * in direction d (3 floats; zero where pdf is 0).  A parity hook: it runs the device functions k_shade_g runs.  PHX_ERR_STATE before preprocess;
 * PHX_ERR_ARG when the preprocessed scene does not sample its environment.  Under that option phx_dev_light_sample answers an environment pick
 * with light = nlights, tri = 0xffffffff and zeros elsewhere, and phx_dev_light_emission with zeros. */
int phx_dev_environment_sample(phx_device* dev, uint32_t n, const float* u3, uint32_t* light, uint32_t* texel, float* st, float* dir, float* pdf, float* e);

/* One pass of the film stage with phx_frame.moments_channel on, run on the caller's data: radiance holds num_pixels x num_samples records
 * of 4 floats (r, g, b, unused), pixel-major, the samples samples_done .. samples_done + num_samples - 1 of every pixel; acc holds 6 floats
 * per pixel, primary rgb and m2 rgb, as the previous passes left them (zeros before the first), and receives both after this pass by the
 * rule of phx_frame.moments_channel with s0 = samples_done.  A parity hook: it runs the film kernel of such a frame itself.  It needs a
 * device but no scene.  PHX_ERR_ARG for a null array or num_pixels x num_samples of 2^31 or more. */
int phx_dev_film_moments(phx_device* dev, uint32_t num_pixels, uint32_t num_samples, uint32_t samples_done, float inv,
                         const float* radiance, float* acc);

/* The selection of adaptive sampling after a round that ended at samples_done, run on the caller's data: the decision of phx_adaptive for
 * every row named by `active`, the rescale of the rows that stop (samples = (float)samples_done), and the rows that go on, in the order of
 * `active` (a STABLE compaction), in survivors[0 .. *num_survivors - 1].  acc holds 7 floats per row: primary rgb, m2 rgb, samples; rows that
 * go on and rows outside `active` come back unchanged.  A parity hook: it runs the selection kernels of such a frame themselves.  It needs a
 * device but no scene.  PHX_ERR_ARG for a null array, samples_done < 2, samples_done >= spp, an index >= num_rows, indices that do not
 * ascend strictly, num_active > num_rows, or a phx_adaptive that phx_dev_set_adaptive would refuse. */
int phx_dev_adaptive_select(phx_device* dev, uint32_t num_active, const uint32_t* active /* indices into acc rows, ascending; NULL = 0..num_active-1 */,
                            uint32_t num_rows, float* acc /* num_rows x 7: primary rgb, m2 rgb, samples; in and out */,
                            uint32_t samples_done, uint32_t spp, const phx_adaptive* a,
                            uint32_t* survivors /* num_active words */, uint32_t* num_survivors);

/* The film denoiser (phx_denoise above states the rule): film_in -> film_out, both width x height x xstride floats, row-major; film_out may
 * equal film_in, and must not overlap it otherwise.  Synchronous.  It needs a device but no scene.  Call it after phx_dev_join, and on
 * several GPUs after the films are reduced.  PHX_ERR_STATE while a frame is started and not joined; PHX_ERR_ARG, with the field's name in
 * the message, for a value outside the ranges stated at the struct, channels that overlap "primary" (floats 0 .. 2) or each other, a
 * non-zero reserved word or a null pointer.  Its working memory (96 bytes a pixel) is allocated in the call and freed before it returns
 * (PHX_ERR_OOM if it cannot be had): phx_stats.device_bytes and every later frame are what they were. */
int phx_dev_denoise(phx_device* dev, const phx_denoise* d, const float* film_in, float* film_out);
/* HIP-event times of the last phx_dev_denoise of this device in milliseconds: ms[0] the pack stage, ms[1 .. 8] the iterations (0 for those
 * not run), ms[9] the unpack stage (with the film copy when film_out != film_in), ms[10] the whole call on the host's clock. */
int phx_dev_denoise_times(const phx_device* dev, double* ms /* 11 */);

/* The first-hit guide film of the preprocessed scene (phx_guides above states the rule): film receives W x H x 8 floats, row-major.
 * Synchronous, on the device object's stream.  PHX_ERR_STATE without a preprocessed scene and while a frame is started and not joined;
 * PHX_ERR_ARG, with the field's name in the message, for samples outside 1 .. samples_per_pixel, on_device above 1, a non-zero reserved
 * word or a null film.  Its working memory (the film's pixel table, the jitter table and, for a host film, the film itself) is allocated
 * in the call and freed before it returns: phx_stats.device_bytes and every later frame are what they were. */
int phx_dev_render_guides(phx_device* dev, const phx_guides* g, float* film /* W * H * 8 fp32 */);
/* Times of the last phx_dev_render_guides of this device in milliseconds: ms[0] the kernel (HIP events), ms[1] the whole call on the host's clock
 * (the tables' upload, the allocations and, for a host film, the download included). */
int phx_dev_guides_times(const phx_device* dev, double* ms /* 2 */);
/* phx_dev_denoise with guides (phx_denoise_guides above).  g == NULL or g->flags == 0: phx_dev_denoise itself.  Otherwise the same calls'
 * checks, and PHX_ERR_ARG, with the field's name in the message, for unknown flags, PHX_GUIDE_PLANE without normals_offset, xstride < 8, a
 * non-finite or non-positive albedo_floor (DEMODULATE) / sigma_x / plane_scale (PLANE), a non-zero reserved word or null guides.  Working
 * memory: 96 bytes a pixel, 112 under PHX_GUIDE_PLANE, and the guide film's copy for host films.  phx_dev_denoise_times reports its stages. */
int phx_dev_denoise_guided(phx_device* dev, const phx_denoise* d, const phx_denoise_guides* g, const float* film_in, float* film_out);

/* Film accumulation (phx_accumulate above states the rule): frame_film is pooled into acc, width x height pixels each, row-major, of
 * xstride_a and xstride_b floats; summary may be NULL.  Synchronous, one kernel launch.  It needs a device but no scene.  Call it after
 * phx_dev_join, and on several GPUs after the films are reduced.  PHX_ERR_STATE while a frame is started and not joined; PHX_ERR_ARG, with
 * the field's name in the message, for a value outside the ranges stated at the struct, channels that overlap "primary" (floats 0 .. 2) or
 * each other, samples_offset_a == 0, spp_b == 0 without a samples channel, a non-zero reserved word, a null pointer, or acc overlapping
 * frame_film: acc is then untouched.  Its working memory (the counters and, for host films, the two films' copies) is allocated in the
 * call and freed before it returns (PHX_ERR_OOM if it cannot be had): phx_stats.device_bytes and every later frame are what they were. */
int phx_dev_film_accumulate(phx_device* dev, const phx_accumulate* a, float* acc, const float* frame_film, phx_accumulate_summary* summary /* may be NULL */);
/* Times of the last phx_dev_film_accumulate of this device in milliseconds: ms[0] the kernel (HIP events), ms[1] the whole call on the
 * host's clock (the allocations and, for host films, the uploads and the download included). */
int phx_dev_accumulate_times(const phx_device* dev, double* ms /* 2 */);

/* The tile map (phx_tile_map above states the rule): acc, width x height pixels of xstride floats, row-major, is read, and records receives
 * ceil(width / tile_width) * ceil(height / tile_height) records; summary is host memory whatever on_device says and may be NULL.
 * Synchronous, one kernel launch, a workgroup per tile.  It needs a device but no scene.  PHX_ERR_STATE while a frame is started and not
 * joined; PHX_ERR_ARG, with the field's name in the message, for a value outside the ranges stated at the struct, channels that overlap
 * "primary" or each other, a non-zero reserved word, a null pointer ("acc", "records") or records sharing a byte with acc: records and
 * summary are then untouched.  Its working memory (the counters and, for host memory, the copies of film and records) is allocated in the
 * call and freed before it returns (PHX_ERR_OOM if it cannot be had): phx_stats.device_bytes and every later frame are what they were. */
int phx_dev_film_tile_map(phx_device* dev, const phx_tile_map* m, const float* acc, phx_tile_record* records, phx_tile_map_summary* summary /* may be NULL */);
/* Times of the last phx_dev_film_tile_map of this device in milliseconds: ms[0] the kernel (HIP events), ms[1] the whole call on the
 * host's clock (the allocations and, for host memory, the upload and the download included). */
int phx_dev_tile_map_times(const phx_device* dev, double* ms /* 2 */);

/* The display pass (phx_display above states the rule): film, width x height pixels of xstride floats, row-major, becomes image, height
 * rows of width RGBA8 pixels image_pitch bytes apart; image must be 4-byte aligned, and film and image must not share a byte.  summary and
 * histogram (256 counts) are host memory whatever on_device says, and either may be NULL.  Synchronous: at most three kernel launches
 * (histogram, exposure, encode) with no host round trip between them.  It needs a device but no scene.  PHX_ERR_STATE while a frame is
 * started and not joined; PHX_ERR_ARG, with the field's name in the message, for a value outside the ranges stated at the struct, unknown
 * flags, a non-zero reserved word, a null or misaligned pointer, or film overlapping image: image, summary and histogram are then
 * untouched.  Its working memory (the counters and, for host memory, the copies of film and image) is allocated in the call and freed
 * before it returns (PHX_ERR_OOM if it cannot be had): phx_stats.device_bytes and every later frame are what they were. */
int phx_dev_film_display(phx_device* dev, const phx_display* p, const float* film, uint8_t* image,
                         phx_display_summary* summary /* may be NULL */, uint64_t* histogram /* 256, may be NULL */);
/* Times of the last phx_dev_film_display of this device in milliseconds: ms[0] histogram + exposure and ms[1] the encode (HIP events; 0 for
 * a stage not run), ms[2] the whole call on the host's clock (the allocations, uploads and the image's download included). */
int phx_dev_display_times(const phx_device* dev, double* ms /* 3: histogram + exposure, encode, call */);

/* Reprojection (phx_reproject above states the rule): acc_from, guides_from and guides_to are read, every float of acc_to is written;
 * summary may be NULL.  Synchronous, one kernel launch.  It needs a device but no scene.  PHX_ERR_STATE while a frame is started and not
 * joined; PHX_ERR_ARG, with the field's name in the message, for a value outside the ranges stated at the struct, channels that overlap
 * "primary" or each other, a camera whose film is not width x height or whose matrix is singular or not finite ("from" / "to"), a
 * non-zero reserved word, a null pointer, or acc_to sharing a byte with any of the three inputs: acc_to is then untouched.  Its working
 * memory (the counters and, for host films, the four films' copies) is allocated in the call and freed before it returns (PHX_ERR_OOM if
 * it cannot be had): phx_stats.device_bytes and every later frame are what they were. */
int phx_dev_film_reproject(phx_device* dev, const phx_reproject* r, const float* acc_from, const float* guides_from, const float* guides_to,
                           float* acc_to, phx_reproject_summary* summary /* may be NULL */);
/* Times of the last phx_dev_film_reproject of this device in milliseconds: ms[0] the kernel (HIP events), ms[1] the whole call on the
 * host's clock (the allocations and, for host films, the uploads and the download included). */
int phx_dev_reproject_times(const phx_device* dev, double* ms /* 2 */);

/* The outlier clamp (phx_outlier_clamp above states the rule): film is clamped against ref's neighbourhoods into film_out; summary may be
 * NULL.  Synchronous, one kernel launch.  It needs a device but no scene.  PHX_ERR_STATE while a frame is started and not joined;
 * PHX_ERR_ARG, with the field's name in the message, for a value outside the ranges stated at the struct, channels that overlap
 * "primary" or each other, unknown flags, clamped_history without a samples channel, a non-zero reserved word, a null pointer ("film",
 * "ref", "film_out") or a partial overlap of two films ("ref": with film; "film_out": with film or ref): film_out and summary are then
 * untouched.  Its working memory (the counters, ref's copy where film_out shares bytes with ref and, for host films, the films' copies)
 * is allocated in the call and freed before it returns (PHX_ERR_OOM if it cannot be had): phx_stats.device_bytes and every later frame
 * are what they were. */
int phx_dev_film_outlier_clamp(phx_device* dev, const phx_outlier_clamp* c, const float* film, const float* ref, float* film_out,
                               phx_outlier_clamp_summary* summary /* may be NULL */);
/* Times of the last phx_dev_film_outlier_clamp of this device in milliseconds: ms[0] the kernel (HIP events), ms[1] the whole call on the
 * host's clock (the allocations, ref's copy and, for host films, the uploads and the download included). */
int phx_dev_outlier_clamp_times(const phx_device* dev, double* ms /* 2 */);

/* The acceleration structure of the preprocessed scene as the traversal kernels read it (a parity hook: the tests check that every box the
 * device builder stored contains what hangs below it).  Copies min(capacity, size) bytes of the pool of 64-byte elements (csrc/bvh8.h:
 * element 0 = root nodelet) to `out`, stores the pool's size in *bytes and the per-scene grid of the nodelets' origins in grid6
 * (lo.xyz, cell.xyz; origin = fma(i, cell, lo)). */
int phx_dev_copy_bvh(phx_device* dev, void* out, uint64_t capacity, uint64_t* bytes, float* grid6);

/* ---- geometry updates -----------------------------------------------------------------------------------------------------
 * phx_dev_update_geometry takes new vertex positions and normals for the preprocessed scene at a fraction of phx_dev_preprocess's cost.
 * `moved` is the committed scene with other vertex positions and normals.  The call re-derives everything that geometry feeds: the
 * triangle records of the pool (v0, e0 = b - a, e1 = c - a), the nodelets, the scene grid, the shade records (flat normals), the vertex
 * normals by pool element, the light tables (every light's area and pick density, the light triangles' positions and normals, the area
 * CDF, the power selection table with the environment's entry: a lamp that is stretched changes its pdf and its selection weight exactly
 * as under a fresh preprocess) — and the corner UVs' order when a rebuild moved the elements.  It does not re-read, re-bake or re-upload
 * materials, lobes, textures and texels, the environment image and its CDF, UV values, options, or the camera (phx_dev_set_camera).
 *
 * PHX_UPDATE_REFIT keeps the tree's topology — slots, masks, child bases, the triangles' places — and recomputes every box bottom-up:
 * a triangle's box from its three vertices, grown by the tree's tolerance delta = 2^-18 (largest extent + largest coordinate of the new
 * bounds); a nodelet's box as the fp32 min / max of its children's; every nodelet encoded again on the scene grid of the NEW bounds, so a
 * scene that moved outside its old bounds needs no fallback.  The pool is then what the builder's emission would write for this topology
 * over the new triangles.  Slot order and cuts are those of the OLD geometry: trace speed degrades with deformation, phx_stats.bvh_cost_model
 * keeps the build's value, and when to rebuild is the caller's decision.  PHX_UPDATE_REBUILD runs the same path but builds a new tree
 * (by options.bvh_builder) and recomputes the traversal plan: the fallback when a deformation has ruined the topology.
 *
 * A frame after an update equals, bit for bit, the frame of a device freshly preprocessed with the moved scene (the film depends on the
 * triangles, not on the tree).  Films accumulated before an update are stale.  Topology changes need phx_dev_preprocess.
 *
 * Refused with PHX_ERR_ARG, the device untouched and still serving its old scene, when any of these differ from the committed scene: the
 * triangle count; a primitive's material word (material | smooth << 31) in scene_t::triangles() order; the number of lights or a light's
 * triangle count; whether any face is smooth; the texture classes (some lobe or emitter reads an image at the hit's UV, some mix factor
 * is an image); also for a vertex that is not finite, for geometry phx_dev_preprocess refuses, for an unknown mode and for a non-zero
 * reserved word.  The face index arrays themselves are not compared: the triangles given are the triangles rendered.
 * PHX_ERR_STATE without a preprocessed scene and while a frame is started and not joined.  A failure after the first device write leaves
 * the device without a scene, as a failed phx_dev_preprocess does.  Everything the call allocates besides the scene's own tables (the new
 * triangles, elem_of_prim, per-element boxes and marks, the tables in primitive order) lives only during the call.  After a refit the
 * device holds no more memory after the call than before: phx_stats.device_bytes is unchanged.  A rebuild sizes the pool and the tables by
 * pool element for the NEW tree and releases what the old one held beyond that: afterwards the device holds exactly what a device freshly
 * preprocessed with the moved scene holds (more or less than before by the difference of the trees' element counts).  The call returns
 * after synchronising the device's stream. */
enum { PHX_UPDATE_REFIT = 0, PHX_UPDATE_REBUILD = 1 };
typedef struct phx_geometry_update {
  uint32_t mode;        /* PHX_UPDATE_* */
  uint32_t reserved[3]; /* must be 0 */
} phx_geometry_update;
typedef struct phx_geometry_summary {
  uint32_t mode, triangles, nodes, levels, lights, light_triangles; /* levels: of nodelets (phx_stats.bvh_depth) */
  float bounds[6];      /* the geometry's new bounds, lo.xyz hi.xyz */
  float delta;          /* the triangle boxes' inflation on those bounds */
} phx_geometry_summary;
int phx_dev_update_geometry(phx_device* dev, const phx_scene* moved, const phx_geometry_update* u, phx_geometry_summary* summary /* may be NULL */);
/* Times of the last phx_dev_update_geometry of this device in milliseconds, on the host's clock: ms[0] the host's flattening of the moved
 * scene (validation, the walk over the meshes, the light tables, the bounds), ms[1] the uploads (the triangles under a refit, normals,
 * light tables), ms[2] the device's work, each stretch ending in a synchronise (the refit or the rebuild with its scratch allocations, the
 * shade records and the permutations, the release of the call's device buffers; under a rebuild the builder uploads the triangles itself,
 * so that upload is counted here and not in ms[1]), ms[3] the whole call. */
int phx_dev_update_geometry_times(const phx_device* dev, double* ms /* 4 */);

#ifdef __cplusplus
}
#endif
#endif /* PHX_XPU_H */
