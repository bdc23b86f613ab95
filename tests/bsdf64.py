"""A float64 model of the closure layer, for tests: the seven lobe models, the host's parameter maps, bsdf_t's rules (f summed with the
n.wi factor; sample's lobe pick, matched-lobe sum and averaged pdf) and the per-hit mix factor of Blender's glass node.

Written from the formulas of SURVEY Appendix D and the reference lines cited below; it shares no code with oracle/obsdf.h or csrc/bsdf.h.
Inputs are fp32 arrays widened exactly to float64 and every step after that is float64 -- except the lobe pick of bsdf_t::sample
(bsdf.cpp:133-150), a discrete decision on fp32 values that the model takes in fp32 so that it picks the same lobe.

Every quirk of Appendix D is a named switch (QUIRKS); `quirks=True` turns all of them on (the reference), `quirks=False` none (the
textbook model), a set turns on the ones it names.  Besides the pdf a sampler REPORTS, the model gives the TRUE density of each sampling
procedure (`Model.true_pdf`, `ggx_true_density`): the textbook visible-normal density with the textbook Lambda, times what the rational
fit of ggx_sample_slope (microfacet.hpp:351-398) does to it, mapped to wo by the textbook Jacobian.

Directions: bsdf f(wi = to the light, wo = the view); sample(u, wi = the view) -> wo.  Tangent space: y = the shading normal.
"""
import numpy as np

from phosphorus_mk2_amd import abi

PI = np.pi
FLT_EPS = 2.0 ** -23

QUIRKS = {
    "fresnel_half": "Cook-Torrance reflect (GGX and sheen) uses dielectric Fresnel with eta 0.5 (microfacet.hpp:209); textbook: F = 1",
    "g1_world": "the GGX reflect pdf evaluates G1 on the WORLD-space wi (microfacet.hpp:234); textbook: on li",
    "lambda_alpha": "GGX Lambda's alpha = sqrt(cos2phi ax ay + sin2phi ax ay) (microfacet.hpp:342-344); textbook: sqrt(cos2phi ax^2 + sin2phi ay^2)",
    "pdf_precedence": "GGX refract pdf: |eta^2 lo.wh| / d * d (microfacet.hpp:113); textbook: / (d * d)",
    "pdf_side_world": "GGX refract pdf tests the side with the world-space wo.wi (microfacet.hpp:108); textbook: li.y lo.y",
    "jacobian_eta": "GGX refract sampler's Jacobian uses the sampler's inverse eta (microfacet.hpp:165-167); textbook: the eta of f",
    "wh_zero": "Cook-Torrance reflect f is 0 where a component of li + lo is exactly 0 (microfacet.hpp:201)",
    "diffuse_pdf_wi": "Lambert / Oren-Nayar / sheen pdf = n.wi / pi of the FIRST argument (bsdf.cpp:29-60); textbook: |n.wo| / pi",
    "on_degrees": "Oren-Nayar sigma = radians(alpha), alpha read as degrees (params.hpp:38); textbook: sigma = alpha",
}
ALL = frozenset(QUIRKS)

SHEEN_P0 = (25.3245, 3.32435, 0.16801, -1.27393, -4.85967)  # sheen.hpp:20-25, the r -> 0 and r -> 1 fits of L
SHEEN_P1 = (21.5473, 3.82987, 0.19823, -1.97760, -4.32054)
FIT_NUM = (0.27385, -0.73369, 0.46341)        # ggx_sample_slope's rational fit of the inverse CDF of slope_y (microfacet.hpp:390-393)
FIT_DEN = (0.093073, 0.309420, -1.0, 0.597999)


def _q(quirks):
    return ALL if quirks is True else (frozenset() if quirks is False else frozenset(quirks))


def f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def dot(a, b):
    return (a * b).sum(-1)


def normalize(v):  # a zero vector stays zero (Vec3::normalize)
    n = np.sqrt(dot(v, v))[..., None]
    return np.where(n != 0, v / np.where(n != 0, n, 1.0), v)


# ---- tangent frame (orthogonal_base_t(n), orthogonal_base.hpp:11-19) and tangent-space trigonometry (vector.hpp:24-72) ------------------
def frame(n):
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    first = (x != y) | (x != z)
    a = np.where(first[:, None], np.stack([z - y, x - z, y - x], 1), np.stack([z - y, x + z, -y - x], 1))
    a = normalize(a)
    return a, n, normalize(np.cross(a, n))


def to_local(F, v):
    return np.stack([dot(F[0], v), dot(F[1], v), dot(F[2], v)], 1)


def to_world(F, l):
    return l[:, 0:1] * F[0] + l[:, 1:2] * F[1] + l[:, 2:3] * F[2]


def sin2_theta(v):
    return np.maximum(0.0, 1.0 - v[:, 1] * v[:, 1])


def cos_sin_phi(v):
    s = np.sqrt(sin2_theta(v))
    with np.errstate(all="ignore"):
        c = np.where(s == 0, 1.0, np.clip(v[:, 0] / s, -1.0, 1.0))
        t = np.where(s == 0, 0.0, np.clip(v[:, 2] / s, -1.0, 1.0))
    return c, t


def osl_fresnel_dielectric(cosi, eta):  # the OSL helper src/shaders/fresnel.h:1-19: no eta == 0 case, no inversion
    c = np.abs(cosi)
    g = eta * eta - 1.0 + c * c
    pos = g > 0
    with np.errstate(all="ignore"):
        gs = np.sqrt(np.where(pos, g, 1.0))
        A = (gs - c) / (gs + c)
        B = (c * (gs + c) - 1.0) / (c * (gs - c) + 1.0)
        return np.where(pos, 0.5 * A * A * (1.0 + B * B), 1.0)


def fresnel_dielectric(cosi, eta):  # fresnel::dielectric, math/fresnel.hpp:6-28
    cosi, eta = np.broadcast_arrays(np.asarray(cosi, np.float64), np.asarray(eta, np.float64))
    with np.errstate(all="ignore"):
        out = osl_fresnel_dielectric(cosi, np.where(cosi < 0, 1.0 / eta, eta))
    return np.where(eta == 0, 1.0, out)


def fresnel_mix_factor(ior, n, view):  # fresnel_dielectric_node.osl:16-20 on I = view, N = n, backfacing = N.I < 0
    f = max(1.0e-5, float(ior))
    c = dot(view, n)
    return osl_fresnel_dielectric(c, np.where(c < 0, 1.0 / f, f))


# ---- host parameter maps (scene_flatten.cpp bake_material; params.hpp:36-43, 86-99) --------------------------------------------------------
def roughness_to_alpha(r):
    """the polynomial in log(max(r, 1e-5)), clamped to [1e-4, 1].  It is not monotonic: r = 0 gives 0.296, its minimum is ~0.0093
    near r = 1.5e-4, so the 1e-4 clamp is never reached."""
    x = np.log(max(float(r), 1e-5))
    a = 1.62142 + 0.819955 * x + 0.1734 * x * x + 0.0171201 * x ** 3 + 0.000640711 * x ** 4
    return min(1.0, max(1e-4, a))


def oren_nayar_ab(alpha, quirks=True):
    s = float(alpha) * PI / 180.0 if "on_degrees" in _q(quirks) else float(alpha)
    s2 = s * s
    return 1.0 - s2 / (2.0 * (s2 + 0.33)), 0.45 * s2 / (s2 + 0.09)


def sheen_L(x, r):  # sheen.hpp:30-38
    t = (1.0 - r) ** 2
    a, b, c, d, e = (t * p0 + (1.0 - t) * p1 for p0, p1 in zip(SHEEN_P0, SHEEN_P1))
    with np.errstate(invalid="ignore"):
        return a / (1.0 + b * np.power(x, c)) + d * x + e


def sheen_L5_of(materials):
    """L(0.5, r) of the first sheen lobe of the material table (the process-wide static of sheen.hpp:57, as the device fixes it)"""
    for m in materials:
        for l in m.lobes:
            if l.type == abi.LOBE_SHEEN:
                return float(sheen_L(0.5, float(np.float32(l.r))))
    return 0.0


class Lobe:
    """one lobe after add_lobe + precompute (bsdf.hpp:54-82), parameters in float64"""

    def __init__(self, d, quirks=True):
        w = lambda t: np.array([float(np.float32(x)) for x in t])
        self.type, self.weight, self.pre = d.type, w(d.weight), w(d.pre_weight)
        self.fac_mode, self.fac_ior = d.fac_mode, float(np.float32(d.fac_ior))
        self.eta, self.refract, self.r = float(np.float32(d.eta)), int(d.refract), float(np.float32(d.r))
        self.a = self.b = self.ax = self.ay = 0.0
        t = d.type
        if t in (abi.LOBE_DIFFUSE, abi.LOBE_OREN_NAYAR):
            self.flags = abi.BSDF_REFLECT | abi.BSDF_DIFFUSE
            if t == abi.LOBE_OREN_NAYAR:
                self.a, self.b = oren_nayar_ab(float(np.float32(d.alpha)), quirks)
        elif t == abi.LOBE_REFLECTION:
            self.flags = abi.BSDF_REFLECT | abi.BSDF_SPECULAR
        elif t == abi.LOBE_REFRACTION:
            self.flags = abi.BSDF_TRANSMIT | abi.BSDF_SPECULAR
        elif t == abi.LOBE_MICROFACET:
            self.flags = abi.BSDF_TRANSMIT if d.refract else abi.BSDF_REFLECT
            self.ax, self.ay = roughness_to_alpha(np.float32(d.xalpha)), roughness_to_alpha(np.float32(d.yalpha))
        elif t == abi.LOBE_SHEEN:
            self.flags = abi.BSDF_REFLECT | abi.BSDF_GLOSSY
        elif t == abi.LOBE_TRANSPARENT:
            self.flags = abi.BSDF_TRANSMIT
        else:
            raise ValueError(t)

    @property
    def ct(self):  # evaluated by the Cook-Torrance reflect f (GGX reflect, sheen)
        return self.type == abi.LOBE_SHEEN or (self.type == abi.LOBE_MICROFACET and not self.refract)

    def weight_at(self, n, view):
        """(k, 3) weight at the hit and whether the lobe is there: (pre * term) * weight under a Fresnel mix, dropped when all zero"""
        k = len(n)
        if self.fac_mode == abi.FAC_NONE:
            return np.tile(self.weight, (k, 1)), np.ones(k, bool)
        fac = fresnel_mix_factor(self.fac_ior, n, view)
        term = fac if self.fac_mode == abi.FAC_MIX_B else 1.0 - fac
        w = (self.pre[None, :] * term[:, None]) * self.weight[None, :]
        return w, (w != 0).any(1)


# ---- GGX (microfacet.hpp:306-435) -------------------------------------------------------------------------------------------------
def ggx_D(ax, ay, v):
    c2 = v[:, 1] * v[:, 1]
    with np.errstate(all="ignore"):
        tan2 = sin2_theta(v) / c2
        cp, sp = cos_sin_phi(v)
        e = (cp * cp / (ax * ax) + sp * sp / (ay * ay)) * tan2
        d = 1.0 / (PI * ax * ay * c2 * c2 * (1.0 + e) ** 2)
    return np.where(np.isinf(tan2), 0.0, d)


def ggx_Lambda(ax, ay, v, quirks=True):
    with np.errstate(all="ignore"):
        att = np.abs(np.sqrt(sin2_theta(v)) / v[:, 1])
        cp, sp = cos_sin_phi(v)
        a2 = cp * cp * ax * ay + sp * sp * ax * ay if "lambda_alpha" in _q(quirks) else cp * cp * ax * ax + sp * sp * ay * ay
        x2 = a2 * att * att
        lam = 0.5 * x2 / (1.0 + np.sqrt(1.0 + x2))  # = (-1 + sqrt(1 + x2)) / 2 without the cancellation
    return np.where(np.isinf(att), 0.0, lam)


def ggx_G1(ax, ay, v, quirks=True):
    return 1.0 / (1.0 + ggx_Lambda(ax, ay, v, quirks))


def slope_fit(v):
    return (v * (v * (v * FIT_NUM[0] + FIT_NUM[1]) + FIT_NUM[2])) / (v * (v * (v * FIT_DEN[0] + FIT_DEN[1]) + FIT_DEN[2]) + FIT_DEN[3])


def slope_fit_derivative(v):
    N = ((FIT_NUM[0] * v + FIT_NUM[1]) * v + FIT_NUM[2]) * v
    dN = (3 * FIT_NUM[0] * v + 2 * FIT_NUM[1]) * v + FIT_NUM[2]
    D = ((FIT_DEN[0] * v + FIT_DEN[1]) * v + FIT_DEN[2]) * v + FIT_DEN[3]
    dD = (3 * FIT_DEN[0] * v + 2 * FIT_DEN[1]) * v + FIT_DEN[2]
    return (dN * D - N * dD) / (D * D)


_FIT_V = np.linspace(0.0, 1.0, 1 << 16)
_FIT_Z = slope_fit(_FIT_V)


def slope_fit_inverse(z):
    """v in [0, 1] with slope_fit(v) = z (the fit increases on [0, 1]); NaN past slope_fit(1) = 7.26: the fit never draws such |t|"""
    v = np.interp(z, _FIT_Z, _FIT_V)
    for _ in range(3):  # Newton from the table
        v = np.clip(v - (slope_fit(v) - z) / slope_fit_derivative(v), 0.0, 1.0)
    return np.where(z <= _FIT_Z[-1], v, np.nan)


def exact_t_density(t):
    """density of |t| for the exact conditional slope_y / sqrt(1 + slope_x^2) of unit-roughness GGX: 4 / (pi (1 + t^2)^2)"""
    return 4.0 / (PI * (1.0 + t * t) ** 2)


def fit_ratio(t):
    """(density of |t| the fit draws) / (exact density): what the rational fit does to the visible-normal density at |t|"""
    v = slope_fit_inverse(t)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(v), 0.0, 1.0 / (slope_fit_derivative(np.nan_to_num(v)) * exact_t_density(t)))


def ggx_sample_slope(cos_t, u, v):  # TrowbridgeReitzSample11 (microfacet.hpp:351-398)
    with np.errstate(all="ignore"):
        r = np.sqrt(u / (1.0 - u)); phi = 2.0 * PI * v
        sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
        tan_t = sin_t / cos_t
        a = 1.0 / tan_t
        g1 = 2.0 / (1.0 + np.sqrt(1.0 + 1.0 / (a * a)))
        A = 2.0 * u / g1 - 1.0
        tmp = 1.0 / (A * A - 1.0)
        tmp = np.where(tmp > 1e10, 1e10, tmp)
        B = tan_t
        Dv = np.sqrt(np.maximum(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.0))
        sx1, sx2 = B * tmp - Dv, B * tmp + Dv
        sx = np.where((A < 0) | (sx2 > 1.0 / tan_t), sx1, sx2)
        S = np.where(v > 0.5, 1.0, -1.0)
        vv = np.where(v > 0.5, 2.0 * (v - 0.5), 2.0 * (0.5 - v))
        sy = S * slope_fit(vv) * np.sqrt(1.0 + sx * sx)
    normal = cos_t > 0.9999
    return np.where(normal, r * np.cos(phi), sx), np.where(normal, r * np.sin(phi), sy)


def ggx_stretched(ax, ay, li):
    return normalize(np.stack([ax * li[:, 0], li[:, 1], ay * li[:, 2]], 1))


def ggx_sample(ax, ay, li, u, v, quirks=True):
    """-> (wh, the visible-normal pdf the procedure reports); microfacet.hpp:400-434"""
    st = ggx_stretched(ax, ay, li)
    sx, sy = ggx_sample_slope(st[:, 1], u, v)
    cp, sp = cos_sin_phi(st)
    sx, sy = (cp * sx - sp * sy) * ax, (sp * sx + cp * sy) * ay
    wh = normalize(np.stack([-sx, np.ones_like(sx), -sy], 1))
    with np.errstate(all="ignore"):
        pdf = ggx_D(ax, ay, wh) * ggx_G1(ax, ay, li, quirks) * np.abs(dot(li, wh)) / np.abs(li[:, 1])
    return wh, pdf


def ggx_unit_t(ax, ay, li, wh):
    """|t| = |slope_y| / sqrt(1 + slope_x^2) of the unit-roughness slopes (rotated into wi's azimuth) that give wh"""
    cp, sp = cos_sin_phi(ggx_stretched(ax, ay, li))
    with np.errstate(all="ignore"):
        mx, my = -wh[:, 0] / wh[:, 1] / ax, -wh[:, 2] / wh[:, 1] / ay
        x, y = cp * mx + sp * my, -sp * mx + cp * my
        return np.abs(y) / np.sqrt(1.0 + x * x)


def ggx_true_density(ax, ay, li, wh):
    """density over the solid angle of wh of what ggx_sample draws (li.y > 0, wh.y > 0): the textbook visible-normal density
    D G1(li) <li, wh>+ / cos(theta_i) (textbook Lambda) times fit_ratio(|t|); where the stretched cos(theta) > 0.9999 the slopes come
    from D itself: D(wh) cos(theta_h)"""
    with np.errstate(all="ignore"):
        vndf = ggx_D(ax, ay, wh) * ggx_G1(ax, ay, li, False) * np.maximum(0.0, dot(li, wh)) / li[:, 1]
        return np.where(ggx_stretched(ax, ay, li)[:, 1] > 0.9999, ggx_D(ax, ay, wh) * wh[:, 1], vndf * fit_ratio(ggx_unit_t(ax, ay, li, wh)))


# ---- sheen (sheen.hpp:16-64) -------------------------------------------------------------------------------------------------------
def sheen_D(r, v):
    with np.errstate(all="ignore"):
        oor = 1.0 / r if r != 0 else np.inf
        return (2.0 + oor) * np.power(np.sqrt(sin2_theta(v)), oor) / (2.0 * PI)


def sheen_Lambda(r, v, L5):
    ct = v[:, 1]
    with np.errstate(all="ignore"):
        return np.exp(np.where(ct < 0.5, sheen_L(ct, r), 2.0 * L5 - sheen_L(1.0 - ct, r)))


# ---- the lobe models on local directions ------------------------------------------------------------------------------------------
def ct_f(lobe, li, lo, L5, q):  # Cook-Torrance reflect, microfacet.hpp:175-214; GGX or sheen
    wh = li + lo
    ci, co = np.abs(li[:, 1]), np.abs(lo[:, 1])
    live = (li[:, 1] * lo[:, 1] > 0) & (ci != 0) & (co != 0)
    if "wh_zero" in q:
        live &= (wh != 0).all(1)
    wh = normalize(wh)
    with np.errstate(all="ignore"):
        if lobe.type == abi.LOBE_SHEEN:
            d, g = sheen_D(lobe.r, wh), 1.0 / (1.0 + sheen_Lambda(lobe.r, li, L5) + sheen_Lambda(lobe.r, lo, L5))
        else:
            d, g = ggx_D(lobe.ax, lobe.ay, wh), 1.0 / (1.0 + ggx_Lambda(lobe.ax, lobe.ay, li, q) + ggx_Lambda(lobe.ax, lobe.ay, lo, q))
        whf = np.where((wh[:, 1] < 0)[:, None], -wh, wh)
        F = fresnel_dielectric(dot(lo, whf), 0.5) if "fresnel_half" in q else 1.0
        f = d * g * F / (4.0 * ci * co)
    return np.where(live, f, 0.0)


def ct_pdf(lobe, wi_world, li, lo, q):  # microfacet.hpp:216-235
    wh = normalize(li + lo)
    with np.errstate(all="ignore"):
        g1 = ggx_G1(lobe.ax, lobe.ay, wi_world if "g1_world" in q else li, q)
        p = ggx_D(lobe.ax, lobe.ay, wh) * g1 * np.abs(dot(li, wh)) / np.abs(li[:, 1]) / (4.0 * dot(li, wh))
    return np.where(li[:, 1] * lo[:, 1] > 0, p, 0.0)


def ctr_eta(lobe, li):
    return np.where(li[:, 1] > 0, lobe.eta, 1.0 / lobe.eta)


def ctr_f(lobe, li, lo, q):  # Cook-Torrance refract, microfacet.hpp:38-92
    eta = ctr_eta(lobe, li)
    ci, co = li[:, 1], lo[:, 1]
    wh = normalize(li + lo * eta[:, None])
    wh = np.where((wh[:, 1] < 0)[:, None], -wh, wh)
    lw, iw = dot(lo, wh), dot(li, wh)
    live = ~(ci * co > 0) & (ci != 0) & (co != 0) & ~(lw * iw > 0)
    with np.errstate(all="ignore"):
        F = fresnel_dielectric(lw, eta)
        sd = iw + eta * lw
        d = ggx_D(lobe.ax, lobe.ay, wh)
        g = 1.0 / (1.0 + ggx_Lambda(lobe.ax, lobe.ay, li, q) + ggx_Lambda(lobe.ax, lobe.ay, lo, q))
        f = (1.0 - F) * np.abs(d * g * np.abs(lw) * np.abs(iw) / (ci * co * sd * sd))  # eta^2 (1 / eta)^2 = 1
    return np.where(live, f, 0.0)


def ctr_pdf(lobe, wi_world, wo_world, li, lo, q):  # microfacet.hpp:94-116
    eta = ctr_eta(lobe, li)
    wh = normalize(li + lo * eta[:, None])
    with np.errstate(all="ignore"):
        sd = dot(li, wh) + eta * dot(lo, wh)
        j = np.abs(eta * eta * dot(lo, wh))
        j = j if "pdf_precedence" in q else j / (sd * sd)
        p = ggx_D(lobe.ax, lobe.ay, wh) * wh[:, 1] * j
    same = dot(wo_world, wi_world) > 0 if "pdf_side_world" in q else li[:, 1] * lo[:, 1] > 0
    return np.where(same, 0.0, p)


def oren_nayar_f(lobe, li, lo):  # oren_nayar.hpp:9-47
    ci, co = np.abs(li[:, 1]), np.abs(lo[:, 1])
    si, so = np.sqrt(sin2_theta(li)), np.sqrt(sin2_theta(lo))
    cpi, spi = cos_sin_phi(li); cpo, spo = cos_sin_phi(lo)
    mc = np.where((si > 1e-4) & (so > 1e-4), np.maximum(0.0, cpi * cpo + spi * spo), 0.0)
    with np.errstate(all="ignore"):
        sa, tb = np.where(ci > co, so, si), np.where(ci > co, si / ci, so / co)
    return (lobe.a + lobe.b * mc * sa * tb) / PI


def lobe_eval(lobe, F, wi, wo, L5, q):
    """eval() of bsdf.cpp:29-107 on world directions -> (f, pdf); delta lobes are 0, 0"""
    t, k = lobe.type, len(wi)
    if t in (abi.LOBE_DIFFUSE, abi.LOBE_OREN_NAYAR, abi.LOBE_SHEEN):
        pdf = (dot(F[1], wi) if "diffuse_pdf_wi" in q else np.abs(dot(F[1], wo))) / PI
        if t == abi.LOBE_DIFFUSE:
            return np.full(k, 1.0 / PI), pdf
        li, lo = to_local(F, wi), to_local(F, wo)
        return (oren_nayar_f(lobe, li, lo) if t == abi.LOBE_OREN_NAYAR else ct_f(lobe, li, lo, L5, q)), pdf
    if t == abi.LOBE_MICROFACET:
        li, lo = to_local(F, wi), to_local(F, wo)
        if lobe.refract:
            return ctr_f(lobe, li, lo, q), ctr_pdf(lobe, wi, wo, li, lo, q)
        return ct_f(lobe, li, lo, L5, q), ct_pdf(lobe, wi, li, lo, q)
    return np.zeros(k), np.zeros(k)


def lobe_sample(lobe, F, n, wi, u, v, L5, q):
    """one lobe's sampler (bsdf.cpp:133-214 and the lobe files) -> (wo, f, pdf, live, wh); live = False: the path terminates"""
    k = len(wi)
    t = lobe.type
    ones, yes, nowh = np.ones(k), np.ones(k, bool), np.full((k, 3), np.nan)
    if t in (abi.LOBE_DIFFUSE, abi.LOBE_OREN_NAYAR, abi.LOBE_SHEEN):  # cosine-weighted, math/sampling.hpp:23-36
        r, th = np.sqrt(u), 2.0 * PI * v
        l = np.stack([r * np.cos(th), np.sqrt(np.maximum(0.0, 1.0 - u)), r * np.sin(th)], 1)
        wo = to_world(F, l)
        if t == abi.LOBE_DIFFUSE:
            f = ones / PI
        elif t == abi.LOBE_OREN_NAYAR:
            f = oren_nayar_f(lobe, to_local(F, wi), to_local(F, wo))
        else:
            f = ct_f(lobe, to_local(F, wi), to_local(F, wo), L5, q)
        return wo, f, l[:, 1] / PI, yes, nowh
    if t == abi.LOBE_REFLECTION:  # reflection.hpp:8-21
        return -wi + 2.0 * dot(n, wi)[:, None] * n, ones, ones, yes, nowh
    if t == abi.LOBE_TRANSPARENT:  # bsdf.cpp:209-214
        return -wi, ones, ones, yes, nowh
    if t == abi.LOBE_REFRACTION:  # refraction.hpp:10-46: TIR is black (pdf 1, wo left at 0)
        c = dot(n, wi)
        s2 = np.maximum(0.0, 1.0 - c * c)
        out = c > 0
        nn = np.where(out[:, None], n, -n)
        eta = np.where(out, 1.0 / lobe.eta, lobe.eta)
        arg = 1.0 - eta * eta * s2
        ok = arg >= 0
        with np.errstate(invalid="ignore"):
            wo = -wi * eta[:, None] + nn * (eta * np.abs(c) - np.sqrt(arg))[:, None]
        return np.where(ok[:, None], wo, 0.0), ok.astype(np.float64), ones, yes, nowh
    # microfacet
    if lobe.refract and lobe.eta == 1.0:  # microfacet.hpp:120: straight through
        return -wi, ones, ones, yes, nowh
    li = to_local(F, wi)
    wh, dpdf = ggx_sample(lobe.ax, lobe.ay, li, u, v, q)
    iw = dot(li, wh)
    live = (li[:, 1] != 0) & ~(iw < 0)
    with np.errstate(all="ignore"):
        if lobe.refract:  # microfacet.hpp:118-171
            e = np.where(li[:, 1] > 0, 1.0 / lobe.eta, lobe.eta)
            s2t = e * e * np.maximum(0.0, 1.0 - iw * iw)
            live &= ~(s2t >= 1.0)
            lo = -e[:, None] * li + (e * iw - np.sqrt(1.0 - s2t))[:, None] * wh
            ej = e if "jacobian_eta" in q else 1.0 / e
            sd = iw + ej * dot(lo, wh)
            pdf = dpdf * np.abs(ej * ej * dot(lo, wh) / (sd * sd))
            wo = to_world(F, lo)
            f = ctr_f(lobe, to_local(F, wi), to_local(F, wo), q)
        else:  # microfacet.hpp:237-277
            lo = -li + (2.0 * iw)[:, None] * wh
            live &= li[:, 1] * lo[:, 1] > 0
            pdf = dpdf / (4.0 * iw)
            wo = to_world(F, lo)
            f = ct_f(lobe, to_local(F, wi), to_local(F, wo), L5, q)
    return wo, f, pdf, live, wh


class Model:
    """one material (scenes.MaterialDesc) with the L5 of its scene's material table"""

    def __init__(self, material, L5=0.0, quirks=True):
        self.q = _q(quirks)
        self.lobes = [Lobe(d, self.q) for d in material.lobes if d.type not in (abi.LOBE_EMISSIVE, abi.LOBE_BACKGROUND)]
        self.L5 = float(L5)

    def f(self, n, wi, wo):
        """bsdf_t::f (bsdf.cpp:113-131): sum over the lobes on the right side of weight * f * (n.wi); wi = to the light, wo = the view"""
        n, wi, wo = f64(n), f64(wi), f64(wo)
        F = frame(n)
        out = np.zeros_like(wi)
        atl = dot(n, wi)
        reflect = atl * dot(n, wo) > 0
        for l in self.lobes:
            w, keep = l.weight_at(n, wo)
            m = keep & ((reflect & bool(l.flags & abi.BSDF_REFLECT)) | (~reflect & bool(l.flags & abi.BSDF_TRANSMIT)))
            if m.any():
                e, _ = lobe_eval(l, F, wi, wo, self.L5, self.q)
                out += np.where(m[:, None], e[:, None] * w * atl[:, None], 0.0)
        return out

    def pick(self, n, wi, u1):
        """bsdf_t::sample's lobe pick on the lobes at this hit -> (chosen lobe index or -1, remapped u, keep mask)"""
        k = len(n)
        ws = [l.weight_at(n, wi) for l in self.lobes]
        keep = np.stack([kp for _, kp in ws], 1) if self.lobes else np.zeros((k, 0), bool)
        count = keep.sum(1)
        with np.errstate(all="ignore"):  # in fp32, like the reference
            fl = count.astype(np.float32)
            index = np.minimum(np.floor(u1 * fl), np.maximum(fl - np.float32(1), np.float32(0))).astype(np.int64)
            u = np.minimum(u1 * fl - index.astype(np.float32), np.float32(1.0 - FLT_EPS)).astype(np.float64)
        rank = np.cumsum(keep, 1) - 1
        chosen = np.full(k, -1)
        for i in range(len(self.lobes)):
            chosen = np.where(keep[:, i] & (rank[:, i] == index) & (count > 0), i, chosen)
        return chosen, u, ws, keep

    def sample(self, n, wi, u2, with_wh=False):
        """bsdf_t::sample (bsdf.cpp:133-248) -> (wo, f, pdf, flags), a terminated path as (0, 0, 0, 0); with_wh: also the sampled
        microfacet normal (local frame, NaN for other lobes) and the chosen lobe"""
        u1 = np.asarray(u2, np.float32)[:, 0]
        n, wi, u2 = f64(n), f64(wi), f64(u2)
        k = len(wi)
        F = frame(n)
        chosen, u, ws, keep = self.pick(n, wi, u1)
        wo = np.zeros((k, 3)); f = np.zeros((k, 3)); pdf = np.zeros(k); flags = np.zeros(k, np.uint32); whs = np.full((k, 3), np.nan)
        for i, l in enumerate(self.lobes):
            m = chosen == i
            if not m.any():
                continue
            Fm = (F[0][m], F[1][m], F[2][m])
            s_wo, s_f, s_pdf, live, wh = lobe_sample(l, Fm, n[m], wi[m], u[m], u2[m, 1], self.L5, self.q)
            res, p, matched = s_f[:, None] * ws[i][0][m], s_pdf.copy(), np.ones(m.sum())
            reflect = dot(n[m], wi[m]) * dot(n[m], s_wo) > 0
            for j, o in enumerate(self.lobes):
                if j == i or (l.flags & o.flags) != o.flags:
                    continue
                hit = keep[m, j] & ((reflect & bool(o.flags & abi.BSDF_REFLECT)) | (~reflect & bool(o.flags & abi.BSDF_TRANSMIT)))
                e, ep = lobe_eval(o, Fm, wi[m], s_wo, self.L5, self.q)
                res = res + np.where(hit[:, None], e[:, None] * ws[j][0][m], 0.0)
                p, matched = p + np.where(hit, ep, 0.0), matched + hit
            with np.errstate(all="ignore"):
                p = p / matched
            ok = live & (s_pdf != 0)
            wo[m] = np.where(ok[:, None], s_wo, 0.0); f[m] = np.where(ok[:, None], res, 0.0)
            pdf[m] = np.where(ok, p, 0.0); flags[m] = np.where(ok, l.flags, 0); whs[m] = wh
        return (wo, f, pdf, flags, whs, chosen) if with_wh else (wo, f, pdf, flags)

    def reported_pdf(self, n, wi, wo):
        """the pdf a one-lobe material's sampler reports for the direction wo it drew (wi = the view)"""
        l, (n, wi, wo) = self.lobes[0], (np.asarray(a, np.float64) for a in (n, wi, wo))
        F = frame(n)
        li, lo = to_local(F, wi), to_local(F, wo)
        if l.type in (abi.LOBE_DIFFUSE, abi.LOBE_OREN_NAYAR, abi.LOBE_SHEEN):
            return lo[:, 1] / PI
        with np.errstate(all="ignore"):
            wh = self.half_vector(li, lo)
            dpdf = ggx_D(l.ax, l.ay, wh) * ggx_G1(l.ax, l.ay, li, self.q) * np.abs(dot(li, wh)) / np.abs(li[:, 1])
            if not l.refract:
                return dpdf / (4.0 * dot(li, wh))
            e = np.where(li[:, 1] > 0, 1.0 / l.eta, l.eta)
            ej = e if "jacobian_eta" in self.q else 1.0 / e
            sd = dot(li, wh) + ej * dot(lo, wh)
            return dpdf * np.abs(ej * ej * dot(lo, wh) / (sd * sd))

    def half_vector(self, li, lo):
        """the microfacet normal (y > 0) that takes li to lo: reflection, or refraction with f's eta"""
        l = self.lobes[0]
        if not l.refract:
            return normalize(li + lo)
        wh = normalize(li + lo * ctr_eta(l, li)[:, None])
        return np.where((wh[:, 1] < 0)[:, None], -wh, wh)

    def true_pdf(self, n, wi, wo):
        """density over the solid angle of wo of what a one-lobe material's sampler draws (not a delta; wi = the view, li.y > 0)"""
        l, (n, wi, wo) = self.lobes[0], (np.asarray(a, np.float64) for a in (n, wi, wo))
        F = frame(n)
        li, lo = to_local(F, wi), to_local(F, wo)
        if l.type in (abi.LOBE_DIFFUSE, abi.LOBE_OREN_NAYAR, abi.LOBE_SHEEN):
            return np.maximum(0.0, lo[:, 1]) / PI
        wh = self.half_vector(li, lo)
        with np.errstate(all="ignore"):
            if not l.refract:
                return np.where(lo[:, 1] > 0, ggx_true_density(l.ax, l.ay, li, wh) / (4.0 * np.abs(dot(lo, wh))), 0.0)
            eta = ctr_eta(l, li)
            sd = dot(li, wh) + eta * dot(lo, wh)
            return np.where(lo[:, 1] < 0, ggx_true_density(l.ax, l.ay, li, wh) * np.abs(eta * eta * dot(lo, wh)) / (sd * sd), 0.0)


# ---- the sweep: materials and edge inputs ------------------------------------------------------------------------------------------
SWEEP_GGX_ROUGHNESS = (0.0, 1e-3, 0.01, 0.09, 0.3, 1.0, 4.0)
SWEEP_GGX_ANISO = (1.0, 4.0, 16.0)          # xalpha / yalpha of the inputs, xalpha = 0.25
SWEEP_ETA = (1.0, 1.0 - 1e-4, 1.0 + 1e-4, 0.75, 1.33, 1.5, 2.4)
SWEEP_ON_ALPHA = (5.0, 30.0, 90.0)
SWEEP_SHEEN_R = (1e-3, 0.05, 0.4, 1.0, 0.0)
SWEEP_GLASS_IOR = (1e-6, 1.0, 1.45, 3.0)


def sweep_materials():
    """-> [(name, MaterialDesc)]: every single-lobe material of the sweep but sheen, a few closure_zoo mixes and the glass node"""
    from phosphorus_mk2_amd import scenes
    L, M = scenes.LobeDesc, scenes.MaterialDesc
    out = [("diffuse", scenes.diffuse(0.73, 0.73, 0.73))]
    out += [(f"oren_nayar_{a:g}", M([L(abi.LOBE_OREN_NAYAR, (0.6, 0.5, 0.4), alpha=a)])) for a in SWEEP_ON_ALPHA]
    out += [(f"ggx_r{r:g}", M([L(abi.LOBE_MICROFACET, (0.8, 0.7, 0.3), xalpha=r, yalpha=r)])) for r in SWEEP_GGX_ROUGHNESS]
    out += [(f"ggx_aniso{k:g}", M([L(abi.LOBE_MICROFACET, (0.7, 0.7, 0.7), xalpha=0.25, yalpha=0.25 / k)])) for k in SWEEP_GGX_ANISO]
    out += [(f"ggx_refract_eta{e:g}", M([L(abi.LOBE_MICROFACET, (0.9, 0.9, 0.9), eta=e, xalpha=0.2, yalpha=0.2, refract=1)])) for e in SWEEP_ETA]
    out += [("ggx_refract_eta1.5_r0.5", M([L(abi.LOBE_MICROFACET, (0.9, 0.9, 0.9), eta=1.5, xalpha=0.5, yalpha=0.5, refract=1)]))]
    out += [(f"refraction_eta{e:g}", M([L(abi.LOBE_REFRACTION, (0.95, 0.95, 0.95), eta=e)])) for e in SWEEP_ETA]
    out += [("reflection", M([L(abi.LOBE_REFLECTION, (0.9, 0.9, 0.9))])), ("transparent", M([L(abi.LOBE_TRANSPARENT, (0.8, 0.9, 0.8))]))]
    zoo = scenes.closure_zoo()
    out += [("zoo8_diffuse_glossy", zoo[8]), ("zoo9_three_lobes", zoo[9]), ("zoo10_glass_mix", zoo[10])]
    out += [(f"glass_ior{i:g}", scenes.glass(i)) for i in SWEEP_GLASS_IOR]
    return out


def sweep_scenes():
    """-> [(scene, [(material index, name)])]: the sweep on small soups.  The first holds sweep_materials() (its first sheen lobe is
    zoo #9's, r = 0.4); then one scene per sheen r, because L5 is the first sheen lobe's of the table."""
    from phosphorus_mk2_amd import scenes
    mats = sweep_materials()
    out = [(scenes.soup(2 * len(mats), width=8, height=8, materials=[m for _, m in mats]), [(i, nm) for i, (nm, _) in enumerate(mats)])]
    for r in SWEEP_SHEEN_R:
        m = scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_SHEEN, (0.5, 0.2, 0.6), r=r)])
        out.append((scenes.soup(4, width=8, height=8, materials=[m]), [(0, f"sheen_r{r:g}")]))
    return out


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _at_cos(rng, n, c):
    """fp32 unit vectors at (float64) cosine c to the fp32 normals n, random azimuth"""
    n64 = n.astype(np.float64)
    t = np.cross(n64, rng.normal(size=n64.shape))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return _unit(c[:, None] * n64 + np.sqrt(np.maximum(0.0, 1.0 - c * c))[:, None] * t)


def _ulp_walk(rng, v, steps=4):
    """v with each component moved by up to `steps` fp32 ulp"""
    out = v.copy()
    for _ in range(steps):
        d = rng.integers(-1, 2, v.shape)
        out = np.where(d > 0, np.nextafter(out, np.float32(np.inf)), np.where(d < 0, np.nextafter(out, np.float32(-np.inf)), out))
    return out.astype(np.float32)


SET_SIZES = {"random": 6144, "grazing": 512, "normal": 96, "onb_axes": 160, "back": 512, "critical": 96, "u_edges": 108}


def edge_inputs(seed=0, sizes=SET_SIZES, etas=SWEEP_ETA):
    """-> {set name: (n, wi, wo, u2)}, fp32: random; grazing (|n.w| 1e-7 .. 1e-2, either side); wi or wo on the normal or within a few
    ulp of it (both, for one in eight); the ONB's second branch (n.x == n.y == n.z, both signs) and the axis normals; back-facing wi
    and wo; wi within a few ulp of each eta's critical angle, from the side where it has one; u2 at 0, 0.5, 1 - 2^-24."""
    rng = np.random.default_rng(seed)
    rnd = lambda m: _unit(rng.normal(size=(m, 3)))
    u2s = lambda m: rng.random((m, 2)).astype(np.float32)
    out = {}
    k = sizes["random"]
    out["random"] = (rnd(k), rnd(k), rnd(k), u2s(k))
    k = sizes["grazing"]
    n = rnd(k)
    g = lambda: np.where(rng.random(k) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-7, -2, k)
    out["grazing"] = (n, _at_cos(rng, n, g()), _at_cos(rng, n, g()), u2s(k))
    k = sizes["normal"]
    n, i = rnd(k), np.arange(k)
    near = lambda: np.where((rng.random(k) < 0.5)[:, None], n, _ulp_walk(rng, n))
    on_i, on_o = (i % 2 == 0) | (i % 8 == 1), (i % 2 == 1)
    out["normal"] = (n, np.where(on_i[:, None], near(), rnd(k)), np.where(on_o[:, None], near(), rnd(k)), u2s(k))
    k = sizes["onb_axes"]
    s, i = np.float32(1.0 / np.sqrt(3.0)), np.arange(k)
    axes = np.array([[s, s, s], [-s, -s, -s], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    n = axes[i % len(axes)]
    out["onb_axes"] = (n, np.where((i % 5 == 0)[:, None], n, rnd(k)), rnd(k), u2s(k))
    k = sizes["back"]
    n = rnd(k)
    out["back"] = (n, _at_cos(rng, n, -rng.uniform(0, 1, k)), _at_cos(rng, n, -rng.uniform(0, 1, k)), u2s(k))
    crit = []  # cos(theta_c) of wi: outside (n.wi > 0) the sampler uses 1/eta, inside eta
    for e in etas:
        if e < 1.0:
            crit.append(np.sqrt(1.0 - e * e))
        if e > 1.0:
            crit.append(-np.sqrt(1.0 - 1.0 / (e * e)))
    k = sizes["critical"]
    n, i = rnd(k), np.arange(k)
    out["critical"] = (n, _ulp_walk(rng, _at_cos(rng, n, np.array(crit)[i % len(crit)]), 6), rnd(k), u2s(k))
    k = sizes["u_edges"]
    u = np.array([0.0, 0.5, 1.0 - 2.0 ** -24], np.float32)
    grid = np.stack(np.meshgrid(u, u), -1).reshape(-1, 2)
    n, i = rnd(k), np.arange(k)
    out["u_edges"] = (n, _at_cos(rng, n, rng.uniform(-1, 1, k)), rnd(k), grid[i % len(grid)])
    return out


def all_inputs(seed=0):
    """edge_inputs() concatenated -> (n, wi, wo, u2, set name per row)"""
    sets = edge_inputs(seed)
    cat = lambda j: np.ascontiguousarray(np.concatenate([v[j] for v in sets.values()]))
    return cat(0), cat(1), cat(2), cat(3), np.concatenate([[name] * len(v[0]) for name, v in sets.items()])


# ---- holding an fp32 implementation to the model (tests A and C) -------------------------------------------------------------------
U = 2.0 ** -24            # fp32 unit roundoff
RTOL = 512 * 2.0 ** -23   # the stated relative bound: 512 fp32 ulp of 1 (6.1e-5) ...
RTOL_GGX_SAMPLE = 4096 * 2.0 ** -23  # ... and for what ggx_sample feeds (its slope solve cancels: B tmp - sqrt(..) with tmp up to 1e10)
FLOOR = 2.0 ** -20        # plus an absolute floor: this times the largest finite |value| of the quantity over the material's sweep
BAND = 16.0 * U           # rounding band of the fp32 TIR and Fresnel-drop tests, times (1 + eta^2)
GRAZE = 8.0 * U           # plus GRAZE / |cos| relative: an fp32 cosine of unit vectors is off by up to ~3u absolute, and lobes divide by it


def _cos_terms(n, *ws):
    c = np.min([np.abs(dot(normalize(n), normalize(w))) for w in ws], axis=0)
    with np.errstate(divide="ignore"):
        return GRAZE / c


def sample_exclusions(model, n, wi, u2):
    """-> {predicate name: row mask} for sample(): inputs where an fp32 sampler may take the other branch than exact arithmetic, chosen
    on the inputs only (float64 quantities the model computes from them), never on an output:
      side        the sign of n.wi is within fp32 rounding of zero (3-term dot product bound);
      tmp_clamp   ggx_sample_slope's tmp = 1 / (A^2 - 1) reaches the 1e10 clamp (|A^2 - 1| < 1e-7): the slope is then fp32 noise; and
                  for GGX refraction u > 1 - 2^-20, the far end of slope_x's CDF (B tmp - sqrt(..) cancels; wh is near the horizon);
      branch      the stretched cos(theta) within 1e-6 of ggx_sample_slope's 0.9999 switch, or wi within 1e-3 rad of the normal
                  (ggx_sample rotates the slopes into wi's azimuth, which rounding then decides);
      reject      li.wh, or lo.y of the reflected direction, within 1e-6 of zero (the sampler's rejection tests);
      tir         1 - sin^2 of the transmitted direction within 1e-5 (1 + eta^2) of zero (GGX refract: wh is sampled), or refraction's
                  arg = 1 - eta^2 (1 - cos^2) within BAND (1 + eta^2) of zero (its fp32 rounding bound);
      fac         the glass node's g = eta^2 - 1 + cos^2 within BAND (1 + eta^2) of zero (a lobe's weight becomes exactly 0: dropped)."""
    n64, wi64, u64 = f64(n), f64(wi), f64(u2)
    F = frame(n64)
    chosen, u, ws, keep = model.pick(n64, wi64, np.asarray(u2, np.float32)[:, 0])
    k = len(n)
    ex = {name: np.zeros(k, bool) for name in ("side", "tmp_clamp", "branch", "reject", "tir", "fac")}
    ex["side"] = np.abs(dot(n64, wi64)) <= 3 * U * dot(np.abs(n64), np.abs(wi64))
    li = to_local(F, wi64)
    for i, l in enumerate(model.lobes):
        m = chosen == i
        if l.fac_mode != abi.FAC_NONE:
            c = dot(wi64, n64)
            f = max(1.0e-5, l.fac_ior)
            e = np.where(c < 0, 1.0 / f, f)
            ex["fac"] |= np.abs(e * e - 1.0 + c * c) < BAND * (1.0 + e * e)
        if l.type == abi.LOBE_REFRACTION:
            c = dot(n64, wi64)
            e = np.where(c > 0, 1.0 / l.eta, l.eta)
            ex["tir"] |= m & (e != 1.0) & (np.abs(1.0 - e * e * (1.0 - c * c)) < BAND * (1.0 + e * e))  # eta 1: arg = cos^2 >= 0
        if l.type != abi.LOBE_MICROFACET or (l.refract and l.eta == 1.0):
            continue
        st = ggx_stretched(l.ax, l.ay, li)
        with np.errstate(all="ignore"):
            tan_t = np.sqrt(np.maximum(0.0, 1.0 - st[:, 1] ** 2)) / st[:, 1]
            g1 = 2.0 / (1.0 + np.sqrt(1.0 + tan_t * tan_t))
            A = 2.0 * u / g1 - 1.0
        ex["tmp_clamp"] |= m & (st[:, 1] <= 0.9999) & ((np.abs(A * A - 1.0) < 1e-7) | ((u > 1.0 - 2.0 ** -20) & bool(l.refract)))
        ex["branch"] |= m & ((np.abs(st[:, 1] - 0.9999) < 1e-6) | (sin2_theta(normalize(li)) < 1e-6))
        wh, _ = ggx_sample(l.ax, l.ay, li, u, u64[:, 1])
        iw = dot(li, wh)
        ex["reject"] |= m & (np.abs(iw) < 1e-6)
        if l.refract:
            e = np.where(li[:, 1] > 0, 1.0 / l.eta, l.eta)
            ex["tir"] |= m & (np.abs(1.0 - e * e * (1.0 - iw * iw)) < 1e-5 * (1.0 + e * e))
        else:
            ex["reject"] |= m & (np.abs((-li + (2.0 * iw)[:, None] * wh)[:, 1]) < 1e-6)
    return ex


def f_exclusions(model, n, wi, wo):
    """-> {predicate name: row mask} for f(wi, wo), chosen on the inputs only:
      side        the sign of n.wi or n.wo is within fp32 rounding of zero;
      wh_zero     a Cook-Torrance reflect lobe and a component of li + lo within 1e-6 of zero (its exactly-zero test, microfacet.hpp:201);
      fac         the glass node's g within BAND (1 + eta^2) of zero (as for sample)."""
    n64, wi64, wo64 = f64(n), f64(wi), f64(wo)
    F = frame(n64)
    ex = {"side": (np.abs(dot(n64, wi64)) <= 3 * U * dot(np.abs(n64), np.abs(wi64))) |
                  (np.abs(dot(n64, wo64)) <= 3 * U * dot(np.abs(n64), np.abs(wo64)))}
    ex["wh_zero"] = np.zeros(len(n), bool)
    ex["fac"] = np.zeros(len(n), bool)
    if any(l.ct for l in model.lobes):
        ex["wh_zero"] = (np.abs(to_local(F, wi64) + to_local(F, wo64)) < 1e-6).any(1)
    for l in model.lobes:
        if l.fac_mode != abi.FAC_NONE:
            c = dot(wo64, n64)
            f = max(1.0e-5, l.fac_ior)
            e = np.where(c < 0, 1.0 / f, f)
            ex["fac"] |= np.abs(e * e - 1.0 + c * c) < BAND * (1.0 + e * e)
    return ex


def sheen_nonfinite_inputs(model, n, *ws):
    """the documented inputs where f or sample may be non-finite, all of them the sheen lobe's (sheen.hpp:40-64, no guard in the
    reference): a direction within 1e-6 of the normal (cos theta may round to 1 + 1 ulp and Lambda raises 1 - cos theta < 0 to a
    fractional power); f with BOTH directions below the surface (Lambda raises cos theta < 0 to a fractional power); r = 0
    (D = (2 + inf) 0 for every direction)"""
    n64 = f64(n)
    if not any(l.type == abi.LOBE_SHEEN for l in model.lobes):
        return np.zeros(len(n), bool)
    if any(l.type == abi.LOBE_SHEEN and l.r == 0 for l in model.lobes):
        return np.ones(len(n), bool)
    cos = [dot(normalize(n64), normalize(f64(w))) for w in ws]
    out = np.any([1.0 - np.abs(c) < 1e-6 for c in cos], axis=0)
    return out | (np.all([c < 0 for c in cos], axis=0) if len(ws) > 1 else False)


KAPPA_MAX = 1e5          # beyond it fp32 f and pdf of GGX refraction overflow or are not resolved at all: excluded (refract_cond)
REFRACT_COND = 64 * U  # GGX refraction: plus this times kappa^2, kappa = (|li.wh| + |eta lo.wh|) / |li.wh + eta lo.wh| (f, pdf divide by its square)


def refract_condition(model, n, wi, wo):
    """kappa of li.wh + eta lo.wh for the GGX refract lobes of the material, with f's eta and with the sampler's 1 / eta (0 elsewhere)"""
    n64, wi64, wo64 = f64(n), f64(wi), np.asarray(wo, np.float64)
    F = frame(n64)
    li, lo = to_local(F, wi64), to_local(F, wo64)
    out = np.zeros(len(n))
    for l in model.lobes:
        if l.type != abi.LOBE_MICROFACET or not l.refract:
            continue
        for eta in (ctr_eta(l, li), 1.0 / ctr_eta(l, li)):
            wh = normalize(li + lo * ctr_eta(l, li)[:, None])
            with np.errstate(all="ignore"):
                k = (np.abs(dot(li, wh)) + np.abs(eta * dot(lo, wh))) / np.abs(dot(li, wh) + eta * dot(lo, wh))
            out = np.fmax(out, np.where(np.isfinite(k), k, 0.0))
    return out


def fresnel_condition(model, n, wi, wo):
    """the microfacet lobes' Fresnel takes sqrt(g), g = eta^2 - 1 + c^2 (c = lo.wh; eta 0.5 in the reflect f, f's eta in the refract f),
    whose fp32 rounding is ~ 2u (1 + eta^2 + c^2) / |g|: 4u (1 + eta^2 + c^2) / |g| (0 for other lobes)"""
    n64, wi64, wo64 = f64(n), f64(wi), f64(wo)
    F = frame(n64)
    li, lo = to_local(F, wi64), to_local(F, wo64)
    out = np.zeros(len(n))
    for l in model.lobes:
        if l.ct or (l.type == abi.LOBE_MICROFACET and l.refract):
            for a, b in ((li, lo), (lo, li)):  # f(wi, wo) takes lo = the view; the sampler's f takes lo = the sampled direction
                if l.ct:
                    wh = normalize(a + b); e = np.full(len(n), 0.5)
                else:
                    e = ctr_eta(l, a); wh = normalize(a + b * e[:, None]); wh = np.where((wh[:, 1] < 0)[:, None], -wh, wh)
                c = dot(b, wh)
                e = np.where(c < 0, 1.0 / e, e)
                with np.errstate(divide="ignore", invalid="ignore"):
                    k = 4.0 * U * (1.0 + e * e + c * c) / np.abs(e * e - 1.0 + c * c)
                out = np.fmax(out, np.where(np.isfinite(k), k, 0.0))
    return out


def azimuth_condition(model, n, wi, chosen):
    """GGX samplers: ggx_sample rotates the slopes into the azimuth of the stretched wi, cos phi = x / sqrt(1 - y^2), whose fp32 rounding
    is ~ u / sin^2 theta: 8 u / sin^2 theta of the stretched wi (0 for other lobes)"""
    n64, wi64 = f64(n), f64(wi)
    li = to_local(frame(n64), wi64)
    out = np.zeros(len(n))
    for i, l in enumerate(model.lobes):
        if l.type == abi.LOBE_MICROFACET:
            with np.errstate(divide="ignore"):
                out = np.where(chosen == i, 8.0 * U / sin2_theta(ggx_stretched(l.ax, l.ay, li)), out)
    return out


def _close(got, ref, peak, rtol):
    got = np.asarray(got, np.float64).reshape(len(ref), -1); ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(got - ref) <= rtol[:, None] * np.abs(ref) + FLOOR * peak) | (got == ref) | (np.isnan(got) & np.isnan(ref))
    return ok.all(1)


def _peak(a):
    a = np.abs(np.asarray(a, np.float64))
    return max(float(a[np.isfinite(a)].max(initial=0.0)), 1e-30)


def compare(model, n, wi, wo, u2, f_impl, sample_impl):
    """hold an fp32 implementation (f_impl(n, wi, wo), sample_impl(n, wi, u2): the oracle's or the device's) to the model on these rows
    -> dict: rows, excluded rows per predicate (f, sample), allowed non-finite rows, and the rows that fail"""
    fm = model.f(n, wi, wo); fi = f_impl(n, wi, wo)
    sm = model.sample(n, wi, u2); si = sample_impl(n, wi, u2)
    fx, sx = f_exclusions(model, n, wi, wo), sample_exclusions(model, n, wi, u2)
    fx["refract_cond"] = refract_condition(model, n, wi, wo) > KAPPA_MAX
    sx["refract_cond"] = refract_condition(model, n, wi, sm[0].astype(np.float32)) > KAPPA_MAX
    f_ex = np.any(list(fx.values()), axis=0); s_ex = np.any(list(sx.values()), axis=0)
    nf_f = sheen_nonfinite_inputs(model, n, wi, wo)
    nf_s = sheen_nonfinite_inputs(model, n, wi) | (sheen_nonfinite_inputs(model, n, n) & (np.asarray(u2)[:, 0] == 0))  # u = 0 samples the normal
    # f: finite where the model is finite, outside the documented inputs; within the tolerance
    rt_f = RTOL + _cos_terms(f64(n), f64(wi), f64(wo)) + REFRACT_COND * refract_condition(model, n, wi, wo) ** 2 + fresnel_condition(model, n, wi, wo)
    bad_f = ~_close(fi, fm, _peak(fm), rt_f)
    fin_i, fin_m = np.isfinite(fi).all(1), np.isfinite(fm).all(1)
    bad_f |= fin_i != fin_m
    bad_f &= ~f_ex & ~nf_f
    # sample: flags equal, wo / f / pdf within the tolerance
    ggx = np.array([l.type == abi.LOBE_MICROFACET for l in model.lobes])
    chosen = model.pick(f64(n), f64(wi), np.asarray(u2, np.float32)[:, 0])[0]
    rt_s = np.where((chosen >= 0) & ggx[np.maximum(chosen, 0)] if len(ggx) else False, RTOL_GGX_SAMPLE, RTOL) + _cos_terms(f64(n), f64(wi))
    rt_s = rt_s + REFRACT_COND * refract_condition(model, n, wi, sm[0].astype(np.float32)) ** 2 + azimuth_condition(model, n, wi, chosen) \
        + fresnel_condition(model, n, wi, sm[0].astype(np.float32))
    bad_s = si[3] != sm[3]
    bad_s |= (np.abs(np.asarray(si[0], np.float64) - sm[0]) > rt_s[:, None] + FLOOR).any(1)  # wo: unit vectors, an absolute bound
    for j in (1, 2):
        bad_s |= ~_close(si[j], sm[j], _peak(sm[j]), rt_s)
        bad_s |= np.isfinite(np.asarray(si[j]).reshape(len(n), -1)).all(1) != np.isfinite(np.asarray(sm[j]).reshape(len(n), -1)).all(1)
    bad_s &= ~s_ex & ~nf_s
    return {"rows": len(n), "f_excluded": {k: int(v.sum()) for k, v in fx.items()}, "s_excluded": {k: int(v.sum()) for k, v in sx.items()},
            "f_excluded_rows": int(f_ex.sum()), "s_excluded_rows": int(s_ex.sum()), "nonfinite_allowed": int((nf_f | nf_s).sum()),
            "bad_f": np.nonzero(bad_f)[0], "bad_s": np.nonzero(bad_s)[0]}
