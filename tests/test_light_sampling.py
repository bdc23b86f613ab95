"""Picking a mesh light's triangle by area (phx_options.light_sampling = PHX_LIGHTS_BY_AREA), the parts that need no GPU: the ABI, a numpy
fp32 restatement of the rule in include/phx_xpu.h (the light table, the CDF, the pick, triangle_t::sample; tests/test_gpu_light_sampling.py
holds the device to it bit for bit), and the quirk the option switches off, pinned on the CPU oracle: a lamp cut into strips of unequal
width is lit by the reference as if every strip emitted the same power (uniform_triangle_pick, SURVEY A-12)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from phosphorus_mk2_amd import abi, scenes
from test_analytic_direct_light import CAM_Y, FOV, H_LAMP, LE, RHO, SPP, W, corner

F = np.float32
EPS = F(np.finfo(np.float32).eps)
ONE_MINUS_EPS = F(1.0) - EPS


# ---- 1. ABI -------------------------------------------------------------------------------------------------------------------------------
def test_abi_light_sampling():
    from phosphorus_mk2_amd import xpu
    hdr = open(os.path.join(ROOT, "include", "phx_xpu.h")).read()
    declared = {n: int(v) for n, v in re.findall(r"\bPHX_LIGHTS_([A-Z_]+)\s*=\s*(\d+)", hdr)}
    assert declared == {"REFERENCE": abi.LIGHTS_REFERENCE, "BY_AREA": abi.LIGHTS_BY_AREA} == {"REFERENCE": 0, "BY_AREA": 1}
    # light_sampling sits where reserved[0] sat: behind bvh_builder, the 12th word, and the struct keeps its 16 words
    names = [n for n, _ in abi.Options._fields_]
    assert names[names.index("bvh_builder") + 1:] == ["light_sampling", "reserved"]
    assert abi.Options.light_sampling.offset == 44 == abi.Options.bvh_builder.offset + 4 and abi.Options.reserved.offset == 48
    assert C.sizeof(abi.Options) == 64 == xpu.load_library().phx_abi_sizeof(0)
    m = re.search(r"typedef struct phx_options \{(.*?)\} phx_options;", hdr, re.S)
    fields = re.findall(r"^\s*u?int32_t\s+(\w+)(?:\[(\d+)\])?;", m.group(1), re.M)
    assert fields[-3:] == [("bvh_builder", ""), ("light_sampling", ""), ("reserved", "4")] and sum(int(n or 1) for _, n in fields) == 16
    # zero-filled options are the reference's pick; the Python names map onto the enumerators
    assert abi.Options().light_sampling == abi.LIGHTS_REFERENCE == xpu.Options().pack().light_sampling
    assert xpu.Options(light_sampling="area").pack().light_sampling == abi.LIGHTS_BY_AREA
    assert xpu.Options(light_sampling=2).pack().light_sampling == 2  # an int passes through (the refusal test needs a bad one)
    with pytest.raises(KeyError):
        xpu.Options(light_sampling="power").pack()


# ---- 2. the rule, restated in numpy fp32 --------------------------------------------------------------------------------------------------
def _length(v):
    """Imath Vec3::length as csrc/phx_math.h states it (lengthTiny below 2 FLT_MIN), fp32"""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    l2 = (x * x + y * y) + z * z
    out = np.sqrt(l2)
    tiny = l2 < F(2.0) * F(np.finfo(np.float32).tiny)
    if tiny.any():
        a = np.abs(v[tiny]); m = a.max(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            a = a / m[:, None]
            t = m * np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
        out[tiny] = np.where(m == 0, F(0), t)
    return out.astype(F)


def tri_areas(abc):
    """triangle_t::area (mesh.cpp:293-300): 0.5 * |(b - a) x (c - a)|, fp32, no contraction.  abc (n, 3, 3) f32"""
    abc = np.asarray(abc, F)
    ab, ac = abc[:, 1] - abc[:, 0], abc[:, 2] - abc[:, 0]
    cr = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], -1)
    return F(0.5) * _length(cr)


class LightTable:
    """The scene's lights as the device builds them: every face set of an emitting material, in mesh x face-set order, its triangles in the
    set's face order; per light the fp32 running sum of the areas (the last is the light's area), the CDF acc_i / area and lpdf."""

    def __init__(self, scene):
        self.tris, self.acc, self.area = [], [], []
        for m in scene.meshes:
            for mat, faces in m.sets:
                if scene.materials[mat].is_emitter and len(faces):
                    abc = m.vertices[m.faces[faces]].astype(F)
                    a = tri_areas(abc)
                    acc = np.zeros(len(a), F); run = F(0)
                    for i, x in enumerate(a):
                        run = F(run + x); acc[i] = run
                    self.tris.append(abc); self.acc.append(acc); self.area.append(run)
        self.n = len(self.tris)
        self.cdf = [(acc / area).astype(F) for acc, area in zip(self.acc, self.area)]
        self.areas = [tri_areas(t) for t in self.tris]
        self.lpdf = [F(F(F(1.0) / a) / F(self.n)) for a in self.area]

    def equal_pairs_only(self):
        """every light is one triangle, or two of bit-equal fp32 area: the lights the two modes sample alike"""
        return all(len(a) == 1 or (len(a) == 2 and a[0].tobytes() == a[1].tobytes()) for a in self.areas)


def pick_reference(lu, num):
    """light.cpp:55-67: the triangle by index"""
    lu = np.asarray(lu, F); numf = F(num)
    ti = np.minimum(np.floor(lu * numf).astype(np.int64), num - 1)
    return ti.astype(np.uint32), np.minimum(lu * numf - ti.astype(F), ONE_MINUS_EPS).astype(F)


def pick_by_area(lu, cdf):
    """the smallest i with lu < cdf[i] (num - 1 if none), and the draw remapped into [cdf[i - 1], cdf[i])"""
    lu = np.asarray(lu, F); cdf = np.asarray(cdf, F)
    ti = np.minimum(np.searchsorted(cdf, lu, side="right"), len(cdf) - 1)  # side="right": the first entry GREATER than lu
    lo = np.where(ti > 0, cdf[np.maximum(ti, 1) - 1], F(0)).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = ((lu - lo) / (cdf[ti] - lo)).astype(F)
    return ti.astype(np.uint32), np.where(np.isnan(r), ONE_MINUS_EPS, np.minimum(r, ONE_MINUS_EPS)).astype(F)  # fminf(NaN, x) = x


def light_sample(table, u3, by_area):
    """phx_dev_light_sample restated: (pick, lu, lv) -> light, tri, (bu, bv), P, lpdf"""
    u3 = np.asarray(u3, F).reshape(-1, 3)
    pick, lu, lv = u3[:, 0], u3[:, 1], u3[:, 2]
    l = np.minimum(np.floor(pick * F(table.n)).astype(np.int64), table.n - 1)
    tri = np.zeros(len(u3), np.uint32); bary = np.zeros((len(u3), 2), F); P = np.zeros((len(u3), 3), F); pdf = np.zeros(len(u3), F)
    for k in range(table.n):
        sel = l == k
        if not sel.any():
            continue
        ti, rem = pick_by_area(lu[sel], table.cdf[k]) if by_area else pick_reference(lu[sel], len(table.tris[k]))
        x = np.sqrt(rem)
        bu, bv = (F(1) - x).astype(F), (lv[sel] * x).astype(F)  # triangle_t::sample, mesh.cpp:318-324
        t = table.tris[k][ti]
        w = ((F(1) - bu) - bv).astype(F)
        P[sel] = (bu[:, None] * t[:, 0] + bv[:, None] * t[:, 1]) + w[:, None] * t[:, 2]
        tri[sel] = ti; bary[sel] = np.stack([bu, bv], -1); pdf[sel] = table.lpdf[k]
    return {"light": l.astype(np.uint32), "tri": tri, "bary": bary, "P": P, "pdf": pdf}


def _ulp_neighbours(x):
    x = F(x)
    return [np.nextafter(x, F(-1)), x, np.nextafter(x, F(2))]


def edge_draws(cdf=()):
    """0, 1 - 2^-24, and every table entry with its two neighbours (inside [0, 1))"""
    v = [F(0), F(1) - F(2.0 ** -24)]
    for c in cdf:
        v += _ulp_neighbours(c)
    v = np.array(v, F)
    return v[(v >= 0) & (v < 1)]


def _cdf_of(areas):
    acc = np.zeros(len(areas), F); run = F(0)
    for i, a in enumerate(np.asarray(areas, F)):
        run = F(run + a); acc[i] = run
    return (acc / run).astype(F)


def test_one_triangle_and_equal_pairs_are_the_reference_pick():
    rng = np.random.default_rng(11)
    lu = np.concatenate([rng.integers(0, 1 << 24, 1 << 20).astype(F) * F(2.0 ** -24), edge_draws([0.5])])
    assert lu.min() == 0 and lu.max() < 1
    for areas in ([0.5], [0.3737], [1.37], [0.5, 0.5], [0.3737, 0.3737], [1.37, 1.37]):
        cdf = _cdf_of(areas)
        assert cdf.tolist() == ([1.0] if len(areas) == 1 else [0.5, 1.0])
        ta, ra = pick_by_area(lu, cdf)
        tr, rr = pick_reference(lu, len(areas))
        assert np.array_equal(ta, tr) and ra.tobytes() == rr.tobytes(), areas
    # ... and eight equal triangles are NOT: 3 a rounds
    t8, r8 = pick_by_area(lu, _cdf_of([0.3737] * 8))
    tr, rr = pick_reference(lu, 8)
    assert not (np.array_equal(t8, tr) and r8.tobytes() == rr.tobytes())


def test_a_zero_area_triangle_is_never_picked_and_the_table_is_monotone():
    rng = np.random.default_rng(12)
    for areas in ([0.25, 0.0, 0.625], [1e-3, 0.0, 1.0, 3e-2, 0.0], [0.7, 0.1, 0.0], 10.0 ** rng.uniform(-3, 0, 37)):
        cdf = _cdf_of(areas)
        assert (np.diff(cdf) >= 0).all() and cdf[-1] == 1.0 and cdf[0] >= 0
        lu = np.concatenate([rng.integers(0, 1 << 24, 1 << 16).astype(F) * F(2.0 ** -24), edge_draws(cdf)])
        ti, rem = pick_by_area(lu, cdf)
        zero = np.flatnonzero(np.asarray(areas, F) == 0)
        assert not np.isin(ti, zero).any(), areas
        assert (rem >= 0).all() and (rem <= ONE_MINUS_EPS).all()
        lo = np.where(ti > 0, cdf[np.maximum(ti, 1) - 1], F(0))
        assert ((lo <= lu) & (lu < cdf[ti])).all()  # the draw lies in its triangle's interval
        # by area: the share of draws a triangle gets is its share of the area
        uniform = (np.arange(1 << 16, dtype=np.float64) + 0.5) / (1 << 16)
        share = np.bincount(pick_by_area(uniform.astype(F), cdf)[0], minlength=len(cdf)) / len(uniform)
        assert np.abs(share - np.asarray(areas, np.float64) / np.sum(np.asarray(areas, np.float64))).max() < 1e-4


# ---- 3. the striped lamp: the quirk the option removes, pinned on the oracle -----------------------------------------------------------------
CUTS = (-0.5, 0.0, 0.25, 0.375, 0.5)  # strips of width 1/2, 1/4, 1/8, 1/8: dyadic coordinates, every fp32 area exact
LAMP_Z = (-0.375, 0.625)
STRIPS = [(CUTS[i], CUTS[i + 1], LAMP_Z[0], LAMP_Z[1]) for i in range(4)]
QUAD = (-0.75, -0.25, -0.875, -0.375)  # the second lamp of the two-lamp scene: a two-triangle quad in front of the striped one
LE2 = (0.5, 1.5, 4.0)


def G_rect(x, z, rect):
    """test_analytic_direct_light.G_closed for any rectangle (x0, x1, z0, z1) at height H_LAMP"""
    x0, x1, z0, z1 = rect
    return corner(x1 - x, z1 - z, H_LAMP) - corner(x0 - x, z1 - z, H_LAMP) - corner(x1 - x, z0 - z, H_LAMP) + corner(x0 - x, z0 - z, H_LAMP)


def rect_nodes(rect, n):
    """midpoint-rule nodes of a rectangle and the area each stands for"""
    x0, x1, z0, z1 = rect
    xs = x0 + (np.arange(n) + 0.5) * (x1 - x0) / n; zs = z0 + (np.arange(n) + 0.5) * (z1 - z0) / n
    X, Z = np.meshgrid(xs, zs)
    return X.ravel(), Z.ravel(), (x1 - x0) * (z1 - z0) / (n * n)


def G_quadrature(x, z, rect, n=400):
    X, Z, dA = rect_nodes(rect, n)
    d2 = (X - x) ** 2 + (Z - z) ** 2 + H_LAMP ** 2
    return float((H_LAMP * H_LAMP / (d2 * d2)).sum() * dA)  # cos cos / d^2 = h^2 / d^4


def _floor():
    S = scenes
    meshes = []
    for (xa, xb) in ((-2.0, 0.0), (0.0, 2.0)):      # the floor of test_analytic_direct_light.scene()
        for (za, zb) in ((0.0, -2.0), (2.0, 0.0)):
            meshes.append(S._quad((xa, 0.0, za), (xb, 0.0, za), (xb, 0.0, zb), (xa, 0.0, zb), 0))
    return meshes


def rects_mesh(rects, material, y=H_LAMP):
    """rectangles at height y facing down, two triangles each, ONE mesh and ONE face set: one light"""
    v, f = [], []
    for (x0, x1, z0, z1) in rects:
        b = len(v)
        v += [(x0, y, z1), (x0, y, z0), (x1, y, z0), (x1, y, z1)]  # n = -y, as the lamp of test_analytic_direct_light
        f += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    return scenes.MeshDesc(vertices=np.array(v, F), faces=np.array(f, np.uint32), sets=[(material, np.arange(len(f), dtype=np.uint32))])


def _camera():
    M = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, CAM_Y, 0, 1]], F)
    return scenes.CameraDesc(W, W, FOV, to_world=M)


def striped_scene():
    mats = [scenes.diffuse(RHO, RHO, RHO), scenes.emitter(*LE)]
    return scenes.SceneDesc(_floor() + [rects_mesh(STRIPS, 1)], mats, _camera(), name="striped_lamp")


def two_lamp_scene():
    mats = [scenes.diffuse(RHO, RHO, RHO), scenes.emitter(*LE), scenes.emitter(*LE2)]
    return scenes.SceneDesc(_floor() + [rects_mesh(STRIPS, 1), rects_mesh([QUAD], 2)], mats, _camera(), name="two_lamps")


def floor_points():
    """where the pixel centres see the floor (test_analytic_direct_light.expected_film's mapping)"""
    zoom = 1.12 * math.tan(FOV / 2)
    px = np.arange(W, dtype=np.float64)
    fx = (px / W - 0.5) * zoom
    fy = (0.5 - (-0.5 + px) / W + 0.5 / W) * zoom
    return CAM_Y * fx[None, :] * np.ones((W, 1)), -CAM_Y * fy[:, None] * np.ones((1, W))


def striped_G(biased):
    """sum over the strips of G_s (the true form), or of G_s (1/4) / (w_s / W): what a uniform pick of the strip delivers"""
    X, Z = floor_points()
    width = CUTS[-1] - CUTS[0]
    return sum(G_rect(X, Z, r) * ((0.25 / ((r[1] - r[0]) / width)) if biased else 1.0) for r in STRIPS)


def film_of(G, le=LE):
    return np.stack([RHO / math.pi * 4.0 * e * G for e in le], -1)


def ratio_stats(film, expected):
    ratio = film[..., :3].astype(np.float64) / expected
    return abs(ratio.mean() - 1.0), np.abs(ratio - 1.0).max(), ratio.std()


def meets(film, expected):
    """test_analytic_direct_light.check's three tolerances: film mean 3e-3, worst pixel 0.12, std of the pixel ratio 0.03"""
    mean, worst, std = ratio_stats(film, expected)
    print(f"mean off by {mean:.3g}, worst pixel {worst:.3g}, std {std:.3g}")
    return mean < 3e-3 and worst < 0.12 and std < 0.03


def test_each_strip_closed_form_is_the_integral():
    for r in STRIPS + [QUAD]:
        for (x, z) in ((0.0, 0.0), (0.3, -0.2), (-0.45, 0.4), (0.9, 0.9)):
            q = G_quadrature(x, z, r)
            assert abs(G_rect(x, z, r) - q) < 2e-5 * q + 1e-7
    X, Z = floor_points()
    assert np.allclose(striped_G(False), G_rect(X, Z, (CUTS[0], CUTS[-1], *LAMP_Z)), rtol=1e-12)  # the strips tile the lamp


def test_the_striped_lamp_has_unequal_exact_areas():
    t = LightTable(striped_scene())
    assert t.n == 1 and t.areas[0].tolist() == [0.25, 0.25, 0.125, 0.125, 0.0625, 0.0625, 0.0625, 0.0625] and t.area[0] == 1.0
    assert t.cdf[0].tolist() == [0.25, 0.5, 0.625, 0.75, 0.8125, 0.875, 0.9375, 1.0] and not t.equal_pairs_only()
    assert LightTable(two_lamp_scene()).n == 2


@pytest.fixture(scope="module")
def striped_oracle_film(orc):
    return orc.Oracle(striped_scene(), spp=SPP, pps=1, depth=1).render(rng=orc.RNG_COUNTER, seed=3, threads=4)


def test_oracle_lights_the_striped_lamp_by_strip_count_not_by_area(striped_oracle_film):
    """the reference's pick (what PHX_LIGHTS_REFERENCE reproduces): every strip gets a quarter of the samples whatever its width.
    Measured: against the biased form mean 1.6e-4, worst pixel 0.080, std 0.021; against the true form the mean is off by 2.3 %."""
    film, st = striped_oracle_film
    assert st["rays_shadow"] == st["rays_closest"] == W * W * SPP
    assert meets(film, film_of(striped_G(True)))
    mean, worst, std = ratio_stats(film, film_of(striped_G(False)))
    assert mean > 0.015 and not meets(film, film_of(striped_G(False))), (mean, worst, std)


# ---- the standard-error model of the two-lamp test (tests/test_gpu_light_sampling.py) -----------------------------------------------------
TWO_LAMPS = [(STRIPS, LE), ([QUAD], LE2)]


def moments(lamps, n=64):
    """Per pixel centre x and channel c, in float64 from the closed-form integrand g = cos cos / d^2 = h^2 / d^4 alone: the mean of one
    sample, sum_l c_l G_l(x) (closed form), and its second moment sum_l (1/nl) int (nl A_l c_l g)^2 dA / A_l = sum_l nl A_l c_l^2 int g^2 dA
    (midpoint rule, n x n nodes per rectangle), c_l = (rho / pi) 4 L_e.  One sample picks a lamp with probability 1/nl and a point
    uniformly on its area; lamps = [(rectangles, L_e)]."""
    X, Z = floor_points()
    nl = len(lamps)
    mean = np.zeros(X.shape + (3,)); m2 = np.zeros(X.shape + (3,))
    for rects, le in lamps:
        A = sum((r[1] - r[0]) * (r[3] - r[2]) for r in rects)
        G = sum(G_rect(X, Z, r) for r in rects)
        g2 = np.zeros(X.shape)
        for r in rects:
            xs, zs, dA = rect_nodes(r, n)
            d2 = (xs[None, None, :] - X[..., None]) ** 2 + (zs[None, None, :] - Z[..., None]) ** 2 + H_LAMP ** 2
            g2 += ((H_LAMP * H_LAMP / (d2 * d2)) ** 2).sum(-1) * dA
        for c in range(3):
            k = RHO / math.pi * 4.0 * le[c]
            mean[..., c] += k * G
            m2[..., c] += nl * A * k * k * g2
    return mean, m2


def z_scores(film, mean, m2, spp):
    """(film mean's distance from the model's in its standard errors per channel, every pixel's in its own)"""
    var = m2 - mean * mean
    assert (var > 0).all()
    got = film[..., :3].astype(np.float64)
    se_mean = np.sqrt(var.sum((0, 1)) / spp) / (mean.shape[0] * mean.shape[1])
    return np.abs(got.mean((0, 1)) - mean.mean((0, 1))) / se_mean, np.abs(got - mean) / np.sqrt(var / spp)


def test_the_standard_error_model_holds_where_the_reference_pick_is_unbiased(orc):
    """two lamps of two equal triangles each (the whole lamp uncut, and the quad): the reference's pick IS by area there, so the oracle must
    sit inside 4 standard errors of the film mean and 5 of a pixel, and its z scores must have unit spread -- the bounds the device's
    BY_AREA film of the striped pair is held to"""
    whole = (CUTS[0], CUTS[-1], *LAMP_Z)
    mats = [scenes.diffuse(RHO, RHO, RHO), scenes.emitter(*LE), scenes.emitter(*LE2)]
    sc = scenes.SceneDesc(_floor() + [rects_mesh([whole], 1), rects_mesh([QUAD], 2)], mats, _camera(), name="two_plain_lamps")
    assert LightTable(sc).equal_pairs_only()
    film, st = orc.Oracle(sc, spp=SPP, pps=1, depth=1).render(rng=orc.RNG_COUNTER, seed=3, threads=4)
    assert st["rays_shadow"] == st["rays_closest"] == W * W * SPP
    mean, m2 = moments([([whole], LE), ([QUAD], LE2)])
    assert np.allclose(mean, moments(TWO_LAMPS, n=8)[0], rtol=1e-12)  # the strips tile the lamp: the striped pair has the same mean
    z_mean, z_pixel = z_scores(film, mean, m2, SPP)
    print(f"film mean off by {z_mean} standard errors, worst pixel {z_pixel.max():.2f}, rms {np.sqrt((z_pixel ** 2).mean()):.3f}")
    assert (z_mean < 4.0).all() and z_pixel.max() < 5.0
    assert 0.9 < np.sqrt((z_pixel ** 2).mean()) < 1.1  # the model's variance is the film's (1024 pixels: the rms of unit normals is 1 +- 0.022)
