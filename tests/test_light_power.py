"""Choosing next-event estimation's light by power (phx_options.light_sampling = PHX_LIGHTS_BY_AREA | PHX_LIGHT_SELECT_BY_POWER), the parts that
need no GPU: the ABI and the Python keyword, a numpy restatement of the rule in include/phx_xpu.h (binary64 where the rule says so, sequential
sums by np.cumsum, fp32 elsewhere; tests/test_gpu_light_power.py holds the device to it bit for bit), the properties the rule promises,
flatten_scene against the restatement through tests/native/host_flatten_power.cpp, and the variance model of the seven-lamp film."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import native_lib as NL
from phosphorus_mk2_amd import abi, scenes
from test_analytic_direct_light import H_LAMP, LE, RHO, SPP
from test_emission_textures import light_corner_uvs, sample_st
from test_gpu_textures import np_lookup
from test_light_sampling import (LE2, STRIPS, G_rect, LightTable, _camera, _floor, edge_draws, floor_points, moments, pick_by_area, rect_nodes, rects_mesh,
                                 striped_scene, two_lamp_scene)
from test_scene_flatten import ARRAYS, SC_LIGHTS_BY_AREA, WORDS

F = np.float32
D = np.float64
PHI = 0.125  # PHX_LIGHT_POWER_FLOOR
SC_LIGHTS_BY_POWER = 16  # kernels.h: DevScene::any_tex
AREA_POWER = abi.LIGHTS_BY_AREA | 0x100


# ---- (a) ABI and Python ---------------------------------------------------------------------------------------------------------------------
def test_abi_light_selection():
    from phosphorus_mk2_amd import xpu
    hdr = NL.header()
    m = re.search(r"\bPHX_LIGHT_SELECT_BY_POWER\s*=\s*(0x[0-9a-fA-F]+|\d+)", hdr)
    assert m and int(m.group(1), 0) == abi.LIGHT_SELECT_BY_POWER == 0x100
    assert float(re.search(r"#define\s+PHX_LIGHT_POWER_FLOOR\s+([0-9.]+)", hdr).group(1)) == PHI
    assert "PHX_LIGHT_SAMPLING_MODE(x)" in hdr and "PHX_LIGHT_SELECTION(x)" in hdr
    assert xpu.Options(light_sampling="area", light_selection="power").pack().light_sampling == 0x101 == AREA_POWER
    assert xpu.Options(light_sampling=1, light_selection="power").pack().light_sampling == 0x101
    assert xpu.Options(light_sampling="area", light_selection="uniform").pack().light_sampling == abi.LIGHTS_BY_AREA
    assert xpu.Options().pack().light_sampling == 0  # zero-filled options: as before
    for ls in ("reference", 0, 2, 0x101):
        with pytest.raises(ValueError):
            xpu.Options(light_sampling=ls, light_selection="power").pack()
    with pytest.raises(KeyError):
        xpu.Options(light_sampling="power").pack()  # the triangle pick's keyword keeps its names
    with pytest.raises(KeyError):
        xpu.Options(light_sampling="area", light_selection="area").pack()
    assert xpu.Options(light_sampling=0x201).pack().light_sampling == 0x201  # ints still pass through (the refusal test needs bad ones)
    assert C.sizeof(abi.Options) == 64


# ---- (b) the rule, restated -----------------------------------------------------------------------------------------------------------------
def image_mean(texels):
    """per-channel mean of |texel| over all texels: summed sequentially in row-major order in binary64, divided by W * H"""
    t = np.abs(np.asarray(texels, F).astype(D)).reshape(-1, 3)
    return np.cumsum(t, axis=0)[-1] / D(len(t))


class PowerTable(LightTable):
    """LightTable plus the selection by power: w, q (binary64), pcdf, p (fp32) and lpdf = (1 / area) * p per light; fallback: the uniform table"""

    def __init__(self, scene):
        with np.errstate(invalid="ignore", divide="ignore"):  # a lamp of zero area: its CDF is 0 / 0 and 1 / area is inf; it is never chosen
            super().__init__(scene)
        mats = light_corner_uvs(scene)[1]
        self.materials = mats
        w = np.zeros(self.n, D)
        with np.errstate(invalid="ignore", over="ignore"):
            for k, mat in enumerate(mats):
                m = scene.materials[mat]
                mean = image_mean(scene.textures[m.emission_uv_texture - 1].texels) if m.emission_uv_texture else np.ones(3, D)
                e = np.abs(np.array([F(x) for x in m.emission], F).astype(D))
                w[k] = D(self.area[k]) * ((D(0.2126) * e[0] * mean[0] + D(0.7152) * e[1] * mean[1]) + D(0.0722) * e[2] * mean[2])
        self.w = w
        npos = int((w > 0).sum())
        self.fallback = not np.isfinite(w).all() or npos == 0
        if self.fallback:
            q = np.full(self.n, D(1.0) / D(self.n))
        else:
            wsum = np.cumsum(w)[-1]
            q = np.where(w > 0, (D(1.0) - D(PHI)) * w / wsum + D(PHI) / D(npos), D(0.0))
        self.q = q
        acc = np.cumsum(q)
        self.pcdf = (acc / acc[-1]).astype(F)
        lo = np.concatenate([[F(0)], self.pcdf[:-1]]).astype(F)
        self.p = (self.pcdf - lo).astype(F)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.lpdf = [F(F(F(1.0) / a) * p) for a, p in zip(self.area, self.p)]


def select(pcdf, pick):
    """the smallest l with pick < pcdf[l], or n - 1 when there is none"""
    return np.minimum(np.searchsorted(np.asarray(pcdf, F), np.asarray(pick, F), side="right"), len(pcdf) - 1)


def light_sample_power(table, u3):
    """phx_dev_light_sample under (area, power) restated: test_light_sampling.light_sample with the light from the table"""
    u3 = np.asarray(u3, F).reshape(-1, 3)
    pick, lu, lv = u3[:, 0], u3[:, 1], u3[:, 2]
    l = select(table.pcdf, pick)
    tri = np.zeros(len(u3), np.uint32); bary = np.zeros((len(u3), 2), F); P = np.zeros((len(u3), 3), F); pdf = np.zeros(len(u3), F)
    for k in range(table.n):
        sel = l == k
        if not sel.any():
            continue
        ti, rem = pick_by_area(lu[sel], table.cdf[k])
        x = np.sqrt(rem)
        bu, bv = (F(1) - x).astype(F), (lv[sel] * x).astype(F)
        t = table.tris[k][ti]
        w = ((F(1) - bu) - bv).astype(F)
        P[sel] = (bu[:, None] * t[:, 0] + bv[:, None] * t[:, 1]) + w[:, None] * t[:, 2]
        tri[sel] = ti; bary[sel] = np.stack([bu, bv], -1); pdf[sel] = table.lpdf[k]
    return {"light": l.astype(np.uint32), "tri": tri, "bary": bary, "P": P, "pdf": pdf}


def light_emission_power(scene, u3):
    """phx_dev_light_emission behind the new pick: test_emission_textures.light_emission with the light from the table"""
    t = PowerTable(scene)
    s = light_sample_power(t, u3)
    uvs, mats = light_corner_uvs(scene)
    st = np.zeros((len(s["light"]), 2), F); e = np.zeros((len(s["light"]), 3), F)
    for k in range(t.n):
        sel = s["light"] == k
        m = scene.materials[mats[k]]
        em = np.array([F(x) for x in m.emission], F)
        if not m.emission_uv_texture:
            e[sel] = em
            continue
        st[sel] = sample_st(uvs[k][s["tri"][sel]], s["bary"][sel])
        e[sel] = em[None, :] * np_lookup(scene.textures[m.emission_uv_texture - 1], st[sel])
    return {"st": st, "e": e}


def pick_edges(pcdf):
    """0, 1 - 2^-24 and every table entry with both ulp neighbours (inside [0, 1))"""
    return edge_draws(pcdf)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------------
SMALL = [(-1.25, -1.0, -1.0, -0.75), (-1.25, -1.0, 0.75, 1.0), (1.0, 1.25, -1.0, -0.75), (1.0, 1.25, 0.75, 1.0), (-0.125, 0.125, -1.25, -1.0),
         (-0.125, 0.125, 1.0, 1.25)]
SEVEN_LAMPS = [(STRIPS, LE)] + [([r], LE2) for r in SMALL]
BELOW = (-0.5, 0.5, -0.5, 0.5)  # the black quad of the GPU test, at y = -1: under the floor, where no ray goes


def lamps_scene(lamps, name="lamps", textures=()):
    """the floor and camera of test_light_sampling under lamps = [(rectangles, emission[, image + 1[, y]])], one light each, in this order"""
    mats = [scenes.diffuse(RHO, RHO, RHO)]
    meshes = _floor()
    for spec in lamps:
        rects, le = spec[0], spec[1]
        tex = spec[2] if len(spec) > 2 else 0
        y = spec[3] if len(spec) > 3 else H_LAMP
        mats.append(scenes.MaterialDesc([], tuple(le), True, emission_uv_texture=tex))
        meshes.append(rects_mesh(rects, len(mats) - 1, y))
    return scenes.SceneDesc(meshes, mats, _camera(), name=name, textures=list(textures))


def seven_lamp_scene(black=None):
    """lamp A = the striped lamp (eight unequal triangles), six LE2 quads of side 1/4 around it; black: "first" / "last" adds a black emitter
    quad under the floor at that end of the light order"""
    lamps = list(SEVEN_LAMPS)
    dark = ([BELOW], (0.0, 0.0, 0.0), 0, -1.0)
    if black == "first":
        lamps.insert(0, dark)
    elif black == "last":
        lamps.append(dark)
    return lamps_scene(lamps, "seven_lamps" + (f"_black_{black}" if black else ""))


DECADES = [([(-0.9, -0.4, -0.2, 0.3)], (0.03, 0.02, 0.05)), ([(-0.2, 0.3, -0.9, -0.4)], (0.5, 0.3, 0.2)), ([(0.3, 0.9, 0.1, 0.7)], (20.0, 30.0, 10.0))]
BLACK = ([(0.4, 0.8, -0.8, -0.4)], (0.0, 0.0, 0.0))
ZERO_AREA = ([(0.5, 0.5, -0.8, -0.4)], (5.0, 5.0, 5.0))  # x0 == x1: two triangles of zero area
ZERO_IMAGE = scenes.TextureDesc(np.zeros((2, 3, 3), F))
IMG = scenes.TextureDesc(np.random.default_rng(17).uniform(0.0, 2.0, (3, 5, 3)).astype(F) * np.array([1.0, -1.0, 1.0], F))  # a negative channel: |texel|


def _with(pos, extra):
    lamps = list(DECADES); lamps.insert(pos, extra)
    return lamps


RULE_SCENES = {
    "decades": lambda: lamps_scene(DECADES, "decades"),
    "black_first": lambda: lamps_scene(_with(0, BLACK), "black_first"),
    "black_middle": lambda: lamps_scene(_with(1, BLACK), "black_middle"),
    "black_last": lambda: lamps_scene(_with(3, BLACK), "black_last"),
    "zero_area": lambda: lamps_scene(_with(1, ZERO_AREA), "zero_area"),
    "zero_image": lambda: lamps_scene([DECADES[0], (DECADES[1][0], (4.0, 4.0, 4.0), 1), DECADES[2], (BLACK[0], (1.0, 2.0, 3.0), 2)], "zero_image", [ZERO_IMAGE, IMG]),
    "one_light": striped_scene,
    "two_lamps": two_lamp_scene,
    "seven_lamps": seven_lamp_scene,
    "seven_lamps_black_first": lambda: seven_lamp_scene("first"),
    "seven_lamps_black_last": lambda: seven_lamp_scene("last"),
    "all_black": lambda: lamps_scene([(r, (0.0, 0.0, 0.0)) for r, _ in DECADES], "all_black"),
    "nan_emission": lambda: lamps_scene([DECADES[0], (DECADES[1][0], (float("nan"), 1.0, 1.0)), DECADES[2]], "nan_emission"),
    "inf_emission": lambda: lamps_scene([DECADES[0], (DECADES[1][0], (1.0, float("inf"), 1.0)), DECADES[2]], "inf_emission"),
}
DEAD = {"black_first": [0], "black_middle": [1], "black_last": [3], "zero_area": [1], "zero_image": [1], "seven_lamps_black_first": [0],
        "seven_lamps_black_last": [7]}  # the lights that must never be chosen


# ---- (c) properties of the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RULE_SCENES))
def test_the_table_is_monotone_ends_at_one_and_never_returns_a_dead_lamp(name):
    t = PowerTable(RULE_SCENES[name]())
    assert t.pcdf.dtype == F and t.pcdf[-1] == F(1.0) and (np.diff(t.pcdf) >= 0).all() and t.pcdf[0] >= 0
    assert abs(t.p.astype(D).sum() - 1.0) <= t.n * 2.0 ** -24  # sum of p_l = 1 to within nlights ulp
    rng = np.random.default_rng(5)
    pick = np.concatenate([pick_edges(t.pcdf), rng.integers(0, 1 << 24, 1 << 16).astype(F) * F(2.0 ** -24)])
    assert pick.min() == 0 and pick.max() == F(1) - F(2.0 ** -24)
    l = select(t.pcdf, pick)
    lo = np.where(l > 0, t.pcdf[np.maximum(l, 1) - 1], F(0))
    assert ((lo <= pick) & (pick < t.pcdf[l])).all()  # the draw lies in its light's interval
    dead = DEAD.get(name, [])
    assert not t.fallback or name in ("all_black", "nan_emission", "inf_emission")
    for k in dead:
        assert t.w[k] == 0 and t.q[k] == 0 and t.p[k] == 0 and not (l == k).any(), (name, k)
    alive = [k for k in range(t.n) if k not in dead]
    assert set(np.unique(l)) == set(alive)
    if not t.fallback:  # the floor: every lamp that emits keeps q >= 1 / (8 n+), and q sums to one
        assert (t.q[alive] >= PHI / len(alive)).all() and abs(t.q.sum() - 1.0) < 1e-15 * t.n
        share = np.bincount(select(t.pcdf, ((np.arange(1 << 16) + 0.5) / (1 << 16)).astype(F)), minlength=t.n) / (1 << 16)
        assert np.abs(share - t.q).max() < 1e-4  # the share of draws a light gets is its q


def test_one_light_gives_the_table_of_one_and_by_areas_lpdf():
    t = PowerTable(striped_scene())
    assert t.n == 1 and t.pcdf.tolist() == [1.0] and t.p.tolist() == [1.0]
    assert t.lpdf[0].tobytes() == LightTable(striped_scene()).lpdf[0].tobytes() == F(1.0).tobytes()  # (1 / area) * 1 == (1 / area) / 1
    assert not select(t.pcdf, pick_edges(t.pcdf)).any()


@pytest.mark.parametrize("name", ["all_black", "nan_emission", "inf_emission"])
def test_black_and_broken_scenes_fall_back_to_the_uniform_table(name):
    t = PowerTable(RULE_SCENES[name]())
    assert t.fallback and t.n == 3
    acc = np.cumsum(np.full(3, D(1.0) / D(3.0)))
    assert t.pcdf.tobytes() == (acc / acc[-1]).astype(F).tobytes() and t.pcdf[-1] == 1.0
    assert np.abs(t.p.astype(D) - 1.0 / 3.0).max() < 2.0 ** -24


def test_the_image_mean_is_over_absolute_texels_of_the_whole_image():
    t = PowerTable(RULE_SCENES["zero_image"]())
    m = image_mean(IMG.texels)
    assert (m > 0).all() and np.allclose(m, np.abs(IMG.texels.astype(D)).mean((0, 1)), rtol=1e-14) and IMG.texels[..., 1].max() <= 0
    assert t.w[3] == D(t.area[3]) * ((0.2126 * 1.0 * m[0] + 0.7152 * 2.0 * m[1]) + 0.0722 * 3.0 * m[2]) and t.w[1] == 0


def test_seven_lamp_probabilities():
    t = PowerTable(seven_lamp_scene())
    assert t.n == 7 and len(t.areas[0]) == 8 and all(len(a) == 2 for a in t.areas[1:]) and t.area[0] == 1.0 and all(a == 0.0625 for a in t.area[1:])
    assert abs(t.q[0] - 0.714) < 5e-4 and (np.abs(t.q[1:] - 0.0477) < 5e-5).all()
    assert np.abs(t.p.astype(D) - t.q).max() < 2.0 ** -23
    # a black lamp at either end moves no entry of the table of the seven
    for black, sl in (("first", slice(1, 8)), ("last", slice(0, 7))):
        tb = PowerTable(seven_lamp_scene(black))
        assert tb.n == 8 and tb.pcdf[sl].tobytes() == t.pcdf.tobytes() and tb.p[sl].tobytes() == t.p.tobytes()
        assert b"".join(x.tobytes() for x in tb.lpdf[sl]) == b"".join(x.tobytes() for x in t.lpdf)


def test_lamp_showroom_is_one_lamp_and_sixty_four_leds():
    """scenes.lamp_showroom (scripts/light_selection_payoff.py): 65 lights; the LEDs share the floor, the ceiling lamp takes the rest"""
    sc = scenes.lamp_showroom(2000, width=64, height=36)
    t = PowerTable(sc)
    assert t.n == 65 and t.equal_pairs_only() and not t.fallback and sc.num_triangles == scenes.bmw_showroom(2000, 64, 36).num_triangles + 128
    assert t.q[0] > 0.87 and (t.q[1:] < 0.0021).all() and (t.q[1:] >= PHI / 65).all() and np.ptp(t.q[1:]) < 1e-6
    assert (t.p > 0).all() and set(np.unique(select(t.pcdf, pick_edges(t.pcdf)))) == set(range(65))


# ---- (d) flatten_scene ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat_power():
    """the host_flatten_power library: test_scene_flatten's flatten() plus the selection table ("light_pcdf")"""
    lib = NL.load("host_flatten_power")
    lib.hf_flatten.restype = C.c_void_p; lib.hf_flatten.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Options)]
    lib.hf_free.argtypes = [C.c_void_p]
    lib.hf_status.argtypes = [C.c_void_p]
    lib.hf_error.restype = C.c_char_p; lib.hf_error.argtypes = [C.c_void_p]
    lib.hf_array.restype = C.c_void_p; lib.hf_array.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    lib.hf_power_table.restype = C.c_void_p; lib.hf_power_table.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.hf_word.restype = C.c_uint32; lib.hf_word.argtypes = [C.c_void_p, C.c_int]

    def flatten(scene, light_sampling):
        s, keep = scene.pack()
        opt = abi.Options(); opt.light_sampling = light_sampling; opt.path_depth = 9
        h = lib.hf_flatten(C.byref(s), C.byref(opt))
        try:
            out = {"status": lib.hf_status(h), "error": lib.hf_error(h).decode()}
            if out["status"] == 0:
                n = C.c_uint64(0)
                for name, (which, dtype) in ARRAYS.items():
                    p = lib.hf_array(h, which, C.byref(n))
                    out[name] = np.frombuffer(C.string_at(p, n.value) if n.value else b"", dtype).copy()
                p = lib.hf_power_table(h, C.byref(n))
                out["light_pcdf"] = np.frombuffer(C.string_at(p, n.value) if n.value else b"", F).copy()
                for name, which in WORDS.items():
                    out[name] = lib.hf_word(h, which)
            return out
        finally:
            lib.hf_free(h)
    return flatten


@pytest.mark.parametrize("name", list(RULE_SCENES))
def test_flatten_scene_builds_the_restatements_table(flat_power, name):
    sc = RULE_SCENES[name]()
    t = PowerTable(sc)
    r = flat_power(sc, AREA_POWER)
    assert r["status"] == 0, r["error"]
    assert r["num_lights"] == t.n and r["light_pcdf"].tobytes() == t.pcdf.tobytes()
    assert r["lights"]["lpdf"].tobytes() == np.array(t.lpdf, F).tobytes()
    assert r["lights"]["area"].tobytes() == np.array(t.area, F).tobytes()
    tex = 1 if sc.textures else 0
    assert r["any_tex"] == (SC_LIGHTS_BY_AREA | SC_LIGHTS_BY_POWER | tex) and r["diffuse_only"] == 0
    # with the bit clear nothing changes: no table, LightTable's lpdf = (1 / area) / n, and every other array is the one the bit's scene has too
    base = LightTable(sc)
    for word in (abi.LIGHTS_REFERENCE, abi.LIGHTS_BY_AREA):
        r0 = flat_power(sc, word)
        assert r0["status"] == 0 and len(r0["light_pcdf"]) == 0
        assert r0["any_tex"] == ((SC_LIGHTS_BY_AREA if word else 0) | tex) and r0["diffuse_only"] == (0 if word or tex else 2)
        assert r0["lights"]["lpdf"].tobytes() == np.array(base.lpdf, F).tobytes()
        assert len(r0["light_cdf"]) == (sum(len(c) for c in base.cdf) if word else 0)
    lights = r["lights"].copy(); lights["lpdf"] = r0["lights"]["lpdf"]
    assert lights.tobytes() == r0["lights"].tobytes()
    for key in ARRAYS:
        if key not in ("lights", "mat_lite"):
            assert r[key].tobytes() == r0[key].tobytes(), key
    assert r["light_cdf"].tobytes() == np.concatenate(base.cdf).astype(F).tobytes()


@pytest.mark.parametrize("word", [0x100, 0x201, 0x10101, 2 | 0x100, 2, 0x200, 0x80000001])
def test_flatten_scene_refuses_every_other_word(flat_power, word):
    r = flat_power(seven_lamp_scene(), word)
    assert r["status"] == 1 and "light_sampling" in r["error"]
    if (word & 0xff) == 2:
        assert "unknown light_sampling" in r["error"]


# ---- (e) the variance model -----------------------------------------------------------------------------------------------------------------
def moments_p(lamps, p, n=64):
    """test_light_sampling.moments with per-light selection probabilities p: one sample picks lamp l with probability p_l and a point
    uniformly on its area, so its mean is sum_l c_l G_l(x) whatever p, and its second moment sum_l p_l int (A_l c_l g / p_l)^2 dA / A_l =
    sum_l (1 / p_l) A_l c_l^2 int g^2 dA, with g = cos cos / d^2 = h^2 / d^4 and c_l = (rho / pi) 4 L_e.  float64; no render enters it."""
    X, Z = floor_points()
    mean = np.zeros(X.shape + (3,)); m2 = np.zeros(X.shape + (3,))
    for (rects, le), pl in zip(lamps, p):
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
            m2[..., c] += (1.0 / float(pl)) * A * k * k * g2
    return mean, m2


@pytest.fixture(scope="module")
def seven_lamp_moments():
    t = PowerTable(seven_lamp_scene())
    mean, m2_power = moments_p(SEVEN_LAMPS, t.p.astype(D))
    _, m2_uniform = moments_p(SEVEN_LAMPS, np.full(7, 1.0 / 7.0))
    return mean, m2_power, m2_uniform


def test_the_generalised_model_is_the_uniform_model_at_equal_probabilities():
    from test_light_sampling import TWO_LAMPS
    mean, m2 = moments(TWO_LAMPS, n=16)
    mean_p, m2_p = moments_p(TWO_LAMPS, [0.5, 0.5], n=16)
    assert np.allclose(mean, mean_p, rtol=1e-14) and np.allclose(m2, m2_p, rtol=1e-14)


def test_power_selection_cuts_the_seven_lamp_films_variance(seven_lamp_moments):
    """a condition on the scene, from the model alone: under uniform selection the film-summed variance is at least 10 x the power table's in
    every channel (computed: 12.9 / 15.3 / 17.7), and the rms over pixels of the standard-deviation ratio at least 3 (computed: 4.07)"""
    mean, m2_power, m2_uniform = seven_lamp_moments
    var_p, var_u = m2_power - mean * mean, m2_uniform - mean * mean
    assert (var_p > 0).all() and (var_u > 0).all()
    ratio = var_u.sum((0, 1)) / var_p.sum((0, 1))
    rms = math.sqrt((var_u / var_p).mean())
    print(f"film-summed variance, uniform over power: {ratio}; rms of the pixels' sd ratio {rms:.3f}; spp {SPP}")
    assert (ratio >= 10.0).all()
    assert rms >= 3.0
