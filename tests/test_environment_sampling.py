"""Sampling the environment image by next-event estimation (phx_options.light_sampling = 0x301: PHX_LIGHTS_BY_AREA | PHX_LIGHT_SELECT_BY_POWER |
PHX_LIGHT_INCLUDE_ENVIRONMENT), the parts that need no GPU: the ABI and the Python keyword, a numpy restatement of the rule in include/phx_xpu.h
(binary64 where the rule says so, sequential sums by np.cumsum, fp32 elsewhere; tests/test_gpu_environment_sampling.py holds the device to it),
the properties the rule promises, and flatten_scene against the restatement through tests/native/host_flatten_env.cpp."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import native_lib as NL
from phosphorus_mk2_amd import abi, scenes
from test_light_power import DECADES, PHI, SC_LIGHTS_BY_POWER, PowerTable, lamps_scene, select
from test_scene_flatten import ARRAYS, SC_LIGHTS_BY_AREA, SC_TEX_ENV, WORDS

F = np.float32
D = np.float64
SC_LIGHTS_ENV = 32  # kernels.h: DevScene::any_tex
AREA_POWER = 0x101
AREA_POWER_ENV = 0x301
ONE_MINUS_EPS = F(1) - F(2.0 ** -23)  # 1 - FLT_EPSILON


# ---- (a) ABI and Python ---------------------------------------------------------------------------------------------------------------------
def test_abi_environment_sampling():
    from phosphorus_mk2_amd import xpu
    hdr = NL.header()
    m = re.search(r"\bPHX_LIGHT_INCLUDE_ENVIRONMENT\s*=\s*(0x[0-9a-fA-F]+|\d+)", hdr)
    assert m and int(m.group(1), 0) == abi.LIGHT_INCLUDE_ENVIRONMENT == 0x200
    assert re.search(r"#define\s+PHX_LIGHT_ENVIRONMENT\(x\)\s+\(\(x\)\s*&\s*0x200u\)", hdr)
    assert re.search(r"#define\s+PHX_LIGHT_SELECTION\(x\)\s+\(\(x\)\s*&\s*~0xffu\)", hdr)  # means what it meant
    assert "phx_dev_environment_sample" in hdr and "phx_dev_environment_sample" in abi.EXPORTS
    o = xpu.Options(light_sampling="area", light_selection="power", environment_sampling=True)
    assert o.pack().light_sampling == AREA_POWER_ENV == abi.LIGHTS_BY_AREA | abi.LIGHT_SELECT_BY_POWER | abi.LIGHT_INCLUDE_ENVIRONMENT
    assert xpu.Options(light_sampling="area", light_selection="power").pack().light_sampling == AREA_POWER
    assert xpu.Options().pack().light_sampling == 0 and xpu.Options().environment_sampling is False
    for kw in ({}, {"light_sampling": "area"}, {"light_sampling": 1}, {"light_sampling": 0x200}):
        with pytest.raises(ValueError, match="environment_sampling"):
            xpu.Options(environment_sampling=True, **kw).pack()
    with pytest.raises(ValueError):  # "power" without "area" is refused first, as before
        xpu.Options(light_selection="power", environment_sampling=True).pack()
    assert "environment_sampling" in xpu.render.__code__.co_varnames
    assert C.sizeof(abi.Options) == 64


# ---- (b) the rule, restated -----------------------------------------------------------------------------------------------------------------
def _wrap(i, n, mode):
    """bsdf.h: tex_wrap -> (index, outside)"""
    if mode == abi.WRAP_PERIODIC:
        return i % n, np.zeros(i.shape, bool)
    if mode == abi.WRAP_CLAMP:
        return np.clip(i, 0, n - 1), np.zeros(i.shape, bool)
    return np.clip(i, 0, n - 1), (i < 0) | (i > n - 1)


def importance(tex, emission):
    """g (H, W) and the sines of the rows, binary64: y = Y(|e| * |texel|), the 3 x 3 maximum under LINEAR, times sin((pi (j + 0.5)) / H)"""
    img = np.abs(np.asarray(tex.texels, F).astype(D))
    H, W = img.shape[:2]
    e = np.abs(np.array([F(x) for x in emission], F).astype(D))
    with np.errstate(invalid="ignore", over="ignore"):
        y = (D(0.2126) * (e[0] * img[..., 0]) + D(0.7152) * (e[1] * img[..., 1])) + D(0.0722) * (e[2] * img[..., 2])
        m = y.copy()
        if tex.filter == abi.TEX_LINEAR:
            jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            for dj in (-1, 0, 1):
                for di in (-1, 0, 1):
                    x, ox = _wrap(ii + di, W, tex.swrap)
                    yy, oy = _wrap(jj + dj, H, tex.twrap)
                    n = np.where(ox | oy, D(0.0), y[yy, x])
                    m = np.where(n > m, n, m)
        sin_j = np.array([math.sin((math.pi * (j + 0.5)) / H) for j in range(H)], D)
        return m * sin_j[:, None], sin_j


def scene_radius(scene):
    """half the diagonal of the bounding box of every triangle corner: fp32 min / max, the extents and the rest in binary64"""
    pts = np.concatenate([m.vertices[np.concatenate([m.faces[f] for _, f in m.sets]).reshape(-1)] for m in scene.meshes]).astype(F)
    d = pts.max(0).astype(D) - pts.min(0).astype(D)
    return D(0.5) * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


class EnvTable(PowerTable):
    """PowerTable with the environment as one more entry: g, G, w_env, q, pcdf (n + 1 entries), p_env, mcdf, ccdf"""

    def __init__(self, scene):
        super().__init__(scene)  # the mesh lights' w, area, and the tables of the scene WITHOUT the option
        em = scene.materials[scene.environment_material]
        tex = scene.textures[em.emission_texture - 1]
        self.H, self.W = tex.texels.shape[:2]
        g, sin_j = importance(tex, em.emission)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            G = np.cumsum(g.reshape(-1))[-1]
            self.g, self.G = g, G
            self.sphere = not (G > 0 and np.isfinite(G))
            if self.sphere:  # a black or broken image: the direction tables of the uniform sphere
                g = np.repeat(sin_j[:, None], self.W, 1)
            Gt = np.cumsum(g.reshape(-1))[-1]
            run = np.cumsum(g, axis=1)
            rowsum = run[:, -1]
            good = (rowsum > 0) & np.isfinite(rowsum)
            self.ccdf = np.where(good[:, None], run / rowsum[:, None], D(1.0)).astype(F)
            self.mcdf = (np.cumsum(rowsum) / Gt).astype(F)
            self.mcdf[-1] = F(1.0)
            self.g_tables = g
            R = scene_radius(scene)
            self.w_env = ((((D(4.0) * D(math.pi)) * R) * R) * (G / (D(self.W) * D(self.H)))) * (D(math.pi) / D(2.0))
            w = np.concatenate([self.w, [self.w_env]])
            npos = int((w > 0).sum())
            self.fallback = not np.isfinite(w).all() or npos == 0
            if self.fallback:
                q = np.full(self.n + 1, D(1.0) / D(self.n + 1))
            else:
                wsum = np.cumsum(w)[-1]
                q = np.where(w > 0, (D(1.0) - D(PHI)) * w / wsum + D(PHI) / D(npos), D(0.0))
            self.w_all, self.q = w, q
            acc = np.cumsum(q)
            self.pcdf = (acc / acc[-1]).astype(F)
            lo = np.concatenate([[F(0)], self.pcdf[:-1]]).astype(F)
            self.p = (self.pcdf - lo).astype(F)
            self.p_env = self.p[-1]
            self.lpdf = [F(F(F(1.0) / a) * p) for a, p in zip(self.area, self.p[:-1])]

    def env_cdf(self):
        return np.concatenate([self.mcdf, self.ccdf.reshape(-1)]).astype(F)


def sin_pi_t(t):
    """shade_common.h: env_sin_pi_t -- cos(pi (0.5 - t)) by its Taylor polynomial to y^20, Horner in binary64, rounded to fp32 once"""
    y = D(math.pi) * (D(0.5) - np.asarray(t, F).astype(D))
    y2 = y * y
    c = D(1.0) / D(2432902008176640000.0)
    for k in (6402373705728000.0, 20922789888000.0, 87178291200.0, 479001600.0, 3628800.0, 40320.0, 720.0, 24.0, 2.0):
        c = D(1.0) / D(k) - y2 * c
    return (D(1.0) - y2 * c).astype(F)


def _interval(cdf_rows, idx):
    """(lo, p) of entry idx of each row of cdf_rows, fp32"""
    k = np.arange(len(idx))
    lo = np.where(idx > 0, cdf_rows[k, np.maximum(idx, 1) - 1], F(0)).astype(F)
    return lo, (cdf_rows[k, idx] - lo).astype(F)


def environment_sample(t, u3, mapping):
    """phx_dev_environment_sample restated: light, texel, st, pdf in fp32 operation by operation; dir in binary64 from the fp32 (s, t)"""
    u3 = np.asarray(u3, F).reshape(-1, 3)
    pick, lu, lv = u3[:, 0], u3[:, 1], u3[:, 2]
    n = len(u3)
    W, H = t.W, t.H
    light = select(t.pcdf, pick).astype(np.uint32)
    env = light == t.n
    j = select(t.mcdf, lu)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rlo, prow = _interval(np.broadcast_to(t.mcdf, (n, H)), j)
        ru = np.fmin((lu - rlo) / prow, ONE_MINUS_EPS).astype(F)
        rows = t.ccdf[j]
        i = np.minimum((rows <= lv[:, None]).sum(1), W - 1)
        clo, pcol = _interval(rows, i)
        rv = np.fmin((lv - clo) / pcol, ONE_MINUS_EPS).astype(F)
        s = ((i.astype(F) + rv) / F(W)).astype(F)
        tt = ((j.astype(F) + ru) / F(H)).astype(F)
        sin_t = sin_pi_t(tt)
        pdf = (t.p_env * (((prow * pcol) * F(W * H)) / (F((2.0 * math.pi) * math.pi) * sin_t))).astype(F)
        ok = (sin_t > 0) & (pdf > 0) & np.isfinite(pdf)
    phi = ((s - F(0.5)) * F(2.0 * math.pi)).astype(F).astype(D)
    lam = ((F(0.5) - tt) * F(math.pi)).astype(F).astype(D)
    cl, sl, cp, sp = np.cos(lam), np.sin(lam), np.cos(phi), np.sin(phi)
    d = np.stack([cl * cp, cl * sp, sl], -1) if mapping == abi.ENV_LATLONG_Z_UP else np.stack([-(cl * sp), sl, cl * cp], -1)
    z = ~env
    out = {"light": light, "texel": np.stack([i, j], -1).astype(np.uint32), "st": np.stack([s, tt], -1).astype(F), "dir": d,
           "pdf": np.where(ok, pdf, F(0)).astype(F), "ok": ok & env, "prow": prow, "pcol": pcol}
    out["texel"][z] = 0; out["st"][z] = 0; out["dir"][z] = 0; out["pdf"][z] = 0
    return out


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------------
def env_scene(texels, filter=abi.TEX_CLOSEST, swrap=abi.WRAP_PERIODIC, twrap=abi.WRAP_CLAMP, mapping=abi.ENV_LATLONG_Y_UP, emission=(1.0, 0.5, 2.0),
              lamps=DECADES):
    """test_light_power's floor under its three lamps of three decades, plus an environment material with the image `texels`"""
    sc = lamps_scene(lamps, "env")
    sc.textures = [scenes.TextureDesc(np.asarray(texels, F), filter, swrap, twrap)]
    sc.materials.append(scenes.MaterialDesc(lobes=[], emission=tuple(emission), emission_texture=1, emission_mapping=mapping))
    sc.environment_material = len(sc.materials) - 1
    return sc


def _rand(w, h, seed=3):
    return np.random.default_rng(seed).uniform(0.0, 2.0, (h, w, 3)).astype(F)


def _two_suns():
    img = np.full((8, 16, 3), 0.05, F)
    img[0, 3] = (900.0, 800.0, 700.0); img[4, 11] = (500.0, 600.0, 700.0)  # row 0 (the pole: a small sine) and the middle row
    return img


def _zero_row():
    img = _rand(5, 4, 9); img[2] = 0.0
    return img


def _border(w=6, h=4):
    img = np.zeros((h, w, 3), F); img[0, 0] = 50.0; img[h - 1, w - 1] = 20.0
    return img


IMAGES = {
    "1x1": lambda: env_scene(np.full((1, 1, 3), 0.7, F)),
    "5x3": lambda: env_scene(_rand(5, 3)),
    "5x3_linear": lambda: env_scene(_rand(5, 3), abi.TEX_LINEAR),
    "two_suns": lambda: env_scene(_two_suns()),
    "two_suns_linear": lambda: env_scene(_two_suns(), abi.TEX_LINEAR),
    "two_suns_z_up": lambda: env_scene(_two_suns(), mapping=abi.ENV_LATLONG_Z_UP),
    "zero_row": lambda: env_scene(_zero_row()),
    "black": lambda: env_scene(np.zeros((3, 4, 3), F)),
    "negative": lambda: env_scene(-_rand(4, 4, 5), emission=(-1.0, 2.0, -0.5)),
    "nan_emission": lambda: env_scene(_rand(4, 2), emission=(float("nan"), 1.0, 1.0)),
    "inf_texel": lambda: env_scene(np.where(np.arange(24).reshape(2, 4, 3) == 7, np.inf, 1.0).astype(F)),
    **{f"border_{f}_{sw}_{tw}": (lambda f=f, sw=sw, tw=tw: env_scene(_border(), f, sw, tw))
       for f in (abi.TEX_LINEAR, abi.TEX_CLOSEST) for sw in (0, 1, 2) for tw in (0, 1, 2)},
}


# ---- (c) properties of the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IMAGES))
def test_the_tables_are_monotone_end_at_one_and_price_every_texel_that_can_be_seen(name):
    sc = IMAGES[name]()
    t = EnvTable(sc)
    for cdf in [t.pcdf, t.mcdf] + list(t.ccdf):
        assert cdf.dtype == F and cdf[-1] == F(1.0) and (np.diff(cdf) >= 0).all() and cdf[0] >= 0
    assert len(t.pcdf) == t.n + 1 == 4
    if name == "black":
        assert t.G == 0 and t.w_env == 0 and t.p_env == 0 and t.sphere and not t.fallback
        assert t.pcdf[:-1].tobytes() == PowerTable(sc).pcdf.tobytes()  # the mesh lights' table is the one without the option
    elif name in ("nan_emission", "inf_texel"):
        assert t.fallback and t.sphere and np.abs(t.p.astype(D) - 0.25).max() < 2.0 ** -24
    else:
        assert not t.fallback and not t.sphere and t.w_env > 0 and t.p_env >= F(PHI / 4) * F(0.999)
    rng = np.random.default_rng(11)
    u3 = (rng.integers(0, 1 << 24, (1 << 14, 3)).astype(F) * F(2.0 ** -24)).astype(F)
    u3[:, 0] = np.maximum(u3[:, 0], t.pcdf[-2])  # the environment's interval (empty for a black image)
    s = environment_sample(t, u3, sc.materials[-1].emission_mapping)
    if t.p_env == 0:
        assert not s["ok"].any() and not s["pdf"].any()
        return
    i, j = s["texel"][:, 0], s["texel"][:, 1]
    assert (s["light"] == t.n).all() and s["ok"].all() and (t.g_tables[j, i] > 0).all()  # a texel with g = 0 is never returned
    assert ((s["st"] >= 0) & (s["st"] <= 1)).all()
    # (s, t) lies in its texel; a remapped draw within an ulp of (i + 1) of 1 may round onto the texel's far border, the rule's stated limit
    di, dj = np.floor(s["st"][:, 0].astype(D) * t.W) - i, np.floor(s["st"][:, 1].astype(D) * t.H) - j
    assert np.isin(di, (0, 1)).all() and np.isin(dj, (0, 1)).all() and (di != 0).mean() < 1e-3 and (dj != 0).mean() < 1e-3
    assert np.abs(np.linalg.norm(s["dir"], axis=1) - 1.0).max() < 1e-12
    # the density integrates to one: sum over texels of P_row P_col is 1, and pdf_omega d omega = P W H / (2 pi^2 sin) * (2 pi^2 / (W H)) sin ds dt
    mlo = np.concatenate([[F(0)], t.mcdf[:-1]]); clo = np.concatenate([np.zeros((t.H, 1), F), t.ccdf[:, :-1]], 1)
    P = (t.mcdf - mlo).astype(D)[:, None] * (t.ccdf - clo).astype(D)
    assert abs(P.sum() - 1.0) < 1e-5 and ((P > 0) == (t.g_tables > 0)).all()
    if not t.sphere:  # ... and follows g to fp32 rounding
        assert np.abs(P - t.g / t.G).max() < 2.0 ** -22


def test_linear_filtering_prices_the_neighbours_of_a_bright_texel():
    near, lin = EnvTable(IMAGES["two_suns"]()), EnvTable(IMAGES["two_suns_linear"]())
    assert lin.g[4, 10] == lin.g[4, 11] == lin.g[4, 12] and lin.g[4, 10] > 1000 * near.g[4, 10]  # the 3 x 3 maximum is visible
    assert lin.g[3, 11] > 1000 * near.g[3, 11] and lin.g[5, 12] > 1000 * near.g[5, 12] and lin.g[4, 14] == near.g[4, 14]
    assert lin.g[0, 2] > 1000 * near.g[0, 2] and lin.g[1, 4] > 1000 * near.g[1, 4]  # row 0: CLAMP repeats the row, the row below sees it
    assert (lin.g >= near.g).all() and lin.G > near.G


def test_the_wrap_modes_decide_which_border_texels_see_the_bright_corner():
    g = {k: EnvTable(IMAGES[f"border_{abi.TEX_LINEAR}_{k[0]}_{k[1]}"]()).g > 0 for k in [(sw, tw) for sw in (0, 1, 2) for tw in (0, 1, 2)]}
    P, Cl, B = abi.WRAP_PERIODIC, abi.WRAP_CLAMP, abi.WRAP_BLACK
    assert g[(Cl, Cl)].sum() == 8 and g[(B, B)].sum() == 8 and (g[(Cl, Cl)] == g[(B, B)]).all()  # two 2 x 2 corners
    assert g[(P, Cl)][0, 5] and g[(P, Cl)][1, 5] and not g[(Cl, Cl)][0, 5]  # the bright column 0 reaches column W - 1 round the seam
    assert g[(Cl, P)][3, 0] and g[(Cl, P)][3, 1] and not g[(Cl, Cl)][3, 0]  # ... and row 0 reaches row H - 1 under a periodic t
    assert g[(P, P)].sum() > g[(P, Cl)].sum() > g[(Cl, Cl)].sum()
    near = EnvTable(IMAGES[f"border_{abi.TEX_CLOSEST}_0_0"]()).g > 0
    assert near.sum() == 2 and near[0, 0] and near[3, 5]


def test_the_mapping_changes_the_direction_and_nothing_else():
    y, z = IMAGES["two_suns"](), IMAGES["two_suns_z_up"]()
    ty, tz = EnvTable(y), EnvTable(z)
    assert ty.env_cdf().tobytes() == tz.env_cdf().tobytes() and ty.pcdf.tobytes() == tz.pcdf.tobytes()
    u3 = np.array([[0.9999, 0.3, 0.2], [0.9999, 0.7, 0.9]], F)
    a, b = environment_sample(ty, u3, abi.ENV_LATLONG_Y_UP), environment_sample(tz, u3, abi.ENV_LATLONG_Z_UP)
    assert a["pdf"].tobytes() == b["pdf"].tobytes() and (a["texel"] == b["texel"]).all()
    assert np.allclose(a["dir"][:, 1], b["dir"][:, 2]) and np.allclose(a["dir"][:, 2], b["dir"][:, 0]) and np.allclose(-a["dir"][:, 0], b["dir"][:, 1])


def test_the_polynomial_is_the_sine():
    t = np.linspace(0.0, 1.0, 100001).astype(F)
    assert np.abs(sin_pi_t(t).astype(D) - np.sin(math.pi * t.astype(D))).max() < 1e-7 and sin_pi_t(F(0.5)) == 1.0


# ---- (d) flatten_scene ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat_env():
    """the host_flatten_env library: test_light_power's flatten() plus the environment's tables ("env_cdf", "env_p", "env_w")"""
    lib = NL.load("host_flatten_env")
    lib.hf_flatten.restype = C.c_void_p; lib.hf_flatten.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Options)]
    lib.hf_free.argtypes = [C.c_void_p]
    lib.hf_status.argtypes = [C.c_void_p]
    lib.hf_error.restype = C.c_char_p; lib.hf_error.argtypes = [C.c_void_p]
    lib.hf_array.restype = C.c_void_p; lib.hf_array.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    lib.hf_power_table.restype = C.c_void_p; lib.hf_power_table.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.hf_env_cdf.restype = C.c_void_p; lib.hf_env_cdf.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.hf_env_p.restype = C.c_float; lib.hf_env_p.argtypes = [C.c_void_p]
    lib.hf_env_w.restype = C.c_double; lib.hf_env_w.argtypes = [C.c_void_p]
    lib.hf_word.restype = C.c_uint32; lib.hf_word.argtypes = [C.c_void_p, C.c_int]

    def flatten(scene, light_sampling):
        s, keep = scene.pack()
        opt = abi.Options(); opt.light_sampling = light_sampling; opt.path_depth = 9
        h = lib.hf_flatten(C.byref(s), C.byref(opt))
        try:
            out = {"status": lib.hf_status(h), "error": lib.hf_error(h).decode()}
            if out["status"] == 0:
                n = C.c_uint64(0)
                grab = lambda p, dtype: np.frombuffer(C.string_at(p, n.value) if n.value else b"", dtype).copy()
                for name, (which, dtype) in ARRAYS.items():
                    out[name] = grab(lib.hf_array(h, which, C.byref(n)), dtype)
                out["light_pcdf"] = grab(lib.hf_power_table(h, C.byref(n)), F)
                out["env_cdf"] = grab(lib.hf_env_cdf(h, C.byref(n)), F)
                out["env_p"], out["env_w"] = F(lib.hf_env_p(h)), D(lib.hf_env_w(h))
                for name, which in WORDS.items():
                    out[name] = lib.hf_word(h, which)
            return out
        finally:
            lib.hf_free(h)
    return flatten


@pytest.mark.parametrize("name", list(IMAGES))
def test_flatten_scene_builds_the_restatements_tables(flat_env, name):
    sc = IMAGES[name]()
    t = EnvTable(sc)
    r = flat_env(sc, AREA_POWER_ENV)
    assert r["status"] == 0, r["error"]
    assert r["num_lights"] == t.n and r["light_pcdf"].tobytes() == t.pcdf.tobytes()
    assert r["env_w"].tobytes() == D(t.w_env).tobytes() and r["env_p"].tobytes() == t.p_env.tobytes()
    assert len(r["env_cdf"]) == t.H + t.H * t.W and r["env_cdf"].tobytes() == t.env_cdf().tobytes()
    assert r["lights"]["lpdf"].tobytes() == np.array(t.lpdf, F).tobytes()
    assert r["any_tex"] == (SC_TEX_ENV | SC_LIGHTS_BY_AREA | SC_LIGHTS_BY_POWER | SC_LIGHTS_ENV) and r["diffuse_only"] == 0
    # with the bit clear: the selection table and lpdf of light selection by power as it was, no environment table, and every other byte the same
    base = PowerTable(sc)
    r0 = flat_env(sc, AREA_POWER)
    assert r0["status"] == 0 and r0["any_tex"] == (SC_TEX_ENV | SC_LIGHTS_BY_AREA | SC_LIGHTS_BY_POWER)
    assert r0["light_pcdf"].tobytes() == base.pcdf.tobytes() and r0["lights"]["lpdf"].tobytes() == np.array(base.lpdf, F).tobytes()
    assert len(r0["env_cdf"]) == 0 and r0["env_p"] == 0 and r0["env_w"] == 0
    lights = r["lights"].copy(); lights["lpdf"] = r0["lights"]["lpdf"]
    assert lights.tobytes() == r0["lights"].tobytes()
    for key in ARRAYS:
        if key != "lights":
            assert r[key].tobytes() == r0[key].tobytes(), key
    for word in WORDS:
        if word != "any_tex":
            assert r[word] == r0[word], word


@pytest.mark.parametrize("word", [0x200, 0x201, 0x300, 0x302, 0x701])
def test_flatten_scene_refuses_every_other_word(flat_env, word):
    r = flat_env(IMAGES["5x3"](), word)
    assert r["status"] == 1 and "light_sampling" in r["error"]


def test_flatten_scene_accepts_the_word_only_with_an_environment_image(flat_env):
    assert flat_env(IMAGES["5x3"](), AREA_POWER_ENV)["status"] == 0
    no_env = lamps_scene(DECADES)
    constant = lamps_scene(DECADES); constant.materials.append(scenes.MaterialDesc(lobes=[], emission=(0.5, 0.5, 0.5))); constant.environment_material = 4
    for sc in (no_env, constant):
        assert flat_env(sc, AREA_POWER)["status"] == 0
        r = flat_env(sc, AREA_POWER_ENV)
        assert r["status"] == 1 and "light_sampling" in r["error"] and "emission_texture" in r["error"]
    only_sky = IMAGES["5x3"](); only_sky.meshes = only_sky.meshes[:1]  # the floor alone: a scene still needs an emissive face set
    r = flat_env(only_sky, AREA_POWER_ENV)
    assert r["status"] == 1 and "no emissive face set" in r["error"]


def test_sun_floor_is_one_texel_of_light():
    sc = scenes.sun_floor()
    t = EnvTable(sc)
    assert (t.W, t.H) == (64, 32) and t.n == 1 and t.w[0] == 0 and t.p_env == 1.0 and t.pcdf.tolist() == [0.0, 1.0]
    assert sc.textures[0].filter == abi.TEX_CLOSEST and sc.textures[0].texels[8, 40, 0] == 2000.0 and (np.delete(sc.textures[0].texels.reshape(-1, 3), 8 * 64 + 40, 0) == F(0.1)).all()
    mlo = np.concatenate([[F(0)], t.mcdf[:-1]]); clo = np.concatenate([np.zeros((t.H, 1), F), t.ccdf[:, :-1]], 1)
    P = (t.mcdf - mlo).astype(D)[:, None] * (t.ccdf - clo).astype(D)
    assert 0.85 < P[8, 40] < 0.95  # the sun's texel takes most draws; its elevation is about 42 degrees
    assert abs(math.degrees(math.pi * (0.5 - 8.5 / 32)) - 42.2) < 0.1
