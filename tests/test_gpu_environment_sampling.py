"""Sampling the environment image by next-event estimation (light_sampling 0x301) on the device: the parity hook against the numpy
restatement of tests/test_environment_sampling.py, a closed-form film (scenes.sun_floor: mean and variance from a float64 model in this file),
and the films the option must not change, bit for bit."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

from conftest import ROOT, bits_equal
from phosphorus_mk2_amd import abi, scenes
from test_environment_sampling import EnvTable, env_scene, environment_sample
from test_gpu_environment import np_env_st
from test_gpu_shade_kernels import FAMILIES, build, expected_kernels

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
COUNTERS = ("camera_samples", "rays_closest", "rays_shadow", "rays_masked")
AREA_POWER = dict(light_sampling="area", light_selection="power")
AREA_POWER_ENV = dict(light_sampling="area", light_selection="power", environment_sampling=True)
GOLDEN = os.path.join(ROOT, "tests", "golden", "environment_sampling_parent_films.json")


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


# ---- 1. the hook against the restatement ----------------------------------------------------------------------------------------------------
def hook_image(w, h, seed):
    """random texels, a fifth of them black, one black row, a bright texel in row 0 and one in the middle row"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 2.0, (h, w, 3)).astype(F)
    img[rng.uniform(size=(h, w)) < 0.2] = 0.0
    img[h - 2] = 0.0
    img[0, 3] = (300.0, 200.0, 100.0); img[h // 2, w - 2] = (50.0, 80.0, 90.0)
    return img


def neighbours(values):
    """0, 1 - 2^-24 and every value with both of its ulp neighbours (not below 0)"""
    v = np.asarray(values, F).reshape(-1)
    v = np.concatenate([[F(0), F(1) - F(2.0 ** -24)], np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]).astype(F)
    return np.unique(v[v >= 0])


def hook_draws(t, mapping):
    rng = np.random.default_rng(21)
    u = [(rng.integers(0, 1 << 24, (1 << 16, 3)).astype(F) * F(2.0 ** -24)).astype(F)]
    env = F(1) - F(2.0 ** -24)  # a pick inside the environment's interval
    pe = neighbours(t.pcdf); u.append(np.stack([pe, np.full(len(pe), 0.37, F), np.full(len(pe), 0.61, F)], -1))
    le = neighbours(t.mcdf); u.append(np.stack([np.full(len(le), env, F), le, np.full(len(le), 0.61, F)], -1))
    mlo = np.concatenate([[F(0)], t.mcdf[:-1]]).astype(F)
    for j in range(t.H):  # every entry of every row that can be chosen, through a draw in the middle of that row's interval
        lu = F(mlo[j] + (t.mcdf[j] - mlo[j]) * F(0.5))
        if not (mlo[j] <= lu < t.mcdf[j]):
            continue
        ve = neighbours(t.ccdf[j]); u.append(np.stack([np.full(len(ve), env, F), np.full(len(ve), lu, F), ve], -1))
    return np.concatenate(u).astype(F)


@pytest.mark.parametrize("size", [(16, 8), (64, 32)])
@pytest.mark.parametrize("mapping", [abi.ENV_LATLONG_Y_UP, abi.ENV_LATLONG_Z_UP])
@pytest.mark.parametrize("filt", [abi.TEX_LINEAR, abi.TEX_CLOSEST])
def test_the_hook_is_the_restatement(xpu, size, mapping, filt):
    sc = env_scene(hook_image(*size, seed=size[0] + filt), filt, mapping=mapping)
    t = EnvTable(sc)
    assert not t.fallback and not t.sphere and t.p_env > 2.0 ** -20
    u3 = hook_draws(t, mapping)
    assert u3[:, 0].max() > 1 and u3[:, 1].max() > 1 and u3[:, 2].max() > 1 and u3.min() == 0 and len(u3) > (1 << 16) + t.W * t.H
    want = environment_sample(t, u3, mapping)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2, **AREA_POWER_ENV))
    try:
        dev.preprocess(sc)
        got = dev.environment_sample(u3)
        ls, le = dev.light_sample(u3), dev.light_emission(u3)
        ok = got["pdf"] > 0
        looked_up = dev.environment_lookup(got["dir"][ok])
    finally:
        dev.close()
    env = want["light"] == t.n
    assert env.sum() > 1 << 14 and (~env).sum() > 1 << 11
    for key in ("light", "texel", "st", "pdf"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert (ok == want["ok"]).all() and ok.sum() > 1 << 14
    assert np.abs(got["dir"].astype(D) - want["dir"]).max() <= 5e-6
    assert not got["dir"][~env].any() and not got["e"][~ok].any()
    # e is what a miss in that direction adds, bit for bit
    assert got["e"][ok].tobytes() == looked_up.tobytes()
    # a texel with g = 0 is never returned
    i, j = got["texel"][ok, 0], got["texel"][ok, 1]
    assert (t.g[j, i] > 0).all()
    # the direction maps back into the texel that priced it, except for draws within 2^-20 of a texel border
    st, fine = np_env_st(got["dir"][ok], mapping)
    s, tt = got["st"][ok, 0].astype(D) * t.W, got["st"][ok, 1].astype(D) * t.H
    inner = (np.abs(s - np.round(s)) > 2.0 ** -20 * t.W) & (np.abs(tt - np.round(tt)) > 2.0 ** -20 * t.H)
    # (near a pole every s belongs to the same point: the row must match there, the column where cos(lambda) is not tiny)
    away = np.abs(tt - t.H / 2) < t.H / 2 - 2.0 ** -10 * t.H
    assert fine.all() and inner.sum() > 1 << 14  # (the table-entry draws sit on texel borders by construction)
    assert (np.floor(st[inner, 1].astype(D) * t.H) == j[inner]).all()
    assert (np.floor(st[inner & away, 0].astype(D) * t.W) % t.W == i[inner & away]).all()
    # the other two hooks answer an environment pick with nothing, and a mesh pick as they did
    assert (ls["light"] == want["light"]).all() and (ls["tri"][env] == 0xffffffff).all() and (ls["tri"][~env] < 2).all()
    assert not ls["pdf"][env].any() and not ls["P"][env].any() and not ls["bary"][env].any() and not le["e"][env].any() and not le["st"][env].any()
    lpdf = np.array(t.lpdf, F)
    assert ls["pdf"][~env].tobytes() == lpdf[want["light"][~env]].tobytes() and (le["e"][~env] != 0).any(-1).all()


def test_a_black_image_is_never_chosen_and_the_hook_needs_the_option(xpu):
    sc = env_scene(np.zeros((4, 8, 3), F))
    t = EnvTable(sc)
    u3 = hook_draws(t, 0)
    u3 = u3[u3[:, 0] < 1]
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2, **AREA_POWER_ENV))
    try:
        dev.preprocess(sc)
        got = dev.environment_sample(u3)
        assert (got["light"] < t.n).all() and not got["pdf"].any() and not got["e"].any() and got["light"].tobytes() == environment_sample(t, u3, 0)["light"].tobytes()
        one = dev.environment_sample(np.array([[1.0, 0.5, 0.5]], F))  # outside the draws' range: the last entry, with pdf 0 -- no shadow ray
        assert one["light"][0] == t.n and one["pdf"][0] == 0
    finally:
        dev.close()
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2, **AREA_POWER))
    try:
        dev.preprocess(sc)
        with pytest.raises(xpu.DeviceError, match="environment_sample"):
            dev.environment_sample(u3[:4])
    finally:
        dev.close()
    with pytest.raises(xpu.DeviceError, match="light_sampling"):  # no image on the environment: refused at preprocess
        xpu.render(scenes.cornell(16, 16), spp=1, depth=2, **AREA_POWER_ENV)


# ---- 2. the closed form: scenes.sun_floor ---------------------------------------------------------------------------------------------------
SPP, SEED = 256, 5


def sun_floor_model(t, texels):
    """float64, no render and no project code in it: per channel the pixel mean rho / pi * sum over texels of L * int cos d omega, the second
    moment of ONE next-event sample drawn from the table t (P = P_row * P_col of the fp32 tables, p_env = 1) and of one cosine-weighted BSDF
    sample.  The floor's normal is +y and every point sees the whole upper hemisphere: rows 0 .. H / 2 - 1 of the Y-up image.  The integrals over
    a texel (elevation l from l1 down to l0, azimuth 2 pi / W) are closed forms: int sin cos dl = (sin^2 l1 - sin^2 l0) / 2 and
    int sin^2 cos^2 dl = [l / 8 - sin(4 l) / 32]."""
    H, W = texels.shape[:2]
    L = texels[..., 0].astype(D)
    assert (texels[..., 0] == texels[..., 1]).all() and (texels[..., 0] == texels[..., 2]).all() and H % 2 == 0
    rho = np.array(scenes.SUN_FLOOR_RHO, D)
    j = np.arange(H // 2)
    l1, l0 = math.pi * (0.5 - j / H), math.pi * (0.5 - (j + 1) / H)
    dphi = 2.0 * math.pi / W
    cos_w = dphi * (np.sin(l1) ** 2 - np.sin(l0) ** 2) / 2.0                      # int cos(theta) d omega over a texel of row j
    sc2 = dphi * ((l1 / 8 - np.sin(4 * l1) / 32) - (l0 / 8 - np.sin(4 * l0) / 32))  # int sin^2 cos^2 dl dphi
    Lu = L[: H // 2]
    mean = rho / math.pi * (Lu * cos_w[:, None]).sum()
    mlo = np.concatenate([[F(0)], t.mcdf[:-1]]); clo = np.concatenate([np.zeros((H, 1), F), t.ccdf[:, :-1]], 1)
    P = ((t.mcdf - mlo).astype(F)[:, None] * (t.ccdf - clo).astype(F)).astype(D)[: H // 2]
    # X = (rho / pi) L sin(l) / pdf_omega, pdf_omega = P W H / (2 pi^2 cos(l)):  E X^2 = sum (rho / pi)^2 L^2 2 pi^2 / (P W H) int sin^2 cos^2
    m2_nee = (rho / math.pi) ** 2 * (Lu ** 2 * (2.0 * math.pi ** 2 / (P * W * H)) * sc2[:, None]).sum()
    m2_bsdf = rho ** 2 * (Lu ** 2 * cos_w[:, None]).sum() / math.pi  # X = rho L(d), d ~ cos / pi
    return mean, m2_nee - mean ** 2, m2_bsdf - mean ** 2


@pytest.fixture(scope="module")
def sun_floor_films(xpu):
    sc = scenes.sun_floor()
    nee, st_nee = xpu.render(sc, spp=SPP, pps=1, depth=2, seed=SEED, **AREA_POWER_ENV)
    bsdf, st_bsdf = xpu.render(sc, spp=SPP, pps=1, depth=2, seed=SEED, **AREA_POWER)
    return sc, nee[..., :3].astype(D), st_nee, bsdf[..., :3].astype(D), st_bsdf


def test_sun_floor_under_environment_sampling_has_the_models_mean_and_variance(sun_floor_films):
    sc, nee, st, _, _ = sun_floor_films
    t = EnvTable(sc)
    mean, var_nee, var_bsdf = sun_floor_model(t, sc.textures[0].texels)
    npix = nee.shape[0] * nee.shape[1]
    z = (nee - mean) / np.sqrt(var_nee / SPP)
    zm = (nee.mean((0, 1)) - mean) / np.sqrt(var_nee / (SPP * npix))
    rms = np.sqrt((z ** 2).mean((0, 1)))
    rms_b = np.sqrt((((nee - mean) / np.sqrt(var_bsdf / SPP)) ** 2).mean((0, 1)))
    print(f"model mean {mean}, one-sample sd: next-event {np.sqrt(var_nee)}, BSDF sampling {np.sqrt(var_bsdf)}, variance ratio {var_bsdf / var_nee}")
    print(f"film mean {nee.mean((0, 1))}: z of the film mean {zm}, worst pixel {np.abs(z).max((0, 1))}, rms z {rms}; rms against the BSDF model {rms_b}")
    assert st["rays_shadow"] + st["rays_masked"] == st["rays_closest"] and st["rays_shadow"] > 0.4 * st["camera_samples"]
    assert (np.abs(zm) < 4).all()
    assert (np.abs(z) < 5).all()
    assert ((rms > 0.9) & (rms < 1.1)).all()
    assert (rms_b < 0.9).all()  # the same film scored as if BSDF sampling had made it: the test tells the two estimators apart


def test_sun_floor_has_the_same_mean_without_the_option(sun_floor_films):
    sc, nee, _, bsdf, st = sun_floor_films
    mean, var_nee, var_bsdf = sun_floor_model(EnvTable(sc), sc.textures[0].texels)
    npix = bsdf.shape[0] * bsdf.shape[1]
    zm = (bsdf.mean((0, 1)) - mean) / np.sqrt(var_bsdf / (SPP * npix))
    print(f"BSDF sampling: film mean {bsdf.mean((0, 1))}, model {mean}, z {zm}; per-pixel variance {bsdf.var((0, 1))} against {var_bsdf / SPP} (next-event: {nee.var((0, 1))})")
    assert (np.abs(zm) < 4).all()  # the option changes the variance, not the expectation
    assert (bsdf.var((0, 1)) > 20 * nee.var((0, 1))).all()


def test_camera_visible_sky_is_untouched(xpu):
    """depth 1, the camera looking at the horizon: a pixel whose camera rays all miss adds the image at depth 0 under either word, bit for bit;
    the floor's pixels get their light from the new samples alone"""
    sc = scenes.sun_floor(look="horizon")
    a, sa = xpu.render(sc, spp=16, pps=1, depth=1, seed=SEED, normals=True, **AREA_POWER_ENV)
    b, sb = xpu.render(sc, spp=16, pps=1, depth=1, seed=SEED, normals=True, **AREA_POWER)
    sky = (b[..., 4:7] == 0).all(-1)           # every camera ray of the pixel missed
    floor = ~sky & (b[..., :3] == 0).all(-1)   # ... hit the floor: black without the option (the lamp is black, and no bounce at depth 1)
    assert sky.sum() > 200 and floor.sum() > 100 and bits_equal(a[..., 4:7], b[..., 4:7])
    assert bits_equal(a[sky], b[sky]) and (b[sky][:, :3] > 0).all()
    assert (a[floor][:, :3] > 0).any(-1).mean() > 0.9
    assert sa["shade_kernels"] == sb["shade_kernels"] and sa["rays_closest"] == sb["rays_closest"] and sa["rays_shadow"] > sb["rays_shadow"]


# ---- 3. what the option must not change ------------------------------------------------------------------------------------------------------
ENV_FAMILIES = [name for name, f in FAMILIES.items() if f[2]]
assert ENV_FAMILIES == ["env", "env_perhit", "env_tex", "env_tex_perhit", "mask_env"]


def film_record(film, st):
    return {"film_sha256": hashlib.sha256(np.ascontiguousarray(film, F).tobytes()).hexdigest(), **{k: int(st[k]) for k in COUNTERS}, "shade_kernels": int(st["shade_kernels"])}


@pytest.fixture(scope="module")
def family_films(xpu):
    done = {}

    def get(name, word, black=False):
        if (name, word, black) not in done:
            sc = build(name, False)[0]
            if black:
                t = sc.textures[sc.materials[sc.environment_material].emission_texture - 1]
                t.texels = np.zeros_like(t.texels)
            done[(name, word, black)] = xpu.render(sc, spp=16, pps=1, depth=9, seed=5, **(AREA_POWER_ENV if word == 0x301 else AREA_POWER))
        return done[(name, word, black)]
    return get


@pytest.mark.parametrize("name", ENV_FAMILIES)
def test_without_the_bit_an_environment_scene_renders_what_it_rendered(family_films, name):
    """64 x 48 x 16 spp under 0x101 against the record of the commit before the option existed (tests/golden: film hash, counters, kernels): the
    new branch's false side through every ENV instantiation"""
    film, st = family_films(name, 0x101)
    assert film.shape == (48, 64, 4) and st["shade_kernels"] == expected_kernels(FAMILIES[name][0], False)
    assert film_record(film, st) == json.load(open(GOLDEN))[name]


@pytest.mark.parametrize("name", ENV_FAMILIES)
def test_a_black_image_under_the_option_renders_the_film_without_it(family_films, name):
    a, sa = family_films(name, 0x301, black=True)
    b, sb = family_films(name, 0x101, black=True)
    assert bits_equal(a, b) and all(sa[k] == sb[k] for k in COUNTERS) and sa["shade_kernels"] == sb["shade_kernels"]
    assert a[..., :3].any() and sa["device_bytes"] > sb["device_bytes"]  # (the lamp lights the scene; the tables are counted)


@pytest.mark.parametrize("name", ENV_FAMILIES)
def test_a_lit_image_under_the_option_runs_the_same_kernels(family_films, name):
    a, sa = family_films(name, 0x301)
    b, sb = family_films(name, 0x101)
    assert sa["shade_kernels"] == sb["shade_kernels"] == expected_kernels(FAMILIES[name][0], False)
    assert np.isfinite(a).all() and not bits_equal(a, b)
    assert sa["rays_shadow"] + sa["rays_masked"] == sa["rays_closest"] and sa["camera_samples"] == sb["camera_samples"]
