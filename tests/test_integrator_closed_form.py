"""The CPU oracle's integrator against closed forms (tests/integrator64.py, which shares no code with it): furnace scenes whose pixel,
ray counts and survival probabilities are known.

a  a closed Lambert cavity that emits: film mean, rays per sample, masked share and the increment from one depth to the next (roulette
   first sees beta = rho^2 -- two bounces sampled -- so the grey survival chain is rho^2, rho, rho, ...);
b  the same cavity cut into two and three lights of unequal area: nothing changes;
c  zero-variance scenes under a uniform environment: a Lambert floor, a planar mirror, a stack of transparent sheets (roulette only);
d  one-lobe floors (Oren-Nayar, GGX, sheen) whose bounce weight is bsdf64's E[f cos / pdf] at the pixel's view angle;
e  the cavity wall's own emission, seen directly.

Tolerances.  Monte-Carlo scenes are deterministic runs (counter RNG, fixed seed): 4 standard errors, the standard error being a RECORDED
constant -- measured once on the CPU oracle from the spread of its per-pixel means (std over the film / sqrt(pixels)) for that scene and
depth, relative to the model -- never a figure of the film under test.  None exceeds 2 % (asserted).  Ray counts: 4 binomial standard
errors from the model's survival probabilities.  Zero-variance scenes: fp32 rounding of the operations on the model's path.
tests/test_gpu_integrator_closed_form.py runs the same checks on the device."""
import math

import numpy as np
import pytest

import bsdf64
import integrator64 as I
from phosphorus_mk2_amd import abi, scenes

SEED, SPP = 5, 256
DEPTHS = (1, 2, 3, 4, 5, 8, 16)
RHO = {"colour": I.RHO_COLOUR, "grey": I.RHO_GREY}
MC_CAP = 0.02  # no Monte-Carlo tolerance above 2 % relative on any channel

# Relative standard errors (r, g, b) of the oracle's film mean, cavity(rho, nsets), 16 x 16 x 256 spp, seed 5: std of the 256 pixel values /
# 16 / the model's pixel.  Measured on the CPU oracle; key (rho, nsets, depth).
SE_MEAN = {
    ("colour", 1, 1): (4.01e-04, 3.51e-04, 2.34e-04),
    ("colour", 1, 2): (3.12e-04, 2.89e-04, 2.17e-04),
    ("colour", 1, 3): (3.18e-04, 2.82e-04, 2.16e-04),
    ("colour", 1, 4): (9.49e-04, 4.13e-04, 2.17e-04),
    ("colour", 1, 5): (1.51e-03, 5.22e-04, 2.17e-04),
    ("colour", 1, 8): (2.97e-03, 6.65e-04, 2.17e-04),
    ("colour", 1, 16): (4.77e-03, 6.92e-04, 2.17e-04),
    ("grey", 1, 1): (3.51e-04, 3.51e-04, 3.51e-04),
    ("grey", 1, 2): (2.89e-04, 2.89e-04, 2.89e-04),
    ("grey", 1, 3): (2.82e-04, 2.82e-04, 2.82e-04),
    ("grey", 1, 4): (4.44e-04, 4.44e-04, 4.44e-04),
    ("grey", 1, 5): (5.98e-04, 5.98e-04, 5.98e-04),
    ("grey", 1, 8): (8.37e-04, 8.37e-04, 8.37e-04),
    ("grey", 1, 16): (9.11e-04, 9.11e-04, 9.11e-04),
    ("colour", 2, 4): (1.43e-03, 1.07e-03, 8.33e-04),
    ("colour", 3, 4): (1.04e-03, 5.94e-04, 4.09e-04),
    ("grey", 2, 8): (1.28e-03, 1.28e-03, 1.28e-03),
    ("grey", 3, 8): (9.43e-04, 9.43e-04, 9.43e-04),
}
# the same for the mean of film_D - film_D' (D' the next smaller depth of the list: the same draws up to hit D' - 1); key (rho, nsets, D', D)
SE_INCREMENT = {
    ("colour", 1, 1, 2): (5.32e-04, 5.32e-04, 5.32e-04),
    ("grey", 1, 1, 2): (5.32e-04, 5.32e-04, 5.32e-04),
    ("colour", 1, 2, 3): (7.98e-04, 7.98e-04, 7.98e-04),
    ("grey", 1, 2, 3): (7.98e-04, 7.98e-04, 7.98e-04),
    ("colour", 1, 3, 4): (2.91e-03, 2.91e-03, 2.91e-03),
    ("grey", 1, 3, 4): (3.19e-03, 3.19e-03, 3.19e-03),
    ("colour", 1, 4, 5): (3.92e-03, 3.92e-03, 3.92e-03),
}
# cavity_direct(): the next-event factor K(x) of a wall point has mean 1 within 3e-5 and standard deviation 3e-4 over the wall (the facets'
# areas span 0.93 .. 1.20 of their mean); its means over 256, 1 024 (the camera's footprint) and 2 048 points differ by < 4e-5.  A film
# averages it over thousands of hits: 1e-4 relative is allowed for the model's own factor on top of the sampling error.
K_SPREAD, K_MODEL = 5e-4, 1e-4


def render(orc, sc, depth, spp=SPP, seed=SEED):
    film, st = orc.Oracle(sc, spp=spp, pps=1, depth=depth).render(rng=orc.RNG_COUNTER, seed=seed, threads=8)
    return film[..., :3].astype(np.float64), st


_models = {}


def cavity_model(rho, nsets, depth, level=3):
    key = (rho, nsets, depth, level)
    if key not in _models:
        sc = I.cavity(RHO[rho], nsets=nsets, level=level)
        hits, spread = I.cavity_hits(sc, RHO[rho], I.LE_CAVITY, depth)
        assert spread < K_SPREAD, spread
        _models[key] = I.chain(hits, depth)
    return _models[key]


def count_tolerance(events, n):
    return 4.0 * I.binomial_se(events, n)


def check_cavity(film, st, rho, nsets, depth, level=3, se=None):
    """film (H, W, 3) float64 and stats of a cavity render against the model: mean per channel, rays per sample, masked share"""
    m = cavity_model(rho, nsets, depth, level)
    n = st["camera_samples"]
    se = np.asarray(SE_MEAN[(rho, nsets, depth)] if se is None else se)
    tol = 4.0 * se + K_MODEL
    assert (tol <= MC_CAP).all(), tol
    ratio = film.reshape(-1, 3).mean(0) / m["pixel"]
    print(f"cavity {rho} sets {nsets} D {depth}: mean / model {ratio}, tolerance {tol}, rays {st['rays_closest'] / n:.5f} model {float(m['closest']):.5f}")
    assert (np.abs(ratio - 1.0) <= tol).all(), (ratio, tol)
    assert abs(st["rays_closest"] / n - float(m["closest"])) <= count_tolerance(m["reach"][1:], n), (st["rays_closest"] / n, float(m["closest"]))
    # every ray of a closed cavity hits, and every hit asks for one light sample: traced or masked
    assert st["rays_shadow"] + st["rays_masked"] == st["rays_closest"] and st["rays_shadow"] <= st["rays_closest"]
    # masked: the sample lies on the hit's own facet (the shadow ray starts 1e-4 above that plane): 1 / 1 280 with one light
    share, own = st["rays_masked"] / st["rays_closest"], float(m["masked"] / m["closest"])
    assert share <= own + 4.0 * math.sqrt(own / st["rays_closest"]) + 1e-4, (share, own)  # 1e-4: samples next to a shared edge
    return ratio


def check_increment(film_hi, film_lo, rho, nsets, d_lo, d_hi, se=None):
    """film_D - film_D' is what the hits D' .. D - 1 add: 4 Le rho^(k + 1) x survival, on the same draws up to hit D' - 1"""
    want = cavity_model(rho, nsets, d_hi)["pixel"] - cavity_model(rho, nsets, d_lo)["pixel"]
    se = np.asarray(SE_INCREMENT[(rho, nsets, d_lo, d_hi)] if se is None else se)
    tol = 4.0 * se + K_MODEL
    assert (tol <= MC_CAP).all(), tol
    ratio = (film_hi - film_lo).reshape(-1, 3).mean(0) / want
    print(f"cavity {rho} sets {nsets} D {d_lo} -> {d_hi}: increment / model {ratio}, tolerance {tol}")
    assert (np.abs(ratio - 1.0) <= tol).all(), (ratio, tol)
    return ratio


class Films:
    """the one-light cavity by (albedo, depth) and, where 256 spp do not do, (albedo, depth, spp): each rendered once, on first use"""

    def __init__(self, render_one):
        self.render_one, self.done = render_one, {}

    def __getitem__(self, key):
        if key not in self.done:
            rho, depth, spp = key if len(key) == 3 else key + (SPP,)
            self.done[key] = self.render_one(I.cavity(RHO[rho]), depth, spp)
        return self.done[key]


@pytest.fixture(scope="module")
def cavity_films(orc):
    return Films(lambda sc, depth, spp: render(orc, sc, depth, spp=spp))


# film_D - film_(D - 1) at (albedo, D - 1, D, spp).  From the third bounce on roulette makes the increment noisy: 1 024 spp, and the grey
# 4 -> 5 (standard error 0.51 % even then: 4 of them exceed the 2 % cap) is left to the coloured cavity
INCREMENTS = [("colour", 1, 2, SPP), ("grey", 1, 2, SPP), ("colour", 2, 3, SPP), ("grey", 2, 3, SPP),
              ("colour", 3, 4, 1024), ("grey", 3, 4, 1024), ("colour", 4, 5, 1024)]


# ---- the model itself ---------------------------------------------------------------------------------------------------------------------
def test_model_reduces_to_the_closed_form_and_the_survival_chain():
    for rho in RHO.values():
        for d in DEPTHS:
            hits = [I.Hit(weight=np.array(rho), emission=np.array(I.LE_CAVITY), direct=np.array(I.LE_CAVITY) * np.array(rho)) for _ in range(d + 1)]
            assert np.allclose(I.chain(hits, d)["pixel"], I.cavity_closed_form(rho, I.LE_CAVITY, d), rtol=1e-13)
    hits = [I.Hit(weight=np.full(3, 0.5)) for _ in range(17)]
    m = I.chain(hits, 16)
    # grey: roulette first sees beta = rho^2 (two bounces sampled), a survivor's beta returns to 1 and the next bounce makes it rho
    assert np.allclose(m["survival"], [0.25] + [0.5] * 12) and np.isclose(m["closest"], 3 + 0.25 * (1 - 0.5 ** 13) / 0.5)
    c = I.chain([I.Hit(weight=np.array(I.RHO_COLOUR)) for _ in range(5)], 4)
    assert abs(float(c["closest"]) - 3.3178) < 5e-5  # 3 + Y(rho^2)
    # q never falls below 0.05: a path that loses nothing still dies 1 time in 20, and a dim one survives with probability Y(beta)
    assert np.allclose(I.chain([I.Hit(weight=np.ones(3)) for _ in range(5)], 4)["survival"], [0.95])
    assert np.allclose(I.chain([I.Hit(weight=np.full(3, 0.1)) for _ in range(5)], 4)["survival"], [0.01])
    # the textbook integrator on the same furnace: Le / (1 - rho) truncated
    t = I.chain([I.Hit(weight=np.full(3, 0.5), emission=np.ones(3)) for _ in range(40)], 39, quirks={"rr_weight", "rr_luminance", "rr_depth_3", "depth_cut_after_increment"})
    assert np.allclose(t["pixel"], 2.0, rtol=1e-9)


def test_cavity_light_sampler_is_unbiased_on_the_icosphere_only_because_its_facets_are_nearly_equal():
    """the reference picks a light's triangle by count and reports 1 / the set's area (uniform_triangle_pick): exact on a sphere, where
    every patch has the form factor area / 4 pi R^2 from everywhere; on the 1 280-facet icosphere the factor is 1 within 1e-3"""
    for nsets in (1, 3):
        sc = I.cavity(nsets=nsets)
        where = I.cavity_wall_points(sc, 64)
        K, spread, own = I.cavity_direct(sc, I.ALL - {"shadow_distance"}, where)
        assert abs(K - 1.0) < 1e-3 and spread < K_SPREAD, (K, spread)
        assert abs(I.cavity_direct(sc, I.ALL - {"uniform_triangle_pick", "shadow_distance"}, where)[0] - 1.0) < 1e-6  # 1e-6: clipped at the horizon
        assert abs(I.cavity_direct(sc, I.ALL - {"uniform_triangle_pick", "shadow_distance", "shadow_offset"}, where)[0] - 1.0) < 1e-12
        # li() squares the shortened distance: + 2e-4 / d on average
        assert 1.5e-4 < I.cavity_direct(sc, True, where)[0] - K < 3e-4
    tri, which = I.cavity_triangles(I.cavity(nsets=3))
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    share = np.array([area[which == k].sum() for k in range(3)]) / area.sum()
    assert 0.2 < share.min() and share.max() < 0.5 and len(set(np.round(share, 2))) == 3, share  # unequal, none tiny


# ---- a / e: one light ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", list(RHO))
@pytest.mark.parametrize("depth", DEPTHS)
def test_a_cavity_film_mean_and_ray_counts(cavity_films, rho, depth):
    film, st = cavity_films[(rho, depth)]
    check_cavity(film, st, rho, 1, depth)


@pytest.mark.parametrize("rho,lo,hi,spp", INCREMENTS)
def test_a_cavity_increment_between_depths(cavity_films, rho, lo, hi, spp):
    check_increment(cavity_films[(rho, hi, spp)][0], cavity_films[(rho, lo, spp)][0], rho, 1, lo, hi)


def test_e_a_wall_seen_directly_carries_its_own_emission_exactly(orc):
    """emission on a material that also has lobes: with rho = 0 the next-event term and every bounce are zero and the pixel is Le, the
    emission of the first hit and of no later one"""
    sc = I.cavity((0.0, 0.0, 0.0))
    for depth in (1, 4):
        film, st = render(orc, sc, depth, spp=4)
        assert (film == np.array(I.LE_CAVITY)).all()
    # and with rho > 0 at depth 1 no pixel is below Le, the next-event term being non-negative
    film, _ = render(orc, I.cavity(I.RHO_GREY), 1, spp=4)
    assert (film >= np.array(I.LE_CAVITY)).all()


# ---- b: several lights --------------------------------------------------------------------------------------------------------------------
MULTI = [("colour", 2, 4), ("colour", 3, 4), ("grey", 2, 8), ("grey", 3, 8)]


@pytest.mark.parametrize("rho,nsets,depth", MULTI)
def test_b_cavity_cut_into_several_lights(orc, cavity_films, rho, nsets, depth):
    sc = I.cavity(RHO[rho], nsets=nsets)
    assert len({m for m, _ in sc.meshes[0].sets}) == nsets
    film, st = render(orc, sc, depth)
    check_cavity(film, st, rho, nsets, depth)
    assert st["rays_closest"] == cavity_films[(rho, depth)][1]["rays_closest"]  # the light samples steer no path


# ---- c: zero variance under a uniform environment -------------------------------------------------------------------------------------------
def jitter_table(orc, spp, seed=SEED):
    """the film jitters of the counter sampler (one per sample index, shared by all pixels): data for the model's camera"""
    out = np.zeros((spp, 2), np.float32)
    assert orc.load().orc_jitter_table(seed, spp, out.ctypes.data_as(abi.f32p)) == 0
    return out.astype(np.float64)


# Zero-variance tolerances: the fp32 operations on the model's path times 2^-24, relative; next to each the oracle's largest deviation as
# measured on the CPU (the tolerance is at most 4 x that).
#   Lambert floor: f = w / pi, the cosine-weighted pdf and f |n.wo| / pdf (4), beta * e (1), the sample's 1 / spp and the sum (3)
#   mirror: besides, the fp32 camera direction in n.wi and the reflected direction's n.wo (4 more)
#   k sheets: the camera direction (4), and per sheet n.wo (5), f |n.wo| / pdf (2), beta's product (1)
TOL_FLOOR = 8 * I.U               # 4.8e-7; measured 1.35e-7
TOL_MIRROR = 12 * I.U             # 7.2e-7; measured 1.96e-7
def TOL_SHEETS(k): return (4 + 8 * k) * I.U  # k = 2: 1.19e-6; measured 8.64e-7
PITCH = 0.9


def check_floor(film, st, jit, depth, spp):
    sc = I.floor_under_environment(scenes.diffuse(*I.RHO_COLOUR), pitch=PITCH)
    hit, cos, sure = I.floor_hits(sc, jit)
    assert hit.all(-1)[sure].sum() >= 64 and (~hit).all(-1)[sure].sum() >= 32 and sure.mean() > 0.8  # floor, sky and few edge pixels
    per_ray = np.where(hit[..., None], (np.array(I.RHO_COLOUR) * np.array(I.ENV) if depth >= 2 else np.zeros(3)), np.array(I.ENV))
    want = per_ray.mean(2)
    err = np.abs(film - want)[sure] / np.array(I.ENV)
    print(f"floor D {depth}: largest deviation {err.max():.2e} of E, tolerance {TOL_FLOOR:.2e}")
    assert err.max() <= TOL_FLOOR
    if depth == 1:
        assert (film[hit.all(-1) & sure] == 0).all()
    assert (film[(~hit).all(-1) & sure] == np.array(I.ENV, np.float32).astype(np.float64)).all()
    # a camera ray each, one more where it met the floor and the depth allows a bounce; no shadow ray: every light sample is masked
    unsure = int((~sure).sum()) * hit.shape[2]
    assert st["rays_shadow"] == 0 and st["rays_masked"] == st["rays_closest"]
    assert abs(st["rays_closest"] - (hit.size + (hit.sum() if depth >= 2 else 0))) <= (unsure if depth >= 2 else 0)


@pytest.mark.parametrize("depth", [1, 2, 5])
def test_c_lambert_floor_under_the_environment(orc, depth):
    """measured: 0 at depth 1, <= 6.6e-7 relative at depth 2 and 5"""
    spp = 64
    film, st = render(orc, I.floor_under_environment(scenes.diffuse(*I.RHO_COLOUR), pitch=PITCH), depth, spp=spp)
    check_floor(film, st, jitter_table(orc, spp), depth, spp)


MIRROR = 0.9


def check_mirror(film, st, jit):
    sc = I.floor_under_environment(scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_REFLECTION, (MIRROR,) * 3)]), pitch=PITCH)
    hit, cos, sure = I.floor_hits(sc, jit)
    m = I.chain([I.Hit(weight=MIRROR * cos[..., None] * np.ones(3), specular=True)], 3, env=np.array(I.ENV))  # the bounce weighs r cos(theta)
    want = np.where(hit[..., None], m["pixel"], np.array(I.ENV)).mean(2)
    err = np.abs(film - want)[sure] / np.array(I.ENV)
    print(f"mirror: largest deviation {err.max():.2e} of E, tolerance {TOL_MIRROR:.2e}")
    assert err.max() <= TOL_MIRROR
    assert st["rays_shadow"] == 0


def test_c_planar_mirror_weighs_the_bounce_by_the_cosine(orc):
    spp = 64
    film, st = render(orc, I.floor_under_environment(scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_REFLECTION, (MIRROR,) * 3)]), pitch=PITCH), 3, spp=spp)
    check_mirror(film, st, jitter_table(orc, spp))


SHEET = (0.8, 0.9, 0.8)
# (sheets k, depth D, spp): black when k >= D.  Roulette plays from the third sheet on and is the only noise: q = 0.31, then 0.16 per sheet,
# so that 16 x 16 x 256 spp leave 0.24 % (k = 3) and 0.5 % (k = 6) of standard error: 1 024 spp for k = 6 and the 2 % cap
SHEET_CASES = [(2, 2, 256), (2, 3, 256), (3, 3, 256), (3, 4, 256), (6, 6, 256), (6, 7, 1024)]
# relative standard errors of the film mean where roulette plays (3 <= k < D), 16 x 16 pixels, seed 5, measured on the CPU oracle
SE_SHEETS = {
    (3, 4): (2.64e-03, 2.64e-03, 2.64e-03),
    (6, 7): (2.46e-03, 2.46e-03, 2.46e-03),
}


def sheets_model(k, depth, jit):
    sc = I.sheets_before_environment(k, scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_TRANSPARENT, SHEET)]))
    d, _ = I.camera_directions(sc.camera, jit)
    shape = d.shape[:-1]
    n = np.tile(np.array([[0, 0, 1]], np.float32), (d[..., 0].size, 1))
    model = bsdf64.Model(sc.materials[0])
    view = (-d).reshape(-1, 3).astype(np.float32)
    wo, f, pdf, fl = model.sample(n, view, np.full((len(n), 2), 0.5, np.float32))
    assert np.allclose(wo, -view.astype(np.float64)) and (fl == abi.BSDF_TRANSMIT).all()  # straight through, not specular
    w = (f * np.abs((wo * n).sum(1))[:, None] / pdf[:, None]).reshape(shape + (3,))
    return sc, I.chain([I.Hit(weight=w) for _ in range(k)], depth, env=np.array(I.ENV))


def check_sheets(film, st, jit, k, depth, se=None):
    sc, m = sheets_model(k, depth, jit)
    n = st["camera_samples"]
    want = m["pixel"].mean(2)
    closest = float(m["closest"].mean())
    assert len(m["survival"]) == max(0, min(k, depth - 1) - 2)  # roulette from the third sheet on
    events = m["reach"][1:] + ([m["miss"]] if k < depth else [])
    if k >= depth:  # the depth cut comes before the last sheet's bounce: black
        assert (film == 0).all() and abs(st["rays_closest"] / n - closest) <= count_tolerance(events, n) and st["rays_masked"] == 0
        return
    if not m["survival"]:
        err = (np.abs(film - want) / want).max()
        print(f"sheets {k} D {depth}: largest deviation {err:.2e}, tolerance {TOL_SHEETS(k):.2e}")
        assert err <= TOL_SHEETS(k) and st["rays_closest"] == n * (k + 1) and st["rays_masked"] == n
        return
    se = np.asarray(SE_SHEETS[(k, depth)] if se is None else se)
    assert (4.0 * se <= MC_CAP).all()
    ratio = (film / want).reshape(-1, 3).mean(0)  # the expectation differs from pixel to pixel (the view's cosine on the sheets)
    print(f"sheets {k} D {depth}: mean / model {ratio}, tolerance {4 * se}, rays {st['rays_closest'] / n:.5f} model {closest:.5f}")
    assert (np.abs(ratio - 1.0) <= 4.0 * se).all(), (ratio, se)
    assert abs(st["rays_closest"] / n - closest) <= count_tolerance(events, n)
    # the lamp behind the camera faces every sheet: each hit's light sample is traced (and finds nothing to shade: a delta lobe has f = 0)
    assert st["rays_shadow"] == st["rays_closest"] - round(st["rays_masked"]) and abs(st["rays_masked"] / n - float(m["masked"].mean())) <= count_tolerance([m["miss"]], n)


@pytest.mark.parametrize("k,depth,spp", SHEET_CASES)
def test_c_transparent_sheets_before_the_environment(orc, k, depth, spp):
    film, st = render(orc, I.sheets_before_environment(k, scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_TRANSPARENT, SHEET)])), depth, spp=spp)
    check_sheets(film, st, jitter_table(orc, spp), k, depth)


# ---- d: one-lobe floors -------------------------------------------------------------------------------------------------------------------
def lobe_materials():
    z = scenes.closure_zoo()
    return {"oren_nayar": z[1], "ggx": z[4], "sheen": z[6]}


# relative standard errors (r, g, b) of the mean over the floor pixels of film / model, 16 x 16 pixels x LOBE_SPP, seed 5, measured on the CPU oracle
SE_LOBES = {
    "oren_nayar": (3.50e-07, 3.58e-07, 3.56e-07),
    "ggx": (3.41e-03, 3.41e-03, 3.41e-03),
    "sheen": (2.93e-03, 2.93e-03, 2.93e-03),
}
_weights = {}
# E[f cos / pdf] by the midpoint rule on grid x grid sampler inputs, at `count` view cosines; between them a polynomial fit of `degree` or
# linear interpolation.  GGX's sampler rejects 12 - 16 % of its draws along a curve in the unit square, which the rule resolves like
# 1 / grid (384 against 256: 0.15 - 0.26 %, against 512: 0.07 %); the cosine-weighted lobes have smooth integrands (96 against 64: < 0.1 %)
# but the sheen's weight falls from 0.11 to 0.02 between 70 degrees and the normal: many nodes.
QUAD = {"oren_nayar": (17, 96, None), "ggx": (9, 384, 6), "sheen": (65, 96, None)}
QUAD_TOL = 4e-3  # the interpolant against a coarser rule between the nodes (asserted); half of it is allowed for the model's weight


def lobe_floor_model(name, jit):
    """-> (scene, expected film (H, W, 3), mask of the pixels whose rays all meet the floor away from its edge, rays per sample)"""
    mat = lobe_materials()[name]
    sc = I.floor_under_environment(mat, pitch=0.5)
    hit, cos, sure = I.floor_hits(sc, jit)
    if name not in _weights:  # a smooth function of the view's cosine: tabulated, then interpolated
        count, fine, degree = QUAD[name]
        nodes = np.linspace(cos[hit].min() - 0.01, 1.0, count)
        model = bsdf64.Model(mat, bsdf64.sheen_L5_of(sc.materials))
        w, live = I.lobe_weight(model, nodes, grid=fine)
        table = np.concatenate([w, live[:, None]], 1)
        if degree:
            fit = [np.polyfit(nodes, y, degree) for y in table.T]
            at = lambda c: np.stack([np.polyval(f, c) for f in fit], -1)
        else:
            at = lambda c: np.stack([np.interp(c, nodes, y) for y in table.T], -1)
        between = 0.5 * (nodes[:-1] + nodes[1:])[[0, count // 2, -1]]  # checked between the nodes, on a coarser rule
        w2, live2 = I.lobe_weight(model, between, grid=fine * 2 // 3)
        err = np.abs(at(between) / np.concatenate([w2, live2[:, None]], 1) - 1).max()
        assert err < QUAD_TOL, (name, err)
        _weights[name] = at
    table = _weights[name](cos)
    wr, lv = table[..., :3], table[..., 3]
    m = I.chain([I.Hit(weight=wr, live=lv)], 2, env=np.array(I.ENV))
    want = np.where(hit[..., None], m["pixel"], np.array(I.ENV)).mean(2)
    return sc, want, hit.all(-1) & sure, float(np.where(hit, m["closest"], 1.0).mean())


def check_lobe_floor(film, st, jit, name, se=None):
    sc, want, on_floor, closest = lobe_floor_model(name, jit)
    assert on_floor.sum() >= 100
    se = np.asarray(SE_LOBES[name] if se is None else se)
    assert (4.0 * se <= MC_CAP).all()
    ratio = (film[on_floor] / want[on_floor]).mean(0)
    print(f"{name} floor: mean of film / model {ratio}, tolerance {4 * se}, rays {st['rays_closest'] / st['camera_samples']:.5f} model {closest:.5f}")
    assert (np.abs(ratio - 1.0) <= 4.0 * se + QUAD_TOL / 2).all(), (ratio, se)
    assert abs(st["rays_closest"] / st["camera_samples"] - closest) <= 4.0 * math.sqrt(0.25 / st["camera_samples"]) + QUAD_TOL / 2
    assert st["rays_shadow"] == 0


LOBE_SPP = {"oren_nayar": 256, "ggx": 256, "sheen": 1024}  # the sheen's weight is the noisiest: 0.6 % of standard error at 256 spp


@pytest.mark.parametrize("name", list(lobe_materials()))
def test_d_one_lobe_floor_under_the_environment(orc, name):
    film, st = render(orc, I.floor_under_environment(lobe_materials()[name], pitch=0.5), 2, spp=LOBE_SPP[name])
    check_lobe_floor(film, st, jitter_table(orc, LOBE_SPP[name]), name)
