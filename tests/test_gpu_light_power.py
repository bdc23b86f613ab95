"""Choosing next-event estimation's light by power on the device (PHX_LIGHTS_BY_AREA | PHX_LIGHT_SELECT_BY_POWER: the search over the selection
table in light_pick, shade_common.h, run by k_shade_g and by the two light hooks).  The oracle selects uniformly, so the mode is held to: the
numpy restatement of tests/test_light_power.py, bit for bit, through the hooks; the closed form of direct lighting under seven lamps with the
variance of the power table's estimator (which the uniform selection's film does not have); a black lamp that changes nothing; the oracle's
own films, bit for bit, wherever the scene has ONE light (the table is {1}: all 30 k_shade_g instantiations); dispatch, bytes and refusals."""
import math

import numpy as np
import pytest

from conftest import bits_equal
from phosphorus_mk2_amd import abi, scenes
from test_analytic_direct_light import SPP, W
from test_gpu_light_sampling import COUNTERS, G_CASES, three_lights_scene
from test_gpu_shade_kernels import DEPTH as T_DEPTH, FAMILIES, SEED as T_SEED, SPP as T_SPP, build, expected_kernels
from test_light_power import (BLACK, SEVEN_LAMPS, ZERO_AREA, PowerTable, light_emission_power, lamps_scene, light_sample_power, moments_p, pick_edges,
                              seven_lamp_scene)
from test_light_sampling import LE2, LightTable, edge_draws, rects_mesh, striped_scene, z_scores

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
POWER = dict(light_sampling="area", light_selection="power")
AREA = dict(light_sampling="area")


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


# ---- 1. the hooks are the restatement, bit for bit --------------------------------------------------------------------------------------------
def decades_scene():
    """test_gpu_light_sampling's lights of 1, 2 and 37 triangles (first_tri 0, 1, 3) with emissions three decades apart"""
    sc = three_lights_scene()
    sc.materials[1].emission, sc.materials[2].emission, sc.materials[3].emission = (30.0, 20.0, 10.0), LE2, (0.03, 0.05, 0.02)
    sc.name = "decades"
    return sc


def with_lamp(at, lamp, name):
    """decades_scene with one more lamp (rectangles, emission) as light `at` of the four"""
    sc = decades_scene()
    sc.materials.append(scenes.emitter(*lamp[1]))
    sc.meshes.insert(4 + at, rects_mesh(lamp[0], len(sc.materials) - 1))  # behind the floor's four meshes
    sc.name = name
    return sc


IMG53 = np.random.default_rng(53).uniform(0.0, 2.0, (5, 3, 3)).astype(F)


def textured_lamps_scene():
    """the single triangle without an image, the quad under a non-constant image, the 37 triangles under an all-zero one"""
    sc = decades_scene()
    sc.textures = [scenes.TextureDesc(IMG53, abi.TEX_LINEAR), scenes.TextureDesc(np.zeros((2, 2, 3), F))]
    two = sc.meshes[-2]
    assert [m for m, _ in two.sets] == [2] and len(two.vertices) == 4
    two.uvs = np.array([[0.1, 0.9], [0.2, 0.1], [0.8, 0.3], [0.7, 0.8]], F)
    sc.materials[2].emission_uv_texture, sc.materials[3].emission_uv_texture = 1, 2
    sc.name = "textured_lamps"
    return sc


# name: (scene, the lights that must never be chosen)
HOOK_SCENES = {
    "seven_lamps": (seven_lamp_scene, ()),
    "decades": (decades_scene, ()),
    "black_first": (lambda: with_lamp(0, BLACK, "black_first"), (0,)),
    "black_middle": (lambda: with_lamp(2, BLACK, "black_middle"), (2,)),
    "black_last": (lambda: with_lamp(3, BLACK, "black_last"), (3,)),
    "zero_area": (lambda: with_lamp(1, ZERO_AREA, "zero_area"), (1,)),
    "textured": (textured_lamps_scene, (2,)),
    "one_light": (striped_scene, ()),
}


def hook_draws(t):
    """2^16 random triples; pick at 0, 1 - 2^-24 and every pcdf[l] with its two ulp neighbours; and per light that can be chosen, pick inside
    its interval with lu at every entry of its area CDF and its neighbours"""
    rng = np.random.default_rng(31)
    u3 = [rng.random((1 << 16, 3), dtype=F)]
    pe = pick_edges(t.pcdf)
    u3.append(np.stack([pe, rng.random(len(pe), dtype=F), rng.random(len(pe), dtype=F)], -1))
    for k in range(t.n):
        if t.p[k] == 0:
            continue
        mid = F((D(t.pcdf[k - 1] if k else 0.0) + D(t.pcdf[k])) / 2)
        lu = edge_draws(t.cdf[k])
        u3.append(np.stack([np.full(len(lu), mid), lu, rng.random(len(lu), dtype=F)], -1))
    u3.append(np.array([[0.0, 0.0, 0.0], [1 - 2.0 ** -24, 1 - 2.0 ** -24, 1 - 2.0 ** -24], [1 - 2.0 ** -24, 0.0, 0.5]], F))
    return np.concatenate(u3).astype(F)


def _differing(got, want, n):
    return int((np.asarray(got).reshape(n, -1).view(np.uint32) != np.asarray(want).reshape(n, -1).view(np.uint32)).any(1).sum())


@pytest.mark.parametrize("name", list(HOOK_SCENES))
def test_hooks_are_the_restatement_bit_for_bit(xpu, name):
    make, dead = HOOK_SCENES[name]
    sc = make()
    t = PowerTable(sc)
    assert not t.fallback and [k for k in range(t.n) if t.p[k] == 0] == list(dead)
    u3 = hook_draws(t)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=1, **POWER))
    try:
        dev.preprocess(sc)
        got = dev.light_sample(u3)
        emitted = dev.light_emission(u3)
    finally:
        dev.close()
    want = light_sample_power(t, u3)
    assert set(np.unique(want["light"])) == set(range(t.n)) - set(dead)
    for k in set(range(t.n)) - set(dead):  # every triangle of non-zero area of every light that can be chosen is reached
        assert set(np.unique(want["tri"][want["light"] == k])) == set(np.flatnonzero(t.areas[k] > 0)), k
    failed = [f"{key}: {_differing(got[key], want[key], len(u3))} of {len(u3)} differ" for key in ("light", "tri", "bary", "P", "pdf")
              if not bits_equal(got[key], want[key])]
    want_e = light_emission_power(sc, u3)
    failed += [f"light_emission {key}: {_differing(emitted[key], want_e[key], len(u3))} of {len(u3)} differ" for key in ("st", "e")
               if not bits_equal(emitted[key], want_e[key])]
    assert not failed, "\n".join(failed)
    if name == "textured":
        assert len(np.unique(emitted["e"][want["light"] == 1], axis=0)) > 3 and not emitted["st"][want["light"] == 0].any()  # the image is seen
    if name == "one_light":  # the table of one: the pick by area alone, bit for bit
        dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=1, **AREA))
        try:
            dev.preprocess(sc)
            plain = dev.light_sample(u3)
        finally:
            dev.close()
        assert all(bits_equal(plain[key], got[key]) for key in ("light", "tri", "bary", "P", "pdf"))


# ---- 2. the seven lamps' closed form ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seven_films(xpu):
    sc = seven_lamp_scene()
    return xpu.render(sc, spp=SPP, pps=1, depth=1, seed=3, **POWER), xpu.render(sc, spp=SPP, pps=1, depth=1, seed=3, **AREA)


@pytest.fixture(scope="module")
def seven_models():
    t = PowerTable(seven_lamp_scene())
    mean, m2_power = moments_p(SEVEN_LAMPS, t.p.astype(D))
    _, m2_uniform = moments_p(SEVEN_LAMPS, np.full(7, 1.0 / 7.0))
    return mean, m2_power, m2_uniform


def test_power_selection_meets_the_seven_lamps_closed_form_with_its_own_variance(seven_films, seven_models):
    """4 standard errors of the film mean per channel, 5 of any pixel, the z scores' rms in (0.9, 1.1): test_gpu_light_sampling's bounds (1 024
    pixels), with the variance of test_light_power.moments_p under the table's p.  The film rendered with uniform selection has the same mean
    but seven-fold ... thirteen-fold the variance: against the power model its z scores are far too wide, so the test tells the two apart."""
    (film, st), (film_u, st_u) = seven_films
    mean, m2_power, m2_uniform = seven_models
    assert st["rays_shadow"] == st["rays_closest"] == W * W * SPP == st_u["rays_shadow"] == st_u["rays_closest"]
    assert st["shade_general"] == 1
    z_mean, z_pixel = z_scores(film, mean, m2_power, SPP)
    rms = np.sqrt((z_pixel ** 2).mean())
    print(f"seven lamps, by power: film mean off by {z_mean} standard errors, worst pixel {z_pixel.max():.2f}, rms {rms:.3f}")
    zu_mean, zu_pixel = z_scores(film_u, mean, m2_uniform, SPP)
    zu_power = z_scores(film_u, mean, m2_power, SPP)[1]
    rms_u, rms_up = np.sqrt((zu_pixel ** 2).mean()), np.sqrt((zu_power ** 2).mean())
    print(f"seven lamps, uniform selection: film mean off by {zu_mean} of its own standard errors, worst pixel {zu_pixel.max():.2f}, rms {rms_u:.3f}; "
          f"against the power model rms {rms_up:.3f}")
    assert (z_mean < 4.0).all() and z_pixel.max() < 5.0
    assert 0.9 < rms < 1.1
    assert (zu_mean < 4.0).all()
    assert rms_up > 1.1
    assert not bits_equal(film[..., :3], film_u[..., :3])


# ---- 3. a black lamp changes nothing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last"])
def test_a_black_lamp_changes_nothing_under_power_selection(xpu, seven_films, where):
    (film, st), (film_u, st_u) = seven_films
    sc = seven_lamp_scene(where)
    assert LightTable(sc).n == 8
    got, gst = xpu.render(sc, spp=SPP, pps=1, depth=1, seed=3, **POWER)
    assert bits_equal(got, film) and all(gst[k] == st[k] for k in COUNTERS)
    got_u, ust = xpu.render(sc, spp=SPP, pps=1, depth=1, seed=3, **AREA)
    # uniform selection picks it one time in eight (and sends no shadow ray then: the lamp lies under the floor)
    assert not bits_equal(got_u[..., :3], film_u[..., :3]) and ust["rays_closest"] == st_u["rays_closest"] and ust["rays_shadow"] < st_u["rays_shadow"]


# ---- 4. parity with the oracle where the picks agree ------------------------------------------------------------------------------------------
LEFT_OUT = ()  # no case is left out: glass_blobs (perhit, env_perhit) loses its second lamp and keeps its closures, and with them its family


def one_light(sc):
    """the scene reduced to ONE light of at most two triangles: the first emissive face set cut as test_gpu_light_sampling._cut_lamps_to_pairs
    cuts, every further emissive face set dropped (and its mesh with it, when that was its only set)"""
    kept = False
    for m in sc.meshes:
        sets = []
        for mat, faces in m.sets:
            if sc.materials[mat].is_emitter and len(faces):
                if kept:
                    continue
                kept = True
                faces = faces[:2].copy()
            sets.append((mat, faces))
        m.sets = sets
    sc.meshes = [m for m in sc.meshes if m.sets]
    return sc


def _parity_scenes(name, lens):
    if name == "cornell":
        sc = scenes.cornell(64, 48)
        return sc, sc, abi.SHADE_FAMILY_GENERAL
    if name == "soup1k":
        sc = scenes.soup(1000, width=64, height=48)
        return sc, sc, abi.SHADE_FAMILY_GENERAL
    st, sb = build(name, lens)
    assert st is not sb
    return one_light(st), one_light(sb), FAMILIES[name][0]


PARITY = [("cornell", False), ("soup1k", False)] + [c for c in G_CASES if c not in LEFT_OUT]


def test_parity_cases_cover_every_k_shade_g_instantiation():
    assert len(G_CASES) == 20 and len(LEFT_OUT) <= 2
    union = 0
    for name, lens in PARITY[2:]:
        union |= expected_kernels(FAMILIES[name][0], lens)
    want = sum(1 << b for b in range(abi.SHADE_KERNELS) if b // abi.SHADE_PASSES >= abi.SHADE_FAMILY_GENERAL)
    assert union == want and bin(want).count("1") == 30


@pytest.mark.parametrize("name,lens", PARITY, ids=[f"{n}-{'lens' if l else 'pinhole'}" for n, l in PARITY])
def test_power_selection_is_the_oracle_on_scenes_of_one_light(xpu, orc, name, lens):
    """one light of one triangle or two bit-equal ones: pcdf = {1}, l = 0, lpdf = 1 / area and the area CDF is {1} or {0.5, 1}, so the film
    and the ray counters are the oracle's, bit for bit (lowest-primitive tie rule)"""
    st_scene, sb_scene, family = _parity_scenes(name, lens)
    for s in (st_scene, sb_scene):
        t = LightTable(s)
        assert t.n == 1 and t.equal_pairs_only(), "the case is not reduced to one light of bit-equal triangles"
    film, st = xpu.render(st_scene, spp=T_SPP, pps=1, depth=T_DEPTH, seed=T_SEED, **POWER)
    orc.set_tie_rule(1)
    try:
        ref, ost = orc.Oracle(sb_scene, spp=T_SPP, pps=1, depth=T_DEPTH).render(rng=orc.RNG_COUNTER, seed=T_SEED, threads=8)
    finally:
        orc.set_tie_rule(0)
    failed = [f"{k}: {st[k]}, the oracle's {ost[k]}" for k in COUNTERS if st[k] != ost[k]]
    if st["shade_kernels"] != expected_kernels(family, lens):
        failed.append(f"launched {abi.shade_kernel_names(st['shade_kernels'])}, expected {abi.shade_kernel_names(expected_kernels(family, lens))}")
    if not film[..., :3].max() > 0.05:
        failed.append("the film is dark")
    if not bits_equal(film[..., :3], ref[..., :3]):
        failed.append(f"the film differs from the oracle's in {(film[..., :3].view(np.uint32) != ref[..., :3].view(np.uint32)).any(-1).mean():.1%} of the pixels")
    assert not failed, "\n".join(failed)


# ---- 5. dispatch and bytes ----------------------------------------------------------------------------------------------------------------------
def test_power_selection_runs_the_general_kernels_and_counts_its_table(xpu):
    sc = scenes.cornell(32, 32)  # Lambert only, one lobe per material, one light
    f1, st1 = xpu.render(sc, spp=4, pps=1, depth=9, seed=1, **AREA)
    f2, st2 = xpu.render(sc, spp=4, pps=1, depth=9, seed=1, **POWER)
    assert st2["shade_kernels"] == st1["shade_kernels"] == expected_kernels(abi.SHADE_FAMILY_GENERAL, False) and st2["shade_general"] == 1
    assert st2["device_bytes"] - st1["device_bytes"] == 32 == 32 * math.ceil(4 * 1 / 32)  # one float, padded to one record of the light table
    assert bits_equal(f1, f2) and all(st1[k] == st2[k] for k in COUNTERS)  # one light: the same film
    # nine lights (the seven, a black one at either end): 36 bytes of table in two records
    lamps = [([(-0.5, 0.5, -0.5, 0.5)], (0.0, 0.0, 0.0), 0, -1.0)]
    nine = lamps_scene(lamps + list(SEVEN_LAMPS) + lamps, "nine_lamps")
    assert LightTable(nine).n == 9
    _, n1 = xpu.render(nine, spp=4, pps=1, depth=1, seed=1, **AREA)
    _, n2 = xpu.render(nine, spp=4, pps=1, depth=1, seed=1, **POWER)
    assert n2["device_bytes"] - n1["device_bytes"] == 64 == 32 * math.ceil(4 * 9 / 32) and n1["shade_kernels"] == n2["shade_kernels"]


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", [0x100, 0x201, 0x10101, 2 | 0x100], ids=hex)
def test_every_other_word_is_refused_at_preprocess(xpu, word):
    """test_gpu_light_sampling's refusal sequence: the device answers PHX_ERR_STATE before, PHX_ERR_ARG with a message at preprocess, twice,
    closes, and a device made next renders the film rendered before"""
    good = scenes.cornell(32, 32)
    ref, st = xpu.render(good, spp=4, pps=1, depth=9, seed=1, **POWER)
    assert ref[..., :3].max() > 0.05
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=4, paths_per_sample=1, path_depth=9, light_sampling=word))
    try:
        for _ in range(2):
            with pytest.raises(xpu.DeviceError) as e:
                dev.light_sample(np.zeros((1, 3), F))
            assert "(4)" in str(e.value)  # PHX_ERR_STATE before preprocess
            with pytest.raises(xpu.DeviceError) as e:
                dev.preprocess(good)
            assert "(1)" in str(e.value) and "light_sampling" in str(e.value)  # PHX_ERR_ARG with a message
    finally:
        dev.close()
    again, st2 = xpu.render(good, spp=4, pps=1, depth=9, seed=1, **POWER)
    assert bits_equal(again, ref) and all(st[k] == st2[k] for k in COUNTERS)
