"""Frames of odd shapes and over caller-made tile lists (the cases of frame_cases.py): films whose width is no multiple of 8 against the
oracle's strips bit for bit, films smaller than a wave, a k_film block or the queue's eight segments, and tile lists that are not the
32-pixel grid -- through run_frame's Morton sort, its pixel-table cache and k_trace_primary's packets over rows a few pixels wide.
Every frame renders into an add_tile film and a device film at once, both prefilled with a sentinel."""
import numpy as np
import pytest

import frame_cases as F
import integrator64 as I
from phosphorus_mk2_amd import scenes

pytestmark = pytest.mark.gpu

GGX = scenes.closure_zoo()[4]


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


def device(xpu, sc, spp, flight=0, tpb=0, depth=F.DEPTH):
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=spp, paths_per_sample=1, path_depth=depth, samples_in_flight=flight, tiles_per_batch=tpb))
    dev.preprocess(sc)
    return dev


def both_sinks(xpu, dev, sc, tiles=None, seed=F.SEED, normals=False):
    """a frame into an add_tile film and a device film, which must agree -> (film, stats)"""
    host, dev_film, st = F.frame(xpu, dev, sc, seed, tiles=tiles, host="add_tile", device=True, normals=normals)
    assert F.same_bits(host, dev_film)
    return host, st


def rays(st):
    return {k: st[k] for k in F.RAY_KEYS}


# ---- odd films against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flight", [0, 2])
@pytest.mark.parametrize("scene,w,h,spp", F.ODD_FILMS + F.TINY_ORACLE_FILMS)
def test_odd_film_matches_the_oracle_strips(xpu, orc, scene, w, h, spp, flight):
    """17 x 13, 67 x 5, 100 x 3 (and 8 x 1): one partial tile, or a row of them, whose widths are no multiple of 8; 1, 5 and 17 samples
    per pixel put packets of 64 / 128 / 256 camera rays across pixels and tile rows.  The default 32-pixel grid gives the oracle's film;
    the oracle's own strip list (overlapped columns rendered twice) gives it too, and counts the oracle's rays."""
    ref, _, ocounts = F.oracle_case(orc, scene, w, h, spp)
    sc = F.SCENES[scene](w, h)
    dev = device(xpu, sc, spp, flight)
    try:
        film, st = both_sinks(xpu, dev, sc)
        assert F.same_bits(film[..., :3], ref[..., :3]) and (film[..., 3] == 0).all()
        assert st["camera_samples"] == w * h * spp and st["primary_launches"] == (1 if not flight else -(-spp // flight))
        strips = F.strip_tiles(w, h)
        film2, st2 = both_sinks(xpu, dev, sc, tiles=strips)
        assert F.same_bits(film2, film)
        assert rays(st2) == ocounts and st2["tiles"] == len(strips)
        if w % 8 == 0:
            assert rays(st) == ocounts
    finally:
        dev.close()


def test_odd_film_normals_match_the_oracle_strips(xpu, orc):
    ref, nref, _ = F.oracle_case(orc, "soup", 17, 13, 5, normals=True)
    sc = F.soup(17, 13)
    dev = device(xpu, sc, 5)
    try:
        film, _ = both_sinks(xpu, dev, sc, normals=True)
        assert film.shape == (13, 17, 7) and F.same_bits(film[..., :3], ref[..., :3]) and F.same_bits(film[..., 4:], nref)
        assert nref.any() and not nref.any(-1).all()  # hits and misses
    finally:
        dev.close()


# ---- films below 8 pixels wide, and tiny ones --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", F.TINY_SPPS)
@pytest.mark.parametrize("w,h", F.TINY_FILMS)
def test_tiny_film_of_the_black_cavity_is_its_emission(xpu, w, h, spp):
    """fewer paths than a wave, than k_film's 64 pixels, than the queue's 8 segments: black walls that emit LE_CAVITY give exactly that in
    every pixel (as test_wall_emission_is_exact on 16 x 16), on the Lambert kernel and on the general one"""
    for hidden, general in ((None, 0), (GGX, 1)):
        sc = I.cavity((0.0, 0.0, 0.0), width=w, height=h, hidden=hidden)
        dev = device(xpu, sc, spp)
        try:
            film, st = both_sinks(xpu, dev, sc)
            assert film.shape == (h, w, 4) and st["shade_general"] == general and st["camera_samples"] == w * h * spp
            assert (film[..., :3] == np.array(I.LE_CAVITY, np.float32)).all() and (film[..., 3] == 0).all()
        finally:
            dev.close()


@pytest.mark.parametrize("spp", F.TINY_SPPS)
@pytest.mark.parametrize("w,h", F.TINY_FILMS)
def test_tiny_film_of_the_coloured_cavity_is_the_same_under_every_tiling(xpu, w, h, spp):
    sc = I.cavity(width=w, height=h)
    dev, dev2 = device(xpu, sc, spp, depth=5), device(xpu, sc, spp, tpb=2, depth=5)
    try:
        full, st = both_sinks(xpu, dev, sc)
        assert np.isfinite(full).all() and st["camera_samples"] == w * h * spp and st["tiles"] == len(F.default_tiles(xpu, w, h))
        assert (full[..., :3] >= np.array(I.LE_CAVITY, np.float32)).all()  # every camera ray meets the emitting wall
        for name, make in F.TILINGS.items():
            tiles, cover = make(w, h)
            for d in (dev, dev2):
                film, st2 = both_sinks(xpu, d, sc, tiles=tiles)
                F.check_cover(film, full, cover)
                assert st2["tiles"] == len(tiles) and st2["camera_samples"] == int(cover.sum()) * spp, name
                if (cover == 1).all():
                    assert rays(st2) == rays(st), name
    finally:
        dev.close(); dev2.close()


# ---- caller-made tile lists -----------------------------------------------------------------------------------------------------------------
SPP = 5


@pytest.fixture(scope="module")
def tiling_rig(xpu, orc):
    """per film of TILING_FILMS: the scene, a device, one with tiles_per_batch = 2, and the default 32-grid frame, checked against the oracle"""
    rigs = {}
    for (scene, w, h) in F.TILING_FILMS:
        sc = F.SCENES[scene](w, h)
        dev, dev2 = device(xpu, sc, SPP), device(xpu, sc, SPP, tpb=2)
        full, st = both_sinks(xpu, dev, sc)
        ref, _, ocounts = F.oracle_case(orc, scene, w, h, SPP)
        assert F.same_bits(full[..., :3], ref[..., :3]) and ocounts["rays_shadow"] > 0
        assert w % 8 or rays(st) == ocounts
        full.setflags(write=False)
        rigs[(scene, w, h)] = (sc, dev, dev2, full, st)
    yield rigs
    for (_, dev, dev2, _, _) in rigs.values():
        dev.close(); dev2.close()


@pytest.mark.parametrize("tpb", [0, 2])
@pytest.mark.parametrize("name", list(F.TILINGS))
@pytest.mark.parametrize("film", F.TILING_FILMS)
def test_tile_lists_render_the_default_film(xpu, tiling_rig, film, name, tpb):
    sc, dev, dev2, full, st_full = tiling_rig[film]
    d = dev2 if tpb else dev
    _, w, h = film
    tiles, cover = F.TILINGS[name](w, h)
    got, st = both_sinks(xpu, d, sc, tiles=tiles)
    F.check_cover(got, full, cover)
    assert st["tiles"] == len(tiles) and st["camera_samples"] == int(cover.sum()) * SPP
    if (cover == 1).all():
        assert rays(st) == rays(st_full)
    else:
        # rays add up over pixels: the list's count and that of a list which holds what this one has too much (too little) of a full cover
        if name == "covered_twice":
            rest = [t for t in tiles if t not in F.grid(w, h, 5, 3)]
            assert np.array_equal(F.paint(rest, w, h), cover - 1)
        else:
            rest = [t for t in F.grid(w, h, 5, 3) if t not in tiles]
            assert np.array_equal(F.paint(rest, w, h), 1 - cover)
        _, st_rest = both_sinks(xpu, d, sc, tiles=rest)
        sign = 1 if name == "covered_twice" else -1
        assert {k: st[k] - sign * st_rest[k] for k in F.RAY_KEYS} == rays(st_full)
        assert st_rest["rays_shadow"] > 0


@pytest.mark.parametrize("tpb", [0, 2])
@pytest.mark.parametrize("film", F.TILING_FILMS)
def test_one_device_renders_list_a_then_b_then_a(xpu, tiling_rig, film, tpb):
    """B has A's number of tiles and A's sizes at other positions: the pixel table kept from the previous batch must not be taken for it"""
    sc, dev, dev2, full, _ = tiling_rig[film]
    d = dev2 if tpb else dev
    _, w, h = film
    (A, ca), (B, cb) = F.shifted_pair(w, h)
    for tiles, cover in ((A, ca), (B, cb), (A, ca), (A, ca), (B, cb)):
        got, st = both_sinks(xpu, d, sc, tiles=tiles)
        F.check_cover(got, full, cover)
        assert st["tiles"] == len(tiles)
    got, _ = both_sinks(xpu, d, sc)
    assert F.same_bits(got, full)
