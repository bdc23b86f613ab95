"""The frame tests' own cases, on the CPU oracle alone (frame_cases.py): the strip-by-strip oracle film is self-consistent, every film
that a device test compares with it is lit and traces shadow rays, and every tile list covers the pixels it says it covers."""
import numpy as np
import pytest

import frame_cases as F
from conftest import bits_equal


@pytest.mark.parametrize("scene,w,h,spp", F.ORACLE_CASES)
def test_oracle_cases_trace_shadow_rays_and_have_a_lit_pixel(orc, scene, w, h, spp):
    """(oracle_film_by_strips asserts on the way that the columns two strips share are the same bits)"""
    film, _, counts = F.oracle_case(orc, scene, w, h, spp)
    assert film.shape == (h, w, 4) and np.isfinite(film).all()
    assert counts["rays_shadow"] > 0
    assert (film[..., :3] > 0).any()
    assert counts["camera_samples"] == len(F.strip_positions(w)) * 8 * h * spp


def test_strip_positions_cover_every_column_with_8_wide_tiles_inside_the_film():
    for w in (8, 9, 15, 16, 17, 67, 72, 100):
        xs = F.strip_positions(w)
        cover = F.paint(F.strip_tiles(w, 3), w, 3)
        assert (cover >= 1).all() and (cover <= 2).all() and (cover == 2).sum() == 3 * ((8 - w % 8) % 8)
        assert len(xs) == -(-w // 8) and xs == sorted(xs)


@pytest.mark.parametrize("scene", ["soup", "cornell"])
def test_strips_reproduce_the_default_tiling(orc, scene):
    """where the oracle renders the film by itself (a width that 8 divides, 32-pixel tiles), the strips give the same film and counts"""
    w, h, spp = 72, 40, 5
    film, nrm, counts = F.oracle_film_by_strips(orc, F.SCENES[scene](w, h), spp, F.DEPTH, F.SEED, normals=True)
    orc.set_tie_rule(1)
    try:
        ref, st, nref = orc.Oracle(F.SCENES[scene](w, h), spp=spp, pps=1, depth=F.DEPTH).render(rng=orc.RNG_COUNTER, seed=F.SEED, threads=4, normals=True)
    finally:
        orc.set_tie_rule(0)
    assert bits_equal(film[..., :3], ref[..., :3]) and bits_equal(nrm, nref)
    assert all(counts[k] == st[k] for k in F.RAY_KEYS)


def test_overlapped_strips_agree_with_strips_at_other_positions(orc):
    """17 x 13: the columns of the last strip (9 ... 16) once more from a strip at x = 5, which the helper does not use"""
    film, nrm, _ = F.oracle_film_by_strips(orc, F.soup(17, 13), 5, F.DEPTH, F.SEED, normals=True)
    orc.set_tie_rule(1)
    try:
        f, _, n = orc.Oracle(F.soup(17, 13), spp=5, pps=1, depth=F.DEPTH).render(rng=orc.RNG_COUNTER, seed=F.SEED, tiles=[(5, 0, 8, 13)], normals=True)
    finally:
        orc.set_tie_rule(0)
    assert bits_equal(f[:, 5:13, :3], film[:, 5:13, :3]) and bits_equal(n[:, 5:13], nrm[:, 5:13])
    assert nrm.any()


@pytest.mark.parametrize("w,h", [(72, 40), (17, 13)] + list(F.TINY_FILMS))
@pytest.mark.parametrize("name", list(F.TILINGS))
def test_tile_lists_cover_what_they_claim(name, w, h):
    tiles, claim = F.TILINGS[name](w, h)
    assert claim.shape == (h, w) and np.array_equal(F.paint(tiles, w, h), claim)
    assert all(isinstance(v, int) for t in tiles for v in t)
    assert tiles or (name == "partial" and w * h <= 15)  # a film inside the one tile that the partial list leaves out
    if name == "per_pixel":
        assert len(tiles) == w * h
    if name == "whole":
        assert tiles == [(0, 0, w, h)]
    if name == "covered_twice":
        assert claim.max() == 2 and (claim.min() == 1 or w * h <= 28)
    if name == "partial" and w * h > 15:
        assert claim.min() == 0 and claim.max() == 1
    if name == "ragged_5x3" and (w, h) in ((72, 40), (17, 13)):
        assert {t[2] for t in tiles} == {5, w % 5} and {t[3] for t in tiles} == {3, h % 3}
    if name == "mixed" and (w, h) == (72, 40):
        assert len({(t[2], t[3]) for t in tiles}) > 20
    if name in ("shuffled_strips", "per_pixel", "mixed") and len(tiles) > 8:
        assert tiles != sorted(tiles, key=lambda t: (t[1], t[0]))


@pytest.mark.parametrize("w,h", [(72, 40), (17, 13)])
def test_shifted_pair_differs_in_positions_alone(w, h):
    (A, ca), (B, cb) = F.shifted_pair(w, h)
    assert len(A) == len(B) >= 3 and [t[2:] for t in A] == [t[2:] for t in B]
    assert all((b[0] - a[0], b[1] - a[1]) == (3, 2) for a, b in zip(A, B))
    assert ca.max() == 1 and cb.max() == 1 and ca.sum() == cb.sum() and not np.array_equal(ca, cb)
    assert ((ca == 1) & (cb == 0)).any() and ((cb == 1) & (ca == 0)).any()
