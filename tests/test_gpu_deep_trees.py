"""k_trace's stack layouts on trees deep enough to use them (trace.hip: trace_plan / launch_trace).  A lane's stack of pending sibling
groups lives in one of three layouts:

- every level in LDS, 8-byte entries (k_trace<256 / 512 / 1024>): trees of < 10 stack levels;
- SPILL + PACKED (k_trace<1024, true, true>): the top PHX_SPILL_LDS_LEVELS = 7 levels in LDS as 5-byte entries, the deeper ones in HBM
  (sc.stack_spill): >= 10 levels, pools of < 2^24 elements;
- SPILL with 8-byte entries (k_trace<1024, true, false>): >= 10 levels, pools of >= 2^24 elements — here through the twin library
  libphx_hip_nopack.so (-DPHX_STACK_PACKED=0, __graft_entry__.build), whose every SPILL plan launches it.

The ordinary scenes rarely push below level 5, so a wrong HBM offset would change a handful of rays.  scenes.deep_comb is a chain: its rays
walk 14 stack levels (tests/test_host_bvh8.py), and the instrumented twin (libphx_hip_count.so) shows the pushes that land in HBM.  Knob runs
(PHX_LDS_LEVELS, PHX_NTOP: read once per process) go to child processes: this file run as a script renders a list of scenes and prints one
JSON line per scene."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits_equal

pytestmark = pytest.mark.gpu

SPILL_LDS_LEVELS = 7  # trace.hip: PHX_SPILL_LDS_LEVELS
SPILL_FROM_LEVELS = 10  # trace.hip: PHX_SPILL_FROM_LEVELS
COMB_SPP, DEPTH, SEED = 16, 9, 3
LIBDIR = os.path.join(ROOT, "phosphorus_mk2_amd")
COUNT_LIB, NOPACK_LIB = os.path.join(LIBDIR, "libphx_hip_count.so"), os.path.join(LIBDIR, "libphx_hip_nopack.so")


def _scene(key):
    """-> (scene, render keyword arguments) of the scenes the knob runs render"""
    from phosphorus_mk2_amd import scenes
    if key == "comb":        # the host builder's chain: 15 stack levels, 8 of them in HBM under the default plan
        return scenes.deep_comb(), dict(spp=COMB_SPP, bvh_builder="host")
    if key == "cornell":
        return scenes.cornell(64, 64), dict(spp=4)
    if key == "soup":
        return scenes.soup(20000, width=96, height=64), dict(spp=4)
    if key == "zoo":         # 16 closure recipes: k_shade_g
        return scenes.multi_material_soup(3000, width=96, height=64), dict(spp=4)
    if key == "room":        # the closed showroom: a deep tree (SPILL plan) of ordinary meshes
        return scenes.showroom(20000, width=96, height=64, closed=True), dict(spp=4)
    raise KeyError(key)


SWEEP_SCENES = ("comb", "cornell", "soup", "zoo", "room")
PLAN_KEYS = ("bvh_depth", "bvh_bytes", "trace_block", "trace_ntop", "trace_levels", "trace_lds_levels", "trace_stack_packed", "instrumented")
COUNT_KEYS = ("camera_samples", "rays_closest", "rays_shadow", "rays_masked")


def _render_child(keys):
    """(child process) render the scenes `keys` with whatever library PHX_LIB names and whatever knobs the environment sets"""
    from phosphorus_mk2_amd import xpu
    for key in keys:
        sc, kw = _scene(key)
        film, st = xpu.render(sc, depth=DEPTH, seed=SEED, **kw)
        out = {"scene": key, "sha1": hashlib.sha1(film.tobytes()).hexdigest(), "stack_pushes": st["stack_pushes"]}
        out.update({k: st[k] for k in PLAN_KEYS + COUNT_KEYS})
        print("R " + json.dumps(out), flush=True)


def _run(keys, lib=None, **knobs):
    """render `keys` in a child process (PHX_LIB = lib, knobs in its environment) -> {scene: record}"""
    env = {k: v for k, v in os.environ.items() if k not in ("PHX_LIB", "PHX_LDS_LEVELS", "PHX_NTOP", "PHX_TRACE_BLOCK")}
    if lib:
        env["PHX_LIB"] = lib
    env.update({k: str(v) for k, v in knobs.items()})
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(keys), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (lib, knobs, r.stdout[-1000:], r.stderr[-2000:])
    recs = [json.loads(l[2:]) for l in r.stdout.splitlines() if l.startswith("R ")]
    assert [x["scene"] for x in recs] == list(keys), r.stdout[-1000:]
    return {x["scene"]: x for x in recs}


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


def _comb_oracle(orc, material=None):
    """the oracle's film of scenes.deep_comb(material=material) (device tie rule, counter RNG) and its stats"""
    from phosphorus_mk2_amd import scenes
    sc = scenes.deep_comb(material=material)
    orc.set_tie_rule(1)
    try:
        ref, ost = orc.Oracle(sc, spp=COMB_SPP, pps=1, depth=DEPTH).render(rng=orc.RNG_COUNTER, seed=SEED, threads=8)
    finally:
        orc.set_tie_rule(0)
    # lit content and shadow rays: the comparison is not black against black
    assert np.isfinite(ref).all() and (ref[..., :3].sum(-1) > 0).mean() > 0.5
    assert ost["rays_shadow"] > 0.5 * ost["camera_samples"] and ost["rays_closest"] > ost["camera_samples"]
    return ref, ost


@pytest.fixture(scope="module")
def comb_oracle(orc):
    return _comb_oracle(orc)


@pytest.fixture(scope="module")
def default_runs():
    """the product library in a child process without knobs: the films every knob and twin run must reproduce"""
    return _run(SWEEP_SCENES)


@pytest.mark.parametrize("builder", ["host", "device"])
def test_deep_comb_plan_and_stage_hook(xpu, orc, builder):
    """the plan the comb's tree gets (host builder: 15 stack levels, 7 of them in LDS as 5-byte entries, 1024-thread workgroups; device
    builder: whatever its depth implies), and phx_dev_trace (k_trace_rays, an LDS stack of depth levels) on rays that walk down the chain:
    closest and any hits bit-equal to the oracle's brute force"""
    from phosphorus_mk2_amd import scenes
    sc = scenes.deep_comb()
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=COMB_SPP, paths_per_sample=1, path_depth=DEPTH, bvh_builder=builder))
    try:
        dev.preprocess(sc)
        st = dev.stats()
        print(f"\n[comb/{builder}] depth {st['bvh_depth']}, {st['bvh_nodes']} nodes; k_trace plan: block {st['trace_block']}, {st['trace_ntop']} "
              f"elements in LDS, {st['trace_levels']} stack levels ({st['trace_lds_levels']} in LDS, packed {st['trace_stack_packed']})")
        assert st["bvh_built_on_device"] == (1 if builder == "device" else 0)
        levels = max(2, st["bvh_depth"] - 1)
        assert st["trace_levels"] == levels
        if builder == "host":
            assert st["bvh_depth"] >= 14
            assert (st["trace_lds_levels"], st["trace_stack_packed"], st["trace_block"]) == (SPILL_LDS_LEVELS, 1, 1024)
        elif levels >= SPILL_FROM_LEVELS:
            assert (st["trace_lds_levels"], st["trace_stack_packed"], st["trace_block"]) == (SPILL_LDS_LEVELS, 1, 1024)
        else:
            assert (st["trace_lds_levels"], st["trace_stack_packed"]) == (levels, 0)
        o, d, tm = scenes.deep_comb_rays(20000, seed=7)
        tm2 = (o[:, 0] * np.float32(0.08) * np.random.default_rng(8).uniform(0.0, 2.0, len(o)).astype(np.float32)).astype(np.float32)
        g = dev.trace(o, d, tm)
        gs = dev.trace(o, d, tm2, shadow=True)
    finally:
        dev.close()
    orc.set_tie_rule(1)
    try:
        O = orc.Oracle(sc, spp=1)
        r = O.trace(o, d, tm, brute=True)
        rs = O.trace(o, d, tm2, shadow=True, brute=True)
    finally:
        orc.set_tie_rule(0)
    assert g["hit"].mean() > 0.99
    assert np.array_equal(g["prim"], r["prim"]) and bits_equal(g["t"], r["t"]) and bits_equal(g["u"], r["u"]) and bits_equal(g["v"], r["v"])
    assert np.array_equal(gs["hit"], rs["hit"]) and 0.2 < gs["hit"].mean() < 0.8


@pytest.mark.parametrize("material", ["glass", "diffuse"])
def test_deep_comb_films_match_the_oracle(xpu, orc, comb_oracle, material):
    """the comb's film, through k_trace's SPILL + PACKED plan (host builder) and whatever plan the device builder's tree gets, in one pass
    and in passes of 4 samples: every pixel and every ray count is the oracle's; the two builders' films are the same film.  The glass
    comb's refracted rays carry on down the chain (k_trace); the diffuse comb's camera rays stop at its first triangle and bounce back, so
    its deep walks are k_trace_primary's."""
    from phosphorus_mk2_amd import scenes
    mat = None if material == "glass" else scenes.diffuse(0.73, 0.73, 0.73)
    ref, ost = comb_oracle if mat is None else _comb_oracle(orc, mat)
    films = {}
    for builder in ("host", "device"):
        for sif in (0, 4):
            film, st = xpu.render(scenes.deep_comb(material=mat), spp=COMB_SPP, depth=DEPTH, seed=SEED, samples_in_flight=sif, bvh_builder=builder)
            for k in COUNT_KEYS:
                assert st[k] == ost[k], (builder, sif, k, st[k], ost[k])
            assert bits_equal(film[..., :3], ref[..., :3]), (builder, sif)
            films[builder, sif] = film
    assert all(bits_equal(f, films["host", 0]) for f in films.values())


def test_count_twin_pushes_land_in_the_spilled_levels(xpu, default_runs, comb_oracle):
    """proof that the comb's frame runs the HBM levels: the instrumented twin counts k_trace's pushes by the stack index they land at
    (stack_pushes[7] = index 7 and deeper: HBM under the default plan) and renders the product library's film"""
    w = _run(["comb"], lib=COUNT_LIB)["comb"]
    d = default_runs["comb"]
    print(f"\n[count twin, comb] stack pushes by index {w['stack_pushes']}, plan {[w[k] for k in PLAN_KEYS]}")
    assert w["instrumented"] == 1 and d["instrumented"] == 0
    assert (w["trace_lds_levels"], w["trace_stack_packed"]) == (SPILL_LDS_LEVELS, 1) and w["trace_levels"] > SPILL_LDS_LEVELS
    assert w["stack_pushes"][SPILL_LDS_LEVELS] > 0
    assert w["sha1"] == d["sha1"] and all(w[k] == d[k] for k in COUNT_KEYS)
    assert d["rays_closest"] == comb_oracle[1]["rays_closest"]


def test_count_twin_pushes_to_hbm_on_an_ordinary_tree(default_runs):
    """PHX_LDS_LEVELS=2 on Soup(20 000): two stack levels in LDS, every deeper push in HBM — and there are such pushes"""
    w = _run(["soup"], lib=COUNT_LIB, PHX_LDS_LEVELS=2)["soup"]
    d = default_runs["soup"]
    print(f"\n[count twin, soup, PHX_LDS_LEVELS=2] stack pushes by index {w['stack_pushes']}, plan {[w[k] for k in PLAN_KEYS]}")
    assert (w["trace_lds_levels"], w["trace_stack_packed"], w["trace_block"]) == (2, 1, 1024) and w["trace_levels"] > 2
    assert sum(w["stack_pushes"][2:]) > 0
    assert w["sha1"] == d["sha1"] and all(w[k] == d[k] for k in COUNT_KEYS)


@pytest.mark.parametrize("knob,value", [("PHX_LDS_LEVELS", v) for v in (2, 3, 5, 7, 64)] + [("PHX_NTOP", v) for v in (1, 9, 64)])
def test_trace_knobs_render_the_same_films(xpu, orc, default_runs, knob, value):
    """PHX_LDS_LEVELS moves the split between the stack levels in LDS and in HBM (64: every level in LDS), PHX_NTOP the split between
    nodelets staged in LDS and read from the pool: the reported plan follows the knob, and every film and ray count is the default run's"""
    runs = _run(SWEEP_SCENES, **{knob: value})
    for key in SWEEP_SCENES:
        r, d = runs[key], default_runs[key]
        assert r["sha1"] == d["sha1"] and all(r[k] == d[k] for k in COUNT_KEYS), (key, r, d)
        assert (r["bvh_depth"], r["trace_levels"]) == (d["bvh_depth"], d["trace_levels"])
        levels = r["trace_levels"]
        if knob == "PHX_LDS_LEVELS":
            assert r["trace_lds_levels"] == max(2, min(value, levels)), (key, r)
            assert r["trace_ntop"] >= 9 or r["trace_ntop"] == r["bvh_bytes"] // 64
        else:
            assert r["trace_lds_levels"] == d["trace_lds_levels"] and r["trace_ntop"] == min(value, r["bvh_bytes"] // 64), (key, r)
        spill = r["trace_lds_levels"] < levels
        assert r["trace_stack_packed"] == (1 if spill else 0), (key, r)
        if spill:
            assert r["trace_block"] == 1024
    assert runs["comb"]["trace_levels"] >= 13


def test_default_films_match_the_oracle(xpu, orc, default_runs, comb_oracle):
    """the default run's comb and Cornell films are the oracle's (so every knob and twin run that reproduces them is too), and this
    process renders the same films"""
    for key in ("comb", "cornell"):
        sc, kw = _scene(key)
        film, st = xpu.render(sc, depth=DEPTH, seed=SEED, **kw)
        assert hashlib.sha1(film.tobytes()).hexdigest() == default_runs[key]["sha1"], key
        if key == "comb":
            ref, ost = comb_oracle
        else:
            orc.set_tie_rule(1)
            try:
                ref, ost = orc.Oracle(sc, spp=kw["spp"], pps=1, depth=DEPTH).render(rng=orc.RNG_COUNTER, seed=SEED, threads=8)
            finally:
                orc.set_tie_rule(0)
        assert bits_equal(film[..., :3], ref[..., :3]) and all(st[k] == ost[k] for k in COUNT_KEYS), key


def test_unpacked_spill_kernel_renders_the_same_films(default_runs):
    """k_trace<1024, true, false> — the SPILL kernel with 8-byte entries, which the product launches for pools of >= 2^24 elements — through
    the twin built with PHX_STACK_PACKED=0: the comb under the default plan (8 levels in HBM) and Soup(20 000) with PHX_LDS_LEVELS=3"""
    assert os.path.exists(NOPACK_LIB), "build() makes the unpacked-stack twin"
    c = _run(["comb"], lib=NOPACK_LIB)["comb"]
    s = _run(["soup"], lib=NOPACK_LIB, PHX_LDS_LEVELS=3)["soup"]
    print(f"\n[nopack twin] comb plan {[c[k] for k in PLAN_KEYS]}, soup (PHX_LDS_LEVELS=3) plan {[s[k] for k in PLAN_KEYS]}")
    assert c["trace_stack_packed"] == 0 and c["trace_lds_levels"] == SPILL_LDS_LEVELS < c["trace_levels"] and c["trace_block"] == 1024
    assert s["trace_stack_packed"] == 0 and s["trace_lds_levels"] == 3 < s["trace_levels"] and s["trace_block"] == 1024
    for r, key in ((c, "comb"), (s, "soup")):
        d = default_runs[key]
        assert r["sha1"] == d["sha1"] and all(r[k] == d[k] for k in COUNT_KEYS), (key, r, d)


if __name__ == "__main__":
    _render_child(sys.argv[1:])
