"""The hit record as two streams (kernels.h: PassBuffers::hit_tt / hit_uv).  Every closest-hit trace writes (t, triangle), 8 bytes; the
barycentrics (u, v) are a second 8-byte stream that exists only while the committed scene reads them: a smooth face, a UV consumer (lobe
images, masks, emitter images) or a per-hit material (scene_commit.cpp: commit_scene).  k_trace<.., UV> and k_trace_primary<.., UV> are picked by
the stream's presence.

Each case here is rendered on a scene that takes one of the two paths and compared bit for bit, film and ray counts, with the CPU oracle
under the device's tie rule (of two triangles met at bitwise the same distance the lower primitive index wins).  WHICH path a frame took is
read off phx_stats::device_bytes, the one place the stream shows without a new field: with PHX_HIT_UV=1 (tests only: it carries the stream
on a scene that does not need it) a flat scene holds exactly 8 bytes per path in flight more, and a scene that already carries the stream
holds not one byte more.  The forced runs go to ONE child process (this file run as a script), since the variable belongs to a process'
environment like every other knob.  No comparison here carries a tolerance."""
import copy
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, DEPTH, SEED = 64, 48, 16, 9, 5
LENS = (0.03, 3.0)  # aperture radius, focal distance (tests/test_gpu_shade_kernels.py's)
COUNT_KEYS = ("camera_samples", "rays_closest", "rays_shadow", "rays_masked")
FAMILY_CASES = ("tex", "mask", "perhit")  # one family each of tests/test_gpu_shade_kernels.py's table
FORCED_SCENES = ("soup", "lens_soup", "one_smooth", "comb") + FAMILY_CASES


def _corner_normals(sc):
    """per-vertex normals of the soup's mesh 0 (unshared vertices: 3 per triangle): every corner gets its face's geometric normal"""
    m = sc.meshes[0]
    v = m.vertices[m.faces].astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return np.repeat(n, 3, axis=0).astype(F)


def _tilted(n, k):
    """three different unit normals for the corners of triangle k, each within the hemisphere of its geometric normal"""
    g = n[3 * k].astype(np.float64)
    a = np.cross(g, (1.0, 0.0, 0.0) if abs(g[0]) < 0.9 else (0.0, 1.0, 0.0)); a /= np.linalg.norm(a)
    b = np.cross(g, a)
    out = [g + 0.6 * a, g - 0.3 * a + 0.5 * b, g - 0.3 * a - 0.5 * b]
    return np.array([x / np.linalg.norm(x) for x in out], F)


def _soup(width=W, height=H):
    from phosphorus_mk2_amd import scenes
    return scenes.soup(500, width=width, height=height)


def _one_smooth(k):
    """soup(500) with ONE smooth triangle, k, whose corner normals differ from each other and from the face's"""
    sc = _soup()
    m = sc.meshes[0]
    m.normals = _corner_normals(sc)
    m.normals[3 * k:3 * k + 3] = _tilted(m.normals, k)
    m.smooth = np.zeros(len(m.faces), np.uint8); m.smooth[k] = 1
    return sc


def _all_smooth(k):
    """the same scene with EVERY face of the soup on the interpolated-normal path: the flat faces carry their geometric normal at all three
    corners, triangle k its tilted ones.  Every hit then reads its barycentrics, on the device and in the oracle alike."""
    sc = _one_smooth(k)
    sc.meshes[0].smooth = np.ones(len(sc.meshes[0].faces), np.uint8)
    return sc


SMOOTH_K = 0  # set by the `smooth_k` fixture before any scene that names it is built; the child process gets it as its first argument


def _scene(key):
    """-> (the device's scene, the oracle's scene, render keyword arguments)"""
    from phosphorus_mk2_amd import scenes
    kw = dict(spp=SPP, pps=1, depth=DEPTH, seed=SEED)
    if key == "soup":
        sc = _soup()
    elif key == "lens_soup":
        from test_gpu_parity import _with_lens
        sc = _with_lens(_soup(), *LENS)
    elif key == "ragged":  # 24 x 13: one partial tile; 16 samples in passes of 3, 3, 3, 3, 3, 1 through the same buffers
        sc = _soup(24, 13)
        kw["samples_in_flight"] = 3
    elif key == "one_smooth":
        sc = _one_smooth(SMOOTH_K)
    elif key == "all_smooth":
        sc = _all_smooth(SMOOTH_K)
    elif key == "comb":  # tests/test_gpu_deep_trees.py's chain with a Lambert material: flat, and a SPILL + PACKED plan under the host builder
        sc = scenes.deep_comb(material=scenes.diffuse(0.73, 0.73, 0.73))
        kw["bvh_builder"] = "host"
    elif key in FAMILY_CASES:
        from test_gpu_shade_kernels import build
        dev_sc, orc_sc = build(key, False)
        return dev_sc, orc_sc, kw
    else:
        raise KeyError(key)
    return sc, copy.deepcopy(sc), kw


def _record(film, st):
    out = {"sha1": hashlib.sha1(np.ascontiguousarray(film).tobytes()).hexdigest()}
    out.update({k: st[k] for k in COUNT_KEYS + ("device_bytes", "paths_in_flight", "bvh_bytes", "shade_kernels")})
    return out


def _render_child(argv):
    """(child process) render the scenes named on the command line, under whatever the environment sets"""
    global SMOOTH_K
    from phosphorus_mk2_amd import xpu
    SMOOTH_K = int(argv[0])
    for key in argv[1:]:
        sc, _, kw = _scene(key)
        film, st = xpu.render(sc, **kw)
        print("R " + json.dumps(dict(_record(film, st), scene=key)), flush=True)


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


@pytest.fixture(scope="module")
def tie_orc(orc):
    orc.set_tie_rule(1)
    yield orc
    orc.set_tie_rule(0)


@pytest.fixture(scope="module")
def smooth_k(tie_orc):
    """the smooth triangle: the soup triangle that the most camera rays of the film's centre meet first (the oracle's brute-force trace), so
    that its normals reach the film"""
    global SMOOTH_K
    sc = _soup()
    O = tie_orc.Oracle(sc, spp=1)
    o, d = O.camera_rays((W // 4, H // 4, W // 2, H // 2), 0, seed=SEED)
    r = O.trace(o, d, np.full(len(o), np.finfo(F).max, F), brute=True)
    prim = r["prim"][r["hit"] & (r["prim"] < 500)]
    assert len(prim) > 100
    SMOOTH_K = int(np.bincount(prim).argmax())
    return SMOOTH_K


@pytest.fixture(scope="module")
def films(xpu, tie_orc, smooth_k):
    """(device film, device stats, oracle film, oracle stats) by scene key, each rendered once"""
    done = {}

    def get(key):
        if key not in done:
            sc, osc, kw = _scene(key)
            film, st = xpu.render(sc, **kw)
            ref, ost = tie_orc.Oracle(osc, spp=kw["spp"], pps=1, depth=DEPTH).render(rng=tie_orc.RNG_COUNTER, seed=SEED, threads=8)
            done[key] = (film, st, ref, ost)
        return done[key]
    return get


@pytest.fixture(scope="module")
def forced(smooth_k):
    """FORCED_SCENES under PHX_HIT_UV=1, in one child process -> {scene: record}"""
    env = dict(os.environ, PHX_HIT_UV="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(smooth_k)] + list(FORCED_SCENES), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    recs = [json.loads(l[2:]) for l in r.stdout.splitlines() if l.startswith("R ")]
    assert [x["scene"] for x in recs] == list(FORCED_SCENES), r.stdout[-1000:]
    return {x["scene"]: x for x in recs}


def _check_oracle(key, film, st, ref, ost):
    assert "PHX_HIT_UV" not in os.environ, "the unforced runs of this file need an environment without the test switch"
    assert np.isfinite(film).all() and film[..., :3].max() > 0.05, key
    for k in COUNT_KEYS:
        assert st[k] == ost[k], (key, k, st[k], ost[k])
    assert ost["rays_shadow"] > 0 and ost["rays_closest"] > ost["camera_samples"], key  # not black against black
    diff = (film[..., :3].view(np.uint32) != np.ascontiguousarray(ref[..., :3]).view(np.uint32)).any(-1).mean()
    assert bits_equal(film[..., :3], ref[..., :3]), f"{key}: the film differs from the oracle's in {diff:.1%} of the pixels"


def _uv_bytes(st, forced_rec):
    """bytes the forced run holds more than the unforced one, and the size of one barycentrics stream for the frame's paths in flight"""
    assert forced_rec["paths_in_flight"] == st["paths_in_flight"] > 0
    return forced_rec["device_bytes"] - st["device_bytes"], 8 * st["paths_in_flight"]


@pytest.mark.parametrize("key", ["soup", "lens_soup", "comb"])
def test_flat_scene_takes_the_8_byte_path(films, forced, key):
    """a flat Lambert soup through a pinhole (k_trace_primary<., false, false>), through a lens (k_trace_primary<., true, false>) and the flat
    comb (k_trace<1024, true, true, false>): the oracle's film; no barycentrics stream unless forced; the forced run's film and counts are the same"""
    film, st, ref, ost = films(key)
    _check_oracle(key, film, st, ref, ost)
    if key == "comb":
        assert (st["trace_lds_levels"], st["trace_stack_packed"], st["trace_block"]) == (7, 1, 1024) and st["trace_levels"] > 7
    more, stream = _uv_bytes(st, forced[key])
    assert more == stream, (key, more, stream)
    assert forced[key]["sha1"] == _record(film, st)["sha1"] and all(forced[key][k] == st[k] for k in COUNT_KEYS + ("shade_kernels",)), key


def test_one_smooth_triangle_takes_the_uv_path(films, forced, smooth_k):
    """ONE smooth face in a flat soup: the scene carries the stream (forcing adds nothing), the film is the oracle's and not the flat
    soup's; and the variant with every face on the interpolated-normal path (flat faces carrying their geometric normal at their corners)
    is the oracle's too"""
    film, st, ref, ost = films("one_smooth")
    _check_oracle("one_smooth", film, st, ref, ost)
    more, stream = _uv_bytes(st, forced["one_smooth"])
    assert more == 0 and forced["one_smooth"]["sha1"] == _record(film, st)["sha1"]
    flat = films("soup")[0]
    changed = (film[..., :3].view(np.uint32) != flat[..., :3].view(np.uint32)).any(-1).mean()
    print(f"triangle {smooth_k} smooth: {changed:.1%} of the pixels change")
    assert changed > 0  # (500 triangles leave most of the film empty: the one triangle covers about 1 % of it)
    # against the flat scene the smooth one holds the stream and the normals table (36 bytes per pool element), nothing else
    fst = films("soup")[1]
    assert st["bvh_bytes"] == fst["bvh_bytes"] and st["paths_in_flight"] == fst["paths_in_flight"]
    assert st["device_bytes"] - fst["device_bytes"] == 8 * st["paths_in_flight"] + 36 * (st["bvh_bytes"] // 64)
    film2, st2, ref2, ost2 = films("all_smooth")
    _check_oracle("all_smooth", film2, st2, ref2, ost2)
    assert st2["device_bytes"] == st["device_bytes"]


@pytest.mark.parametrize("key", FAMILY_CASES)
def test_uv_consumers_take_the_uv_path(films, forced, key):
    """a textured lobe, an image mask, a per-hit (glass) material: each carries the stream unforced, and renders the oracle's film of the
    scene with its images baked in"""
    film, st, ref, ost = films(key)
    _check_oracle(key, film, st, ref, ost)
    more, stream = _uv_bytes(st, forced[key])
    assert more == 0, (key, more, stream)
    assert forced[key]["sha1"] == _record(film, st)["sha1"] and forced[key]["shade_kernels"] == st["shade_kernels"]


def test_ragged_film_in_passes_of_three_samples(films):
    """24 x 13 pixels, samples_in_flight = 3: a partial tile, six passes (the last one of a single sample) through the same hit_tt buffer"""
    film, st, ref, ost = films("ragged")
    assert st["paths_in_flight"] == 24 * 13 * 3
    _check_oracle("ragged", film, st, ref, ost)


def test_scene_switch_on_one_device(xpu, films, smooth_k):
    """flat -> smooth -> flat on ONE device object: the stream appears with the scene that reads it and leaves with it, and no film sees a
    record of the scene before"""
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=DEPTH))
    got = []
    try:
        for key in ("soup", "one_smooth", "soup", "all_smooth"):
            sc = _scene(key)[0]
            dev.preprocess(sc)
            film, (st,) = xpu.render_on([dev], sc, seed=SEED)
            got.append((key, film.copy(), st))
    finally:
        dev.close()
    for key, film, st in got:
        _, _, ref, ost = films(key)
        _check_oracle(f"switch/{key}", film, st, ref, ost)
    (_, _, flat), (_, _, smooth), (_, _, flat2), (_, _, smooth2) = got
    assert smooth["device_bytes"] - flat["device_bytes"] == 8 * smooth["paths_in_flight"] + 36 * (smooth["bvh_bytes"] // 64)
    assert flat2["device_bytes"] == flat["device_bytes"] and smooth2["device_bytes"] == smooth["device_bytes"]


if __name__ == "__main__":
    _render_child(sys.argv[1:])
