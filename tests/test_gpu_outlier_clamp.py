"""The outlier clamp on the device (phx_dev_film_outlier_clamp, csrc/outlier_clamp.hip), held to the float64 model of
tests/outlier_clamp64.py bit for bit (a NaN matching a NaN): film, m2, samples, every other float and the summary.  Synthetic films
(tests/outlier_clamp_cases.py) over film sizes around the kernel's tile and halo, every radius, trim, flag word, pixel layout and way the
three films can be one another, host and device films; the refusals; then real frames: render_progressive(despeckle=),
render_camera_path(history_clamp=) and the plain-C example."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import accumulate64 as ac
import frame_cases as FC
import outlier_clamp64 as oc
import outlier_clamp_cases as OC
import reproject64 as rp
import reproject_cases as RC
from conftest import ROOT, bits_equal

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
PHX_ERR_ARG, PHX_ERR_STATE = 1, 4  # include/phx_xpu.h
SPP = 8
TILE = 16  # PHX_OUTLIER_TILE (csrc/kernels.h): a workgroup's tile of output pixels; its halo is the radius, 1 .. 3
EX, UP = oc.EXCLUDE_CENTRE, oc.UPPER_ONLY
SETTINGS = dict(gamma=1.0, floor=0.125, min_taps=3, clamped_history=3)   # tight bounds and a low cap: every branch is reached on a heavy-tailed film


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


@pytest.fixture(scope="module")
def dev(xpu):
    """a device without a scene: the call needs none"""
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=4))
    yield d
    d.close()


def test_the_tile_is_the_one_the_sizes_were_chosen_for():
    src = open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"PHX_OUTLIER_TILE = (\d+)", src).group(1)) == TILE
    kernel = open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "outlier_clamp.hip")).read()
    assert "blockIdx.x * TILE" in kernel and "blockIdx.y * TILE" in kernel and not re.search(r"\+= *gridDim", kernel)  # a thread per pixel, no stride over the grid
    # one pixel; one row and one column narrower than a halo; exactly a tile; a tile and one more column, one row short; two tiles and a
    # column whose halo of 2 and 3 reaches over a whole neighbour tile; three tiles across and two down, both ragged
    assert OC.SIZES == [(1, 1), (7, 1), (1, 7), (TILE, TILE), (TILE + 1, TILE - 1), (2 * TILE + 1, TILE + 2), (2 * TILE + 5, 2 * TILE - 3)]


@functools.lru_cache(maxsize=None)
def case(width, height, layout="x7", xb=4, self_ref=False, radius=2, trim=2, flags=0):
    """-> (A, B, the model's film, the model's summary), read-only and shared; B is A under self_ref"""
    xa, mo, so = OC.LAYOUTS[layout]
    rng = np.random.default_rng(width * 1000 + height * 10 + xa)
    A = OC.heavy(rng, width, height, xa, mo, so)
    B = A if self_ref else OC.heavy(rng, width, height, xb)
    s = dict(SETTINGS, clamped_history=SETTINGS["clamped_history"] if so else 0)
    want, summary, _ = oc.clamp(A, B, mo, so, radius, s["gamma"], s["floor"], trim, s["min_taps"], flags, s["clamped_history"])
    for arr in (A, B, want):
        arr.setflags(write=False)
    return A, B, want, summary


def check(got, summary, want, want_summary, what):
    assert got.shape == want.shape and got.dtype == F
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} floats differ from the model, first at {tuple(np.argwhere(diff)[0])}"
    assert summary == want_summary, what


def call(dev, A, B, layout, radius, trim, flags, out="new", summary=True):
    """through HipDevice.clamp_outliers on host films -> (film, summary); out: "new" (a fresh array), "film" (in place, on a copy) or "ref" """
    xa, mo, so = OC.LAYOUTS[layout]
    film = A.copy()
    ref = None if B is A else B.copy()
    target = np.full(A.shape, FC.SENTINEL, F) if out == "new" else None if out == "film" else ref
    got, s = dev.clamp_outliers(film, ref, radius, SETTINGS["gamma"], SETTINGS["floor"], trim, SETTINGS["min_taps"], bool(flags & EX), bool(flags & UP),
                                SETTINGS["clamped_history"] if so else 0, m2_offset=mo, samples_offset=so, summary=summary, out=target)
    if out != "film":
        assert bits_equal(film, A)   # film is read only
    return got, s


def run(dev, width, height, layout="x7", xb=4, self_ref=False, radius=2, trim=2, flags=0, out="new"):
    A, B, want, want_summary = case(width, height, layout, xb, self_ref, radius, trim, flags)
    got, s = call(dev, A, B, layout, radius, trim, flags, out)
    check(got, s, want, want_summary, f"{width} x {height}, {layout}, ref stride {xb}, self {self_ref}, radius {radius}, trim {trim}, flags {flags}, out {out}")
    return want_summary


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("width,height", OC.SIZES)
def test_sizes_and_radii(dev, width, height, radius):
    s = run(dev, width, height, radius=radius, trim=3 if radius != 2 else 0)
    assert s["pixels"] == width * height == s["skipped"] + s["unbounded"] + s["inside"] + s["clamped"]
    if (width, height) == (37, 29):
        assert min(s["skipped"], s["inside"], s["clamped"], s["capped"]) > 10       # every class is reached
    if width * height == 1:
        assert s["skipped"] + s["unbounded"] + s["inside"] + s["clamped"] == 1


def test_more_workgroups_than_summary_slots(dev):
    """9 x 8 = 72 ragged tiles over the 64 slots a workgroup adds its counts to by (linear workgroup id % PHX_SUMMARY_SLOTS)"""
    width, height = 141, 123
    src = open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "kernels.h")).read()
    assert -(-width // TILE) * -(-height // TILE) == 72 > int(re.search(r"PHX_SUMMARY_SLOTS = (\d+)", src).group(1)) == 64
    s = run(dev, width, height, radius=2)
    assert s["pixels"] == width * height == s["skipped"] + s["unbounded"] + s["inside"] + s["clamped"]


@pytest.mark.parametrize("width,height", OC.SIZES)
def test_a_film_against_itself_in_place(dev, width, height):
    """the despeckle: B is A, film_out is film, the centre excluded and upper only: the bounds come from the film as it was"""
    s = run(dev, width, height, self_ref=True, radius=2, trim=2, flags=EX | UP, out="film")
    if (width, height) == (37, 29):
        assert s["clamped"] > 10 and s["unbounded"] == 0
    if (width, height) == (1, 1):
        assert s["clamped"] == 0                                                      # no tap: skipped or unbounded


@pytest.mark.parametrize("trim", [0, 3])
@pytest.mark.parametrize("flags", [0, EX, UP, EX | UP])
def test_flag_words_and_trims(dev, flags, trim):
    run(dev, 37, 29, radius=3, trim=trim, flags=flags)
    run(dev, 17, 15, self_ref=True, radius=1, trim=trim, flags=flags)


@pytest.mark.parametrize("layout,xb", [("x6", 3), ("x7", 7), ("x10", 10), ("x11", 11), ("x24", 24), ("x4", 6), ("x5", 5)])
def test_layouts(dev, layout, xb):
    """3 and 4 components, strides 6, 7, 10, 11 and 24 with the channels permuted, a film without m2, a film without samples; ref's strides besides"""
    s = run(dev, 37, 29, layout, xb, radius=2, trim=1)
    assert s["clamped"] > 10
    if OC.LAYOUTS[layout][0] == xb:
        run(dev, 33, 18, layout, xb, self_ref=True, radius=3, trim=2, flags=EX)     # and against itself


@pytest.mark.parametrize("out", ["new", "film", "ref"])
@pytest.mark.parametrize("self_ref", [False, True], ids=["other", "self"])
def test_every_way_the_films_can_be_one_another_on_the_host(dev, self_ref, out):
    if self_ref and out == "ref":
        out = "film"   # ref is film: the same case as in place
    run(dev, 33, 18, "x11", 11, self_ref=self_ref, radius=2, trim=1, out=out)


def test_without_a_summary_the_film_is_the_same(dev):
    A, B, want, _ = case(33, 18)
    got, s = call(dev, A, B, "x7", 2, 2, 0, summary=False)
    assert s is None
    check(got, None, want, None, "no summary")


MODES = ["out of place", "in place", "self, out of place", "self, in place", "out is ref"]


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("mode", MODES)
def test_device_resident_films(xpu, dev, mode, misaligned):
    """the films in device memory, in every way they can be one another; once 4 bytes past a 16-byte boundary, every one of them"""
    self_ref = mode.startswith("self")
    A, B, want, want_summary = case(37, 29, "x11", 11, self_ref, 2, 1, 0)
    pad = 1 if misaligned else 0
    mk = lambda x: FC.DeviceFilm(xpu, (x.size + 2 * pad,), np.concatenate([np.full(pad, FC.SENTINEL, F), x.ravel(), np.full(pad, FC.SENTINEL, F)]))
    fa = mk(A)
    fb = fa if self_ref else mk(B)
    fo = fa if "in place" in mode else fb if mode == "out is ref" else mk(np.full(A.shape, FC.SENTINEL, F))
    try:
        film, s = dev.clamp_outliers(A.shape, B.shape, 2, SETTINGS["gamma"], SETTINGS["floor"], 1, SETTINGS["min_taps"], False, False, SETTINGS["clamped_history"],
                                     m2_offset=7, samples_offset=10, device_ptrs=[f.ptr + 4 * pad for f in (fa, fb, fo)])
        assert film is None
        got = fo.numpy()
        assert (got[:pad] == F(FC.SENTINEL)).all() and (got[got.size - pad:] == F(FC.SENTINEL)).all()   # nothing before the film, nothing behind it
        check(got[pad:pad + A.size].reshape(A.shape), s, want, want_summary, f"device-resident, {mode}, misaligned {misaligned}")
        for f, x in ((fa, A), (fb, B)):
            if f is not fo:                                                                              # an input that is not the output is read only
                kept = f.numpy()[pad:pad + x.size]
                assert np.array_equal(kept.view(np.uint32), x.ravel().view(np.uint32))
    finally:
        for f in {id(f): f for f in (fa, fb, fo)}.values():
            f.free()


def test_a_refused_call_leaves_film_out_the_summary_the_times_and_the_device_alone(xpu, dev):
    A, B, want, want_summary = case(33, 18, "x11", 11)
    call(dev, A, B, "x11", 2, 2, 0)
    times = dev.outlier_clamp_times()
    assert set(times) == {"kernel", "call"} and 0 < times["kernel"] <= times["call"]
    lib = xpu.load_library()
    out, s = np.full(A.shape, FC.SENTINEL, F), xpu.abi.OutlierClampSummary(pixels=7)
    current = FC.current_hip_device(xpu)
    settings = lambda: xpu.outlier_clamp_settings(A.shape, B.shape, 2, 1.0, 0.125, 2, 3, False, False, 3, m2_offset=7, samples_offset=10)

    def refused(q, ptrs=None):
        p = ptrs or (A.ctypes.data, B.ctypes.data, out.ctypes.data)
        return lib.phx_dev_film_outlier_clamp(dev._h, C.byref(q), *p, C.byref(s)), lib.phx_last_error().decode()
    for field, change in (("on_device", dict(on_device=2)), ("flags", dict(flags=4)), ("radius", dict(radius=4)), ("trim", dict(trim=4)), ("min_taps", dict(min_taps=26)),
                          ("gamma", dict(gamma=float("nan"))), ("floor", dict(floor=-1.0)), ("clamped_history", dict(samples_offset_a=0)), ("xstride_b", dict(xstride_b=2)),
                          ("m2_offset_a", dict(m2_offset_a=9))):
        q = settings()
        for k, v in change.items():
            setattr(q, k, v)
        assert refused(q) == (PHX_ERR_ARG, f"outlier_clamp: {field} is outside its range (phx_outlier_clamp)")
    q = settings()
    for ptrs, field in (((A.ctypes.data, B.ctypes.data, A.ctypes.data + 8), "film_out"), ((A.ctypes.data, A.ctypes.data + 44, out.ctypes.data), "ref"),
                        ((A.ctypes.data, B.ctypes.data, B.ctypes.data + 4), "film_out"), ((None, B.ctypes.data, out.ctypes.data), "film"),
                        ((A.ctypes.data, None, out.ctypes.data), "ref"), ((A.ctypes.data, B.ctypes.data, None), "film_out")):
        rc, msg = refused(q, ptrs)
        assert rc == PHX_ERR_ARG and re.search(rf": {field} is outside", msg), msg
    assert lib.phx_dev_film_outlier_clamp(dev._h, None, A.ctypes.data, B.ctypes.data, out.ctypes.data, C.byref(s)) == PHX_ERR_ARG
    assert lib.phx_dev_film_outlier_clamp(None, C.byref(q), A.ctypes.data, B.ctypes.data, out.ctypes.data, C.byref(s)) == PHX_ERR_ARG
    with pytest.raises(ValueError, match="pixels"):
        dev.clamp_outliers(A, B[:, :-1])
    assert (out == F(FC.SENTINEL)).all() and (s.pixels, s.skipped, s.clamped, s.capped) == (7, 0, 0, 0)
    assert dev.outlier_clamp_times() == times and FC.current_hip_device(xpu) == current
    before = dev.stats()["device_bytes"]
    got, summary = call(dev, A, B, "x11", 2, 2, 0)
    check(got, summary, want, want_summary, "after the refusals")
    got, summary = call(dev, A, B, "x11", 2, 2, 0, out="ref")                          # the call that copies ref
    check(got, summary, want, want_summary, "film_out is ref")
    assert dev.stats()["device_bytes"] == before


# ---- real frames ----------------------------------------------------------------------------------------------------------------------------
W, H = 32, 24
OFFS_ACC, OFFS_UNIFORM = (0, 4, 7), (0, 4, 0)         # render_progressive's accumulator (8 floats) and frame film (7): (normals, m2, samples)
OFFS_PATH = RC.layout(4)[1]                           # render_camera_path's accumulator (11 floats); its frame films have 10
OFFS_PATH_FRAME = (4, 7, 0)
DESPECKLE = dict(radius=2, gamma=2.0, trim=2, min_taps=4)
HISTORY = dict(radius=1, gamma=1.0, floor=0.0, trim=0, min_taps=4, clamped_history=4)


@pytest.fixture(scope="module")
def scene():
    return FC.SCENES["cornell"](W, H, 1.0)


def make(xpu, scene):
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=4))
    d.preprocess(scene)
    return d


def frame(xpu, d, scene, seed, normals):
    film = xpu.Film(W, H, 4, normals, True, False)
    d.start(scene, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, native_sink=True))
    d.join()
    return film.data


def test_a_call_between_start_and_join_is_refused_and_device_bytes_and_a_later_frame_are_unchanged(xpu, scene):
    d = make(xpu, scene)
    tensor = FC.DeviceFilm(xpu, (H, W, 7), FC.SENTINEL)
    try:
        first = frame(xpu, d, scene, 3, False).copy()
        before = d.stats()["device_bytes"]
        d.start(scene, xpu.FrameState(3, xpu.Tiles.make(W, H, 32), None, device_film_ptr=tensor.ptr, primary_components=4, moments=True))
        out = np.full(first.shape, FC.SENTINEL, F)
        q = xpu.outlier_clamp_settings(first.shape, first.shape)
        rc = d._lib.phx_dev_film_outlier_clamp(d._h, C.byref(q), first.ctypes.data, first.ctypes.data, out.ctypes.data, None)
        msg = d._lib.phx_last_error().decode()
        d.join()
        assert rc == PHX_ERR_STATE and "frame" in msg and (out == F(FC.SENTINEL)).all()
        assert bits_equal(tensor.numpy(), first)
        got, s = d.clamp_outliers(first.copy(), **DESPECKLE)
        want, want_s, _ = oc.clamp(first, first, 4, 0, 2, 2.0, 0.0, 2, 4, EX | UP)
        check(got, s, want, want_s, "a real frame film against itself")
        assert s["clamped"] > 0
        assert d.stats()["device_bytes"] == before and bits_equal(frame(xpu, d, scene, 3, False), first)
    finally:
        tensor.free()
        d.close()


def test_render_progressive_despeckles_each_frame_before_it_is_pooled(xpu, scene):
    plain = [film.copy() for film, _, _ in xpu.render_progressive(scene, SPP, 2, seed=1, depth=4)]
    none = [film.copy() for film, _, _ in xpu.render_progressive(scene, SPP, 2, seed=1, depth=4, despeckle=None)]
    got = [film.copy() for film, _, _ in xpu.render_progressive(scene, SPP, 2, seed=1, depth=4, despeckle=DESPECKLE)]
    d = make(xpu, scene)
    try:
        acc, acc_plain = np.zeros((H, W, 8), F), np.zeros((H, W, 8), F)
        for k in range(2):
            film = frame(xpu, d, scene, 1 + k, False)
            acc_plain = ac.accumulate(acc_plain, film, OFFS_ACC, OFFS_UNIFORM, SPP)
            clamped, s, _ = oc.clamp(film, film, 4, 0, 2, 2.0, 0.0, 2, 4, EX | UP)
            assert s["clamped"] > 0
            acc = ac.accumulate(acc, clamped, OFFS_ACC, OFFS_UNIFORM, SPP)
            assert bits_equal(plain[k], acc_plain) and bits_equal(none[k], acc_plain), f"without despeckle, frame {k + 1}: the chain as before"
            assert bits_equal(got[k], acc) and not bits_equal(got[k], acc_plain), f"with despeckle, frame {k + 1}"
    finally:
        d.close()


def test_render_camera_path_clamps_the_history_against_the_first_frame(xpu, scene):
    import dataclasses
    cam = scene.camera
    M = cam.to_world.astype(D).copy()
    M[:3, :3] = RC.rot_y(0.04) @ M[:3, :3]
    M[3, :3] += (0.12, 0.05, -0.1)
    path = [cam, dataclasses.replace(cam, to_world=M.astype(F))]
    settings = dict(sigma_plane=1.0, sigma_dist=4.0, max_history=24)
    args = dict(frames_per_camera=2, seed=5, guide_samples=4, reproject=settings, depth=4)
    plain = [(film.copy(), moved) for film, _, _, moved in xpu.render_camera_path(scene, path, SPP, **args)]
    none = [(film.copy(), moved) for film, _, _, moved in xpu.render_camera_path(scene, path, SPP, history_clamp=None, **args)]
    got = [(film.copy(), moved) for film, _, _, moved in xpu.render_camera_path(scene, path, SPP, history_clamp=HISTORY, **args)]
    assert len(plain) == len(none) == len(got) == 4
    model_camera = lambda c: rp.derive(c.to_world, c.fov, c.width, c.height)
    d = make(xpu, scene)
    try:
        accs = {False: xpu.accumulator(W, H, 4, True), True: xpu.accumulator(W, H, 4, True)}
        k, before, guides_before, clamped_pixels = 0, None, None, 0
        for c in path:
            d.set_camera(c)
            guides = d.render_guides(5 + k, 4)
            summary = {}
            if before is not None:
                for with_clamp in (False, True):
                    accs[with_clamp], summary[with_clamp] = rp.reproject(accs[with_clamp], guides_before, guides, model_camera(before), model_camera(c), OFFS_PATH, **settings)
            for first in (True, False):
                film = frame(xpu, d, scene, 5 + k, True)
                if before is not None and first:
                    accs[True], s, _ = oc.clamp(accs[True], film, 7, 10, 1, 1.0, 0.0, 0, 4, 0, 4)
                    clamped_pixels = s["clamped"]
                    assert s["capped"] > 0
                for with_clamp in (False, True):
                    accs[with_clamp] = ac.accumulate(accs[with_clamp], film, OFFS_PATH, OFFS_PATH_FRAME, SPP)
                assert bits_equal(plain[k][0], accs[False]) and bits_equal(none[k][0], accs[False]), f"without history_clamp, frame {k + 1}: the chain as before"
                assert bits_equal(got[k][0], accs[True]) and got[k][1] == plain[k][1] == none[k][1] == (summary.get(True) if before is not None else None), f"frame {k + 1}"
                k += 1
            before, guides_before = c, guides
        assert clamped_pixels > 0 and bits_equal(got[1][0], plain[1][0]) and not bits_equal(got[2][0], plain[2][0])
    finally:
        d.close()


def test_the_c_example_despeckles_and_clamps_an_orbit(tmp_path):
    """examples/render_room.c `despeckle display`: the summary line and an image; `orbit 2 clamp`: the clamp's line for the second camera and two images"""
    exe = os.path.join(ROOT, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "examples")], check=True)
    out = str(tmp_path / "room.f32")
    head = b"P6\n128 96\n255\n"
    r = subprocess.run([exe, out, "host-bvh", "despeckle", "display"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.findall(r"despeckle: frame (\d+) clamped (\d+) inside (\d+) skipped (\d+) unbounded (\d+) of (\d+) film mean (\S+) -> (\S+)", r.stdout)
    assert len(m) == 1 and int(m[0][0]) == 1 and int(m[0][5]) == 128 * 96 == sum(int(v) for v in m[0][1:5]) and float(m[0][7]) <= float(m[0][6])
    data = open(out + ".ppm", "rb").read()
    assert data.startswith(head) and len(data) == len(head) + 128 * 96 * 3 and os.path.getsize(out) == 128 * 96 * 16
    r = subprocess.run([exe, out, "host-bvh", "orbit", "2", "clamp"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.findall(r"orbit: camera (\d+) clamped (\d+) capped (\d+) inside (\d+) skipped (\d+) unbounded (\d+) of (\d+)", r.stdout)
    assert len(m) == 1 and int(m[0][0]) == 2 and int(m[0][6]) == 128 * 96 == int(m[0][1]) + sum(int(v) for v in m[0][3:6]) and int(m[0][2]) <= int(m[0][1])
    assert re.search(r"orbit: camera 2 reused \d+", r.stdout)
    for k in (1, 2):
        data = open(f"{out}.orbit{k}.ppm", "rb").read()
        assert data.startswith(head) and len(data) == len(head) + 128 * 96 * 3
