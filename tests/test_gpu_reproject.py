"""set_camera and reprojection on the device (phx_dev_set_camera, phx_dev_film_reproject, csrc/reproject.hip).  The reprojection is held
to the float64 model of tests/reproject64.py bit for bit, film, normals and summary: synthetic films (tests/reproject_cases.py) over pixel
counts around the kernel's workgroup, film shapes, pixel layouts, camera pairs, host and device films, and the refusals; then real frames:
set_camera against a fresh preprocess, the reprojection of real accumulators, render_camera_path and the plain-C example."""
import ctypes as C
import dataclasses
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import accumulate64 as ac
import frame_cases as FC
import reproject64 as rp
import reproject_cases as RC
from conftest import ROOT, bits_equal

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
PHX_ERR_ARG, PHX_ERR_STATE = 1, 4  # include/phx_xpu.h
SPP = 8
BLOCK = 256  # PHX_REPROJECT_BLOCK (csrc/kernels.h): the pixels of one workgroup.  One thread per pixel and no grid stride: the grid has no span of its own
COUNTS = [BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 77]   # as one-row films
SHAPES = [(1, 1), (1, 7), (7, 1), (65, 3), (37, 29)]      # (width, height)
PAIRS = ["identical", "translation", "rotation", "both", "behind"]
SETTINGS = dict(sigma_plane=1.0, sigma_dist=4.0, max_history=16)  # 16: the cap bites on the pixels of 32 samples


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


def test_the_block_is_the_one_the_counts_were_chosen_for():
    src = open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"PHX_REPROJECT_BLOCK = (\d+)", src).group(1)) == BLOCK
    kernel = open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "reproject.hip")).read()
    assert "blockIdx.x * BLOCK + t" in kernel and not re.search(r"gridDim", kernel)  # a thread per pixel, no stride over the grid
    assert {BLOCK - 1, BLOCK, BLOCK + 1} <= set(COUNTS) and any(c > 2 * BLOCK and c % BLOCK for c in COUNTS)


def model_camera(cam):
    return rp.derive(cam.to_world, cam.fov, cam.width, cam.height)


@functools.lru_cache(maxsize=None)
def case(width, height, pair="both", pc=4, guide_stride=8):
    """-> (acc, guides_from, guides_to, camera_from, camera_to, the model's film, the model's summary), read-only and shared"""
    a, b = RC.pairs(width, height)[pair]
    rng = np.random.default_rng(width * 1000 + height)
    off = lambda: rng.uniform(-0.5, 0.5, (height, width))
    world = RC.WORLD if min(width, height) >= 3 else RC.OPEN_WALL
    (gf, normals), (gt, _) = RC.trace(world, a, off(), off()), RC.trace(world, b, off(), off())
    acc = RC.accumulator(normals, pc)
    gf, gt = RC.spoil_guides(gf, 4), RC.spoil_guides(gt, 5)
    if guide_stride != 8:
        pad = lambda g: np.concatenate([g, rng.uniform(1, 2, g.shape[:2] + (guide_stride - 8,)).astype(F)], -1)
        gf, gt = pad(gf), pad(gt)
    want, summary = rp.reproject(acc, gf, gt, model_camera(a), model_camera(b), RC.layout(pc)[1], **SETTINGS)
    for arr in (acc, gf, gt, want):
        arr.setflags(write=False)
    return acc, gf, gt, a, b, want, summary


def check(got, summary, want, want_summary, what):
    assert got.shape == want.shape and got.dtype == F
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} floats differ from the model, first at {tuple(np.argwhere(diff)[0])}"
    assert summary == want_summary, what


def run(dev, width, height, pair="both", pc=4, guide_stride=8):
    acc, gf, gt, a, b, want, want_summary = case(width, height, pair, pc, guide_stride)
    got, summary = dev.reproject(acc, gf, gt, a, b, primary_components=pc, **SETTINGS)
    check(got, summary, want, want_summary, f"{width} x {height}, {pair}, {pc} components, guide stride {guide_stride}")
    return want, want_summary


@pytest.mark.parametrize("count", COUNTS)
def test_pixel_counts_around_the_block(dev, count):
    want, s = run(dev, count, 1, "translation")
    assert s["reused"] > count // 2


def test_more_workgroups_than_summary_slots(dev):
    """66 workgroups, the last of 3 pixels, over the 64 slots a workgroup adds its counts to by (workgroup id % PHX_SUMMARY_SLOTS)"""
    count = 65 * BLOCK + 3
    src = open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "kernels.h")).read()
    assert -(-count // BLOCK) > int(re.search(r"PHX_SUMMARY_SLOTS = (\d+)", src).group(1)) == 64
    want, s = run(dev, count, 1, "translation")
    assert s["reused"] > count // 2


@pytest.mark.parametrize("width,height", SHAPES)
def test_shapes(dev, width, height):
    run(dev, width, height, "translation")


@pytest.mark.parametrize("pair", PAIRS)
def test_camera_pairs(dev, pair):
    want, s = run(dev, 37, 29, pair)
    assert s["pixels"] == 37 * 29 == s["reused"] + s["no_geometry"] + s["disoccluded"]
    assert s["reused"] > 100 and s["no_geometry"] > 0 and s["disoccluded"] > 0      # every branch is reached
    assert (want[..., RC.layout(4)[1][2]] == SETTINGS["max_history"]).any()            # the cap bites somewhere
    if pair == "identical":
        acc = case(37, 29, pair)[0]
        kept = want.any(-1) & (acc[..., 10] <= SETTINGS["max_history"])
        assert kept.sum() > 100 and bits_equal(want[kept], acc[kept])
    else:
        assert len(np.unique(want[..., 0])) > 200                                     # real mixes, not copies


@pytest.mark.parametrize("pc", [3, 4])
@pytest.mark.parametrize("guide_stride", [8, 11])
def test_layouts(dev, pc, guide_stride):
    run(dev, 37, 29, "both", pc, guide_stride)


def test_the_widest_pixels_with_the_channels_in_any_order(xpu, dev):
    """straight through the C ABI: 24 floats a pixel, samples before m2 before normals, floats of no channel in between, which travel with the
    tap of largest weight"""
    acc0, gf, gt, a, b, _, _ = case(37, 29)
    rng = np.random.default_rng(5)
    old, new = RC.layout(4)[1], (17, 9, 5)  # (normals, m2, samples)
    acc = rng.uniform(1.0, 2.0, acc0.shape[:2] + (24,)).astype(F)
    acc[..., 0:3] = acc0[..., 0:3]
    for o, n, k in zip(old, new, (3, 3, 1)):
        acc[..., n:n + k] = acc0[..., o:o + k]
    want, want_summary = rp.reproject(acc, gf, gt, model_camera(a), model_camera(b), new, **SETTINGS)
    q = xpu.reproject_settings((29, 37, 11), gf.shape, gt.shape, a, b, **SETTINGS)
    q.xstride_a, q.normals_offset_a, q.m2_offset_a, q.samples_offset_a = 24, *new
    got, s = np.full(acc.shape, FC.SENTINEL, F), xpu.abi.ReprojectSummary()
    lib = xpu.load_library()
    assert lib.phx_dev_film_reproject(dev._h, C.byref(q), acc.ctypes.data, gf.ctypes.data, gt.ctypes.data, got.ctypes.data, C.byref(s)) == 0, lib.phx_last_error()
    check(got, {k: int(getattr(s, k)) for k, _ in s._fields_}, want, want_summary, "xstride 24, permuted channels")
    assert want_summary["reused"] > 100


def test_without_a_summary_the_film_is_the_same(dev):
    acc, gf, gt, a, b, want, _ = case(65, 3, "translation")
    got, summary = dev.reproject(acc, gf, gt, a, b, summary=False, **SETTINGS)
    assert summary is None
    check(got, None, want, None, "no summary")


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
def test_device_resident_films(xpu, dev, misaligned):
    """the four films in device memory; once 4 bytes past a 16-byte boundary, every one of them"""
    acc, gf, gt, a, b, want, want_summary = case(37, 29)
    pad = 1 if misaligned else 0
    films = [FC.DeviceFilm(xpu, (x.size + pad,), np.concatenate([np.full(pad, FC.SENTINEL, F), x.ravel()])) for x in (acc, gf, gt)]
    out = FC.DeviceFilm(xpu, (acc.size + 2 * pad,), FC.SENTINEL)
    try:
        film, summary = dev.reproject(acc.shape, gf.shape, gt.shape, a, b, device_ptrs=[f.ptr + 4 * pad for f in films] + [out.ptr + 4 * pad], **SETTINGS)
        assert film is None
        got = out.numpy()
        assert (got[:pad] == F(FC.SENTINEL)).all() and (got[got.size - pad:] == F(FC.SENTINEL)).all()   # nothing before the film, nothing behind it
        for f, x in zip(films, (acc, gf, gt)):
            assert bits_equal(f.numpy()[pad:], x.ravel())                                                # the inputs are read only
        check(got[pad:pad + acc.size].reshape(acc.shape), summary, want, want_summary, f"device-resident, misaligned {misaligned}")
    finally:
        for f in films + [out]:
            f.free()


def test_a_refused_call_leaves_acc_to_the_times_and_the_device_alone(xpu, dev):
    acc, gf, gt, a, b, want, want_summary = case(37, 29)
    dev.reproject(acc, gf, gt, a, b, **SETTINGS)
    times = dev.reproject_times()
    assert set(times) == {"kernel", "call"} and 0 < times["kernel"] <= times["call"]
    lib = xpu.load_library()
    out, s = np.full(acc.shape, FC.SENTINEL, F), xpu.abi.ReprojectSummary(pixels=7)
    current = FC.current_hip_device(xpu)

    def call(q, ptrs=None):
        p = ptrs or (acc.ctypes.data, gf.ctypes.data, gt.ctypes.data, out.ctypes.data)
        return lib.phx_dev_film_reproject(dev._h, C.byref(q), *p, C.byref(s)), lib.phx_last_error().decode()
    for field, change in (("on_device", dict(on_device=2)), ("max_history", dict(max_history=1)), ("sigma_dist", dict(sigma_dist=float("nan"))),
                          ("xstride_g", dict(xstride_g=7)), ("normals_offset_a", dict(normals_offset_a=0))):
        q = xpu.reproject_settings(acc.shape, gf.shape, gt.shape, a, b, **SETTINGS)
        for k, v in change.items():
            setattr(q, k, v)
        assert call(q) == (PHX_ERR_ARG, f"reproject: {field} is outside its range (phx_reproject)")
    q = xpu.reproject_settings(acc.shape, gf.shape, gt.shape, a, b, **SETTINGS)
    q.to.to_world[0] = q.to.to_world[1] = q.to.to_world[2] = 0.0  # a zero row: singular
    assert call(q) == (PHX_ERR_ARG, "reproject: to is outside its range (phx_reproject)")
    getattr(q, "from").film_width = 36
    assert call(q)[1] == "reproject: from is outside its range (phx_reproject)"
    q = xpu.reproject_settings(acc.shape, gf.shape, gt.shape, a, b, **SETTINGS)
    for ptrs, field in (((acc.ctypes.data, gf.ctypes.data, gt.ctypes.data, acc.ctypes.data + 8), "acc_to"), ((acc.ctypes.data, gf.ctypes.data, gt.ctypes.data, gt.ctypes.data), "acc_to"),
                        ((None, gf.ctypes.data, gt.ctypes.data, out.ctypes.data), "acc_from"), ((acc.ctypes.data, gf.ctypes.data, gt.ctypes.data, None), "acc_to")):
        rc, msg = call(q, ptrs)
        assert rc == PHX_ERR_ARG and field in msg, msg
    with pytest.raises(ValueError, match="normals=True"):
        dev.reproject(acc[..., :8], gf, gt, a, b)
    assert (out == F(FC.SENTINEL)).all() and (s.pixels, s.reused, s.samples) == (7, 0, 0)
    assert dev.reproject_times() == times and FC.current_hip_device(xpu) == current
    before = dev.stats()["device_bytes"]
    got, summary = dev.reproject(acc, gf, gt, a, b, **SETTINGS)
    check(got, summary, want, want_summary, "after the refusals")
    assert dev.stats()["device_bytes"] == before


# ---- real frames ----------------------------------------------------------------------------------------------------------------------------
W, H = 32, 24
OFFS = RC.layout(4)[1]
OFFS_FRAME = (4, 7, 0)  # a uniform frame film with normals: 10 floats


def moved(cam, origin=(0.0, 0.0, 0.0), m3=None, **kw):
    M = cam.to_world.astype(D).copy()
    if m3 is not None:
        M[:3, :3] = m3 @ M[:3, :3]
    M[3, :3] += origin
    return dataclasses.replace(cam, to_world=M.astype(F), **kw)


@pytest.fixture(scope="module")
def scene():
    return FC.SCENES["cornell"](W, H, 1.0)  # through a lens narrow enough that every camera ray of the cameras below meets the box


@pytest.fixture(scope="module")
def cameras(scene):
    c = scene.camera
    return {"home": c, "near": moved(c, (0.12, 0.05, -0.1), RC.rot_y(0.04)), "lens": moved(c, (-0.1, 0.0, 0.0), aperture_radius=0.05, focal_distance=2.5)}


def make(xpu, scene):
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=4))
    d.preprocess(scene)
    return d


def frame(xpu, d, scene, seed):
    """one frame with normals and m2 -> (film (H, W, 10), the ray counts of its statistics)"""
    film = xpu.Film(W, H, 4, True, True, False)
    d.start(scene, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, native_sink=True))
    d.join()
    st = d.stats()
    return film.data, {k: st[k] for k in ("camera_samples", "rays_closest", "rays_shadow", "rays_masked", "shade_kernels")}


@pytest.fixture(scope="module")
def fresh(xpu, scene, cameras):
    """per camera: the frame of seed 3, its ray counts and the guide film of a device preprocessed with the scene under that camera"""
    out = {}
    for name, cam in cameras.items():
        sc = dataclasses.replace(scene, camera=cam)
        d = make(xpu, sc)
        try:
            film, counts = frame(xpu, d, sc, 3)
            out[name] = (film.copy(), counts, d.render_guides(3, 4))
        finally:
            d.close()
    assert not bits_equal(out["home"][0], out["near"][0]) and not bits_equal(out["home"][0], out["lens"][0])
    return out


@pytest.mark.parametrize("first,then", [("home", "near"), ("home", "lens"), ("lens", "home")])
def test_set_camera_then_a_frame_is_a_fresh_preprocess(xpu, scene, cameras, fresh, first, then):
    """film, normals, m2 and the ray counts; between a pinhole and a lens the trace and shade kernels change their instantiation"""
    sc = dataclasses.replace(scene, camera=cameras[first])
    d = make(xpu, sc)
    try:
        film, counts = frame(xpu, d, sc, 3)
        assert bits_equal(film, fresh[first][0]) and counts == fresh[first][1]
        d.set_camera(cameras[then])
        film, counts = frame(xpu, d, sc, 3)
        assert bits_equal(film, fresh[then][0]) and counts == fresh[then][1]
        assert bits_equal(d.render_guides(3, 4), fresh[then][2])
        d.set_camera(cameras[first])   # and back
        assert bits_equal(frame(xpu, d, sc, 3)[0], fresh[first][0]) and bits_equal(d.render_guides(3, 4), fresh[first][2])
    finally:
        d.close()


def test_refused_and_idle_set_camera_calls_change_no_frame(xpu, scene, cameras, fresh):
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=4))
    try:
        with pytest.raises(xpu.DeviceError, match="before preprocess"):
            d.set_camera(cameras["near"])
        d.preprocess(scene)
        d.set_camera(cameras["home"])                                       # the same camera: nothing changes
        assert bits_equal(frame(xpu, d, scene, 3)[0], fresh["home"][0])
        for bad, why in ((dataclasses.replace(cameras["near"], width=W + 1), "film size"), (dataclasses.replace(cameras["near"], height=H - 1), "film size"),
                         (dataclasses.replace(cameras["near"], aperture_radius=float("nan")), "not finite"),
                         (dataclasses.replace(cameras["near"], aperture_radius=0.1, focal_distance=float("inf")), "not finite"),
                         (dataclasses.replace(cameras["near"], width=0), "film size")):
            with pytest.raises(xpu.DeviceError, match=why):
                d.set_camera(bad)
        assert d._lib.phx_dev_set_camera(d._h, None) == PHX_ERR_ARG
        tensor = FC.DeviceFilm(xpu, (H, W, 10), FC.SENTINEL)
        try:
            d.start(scene, xpu.FrameState(3, xpu.Tiles.make(W, H, 32), None, device_film_ptr=tensor.ptr, primary_components=4, normals=True, moments=True))
            c = xpu.pack_camera(cameras["near"])
            rc = d._lib.phx_dev_set_camera(d._h, C.byref(c))
            msg = d._lib.phx_last_error().decode()
            d.join()
            assert rc == PHX_ERR_STATE and "frame" in msg
            assert bits_equal(tensor.numpy(), fresh["home"][0])             # the frame in flight was the old camera's
        finally:
            tensor.free()
        assert bits_equal(frame(xpu, d, scene, 3)[0], fresh["home"][0]) and bits_equal(d.render_guides(3, 4), fresh["home"][2])
    finally:
        d.close()


@pytest.fixture(scope="module")
def real(xpu, scene, cameras, fresh):
    """the accumulator of seeds 3 and 4 under the home camera"""
    acc = xpu.accumulator(W, H, 4, True)
    acc = ac.accumulate(acc, fresh["home"][0], OFFS, OFFS_FRAME, SPP)
    second = xpu.render(scene, spp=SPP, depth=4, seed=4, normals=True, moments=True, native_sink=True)[0]
    acc = ac.accumulate(acc, second, OFFS, OFFS_FRAME, SPP)
    acc.setflags(write=False)
    assert np.isfinite(acc).all() and (acc[..., 10] == 2 * SPP).all()
    return acc


def test_a_real_accumulator_under_an_unchanged_camera_is_the_copy(dev, cameras, fresh, real):
    g = fresh["home"][2]
    got, s = dev.reproject(real, g, g, cameras["home"], cameras["home"], max_history=64)
    assert (g[..., 3] > 0).all() and s == {"pixels": W * H, "reused": W * H, "no_geometry": 0, "disoccluded": 0, "samples": 2 * SPP * W * H}
    assert bits_equal(got, real)


@pytest.mark.parametrize("to", ["near", "lens"])
def test_a_real_accumulator_under_a_moved_camera_is_the_models(dev, cameras, fresh, real, to):
    gf, gt = fresh["home"][2], fresh[to][2]
    got, s = dev.reproject(real, gf, gt, cameras["home"], cameras[to], max_history=12)
    want, want_s = rp.reproject(real, gf, gt, model_camera(cameras["home"]), model_camera(cameras[to]), OFFS, max_history=12)
    check(got, s, want, want_s, f"real frames, home -> {to}")
    assert s["reused"] > W * H // 2 and s["pixels"] == W * H and not bits_equal(got[..., 0:3], real[..., 0:3])
    assert (got[..., 10][got.any(-1)] == 12).all()


def test_a_call_between_start_and_join_is_refused_and_disturbs_nothing(xpu, scene, cameras, fresh, real):
    d = make(xpu, scene)
    tensor = FC.DeviceFilm(xpu, (H, W, 10), FC.SENTINEL)
    try:
        d.start(scene, xpu.FrameState(3, xpu.Tiles.make(W, H, 32), None, device_film_ptr=tensor.ptr, primary_components=4, normals=True, moments=True))
        g, out = fresh["home"][2], np.full(real.shape, FC.SENTINEL, F)
        q = xpu.reproject_settings(real.shape, g.shape, g.shape, cameras["home"], cameras["near"])
        rc = d._lib.phx_dev_film_reproject(d._h, C.byref(q), real.ctypes.data, g.ctypes.data, g.ctypes.data, out.ctypes.data, None)
        msg = d._lib.phx_last_error().decode()
        d.join()
        assert rc == PHX_ERR_STATE and "frame" in msg and (out == F(FC.SENTINEL)).all()
        assert bits_equal(tensor.numpy(), fresh["home"][0])
    finally:
        tensor.free()
        d.close()


PATH_SETTINGS = dict(sigma_plane=1.0, sigma_dist=4.0, max_history=24)


def test_render_camera_path_is_the_chain_of_its_calls(xpu, scene, cameras):
    path = [cameras["home"], cameras["near"], cameras["lens"]]
    got = [(film.copy(), summary, done, moved_) for film, summary, done, moved_ in
           xpu.render_camera_path(scene, path, SPP, frames_per_camera=2, seed=5, guide_samples=4, reproject=PATH_SETTINGS, depth=4)]
    assert [g[2] for g in got] == [1, 2, 3, 4, 5, 6] and all(g[1] is None for g in got)
    d = make(xpu, scene)
    try:
        acc, k, before, guides_before = xpu.accumulator(W, H, 4, True), 0, None, None
        for cam in path:
            d.set_camera(cam)
            guides = d.render_guides(5 + k, 4)
            summary = None
            if before is not None:
                acc, summary = rp.reproject(acc, guides_before, guides, model_camera(before), model_camera(cam), OFFS, **PATH_SETTINGS)
            for _ in range(2):
                film, _counts = frame(xpu, d, scene, 5 + k)
                acc = ac.accumulate(acc, film, OFFS, OFFS_FRAME, SPP)
                assert bits_equal(got[k][0], acc) and got[k][3] == summary, f"frame {k + 1}"
                k += 1
            before, guides_before = cam, guides
        assert got[0][3] is None and got[2][3]["reused"] > W * H // 2 and got[4][3]["pixels"] == W * H
    finally:
        d.close()


def test_render_camera_path_denoises_by_each_cameras_guides_and_displays_that(xpu):
    """guided denoise with plane=True and display={} on a 32 x 32 path of two cameras of different fov: over the chain above, each yielded film
    is the denoise of the accumulator by that camera's guide film and that camera's plane scale, and each image the display of that film"""
    w, h, spp = 32, 32, 4
    sc = FC.SCENES["cornell"](w, h, 1.0)
    path = [sc.camera, moved(sc.camera, (0.12, 0.05, -0.1), RC.rot_y(0.04), fov=0.9)]
    got = [(film.copy(), image) for film, _, _, _, image in
           xpu.render_camera_path(sc, path, spp, seed=5, guide_samples=4, reproject=PATH_SETTINGS, depth=4, denoise=dict(iterations=3, guides=dict(plane=True)), display={})]
    assert len(got) == 2 and xpu.guide_plane_scale(path[0]) != xpu.guide_plane_scale(path[1])
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=spp, paths_per_sample=1, path_depth=4))
    try:
        d.preprocess(sc)
        acc, before, guides_before = xpu.accumulator(w, h, 4, True), None, None
        for k, cam in enumerate(path):
            d.set_camera(cam)
            guides = d.render_guides(5 + k, 4)
            if before is not None:
                acc, _ = rp.reproject(acc, guides_before, guides, model_camera(before), model_camera(cam), OFFS, **PATH_SETTINGS)
            film = xpu.Film(w, h, 4, True, True, False)
            d.start(sc, xpu.FrameState(5 + k, xpu.Tiles.make(w, h, 32), film, native_sink=True))
            d.join()
            acc = ac.accumulate(acc, film.data, OFFS, OFFS_FRAME, spp)
            want = d.denoise(acc, spp, 4, True, True, iterations=3, guides=guides, plane=True, plane_scale=xpu.guide_plane_scale(cam))
            assert bits_equal(got[k][0], want) and not bits_equal(want, acc), f"camera {k + 1}"
            assert got[k][1].shape == (h, w, 4) and np.array_equal(got[k][1], d.display(want)), f"camera {k + 1}"
            before, guides_before = cam, guides
    finally:
        d.close()


def test_with_every_camera_equal_the_path_is_render_progressive(xpu, scene, cameras):
    """max_history large and every pixel with geometry: each reprojection is the copy, so the accumulators are render_progressive's bit for bit"""
    want = [film.copy() for film, _, _ in xpu.render_progressive(scene, SPP, 3, seed=9, depth=4, normals=True)]
    got = [(film.copy(), moved_) for film, _, _, moved_ in
           xpu.render_camera_path(scene, [cameras["home"]] * 3, SPP, seed=9, depth=4, reproject=dict(max_history=1 << 20))]
    assert len(got) == 3
    for k in range(3):
        assert bits_equal(got[k][0], want[k]), f"after frame {k + 1}"
        assert got[k][1] is None if k == 0 else got[k][1] == {"pixels": W * H, "reused": W * H, "no_geometry": 0, "disoccluded": 0, "samples": k * SPP * W * H}


def test_the_c_example_orbits(tmp_path):
    """examples/render_room.c `orbit 2`: two cameras on an arc, one frame each, the second on top of the reprojected first; two images through
    the display pass, and the second is not the first"""
    exe = os.path.join(ROOT, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "examples")], check=True)
    out = str(tmp_path / "room.f32")
    r = subprocess.run([exe, out, "host-bvh", "orbit", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = re.findall(r"orbit: camera (\d+) reused (\d+) no_geometry (\d+) disoccluded (\d+) of (\d+)", r.stdout)
    assert [int(l[0]) for l in lines] == [2] and int(lines[0][4]) == 128 * 96 == sum(int(v) for v in lines[0][1:4]) and int(lines[0][1]) > 128 * 96 // 2
    images = []
    for k in (1, 2):
        data = open(f"{out}.orbit{k}.ppm", "rb").read()
        assert data.startswith(b"P6\n128 96\n255\n") and len(data) == len(b"P6\n128 96\n255\n") + 128 * 96 * 3
        images.append(data)
    assert images[0] != images[1]
