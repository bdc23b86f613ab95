"""The film denoiser on the device (phx_dev_denoise, csrc/denoise.hip) against the float64 model of tests/denoise64.py, bit for bit: the call
on synthetic films that reach every branch of the rule — film shapes around the 64 x 4 workgroup, iteration counts, settings, pixel layouts,
host and device films, in place and out of place — and end to end behind render(), a device-resident film and the plain-C example."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import denoise64 as dn
import frame_cases as FC
from conftest import ROOT, bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
PHX_ERR_STATE = 4  # include/phx_xpu.h
SPP = 16
BLOCK = (64, 4)  # PHX_DENOISE_BX, PHX_DENOISE_BY (csrc/kernels.h)
# the issue's shapes, and the block's own width and height -+ 1 (63 and 65 columns, 3 and 5 rows) where they were not among them
SHAPES = [(1, 1), (1, 9), (9, 1), (5, 5), (37, 29), (70, 3), (64, 64), (65, 67), (63, 5)]  # (width, height)


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


@pytest.fixture(scope="module")
def dev(xpu):
    """a device without a scene: the denoiser needs none"""
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=5))
    yield d
    d.close()


def test_the_block_is_the_one_the_shapes_were_chosen_for():
    src = open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "kernels.h")).read()
    m = re.search(r"PHX_DENOISE_BX = (\d+), PHX_DENOISE_BY = (\d+)", src)
    assert (int(m.group(1)), int(m.group(2))) == BLOCK
    widths, heights = {w for w, _ in SHAPES}, {h for _, h in SHAPES}
    assert {BLOCK[0] - 1, BLOCK[0], BLOCK[0] + 1} <= widths and {BLOCK[1] - 1, BLOCK[1] + 1} <= heights


@functools.lru_cache(maxsize=None)
def case(width, height, pc=4, normals=True, adaptive=True, iterations=5, sigma_l=4.0, power=7):
    """-> (the synthetic film, its offsets, the model's answer), all read-only and shared"""
    film, offs = dn.synthetic_film(height, width, pc, normals, adaptive, SPP)
    want = dn.denoise(film, SPP, *offs, iterations=iterations, sigma_l=sigma_l, normal_power_log2=power)
    film.setflags(write=False); want.setflags(write=False)
    return film, offs, want


def check(got, film, offs, want, what):
    """primary and m2 bit for bit the model's; every other float the input's"""
    no, mo, so = offs
    ours = [0, 1, 2, mo, mo + 1, mo + 2]
    rest = [c for c in range(film.shape[-1]) if c not in ours]
    assert got.shape == film.shape
    diff = got[..., ours].view(np.uint32) != want[..., ours].view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} floats differ from the model, first at {tuple(np.argwhere(diff)[0])}"
    assert bits_equal(got[..., rest], film[..., rest]), f"{what}: a float outside primary and m2 changed"


def test_the_synthetic_film_reaches_every_branch():
    film, (no, mo, so), want = case(37, 29)
    rgb, m2, n = film[..., 0:3], film[..., mo:mo + 3], film[..., so]
    pos = rgb[np.isfinite(rgb) & (rgb > 0)]
    assert (rgb == 0).any() and np.log10(pos.max() / pos.min()) >= 9
    assert (m2 == 0).any() and np.isnan(rgb).sum() == 1 and np.isinf(m2).sum() == 1 and (m2 < 0).sum() == 1
    assert (n == 1).sum() == 1 and n.min() == 1 and n.max() == SPP and len(np.unique(n)) > 8
    nrm = film[..., no:no + 3]
    missed = (nrm == 0).all(-1)
    assert missed.any() and len({tuple(np.round(v, 0)) for v in nrm[~missed]}) >= 3
    C, V, N, valid, _ = dn.init_state(film, SPP, no, mo, so)
    assert (~valid).sum() == 4
    assert not bits_equal(want[..., 0:3][valid], film[..., 0:3][valid])  # the filter does something here
    weights = []
    dn.iterate(C, V, N, valid, 1, 4.0, 7, weights)
    w = np.stack([np.where(ok, wt, np.nan) for dy, dx, ok, wt in weights if (dy, dx) != (0, 0)])
    assert (w == 0).any() and ((w > 0) & (w < 1e-3)).any() and (w > 0.05).any()  # rejected, nearly rejected and accepted taps


@pytest.mark.parametrize("width,height", SHAPES)
def test_shapes(dev, width, height):
    film, offs, want = case(width, height)
    check(dev.denoise(film, SPP, 4, True, True), film, offs, want, f"{width} x {height}")


@pytest.mark.parametrize("iterations", [0, 1, 2, 5, 7])
@pytest.mark.parametrize("width,height", [(37, 29), (9, 1), (1, 9)])
def test_iterations(dev, width, height, iterations):
    """(7 iterations end at step 64: on the 9-pixel films every tap but the centre is outside)"""
    film, offs, want = case(width, height, iterations=iterations)
    check(dev.denoise(film, SPP, 4, True, True, iterations=iterations), film, offs, want, f"{iterations} iterations")
    if iterations == 0:
        assert bits_equal(want, film)


@pytest.mark.parametrize("sigma_l", [0.5, 4.0])
@pytest.mark.parametrize("power", [0, 7, 10])
def test_settings(dev, sigma_l, power):
    film, offs, want = case(37, 29, sigma_l=sigma_l, power=power)
    check(dev.denoise(film, SPP, 4, True, True, sigma_l=sigma_l, normal_power_log2=power), film, offs, want, f"sigma_l {sigma_l}, power {power}")


@pytest.mark.parametrize("pc", [3, 4])
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("adaptive", [False, True])
def test_layouts(dev, pc, normals, adaptive):
    film, offs, want = case(37, 29, pc, normals, adaptive)
    check(dev.denoise(film, SPP, pc, normals, adaptive), film, offs, want, f"{pc} components, normals {normals}, adaptive {adaptive}")


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("in_place", [False, True])
def test_host_and_device_films_in_and_out_of_place(xpu, dev, on_device, in_place):
    """straight through the C ABI: both pointers host or both device memory, film_out == film_in or another film (prefilled with a sentinel)"""
    import ctypes as C
    film, offs, want = case(65, 67)
    q = xpu.denoise_settings(film.shape, SPP, 4, True, True)
    q.on_device = on_device
    lib = xpu.load_library()
    if on_device:
        src = FC.DeviceFilm(xpu, film.shape, film)
        dst = src if in_place else FC.DeviceFilm(xpu, film.shape, FC.SENTINEL)
        try:
            rc = lib.phx_dev_denoise(dev._h, C.byref(q), src.ptr, dst.ptr)
            assert rc == 0, lib.phx_last_error()
            got = dst.numpy()
            if not in_place:
                assert bits_equal(src.numpy(), film)  # film_in is read only
        finally:
            src.free(); dst.free()
    else:
        a = film.copy()
        b = a if in_place else np.full(film.shape, FC.SENTINEL, F)
        rc = lib.phx_dev_denoise(dev._h, C.byref(q), a.ctypes.data, b.ctypes.data)
        assert rc == 0, lib.phx_last_error()
        got = b
        if not in_place:
            assert bits_equal(a, film)
    check(got, film, offs, want, f"on_device {on_device}, in place {in_place}")


def test_refusals_reach_the_caller(xpu, dev):
    film, offs, _ = case(5, 5)
    with pytest.raises(xpu.DeviceError, match="iterations"):
        dev.denoise(film, SPP, 4, True, True, iterations=9)
    with pytest.raises(xpu.DeviceError, match="sigma_l"):
        dev.denoise(film, SPP, 4, True, True, sigma_l=0.0)
    with pytest.raises(xpu.DeviceError, match="spp"):
        dev.denoise(film, 1, 4, True, True)
    with pytest.raises(ValueError, match="moments=True"):
        dev.denoise(film[..., :7], SPP, 4, True, False)
    t = dev.denoise_times()
    assert set(t) == {"pack", "iterations", "unpack", "call"} and len(t["iterations"]) == 8


def test_stage_times_are_the_last_calls(dev):
    film, offs, _ = case(64, 64)
    dev.denoise(film, SPP, 4, True, True, iterations=3)
    t = dev.denoise_times()
    assert t["pack"] > 0 and t["unpack"] > 0 and t["call"] > 0
    assert [v > 0 for v in t["iterations"]] == [True] * 3 + [False] * 5


def test_a_call_the_check_refuses_leaves_films_times_and_device_alone(xpu, dev):
    """behind a successful call, one the argument check refuses (on_device = 2): PHX_ERR_ARG with the check's text, both films bit for bit
    what they were, the times still the successful call's, and the caller's current HIP device what it was
    (On a machine with one GPU the current device is 0 before and after whatever the call does: that last assertion can fail only where
    there are several.)"""
    import ctypes as C
    film, offs, _ = case(8, 8)
    dev.denoise(film, SPP, 4, True, True, iterations=2)
    times = dev.denoise_times()
    assert times["pack"] > 0 and times["iterations"][1] > 0 and times["unpack"] > 0 and times["call"] > 0
    q = xpu.denoise_settings(film.shape, SPP, 4, True, True)
    q.on_device = 2
    a, b = film.copy(), np.full(film.shape, FC.SENTINEL, F)
    lib = xpu.load_library()
    current = FC.current_hip_device(xpu)
    rc = lib.phx_dev_denoise(dev._h, C.byref(q), a.ctypes.data, b.ctypes.data)
    assert rc == 1 and lib.phx_last_error().decode() == "denoise: on_device is outside its range (phx_denoise)"  # PHX_ERR_ARG
    assert bits_equal(a, film) and bits_equal(b, np.full(film.shape, FC.SENTINEL, F))
    assert dev.denoise_times() == times
    assert FC.current_hip_device(xpu) == current


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
RENDER = dict(spp=8, depth=5, normals=True, moments=True)
ADAPTIVE = dict(threshold=0.2, min_samples=4, step=2)


@pytest.fixture(scope="module")
def cornell():
    from phosphorus_mk2_amd import scenes
    return scenes.cornell(32, 32)


@pytest.mark.parametrize("adaptive", [None, ADAPTIVE], ids=["uniform", "adaptive"])
def test_render_with_denoise_is_the_model_on_the_plain_render(xpu, cornell, adaptive):
    plain, st0 = xpu.render(cornell, adaptive=adaptive, **RENDER)
    again, _ = xpu.render(cornell, adaptive=adaptive, **RENDER)
    assert bits_equal(plain, again)
    got, st1 = xpu.render(cornell, adaptive=adaptive, denoise=dict(), **RENDER)
    xstride, no, mo, so = dn.layout(4, True, adaptive is not None)
    assert plain.shape == (32, 32, xstride)
    want = dn.denoise(plain, 8, no, mo, so)
    check(got, plain, (no, mo, so), want, "render(denoise={})")
    assert not bits_equal(got[..., 0:3], plain[..., 0:3])
    assert st0["camera_samples"] == st1["camera_samples"] and st0["rays_closest"] == st1["rays_closest"]
    got2, _ = xpu.render(cornell, adaptive=adaptive, denoise=dict(iterations=2, sigma_l=2.0, normal_power_log2=3), **RENDER)
    check(got2, plain, (no, mo, so), dn.denoise(plain, 8, no, mo, so, iterations=2, sigma_l=2.0, normal_power_log2=3), "render(denoise=settings)")


def test_device_resident_film_state_refusal_and_memory(xpu, cornell):
    """One device: a frame into a device-resident film is denoised in place through device_ptr; between start and join the call is refused with
    PHX_ERR_STATE and the frame then completes as ever; device_bytes is the same before and after a call; a later frame is what it was."""
    import ctypes as C
    W = H = 32
    xstride, no, mo, so = dn.layout(4, True, False)
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=8, paths_per_sample=1, path_depth=5))
    tensor = FC.DeviceFilm(xpu, (H, W, xstride), FC.SENTINEL)
    try:
        d.preprocess(cornell)

        def start():
            d.start(cornell, xpu.FrameState(1, xpu.Tiles.make(W, H, 32), None, device_film_ptr=tensor.ptr, primary_components=4, normals=True, moments=True))
        start()
        q = xpu.denoise_settings((H, W, xstride), 8, 4, True, False)
        q.on_device = 1
        rc = d._lib.phx_dev_denoise(d._h, C.byref(q), tensor.ptr, tensor.ptr)
        msg = d._lib.phx_last_error().decode()
        d.join()
        assert rc == PHX_ERR_STATE and "frame" in msg
        plain = tensor.numpy()
        ref, _ = xpu.render(cornell, seed=1, **RENDER)
        assert bits_equal(plain, ref)  # the refused call disturbed nothing
        before = d.stats()["device_bytes"]
        assert d.denoise((H, W, xstride), 8, 4, True, False, device_ptr=tensor.ptr) is None
        assert d.stats()["device_bytes"] == before
        check(tensor.numpy(), plain, (no, mo, so), dn.denoise(plain, 8, no, mo, so), "device-resident film")
        tensor.fill(FC.SENTINEL)
        start(); d.join()
        assert bits_equal(tensor.numpy(), plain) and d.stats()["device_bytes"] == before
    finally:
        tensor.free()
        d.close()


def test_the_c_example_with_and_without_the_keyword(xpu, tmp_path):
    """examples/render_room.c: with `denoise` it prints a smaller mean m2 and writes the model's film; without it, the film it always wrote"""
    from test_gpu_parity import _room_scene
    exe = os.path.join(ROOT, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "examples")], check=True)
    films, outs = [], []
    for args in (["host-bvh"], ["host-bvh", "denoise"]):
        out = str(tmp_path / f"room{len(films)}.f32")
        r = subprocess.run([exe, out] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        films.append(np.fromfile(out, F).reshape(96, 128, 4)); outs.append(r.stdout)
    assert "denoise:" not in outs[0] and "error estimate:" not in outs[0]
    plain, _ = xpu.render(_room_scene(), spp=8, pps=1, depth=5, seed=7, native_sink=True, bvh_builder="host", moments=True)
    assert bits_equal(films[0], plain[..., :4])  # without the keyword: the film of the frame, as before
    want = dn.denoise(plain, 8, 0, 4, 0)
    assert bits_equal(films[1], want[..., :4]) and not bits_equal(films[1], films[0])
    m = re.search(r"denoise: mean m2 ([0-9.e+-]+) -> ([0-9.e+-]+)", outs[1])
    assert m and float(m.group(2)) < float(m.group(1))
    assert abs(float(m.group(1)) - plain[..., 4:7].astype(np.float64).mean()) <= 1e-5 * float(m.group(1))
    assert abs(float(m.group(2)) - want[..., 4:7].astype(np.float64).mean()) <= 1e-5 * float(m.group(2))
