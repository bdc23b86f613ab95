"""Film accumulation on the device (phx_dev_film_accumulate, csrc/accumulate.hip) against the float64 model of tests/accumulate64.py, bit for bit
(a NaN matching a NaN): the call on synthetic films that reach every branch of the rule — pixel counts around the kernel's workgroup span, film
shapes, pixel layouts, host and device films — the exact-pooling chain, the refusals, and end to end on real frames, behind
render_progressive() and in the plain-C example."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import accumulate64 as ac
import denoise64 as dn
import frame_cases as FC
from conftest import ROOT, bits_equal
from test_accumulate import OFFS_A, OFFS_B, exact_film, integer_parts

pytestmark = pytest.mark.gpu

F = np.float32
PHX_ERR_ARG, PHX_ERR_STATE = 1, 4  # include/phx_xpu.h
SPP = 8
SPAN = 256  # PHX_ACCUMULATE_SPAN (csrc/kernels.h): the pixels of one workgroup
TAU, FLOOR = 0.3, 0.01
# pixel counts around the span, as one-row films: one pixel, span - 1, span, span + 1, three spans and a ragged tail
COUNTS = [1, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 77]
SHAPES = [(1, 1), (1, 9), (9, 1), (37, 29), (65, 67)]  # (width, height)


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


def test_the_span_is_the_one_the_counts_were_chosen_for():
    src = open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"PHX_ACCUMULATE_SPAN = (\d+)", src).group(1)) == SPAN
    assert {1, SPAN - 1, SPAN, SPAN + 1} <= set(COUNTS) and any(c > 2 * SPAN and c % SPAN for c in COUNTS)
    assert any(w * h > 2 * SPAN and (w * h) % SPAN for w, h in SHAPES)


@functools.lru_cache(maxsize=None)
def case(width, height, pc=4, normals=True, frame_samples=True):
    """-> (acc, frame, offs_a, offs_b, the model's pooled film, the model's summary), all read-only and shared"""
    acc, frame, offs_a, offs_b = ac.synthetic_films((height, width), pc, normals, frame_samples, SPP)
    want = ac.accumulate(acc, frame, offs_a, offs_b, SPP)
    for a in (acc, frame, want):
        a.setflags(write=False)
    return acc, frame, offs_a, offs_b, want, ac.summary(want, offs_a, TAU, FLOOR)


def check(got, summary, acc, offs_a, want, want_summary, what):
    """primary rgb, normals, m2 and samples the model's; every other float acc's; the summary the model's integers"""
    no, mo, so = offs_a
    ours = [0, 1, 2, mo, mo + 1, mo + 2, so] + ([no, no + 1, no + 2] if no else [])
    rest = [c for c in range(acc.shape[-1]) if c not in ours]
    assert got.shape == acc.shape
    g, w = got[..., ours], want[..., ours]
    diff = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} floats differ from the model, first at {tuple(np.argwhere(diff)[0])}"
    assert bits_equal(got[..., rest], acc[..., rest]), f"{what}: a float outside the four channels changed"
    assert summary == want_summary, what


def run(dev, width, height, pc=4, normals=True, frame_samples=True):
    acc, frame, offs_a, offs_b, want, want_summary = case(width, height, pc, normals, frame_samples)
    mine = acc.copy()
    got, summary = dev.accumulate(mine, frame, SPP, pc, normals, frame_samples, threshold=TAU, floor=FLOOR)
    assert got is mine  # a C-contiguous float32 accumulator is pooled in place
    check(got, summary, acc, offs_a, want, want_summary, f"{width} x {height}, {pc} components, normals {normals}, frame samples {frame_samples}")
    return acc, want


@pytest.mark.parametrize("count", COUNTS)
def test_pixel_counts_around_the_span(dev, count):
    run(dev, count, 1)


def summary_slots():
    """PHX_SUMMARY_SLOTS (csrc/kernels.h): a workgroup adds its counts to slot (workgroup id % slots)"""
    return int(re.search(r"PHX_SUMMARY_SLOTS = (\d+)", open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "kernels.h")).read()).group(1))


def test_more_workgroups_than_summary_slots(dev):
    """66 workgroups, the last of 3 pixels: the slots are gone round once and two of them are added to twice"""
    count = 65 * SPAN + 3
    assert -(-count // SPAN) > summary_slots() == 64
    run(dev, count, 1)


@pytest.mark.parametrize("width,height", SHAPES)
def test_shapes(dev, width, height):
    acc, want = run(dev, width, height)
    if width * height >= 32:
        assert not ac.same(want, acc) and np.isnan(want).any()  # the call does something here, and the films hold the special pixels


@pytest.mark.parametrize("pc", [3, 4])
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("frame_samples", [False, True])
def test_layouts(dev, pc, normals, frame_samples):
    """the two films' strides differ whenever the frame film has no "samples"; 4 components without normals is the stride of 8 floats, at
    which the threads of a wave meet 8-way bank conflicts on their own pixels"""
    run(dev, 37, 29, pc, normals, frame_samples)


def test_the_widest_pixels_with_the_channels_in_any_order(xpu, dev):
    """straight through the C ABI: both films at the largest xstride (24: the largest launch, 48 KB of LDS), m2 before samples before normals in
    acc and normals, samples, m2 in the frame film, floats of no channel in between, which must come back as they were"""
    acc0, frame0, offs_a, offs_b, _, _ = case(37, 29)
    rng = np.random.default_rng(5)

    def widen(film, offs, new):
        out = rng.uniform(1.0, 2.0, film.shape[:2] + (24,)).astype(F)
        out[..., 0:3] = film[..., 0:3]
        for o, n, k in zip(offs, new, (3, 3, 1)):
            out[..., n:n + k] = film[..., o:o + k]
        return out
    new_a, new_b = (17, 3, 9), (5, 20, 12)  # (normals, m2, samples)
    acc, frame = widen(acc0, offs_a, new_a), widen(frame0, offs_b, new_b)
    want = ac.accumulate(acc, frame, new_a, new_b)
    assert np.isnan(want).any() and not ac.same(want, acc)
    q = xpu.abi.Accumulate(width=37, height=29, xstride_a=24, normals_offset_a=17, m2_offset_a=3, samples_offset_a=9, xstride_b=24, normals_offset_b=5,
                           m2_offset_b=20, samples_offset_b=12, spp_b=0, on_device=0, tau=TAU, floor=FLOOR)
    got, s = acc.copy(), xpu.abi.AccumulateSummary()
    lib = xpu.load_library()
    assert lib.phx_dev_film_accumulate(dev._h, C.byref(q), got.ctypes.data, frame.ctypes.data, C.byref(s)) == 0, lib.phx_last_error()
    check(got, {k: int(getattr(s, k)) for k, _ in s._fields_}, acc, new_a, want, ac.summary(want, new_a, TAU, FLOOR), "xstride 24, permuted channels")


def test_without_a_summary_the_film_is_the_same(dev):
    acc, frame, offs_a, offs_b, want, _ = case(65, 67)
    got, summary = dev.accumulate(acc.copy(), frame, SPP, 4, True, True)
    assert summary is None
    check(got, None, acc, offs_a, want, None, "no summary")


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
def test_device_resident_films(xpu, dev, misaligned):
    """both films in device memory, pooled in place; once 4 bytes past a 16-byte boundary, where the kernel moves single floats"""
    acc, frame, offs_a, offs_b, want, want_summary = case(65, 67)
    pad = 1 if misaligned else 0
    da = FC.DeviceFilm(xpu, (acc.size + pad,), np.concatenate([np.zeros(pad, F), acc.ravel()]))
    db = FC.DeviceFilm(xpu, (frame.size + pad,), np.concatenate([np.full(pad, FC.SENTINEL, F), frame.ravel()]))
    try:
        out, summary = dev.accumulate(acc.shape, frame.shape, SPP, 4, True, True, threshold=TAU, floor=FLOOR, device_ptrs=(da.ptr + 4 * pad, db.ptr + 4 * pad))
        assert out is None
        got = da.numpy()
        assert not got[:pad].any() and bits_equal(db.numpy()[pad:], frame.ravel())  # nothing before the film, and the frame film is read only
        check(got[pad:].reshape(acc.shape), summary, acc, offs_a, want, want_summary, f"device-resident, misaligned {misaligned}")
    finally:
        da.free(); db.free()


def test_exact_pooling_chain_on_the_device(dev):
    """the 4 | 4 | 8 | 16 chain of tests/test_accumulate.py: the device's pooled film is the whole set's (V, m2, 32) bit for bit, in both associations"""
    x = integer_parts()
    whole = exact_film(x, True)
    cuts = [x[..., 0:4], x[..., 4:8], x[..., 8:16], x[..., 16:32]]

    def chain(parts):
        acc = np.zeros((1, x.shape[0], 7), F)
        for p in parts:
            dev.accumulate(acc, exact_film(p, False)[None], p.shape[-1], 3, False, False)
        return acc
    assert bits_equal(chain(cuts)[0], whole)
    first, rest = chain(cuts[3:]), chain(cuts[:3])
    got, s = dev.accumulate(first, rest, 0, 3, False, True, threshold=0.0)
    assert bits_equal(got[0], whole) and s == {"pixels": x.shape[0], "invalid": 0, "converged": 0, "samples": 32 * x.shape[0]}


def test_refusals_leave_acc_untouched_and_the_device_usable(xpu, dev):
    acc, frame, offs_a, offs_b, want, want_summary = case(37, 29, 4, True, False)
    mine = acc.copy()
    with pytest.raises(xpu.DeviceError, match="spp_b"):
        dev.accumulate(mine, frame, 0, 4, True, False)
    with pytest.raises(xpu.DeviceError, match="tau"):
        dev.accumulate(mine, frame, SPP, 4, True, False, threshold=-1.0)
    with pytest.raises(xpu.DeviceError, match="floor"):
        dev.accumulate(mine, frame, SPP, 4, True, False, threshold=0.1, floor=float("nan"))
    with pytest.raises(ValueError, match="moments=True"):
        dev.accumulate(mine, frame[..., :7], SPP, 4, True, False)
    q = xpu.accumulate_settings(acc.shape, frame.shape, SPP, 4, True, False)
    lib = xpu.load_library()
    s = xpu.abi.AccumulateSummary(pixels=7)
    for a, b, field in ((mine.ctypes.data, mine.ctypes.data, "frame_film"), (mine.ctypes.data, mine.ctypes.data + 44, "frame_film"), (None, frame.ctypes.data, "acc")):
        assert lib.phx_dev_film_accumulate(dev._h, C.byref(q), a, b, C.byref(s)) == PHX_ERR_ARG and field in lib.phx_last_error().decode()
    q.samples_offset_a = 0
    assert lib.phx_dev_film_accumulate(dev._h, C.byref(q), mine.ctypes.data, frame.ctypes.data, None) == PHX_ERR_ARG
    assert "samples_offset_a" in lib.phx_last_error().decode()
    assert bits_equal(mine, acc) and s.pixels == 7
    before = dev.stats()["device_bytes"]
    got, summary = dev.accumulate(mine, frame, SPP, 4, True, False, threshold=TAU, floor=FLOOR)
    check(got, summary, acc, offs_a, want, want_summary, "after the refusals")
    assert dev.stats()["device_bytes"] == before
    t = dev.accumulate_times()
    assert set(t) == {"kernel", "call"} and 0 < t["kernel"] <= t["call"]


def test_a_call_the_check_refuses_leaves_films_times_and_device_alone(xpu, dev):
    """behind a successful call, one the argument check refuses (on_device = 2): PHX_ERR_ARG with the check's text, both films and the summary
    bit for bit what they were, the times still the successful call's, and the caller's current HIP device what it was
    (On a machine with one GPU the current device is 0 before and after whatever the call does: that last assertion can fail only where
    there are several.)"""
    acc, frame, offs_a, offs_b, want, _ = case(8, 8)
    dev.accumulate(acc.copy(), frame, SPP, 4, True, True, threshold=TAU, floor=FLOOR)
    times = dev.accumulate_times()
    assert 0 < times["kernel"] <= times["call"]
    q = xpu.accumulate_settings(acc.shape, frame.shape, SPP, 4, True, True, TAU, FLOOR)
    q.on_device = 2
    a, b, s = acc.copy(), frame.copy(), xpu.abi.AccumulateSummary(pixels=7)
    lib = xpu.load_library()
    current = FC.current_hip_device(xpu)
    rc = lib.phx_dev_film_accumulate(dev._h, C.byref(q), a.ctypes.data, b.ctypes.data, C.byref(s))
    assert rc == PHX_ERR_ARG and lib.phx_last_error().decode() == "accumulate: on_device is outside its range (phx_accumulate)"
    assert bits_equal(a, acc) and bits_equal(b, frame) and (s.pixels, s.invalid, s.converged, s.samples) == (7, 0, 0, 0)
    assert dev.accumulate_times() == times
    assert FC.current_hip_device(xpu) == current


# ---- real frames ----------------------------------------------------------------------------------------------------------------------------
W, H = 37, 29
RENDER = dict(spp=SPP, depth=4, moments=True)
ADAPTIVE = dict(threshold=0.2, min_samples=4, step=2)
OFFS_ACC, OFFS_UNIFORM, OFFS_ADAPTIVE = ac.layout(4, False, True)[1:], ac.layout(4, False, False)[1:], ac.layout(4, False, True)[1:]


@pytest.fixture(scope="module")
def scene():
    return FC.SCENES["cornell"](W, H)


@pytest.fixture(scope="module")
def frames(xpu, scene):
    """the device's films of seeds 1, 2, 3 (uniform) and of seed 2 under adaptive sampling, read-only"""
    out = {seed: xpu.render(scene, seed=seed, **RENDER)[0] for seed in (1, 2, 3)}
    out["adaptive"] = xpu.render(scene, seed=2, adaptive=ADAPTIVE, **RENDER)[0]
    for f in out.values():
        f.setflags(write=False)
    assert out[1].shape == (H, W, 7) and out["adaptive"].shape == (H, W, 8) and not bits_equal(out[1], out[2])
    assert (out["adaptive"][..., 7] < SPP).any()
    return out


@pytest.mark.parametrize("second", ["uniform", "adaptive"])
def test_real_frames_pool_as_the_model_pools_them(xpu, dev, frames, second):
    b, offs_b = (frames[2], OFFS_UNIFORM) if second == "uniform" else (frames["adaptive"], OFFS_ADAPTIVE)
    acc = xpu.accumulator(W, H)
    dev.accumulate(acc, frames[1], SPP)
    want = ac.accumulate(xpu.accumulator(W, H), frames[1], OFFS_ACC, OFFS_UNIFORM, SPP)
    assert bits_equal(acc, want) and bits_equal(acc[..., [0, 1, 2, 4, 5, 6]], frames[1][..., [0, 1, 2, 4, 5, 6]]) and (acc[..., 7] == SPP).all()
    got, summary = dev.accumulate(acc, b, SPP, frame_adaptive=second == "adaptive", threshold=TAU, floor=FLOOR)
    want2 = ac.accumulate(want, b, OFFS_ACC, offs_b, SPP)
    check(got, summary, want, OFFS_ACC, want2, ac.summary(want2, OFFS_ACC, TAU, FLOOR), f"real frames, the second {second}")
    assert np.isfinite(got).all() and summary["invalid"] == 0 and 0 < summary["converged"] < summary["pixels"]
    assert summary["samples"] == int(got[..., 7].astype(np.float64).sum()) and (second == "adaptive") == (summary["samples"] < 2 * SPP * W * H)


def test_a_call_between_start_and_join_is_refused_and_disturbs_nothing(xpu, scene, frames):
    """One device: a frame into a device-resident film; between start and join the call is PHX_ERR_STATE and the frame then completes as ever, the
    accumulator untouched; afterwards the call pools that film, device_bytes is what it was, and a later frame is what it was."""
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=4))
    acc0 = ac.accumulate(xpu.accumulator(W, H), frames[1], OFFS_ACC, OFFS_UNIFORM, SPP)
    tensor, acc = FC.DeviceFilm(xpu, (H, W, 7), FC.SENTINEL), FC.DeviceFilm(xpu, (H, W, 8), acc0)
    try:
        d.preprocess(scene)

        def start():
            d.start(scene, xpu.FrameState(2, xpu.Tiles.make(W, H, 32), None, device_film_ptr=tensor.ptr, primary_components=4, normals=False, moments=True))
        start()
        q = xpu.accumulate_settings((H, W, 8), (H, W, 7), SPP)
        q.on_device = 1
        rc = d._lib.phx_dev_film_accumulate(d._h, C.byref(q), acc.ptr, tensor.ptr, None)
        msg = d._lib.phx_last_error().decode()
        d.join()
        assert rc == PHX_ERR_STATE and "frame" in msg
        assert bits_equal(tensor.numpy(), frames[2]) and bits_equal(acc.numpy(), acc0)  # the refused call disturbed neither
        before = d.stats()["device_bytes"]
        out, summary = d.accumulate((H, W, 8), (H, W, 7), SPP, threshold=TAU, floor=FLOOR, device_ptrs=(acc.ptr, tensor.ptr))
        want = ac.accumulate(acc0, frames[2], OFFS_ACC, OFFS_UNIFORM, SPP)
        assert out is None and d.stats()["device_bytes"] == before
        check(acc.numpy(), summary, acc0, OFFS_ACC, want, ac.summary(want, OFFS_ACC, TAU, FLOOR), "device-resident frame")
        tensor.fill(FC.SENTINEL)
        start(); d.join()
        assert bits_equal(tensor.numpy(), frames[2]) and d.stats()["device_bytes"] == before
    finally:
        tensor.free(); acc.free()
        d.close()


def test_a_film_without_a_valid_pixel_has_not_converged(xpu, scene):
    """1 spp: after the first frame every pixel has n = 1 and is invalid, so however loose the threshold the loop goes on; after the second it stops"""
    got = [(s, done) for _, s, done in xpu.render_progressive(scene, 1, 4, seed=1, depth=4, stop=dict(threshold=1e9, floor=1.0))]
    assert [done for _, done in got] == [1, 2]
    assert got[0][0]["invalid"] == got[0][0]["pixels"] == W * H and got[0][0]["converged"] == 0
    assert got[1][0]["invalid"] == 0 and got[1][0]["converged"] == W * H and got[1][0]["samples"] == 2 * W * H


def by_hand(frames, seeds):
    acc = np.zeros((H, W, 8), F)
    for s in seeds:
        acc = ac.accumulate(acc, frames[s], OFFS_ACC, OFFS_UNIFORM, SPP)
    return acc


def test_render_progressive_is_the_chain_of_its_frames(xpu, scene, frames):
    got = [(film.copy(), summary, done) for film, summary, done in xpu.render_progressive(scene, SPP, 3, seed=1, depth=4)]
    assert [g[2] for g in got] == [1, 2, 3] and all(g[1] is None for g in got)
    for k in range(3):
        assert bits_equal(got[k][0], by_hand(frames, (1, 2, 3)[:k + 1])), f"after frame {k + 1}"
    film, summary = xpu.render(scene, seed=1, progressive=dict(frames=2), **RENDER)
    assert bits_equal(film, got[1][0]) and summary is None


def test_render_progressive_stops_at_its_coverage(xpu, scene, frames):
    loose = list(xpu.render_progressive(scene, SPP, 3, seed=1, depth=4, stop=dict(threshold=1e9, floor=1.0)))
    assert len(loose) == 1 and loose[0][2] == 1
    s = loose[0][1]
    assert s == ac.summary(by_hand(frames, (1,)), OFFS_ACC, 1e9, 1.0) and s["converged"] == s["pixels"] - s["invalid"] > 0
    strict = [(summary, done) for _, summary, done in xpu.render_progressive(scene, SPP, 2, seed=1, depth=4, stop=dict(threshold=0.0))]
    assert [d for _, d in strict] == [1, 2]  # a lit scene: the pixels with m2 == 0 are far from 95 %
    assert strict[1][0] == ac.summary(by_hand(frames, (1, 2)), OFFS_ACC, 0.0, 0.0)
    assert strict[1][0]["converged"] < 0.95 * (strict[1][0]["pixels"] - strict[1][0]["invalid"])


def test_render_progressive_never_filters_the_accumulator(xpu, scene, frames):
    got = [film.copy() for film, _, _ in xpu.render_progressive(scene, SPP, 2, seed=1, depth=4, denoise=dict())]
    for k, film in enumerate(got):
        plain = by_hand(frames, (1, 2)[:k + 1])  # the UNFILTERED chain: had frame 1's yield been filtered in place, frame 2's would differ
        want = dn.denoise(plain, SPP, 0, 4, 7)
        assert bits_equal(film, want) and not bits_equal(film[..., 0:3], plain[..., 0:3]), f"after frame {k + 1}"


def test_the_c_example_pools_two_frames(xpu, tmp_path):
    """examples/render_room.c `progressive 2`: two summary lines whose samples add up, and the accumulator of the frames of seeds 7 and 8 on file"""
    from test_gpu_parity import _room_scene
    exe = os.path.join(ROOT, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "examples")], check=True)
    out = str(tmp_path / "room.f32")
    r = subprocess.run([exe, out, "host-bvh", "progressive", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = re.findall(r"progressive: frame (\d+) seed (\d+) samples (\d+) converged (\d+) of (\d+) invalid (\d+)", r.stdout)
    assert len(lines) == 2 and [(int(l[0]), int(l[1])) for l in lines] == [(1, 7), (2, 8)]
    acc = np.zeros((96, 128, 8), F)
    for k, seed in enumerate((7, 8)):
        frame, _ = xpu.render(_room_scene(), spp=8, pps=1, depth=5, seed=seed, native_sink=True, bvh_builder="host", moments=True)
        acc = ac.accumulate(acc, frame, OFFS_ACC, OFFS_UNIFORM, 8)
        s = ac.summary(acc, OFFS_ACC, 0.05, 0.01)
        assert tuple(int(v) for v in lines[k][2:]) == (s["samples"], s["converged"], s["pixels"], s["invalid"])
    assert int(lines[1][2]) == 2 * int(lines[0][2]) == 2 * 8 * 128 * 96
    assert bits_equal(np.fromfile(out, F).reshape(96, 128, 4), acc[..., :4])
