"""The display pass on the device (phx_dev_film_display, csrc/display.hip) against the numpy model of tests/display_model.py: the image's bytes, the
summary and the histogram are the model's exactly, with no tolerance and no excluded pixel, on synthetic films that reach every branch of the rule
-- pixel counts around the kernels' span, film shapes off the dither's period, a film long enough for the histogram's grid to wrap, pixel
strides, a misaligned film, a padded image, every setting, the three memory modes -- then the refusals, and end to end on real frames, behind
render_progressive() and in the plain-C example."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import display_model as dm
import frame_cases as FC
from conftest import ROOT, bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
PHX_ERR_ARG, PHX_ERR_STATE = 1, 4  # include/phx_xpu.h
COUNTS = [1, 255, 256, 257, 845]  # as one-row films: around PHX_DISPLAY_SPAN, and three spans with a ragged tail
SHAPES = [(1, 1), (1, 9), (9, 1), (37, 29), (65, 67)]  # (width, height): widths off the dither's period and off 4
TONE_NAMES = {v: k for k, v in dm.TONES.items()}
CSRC = os.path.join(ROOT, "phosphorus_mk2_amd", "csrc")


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


@pytest.fixture(scope="module")
def dev(xpu):
    """a device without a scene: the call needs none"""
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=8, paths_per_sample=1, path_depth=4))
    yield d
    d.close()


def constants():
    span = int(re.search(r"PHX_DISPLAY_SPAN = (\d+)", open(os.path.join(CSRC, "kernels.h")).read()).group(1))
    groups = int(re.search(r"PHX_DISPLAY_HIST_MAX_GROUPS = (\d+)", open(os.path.join(CSRC, "display_check.h")).read()).group(1))
    return span, groups


def test_the_span_is_the_one_the_counts_were_chosen_for():
    span, groups = constants()
    assert span == 256 and {1, span - 1, span, span + 1} <= set(COUNTS) and any(c > 2 * span and c % span for c in COUNTS)
    assert any(w * h > 2 * span and (w * h) % span for w, h in SHAPES) and groups >= 1


@functools.lru_cache(maxsize=None)
def film_of(width, height, xstride=4, seed=1):
    f = dm.synthetic_film((height, width), xstride, seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def wanted(width, height, xstride, seed, tone, flags, scale):
    """the model's (image, summary) of film_of(...), computed once and shared"""
    image, s = dm.display(film_of(width, height, xstride, seed), tone=tone, flags=flags, scale=scale)
    image.setflags(write=False)
    return image, s


def same_scale(a, b):
    return struct.pack("<f", a) == struct.pack("<f", b)


def check(got, gs, want, ws, what):
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = (got != want).any(axis=-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ from the model, first at {tuple(np.argwhere(diff)[0])}: " \
                           f"{got[tuple(np.argwhere(diff)[0])]} for {want[tuple(np.argwhere(diff)[0])]}"
    if gs is not None:
        assert {k: gs[k] for k in ("pixels", "invalid", "unlit", "counted", "from_histogram")} == {k: ws[k] for k in ("pixels", "invalid", "unlit", "counted", "from_histogram")}, what
        assert same_scale(gs["scale"], ws["scale"]), (what, gs["scale"], ws["scale"])
        assert np.array_equal(gs["histogram"], ws["histogram"]), what


def run(dev, width, height, xstride=4, seed=1, tone=dm.ACES, flags=dm.DITHER | dm.AUTO, scale=1.5):
    film = film_of(width, height, xstride, seed)
    want, ws = wanted(width, height, xstride, seed, tone, flags, scale)
    got, gs = dev.display(film, "auto" if flags & dm.AUTO else scale, TONE_NAMES[tone], dither=bool(flags & dm.DITHER), summary=True, fallback=scale)
    check(got, gs, want, ws, f"{width} x {height}, xstride {xstride}, tone {tone}, flags {flags}")
    return want, ws


@pytest.mark.parametrize("count", COUNTS)
def test_pixel_counts_around_the_span(dev, count):
    run(dev, count, 1)


@pytest.mark.parametrize("width,height", SHAPES)
def test_shapes(dev, width, height):
    want, ws = run(dev, width, height)
    if width * height >= 32:
        assert ws["invalid"] == 3 and ws["unlit"] == 3 and ws["from_histogram"] == 1 and len(np.unique(want[..., :3])) > 20


def test_a_film_long_enough_for_the_histograms_grid_to_wrap(dev):
    """PHX_DISPLAY_HIST_MAX_GROUPS x span + 257 pixels: more spans than the largest grid has workgroups"""
    span, groups = constants()
    n = groups * span + 257
    width = 523  # prime: off the dither's period and off the span
    height = -(-n // width)  # whole rows: at least n pixels
    assert n <= width * height < n + width and -(-width * height // span) > groups
    run(dev, width, height, 3, seed=7)


@pytest.mark.parametrize("xstride", [3, 4, 7, 8, 11, 24])
def test_layouts(dev, xstride):
    """only the first three floats of a pixel are read: the others are NaN in these films"""
    run(dev, 37, 29, xstride)


@pytest.mark.parametrize("tone", [dm.CLAMP, dm.REINHARD, dm.ACES])
@pytest.mark.parametrize("flags", [0, dm.DITHER, dm.AUTO, dm.DITHER | dm.AUTO])
def test_settings(dev, tone, flags):
    run(dev, 65, 67, 7, seed=3, tone=tone, flags=flags)


def test_without_a_summary_the_image_is_the_same(dev):
    film = film_of(65, 67, 7, 3)
    for flags in (dm.DITHER, dm.DITHER | dm.AUTO):
        got = dev.display(film, "auto" if flags & dm.AUTO else 1.5, "aces", fallback=1.5)
        check(got, None, wanted(65, 67, 7, 3, dm.ACES, flags, 1.5)[0], None, f"no summary, flags {flags}")
    t = dev.display_times()
    assert set(t) == {"histogram", "encode", "call"} and 0 < t["histogram"] and 0 < t["encode"] and t["histogram"] + t["encode"] <= t["call"]


def test_other_settings_straight_through_the_abi(xpu, dev):
    """white, key, the percentiles and the scale's range as the model reads them; a histogram without a summary and a summary without a histogram"""
    film = film_of(37, 29, 8, 2)
    lib = xpu.load_library()
    for kw in (dict(tone=dm.REINHARD, white=1.5, flags=3, key=0.5, low_q16=1000, high_q16=65536, min_scale=1e-3, max_scale=1e3),
               dict(tone=dm.REINHARD, white=100.0, flags=2, key=0.18, low_q16=0, high_q16=1, min_scale=1.0, max_scale=1.0),
               dict(tone=dm.CLAMP, flags=3, key=0.18, low_q16=65535, high_q16=65536, min_scale=1e-30, max_scale=1e30)):
        s = dict(dm.DEFAULTS, **kw)
        want, ws = dm.display(film, **s)
        q = xpu.abi.Display(width=37, height=29, xstride=8, image_pitch=0, on_device=0, **s)
        got, summ, h = np.zeros((29, 37, 4), np.uint8), xpu.abi.DisplaySummary(), np.zeros(256, np.uint64)
        assert lib.phx_dev_film_display(dev._h, C.byref(q), film.ctypes.data, got.ctypes.data, C.byref(summ), None) == 0, lib.phx_last_error()
        gs = {k: int(getattr(summ, k)) for k in ("pixels", "invalid", "unlit", "counted", "from_histogram")}
        gs.update(scale=float(summ.scale), histogram=ws["histogram"])
        check(got, gs, want, ws, str(kw))
        got2 = np.zeros_like(got)
        assert lib.phx_dev_film_display(dev._h, C.byref(q), film.ctypes.data, got2.ctypes.data, None, h.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
        assert np.array_equal(got2, want) and np.array_equal(h, ws["histogram"])


def test_special_pixels_and_a_film_with_no_lit_pixel(dev):
    """NaN, +-inf, negative and zero pixels are shown by the rule (NaN -> 0, +inf -> white) and counted; with no lit pixel the exposure falls back"""
    film = np.zeros((5, 8, 4), F)
    film[0, 0, :3] = np.nan; film[0, 1, :3] = np.inf; film[0, 2, :3] = -np.inf; film[0, 3, :3] = -1.0; film[0, 4, :3] = (np.nan, np.inf, 0.5)
    got, s = dev.display(film, "auto", "clamp", dither=False, summary=True, fallback=2.0)
    want, ws = dm.display(film, tone=dm.CLAMP, flags=dm.AUTO, scale=2.0)
    check(got, s, want, ws, "no lit pixel")
    assert (s["pixels"], s["invalid"], s["unlit"], s["counted"], s["from_histogram"], s["scale"]) == (40, 4, 36, 0, 0, 2.0) and not s["histogram"].any()
    assert got[0, 0].tolist() == [0, 0, 0, 255] and got[0, 1].tolist() == [255] * 4 and got[0, 2].tolist() == [0, 0, 0, 255] and got[0, 4].tolist() == [0, 255, 255, 255]
    film2 = film.copy(); film2[4, 7, :3] = 0.25  # one lit pixel: N = 1
    got, s = dev.display(film2, "auto", "clamp", dither=False, summary=True, fallback=2.0)
    check(got, s, *dm.display(film2, tone=dm.CLAMP, flags=dm.AUTO, scale=2.0), "one lit pixel")
    assert s["counted"] == 1 and s["from_histogram"] == 1 and 0.5 < s["scale"] < 1.0


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
def test_device_resident_films(xpu, dev, mode, misaligned):
    """on_device 1 (film and image in device memory, the image with a padded pitch whose sentinel must survive) and 2 (the preview: the film in
    device memory, the image back on the host); once with the film 4 bytes past a 16-byte boundary"""
    W, H, xs = 65, 67, 7
    film = film_of(W, H, xs, 3)
    want, ws = wanted(W, H, xs, 3, dm.ACES, dm.DITHER | dm.AUTO, 1.5)
    pad = 1 if misaligned else 0
    df = FC.DeviceFilm(xpu, (film.size + pad,), np.concatenate([np.zeros(pad, F), film.ravel()]))
    pitch = 4 * W + 20
    di = FC.DeviceFilm(xpu, (H * pitch // 4,), FC.SENTINEL)
    try:
        if mode == 2:
            got, gs = dev.display((H, W, xs), "auto", "aces", summary=True, fallback=1.5, device_ptr=df.ptr + 4 * pad)
        else:
            out, gs = dev.display((H, W, xs), "auto", "aces", summary=True, fallback=1.5, device_ptr=df.ptr + 4 * pad, image_on_host=False, image_ptr=di.ptr, image_pitch=pitch)
            assert out is None
            raw = di.numpy().view(np.uint8).reshape(H, pitch)
            got = raw[:, :4 * W].reshape(H, W, 4)
            assert bits_equal(raw[:, 4 * W:].copy().view(F), np.full((H, 5), FC.SENTINEL, F))  # bytes past 4 * width of a row are never written
        check(got, gs, want, ws, f"on_device {mode}, misaligned {misaligned}")
        assert bits_equal(df.numpy()[pad:], film.ravel()) and not df.numpy()[:pad].any()  # the film is read only
    finally:
        df.free(); di.free()


def test_a_padded_host_image_keeps_its_padding(xpu, dev):
    W, H, xs = 37, 29, 4
    film = film_of(W, H, xs)
    want, ws = wanted(W, H, xs, 1, dm.ACES, dm.DITHER | dm.AUTO, 1.5)
    q = xpu.display_settings(film.shape, "auto", fallback=1.5)
    q.image_pitch = 4 * W + 8
    image = np.full((H, q.image_pitch), 0x5a, np.uint8)
    lib = xpu.load_library()
    assert lib.phx_dev_film_display(dev._h, C.byref(q), film.ctypes.data, image.ctypes.data, None, None) == 0, lib.phx_last_error()
    assert (image[:, 4 * W:] == 0x5a).all()
    check(image[:, :4 * W].reshape(H, W, 4), None, want, None, "padded host image")


def test_a_call_the_check_refuses_leaves_image_times_and_device_alone(xpu, dev):
    """behind a successful call, calls the argument check refuses: PHX_ERR_ARG with the check's text, image, summary and histogram what they were,
    the times still the successful call's, the caller's current HIP device what it was, device_bytes unchanged; then the device serves again"""
    film = film_of(37, 29)
    want, ws = wanted(37, 29, 4, 1, dm.ACES, dm.DITHER | dm.AUTO, 1.5)
    before = dev.stats()["device_bytes"]
    dev.display(film, "auto", fallback=1.5)
    times = dev.display_times()
    lib = xpu.load_library()
    current = FC.current_hip_device(xpu)
    image, summ, h = np.full((29, 37, 4), 7, np.uint8), xpu.abi.DisplaySummary(pixels=7), np.full(256, 9, np.uint64)
    for field, kw in (("on_device", dict(on_device=3)), ("flags", dict(flags=4)), ("tone", dict(tone=3)), ("scale", dict(scale=0.0)), ("xstride", dict(xstride=2)),
                      ("image_pitch", dict(image_pitch=6)), ("reserved", dict(reserved=(C.c_uint32 * 2)(0, 1)))):
        q = xpu.display_settings(film.shape, "auto")
        for k, v in kw.items():
            setattr(q, k, v)
        rc = lib.phx_dev_film_display(dev._h, C.byref(q), film.ctypes.data, image.ctypes.data, C.byref(summ), h.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert rc == PHX_ERR_ARG and lib.phx_last_error().decode() == f"display: {field} is outside its range (phx_display)"
    q = xpu.display_settings(film.shape, "auto")
    for f, i, field in ((None, image.ctypes.data, "film"), (film.ctypes.data, None, "image"), (film.ctypes.data, image.ctypes.data + 2, "image"),
                        (film.ctypes.data, film.ctypes.data + 64, "image")):
        assert lib.phx_dev_film_display(dev._h, C.byref(q), f, i, C.byref(summ), None) == PHX_ERR_ARG and field in lib.phx_last_error().decode()
    assert lib.phx_dev_film_display(dev._h, None, film.ctypes.data, image.ctypes.data, None, None) == PHX_ERR_ARG
    assert (image == 7).all() and (h == 9).all() and (summ.pixels, summ.invalid, summ.unlit, summ.counted, summ.from_histogram) == (7, 0, 0, 0, 0)
    assert dev.display_times() == times and FC.current_hip_device(xpu) == current
    with pytest.raises(xpu.DeviceError, match="white"):
        dev.display(film, 1.0, "reinhard", white=0.0)
    got, gs = dev.display(film, "auto", summary=True, fallback=1.5)
    check(got, gs, want, ws, "after the refusals")
    assert dev.stats()["device_bytes"] == before


# ---- real frames ----------------------------------------------------------------------------------------------------------------------------
W, H, SPP = 37, 29, 8


@pytest.fixture(scope="module")
def scene():
    return FC.SCENES["cornell"](W, H)


@pytest.fixture(scope="module")
def frame(xpu, scene):
    film = xpu.render(scene, spp=SPP, depth=4, seed=1, moments=True)[0]
    film.setflags(write=False)
    assert film.shape == (H, W, 7)
    return film


def test_a_real_frames_image_is_the_models(xpu, dev, frame):
    for exposure, tone in (("auto", "aces"), (1.0, "reinhard"), ("auto", "clamp")):
        got, gs = dev.display(frame, exposure, tone, summary=True)
        want, ws = dm.display(frame, tone=dm.TONES[tone], flags=dm.DITHER | (dm.AUTO if exposure == "auto" else 0))
        check(got, gs, want, ws, f"cornell, {exposure}, {tone}")
    assert gs["invalid"] == 0 and gs["counted"] > W * H // 2 and 0.1 < gs["scale"] < 10.0 and 20 < got[..., :3].mean() < 235
    got = xpu.display(frame, exposure="auto")  # the convenience: a device of its own
    assert np.array_equal(got, dm.display(frame, flags=3)[0])


def test_a_call_between_start_and_join_is_refused_and_disturbs_nothing(xpu, scene, frame):
    """One device: a frame into a device-resident film; between start and join the call is PHX_ERR_STATE and the frame then completes as ever, the
    image untouched; afterwards the preview of that film is the model's, device_bytes is what it was, and a later frame is what it was."""
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=4))
    tensor = FC.DeviceFilm(xpu, (H, W, 7), FC.SENTINEL)
    try:
        d.preprocess(scene)

        def start():
            d.start(scene, xpu.FrameState(1, xpu.Tiles.make(W, H, 32), None, device_film_ptr=tensor.ptr, primary_components=4, normals=False, moments=True))
        start()
        q = xpu.display_settings((H, W, 7), "auto")
        q.on_device = 2
        image = np.full((H, W, 4), 7, np.uint8)
        rc = d._lib.phx_dev_film_display(d._h, C.byref(q), tensor.ptr, image.ctypes.data, None, None)
        msg = d._lib.phx_last_error().decode()
        d.join()
        assert rc == PHX_ERR_STATE and "frame" in msg and (image == 7).all()
        assert bits_equal(tensor.numpy(), frame)
        before = d.stats()["device_bytes"]
        got, gs = d.display((H, W, 7), "auto", summary=True, device_ptr=tensor.ptr)
        check(got, gs, *dm.display(frame, flags=3), "the preview of a device-resident frame")
        assert d.stats()["device_bytes"] == before and bits_equal(tensor.numpy(), frame)
        tensor.fill(FC.SENTINEL)
        start(); d.join()
        assert bits_equal(tensor.numpy(), frame) and d.stats()["device_bytes"] == before
    finally:
        tensor.free()
        d.close()


def test_render_progressive_yields_the_image_of_each_film(xpu, dev, scene):
    plain = [(f.copy(), s, k) for f, s, k in xpu.render_progressive(scene, SPP, 2, seed=1, depth=4)]
    shown = [(f.copy(), s, k, i) for f, s, k, i in xpu.render_progressive(scene, SPP, 2, seed=1, depth=4, display=dict(exposure="auto", tone="reinhard"))]
    assert len(plain) == len(shown) == 2
    for (f0, s0, k0), (f1, s1, k1, image) in zip(plain, shown):
        assert bits_equal(f0, f1) and s0 == s1 and k0 == k1  # the first three items are what they are without display=
        assert np.array_equal(image, dev.display(f1, "auto", "reinhard")) and np.array_equal(image, dm.display(f1, tone=dm.REINHARD, flags=3)[0])
    # with denoise= the image is the denoised copy's
    for f, _, _, image in xpu.render_progressive(scene, SPP, 1, seed=1, depth=4, denoise=dict(), display=dict()):
        assert not bits_equal(f[..., :3], plain[0][0][..., :3]) and np.array_equal(image, dm.display(f, flags=dm.DITHER)[0])


def test_the_c_example_writes_the_models_image(xpu, tmp_path):
    """examples/render_room.c `display auto`: the .ppm beside the film is the model's image of the film written, and the line printed its summary"""
    from phosphorus_mk2_amd import sceneio
    exe = os.path.join(ROOT, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "examples")], check=True)
    out = str(tmp_path / "room.f32")
    r = subprocess.run([exe, out, "host-bvh", "display", "auto"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"display: scale (\S+) from_histogram (\d) pixels (\d+) invalid (\d+) unlit (\d+) counted (\d+)", r.stdout)
    assert m, r.stdout
    film = np.fromfile(out, F).reshape(96, 128, 4)
    want, ws = dm.display(film, flags=3)
    assert [int(v) for v in m.groups()[1:]] == [ws["from_histogram"], ws["pixels"], ws["invalid"], ws["unlit"], ws["counted"]] and same_scale(float(m.group(1)), ws["scale"])
    assert np.array_equal(sceneio.load_ppm(out + ".ppm"), want[..., :3].astype(F) / F(255))
    r = subprocess.run([exe, out, "host-bvh", "display"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and re.search(r"display: scale 1 from_histogram 0", r.stdout), r.stdout
    assert np.array_equal(sceneio.load_ppm(out + ".ppm"), dm.display(film, flags=dm.DITHER)[0][..., :3].astype(F) / F(255))
