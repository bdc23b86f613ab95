"""The display pass (phx_display) without a GPU: the ABI and the header's text, every refusal of the argument check
(csrc/display_check.cpp through tests/native/host_display.cpp), csrc/display_rule.h compiled for the host against the numpy model of
tests/display_model.py bit for bit, and the model's own properties.  The device is held to the same model in tests/test_gpu_display.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import display_model as dm
import native_lib as NL
from native_lib import ERR_ARG

F, D = np.float32, np.float64
FIELDS = ["width", "height", "xstride", "image_pitch", "on_device", "flags", "tone", "scale", "white", "key", "low_q16", "high_q16", "min_scale",
          "max_scale", "reserved"]
SUMMARY = ["pixels", "invalid", "unlit", "counted", "scale", "from_histogram"]
TONES = (dm.CLAMP, dm.REINHARD, dm.ACES)


# ---- 1. the ABI and the header ------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_field_offsets():
    from phosphorus_mk2_amd import abi
    assert C.sizeof(abi.Display) == 64
    assert [f for f, _ in abi.Display._fields_] == FIELDS
    assert [getattr(abi.Display, f).offset for f in FIELDS] == [4 * i for i in range(15)]
    assert abi.Display.reserved.size == 8 and all(getattr(abi.Display, f).size == 4 for f in FIELDS[:-1])
    assert [f for f, _ in abi.DisplaySummary._fields_] == SUMMARY
    assert C.sizeof(abi.DisplaySummary) == 40 and [getattr(abi.DisplaySummary, f).offset for f in SUMMARY] == [0, 8, 16, 24, 32, 36]
    assert "phx_dev_film_display" in abi.EXPORTS and "phx_dev_display_times" in abi.EXPORTS
    assert (abi.DISPLAY_DITHER, abi.DISPLAY_AUTO_EXPOSURE) == (dm.DITHER, dm.AUTO) == (1, 2)
    assert (abi.TONE_CLAMP, abi.TONE_REINHARD, abi.TONE_ACES) == TONES == (0, 1, 2)


def test_struct_sizes_are_the_librarys():
    from phosphorus_mk2_amd import abi, xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = xpu.load_library()
    assert lib.phx_abi_sizeof(19) == C.sizeof(abi.Display) == 64
    assert lib.phx_abi_sizeof(20) == C.sizeof(abi.DisplaySummary) == 40
    # the earlier indices stay
    assert lib.phx_abi_sizeof(18) == C.sizeof(abi.Accumulate) and lib.phx_abi_sizeof(12) == lib.phx_abi_sizeof(14) == lib.phx_abi_sizeof(17) == 0


def test_header_states_the_structs_and_the_rule():
    hdr, body = NL.header(), NL.struct_body("phx_display", strip_comments=False)
    assert re.findall(r"\b(\w+)(?:\[2\])?;", NL.struct_body("phx_display")) == FIELDS[1:]
    assert re.search(r"uint32_t\s+width,\s*height;", body) and all(re.search(rf"float\s+{f};", body) for f in ("scale", "white", "key", "min_scale", "max_scale"))
    assert re.search(r"uint64_t\s+pixels,\s*invalid,\s*unlit,\s*counted;\s*float\s+scale;[^}]*uint32_t\s+from_histogram;[^}]*\} phx_display_summary;", hdr)
    assert re.search(r"int\s+phx_dev_film_display\(phx_device\* dev, const phx_display\* p, const float\* film, uint8_t\* image,\s*"
                     r"phx_display_summary\* summary[^,]*, uint64_t\* histogram", hdr)
    assert re.search(r"int\s+phx_dev_display_times\(const phx_device\* dev, double\* ms", hdr)
    assert re.search(r"PHX_DISPLAY_DITHER = 1, PHX_DISPLAY_AUTO_EXPOSURE = 2", hdr) and re.search(r"PHX_TONE_CLAMP = 0, PHX_TONE_REINHARD = 1, PHX_TONE_ACES = 2", hdr)
    rule = hdr[hdr.index("the display pass (DESIGN 21)"):hdr.index("typedef struct phx_display")]
    flat = NL.flat(rule)
    for phrase in ["(x, y) = (i mod width, i div width)", "`invalid` when r, g or b is not finite", "Y = fp32((0.2126 r + 0.7152 g) + 0.0722 b)",
                   "in binary64", "Y <= 0 counts as `unlit`", "bin = clamp((bits(Y) >> 20) - 888, 0, 255)", "counted = the sum of the bins = pixels - invalid - unlit",
                   "linear inside its octave", "up to 0.09 stop", "N == 0: scale := the struct's scale, from_histogram = 0",
                   "c_lo = (N low_q16) >> 16", "c_hi = (N high_q16 + 65535) >> 16", "[C_k, C_k + h_k) with [c_lo, c_hi)", "S = sum of w_k (2k + 1)",
                   "p = fp32((double)S / (double)(16 W) - 16.0)", "Ybar = powf_(2.0f, p)", "scale = fminf(fmaxf(key / Ybar, min_scale), max_scale)",
                   "x = scale v_c; if !(x > 0) then x = 0", "x = fminf(x, 65536.0f)", "t = (x (1 + x / (white white))) / (1 + x)",
                   "t = (x (2.51f x + 0.03f)) / (x (2.43f x + 0.59f) + 0.14f)", "t = fminf(t, 1.0f)",
                   "e = t <= 0.0031308f ? 12.92f t : 1.055f powf_(t, 1.0f / 2.4f) - 0.055f", "q = 255.0f e + d", "d = (B[y & 3][x & 3] + 0.5f) / 16.0f",
                   "B = {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}}", "code = (uint8_t)(int)q", "NaN -> 0, +inf -> white", "R, G, B, 255"]:
        assert " ".join(phrase.split()) in flat, phrase


def test_python_settings():
    from phosphorus_mk2_amd import abi, xpu
    q = xpu.display_settings((5, 7, 8))
    assert (q.width, q.height, q.xstride, q.image_pitch, q.on_device, q.flags, q.tone) == (7, 5, 8, 0, 0, abi.DISPLAY_DITHER, abi.TONE_ACES)
    assert (q.scale, q.white, list(q.reserved)) == (1.0, 4.0, [0, 0])
    q = xpu.display_settings((5, 7, 3), "auto", "reinhard", 2.0, False, 0.25, (0.25, 1.0), (0.5, 8.0), fallback=3.0)
    assert (q.flags, q.tone, q.scale, q.white, q.key, q.low_q16, q.high_q16, q.min_scale, q.max_scale) == (abi.DISPLAY_AUTO_EXPOSURE, abi.TONE_REINHARD, 3.0, 2.0, 0.25, 16384, 65536, 0.5, 8.0)
    d = xpu.display_settings((5, 7, 3), "auto")
    assert (d.low_q16, d.high_q16, d.key, d.min_scale, d.max_scale) == (dm.DEFAULTS["low_q16"], dm.DEFAULTS["high_q16"], F(0.18), 2.0 ** -12, 2.0 ** 12)
    with pytest.raises(ValueError, match="tone"):
        xpu.display_settings((5, 7, 3), tone="filmic")
    with pytest.raises(ValueError, match="height, width, xstride"):
        xpu.display_settings((5, 7))
    with pytest.raises(ValueError, match="auto"):
        xpu.display_settings((5, 7, 3), "manual")


def test_save_ppm_round_trip(tmp_path):
    from phosphorus_mk2_amd import sceneio
    rng = np.random.default_rng(2)
    image = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    path = str(tmp_path / "a.ppm")
    sceneio.save_ppm(path, image)
    assert open(path, "rb").read() == b"P6\n7 5\n255\n" + image[..., :3].tobytes()  # alpha is dropped
    back = sceneio.load_ppm(path)
    assert back.shape == (5, 7, 3) and np.array_equal(back, image[..., :3].astype(F) / F(255))
    sceneio.save_ppm(path, image[..., :3])
    assert np.array_equal(sceneio.load_ppm(path), back)
    with pytest.raises(ValueError, match="uint8"):
        sceneio.save_ppm(path, image.astype(F))


# ---- 2. display_rule.h on the host against the model ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    """the host_display library; .check is hd_check -> (status, message)"""
    from phosphorus_mk2_amd import abi
    lib = NL.load("host_display")
    vp = C.c_void_p
    lib.check = NL.checker(lib, "hd_check", [C.POINTER(abi.Display), vp, vp])
    lib.hd_sizeof.restype = C.c_uint32; lib.hd_sizeof_summary.restype = C.c_uint32
    lib.hd_bins.argtypes = [C.c_uint64, vp, vp]; lib.hd_bins.restype = None
    lib.hd_exposure.argtypes = [vp, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]; lib.hd_exposure.restype = None
    lib.hd_codes.argtypes = [C.c_uint64, vp, C.c_float, C.c_uint32, C.c_float, C.c_float, vp]; lib.hd_codes.restype = None
    lib.hd_display.argtypes = [C.POINTER(abi.Display), vp, vp, C.POINTER(abi.DisplaySummary), vp, C.c_char_p, C.c_uint32]; lib.hd_display.restype = C.c_int
    assert lib.hd_sizeof() == C.sizeof(abi.Display) and lib.hd_sizeof_summary() == C.sizeof(abi.DisplaySummary)
    return lib


def host_bins(host, rgb):
    rgb = np.ascontiguousarray(rgb, F).reshape(-1, 3)
    out = np.empty(len(rgb), np.uint32)
    host.hd_bins(len(rgb), rgb.ctypes.data, out.ctypes.data)
    return out


def host_exposure(host, h, fallback, key, lo, hi, mn, mx):
    a = np.array(h, np.uint64)
    scale, frm = C.c_float(), C.c_uint32()
    host.hd_exposure(a.ctypes.data, fallback, key, lo, hi, mn, mx, C.byref(scale), C.byref(frm))
    return F(scale.value), frm.value


def host_codes(host, v, scale, tone, white, d):
    v = np.ascontiguousarray(v, F).ravel()
    out = np.empty(len(v), np.uint8)
    host.hd_codes(len(v), v.ctypes.data, scale, tone, white, d, out.ctypes.data)
    return out


def same_scale(a, b):
    return struct.pack("<f", a) == struct.pack("<f", b)


EDGES = [2.0 ** -16, np.nextafter(F(2.0 ** -16), F(0)), 1.0, 1.125, np.nextafter(F(1.125), F(0)), np.nextafter(F(2), F(0)), 2.0, 65536.0, np.nextafter(F(65536), F(0)),
         1e-6, 1e9, 0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-40, 3.4e38, 0.18, 2.0 ** -8, 2.0 ** 15.99]


def test_bins_at_their_edges(host):
    """a grey pixel has Y = the value to a rounding (the weights add up to 1): every edge as a grey pixel, and in one colour alone"""
    e = np.array(EDGES, F)
    grey = np.stack([e, e, e], -1)
    want = dm.bins(grey)
    assert np.array_equal(host_bins(host, grey), want)
    named = dict(zip([float(v) for v in e], want))
    at = lambda v: named[float(F(v))]
    assert at(1.0) in (127, 128) and at(1.125) - at(np.nextafter(F(1.125), F(0))) in (0, 1)
    assert at(1e-6) == 0 and at(1e9) == 255 and at(65536.0) == 255 and at(0.0) == dm.UNLIT and at(-1.0) == dm.UNLIT
    assert want[np.isnan(e) | np.isinf(e)].tolist() == [dm.INVALID] * 3 and at(1e-40) == 0 and at(3.4e38) == 255
    # exact powers of two in the green channel alone: Y = fp32(0.7152 * g), inside the octave below
    for c in range(3):
        one = np.zeros((len(e), 3), F); one[:, c] = e
        assert np.array_equal(host_bins(host, one), dm.bins(one)), c
    # a non-finite colour makes the pixel invalid whatever the others are, and a negative sum is unlit
    mixed = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.inf, -np.inf, 0], [-5, 0.001, 0.001], [0, 0, 0], [-0.0, 0, 0]], F)
    assert dm.bins(mixed).tolist() == [dm.INVALID] * 4 + [dm.UNLIT] * 3 and np.array_equal(host_bins(host, mixed), dm.bins(mixed))
    # the bins are 8 an octave: 2^(k / 8 - 16) exactly representable for k a multiple of 8
    y = np.exp2(np.arange(-16, 16, dtype=D)).astype(F)
    k = host_bins(host, np.stack([y, y, y], -1))
    assert (np.diff(k.astype(int)) == 8).all()


def test_bins_on_random_pixels(host):
    rng = np.random.default_rng(3)
    rgb = np.exp2(rng.uniform(-20, 20, (200000, 3))).astype(F) * rng.choice([1, 1, 1, -1], (200000, 3)).astype(F)
    want = dm.bins(rgb)
    assert np.array_equal(host_bins(host, rgb), want) and len(np.unique(want)) > 250


def hist(**bins_):
    h = [0] * 256
    for k, v in bins_.items():
        h[int(k[1:])] = v
    return h


HISTOGRAMS = {
    "empty": hist(), "one pixel": hist(b100=1), "one bin": hist(b131=5000), "all in bin 0": hist(b0=777), "all in bin 255": hist(b255=2 ** 32),
    "both ends": hist(b0=10, b255=10), "a cut inside a bin": hist(b90=10, b100=1000, b110=10), "three bins": hist(b120=3, b121=5, b122=2),
    "ramp": [k + 1 for k in range(256)], "huge": [2 ** 24] * 256,
}
PERCENTILES = [(32768, 62259), (0, 65536), (0, 1), (65535, 65536), (1000, 1001), (30000, 40000)]


@pytest.mark.parametrize("name", list(HISTOGRAMS))
def test_exposure_on_hand_made_histograms(host, name):
    h = HISTOGRAMS[name]
    for lo, hi in PERCENTILES:
        for key, mn, mx in ((0.18, 2.0 ** -12, 2.0 ** 12), (0.5, 1e-30, 1e30), (0.18, 0.9, 1.1)):
            want = dm.exposure(h, 3.0, key, lo, hi, mn, mx)
            got = host_exposure(host, h, 3.0, key, lo, hi, mn, mx)
            assert got[1] == want[1] == (0 if name == "empty" else 1) and same_scale(got[0], want[0]), (name, lo, hi, key, got, want)


def test_exposure_by_hand():
    """values worked out on paper: one bin k gives p = (2k + 1) / 16 - 16 whatever the percentiles; N = 1; two bins cut by the ranks"""
    s, f = dm.exposure(hist(b128=9), 1.0, 0.18, 32768, 62259, 1e-30, 1e30)
    assert f == 1 and s == F(0.18) / dm.powf(np.array([2.0], F), F(257.0 / 16.0 - 16.0))[0] and abs(float(s) - 0.18 / 2 ** 0.0625) < 1e-7
    assert dm.exposure(hist(b128=1), 1.0, 0.18, 65535, 65536, 1e-30, 1e30)[0] == s
    # 10 in bin 96, 10 in bin 160, ranks [5, 15): 5 of each: the mean of 193 and 321 is 257: bin 128 again
    assert dm.exposure(hist(b96=10, b160=10), 1.0, 0.18, 16384, 49152, 1e-30, 1e30)[0] == s
    # the clamp and the fallback
    assert dm.exposure(hist(b128=9), 1.0, 0.18, 0, 65536, 0.5, 2.0)[0] == F(0.5) and dm.exposure(hist(b0=9), 1.0, 0.18, 0, 65536, 0.5, 2.0)[0] == F(2.0)
    assert dm.exposure(hist(), 7.0, 0.18, 0, 65536, 0.5, 2.0) == (F(7.0), 0)


SWEEP = np.linspace(0.0, 1.0, 2_000_001).astype(F)
DS = (0.5, 0.5 / 16.0, 15.5 / 16.0)  # no dither, the matrix's 0 and its 15


@pytest.fixture(scope="module")
def sweep_codes():
    """the model's codes of SWEEP per (tone, d), computed once"""
    return {(tone, d): dm.codes(SWEEP, 1.0, tone, 4.0, F(d)) for tone in TONES for d in DS}


@pytest.mark.parametrize("tone", TONES)
def test_encode_sweep_of_0_to_1(host, sweep_codes, tone):
    for d in DS:
        assert np.array_equal(host_codes(host, SWEEP, 1.0, tone, 4.0, d), sweep_codes[tone, d]), d


@pytest.mark.parametrize("tone", TONES)
def test_encode_far_outside_0_to_1(host, tone):
    rng = np.random.default_rng(4)
    v = np.concatenate([np.exp2(rng.uniform(-40, 100, 200000)).astype(F), -np.exp2(rng.uniform(-40, 100, 1000)).astype(F),
                        np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, 3.4e38, 1e-45, 65536.0, 65537.0, 0.0031308, 0.00313081], F)])
    for scale, white in ((1.0, 4.0), (1.005, 1.0), (2.0 ** -12, 1000.0), (2.0 ** 12, 0.25)):
        for d in DS:
            want = dm.codes(v, scale, tone, white, F(d))
            assert np.array_equal(host_codes(host, v, scale, tone, white, d), want), (scale, white, d)
    want = dm.codes(v, 1.0, tone, 4.0, F(0.5))
    assert want[-12] == 0 and want[-11] == 255 and want[-10] == 0 and want[-9] == 0 and want[-8] == 0 and want[-7] == 255  # NaN -> 0, +inf -> white


def run_host(host, film, image_pitch=0, **settings):
    from phosphorus_mk2_amd import abi
    s = dict(dm.DEFAULTS, **settings)
    H, W, xs = film.shape
    q = abi.Display(width=W, height=H, xstride=xs, image_pitch=image_pitch, **s)
    pitch = image_pitch or 4 * W
    image = np.full((H, pitch), 0x5a, np.uint8)
    summ, h, err = abi.DisplaySummary(), np.zeros(256, np.uint64), C.create_string_buffer(256)
    film = np.ascontiguousarray(film, F)
    rc = host.hd_display(C.byref(q), film.ctypes.data, image.ctypes.data, C.byref(summ), h.ctypes.data, err, 256)
    assert rc == 0, err.value
    assert (image[:, 4 * W:] == 0x5a).all()
    info = {k: int(getattr(summ, k)) for k in ("pixels", "invalid", "unlit", "counted", "from_histogram")}
    info.update(scale=float(summ.scale), histogram=h)
    return image[:, :4 * W].reshape(H, W, 4), info


def same_summary(a, b):
    return all(a[k] == b[k] for k in ("pixels", "invalid", "unlit", "counted", "from_histogram")) and same_scale(a["scale"], b["scale"]) and \
        np.array_equal(a["histogram"], b["histogram"])


@pytest.mark.parametrize("tone", TONES)
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_the_whole_call_on_the_host(host, tone, flags):
    film = dm.synthetic_film((29, 37), 7, seed=5)
    want, ws = dm.display(film, tone=tone, flags=flags, scale=1.5)
    got, gs = run_host(host, film, image_pitch=4 * 37 + 12, tone=tone, flags=flags, scale=1.5)
    assert np.array_equal(got, want) and same_summary(gs, ws)
    assert ws["invalid"] == 3 and ws["unlit"] == 3 and ws["counted"] == 29 * 37 - 6 and ws["from_histogram"] == (flags >> 1) and (want[..., 3] == 255).all()


# ---- 3. properties of the model ---------------------------------------------------------------------------------------------------------------
def test_every_code_survives_decode_and_encode():
    k = np.arange(256)
    assert np.array_equal(dm.codes(dm.srgb_decode(k).astype(F), 1.0, dm.CLAMP, 4.0, F(0.5)), k)


@pytest.mark.parametrize("tone", TONES)
def test_codes_are_monotone_in_the_input(sweep_codes, tone):
    for d in DS:
        c = sweep_codes[tone, d].astype(int)
        assert (np.diff(c) >= 0).all() and c[0] == 0 and c[-1] >= 190  # (Reinhard with white 4 shows 1.0 as 193)
    wide = np.exp2(np.linspace(-20.0, 17.0, 400001)).astype(F)
    assert (np.diff(dm.codes(wide, 1.0, tone, 4.0, F(0.5)).astype(int)) >= 0).all()


SCALE_RTOL = 2.0 * (np.log(2.0) * 2.0 ** -21 + 1.5 * 2.0 ** -23)  # two scales, each with the roundings listed in the test below


def test_a_brighter_film_shifts_the_histogram_by_whole_bins():
    rng = np.random.default_rng(6)
    film = np.exp2(rng.uniform(-10.0, 4.0, (64, 64, 3))).astype(F)
    h0 = dm.histogram(film)[0]
    for k in (-2, 1, 3):
        h = dm.histogram(film * F(2.0 ** k))[0]
        assert sum(h) == sum(h0) == 64 * 64 and h[max(0, 8 * k):256 + min(0, 8 * k)] == h0[max(0, -8 * k):256 - max(0, 8 * k)]
    # and the exposure answers with the inverse factor, to the roundings of the rule: p is rounded to fp32 at |p| < 16, an absolute 2^-21,
    # which 2^p turns into a relative ln 2 * 2^-21; powf_ is within one ulp (tests/test_oracle_math.py) and the division within half of one
    s1 = dm.exposure(h0, 1.0, 0.18, 32768, 62259, 1e-30, 1e30)[0]
    s4 = dm.exposure(dm.histogram(film * F(4))[0], 1.0, 0.18, 32768, 62259, 1e-30, 1e30)[0]
    assert abs(float(s4) * 4.0 - float(s1)) <= SCALE_RTOL * float(s1)


def test_dither_averages_to_the_value():
    """a flat grey under the 4 x 4 matrix: the block's mean code is 255 e to 1 / 16 (plain rounding is off by up to 1 / 2)"""
    d = dm.dither_plane(4, 4, True)
    assert sorted((d.ravel() * 16 - 0.5).tolist()) == list(range(16))
    worst, worst_plain = 0.0, 0.0
    for v in np.linspace(0.001, 1.0, 331).astype(F):
        t = F(v)
        e = F(12.92) * t if t <= F(0.0031308) else F(1.055) * dm.powf(np.array([t], F), F(1) / F(2.4))[0] - F(0.055)
        block = dm.codes(np.full((4, 4, 1), v, F), 1.0, dm.CLAMP, 4.0, d)
        worst = max(worst, abs(float(block.mean()) - 255.0 * float(e)))
        worst_plain = max(worst_plain, abs(float(dm.codes(np.array([v], F), 1.0, dm.CLAMP, 4.0, F(0.5))[0]) - 255.0 * float(e)))
    assert worst <= 1.0 / 16.0 and worst_plain > 0.4
    # 100.3: plain rounding says 100, the dithered block 100.3125
    v = dm.srgb_decode(100.3).astype(F)
    assert dm.codes(np.array([v], F), 1.0, dm.CLAMP, 4.0, F(0.5))[0] == 100
    assert float(dm.codes(np.full((4, 4, 1), v, F), 1.0, dm.CLAMP, 4.0, d).mean()) == 100.3125


@pytest.fixture(scope="module")
def cornell_film(orc):
    from phosphorus_mk2_amd import scenes
    film = orc.Oracle(scenes.cornell(32, 32), spp=4, pps=1, depth=9).render(rng=orc.RNG_COUNTER, seed=1, threads=4)[0]
    film.setflags(write=False)
    return film


def test_the_oracles_cornell_film_by_a_plain_loop(host, cornell_film):
    """the scale of the oracle's 32 x 32 cornell film: the model, the host compile, and a loop over the pixels that sorts their bins"""
    ks, invalid, unlit = [], 0, 0
    for r, g, b in cornell_film[..., :3].reshape(-1, 3).tolist():
        if not all(np.isfinite((r, g, b))):
            invalid += 1
            continue
        (y,) = struct.unpack("<f", struct.pack("<f", (0.2126 * r + 0.7152 * g) + 0.0722 * b))
        if y <= 0:
            unlit += 1
            continue
        (bits,) = struct.unpack("<I", struct.pack("<f", y))
        ks.append(min(max((bits >> 20) - 888, 0), 255))
    ks.sort()
    n = len(ks)
    mid = ks[(n * 32768) >> 16:(n * 62259 + 65535) >> 16]
    p = F(sum(2 * k + 1 for k in mid) / (16 * len(mid)) - 16.0)
    scale = np.minimum(np.maximum(F(0.18) / dm.powf(np.array([2.0], F), p)[0], F(2.0 ** -12)), F(2.0 ** 12))
    image, s = dm.display(cornell_film, flags=dm.AUTO | dm.DITHER)
    assert (s["invalid"], s["unlit"], s["counted"], s["from_histogram"]) == (invalid, unlit, n, 1) and n > 500
    assert same_scale(s["scale"], scale) and 0.5 < s["scale"] < 2.0
    got, gs = run_host(host, np.array(cornell_film), flags=dm.AUTO | dm.DITHER)
    assert np.array_equal(got, image) and same_summary(gs, s)
    # four times the light: a quarter of the scale, to the rule's roundings
    s4 = dm.display(cornell_film * F(4), flags=dm.AUTO | dm.DITHER)[1]
    assert abs(s4["scale"] * 4.0 - s["scale"]) <= SCALE_RTOL * s["scale"]
    assert 20 < image[..., :3].mean() < 235 and len(np.unique(image[..., :3])) > 50  # a picture, neither black nor burnt out


# ---- 4. the refusals ----------------------------------------------------------------------------------------------------------------------------
def good(**kw):
    from phosphorus_mk2_amd import abi
    q = abi.Display(width=64, height=48, xstride=8, image_pitch=0, on_device=0, flags=3, tone=1, scale=1.0, white=4.0, key=0.18, low_q16=32768, high_q16=62259,
                    min_scale=2.0 ** -12, max_scale=2.0 ** 12)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


NAN, INF = float("nan"), float("inf")
ACCEPTED = [dict(), dict(width=1, height=1), dict(width=65536, height=65536), dict(xstride=3), dict(xstride=24), dict(image_pitch=256), dict(image_pitch=260),
            dict(on_device=1), dict(on_device=2), dict(flags=0), dict(flags=1), dict(flags=2), dict(tone=0), dict(tone=2), dict(low_q16=0, high_q16=65536),
            dict(low_q16=0, high_q16=1), dict(min_scale=1.0, max_scale=1.0), dict(scale=1e-30), dict(scale=1e30),
            # fields the settings do not read are not checked
            dict(tone=0, white=0.0), dict(tone=2, white=NAN), dict(flags=1, key=0.0, low_q16=9, high_q16=3, min_scale=-1.0, max_scale=NAN)]
REFUSED = [("width", dict(width=0)), ("width", dict(width=65537)), ("height", dict(height=0)), ("height", dict(height=65537)),
           ("xstride", dict(xstride=2)), ("xstride", dict(xstride=25)), ("xstride", dict(xstride=0)),
           ("image_pitch", dict(image_pitch=252)), ("image_pitch", dict(image_pitch=258)), ("image_pitch", dict(image_pitch=4)),
           ("on_device", dict(on_device=3)), ("flags", dict(flags=4)), ("flags", dict(flags=0x80000001)), ("tone", dict(tone=3)),
           ("scale", dict(scale=0.0)), ("scale", dict(scale=-1.0)), ("scale", dict(scale=NAN)), ("scale", dict(scale=INF)),
           ("white", dict(white=0.0)), ("white", dict(white=NAN)), ("white", dict(white=INF)), ("white", dict(white=-4.0)),
           ("key", dict(key=0.0)), ("key", dict(key=NAN)), ("key", dict(key=INF)),
           ("low_q16", dict(low_q16=62259)), ("low_q16", dict(low_q16=65536)), ("high_q16", dict(high_q16=65537)),
           ("min_scale", dict(min_scale=0.0)), ("min_scale", dict(min_scale=NAN)), ("min_scale", dict(min_scale=INF)),
           ("max_scale", dict(max_scale=2.0 ** -13)), ("max_scale", dict(max_scale=NAN)), ("max_scale", dict(max_scale=INF)),
           ("reserved", dict(reserved=(C.c_uint32 * 2)(1, 0))), ("reserved", dict(reserved=(C.c_uint32 * 2)(0, 1)))]
FILM, IMAGE = 0x10000, 1 << 44  # far apart: the largest film is 2^32 pixels of 96 bytes


def check(host, q, film=FILM, image=IMAGE):
    return host.check(C.byref(q), film, image)


@pytest.mark.parametrize("kw", ACCEPTED, ids=[str(i) for i in range(len(ACCEPTED))])
def test_accepted(host, kw):
    assert check(host, good(**kw)) == (0, "")


@pytest.mark.parametrize("field,kw", REFUSED, ids=[f"{f}-{i}" for i, (f, _) in enumerate(REFUSED)])
def test_refused_with_the_fields_name(host, field, kw):
    assert check(host, good(**kw)) == (ERR_ARG, f"display: {field} is outside its range (phx_display)")


def test_the_first_field_outside_its_range_is_named(host):
    assert "width" in check(host, good(width=0, height=0, tone=9))[1] and "xstride" in check(host, good(xstride=1, flags=8, scale=0.0))[1]
    assert "flags" in check(host, good(flags=8, tone=9, scale=NAN))[1] and "low_q16" in check(host, good(low_q16=70000, high_q16=70000))[1]


def test_pointers(host):
    q = good()
    film_bytes, image_bytes = 64 * 48 * 8 * 4, 64 * 48 * 4
    assert "film" in check(host, q, 0, IMAGE)[1] and "image" in check(host, q, FILM, 0)[1]
    for off in (1, 2, 3):
        assert check(host, q, FILM, IMAGE + off) == (ERR_ARG, "display: image is outside its range (phx_display)")
    assert check(host, q, FILM, IMAGE + 4)[0] == 0
    base = 1 << 30
    for f, i in ((base, base), (base, base + film_bytes - 4), (base + image_bytes - 4, base)):
        assert check(host, q, f, i) == (ERR_ARG, "display: image is outside its range (phx_display)"), (f, i)
    assert check(host, q, base, base + film_bytes)[0] == 0 and check(host, q, base + image_bytes, base)[0] == 0  # they touch and share nothing
    # with a pitch, the image ends behind the last row's pixels, not behind its padding
    p = good(image_pitch=512)
    last = 47 * 512 + 256
    assert check(host, p, base + last, base)[0] == 0 and check(host, p, base + last - 4, base)[0] == ERR_ARG


def test_the_rule_and_the_check_under_the_sanitizers(host, tmp_path):
    """host_display.cpp's own main() under AddressSanitizer and UBSan: the check's cases get their answers, the whole call on a film of special
    pixels with a padded pitch gives the model's image and summary, and the program ends without a report"""
    stdout = NL.run_sanitized(tmp_path, "host_display", "HOST_DISPLAY_MAIN")
    got = {l.split()[0]: l.split()[1:] for l in stdout.splitlines()}
    want = {"good": None, "null-film": "film", "null-image": "image", "misaligned": "image", "overlap": "image", "width": "width", "height": "height",
            "xstride": "xstride", "pitch": "image_pitch", "on-device": "on_device", "flags": "flags", "tone": "tone", "scale": "scale", "white": "white",
            "key": "key", "low": "low_q16", "high": "high_q16", "min-scale": "min_scale", "max-scale": "max_scale", "reserved": "reserved"}
    for name, field in want.items():
        assert (got[name][0] == "0") if field is None else (got[name][0] == str(ERR_ARG) and field in got[name]), (name, got[name])
    special = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-30, 1e30, 3.4e38, 1.0, 0.18, 65536.0], F)
    film = np.full((5, 7, 8), np.nan, F)
    for i in range(35):
        for c in range(3):
            film.reshape(-1, 8)[i, c] = special[(i + 5 * c) % 12]
    for tone in TONES:
        for flags in range(4):
            image, s = dm.display(film, tone=tone, flags=flags, white=4.0, scale=1.0)
            line = got[f"call-{tone}-{flags}"]
            assert line[0] == "0" and int(line[2]) == int(image[..., :].reshape(5, 28).astype(int).sum()) and line[4] == "0", line
            assert [int(line[k]) for k in (6, 8, 10, 12)] == [s["pixels"], s["invalid"], s["unlit"], s["counted"]] and int(line[16]) == s["from_histogram"]
            assert same_scale(float(line[14]), s["scale"])
    assert got["empty"] == ["0", "3", "0"] and got["top"][2] == "1" and got["bottom"][2] == "1"
    assert same_scale(float(got["top"][1]), dm.exposure(hist(b255=2 ** 32), 3.0, 0.18, 0, 65536, 1e-30, 1e30)[0])
    assert same_scale(float(got["bottom"][1]), dm.exposure(hist(b0=1), 3.0, 0.18, 65535, 65536, 1e-30, 1e30)[0])
    assert len(got) == len(want) + 12 + 3
