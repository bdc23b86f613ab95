"""The one film-layout rule of the argument checks (csrc/film_checks.h: film_layout_invalid) without a GPU, exhaustively: every small layout
and the wrap-around offsets, asked of denoise_check, of accumulate_check for either film and of outlier_clamp_check for its film through the
wrappers of tests/test_denoise.py, tests/test_accumulate.py and tests/test_outlier_clamp.py, against a restatement in Python integers of the
ranges include/phx_xpu.h states for phx_denoise, phx_accumulate and phx_outlier_clamp.  Those three modules hold the listed cases of every
other field."""
import ctypes as C
import itertools
import re

import native_lib as NL
import test_accumulate as TA
import test_denoise as TD
import test_outlier_clamp as TO
from native_lib import ERR_ARG

WRAP = [0xfffffffe, 0xffffffff]
XSTRIDES = list(range(3, 13))
OFFSETS = list(range(0, 13)) + WRAP
NO_MAX = 0xffffffff
# (smallest xstride, largest xstride, samples required): phx_denoise; acc and the frame film of phx_accumulate
DENOISE, ACC, FRAME = (6, NO_MAX, False), (7, 24, True), (6, 24, False)
# ... and (m2 required): the film of phx_outlier_clamp, which has no normals; its xstrides reach past both ends of the range
CLAMP = (3, 24, False, False)
CLAMP_XSTRIDES = [0, 2] + XSTRIDES + [24, 25, 0xffffffff]


def first_invalid(xstride, normals, m2, samples, lo, hi, samples_required, m2_required=True):
    """include/phx_xpu.h, in Python integers: xstride within its range; m2 (0: none, unless required) >= 3, m2 + 3 <= xstride; normals 0 or >= 3
    and normals + 3 <= xstride; samples 0 (unless required) or >= 3 and < xstride; no two channels share a float.  -> the first field outside
    its range in the order xstride, m2, normals, samples, or None"""
    def inside(off, length):
        return off >= 3 and off + length <= xstride

    def disjoint(a, alen, b, blen):
        return a + alen <= b or b + blen <= a
    if not lo <= xstride <= hi:
        return "xstride"
    if not (inside(m2, 3) if m2 else not m2_required):
        return "m2_offset"
    if normals and not (inside(normals, 3) and (not m2 or disjoint(normals, 3, m2, 3))):
        return "normals_offset"
    if not samples:
        return "samples_offset" if samples_required else None
    if not (inside(samples, 1) and (not m2 or disjoint(samples, 1, m2, 3)) and (not normals or disjoint(samples, 1, normals, 3))):
        return "samples_offset"
    return None


def answer(rc, text, call, struct, suffix=""):
    """(status, refusal text) -> the field the refusal names without `suffix`, or None; the text is the one every check gives"""
    if rc == 0:
        assert text == ""
        return None
    m = re.fullmatch(rf"{call}: (\w+) is outside its range \({struct}\)", text)
    assert rc == ERR_ARG and m and m.group(1).endswith(suffix), (rc, text)
    return m.group(1)[:len(m.group(1)) - len(suffix)]


def test_every_small_layout_and_the_wrapping_offsets():
    from phosphorus_mk2_amd import abi
    hd, ha = NL.load("host_denoise"), NL.load("host_accumulate")
    hd.hd_check.argtypes = [C.POINTER(abi.Denoise), C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32]
    ha.ha_check.argtypes = [C.POINTER(abi.Accumulate), C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32]
    err = C.create_string_buffer(256)
    d, a, b = TD.good(), TA.good(), TA.good()  # everything but the layout under test is valid
    assert hd.hd_check(C.byref(d), 0x10000, 0x10000, err, 256) == 0 and ha.ha_check(C.byref(a), 0x10000, 1 << 44, err, 256) == 0
    cases, refused = 0, {k: {} for k in ("denoise", "acc", "frame")}
    for xs, n, m2, s in itertools.product(XSTRIDES, OFFSETS, OFFSETS, OFFSETS):
        d.xstride, d.normals_offset, d.m2_offset, d.samples_offset = xs, n, m2, s
        a.xstride_a, a.normals_offset_a, a.m2_offset_a, a.samples_offset_a = xs, n, m2, s
        b.xstride_b, b.normals_offset_b, b.m2_offset_b, b.samples_offset_b = xs, n, m2, s
        got = {"denoise": answer(hd.hd_check(C.byref(d), 0x10000, 0x10000, err, 256), err.value.decode(), "denoise", "phx_denoise"),
               "acc": answer(ha.ha_check(C.byref(a), 0x10000, 1 << 44, err, 256), err.value.decode(), "accumulate", "phx_accumulate", "_a"),
               "frame": answer(ha.ha_check(C.byref(b), 0x10000, 1 << 44, err, 256), err.value.decode(), "accumulate", "phx_accumulate", "_b")}
        want = {"denoise": first_invalid(xs, n, m2, s, *DENOISE), "acc": first_invalid(xs, n, m2, s, *ACC), "frame": first_invalid(xs, n, m2, s, *FRAME)}
        assert got == want, (xs, n, m2, s, got, want)
        cases += 1
        for k, field in got.items():
            refused[k][field] = refused[k].get(field, 0) + 1
    assert cases == len(XSTRIDES) * len(OFFSETS) ** 3 == 33750
    for k in refused:  # the grid reaches every answer of every check
        assert set(refused[k]) == {None, "xstride", "m2_offset", "normals_offset", "samples_offset"}, (k, refused[k])
    # the clamp's film: no normals, m2 optional
    ho = NL.load("host_outlier_clamp")
    ho.ho_check.argtypes = [C.POINTER(abi.OutlierClamp)] + [C.c_void_p] * 3 + [C.c_char_p, C.c_uint32, C.POINTER(C.c_int)]
    c, copy = TO.good(), C.c_int(0)
    assert ho.ho_check(C.byref(c), *TO.FAR, err, 256, C.byref(copy)) == 0
    refused["clamp"] = {}
    for xs, m2, s in itertools.product(CLAMP_XSTRIDES, OFFSETS, OFFSETS):
        c.xstride_a, c.m2_offset_a, c.samples_offset_a = xs, m2, s
        got = answer(ho.ho_check(C.byref(c), *TO.FAR, err, 256, C.byref(copy)), err.value.decode(), "outlier_clamp", "phx_outlier_clamp", "_a")
        assert got == first_invalid(xs, 0, m2, s, *CLAMP), (xs, m2, s, got)
        refused["clamp"][got] = refused["clamp"].get(got, 0) + 1
    assert sum(refused["clamp"].values()) == len(CLAMP_XSTRIDES) * len(OFFSETS) ** 2 == 3375
    assert set(refused["clamp"]) == {None, "xstride", "m2_offset", "samples_offset"}, refused["clamp"]
    print("film layout grid:", cases, "cases;", {k: {str(f): c for f, c in v.items()} for k, v in refused.items()})


def test_the_corner_cases_under_the_sanitizers(tmp_path):
    """host_film_checks.cpp's main() under AddressSanitizer and UBSan: its corner cases get the restatement's answers, and the program ends
    without a report"""
    index = {None: -1, "xstride": 0, "normals_offset": 1, "m2_offset": 2, "samples_offset": 3}
    lines = NL.run_sanitized(tmp_path, "host_film_checks").splitlines()
    assert len(lines) == 8 * 13 ** 3
    for line in lines:
        xs, n, m2, s, *got = (int(w) for w in line.split())
        assert got == [index[first_invalid(xs, n, m2, s, *rule)] for rule in (DENOISE, ACC, FRAME)] + [index[first_invalid(xs, 0, m2, s, *CLAMP)]], line
