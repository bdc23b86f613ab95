"""Film accumulation across frames (phx_accumulate) without a GPU: the ABI and the header's text, every refusal of the argument check
(csrc/accumulate_check.cpp through tests/native/host_accumulate.cpp), the Python layout helpers, and the float64 model of the rule
(tests/accumulate64.py): exact pooling, general counts against the two-pass statistic, its identities, the summary's counters, and the
oracle's films of two seeds.  The device is held to the same model bit for bit in tests/test_gpu_accumulate.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import accumulate64 as ac
import frame_cases as FC
import native_lib as NL
from conftest import bits_equal
from native_lib import CSRC, ERR_ARG

F, D = np.float32, np.float64


# ---- 1. the ABI and the header ------------------------------------------------------------------------------------------------------------
FIELDS = ["width", "height", "xstride_a", "normals_offset_a", "m2_offset_a", "samples_offset_a", "xstride_b", "normals_offset_b", "m2_offset_b",
          "samples_offset_b", "spp_b", "on_device", "tau", "floor", "reserved"]


def test_struct_size_and_field_offsets():
    from phosphorus_mk2_amd import abi
    assert C.sizeof(abi.Accumulate) == 64
    assert [f for f, _ in abi.Accumulate._fields_] == FIELDS
    assert [getattr(abi.Accumulate, f).offset for f in FIELDS] == [4 * i for i in range(15)]
    assert abi.Accumulate.tau.size == 4 and abi.Accumulate.floor.size == 4 and abi.Accumulate.reserved.size == 8
    assert [f for f, _ in abi.AccumulateSummary._fields_] == ["pixels", "invalid", "converged", "samples"]
    assert C.sizeof(abi.AccumulateSummary) == 32 and [getattr(abi.AccumulateSummary, f).offset for f, _ in abi.AccumulateSummary._fields_] == [0, 8, 16, 24]
    assert "phx_dev_film_accumulate" in abi.EXPORTS and "phx_dev_accumulate_times" in abi.EXPORTS


def test_struct_size_is_the_librarys():
    from phosphorus_mk2_amd import abi, xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = xpu.load_library()
    assert lib.phx_abi_sizeof(18) == C.sizeof(abi.Accumulate) == 64
    # the earlier indices stay
    assert lib.phx_abi_sizeof(13) == C.sizeof(abi.Denoise) and lib.phx_abi_sizeof(15) == C.sizeof(abi.Guides) and lib.phx_abi_sizeof(16) == C.sizeof(abi.DenoiseGuides)


def test_header_states_the_struct_and_the_rule():
    hdr, body = NL.header(), NL.struct_body("phx_accumulate", strip_comments=False)
    assert re.findall(r"\b(\w+)(?:\[2\])?;", NL.struct_body("phx_accumulate")) == FIELDS[1:]
    assert re.search(r"uint32_t\s+width,\s*height;", body) and re.search(r"float\s+tau;", body) and re.search(r"float\s+floor;", body)
    assert re.search(r"uint64_t\s+pixels,\s*invalid,\s*converged,\s*samples;\s*\} phx_accumulate_summary;", hdr)
    assert re.search(r"int\s+phx_dev_film_accumulate\(phx_device\* dev, const phx_accumulate\* a, float\* acc, const float\* frame_film, "
                     r"phx_accumulate_summary\* summary", hdr)
    assert re.search(r"int\s+phx_dev_accumulate_times\(const phx_device\* dev, double\* ms", hdr)
    rule = hdr[hdr.index("film accumulation across frames (DESIGN 20)"):hdr.index("typedef struct phx_accumulate")]
    flat = NL.flat(rule)
    for phrase in ["n_b = samples_offset_b ? (double)samples_b : (double)spp_b", "n = n_a + n_b", "n_b == 0: the pixel of acc is not touched",
                   "n_a == 0: primary rgb, m2 := the frame's floats bit for bit; samples := fp32(n_b)", "Q_a = (m2_a n_a) n_a", "Q_b = (m2_b n_b) n_b",
                   "d = V_b - V_a", "V = fp32(V_a + (d n_b) / n)", "Q = (Q_a + Q_b) + ((d d) (n_a n_b)) / n", "m2 = fp32((Q / n) / n)",
                   "samples = fp32(n)", "the last sample with a hit wins", "A fourth component of primary stays acc's",
                   "NaN, infinite or negative", "in binary64, without contraction", "m2 n / (n - 1)", "different sampler_seeds",
                   "share paths_per_sample", "as one sample set", "must be reduced before it is accumulated",
                   "L = m2_c (n / (n - 1))", "b = tau (fabs(V_c) + floor)", "ok_c = L <= b b", "n < 2", "exact up to 2^24 samples a pixel"]:
        assert " ".join(phrase.split()) in flat, phrase


@pytest.mark.parametrize("pc", [3, 4])
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("frame_adaptive", [False, True])
def test_python_layouts_are_the_films(pc, normals, frame_adaptive):
    from phosphorus_mk2_amd import xpu
    acc = xpu.accumulator(7, 5, pc, normals)
    like = xpu.Film(7, 5, pc, normals, True, True)  # the accumulator is laid out as an adaptive film
    frame = xpu.Film(7, 5, pc, normals, True, frame_adaptive)
    assert acc.shape == like.data.shape and acc.dtype == F and not acc.any()
    q = xpu.accumulate_settings(acc.shape, frame.data.shape, 16, pc, normals, frame_adaptive, 0.05, 0.01)
    assert (q.width, q.height) == (7, 5)
    assert (q.xstride_a, q.normals_offset_a, q.m2_offset_a, q.samples_offset_a) == ac.layout(pc, normals, True) == \
        (like.xstride, pc if normals else 0, like.m2_offset, like.samples_offset)
    assert (q.xstride_b, q.normals_offset_b, q.m2_offset_b, q.samples_offset_b) == ac.layout(pc, normals, frame_adaptive) == \
        (frame.xstride, pc if normals else 0, frame.m2_offset, frame.samples_offset if frame_adaptive else 0)
    assert (q.spp_b, q.on_device, q.tau, q.floor, list(q.reserved)) == (16, 0, F(0.05), F(0.01), [0, 0])
    no_m2 = xpu.Film(7, 5, pc, normals, False, False)
    with pytest.raises(ValueError, match="moments=True"):
        xpu.accumulate_settings(acc.shape, no_m2.data.shape, 16, pc, normals, frame_adaptive)
    with pytest.raises(ValueError, match="xpu.accumulator"):
        xpu.accumulate_settings(frame.data.shape[:2] + (5,), frame.data.shape, 16, pc, normals, frame_adaptive)
    with pytest.raises(ValueError, match="pixels"):
        xpu.accumulate_settings((5, 8, acc.shape[2]), frame.data.shape, 16, pc, normals, frame_adaptive)


def test_render_refuses_progressive_without_moments():
    from phosphorus_mk2_amd import scenes, xpu
    with pytest.raises(ValueError, match="moments=True"):
        xpu.render(scenes.cornell(32, 32), spp=2, progressive=dict(frames=2))


# ---- 2. the refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check():
    """the host_accumulate library: (abi.Accumulate, acc address, frame film address) -> (status, message)"""
    from phosphorus_mk2_amd import abi
    lib = NL.load("host_accumulate")
    ha_check = NL.checker(lib, "ha_check", [C.POINTER(abi.Accumulate), C.c_void_p, C.c_void_p])
    lib.ha_sizeof.restype = C.c_uint32; lib.ha_sizeof_summary.restype = C.c_uint32
    assert lib.ha_sizeof() == C.sizeof(abi.Accumulate) and lib.ha_sizeof_summary() == C.sizeof(abi.AccumulateSummary)
    return lambda q, acc=0x10000, frame=1 << 44: ha_check(C.byref(q), acc, frame)  # (far apart: the largest film is 2^32 pixels of 96 bytes)


def good(**kw):
    from phosphorus_mk2_amd import abi
    q = abi.Accumulate(width=64, height=48, xstride_a=11, normals_offset_a=4, m2_offset_a=7, samples_offset_a=10, xstride_b=10, normals_offset_b=4,
                       m2_offset_b=7, samples_offset_b=0, spp_b=16, on_device=0, tau=0.05, floor=0.01)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


ACCEPTED = [dict(), dict(width=1, height=1), dict(width=65536, height=65536), dict(normals_offset_a=0), dict(normals_offset_b=0), dict(on_device=1),
            dict(tau=0.0, floor=0.0), dict(spp_b=1), dict(xstride_b=11, samples_offset_b=10, spp_b=0), dict(xstride_a=24, xstride_b=24),
            dict(xstride_a=7, normals_offset_a=0, m2_offset_a=3, samples_offset_a=6, xstride_b=6, normals_offset_b=0, m2_offset_b=3),
            dict(xstride_a=12, normals_offset_a=9, m2_offset_a=3, samples_offset_a=6)]
REFUSED = [("width", dict(width=0)), ("width", dict(width=65537)), ("height", dict(height=0)), ("height", dict(height=65537)),
           ("xstride_a", dict(xstride_a=6)), ("xstride_a", dict(xstride_a=25)), ("xstride_b", dict(xstride_b=5)), ("xstride_b", dict(xstride_b=25)),
           ("m2_offset_a", dict(m2_offset_a=0)), ("m2_offset_a", dict(m2_offset_a=2)), ("m2_offset_a", dict(m2_offset_a=9)),
           ("m2_offset_a", dict(m2_offset_a=0xfffffffe)), ("m2_offset_b", dict(m2_offset_b=0)), ("m2_offset_b", dict(m2_offset_b=8)),
           ("normals_offset_a", dict(normals_offset_a=2)), ("normals_offset_a", dict(normals_offset_a=9)), ("normals_offset_a", dict(normals_offset_a=5)),
           ("normals_offset_b", dict(normals_offset_b=6)), ("normals_offset_b", dict(normals_offset_b=0xffffffff)),
           ("samples_offset_a", dict(samples_offset_a=0)), ("samples_offset_a", dict(samples_offset_a=2)), ("samples_offset_a", dict(samples_offset_a=11)),
           ("samples_offset_a", dict(samples_offset_a=8)), ("samples_offset_a", dict(samples_offset_a=5)),
           ("samples_offset_b", dict(samples_offset_b=10)), ("samples_offset_b", dict(samples_offset_b=7)), ("samples_offset_b", dict(samples_offset_b=0xffffffff)),
           ("spp_b", dict(spp_b=0)), ("on_device", dict(on_device=2)),
           ("tau", dict(tau=-1.0)), ("tau", dict(tau=float("nan"))), ("tau", dict(tau=float("inf"))),
           ("floor", dict(floor=-1.0)), ("floor", dict(floor=float("nan"))), ("floor", dict(floor=float("inf")))]


@pytest.mark.parametrize("kw", ACCEPTED, ids=NL.case_ids(ACCEPTED))
def test_check_accepts(check, kw):
    assert check(good(**kw)) == (0, "")


@pytest.mark.parametrize("field,kw", REFUSED, ids=NL.case_ids(kw for _, kw in REFUSED))
def test_check_refuses_and_names_the_field(check, field, kw):
    rc, msg = check(good(**kw))
    assert rc == ERR_ARG and re.search(rf"\b{field}\b", msg), (rc, msg)


def test_the_xstride_limit_is_the_one_constant_of_check_and_kernel(check):
    """PHX_ACCUMULATE_MAX_XSTRIDE (csrc/accumulate_check.h) is what the check enforces and what the kernel's LDS is sized by"""
    limit = int(re.search(r"PHX_ACCUMULATE_MAX_XSTRIDE = (\d+)", open(os.path.join(CSRC, "accumulate_check.h")).read()).group(1))
    assert limit == 24
    assert check(good(xstride_a=limit, xstride_b=limit)) == (0, "")
    assert "xstride_a" in check(good(xstride_a=limit + 1))[1] and "xstride_b" in check(good(xstride_b=limit + 1))[1]
    assert "PHX_ACCUMULATE_MAX_XSTRIDE" in open(os.path.join(CSRC, "accumulate_check.cpp")).read()
    kernel = open(os.path.join(CSRC, "accumulate.hip")).read()
    assert re.search(r"static_assert\(SPAN \* 2u \* PHX_ACCUMULATE_MAX_XSTRIDE", kernel)

def test_check_refuses_reserved_words_and_bad_films(check):
    for i in range(2):
        q = good()
        q.reserved[i] = 1
        rc, msg = check(q)
        assert rc == ERR_ARG and "reserved" in msg
    q = good()
    bytes_a, bytes_b = 64 * 48 * 11 * 4, 64 * 48 * 10 * 4
    rc, msg = check(q, 0, 0x10000)
    assert rc == ERR_ARG and re.search(r"\bacc\b", msg)
    rc, msg = check(q, 0x10000, 0)
    assert rc == ERR_ARG and "frame_film" in msg
    base = 0x1000000
    assert check(q, base, base + bytes_a) == (0, "") and check(q, base + bytes_b, base) == (0, "")  # two films back to back, either order
    for a, b in ((base, base), (base, base + bytes_a - 4), (base + bytes_b - 4, base), (base, base + 4), (base + 4, base)):
        rc, msg = check(q, a, b)
        assert rc == ERR_ARG and "frame_film" in msg, (a, b, msg)


def test_the_check_under_the_sanitizers(tmp_path):
    """host_accumulate.cpp's own main() under AddressSanitizer and UBSan: its cases get the answers above, and the program ends without a report"""
    stdout = NL.run_sanitized(tmp_path, "host_accumulate", "HOST_ACCUMULATE_MAIN")
    got = {l.split()[0]: (int(l.split()[1]), l) for l in stdout.splitlines()}
    want = {"good": None, "same": "frame_film", "overlap": "frame_film", "null-acc": "acc", "null-frame": "frame_film", "width": "width", "height": "height",
            "xstride-a": "xstride_a", "xstride-b": "xstride_b", "m2-wrap": "m2_offset_a", "normals-overlap": "normals_offset_b",
            "no-samples-a": "samples_offset_a", "samples-past": "samples_offset_b", "spp": "spp_b", "on-device": "on_device", "tau-nan": "tau",
            "floor": "floor", "reserved": "reserved"}
    assert sorted(got) == sorted(want)
    for name, field in want.items():
        rc, line = got[name]
        assert (rc == 0) if field is None else (rc == ERR_ARG and field in line), line


# ---- 3. the synthetic films ------------------------------------------------------------------------------------------------------------------
def test_the_synthetic_films_reach_every_branch():
    acc, frame, offs_a, offs_b = ac.synthetic_films((29, 37), 4, True, True)
    (no_a, mo_a, so_a), (no_b, mo_b, so_b) = offs_a, offs_b
    n_a, n_b, bad, skip, copy, pool = ac.counts(acc, frame, offs_a, offs_b, 0)
    assert copy.any() and (skip & (n_a != 0)).any() and (skip & (n_a == 0)).any() and pool.sum() > 1000
    for v in (1.0, 2.0, 2.0 ** 24 - 1):
        assert (n_a == v).any()
    assert (n_b == 1).any()
    assert np.isnan(n_a).sum() == 1 and np.isinf(n_a).sum() == 1 and (n_b < 0).sum() == 1 and bad.sum() == 3
    assert np.isnan(frame[..., 0:3]).sum() == 1 and np.isinf(acc[..., 0:3]).sum() == 1
    m2_a, m2_b = acc[..., mo_a:mo_a + 3], frame[..., mo_b:mo_b + 3]
    assert (pool & (m2_a == 0).all(-1) & (m2_b == 0).all(-1)).any() and (m2_b < 0).sum() == 1
    for f in (acc, frame):
        pos = f[..., 0:3][np.isfinite(f[..., 0:3]) & (f[..., 0:3] > 0)]
        assert np.log10(pos.max() / pos.min()) >= 9
    assert (pool & (acc[..., 0:3] == frame[..., 0:3]).all(-1)).any()  # d == 0
    N_b = frame[..., no_b:no_b + 3]
    zero, some = (N_b == 0).all(-1), (N_b == 0).any(-1)
    assert (pool & zero).any() and (pool & some & ~zero).any() and (pool & ~some).any()
    # a frame film without "samples": every n_b is spp_b, and the bad counts are all acc's
    acc2, frame2, oa, ob = ac.synthetic_films((29, 37), 3, False, False)
    n_a, n_b, bad, skip, copy, pool = ac.counts(acc2, frame2, oa, ob, 8)
    assert (n_b == 8).all() and bad.sum() == 3 and not skip.any() and copy.sum() == 2
    # and a film too small for the special pixels is ordinary pixels
    acc3, frame3, oa, ob = ac.synthetic_films((1, 9), 4, True, True)
    assert ac.counts(acc3, frame3, oa, ob, 0)[5].all()


# ---- 4. exact pooling ------------------------------------------------------------------------------------------------------------------------
def integer_parts(npix=300, seed=1):
    """integer samples in [0, 64], 32 per pixel and colour -> x (npix, 3, 32) int64"""
    return np.random.default_rng(seed).integers(0, 65, (npix, 3, 32))


def exact_film(x, samples_channel):
    """the film (npix, 6 or 7) of the samples x (npix, 3, n), n a power of two: V = sum / n and m2 = (n * sum of squares - sum^2) / n^3, both exact
    in fp32 for integer samples in [0, 64] and n <= 32 (the numerator is below 32 * 32 * 4096 = 2^22)"""
    n = x.shape[-1]
    s1, s2 = x.sum(-1), (x * x).sum(-1)
    V, m2 = s1 / D(n), (n * s2 - s1 * s1) / D(n ** 3)
    assert (V.astype(F).astype(D) == V).all() and (m2.astype(F).astype(D) == m2).all()
    film = np.zeros((x.shape[0], 7 if samples_channel else 6), F)
    film[:, 0:3] = V; film[:, 3:6] = m2
    if samples_channel:
        film[:, 6] = n
    return film


OFFS_A, OFFS_B = (0, 3, 6), (0, 3, 0)  # 3 components, no normals: the accumulator has 7 floats, a uniform frame film 6


def chain(parts, pool=ac.accumulate):
    acc = np.zeros((parts[0].shape[0], 7), F)
    for x in parts:
        acc = pool(acc, exact_film(x, False), OFFS_A, OFFS_B, x.shape[-1])
    return acc


def test_exact_pooling_is_the_whole_sets_statistic_bit_for_bit():
    """4 | 4 | 8 | 16 of 32 integer samples, in this order and in the other association (16 first): every intermediate of the rule is exact, so the pooled film is
    the whole set's (V, m2, 32) to the bit.  (a + b) / 2 and "add the m2s" both fail this."""
    x = integer_parts()
    whole = exact_film(x, True)
    cuts = [x[..., 0:4], x[..., 4:8], x[..., 8:16], x[..., 16:32]]
    assert bits_equal(chain(cuts), whole)
    # the other association, the 16 first: 16 + ((4 + 4) + 8), the pooled sixteen coming in as a film with its own "samples" (every count stays
    # a power of two, which is what keeps the divisions exact)
    assert bits_equal(ac.accumulate(chain(cuts[3:]), chain(cuts[:3]), OFFS_A, OFFS_A), whole)
    assert (whole[:, 3:6] > 0).all()

    def averaged(acc, frame, offs_a, offs_b, spp_b):  # the two wrong rules, for the record that this test tells them apart
        if not acc.any():
            return ac.accumulate(acc, frame, offs_a, offs_b, spp_b)
        out = acc.copy()
        out[:, 0:6] = (acc[:, 0:6] + frame[:, 0:6]) / F(2)
        out[:, 6] = acc[:, 6] + spp_b
        return out

    def added(acc, frame, offs_a, offs_b, spp_b):  # Chan's rule without the term in d
        out = ac.accumulate(acc, frame, offs_a, offs_b, spp_b)
        n_a, n = acc[:, 6:7].astype(D), out[:, 6:7].astype(D)
        if n_a.any():
            out[:, 3:6] = ((acc[:, 3:6].astype(D) * n_a * n_a + frame[:, 3:6].astype(D) * spp_b * spp_b) / n / n).astype(F)
        return out
    assert not bits_equal(chain(cuts, averaged)[:, 0:6], whole[:, 0:6]) and not bits_equal(chain(cuts, added)[:, 3:6], whole[:, 3:6])
    assert bits_equal(chain(cuts, added)[:, 0:3], whole[:, 0:3])


# ---- 5. general counts -----------------------------------------------------------------------------------------------------------------------
def two_pass(x):
    """-> (V, m2) f64 of the samples x (..., n): the mean and the centred sum of squares over n^2, two passes in binary64"""
    n = x.shape[-1]
    mean = x.sum(-1) / n
    return mean, ((x - mean[..., None]) ** 2).sum(-1) / (n * n)


def test_general_counts_against_the_two_pass_statistic():
    """5 | 11 | 3 real-valued samples per pixel and colour, each part's (V, m2) rounded to fp32 and pooled by the model, against the two-pass
    statistic of the 19 samples in binary64.  With u = 2^-24 (an fp32 rounding), X = the largest |sample| of the pixel and colour, n = 19, and
    binary64's own roundings (2^-53) left to the slack in the factors:
      V   every part's V is off by at most u X; a pooled V is a weighted mean of its inputs, so it inherits at most u X from them and adds
          u X by its own rounding, twice in this chain:                                   |V - V_ref| <= 3 u X, asserted as 4 u X.
      m2  = Q / n^2.  The parts' own Q_i carry m2_i's relative error u, and each of the two pooled m2 is rounded once more: a relative
          error of at most 3 u in all on the within-part share of m2, asserted as 4 u m2_ref.  The between-part term (d^2 n_a n_b / n) / n^2
          takes d = V_b - V_a with |d| <= 2 X and an error of at most 2 * 3 u X, so d^2 is off by at most 2 * 2 X * 6 u X = 24 u X^2, and with
          n_a n_b <= n^2 / 4 the term is off by at most 6 u X^2 / n per pooling, 12 u X^2 / n for the two:
                                                                                           |m2 - m2_ref| <= 4 u m2_ref + 12 u X^2 / n."""
    rng = np.random.default_rng(2)
    npix, cuts = 400, (5, 11, 3)
    x = rng.uniform(0.0, 1.0, (npix, 3, 19)) * 10.0 ** rng.integers(-4, 5, (npix, 1, 1))
    x[:40] = x[:40, :, :1] + 1e-3 * x[:40]  # nearly equal samples: m2 far below V^2
    acc = np.zeros((npix, 7), F)
    at = 0
    for k in cuts:
        V, m2 = two_pass(x[..., at:at + k])
        film = np.zeros((npix, 6), F)
        film[:, 0:3] = V; film[:, 3:6] = m2
        acc = ac.accumulate(acc, film, OFFS_A, OFFS_B, k)
        at += k
    V_ref, m2_ref = two_pass(x)
    u, X, n = D(2.0) ** -24, np.abs(x).max(-1), D(19)
    err_V = np.abs(acc[:, 0:3].astype(D) - V_ref) / (u * X)
    err_m2 = np.abs(acc[:, 3:6].astype(D) - m2_ref) / (4 * u * m2_ref + 12 * u * X * X / n)
    print(f"general counts: |V - V_ref| up to {err_V.max():.3f} u X (bound 4); m2's error up to {err_m2.max():.3f} of its bound")
    assert (acc[:, 6] == 19).all()
    assert (err_V <= 4).all() and (err_m2 <= 1).all()


# ---- 6. identities of the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc,normals,frame_samples", [(4, True, True), (3, False, False), (4, True, False)])
def test_accumulating_into_zeros_is_the_copy(pc, normals, frame_samples):
    _, frame, offs_a, offs_b = ac.synthetic_films((9, 11), pc, normals, frame_samples)
    frame = np.where(np.isfinite(frame), frame, F(1.0))
    if offs_b[2]:
        frame[..., offs_b[2]] = np.abs(frame[..., offs_b[2]]) + 2
    xa = ac.layout(pc, normals, True)[0]
    out = ac.accumulate(np.zeros(frame.shape[:2] + (xa,), F), frame, offs_a, offs_b, 8)
    assert bits_equal(out[..., 0:3], frame[..., 0:3]) and bits_equal(out[..., offs_a[1]:offs_a[1] + 3], frame[..., offs_b[1]:offs_b[1] + 3])
    assert bits_equal(out[..., offs_a[2]], frame[..., offs_b[2]] if offs_b[2] else np.full(frame.shape[:2], 8, F))
    if normals:
        assert bits_equal(out[..., offs_a[0]:offs_a[0] + 3], frame[..., offs_b[0]:offs_b[0] + 3])
    if pc == 4:
        assert not out[..., 3].any()  # the fourth component stays acc's


def test_an_empty_frame_pixel_leaves_acc_alone_and_a_nan_stays_in_its_pixel():
    acc, frame, offs_a, offs_b = ac.synthetic_films((29, 37), 4, True, True)
    out = ac.accumulate(acc, frame, offs_a, offs_b)
    n_a, n_b, bad, skip, copy, pool = ac.counts(acc, frame, offs_a, offs_b, 0)
    assert skip.sum() == 2 and bits_equal(out[skip], acc[skip])
    mo, so = offs_a[1], offs_a[2]
    ours = [0, 1, 2, mo, mo + 1, mo + 2, so]
    rest = [c for c in range(acc.shape[-1]) if c not in ours]
    assert np.isnan(out[bad][:, ours]).all() and bits_equal(out[bad][:, rest], acc[bad][:, rest])
    assert bits_equal(out[..., 3], acc[..., 3])
    # a pixel that held no NaN and no bad count holds none afterwards; one non-finite colour poisons its own pixel's colour alone
    clean = ~bad & np.isfinite(acc).all(-1) & np.isfinite(frame).all(-1)
    assert np.isfinite(out[clean]).all() and clean.sum() == acc.shape[0] * acc.shape[1] - 5
    y, x = np.argwhere(np.isnan(frame[..., 1]))[0]
    assert np.isnan(out[y, x, 1]) and np.isnan(out[y, x, mo + 1]) and np.isfinite(out[y, x, [0, 2, mo, mo + 2]]).all()
    other = frame.copy(); other[y, x, 1] = 0.5
    out2 = ac.accumulate(acc, other, offs_a, offs_b)
    mask = np.ones(acc.shape[:2], bool); mask[y, x] = False
    assert ac.same(out[mask], out2[mask]) and np.isfinite(out2[y, x, 0:3]).all()
    # the normals: the frame's where it has a non-zero one, acc's elsewhere
    no_a, no_b = offs_a[0], offs_b[0]
    hit = (copy | pool) & (frame[..., no_b:no_b + 3] != 0).any(-1)
    assert bits_equal(out[hit][:, no_a:no_a + 3], frame[hit][:, no_b:no_b + 3]) and bits_equal(out[~hit][:, no_a:no_a + 3], acc[~hit][:, no_a:no_a + 3])
    assert (~hit & pool).any()


def test_pooling_a_film_with_itself_keeps_v_and_halves_m2():
    """n_a = n_b = n, an integer up to 64: d = 0, Q = 2 m2 n^2 exactly, (2 m2 n^2) / (2 n) = m2 n exactly (representable, so the correctly
    rounded quotient is it), and (m2 n) / (2 n) = m2 / 2 exactly; m2 is kept clear of fp32's subnormals"""
    rng = np.random.default_rng(3)
    film = np.zeros((500, 7), F)
    film[:, 0:3] = rng.uniform(0, 3, (500, 3)) * 10.0 ** rng.integers(-5, 6, (500, 1))
    film[:, 3:6] = rng.uniform(1e-20, 1e3, (500, 3))
    film[:, 6] = rng.integers(1, 65, 500)
    out = ac.accumulate(film, film, OFFS_A, OFFS_A)
    assert bits_equal(out[:, 0:3], film[:, 0:3]) and bits_equal(out[:, 3:6], film[:, 3:6] / F(2)) and bits_equal(out[:, 6], film[:, 6] * F(2))


# ---- 7. the summary ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau,floor", [(0.0, 0.0), (0.05, 0.01), (0.3, 0.0), (1e9, 1.0)])
def test_summary_counters_are_a_plain_loop_over_the_pixels(tau, floor):
    import math
    acc, frame, offs_a, offs_b = ac.synthetic_films((29, 37), 4, True, True)
    film = ac.accumulate(acc, frame, offs_a, offs_b)
    _, mo, so = offs_a
    pixels = invalid = converged = samples = 0
    t, a = float(F(tau)), float(F(floor))
    for px in film.reshape(-1, film.shape[-1]).astype(D).tolist():
        pixels += 1
        V, m2, n = px[0:3], px[mo:mo + 3], px[so]
        if not (all(math.isfinite(v) for v in V + m2 + [n]) and all(m >= 0 for m in m2) and n >= 2):
            invalid += 1
            continue
        samples += int(min(n, 2.0 ** 53))
        q = n / (n - 1.0)
        if all(m2[c] * q <= (t * (abs(V[c]) + a)) ** 2 for c in range(3)):
            converged += 1
    got = ac.summary(film, offs_a, tau, floor)
    assert got == {"pixels": pixels, "invalid": invalid, "converged": converged, "samples": samples % (1 << 64)}
    assert pixels == 29 * 37 and invalid >= 6
    if tau == 0.0:
        m2 = film[..., mo:mo + 3]
        valid, _ = ac.valid_pixels(film, offs_a)
        assert converged == int((valid & (m2 == 0).all(-1)).sum()) >= 1
    if tau == 1e9:
        assert converged == pixels - invalid
    if tau == 0.3:
        assert 0 < converged < pixels - invalid


# ---- 8. the oracle's films ---------------------------------------------------------------------------------------------------------------------
SPP, DEPTH = 8, 4


def moments_of(y):
    """the m2 channel of a one-pass frame from its per-sample films y (H, W, S, 3) f32: the rule of phx_frame.moments_channel"""
    f = np.zeros(y.shape[:2] + (3,), F); mean = np.zeros(f.shape, D); M2 = np.zeros(f.shape, D)
    for k in range(y.shape[2]):
        ys = y[:, :, k, :]
        f = (f + ys).astype(F)
        yd = ys.astype(D)
        d = yd - mean
        mean = mean + d * (D(1.0) / D(k + 1))
        M2 = M2 + d * (yd - mean)
    return f, M2.astype(F)


def oracle_film(orc, scene, seed):
    """-> the oracle's frame of SPP samples at `seed` as a film with the m2 channel (H, W, 7) f32: primary rgba, m2"""
    orc.set_tie_rule(True)
    try:
        O = orc.Oracle(scene, spp=SPP, pps=1, depth=DEPTH)
        kw = dict(rng=orc.RNG_COUNTER, seed=seed, threads=4)
        y = np.stack([O.render(sample_begin=s, sample_end=s + 1, **kw)[0][..., :3] for s in range(SPP)], axis=2)
        whole = O.render(**kw)[0]
        O.close()
    finally:
        orc.set_tie_rule(False)
    f, m2 = moments_of(np.ascontiguousarray(y))
    assert bits_equal(f, whole[..., :3])  # the per-sample films add up to the frame
    film = np.zeros(f.shape[:2] + (7,), F)
    film[..., 0:3] = f; film[..., 3] = whole[..., 3]; film[..., 4:7] = m2
    return film


def test_oracle_films_of_two_seeds_pool_to_their_mean(orc):
    """a 16 x 12 cornell box of frame_cases, 8 spp at seeds 1 and 2: n_a = n_b, so the rule's V is (V_a + V_b) / 2 formed exactly in binary64 and
    rounded to fp32 once; the pooled variance estimate is finite and >= 0 wherever both frames' are"""
    from phosphorus_mk2_amd import xpu
    scene = FC.SCENES["cornell"](16, 12)
    a, b = oracle_film(orc, scene, 1), oracle_film(orc, scene, 2)
    assert not bits_equal(a[..., 0:3], b[..., 0:3])
    offs_a, offs_b = ac.layout(4, False, True)[1:], ac.layout(4, False, False)[1:]
    acc = ac.accumulate(xpu.accumulator(16, 12), a, offs_a, offs_b, SPP)
    assert bits_equal(acc[..., [0, 1, 2, 4, 5, 6]], a[..., [0, 1, 2, 4, 5, 6]]) and (acc[..., 7] == SPP).all() and not acc[..., 3].any()
    acc = ac.accumulate(acc, b, offs_a, offs_b, SPP)
    assert bits_equal(acc[..., 0:3], ((a[..., 0:3].astype(D) + b[..., 0:3].astype(D)) / D(2)).astype(F)) and (acc[..., 7] == 2 * SPP).all()
    va, vb = xpu.film_variance(a, SPP), xpu.film_variance(b, SPP)
    v = xpu.film_variance(acc, 0, adaptive=True)
    fine = np.isfinite(va) & np.isfinite(vb) & (va >= 0) & (vb >= 0)
    assert fine.all() and np.isfinite(v[fine]).all() and (v[fine] >= 0).all() and (v > 0).any()
    s = ac.summary(acc, offs_a, 0.5, 0.01)
    assert s["pixels"] == 16 * 12 and s["invalid"] == 0 and s["samples"] == 16 * 12 * 2 * SPP and 0 < s["converged"] <= s["pixels"]
