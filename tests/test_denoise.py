"""The film denoiser (phx_denoise) without a GPU: the ABI and the header's text, every refusal of the argument check
(csrc/denoise_check.cpp through tests/native/host_denoise.cpp), the exact properties of the float64 model (tests/denoise64.py), its variance
output on an iid film, and what it does to the oracle's films.  The device is held to the same model bit for bit in tests/test_gpu_denoise.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise64 as dn
import native_lib as NL
from conftest import bits_equal
from native_lib import ERR_ARG

F, D = np.float32, np.float64


# ---- 1. the ABI and the header ------------------------------------------------------------------------------------------------------------
FIELDS = ["width", "height", "xstride", "normals_offset", "m2_offset", "samples_offset", "spp", "iterations", "sigma_l", "normal_power_log2",
          "on_device", "reserved"]


def test_struct_size_and_field_offsets():
    from phosphorus_mk2_amd import abi
    assert C.sizeof(abi.Denoise) == 64
    assert [f for f, _ in abi.Denoise._fields_] == FIELDS
    assert [getattr(abi.Denoise, f).offset for f in FIELDS] == [4 * i for i in range(12)]
    assert abi.Denoise.sigma_l.size == 4 and abi.Denoise.reserved.size == 20
    assert "phx_dev_denoise" in abi.EXPORTS


def test_struct_size_is_the_librarys():
    from phosphorus_mk2_amd import abi, xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = xpu.load_library()
    assert lib.phx_abi_sizeof(13) == C.sizeof(abi.Denoise) == 64
    # the earlier indices stay (10 and 11 were taken before this struct; 12 is pinned to 0 by tests/test_adaptive_sampling.py)
    assert lib.phx_abi_sizeof(10) == C.sizeof(abi.Texture) and lib.phx_abi_sizeof(11) == C.sizeof(abi.Adaptive) and lib.phx_abi_sizeof(12) == 0
    assert lib.phx_abi_sizeof(14) == 0


def test_header_states_the_struct_and_the_rule():
    hdr, body = NL.header(), NL.struct_body("phx_denoise", strip_comments=False)
    assert re.findall(r"\b(\w+)(?:\[5\])?;", NL.struct_body("phx_denoise")) == ["height", "xstride", "normals_offset", "m2_offset", "samples_offset", "spp", "iterations",
                                                       "sigma_l", "normal_power_log2", "on_device", "reserved"]
    assert re.search(r"uint32_t\s+width,\s*height;", body)
    assert re.search(r"int\s+phx_dev_denoise\(phx_device\* dev, const phx_denoise\* d, const float\* film_in, float\* film_out\);", hdr)
    rule = hdr[hdr.index("film denoiser (DESIGN 18)"):hdr.index("typedef struct phx_denoise")]
    flat = NL.flat(rule)
    for phrase in ["V_c = fp32(m2_c (n / (n - 1)))", "(0.2126 C_r + 0.7152 C_g) + 0.0722 C_b", "(0.2126 sqrt(V_r) + 0.7152 sqrt(V_g)) + 0.0722 sqrt(V_b)",
                   "k3 = (1/4, 1/2, 1/4)", "k5 = (1/16, 1/4, 3/8, 1/4, 1/16)", "sig = sigma_l sqrt(S_p)", "d = d > 0 ? d : 0",
                   "u = fabs(l_q - l_p) / sig", "w_l = u < 1 ? t t : 0", "w = (h w_n) w_l", "A_c += w (C_q,c - C_p,c)", "B_c += (w w) V_q,c",
                   "fp32(C_p,c + A_c / W)", "fp32(B_c / (W W))", "fp32(V_c ((n - 1) / n))", "iterations == 0 copies the film",
                   "dy = -2 .. 2 outer", "dy = -1 .. 1 outer", "binary64, without contraction", "understates the true error",
                   "must be reduced before the call"]:
        assert " ".join(phrase.split()) in flat, phrase


@pytest.mark.parametrize("pc", [3, 4])
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("adaptive", [False, True])
def test_python_offsets_are_the_films(pc, normals, adaptive):
    from phosphorus_mk2_amd import xpu
    film = xpu.Film(7, 5, pc, normals, True, adaptive)
    q = xpu.denoise_settings(film.data.shape, 16, pc, normals, adaptive)
    assert (q.width, q.height, q.xstride) == (7, 5, film.xstride)
    assert q.m2_offset == film.m2_offset and q.normals_offset == (pc if normals else 0)
    assert q.samples_offset == (film.samples_offset if adaptive else 0)
    assert (q.xstride, q.normals_offset, q.m2_offset, q.samples_offset) == dn.layout(pc, normals, adaptive)
    assert (q.spp, q.iterations, q.sigma_l, q.normal_power_log2, q.on_device, list(q.reserved)) == (16, 5, 4.0, 7, 0, [0] * 5)
    no_m2 = xpu.Film(7, 5, pc, normals, False, False)
    with pytest.raises(ValueError, match="moments=True"):
        xpu.denoise_settings(no_m2.data.shape, 16, pc, normals, adaptive)


def test_render_refuses_denoise_without_moments():
    from phosphorus_mk2_amd import scenes, xpu
    with pytest.raises(ValueError, match="moments=True"):
        xpu.render(scenes.cornell(32, 32), spp=2, denoise={})


# ---- 2. the refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check():
    """the host_denoise library: (abi.Denoise, film_in address, film_out address) -> (status, message)"""
    from phosphorus_mk2_amd import abi
    lib = NL.load("host_denoise")
    hd_check = NL.checker(lib, "hd_check", [C.POINTER(abi.Denoise), C.c_void_p, C.c_void_p])
    lib.hd_sizeof.restype = C.c_uint32
    assert lib.hd_sizeof() == C.sizeof(abi.Denoise)
    return lambda q, film_in=0x10000, film_out=0x10000: hd_check(C.byref(q), film_in, film_out)


def good(**kw):
    from phosphorus_mk2_amd import abi
    q = abi.Denoise(width=64, height=48, xstride=11, normals_offset=4, m2_offset=7, samples_offset=10, spp=16, iterations=5, sigma_l=4.0,
                    normal_power_log2=7, on_device=0)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


ACCEPTED = [dict(), dict(width=1, height=1), dict(width=65536, height=65536), dict(normals_offset=0), dict(samples_offset=0), dict(iterations=0),
            dict(iterations=8), dict(normal_power_log2=0), dict(normal_power_log2=10), dict(on_device=1), dict(spp=2), dict(sigma_l=1e-30),
            dict(xstride=6, normals_offset=0, m2_offset=3, samples_offset=0), dict(xstride=12, normals_offset=9, m2_offset=3, samples_offset=6)]
REFUSED = [("width", dict(width=0)), ("width", dict(width=65537)), ("height", dict(height=0)), ("height", dict(height=65537)),
           ("xstride", dict(xstride=5)), ("xstride", dict(xstride=0)),
           ("m2_offset", dict(m2_offset=0)), ("m2_offset", dict(m2_offset=2)), ("m2_offset", dict(m2_offset=9)), ("m2_offset", dict(m2_offset=0xfffffffe)),
           ("normals_offset", dict(normals_offset=2)), ("normals_offset", dict(normals_offset=9)), ("normals_offset", dict(normals_offset=5)),
           ("normals_offset", dict(normals_offset=7)), ("normals_offset", dict(normals_offset=0xffffffff)),
           ("samples_offset", dict(samples_offset=2)), ("samples_offset", dict(samples_offset=11)), ("samples_offset", dict(samples_offset=8)),
           ("samples_offset", dict(samples_offset=5)), ("samples_offset", dict(samples_offset=0xffffffff)),
           ("spp", dict(spp=0)), ("spp", dict(spp=1)), ("iterations", dict(iterations=9)),
           ("sigma_l", dict(sigma_l=0.0)), ("sigma_l", dict(sigma_l=-1.0)), ("sigma_l", dict(sigma_l=float("nan"))), ("sigma_l", dict(sigma_l=float("inf"))),
           ("normal_power_log2", dict(normal_power_log2=11)), ("on_device", dict(on_device=2))]


@pytest.mark.parametrize("kw", ACCEPTED, ids=NL.case_ids(ACCEPTED))
def test_check_accepts(check, kw):
    assert check(good(**kw)) == (0, "")


@pytest.mark.parametrize("field,kw", REFUSED, ids=NL.case_ids(kw for _, kw in REFUSED))
def test_check_refuses_and_names_the_field(check, field, kw):
    rc, msg = check(good(**kw))
    assert rc == ERR_ARG and re.search(rf"\b{field}\b", msg), (rc, msg)


def test_check_refuses_reserved_words_and_bad_films(check):
    for i in range(5):
        q = good()
        q.reserved[i] = 1
        rc, msg = check(q)
        assert rc == ERR_ARG and "reserved" in msg
    q = good()
    nbytes = 64 * 48 * 11 * 4
    assert check(q, 0, 0x10000)[0] == ERR_ARG and "film_in" in check(q, 0, 0x10000)[1]
    assert check(q, 0x10000, 0)[0] == ERR_ARG and "film_out" in check(q, 0x10000, 0)[1]
    assert check(q, 0x10000, 0x10000 + nbytes) == (0, "") and check(q, 0x10000 + nbytes, 0x10000) == (0, "")  # two films back to back
    for a, b in ((0x10000, 0x10000 + nbytes - 4), (0x10000 + nbytes - 4, 0x10000), (0x10000, 0x10004)):
        rc, msg = check(q, a, b)
        assert rc == ERR_ARG and "film_out" in msg, (a, b, msg)


def test_the_check_under_the_sanitizers(tmp_path):
    """host_denoise.cpp's own main() under AddressSanitizer and UBSan: its cases get the answers above, and the program ends without a report"""
    stdout = NL.run_sanitized(tmp_path, "host_denoise", "HOST_DENOISE_MAIN")
    got = {l.split()[0]: (int(l.split()[1]), l) for l in stdout.splitlines()}
    want = {"good": None, "in-place": None, "overlap": "film_out", "null-in": "film_in", "null-out": "film_out", "width": "width", "height": "height",
            "xstride": "xstride", "m2-wrap": "m2_offset", "normals-overlap": "normals_offset", "samples-past": "samples_offset", "spp": "spp",
            "iterations": "iterations", "sigma-nan": "sigma_l", "power": "normal_power_log2", "on-device": "on_device", "reserved": "reserved"}
    assert sorted(got) == sorted(want)
    for name, field in want.items():
        rc, line = got[name]
        assert (rc == 0) if field is None else (rc == ERR_ARG and field in line), line


# ---- 3. exact properties of the model ------------------------------------------------------------------------------------------------------
def run(film, offs, spp=16, **kw):
    return dn.denoise(film, spp, *offs, **kw)


def clean_film(h, w, seed, normals=True, adaptive=False):
    """a synthetic film without the special pixels: every pixel valid"""
    rng = np.random.default_rng(seed)
    xstride, no, mo, so = dn.layout(4, normals, adaptive)
    film = np.zeros((h, w, xstride), F)
    film[..., 0:4] = rng.uniform(0.1, 1.0, (h, w, 4))
    film[..., mo:mo + 3] = rng.uniform(0.0, 0.02, (h, w, 3))
    if normals:
        film[..., no + 2] = 1.0
    if adaptive:
        film[..., so] = rng.integers(2, 17, (h, w))
    return film, (no, mo, so)


def test_zero_iterations_is_the_identity():
    film, offs = dn.synthetic_film(9, 11, 4, True, True)
    assert bits_equal(run(film, offs, iterations=0), film)


def test_zero_m2_is_the_identity():
    film, offs = clean_film(9, 11, 1)
    film[..., offs[1]:offs[1] + 3] = 0
    for it in (1, 5):
        assert bits_equal(run(film, offs, iterations=it), film)


def test_constant_film_keeps_primary_exactly():
    film, offs = clean_film(12, 13, 2)
    film[..., 0:3] = np.array([0.3, 0.7, 0.1], F)
    out = run(film, offs)
    assert bits_equal(out[..., 0:3], film[..., 0:3])
    assert (out[..., offs[1]:offs[1] + 3] < film[..., offs[1]:offs[1] + 3]).mean() > 0.9  # and the variance estimate drops
    untouched = [c for c in range(film.shape[-1]) if c >= 3 and not offs[1] <= c < offs[1] + 3]
    assert bits_equal(out[..., untouched], film[..., untouched])


def cross_weights(film, offs, left, iterations=5):
    """-> the largest weight of a tap between the columns `left` and the others, over all pixels, taps and iterations"""
    C, V, N, valid, n = dn.init_state(film, 16, *offs)
    side = np.zeros(film.shape[:2], bool); side[:, left] = True
    worst = 0.0
    for i in range(iterations):
        weights = []
        C, V = dn.iterate(C, V, N, valid, 1 << i, 4.0, 7, weights)
        for dy, dx, ok, w in weights:
            inside, other = dn._gather(side, (1 << i) * dx, (1 << i) * dy)
            cross = ok & inside & (other != side)
            if cross.any():
                worst = max(worst, float(np.abs(w[cross]).max()))
    return worst


def test_orthogonal_normals_do_not_mix():
    """Two half-films with orthogonal normals.  No tap crosses the edge with a weight other than exactly 0, in any iteration; after ONE
    iteration changing one half's colours changes no bit of the other half.  (From the second iteration on the halves are coupled through the
    yardstick alone: the 3 x 3 of e is taken over every valid neighbour, whatever its normal, and e then depends on the first iteration's
    weights.  Colour still never crosses.)"""
    film, offs = clean_film(10, 16, 3)
    no = offs[0]
    film[:, 8:, no:no + 3] = np.array([1.0, 0.0, 0.0], F)  # right half faces x, left half z
    other = film.copy()
    other[:, 8:, 0:3] = np.random.default_rng(4).uniform(5.0, 9.0, (10, 8, 3))
    a, b = run(film, offs, iterations=1), run(other, offs, iterations=1)
    assert bits_equal(a[:, :8], b[:, :8]) and not bits_equal(a[:, 8:], b[:, 8:])
    assert not bits_equal(a[:, :8, 0:3], film[:, :8, 0:3])  # the left half WAS filtered
    assert cross_weights(film, offs, slice(0, 8)) == 0.0 and cross_weights(other, offs, slice(0, 8)) == 0.0
    # five iterations: the left half's colours stay inside the range of the left half's own input
    five = run(other, offs)
    assert five[:, :8, 0:3].max() <= film[:, :8, 0:3].max() and five[:, 8:, 0:3].min() >= other[:, 8:, 0:3].min()


def test_missed_half_mixes_with_itself_only():
    """a half whose camera rays missed (zero normals) and a half that was hit: as for orthogonal normals, and the missed half does mix (w_n = 1)"""
    film, offs = clean_film(10, 16, 5)
    no = offs[0]
    film[:, 8:, no:no + 3] = 0.0  # the camera rays of the right half missed
    other = film.copy()
    other[:, 8:, 0:3] = np.random.default_rng(6).uniform(5.0, 9.0, (10, 8, 3))
    a, b = run(film, offs, iterations=1), run(other, offs, iterations=1)
    assert bits_equal(a[:, :8], b[:, :8]) and not bits_equal(a[:, 8:], b[:, 8:])
    assert not bits_equal(a[:, 8:, 0:3], film[:, 8:, 0:3])  # missed pixels mix among themselves
    swapped = film.copy()
    swapped[:, :8, 0:3] = np.random.default_rng(7).uniform(5.0, 9.0, (10, 8, 3))
    assert bits_equal(run(swapped, offs, iterations=1)[:, 8:], a[:, 8:])
    assert cross_weights(film, offs, slice(0, 8)) == 0.0 and cross_weights(swapped, offs, slice(0, 8)) == 0.0


@pytest.mark.parametrize("what", ["nan", "inf", "negative-m2", "one-sample", "nan-normal", "inf-m2"])
def test_an_invalid_pixel_is_untouched_and_invisible(what):
    film, offs = clean_film(9, 10, 8, adaptive=True)
    no, mo, so = offs
    y, x = 4, 5
    bad = film.copy()
    if what == "nan":
        bad[y, x, 0] = np.nan
    elif what == "inf":
        bad[y, x, 2] = np.inf
    elif what == "negative-m2":
        bad[y, x, mo + 1] = -1e-6
    elif what == "one-sample":
        bad[y, x, so] = 1.0
    elif what == "nan-normal":
        bad[y, x, no] = np.nan
    else:
        bad[y, x, mo] = np.inf
    ref = film.copy()
    ref[y, x, so] = 0.0  # merely invalid: fewer than 2 samples, every other float ordinary
    a, b = run(bad, offs), run(ref, offs)
    assert bits_equal(a[y, x], bad[y, x]) and bits_equal(b[y, x], ref[y, x])
    mask = np.ones(film.shape[:2], bool); mask[y, x] = False
    assert bits_equal(a[mask], b[mask])
    assert not bits_equal(a[mask], run(film, offs)[mask])  # a VALID pixel there does change its neighbours


def test_without_normals_the_normal_weight_is_one():
    film, offs = clean_film(9, 10, 9, normals=True)
    no, mo, _ = offs
    film[..., no:no + 3] = np.random.default_rng(10).standard_normal((9, 10, 3))  # normals that WOULD separate the pixels
    with_n = run(film, offs)
    ignored = dn.denoise(film, 16, 0, mo, 0)  # the same floats, the channel not named
    zeroed = film.copy(); zeroed[..., no:no + 3] = 0.0
    assert bits_equal(ignored[..., 0:3], run(zeroed, offs)[..., 0:3]) and bits_equal(ignored[..., no:no + 3], film[..., no:no + 3])
    assert not bits_equal(ignored[..., 0:3], with_n[..., 0:3])
    assert bits_equal(dn.denoise(film, 16, 0, mo, 0, normal_power_log2=0), ignored)


def test_a_step_past_the_film_leaves_the_centre_tap():
    """iteration 6 has step 64: on a 9-pixel film every tap but the centre is outside, so C stays and V' = V"""
    film, offs = clean_film(1, 9, 11)
    C, V, N, valid, n = dn.init_state(film, 16, *offs)
    C2, V2 = dn.iterate(C, V, N, valid, 64, 4.0, 7)
    assert bits_equal(C2, C) and bits_equal(V2, V)


# ---- 4. V' on an iid film ------------------------------------------------------------------------------------------------------------------
def test_variance_of_one_iteration_on_an_iid_film():
    """V' = (sum of w^2 V_q) / (sum of w)^2, recomputed per pixel in Python floats from the weights the model used"""
    rng = np.random.default_rng(12)
    h, w = 8, 9
    xstride, no, mo, so = dn.layout(3, False, False)
    film = np.zeros((h, w, xstride), F)
    var = 0.01
    film[..., 0:3] = 0.5 + np.sqrt(var) * rng.standard_normal((h, w, 3))
    film[..., mo:mo + 3] = var * (15 / 16) * rng.uniform(0.8, 1.2, (h, w, 3))
    C, V, N, valid, n = dn.init_state(film, 16, no, mo, so)
    assert valid.all()
    weights = []
    C2, V2 = dn.iterate(C, V, N, valid, 1, 4.0, 7, weights)
    assert len(weights) == 25
    for y in range(h):
        for x in range(w):
            sw, swwv = 0.0, [0.0, 0.0, 0.0]
            for dy, dx, ok, wt in weights:
                if ok[y, x]:
                    sw += float(wt[y, x])
                    for c in range(3):
                        swwv[c] += float(wt[y, x]) ** 2 * float(V[y + dy, x + dx, c])
            want = np.array([s / (sw * sw) for s in swwv], D).astype(F)
            assert bits_equal(V2[y, x], want), (y, x)
    # the filter averages: well inside the film the estimate is a fraction of the input's
    assert (V2[2:-2, 2:-2] < 0.5 * V[2:-2, 2:-2]).all()


# ---- 5. the oracle's films -----------------------------------------------------------------------------------------------------------------
SPP, DEPTH, SEED, REF_SPP, REF_SEED = 8, 5, 5, 1024, 77


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


def oracle_film(orc, scene):
    """-> (film (H, W, 10) f32: primary rgba, normals, m2 at SPP samples; reference (H, W, 3) at REF_SPP), under the device's tie rule"""
    orc.set_tie_rule(True)
    try:
        O = orc.Oracle(scene, spp=SPP, pps=1, depth=DEPTH)
        kw = dict(rng=orc.RNG_COUNTER, seed=SEED, threads=4)
        y = np.stack([O.render(sample_begin=s, sample_end=s + 1, **kw)[0][..., :3] for s in range(SPP)], axis=2)
        whole, _, nrm = O.render(normals=True, **kw)
        O.close()
        R = orc.Oracle(scene, spp=REF_SPP, pps=1, depth=DEPTH)
        ref = R.render(rng=orc.RNG_COUNTER, seed=REF_SEED, threads=8)[0][..., :3].copy()
        R.close()
    finally:
        orc.set_tie_rule(False)
    f, m2 = moments_of(np.ascontiguousarray(y))
    assert bits_equal(f, whole[..., :3])  # the per-sample films add up to the frame
    film = np.zeros(f.shape[:2] + (10,), F)
    film[..., 0:3] = f; film[..., 3] = whole[..., 3]; film[..., 4:7] = nrm; film[..., 7:10] = m2
    return film, ref


@pytest.mark.parametrize("which,bound", [("cornell", 0.8), ("blobs", 0.4)])
def test_oracle_films_get_closer_to_the_reference(orc, which, bound):
    """8 spp, depth 5, seed 5, 64 x 64 against 1 024 spp, seed 77: MSE denoised / plain below 0.8 (cornell box) and 0.4 (blobs); the
    float64 prototype without the invalid-pixel rule measured 0.552 and 0.176"""
    from phosphorus_mk2_amd import scenes
    scene = scenes.cornell(64, 64) if which == "cornell" else scenes.glass_blobs(64, 64)
    film, ref = oracle_film(orc, scene)
    out = dn.denoise(film, SPP, 4, 7, 0)
    refd = ref.astype(D)
    mse_plain = float(((film[..., 0:3].astype(D) - refd) ** 2).mean())
    mse_den = float(((out[..., 0:3].astype(D) - refd) ** 2).mean())
    shift = float(out[..., 0:3].astype(D).mean() / refd.mean() - 1.0)
    shift_plain = float(film[..., 0:3].astype(D).mean() / refd.mean() - 1.0)
    print(f"denoise {which}: MSE denoised / plain = {mse_den / mse_plain:.3f} ({mse_den:.4g} / {mse_plain:.4g}); film mean vs reference "
          f"{100 * shift:+.2f} % (plain {100 * shift_plain:+.2f} %)")
    assert bits_equal(out[..., 3:7], film[..., 3:7])
    assert mse_den / mse_plain < bound
