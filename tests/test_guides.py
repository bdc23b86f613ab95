"""First-hit guides and the guided denoiser (phx_guides / phx_denoise_guides) without a GPU: the ABI and the header's text, every
refusal of the argument checks (csrc/guides_check.cpp through tests/native/host_guides.cpp), the exact properties of the model
(tests/guides64.py) and its payoff on a synthetic textured film.  The device is held to the same model bit for bit in tests/test_gpu_guides.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise64 as dn
import guides64 as gd
import native_lib as NL
from conftest import bits_equal
from native_lib import ERR_ARG

F, D = np.float32, np.float64


# ---- 1. the ABI and the header ------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_field_offsets():
    from phosphorus_mk2_amd import abi
    assert C.sizeof(abi.Guides) == 32
    assert [(f, getattr(abi.Guides, f).offset) for f, _ in abi.Guides._fields_] == [("sampler_seed", 0), ("samples", 8), ("on_device", 12), ("reserved", 16)]
    assert C.sizeof(abi.DenoiseGuides) == 48
    assert [(f, getattr(abi.DenoiseGuides, f).offset) for f, _ in abi.DenoiseGuides._fields_] == [
        ("guides", 0), ("xstride", 8), ("flags", 12), ("albedo_floor", 16), ("sigma_x", 20), ("plane_scale", 24), ("reserved", 28)]
    assert abi.DenoiseGuides.reserved.size == 16 and abi.Guides.reserved.size == 16
    assert (abi.GUIDE_DEMODULATE, abi.GUIDE_PLANE, abi.GUIDE_FLOATS) == (1, 2, 8) == (gd.DEMODULATE, gd.PLANE, gd.GUIDE_FLOATS)
    assert "phx_dev_render_guides" in abi.EXPORTS and "phx_dev_denoise_guided" in abi.EXPORTS


def test_struct_sizes_are_the_librarys():
    from phosphorus_mk2_amd import abi, xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = xpu.load_library()
    assert lib.phx_abi_sizeof(15) == C.sizeof(abi.Guides) == 32
    assert lib.phx_abi_sizeof(16) == C.sizeof(abi.DenoiseGuides) == 48
    assert lib.phx_abi_sizeof(13) == C.sizeof(abi.Denoise) and lib.phx_abi_sizeof(12) == 0 and lib.phx_abi_sizeof(14) == 0 and lib.phx_abi_sizeof(17) == 0
    assert hasattr(lib, "phx_dev_render_guides") and hasattr(lib, "phx_dev_denoise_guided")


def test_header_states_the_structs_and_the_rules():
    hdr = NL.header()
    assert re.findall(r"\b(\w+)(?:\[4\])?;", NL.struct_body("phx_guides")) == ["sampler_seed", "samples", "on_device", "reserved"]
    assert re.findall(r"\b(\w+)(?:\[4\])?;", NL.struct_body("phx_denoise_guides")) == ["guides", "xstride", "flags", "albedo_floor", "sigma_x", "plane_scale", "reserved"]
    assert re.search(r"enum \{ PHX_GUIDE_DEMODULATE = 1, PHX_GUIDE_PLANE = 2 \};", hdr)
    assert re.search(r"int\s+phx_dev_render_guides\(phx_device\* dev, const phx_guides\* g, float\* film", hdr)
    assert re.search(r"int\s+phx_dev_denoise_guided\(phx_device\* dev, const phx_denoise\* d, const phx_denoise_guides\* g, const float\* film_in, float\* film_out\);", hdr)
    rule = hdr[hdr.index("first-hit guide channels (DESIGN 19)"):hdr.index("typedef struct phx_denoise_guides")]
    flat = NL.flat(rule)
    for phrase in ["X_c = o_c + t d_c", "albedo_sum_c (1.0f / (float)G)", "(float)hits (1.0f / (float)G)", "X_sum_c / (float)hits, or 0 when hits == 0",
                   "t_sum / (float)hits, or 0 when hits == 0", "contribute (1, 1, 1)", "fp32 without contraction", "in lobe order",
                   "D_c = max((double)albedo_c, (double)albedo_floor)", "C_c = fp32(primary_c / D_c)", "V_c = fp32((m2_c (n / (n - 1))) / (D_c D_c))",
                   "primary_c = fp32(C_c D_c)", "m2_c = fp32(((V_c D_c) D_c) ((n - 1) / n))", "w = ((h w_n) w_l) w_x",
                   "r = (N_x dX_x + N_y dX_y) + N_z dX_z", "tol = (sigma_x plane_scale) distance_p", "u = fabs(r) / tol", "w_x = u < 1 ? t t : 0",
                   "w_x = (r == 0 ? 1 : 0) when tol == 0", "8 guide floats to be finite", "flags == 0 is phx_dev_denoise bit for bit",
                   "not what it reflects"]:
        assert " ".join(phrase.split()) in flat, phrase


def test_plane_scale_is_the_cameras_pixel():
    """one pixel step on the film moves the camera-space direction by zoom * stepy = 1.12 tan(fov / 2) / H at z = -1 (shade_common.h: camera_ray)"""
    from phosphorus_mk2_amd import scenes, xpu
    cam = scenes.CameraDesc(96, 54, fov=0.9)
    assert xpu.guide_plane_scale(cam) == pytest.approx(1.12 * np.tan(0.45) / 54, rel=1e-12)


# ---- 2. the refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check():
    """the host_guides library -> (check of phx_guides, check of phx_denoise_guides), each -> (status, message)"""
    from phosphorus_mk2_amd import abi
    lib = NL.load("host_guides")
    check_guides = NL.checker(lib, "hg_check_guides", [C.POINTER(abi.Guides), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p])
    check_denoise_guides = NL.checker(lib, "hg_check_denoise_guides", [C.POINTER(abi.Denoise), C.POINTER(abi.DenoiseGuides)])
    lib.hg_sizeof_guides.restype = lib.hg_sizeof_denoise_guides.restype = C.c_uint32
    assert lib.hg_sizeof_guides() == C.sizeof(abi.Guides) and lib.hg_sizeof_denoise_guides() == C.sizeof(abi.DenoiseGuides)
    guides = lambda g, width=64, height=48, spp=16, film=0x10000: check_guides(C.byref(g), width, height, spp, film)
    return guides, lambda d, g: check_denoise_guides(C.byref(d), C.byref(g))


def good_guides(**kw):
    from phosphorus_mk2_amd import abi
    g = abi.Guides(sampler_seed=7, samples=4, on_device=0)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def good_film(**kw):
    from phosphorus_mk2_amd import abi
    d = abi.Denoise(width=64, height=48, xstride=10, normals_offset=4, m2_offset=7, samples_offset=0, spp=16, iterations=5, sigma_l=4.0, normal_power_log2=7)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def good_denoise_guides(**kw):
    from phosphorus_mk2_amd import abi
    g = abi.DenoiseGuides(guides=0x20000, xstride=8, flags=3, albedo_floor=0.01, sigma_x=1.0, plane_scale=0.002)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


NAN, INF = float("nan"), float("inf")
G_ACCEPTED = [dict(), dict(samples=1), dict(samples=16), dict(on_device=1), dict(sampler_seed=2 ** 64 - 1)]
G_REFUSED = [("samples", dict(samples=0)), ("samples", dict(samples=17)), ("samples", dict(samples=0xffffffff)), ("on_device", dict(on_device=2))]
D_ACCEPTED = [dict(), dict(flags=1), dict(flags=2), dict(xstride=8), dict(xstride=4096), dict(albedo_floor=1e-30), dict(flags=2, albedo_floor=NAN),
              dict(flags=1, sigma_x=NAN, plane_scale=-1.0), dict(sigma_x=1e-30), dict(plane_scale=1e30)]
D_REFUSED = [("flags", dict(flags=4)), ("flags", dict(flags=0x80000001)), ("xstride", dict(xstride=7)), ("xstride", dict(xstride=0)),
             ("albedo_floor", dict(albedo_floor=0.0)), ("albedo_floor", dict(albedo_floor=-0.5)), ("albedo_floor", dict(albedo_floor=NAN)),
             ("albedo_floor", dict(albedo_floor=INF)), ("albedo_floor", dict(flags=1, albedo_floor=0.0)),
             ("sigma_x", dict(sigma_x=0.0)), ("sigma_x", dict(sigma_x=-1.0)), ("sigma_x", dict(sigma_x=NAN)), ("sigma_x", dict(sigma_x=INF)),
             ("plane_scale", dict(plane_scale=0.0)), ("plane_scale", dict(plane_scale=-1.0)), ("plane_scale", dict(plane_scale=NAN)),
             ("plane_scale", dict(flags=2, plane_scale=INF)), ("guides", dict(guides=0))]
ids = NL.case_ids


@pytest.mark.parametrize("kw", G_ACCEPTED, ids=ids(G_ACCEPTED))
def test_guides_check_accepts(check, kw):
    assert check[0](good_guides(**kw)) == (0, "")


@pytest.mark.parametrize("field,kw", G_REFUSED, ids=ids([kw for _, kw in G_REFUSED]))
def test_guides_check_refuses_and_names_the_field(check, field, kw):
    rc, msg = check[0](good_guides(**kw))
    assert rc == ERR_ARG and re.search(rf"\b{field}\b", msg) and "phx_guides" in msg, (rc, msg)


def test_guides_check_refuses_reserved_words_a_null_film_and_too_many_paths(check):
    for i in range(4):
        g = good_guides()
        g.reserved[i] = 1
        rc, msg = check[0](g)
        assert rc == ERR_ARG and "reserved" in msg
    rc, msg = check[0](good_guides(), film=0)
    assert rc == ERR_ARG and "film" in msg
    assert check[0](good_guides(samples=1), spp=1) == (0, "")
    assert check[0](good_guides(samples=2), spp=1)[0] == ERR_ARG
    # pixel * samples + sample is a 31-bit path index
    assert check[0](good_guides(samples=16), width=16384, height=8191, spp=16) == (0, "")
    rc, msg = check[0](good_guides(samples=16), width=16384, height=8192, spp=16)
    assert rc == ERR_ARG and "samples" in msg


@pytest.mark.parametrize("kw", D_ACCEPTED, ids=ids(D_ACCEPTED))
def test_denoise_guides_check_accepts(check, kw):
    assert check[1](good_film(), good_denoise_guides(**kw)) == (0, "")


@pytest.mark.parametrize("field,kw", D_REFUSED, ids=ids([kw for _, kw in D_REFUSED]))
def test_denoise_guides_check_refuses_and_names_the_field(check, field, kw):
    rc, msg = check[1](good_film(), good_denoise_guides(**kw))
    assert rc == ERR_ARG and re.search(rf"\b{field}\b", msg) and "phx_denoise_guides" in msg, (rc, msg)


def test_denoise_guides_check_refuses_reserved_words_and_plane_without_normals(check):
    for i in range(4):
        g = good_denoise_guides()
        g.reserved[i] = 1
        rc, msg = check[1](good_film(), g)
        assert rc == ERR_ARG and "reserved" in msg
    no_normals = good_film(normals_offset=0, xstride=7, m2_offset=4)
    rc, msg = check[1](no_normals, good_denoise_guides(flags=2))
    assert rc == ERR_ARG and "normals_offset" in msg
    assert check[1](no_normals, good_denoise_guides(flags=3))[0] == ERR_ARG
    assert check[1](no_normals, good_denoise_guides(flags=1)) == (0, "")  # demodulation needs no normals


def test_the_checks_under_the_sanitizers(tmp_path):
    """host_guides.cpp's own main() under AddressSanitizer and UBSan: its cases get the answers above, and the program ends without a report"""
    stdout = NL.run_sanitized(tmp_path, "host_guides", "HOST_GUIDES_MAIN")
    got = {l.split()[0]: (int(l.split()[1]), l) for l in stdout.splitlines()}
    want = {"good": None, "all-samples": None, "no-samples": "samples", "samples-past-spp": "samples", "samples-wrap": "samples", "on-device": "on_device",
            "reserved": "reserved", "null-film": "film", "d-good": None, "d-flags": "flags", "d-plane-without-normals": "normals_offset",
            "d-demodulate-without-normals": None, "d-xstride": "xstride", "d-floor-zero": "albedo_floor", "d-floor-nan": "albedo_floor", "d-floor-unused": None,
            "d-sigma-x": "sigma_x", "d-plane-scale": "plane_scale", "d-plane-unused": None, "d-reserved": "reserved", "d-null-guides": "guides"}
    assert sorted(got) == sorted(want)
    for name, field in want.items():
        rc, line = got[name]
        assert (rc == 0) if field is None else (rc == ERR_ARG and field in line), line


# ---- 3. exact properties of the model ------------------------------------------------------------------------------------------------------
PLANE_SCALE = 0.002


def clean_film(h, w, seed, adaptive=False):
    """a film with normals (all +z) in which every pixel is valid, and offsets (normals, m2, samples)"""
    rng = np.random.default_rng(seed)
    xstride, no, mo, so = dn.layout(4, True, adaptive)
    film = np.zeros((h, w, xstride), F)
    film[..., 0:4] = rng.uniform(0.1, 1.0, (h, w, 4))
    film[..., mo:mo + 3] = rng.uniform(0.0, 0.02, (h, w, 3))
    film[..., no + 2] = 1.0
    if adaptive:
        film[..., so] = rng.integers(2, 17, (h, w))
    return film, (no, mo, so)


def flat_guides(h, w, albedo=1.0, depth=4.0):
    """every camera ray hit the plane z = -depth, seen from the origin down -z"""
    g = np.zeros((h, w, 8), F)
    yy, xx = np.mgrid[0:h, 0:w]
    g[..., 0:3] = albedo
    g[..., 3] = 1.0
    g[..., 4] = (xx - w / 2) * PLANE_SCALE * depth; g[..., 5] = (h / 2 - yy) * PLANE_SCALE * depth; g[..., 6] = -depth
    g[..., 7] = depth
    return g


def run(film, offs, guides=None, flags=0, spp=16, **kw):
    return gd.denoise(film, spp, *offs, guides=guides, flags=flags, plane_scale=PLANE_SCALE, **kw)


@pytest.mark.parametrize("shape", [(1, 1), (9, 11)])
def test_flags_zero_and_no_guides_are_the_unguided_filter(shape):
    film, offs = dn.synthetic_film(*shape, 4, True, True)
    want = dn.denoise(film, 16, *offs)
    assert bits_equal(run(film, offs, gd.synthetic_guides(*shape), 0), want)
    assert bits_equal(run(film, offs, None, 3), want)


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_zero_iterations_is_the_identity(flags):
    film, offs = dn.synthetic_film(9, 11, 4, True, True)
    assert bits_equal(run(film, offs, gd.synthetic_guides(9, 11), flags, iterations=0), film)


def test_white_albedo_without_plane_is_the_unguided_filter():
    """albedo == 1 everywhere (and a floor not above it): D = 1, and dividing and multiplying by 1.0 changes no bit"""
    film, offs = dn.synthetic_film(12, 13, 4, True, True)
    g = gd.synthetic_guides(12, 13)
    g[..., 0:3] = np.where(np.isfinite(g[..., 0:3]), F(1.0), g[..., 0:3])
    finite = np.isfinite(g).all(-1)
    want = dn.denoise(np.where(finite[..., None], film, np.nan), 16, *offs)  # a pixel with a non-finite guide float is invalid there as well
    got = run(film, offs, g, gd.DEMODULATE, albedo_floor=1.0)
    assert bits_equal(got[finite], want[finite]) and bits_equal(got[~finite], film[~finite])
    assert bits_equal(run(film, offs, g, gd.DEMODULATE, albedo_floor=0.01), got)


def test_on_one_plane_the_plane_weight_is_one():
    film, offs = clean_film(10, 12, 21)
    assert bits_equal(run(film, offs, flat_guides(10, 12), gd.PLANE, sigma_x=1.0), dn.denoise(film, 16, *offs))


def test_albedo_times_constant_irradiance_comes_back_exactly():
    """primary = A * E with E constant and m2 = 0: the demodulated film is constant, so the delta form returns it and the albedo comes back.  A and E
    have short mantissas (multiples of 1/16 and of 1/4), so that every product and quotient here is exact in fp32 -- the property is the
    filter's, not the rounding's."""
    rng = np.random.default_rng(22)
    h, w = 11, 13
    film, offs = clean_film(h, w, 22)
    A = (rng.integers(1, 17, (h, w, 3)) / 16.0).astype(F)
    E = np.array([0.75, 1.5, 0.25], F)
    film[..., 0:3] = A * E
    film[..., offs[1]:offs[1] + 3] = 0
    g = flat_guides(h, w); g[..., 0:3] = A
    for flags in (gd.DEMODULATE, gd.DEMODULATE | gd.PLANE):
        assert bits_equal(run(film, offs, g, flags), film)
    # with a variance the film is still returned exactly in "primary" (a constant neighbourhood), and m2 drops
    film[..., offs[1]:offs[1] + 3] = (0.01 * A * A).astype(F)
    out = run(film, offs, g, gd.DEMODULATE)
    assert bits_equal(out[..., 0:3], film[..., 0:3]) and (out[..., offs[1]:offs[1] + 3] < film[..., offs[1]:offs[1] + 3]).all()
    # the unguided filter cannot: it averages across the albedo's edges, or not at all
    assert not bits_equal(dn.denoise(film, 16, *offs)[..., 0:3], film[..., 0:3])


def cross_weights(film, offs, guides, left, iterations=5):
    """-> the largest weight of a tap between the columns `left` and the others, over all pixels, taps and iterations, under PLANE"""
    C, V, N, valid, n = gd.init_state(film, guides, gd.PLANE, 16, *offs, 0.01)
    side = np.zeros(film.shape[:2], bool); side[:, left] = True
    worst, taps = 0.0, 0
    for i in range(iterations):
        weights = []
        C, V = gd.iterate(C, V, N, valid, 1 << i, 4.0, 7, guides, D(F(1.0)) * D(F(PLANE_SCALE)), weights)
        for dy, dx, ok, w in weights:
            inside, other = dn._gather(side, (1 << i) * dx, (1 << i) * dy)
            cross = ok & inside & (other != side)
            taps += int(cross.sum())
            if cross.any():
                worst = max(worst, float(np.abs(w[cross]).max()))
    return worst, taps


def test_parallel_planes_exchange_nothing():
    """Two half-films with the SAME normal whose positions lie on parallel planes half a unit apart (tol is 0.008): the normal weight is 1 across the
    edge, the plane weight exactly 0, in every iteration.  Colour therefore never crosses.  What the two halves still share is the yardstick: the
    3 x 3 of e is taken over every valid neighbour (phx_denoise), and e follows from V, which follows from a half's own weights, hence from its
    colours -- so from the SECOND iteration on a change of one half's colours can move the other half's sig (tests/test_denoise.py says the same of
    orthogonal normals).  The bits of the other half are therefore compared (a) after one iteration on a fully noisy film and (b) after five
    iterations where the changed half has m2 = 0: its V and e are then 0 whatever its colours, and nothing at all can cross."""
    h, w = 10, 16
    film, offs = clean_film(h, w, 23)
    g = flat_guides(h, w)
    g[:, 8:, 6] = -4.5; g[:, 8:, 7] = 4.5
    other = film.copy()
    other[:, 8:, 0:3] = np.random.default_rng(24).uniform(5.0, 9.0, (h, 8, 3))
    for a, b in ((film, other),):
        wa, ta = cross_weights(a, offs, g, slice(0, 8)); wb, tb = cross_weights(b, offs, g, slice(0, 8))
        assert wa == 0.0 and wb == 0.0 and ta > 1000 and tb == ta
    one_a, one_b = run(film, offs, g, gd.PLANE, iterations=1), run(other, offs, g, gd.PLANE, iterations=1)
    assert bits_equal(one_a[:, :8], one_b[:, :8]) and not bits_equal(one_a[:, 8:], one_b[:, 8:])
    assert not bits_equal(one_a[:, :8, 0:3], film[:, :8, 0:3])  # the left half WAS filtered
    assert not bits_equal(dn.denoise(film, 16, *offs, iterations=1)[:, :8], dn.denoise(other, 16, *offs, iterations=1)[:, :8])  # unguided: it crosses
    quiet, quiet_other = film.copy(), other.copy()
    for f in (quiet, quiet_other):
        f[:, 8:, offs[1]:offs[1] + 3] = 0
    five_a, five_b = run(quiet, offs, g, gd.PLANE), run(quiet_other, offs, g, gd.PLANE)
    assert bits_equal(five_a[:, :8], five_b[:, :8])
    assert not bits_equal(five_a[:, :8, 0:3], film[:, :8, 0:3])
    # the same under both flags
    assert bits_equal(run(quiet, offs, g, 3)[:, :8], run(quiet_other, offs, g, 3)[:, :8])


def test_open_pixels_mix_with_open_pixels_only():
    """coverage 0 on the right half: no tap crosses (exactly one of the two is open), and the open half mixes among itself (w_x = 1)"""
    h, w = 10, 16
    film, offs = clean_film(h, w, 25)
    g = flat_guides(h, w)
    g[:, 8:, 3:8] = 0
    assert cross_weights(film, offs, g, slice(0, 8)) [0] == 0.0
    out = run(film, offs, g, gd.PLANE, iterations=1)
    assert not bits_equal(out[:, 8:, 0:3], film[:, 8:, 0:3]) and not bits_equal(out[:, :8, 0:3], film[:, :8, 0:3])


@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("slot", range(8))
@pytest.mark.parametrize("what", [np.nan, np.inf])
def test_a_pixel_with_a_non_finite_guide_float_is_untouched_and_invisible(flags, slot, what):
    film, offs = clean_film(9, 10, 26, adaptive=True)
    g = flat_guides(9, 10, albedo=0.5)
    y, x = 4, 5
    bad = g.copy(); bad[y, x, slot] = what
    ref = film.copy(); ref[y, x, offs[2]] = 0.0  # merely invalid in the film: fewer than 2 samples
    a, b = run(film, offs, bad, flags), run(ref, offs, g, flags)
    assert bits_equal(a[y, x], film[y, x]) and bits_equal(b[y, x], ref[y, x])
    mask = np.ones(film.shape[:2], bool); mask[y, x] = False
    assert bits_equal(a[mask], b[mask])
    assert not bits_equal(a[mask], run(film, offs, g, flags)[mask])  # a VALID pixel there does change its neighbours


def test_guide_sums_follow_the_header():
    """three samples of two pixels by hand: sums in sample order in fp32, position and distance over the hits only"""
    one = np.ones(3, F)
    o = np.zeros((2, 3), F); d = np.array([[0, 0, -1], [0.6, 0, -0.8]], F)
    s = [(np.array([[0.2, 0.4, 0.6], one], F), np.array([True, False]), o, d, np.array([2.0, 3e38], F)),
         (np.array([[0.1, 0.1, 0.1], one], F), np.array([True, False]), o, d, np.array([2.5, 3e38], F)),
         (np.array([one, one], F), np.array([False, False]), o, d, np.array([3e38, 3e38], F))]
    g = gd.guide_sums(s)
    third = F(1.0) / F(3.0)
    a0 = F(F(F(0.2) + F(0.1)) + F(1.0)) * third
    assert g[0, 0] == a0 and g[0, 3] == F(2.0) * third and g[0, 6] == F(F(-2.0) + F(-2.5)) / F(2.0) and g[0, 7] == F(2.25)
    assert bits_equal(g[1], np.array([F(3.0) * third] * 3 + [0, 0, 0, 0, 0], F))


# ---- 4. the payoff on a synthetic textured film ---------------------------------------------------------------------------------------------------
PAYOFF_SEED, PAYOFF_OTHER_SEEDS = 19, (1, 2, 3, 4)


def checker_film(seed, n=64, spp=16, rel=0.5):
    """-> (film with normals and m2, offsets, guides, truth): a 2-pixel checker albedo A of 0.1 / 0.9 under a smooth irradiance ramp E, each pixel the
    sum of spp iid samples y_s = A * E * (1 + rel * z_s) / spp (so a sample's deviation scales with A, its variance with A * A), m2 their centred sum
    of squares"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    A = np.where(((xx // 2) + (yy // 2)) % 2 == 0, 0.1, 0.9)[..., None] * np.ones(3)
    E = (0.5 + 1.5 * (xx + 0.5 * yy) / (1.5 * n))[..., None] * np.array([1.0, 0.8, 0.6])
    truth = A * E
    y = (truth[:, :, None, :] * (1.0 + rel * rng.standard_normal((n, n, spp, 3))) / spp).astype(F)
    xstride, no, mo, so = dn.layout(4, True, False)
    film = np.zeros((n, n, xstride), F)
    f = np.zeros((n, n, 3), F); mean = np.zeros((n, n, 3), D); M2 = np.zeros((n, n, 3), D)
    for k in range(spp):  # the rule of phx_frame.moments_channel
        ys = y[:, :, k, :]
        f = (f + ys).astype(F)
        dlt = ys.astype(D) - mean
        mean = mean + dlt * (D(1.0) / D(k + 1))
        M2 = M2 + dlt * (ys.astype(D) - mean)
    film[..., 0:3] = f; film[..., 3] = 1.0; film[..., no + 2] = 1.0; film[..., mo:mo + 3] = M2.astype(F)
    g = flat_guides(n, n); g[..., 0:3] = A.astype(F)
    return film, (no, mo, so), g, truth


def payoff(seed):
    film, offs, g, truth = checker_film(seed)
    mse = lambda out: float(((out[..., 0:3].astype(D) - truth) ** 2).mean())
    return mse(film), mse(dn.denoise(film, 16, *offs)), mse(run(film, offs, g, gd.DEMODULATE))


def test_demodulation_pays_on_a_textured_film():
    """64 x 64, 16 spp, seed 19: MSE guided < unguided < noisy against A * E (measured: 1.928e-4 < 5.446e-4 < 6.874e-3), and guided / unguided below
    1.5 x the model's own value at this seed, 0.3540 (PAYOFF_RATIO_AT_SEED; DESIGN 19 quotes it): 0.531.  The margin covers seeds 1, 2, 3 and 4
    (0.4303, 0.3940, 0.4354, 0.4191), whose ratios the test prints and holds to the same bound."""
    noisy, unguided, guided = payoff(PAYOFF_SEED)
    ratio = guided / unguided
    print(f"guided payoff, seed {PAYOFF_SEED}: MSE noisy {noisy:.4g}, unguided {unguided:.4g}, guided {guided:.4g}; guided / unguided = {ratio:.4f}")
    assert guided < unguided < noisy
    bound = 1.5 * PAYOFF_RATIO_AT_SEED
    assert bound < 1.0 and ratio < bound
    for seed in PAYOFF_OTHER_SEEDS:
        n2, u2, g2 = payoff(seed)
        print(f"guided payoff, seed {seed}: guided / unguided = {g2 / u2:.4f}")
        assert g2 < u2 < n2 and g2 / u2 < bound


PAYOFF_RATIO_AT_SEED = 0.3540  # measured: see the docstring above
