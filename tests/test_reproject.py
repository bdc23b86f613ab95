"""Reprojection (phx_reproject) without a GPU: the ABI and the header's text, every refusal of the argument check and the camera
derivation (csrc/reproject_check.cpp through tests/native/host_reproject.cpp), the Python layout helper, and the float64 model of the rule
(tests/reproject64.py): the copy under an unchanged camera, the cap, non-finite pixels, the film's edges, points behind a camera, the band a
foreground plane disoccludes, and an independent check of the mapping.  The device is held to the same model bit for bit in
tests/test_gpu_reproject.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import native_lib as NL
import reproject64 as rp
import reproject_cases as RC
from native_lib import ERR_ARG

F, D = np.float32, np.float64
FIELDS = ["width", "height", "xstride_a", "normals_offset_a", "m2_offset_a", "samples_offset_a", "xstride_g", "on_device", "from", "to",
          "sigma_plane", "sigma_dist", "max_history", "reserved"]


# ---- 1. the ABI and the header ------------------------------------------------------------------------------------------------------------
def test_struct_size_and_field_offsets():
    from phosphorus_mk2_amd import abi
    assert C.sizeof(abi.Camera) == 84 and C.sizeof(abi.Reproject) == 224
    assert [f for f, _ in abi.Reproject._fields_] == FIELDS
    assert [getattr(abi.Reproject, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 116, 200, 204, 208, 212]
    assert abi.Reproject.reserved.size == 12
    assert [f for f, _ in abi.ReprojectSummary._fields_] == ["pixels", "reused", "no_geometry", "disoccluded", "samples"]
    assert C.sizeof(abi.ReprojectSummary) == 40
    for name in ("phx_dev_set_camera", "phx_dev_film_reproject", "phx_dev_reproject_times"):
        assert name in abi.EXPORTS


def test_struct_size_is_the_librarys():
    from phosphorus_mk2_amd import abi, xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = xpu.load_library()
    assert lib.phx_abi_sizeof(21) == C.sizeof(abi.Reproject) == 224 and lib.phx_abi_sizeof(22) == C.sizeof(abi.ReprojectSummary) == 40
    assert lib.phx_abi_sizeof(19) == C.sizeof(abi.Display) and lib.phx_abi_sizeof(18) == C.sizeof(abi.Accumulate)  # the earlier indices stay


def test_header_states_the_struct_and_the_rule():
    hdr = NL.header()
    names = re.findall(r"\b(\w+)(?:\[3\])?\s*[,;]", NL.struct_body("phx_reproject"))
    assert names == FIELDS
    assert re.search(r"uint64_t\s+pixels,\s*reused,\s*no_geometry,\s*disoccluded,\s*samples;\s*\} phx_reproject_summary;", hdr)
    assert re.search(r"int\s+phx_dev_set_camera\(phx_device\* dev, const phx_camera\* camera\)", hdr)
    assert re.search(r"int\s+phx_dev_film_reproject\(phx_device\* dev, const phx_reproject\* r, const float\* acc_from, const float\* guides_from, "
                     r"const float\* guides_to,\s+float\* acc_to, phx_reproject_summary\* summary", hdr)
    assert re.search(r"int\s+phx_dev_reproject_times\(const phx_device\* dev, double\* ms", hdr)
    rule = hdr[hdr.index("reprojection (DESIGN 22)"):hdr.index("typedef struct phx_reproject {")]
    flat = NL.flat(rule)
    for phrase in ["A = e k - f h", "det = (a A + b B) + c C", "zoom = 1.12 tan((double)fov 0.5)", "c_j = (D_x I_0j + D_y I_1j) + D_z I_2j",
                   "fx = ((c_x / t) / (ratio zoom) + 0.5) W", "fy = (0.5 - (c_y / t) / zoom) H", "sx = x + (fx_from - fx_to)", "x0 = floor(sx)",
                   "tol = plane_scale_from distance_q", "fabs(r) <= sigma_plane tol", "dd <= lim lim", "u_i = w_i / Wsum",
                   "m_c = sum of (u_i u_i) m2_i,c", "n_out = min(n, (double)max_history)", "m_c = m_c (n / n_out)", "STARTS AT its first term",
                   "ties to the first in tap order", "carried as if it were diffuse", "projected as a pinhole", "understates the variance",
                   "binary64, without contraction"]:
        assert " ".join(phrase.split()) in flat, phrase
    assert "nothing is temporal here" in hdr and "DESIGN 22" in hdr[hdr.index("nothing is temporal here"):][:200]


def test_python_settings_are_the_accumulators_layout():
    from phosphorus_mk2_amd import xpu
    a, b = RC.camera(7, 5), RC.camera(7, 5, origin=(1, 2, 3))
    for pc in (3, 4):
        acc = xpu.accumulator(7, 5, pc, True)
        q = xpu.reproject_settings(acc.shape, (5, 7, 8), (5, 7, 8), a, b, 1.5, 3.0, 40, pc)
        assert (q.xstride_a, (q.normals_offset_a, q.m2_offset_a, q.samples_offset_a)) == RC.layout(pc)
        assert (q.width, q.height, q.xstride_g, q.on_device, q.sigma_plane, q.sigma_dist, q.max_history, list(q.reserved)) == (7, 5, 8, 0, 1.5, 3.0, 40, [0, 0, 0])
        assert list(getattr(q, "from").to_world) == list(a.to_world.ravel()) and list(q.to.to_world[12:15]) == [1, 2, 3]
        assert (q.to.film_width, q.to.film_height, q.to.fov) == (7, 5, F(b.fov))
    with pytest.raises(ValueError, match="normals=True"):
        xpu.reproject_settings(xpu.accumulator(7, 5, 4, False).shape, (5, 7, 8), (5, 7, 8), a, b)
    with pytest.raises(ValueError, match="pixels"):
        xpu.reproject_settings((5, 7, 11), (5, 8, 8), (5, 7, 8), a, b)
    with pytest.raises(ValueError, match="one stride"):
        xpu.reproject_settings((5, 7, 11), (5, 7, 8), (5, 7, 11), a, b)


# ---- 2. the refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from phosphorus_mk2_amd import abi
    lib = NL.load("host_reproject")
    lib.check = NL.checker(lib, "hr_check", [C.POINTER(abi.Reproject)] + [C.c_void_p] * 4)
    lib.hr_camera.argtypes = [C.POINTER(abi.Camera), C.POINTER(C.c_double)]; lib.hr_camera.restype = C.c_int
    lib.hr_sizeof.restype = C.c_uint32; lib.hr_sizeof_summary.restype = C.c_uint32
    assert lib.hr_sizeof() == C.sizeof(abi.Reproject) and lib.hr_sizeof_summary() == C.sizeof(abi.ReprojectSummary)
    return lib


FAR = (0x10000, 1 << 40, 2 << 40, 3 << 40)  # far apart: the largest film is 2^32 pixels of 256 bytes


@pytest.fixture(scope="module")
def check(host):
    return lambda q, ptrs=FAR: host.check(C.byref(q), *ptrs)


def good(cam=None, **kw):
    """cam: dict of (which camera, field) -> value, applied after the struct's own fields"""
    from phosphorus_mk2_amd import xpu
    W, H = kw.get("width", 64), kw.get("height", 48)
    q = xpu.reproject_settings((H, W, 11), (H, W, 8), (H, W, 8), RC.camera(W, H), RC.camera(W, H, origin=(0.25, 0, 0)))
    for k, v in kw.items():
        setattr(q, k, v)
    for (which, field), v in (cam or {}).items():
        c = getattr(q, which)
        if field == "to_world":
            for i, x in v.items():
                c.to_world[i] = x
        else:
            setattr(c, field, v)
    return q


ACCEPTED = [dict(), dict(width=1, height=1), dict(width=65535, height=65535), dict(on_device=1), dict(xstride_g=64), dict(max_history=2), dict(max_history=0xffffffff),
            dict(xstride_a=24), dict(xstride_a=10, normals_offset_a=3, m2_offset_a=6, samples_offset_a=9), dict(xstride_a=12, normals_offset_a=9, m2_offset_a=3, samples_offset_a=6),
            dict(sigma_plane=1e-30, sigma_dist=1e30)]
REFUSED = [("width", dict(width=0)), ("width", dict(width=65537)), ("height", dict(height=0)), ("height", dict(height=65537)),
           ("xstride_a", dict(xstride_a=9)), ("xstride_a", dict(xstride_a=25)),
           ("normals_offset_a", dict(normals_offset_a=0)), ("normals_offset_a", dict(normals_offset_a=2)), ("normals_offset_a", dict(normals_offset_a=5)),
           ("normals_offset_a", dict(normals_offset_a=12)), ("m2_offset_a", dict(m2_offset_a=0)), ("m2_offset_a", dict(m2_offset_a=12)),
           ("m2_offset_a", dict(m2_offset_a=0xfffffffe)), ("samples_offset_a", dict(samples_offset_a=0)), ("samples_offset_a", dict(samples_offset_a=14)),
           ("samples_offset_a", dict(samples_offset_a=8)), ("samples_offset_a", dict(samples_offset_a=5)),
           ("xstride_g", dict(xstride_g=7)), ("xstride_g", dict(xstride_g=65)), ("on_device", dict(on_device=2)),
           ("sigma_plane", dict(sigma_plane=0.0)), ("sigma_plane", dict(sigma_plane=-1.0)), ("sigma_plane", dict(sigma_plane=float("nan"))),
           ("sigma_plane", dict(sigma_plane=float("inf"))), ("sigma_dist", dict(sigma_dist=0.0)), ("sigma_dist", dict(sigma_dist=float("nan"))),
           ("sigma_dist", dict(sigma_dist=float("inf"))), ("max_history", dict(max_history=0)), ("max_history", dict(max_history=1))]
NAN, INF = float("nan"), float("inf")
REFUSED_CAMERAS = [("film_width", 63), ("film_height", 49), ("fov", NAN), ("fov", INF), ("fov", 0.0), ("to_world", {0: 0.0}), ("to_world", {0: NAN}),
                   ("to_world", {5: INF}), ("to_world", {12: NAN}), ("to_world", {14: -INF}), ("to_world", {0: 0.0, 5: 0.0, 10: 0.0}),
                   ("to_world", {4: 1.0, 5: 0.0, 6: 0.0})]


@pytest.mark.parametrize("kw", ACCEPTED, ids=NL.case_ids(ACCEPTED))
def test_check_accepts(check, kw):
    assert check(good(**kw)) == (0, "")


@pytest.mark.parametrize("field,kw", REFUSED, ids=NL.case_ids(kw for _, kw in REFUSED))
def test_check_refuses_and_names_the_field(check, field, kw):
    rc, msg = check(good(**kw))
    assert rc == ERR_ARG and msg == f"reproject: {field} is outside its range (phx_reproject)", (rc, msg)


@pytest.mark.parametrize("which", ["from", "to"])
@pytest.mark.parametrize("field,value", REFUSED_CAMERAS, ids=[f"{f}={v}" for f, v in REFUSED_CAMERAS])
def test_check_refuses_a_camera_and_names_it(check, which, field, value):
    rc, msg = check(good(cam={(which, field): value}))
    assert rc == ERR_ARG and msg == f"reproject: {which} is outside its range (phx_reproject)", (rc, msg)


def test_accepted_camera_extremes(check):
    for cam in ({("from", "to_world"): {0: -1.0}}, {("to", "to_world"): {12: 1e30, 13: -1e30}}, {("to", "fov"): 3.0}, {("from", "aperture_radius"): NAN},
                {("to", "to_world"): {0: 1e-12, 5: 1e-12, 10: 1e-12}}, {("from", "to_world"): {3: NAN, 7: NAN, 11: NAN, 15: NAN}}):
        assert check(good(cam=cam)) == (0, ""), cam  # the lens and the matrix's last column are not read


def test_the_refusals_come_in_the_fields_order(check):
    """every field wrong at once, then mended one by one from the front: the check names the first that is still wrong"""
    q = good(width=0, height=0, xstride_a=9, xstride_g=7, on_device=2, sigma_plane=0.0, sigma_dist=0.0, max_history=0,
             cam={("from", "fov"): NAN, ("to", "fov"): NAN})
    q.reserved[0] = 1
    fixes = [("width", dict(width=64)), ("height", dict(height=48)), ("xstride_a", dict(xstride_a=11)), ("xstride_g", dict(xstride_g=8)),
             ("on_device", dict(on_device=0)), ("from", None), ("to", None), ("sigma_plane", dict(sigma_plane=1.0)), ("sigma_dist", dict(sigma_dist=1.0)),
             ("max_history", dict(max_history=2)), ("reserved", None)]
    for field, fix in fixes:
        assert re.search(rf": {field} is outside", check(q)[1]), (field, check(q))
        if fix is not None:
            for k, v in fix.items():
                setattr(q, k, v)
        elif field == "reserved":
            q.reserved[0] = 0
        else:
            c = getattr(q, field)
            c.fov, c.film_width, c.film_height = 1.1, 64, 48
    assert check(q) == (0, "")


def test_check_refuses_reserved_words_and_bad_films(check):
    for i in range(3):
        q = good()
        q.reserved[i] = 1
        assert "reserved" in check(q)[1]
    q = good()
    for i, name in enumerate(["acc_from", "guides_from", "guides_to", "acc_to"]):
        ptrs = list(FAR)
        ptrs[i] = 0
        rc, msg = check(q, ptrs)
        assert rc == ERR_ARG and re.search(rf"\b{name}\b", msg), msg
    bytes_a, bytes_g, base = 64 * 48 * 11 * 4, 64 * 48 * 8 * 4, 0x1000000
    a, gf, gt = base, base + bytes_a, base + bytes_a + bytes_g
    assert check(q, (a, gf, gt, gt + bytes_g)) == (0, "") and check(q, (a + bytes_a, gf + bytes_a, gt + bytes_a, base)) == (0, "")  # back to back
    assert check(q, (a, gf, gf, gt + bytes_g)) == (0, "") and check(q, (a, a, a, gt + bytes_g)) == (0, "")  # the inputs may share what they like
    for out in (a, a + bytes_a - 4, a - bytes_a + 4, gf, gf + bytes_g - 4, gt - 4, gt + bytes_g - 4):
        rc, msg = check(q, (a, gf, gt, out))
        assert rc == ERR_ARG and "acc_to" in msg, (hex(out), msg)


def test_the_check_under_the_sanitizers(tmp_path):
    """host_reproject.cpp's own main() under AddressSanitizer and UBSan: its cases get the answers above, and the program ends without a report"""
    stdout = NL.run_sanitized(tmp_path, "host_reproject", "HOST_REPROJECT_MAIN")
    got = {l.split()[0]: (int(l.split()[1]), l) for l in stdout.splitlines()}
    want = {"good": None, "same": "acc_to", "overlap-guides-from": "acc_to", "overlap-guides-to": "acc_to", "null-acc-from": "acc_from",
            "null-guides-from": "guides_from", "null-guides-to": "guides_to", "null-acc-to": "acc_to", "width": "width", "height": "height",
            "xstride-a": "xstride_a", "m2-wrap": "m2_offset_a", "no-normals": "normals_offset_a", "no-samples": "samples_offset_a", "xstride-g": "xstride_g",
            "on-device": "on_device", "from-size": "from", "from-singular": "from", "to-origin": "to", "to-fov": "to", "sigma-plane": "sigma_plane",
            "sigma-dist": "sigma_dist", "max-history": "max_history", "reserved": "reserved"}
    assert set(want) | {"camera"} == set(got)
    for name, field in want.items():
        rc, line = got[name]
        assert (rc == 0 and line.split()[2:] == []) if field is None else (rc == ERR_ARG and re.search(rf": {field} is outside", line)), line
    assert got["camera"][0] == 1 and [float(v) for v in got["camera"][1].split()[2:]] == [0.5, 1.12 * math.tan(0.5 * float(F(0.9)))]


# ---- 3. the camera derivation ----------------------------------------------------------------------------------------------------------------
def random_matrices():
    rng = np.random.default_rng(11)
    out = []
    for kind in ("rigid", "scaled", "sheared"):
        for _ in range(40):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            if kind == "scaled":
                q = q * rng.uniform(0.01, 100.0, 3)[:, None]
            if kind == "sheared":
                q = q @ (np.eye(3) + np.triu(rng.normal(size=(3, 3)), 1)) * rng.uniform(0.1, 10.0)
            M = np.eye(4)
            M[:3, :3], M[3, :3] = q, rng.uniform(-100, 100, 3)
            out.append((kind, M.astype(F), F(rng.uniform(0.05, 3.0))))
    return out


def test_the_camera_derivation_is_the_models_bit_for_bit(host):
    from phosphorus_mk2_amd import abi
    for kind, M, fov in random_matrices():
        c = abi.Camera(fov=fov, film_width=37, film_height=29)
        c.to_world[:] = [float(v) for v in M.ravel()]
        out = (C.c_double * 16)()
        assert host.hr_camera(C.byref(c), out) == 1, kind
        k = rp.derive(M, fov, 37, 29)
        want = np.concatenate([k.o, k.inv.ravel(), [k.zoom, k.ratio, k.w, k.h]])
        assert np.array(out[:], D).tobytes() == want.astype(D).tobytes(), kind
        # and it IS the inverse: M3 . I = 1 to within the conditioning of the matrix
        m3 = M[:3, :3].astype(D)
        assert np.abs(m3 @ k.inv - np.eye(3)).max() < 1e-9 * np.linalg.cond(m3), kind


def test_singular_and_non_finite_matrices_are_refused_by_check_and_model(host):
    from phosphorus_mk2_amd import abi
    eye = np.eye(4, dtype=F)
    cases = []
    for i in range(3):
        m = eye.copy(); m[i, :3] = 0; cases.append(m)           # a zero row
        m = eye.copy(); m[:3, i] = 0; cases.append(m)           # a zero column
    m = eye.copy(); m[:3, :3] = [[1, 2, 3], [2, 4, 6], [0, 1, 5]]; cases.append(m)    # rank 2, in small integers: every product is exact
    m = eye.copy(); m[:3, :3] = [[1, 2, 3], [4, 5, 6], [5, 7, 9]]; cases.append(m)    # row 3 = row 1 + row 2
    for v in (np.nan, np.inf):
        for i in (0, 6, 13):
            m = eye.copy(); m.ravel()[i] = v; cases.append(m)
    for m in cases:
        c = abi.Camera(fov=1.0, film_width=8, film_height=8)
        c.to_world[:] = [float(v) for v in m.ravel()]
        assert host.hr_camera(C.byref(c), (C.c_double * 16)()) == 0 and rp.derive(m, 1.0, 8, 8) is None, m
    for fov in (np.nan, np.inf, 0.0):
        c = abi.Camera(fov=fov, film_width=8, film_height=8)
        c.to_world[:] = [float(v) for v in eye.ravel()]
        assert host.hr_camera(C.byref(c), (C.c_double * 16)()) == 0 and rp.derive(eye, fov, 8, 8) is None, fov


# ---- 4. properties of the model ------------------------------------------------------------------------------------------------------------------
W, H = 23, 17
OFFS = RC.layout(4)[1]
NO, MO, SO = OFFS
OURS = [0, 1, 2, MO, MO + 1, MO + 2, SO]


def model_camera(cam):
    return rp.derive(cam.to_world, cam.fov, cam.width, cam.height)


def run(acc, gf, gt, a, b, **kw):
    return rp.reproject(acc, gf, gt, model_camera(a), model_camera(b), OFFS, **kw)


def test_an_unchanged_camera_copies_every_valid_pixel_bit_for_bit():
    """whatever the guides' positions: on the pixel centres, off them by a constant, off them by a random offset per pixel; and under a rotated,
    translated, scaled camera as under the identity"""
    rng = np.random.default_rng(1)
    for cam in (RC.camera(W, H), RC.camera(W, H, origin=(3.5, 0.25, -1.0), m3=RC.rot_y(0.3) @ RC.rot_x(-0.2) * 1.7)):
        for ox, oy in ((0.0, 0.0), (0.31, -0.44), (rng.uniform(-0.5, 0.5, (H, W)), rng.uniform(-0.5, 0.5, (H, W)))):
            world = [(tuple(np.array(p) @ (cam.to_world[:3, :3].astype(D) / np.linalg.norm(cam.to_world[0, :3])) + cam.to_world[3, :3]),
                      tuple(np.array(n) @ (cam.to_world[:3, :3].astype(D) / np.linalg.norm(cam.to_world[0, :3]))), -1e30, 1e30) for p, n, _, _ in RC.WORLD]
            g, normals = RC.trace(world, cam, ox, oy)
            assert 0.2 < g[..., 3].mean() <= 1.0
            acc = RC.accumulator(normals)
            gs = RC.spoil_guides(g)
            out, s = run(acc, gs, gs, cam, cam, max_history=32)
            tap = rp.valid_pixels(acc, OFFS) & np.isfinite(gs).all(-1) & (gs[..., 3] > 0)
            assert rp.same(out[tap], acc[tap]) and not out[~tap].any()
            assert s == {"pixels": W * H, "reused": int(tap.sum()), "no_geometry": int((~(gs[..., 3] > 0)).sum()),
                         "disoccluded": int(((gs[..., 3] > 0) & ~tap).sum()), "samples": int(acc[..., SO][tap].astype(D).sum())}
            assert 0 < s["disoccluded"] and 0 < s["reused"] < W * H


def test_the_cap_and_the_scaling_of_m2_that_goes_with_it():
    cam = RC.camera(W, H)
    g, normals = RC.trace(RC.WORLD, cam)
    acc = RC.accumulator(normals, specials=False)
    full, _ = run(acc, g, g, cam, cam, max_history=32)
    out, s = run(acc, g, g, cam, cam, max_history=8)
    hit = g[..., 3] > 0
    n = acc[..., SO].astype(D)
    assert set(np.unique(n)) == {4, 8, 16, 32} and rp.same(full[hit], acc[hit])
    under = hit & (n <= 8)
    assert rp.same(out[under], acc[under])                                   # the cap does not bite: the copy
    over = hit & (n > 8)
    assert (out[..., SO][over] == 8).all() and s["samples"] == int(np.minimum(n, 8)[hit].sum())
    want = (acc[..., MO:MO + 3].astype(D) * (n / 8.0)[..., None]).astype(F)    # n / n_out is 2 or 4: exact
    assert rp.same(out[..., MO:MO + 3][over], want[over]) and rp.same(out[..., 0:3][over], acc[..., 0:3][over]) and rp.same(out[..., NO:NO + 3][over], acc[..., NO:NO + 3][over])
    # "no more confidence than max_history samples of the same spread": the per-sample spread m2 * n is what it was
    assert np.array_equal(out[..., MO:MO + 3][over].astype(D) * 8.0, acc[..., MO:MO + 3][over].astype(D) * n[over][:, None])


def test_an_invalid_or_non_finite_tap_poisons_no_other_pixel():
    """half a pixel of sideways motion: every output pixel mixes two taps.  One spoiled pixel of the old film, by each way of being no tap, changes only
    the outputs that would have read it, those stay finite, and they equal the mix of the taps that are left"""
    a, b = RC.camera(W, H), RC.camera(W, H, origin=(0.3, 0.0, 0.0))
    wall = [((0.0, 0.0, -10.0), (0.0, 0.0, 1.0), -1e30, 1e30)]
    (gf, normals), (gt, _) = RC.trace(wall, a), RC.trace(wall, b)
    acc = RC.accumulator(normals, specials=False)
    clean, s0 = run(acc, gf, gt, a, b)
    assert np.isfinite(clean).all() and s0["reused"] == W * H
    y, x = H // 2, W // 2
    for what, (film, ch, v) in {"nan colour": ("acc", 0, np.nan), "inf m2": ("acc", MO + 1, np.inf), "negative m2": ("acc", MO, -1.0), "n = 1": ("acc", SO, 1.0),
                                "nan n": ("acc", SO, np.nan), "nan normal": ("acc", NO + 2, np.nan), "nan albedo": ("guides", 1, np.nan),
                                "inf position": ("guides", 4, np.inf), "coverage 0": ("guides", 3, 0.0), "nan distance": ("guides", 7, np.nan)}.items():
        acc2, gf2 = acc.copy(), gf.copy()
        (acc2 if film == "acc" else gf2)[y, x, ch] = v
        out, s = run(acc2, gf2, gt, a, b)
        changed = ~(out.view(np.uint32) == clean.view(np.uint32)).all(-1)
        assert np.isfinite(out).all(), what
        ys, xs = np.nonzero(changed)
        assert 1 <= len(ys) <= 2 and (ys == y).all() and (np.abs(xs - x) <= 1).all(), (what, ys, xs)
        assert s["reused"] == s0["reused"] and s["pixels"] == s0["pixels"], what  # each still has its other tap
        for yy, xx in zip(ys, xs):
            others = [q for q in (xx - 1, xx, xx + 1) if q != x and rp.same(out[yy, xx, NO:NO + 3], acc[yy, q, NO:NO + 3]) and rp.same(out[yy, xx, OURS], acc[yy, q, OURS])]
            assert len(others) >= 1, what  # one tap left: its copy (weight w / w = 1)


def test_taps_off_each_of_the_four_film_edges():
    wall = [((0.0, 0.0, -10.0), (0.0, 0.0, 1.0), -1e30, 1e30)]
    a = RC.camera(W, H)
    pix = 10.0 * 1.12 * math.tan(0.55) / H  # world size of a pixel on the wall
    for name, move, lost in (("left", (-2.5 * pix, 0, 0), np.s_[:, :2]), ("right", (2.5 * pix, 0, 0), np.s_[:, -2:]),
                             ("top", (0, 2.5 * pix, 0), np.s_[:2, :]), ("bottom", (0, -2.5 * pix, 0), np.s_[-2:, :])):
        b = RC.camera(W, H, origin=move)
        (gf, normals), (gt, _) = RC.trace(wall, a), RC.trace(wall, b)
        acc = RC.accumulator(normals, specials=False)
        out, s = run(acc, gf, gt, a, b)
        gone = np.zeros((H, W), bool)
        gone[lost] = True                                  # 2.5 pixels of motion: two rows or columns sample wholly outside the film
        assert not out[gone].any() and s["disoccluded"] == int(gone.sum()) and s["reused"] == W * H - int(gone.sum()), name
        edge = np.zeros((H, W), bool)                      # the next one has one tap inside: weight w / w = 1, the copy of the film's edge pixel
        src = {"left": (np.s_[:, 2], np.s_[:, 0]), "right": (np.s_[:, -3], np.s_[:, -1]), "top": (np.s_[2, :], np.s_[0, :]), "bottom": (np.s_[-3, :], np.s_[-1, :])}[name]
        assert rp.same(out[src[0]], acc[src[1]]), name
        assert np.isfinite(out).all()


def test_a_point_behind_either_camera_gets_no_history():
    a, b = RC.pairs(W, H)["behind"]
    (gf, normals), (gt, _) = RC.trace(RC.WORLD, a), RC.trace(RC.WORLD, b)
    acc = RC.accumulator(normals, specials=False)
    out, s = run(acc, gf, gt, a, b, sigma_dist=1e6, sigma_plane=1e6)
    behind_old = (gt[..., 3] > 0) & (gt[..., 6] >= 0)            # the old camera sits at the origin and looks down -z
    assert behind_old.sum() > W and not out[behind_old].any()
    assert s["disoccluded"] >= int(behind_old.sum()) and s["reused"] > 0
    # and the other way round: what the new camera has behind it (its guides cannot show such a point; a guide film that claims one gets nothing)
    out2, s2 = run(acc, gf, gf, a, RC.camera(W, H, origin=(0.0, 0.0, -30.0)), sigma_dist=1e6, sigma_plane=1e6)
    assert not out2.any() and s2["reused"] == 0 and s2["disoccluded"] == int((gf[..., 3] > 0).sum())


def test_a_foreground_plane_disoccludes_exactly_the_band_the_geometry_says():
    """a strip |x| <= 1 at z = -5 before a wall at z = -10, the camera moves sideways by t: a wall pixel of the new view is disoccluded when every
    old pixel its sampling point touches showed the strip or lies off the film.  The test derives the old view's strip columns, the new
    view's, and the wall's motion in film columns from the geometry alone."""
    Wd, Hd, t = 64, 9, 3.0
    a, b = RC.camera(Wd, Hd), RC.camera(Wd, Hd, origin=(t, 0.0, 0.0))
    world = [((0.0, 0.0, -5.0), (0.0, 0.0, 1.0), -1.0, 1.0), ((0.0, 0.0, -10.0), (0.0, 0.0, 1.0), -1e30, 1e30)]
    (gf, normals), (gt, _) = RC.trace(world, a), RC.trace(world, b)
    out, s = run(RC.accumulator(normals, specials=False), gf, gt, a, b)
    k = Wd / ((Wd / Hd) * 1.12 * math.tan(0.55))                # film columns per unit of x / depth
    col = lambda x, depth, cam_x: (x - cam_x) / depth * k + Wd / 2    # the film column of world x at that depth
    cols = np.arange(Wd)
    strip_old = (cols >= col(-1, 5, 0)) & (cols <= col(1, 5, 0))
    strip_new = (cols >= col(-1, 5, t)) & (cols <= col(1, 5, t))
    shift = t / 10 * k                                          # a wall point's column in the old view = its new column + shift
    sx = cols + shift
    x0, frac = np.floor(sx).astype(int), sx - np.floor(sx)
    assert 0.05 < frac[0] < 0.95 and all(abs(v - round(v)) > 0.05 for v in (col(-1, 5, 0), col(1, 5, 0), col(-1, 5, t), col(1, 5, t)))  # no column on a boundary
    blocked = lambda q: (q < 0) | (q >= Wd) | strip_old[np.clip(q, 0, Wd - 1)]
    band = ~strip_new & blocked(x0) & blocked(x0 + 1)
    off_film = x0 + 1 >= Wd
    assert band.sum() - off_film.sum() >= 3 and (band & ~off_film).any()    # a band of several columns beside the strip, besides the film's edge
    got = ~out.any(-1)
    assert (got == band[None, :]).all(), (np.nonzero(got[0])[0], np.nonzero(band)[0])
    assert s == {"pixels": Wd * Hd, "reused": Wd * Hd - Hd * int(band.sum()), "no_geometry": 0, "disoccluded": Hd * int(band.sum()),
                 "samples": int(np.trunc(out[..., SO].astype(D)).sum())}


def test_the_mapping_against_a_projection_of_the_tests_own():
    """The old film is V(q) = a qx + b qy + c on ONE tilted plane, which bilinear interpolation reproduces; the test projects the new view's points
    through both cameras itself (numpy's inverse, the forward ray formula) and demands out(p) = a sx + b sy + c.
    The bound: V(q) is exact in fp32 (multiples of 1/16 below 2^8), so the model's binary64 mix differs from a sx + b sy + c by rounding of
    some twenty binary64 operations on values below 2^8 (< 1e-12) and by (|a| + |b|) times the two projections' disagreement, each some thirty
    operations on coordinates below 2^7 before a division by a depth above 1 and a scale by W <= 2^5: below 1e-10 pixels.  The result is then
    rounded to fp32 once: half an ulp, 2^-24 |v|."""
    Wm, Hm = 31, 19
    ca, cb, cc = 0.5, -0.25, 3.0
    plane = [((0.0, 0.0, -8.0), tuple(np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])), -1e30, 1e30)]
    cam_a = RC.camera(Wm, Hm, origin=(0.2, -0.1, 0.3), m3=RC.rot_y(0.05))
    cam_b = RC.camera(Wm, Hm, origin=(-0.3, 0.2, 0.1), m3=RC.rot_y(-0.08) @ RC.rot_x(0.04) * 1.25)
    (gf, normals), (gt, _) = RC.trace(plane, cam_a, 0.2, -0.3), RC.trace(plane, cam_b, -0.1, 0.4)
    acc = RC.accumulator(normals, specials=False)
    ys, xs = np.mgrid[0:Hm, 0:Wm]
    acc[..., 0] = acc[..., 1] = acc[..., 2] = ca * xs + cb * ys + cc
    acc[..., SO] = 8
    out, s = run(acc, gf, gt, cam_a, cam_b, sigma_plane=2.0, sigma_dist=8.0)

    def film_xy(cam, X):
        M = cam.to_world.astype(D)
        c = (X - M[3, :3]) @ np.linalg.inv(M[:3, :3])
        zoom = 1.12 * math.tan(0.5 * float(F(cam.fov)))
        return (c[..., 0] / -c[..., 2] / (Wm / Hm * zoom) + 0.5) * Wm, (0.5 - c[..., 1] / -c[..., 2] / zoom) * Hm
    X = gt[..., 4:7].astype(D)
    (fxa, fya), (fxb, fyb) = film_xy(cam_a, X), film_xy(cam_b, X)
    sx, sy = xs + (fxa - fxb), ys + (fya - fyb)
    whole = (sx >= 0) & (sx <= Wm - 1) & (sy >= 0) & (sy <= Hm - 1)             # all four taps inside the film (every old pixel is valid and on the plane)
    assert whole.sum() > Wm * Hm // 3 and out[whole].any(-1).all()
    want = ca * sx + cb * sy + cc
    bound = 2.0 ** -24 * np.abs(want) + (abs(ca) + abs(cb)) * 1e-10 + 1e-12
    err = np.abs(out[..., 0].astype(D) - want)
    assert (err[whole] <= bound[whole]).all(), float((err - bound)[whole].max())
    assert np.abs(sx - xs)[whole].max() > 1.0 or np.abs(sy - ys)[whole].max() > 1.0  # the film really moved
    assert (out[..., SO][whole] == 8).all() and rp.same(out[..., 1][whole], out[..., 0][whole])
