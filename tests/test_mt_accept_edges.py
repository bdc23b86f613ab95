"""mt_intersect (csrc/bvh8.h) — the triangle test the host walk and every trace kernel share — against a float32 statement of the reference's
predicate (src/accel/triangle.hpp:149-164 plus the lowest-primitive tie rule), on rays built to land ON the predicate's edges:

    accept  <=>  (det > 1e-8 or det < -1e-8) and us >= 0 and vs >= 0 and us + vs <= 1 and ds >= 0 and (ds < tmax or (ds == tmax and prim < best_prim))

The accept test of mt_intersect is written with fewer instructions than that sentence (one compare of min(vs, ds), no short-circuits); this file
pins that it is the same predicate where the two could differ: -0 in us, vs or ds (-0 >= 0 holds), us + vs at 1 and its neighbours, ds == tmax
with the primitive below / at / above the best one, det at +-1e-8 and the floats next to it, NaN (of either sign) and infinite ray components.
Every case states what the REFERENCE arithmetic yields for it (the -0, the tie, the NaN) and the test asserts that first: a case that does not sit
on its edge fails as such.  The reference arithmetic is restated here in float32 with a correctly rounded fma; mt_intersect runs through
tests/native/host_mt_accept.cpp, compiled on first use."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import native_lib as NL

F = np.float32
EPS = F(0.00000001)
FLT_MAX = np.finfo(np.float32).max
PNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
NNAN = np.array([0xffc00000], np.uint32).view(np.float32)[0]
up = lambda x: np.nextafter(F(x), F(np.inf))
down = lambda x: np.nextafter(F(x), F(-np.inf))


@pytest.fixture(scope="module")
def shim():
    lib = NL.load("host_mt_accept")
    f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    lib.hmt_accept.argtypes = [C.c_uint32, f32p, u32p, f32p, f32p, f32p, u32p, u8p, f32p, f32p, f32p]
    lib.hmt_accept.restype = None
    return lib


# ---- the reference in float32 --------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32 fma with ONE rounding: the exact a * b + c (a rational) rounded to nearest-even; non-finite operands through float64, where the
    product of two float32 is exact and inf / NaN behave as in float32"""
    a, b, c = F(a), F(b), F(c)
    with np.errstate(all="ignore"):
        approx = F(np.float64(a) * np.float64(b) + np.float64(c))
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)) or not np.isfinite(approx):
        return approx  # (a finite a * b + c beyond FLT_MAX is +-inf either way: the cases stay far from that edge)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        return approx  # the sign of an exact zero: float64 gives float32's (-0 only when both addends are -0)
    best = None
    for cand in (down(approx), approx, up(approx)):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - exact)
        even = (int(np.array([cand], np.float32).view(np.uint32)[0]) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, cand, even)
    return best[1]


def sdot(a, b):
    with np.errstate(all="ignore"):
        return fma32(a[0], b[0], fma32(a[1], b[1], F(a[2]) * F(b[2])))


def scross(a, b):
    with np.errstate(all="ignore"):
        return (fma32(a[1], b[2], -(F(a[2]) * F(b[1]))), fma32(a[2], b[0], -(F(a[0]) * F(b[2]))), fma32(a[0], b[1], -(F(a[1]) * F(b[0]))))


def reference(v0, e0, e1, prim, o, wi, tmax, best_prim):
    """-> (accept, us, vs, ds, det, us + vs) as the reference computes them in float32"""
    with np.errstate(all="ignore"):
        t = tuple(F(o[k]) - F(v0[k]) for k in range(3))
        p = scross(wi, e1)
        det = sdot(e0, p)
        ood = F(1.0) / det
        q = scross(t, e0)
        us, vs, ds = sdot(t, p) * ood, sdot(wi, q) * ood, sdot(e1, q) * ood
        s = us + vs
        xmask = bool(det > EPS) or bool(det < -EPS)
        accept = xmask and bool(us >= 0) and bool(vs >= 0) and bool(s <= F(1)) and bool(ds >= 0) and (bool(ds < tmax) or (bool(ds == tmax) and prim < best_prim))
    return accept, us, vs, ds, det, s


# ---- the cases -----------------------------------------------------------------------------------------------------------------
FRONT = ((0, 0, 0), (1, 0, 0), (0, 1, 0))  # v0, e0, e1: a ray along -z at (x, y, 1) gets det = 1, us = x, vs = y, ds = 1
BACK = ((0, 0, 0), (0, 1, 0), (1, 0, 0))   # the same triangle wound the other way: det = -1, us = y, vs = x, and a zero numerator becomes -0
DOWN = (0, 0, -1)
neg0 = lambda x: x == 0 and np.signbit(x)
pos0 = lambda x: x == 0 and not np.signbit(x)


def case(name, tri, o, wi, expect, tmax=FLT_MAX, prim=5, best_prim=0, accept=None):
    return dict(name=name, tri=tri, o=o, wi=wi, tmax=F(tmax), prim=prim, best_prim=best_prim, expect=expect, accept=accept)


def cases():
    c = []
    # rays through a vertex and along an edge: zeros of either sign in us, vs, ds
    c.append(case("front vertex v0: us = vs = +0", FRONT, (0, 0, 1), DOWN, lambda r: pos0(r[1]) and pos0(r[2]), accept=True))
    c.append(case("back vertex v0: us = vs = -0", BACK, (0, 0, 1), DOWN, lambda r: neg0(r[1]) and neg0(r[2]) and r[4] == -1, accept=True))
    c.append(case("back edge e1 (y = 0): us = -0", BACK, (0.25, 0, 1), DOWN, lambda r: neg0(r[1]) and r[2] == F(0.25), accept=True))
    c.append(case("back edge e0 (x = 0): vs = -0", BACK, (0, 0.25, 1), DOWN, lambda r: neg0(r[2]) and r[1] == F(0.25), accept=True))
    c.append(case("front edge e0 (y = 0): vs = +0", FRONT, (0.25, 0, 1), DOWN, lambda r: pos0(r[2]), accept=True))
    c.append(case("front vertex v0 + e0: us = 1, vs = +0", FRONT, (1, 0, 1), DOWN, lambda r: r[1] == 1 and pos0(r[2]) and r[5] == 1, accept=True))
    c.append(case("back vertex v0 + e0: us = 1, vs = -0", BACK, (0, 1, 1), DOWN, lambda r: r[1] == 1 and neg0(r[2]) and r[5] == 1, accept=True))
    c.append(case("just outside edge e0: vs < 0", FRONT, (0.25, -1e-6, 1), DOWN, lambda r: r[2] < 0, accept=False))
    c.append(case("just outside edge e1: us < 0", FRONT, (-1e-6, 0.25, 1), DOWN, lambda r: r[1] < 0, accept=False))
    c.append(case("origin on the front plane: ds = +0", FRONT, (0.25, 0.25, 0), DOWN, lambda r: pos0(r[3]), accept=True))
    c.append(case("origin on the back plane: ds = -0", BACK, (0.25, 0.25, 0), DOWN, lambda r: neg0(r[3]), accept=True))
    c.append(case("ds = -0 meets tmax = +0, lower primitive: the tie", BACK, (0.25, 0.25, 0), DOWN, lambda r: neg0(r[3]), tmax=0.0, prim=5, best_prim=6, accept=True))
    c.append(case("ds = -0 meets tmax = +0, higher primitive", BACK, (0.25, 0.25, 0), DOWN, lambda r: neg0(r[3]), tmax=0.0, prim=5, best_prim=5, accept=False))
    c.append(case("triangle behind the origin: ds < 0", FRONT, (0.25, 0.25, -1), DOWN, lambda r: r[3] == -1, accept=False))
    # us + vs at 1 and next to it
    c.append(case("us + vs = 1", FRONT, (0.5, 0.5, 1), DOWN, lambda r: r[5] == 1, accept=True))
    c.append(case("us + vs = 1 - 1 ulp", FRONT, (0.5, F(0.5) - F(2.0 ** -24), 1), DOWN, lambda r: r[5] == down(1), accept=True))
    c.append(case("us + vs = 1 + 1 ulp", FRONT, (0.5, F(0.5) + F(2.0 ** -23), 1), DOWN, lambda r: r[5] == up(1), accept=False))
    c.append(case("us + vs rounds to 1 from above (tie to even)", FRONT, (0.5, up(0.5), 1), DOWN, lambda r: r[5] == 1 and r[2] > F(0.5), accept=True))
    c.append(case("back: us + vs = 1 + 1 ulp", BACK, (F(0.5) + F(2.0 ** -23), 0.5, 1), DOWN, lambda r: r[5] == up(1), accept=False))
    # ds == tmax: the tie goes to the lower primitive, and only the tie
    for best, acc in ((4, False), (5, False), (6, True)):
        c.append(case(f"ds = tmax, prim 5 against best_prim {best}", FRONT, (0.25, 0.25, 1), DOWN, lambda r: r[3] == 1, tmax=1.0, prim=5, best_prim=best, accept=acc))
    c.append(case("ds 1 ulp below tmax", FRONT, (0.25, 0.25, 1), DOWN, lambda r: r[3] == 1, tmax=up(1), prim=5, best_prim=0, accept=True))
    c.append(case("ds 1 ulp above tmax, lower primitive", FRONT, (0.25, 0.25, 1), DOWN, lambda r: r[3] == 1, tmax=down(1), prim=5, best_prim=6, accept=False))
    c.append(case("ds = tmax = FLT_MAX stays a miss for primitive 0", FRONT, (0.25, 0.25, FLT_MAX), (0, 0, -1), lambda r: r[3] == FLT_MAX, prim=0, best_prim=0, accept=False))
    # det at +-1e-8 and the floats next to it (e0 = (s, 0, 0) makes det = s exactly; the ray goes through v0, so us = vs = 0 whatever 1 / det)
    for s, acc in ((EPS, False), (up(EPS), True), (down(EPS), False), (-EPS, False), (down(-EPS), True), (up(-EPS), False), (F(0), False)):
        c.append(case(f"det = {float(s)!r}", ((0, 0, 0), (s, 0, 0), (0, 1, 0)), (0, 0, 1), DOWN, (lambda s: lambda r: r[4] == s and r[4].tobytes() == s.tobytes())(F(s)), accept=acc))
    # NaN (of either sign) and infinite ray components: whatever they make of us, vs, ds and det, the ray misses
    has_nan = lambda r: any(np.isnan(x) for x in r[1:5])
    for nan, tag in ((PNAN, "+NaN"), (NNAN, "-NaN")):
        c.append(case(f"origin x = {tag}", FRONT, (nan, 0.25, 1), DOWN, has_nan, accept=False))
        c.append(case(f"origin z = {tag}", FRONT, (0.25, 0.25, nan), DOWN, lambda r: np.isnan(r[3]) and r[4] == 1, accept=False))  # det passes; NaN * 0 makes us, vs and ds NaN
        c.append(case(f"direction z = {tag}", FRONT, (0.25, 0.25, 1), (0, 0, nan), lambda r: np.isnan(r[4]), accept=False))
        c.append(case(f"direction x = {tag}", BACK, (0.25, 0.25, 1), (nan, 0, -1), has_nan, accept=False))
    c.append(case("us alone is NaN (vs = ds = +inf, det = -1.125)", ((0, 0, 0), (2, -1, 0.25), (0.5, 0.25, 0.5)), (np.inf, 0.25, 0), (-1, 0.5, 1),
                  lambda r: np.isnan(r[1]) and r[2] == np.inf and r[3] == np.inf and r[4] == F(-1.125), accept=False))
    for inf in (F(np.inf), F(-np.inf)):
        c.append(case(f"origin x = {float(inf)}", FRONT, (inf, 0.25, 1), DOWN, lambda r: np.isinf(r[1]) or np.isnan(r[1]), accept=False))
        c.append(case(f"origin z = {float(inf)}", FRONT, (0.25, 0.25, inf), DOWN, lambda r: not np.isfinite(r[3]), accept=False))
        c.append(case(f"direction z = {float(inf)}", FRONT, (0.25, 0.25, 1), (0, 0, inf), lambda r: not np.isfinite(r[4]) or has_nan(r), accept=False))
        c.append(case(f"direction x = {float(inf)}", FRONT, (0.25, 0.25, 1), (inf, 0, -1), has_nan, accept=False))
    return c


CASES = cases()


def test_every_case_sits_on_its_edge():
    """the reference arithmetic yields the -0, the sum, the tie, the det or the NaN each case is named after, and the verdict written beside it"""
    for k in CASES:
        r = reference(*k["tri"], k["prim"], k["o"], k["wi"], k["tmax"], k["best_prim"])
        assert k["expect"](r), (k["name"], r)
        assert r[0] == k["accept"], (k["name"], r)
    nan_signs = set()
    for k in CASES:
        r = reference(*k["tri"], k["prim"], k["o"], k["wi"], k["tmax"], k["best_prim"])
        nan_signs |= {bool(np.signbit(x)) for x in r[1:5] if np.isnan(x)}
    assert nan_signs == {False, True}  # NaNs with the sign bit clear AND set reach the predicate


def test_mt_intersect_is_the_reference_predicate_on_its_edges(shim):
    n = len(CASES)
    tri = np.array([np.concatenate([np.asarray(v, np.float32) for v in k["tri"]]) for k in CASES], np.float32)
    o = np.array([k["o"] for k in CASES], np.float32); d = np.array([k["wi"] for k in CASES], np.float32)
    tmax = np.array([k["tmax"] for k in CASES], np.float32)
    prim = np.array([k["prim"] for k in CASES], np.uint32); best = np.array([k["best_prim"] for k in CASES], np.uint32)
    acc = np.zeros(n, np.uint8); us = np.zeros(n, np.float32); vs = np.zeros(n, np.float32); ds = np.zeros(n, np.float32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    shim.hmt_accept(n, p(tri, C.c_float), p(prim, C.c_uint32), p(o, C.c_float), p(d, C.c_float), p(tmax, C.c_float), p(best, C.c_uint32),
                    p(acc, C.c_uint8), p(us, C.c_float), p(vs, C.c_float), p(ds, C.c_float))
    same = lambda a, b: (np.isnan(a) and np.isnan(b)) or F(a).tobytes() == F(b).tobytes()  # bit for bit; a NaN's payload is the hardware's business
    for i, k in enumerate(CASES):
        r = reference(*k["tri"], k["prim"], k["o"], k["wi"], k["tmax"], k["best_prim"])
        assert same(us[i], r[1]) and same(vs[i], r[2]) and same(ds[i], r[3]), (k["name"], us[i], vs[i], ds[i], r)
        assert bool(acc[i]) == r[0], (k["name"], bool(acc[i]), r)
    assert 10 < int(acc.sum()) < n - 10  # both verdicts are well represented
