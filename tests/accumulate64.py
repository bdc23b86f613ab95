"""The rule of film accumulation (phx_accumulate in include/phx_xpu.h) restated in float64 numpy, operation by operation.

What is vectorised is the film: every line below is one IEEE operation applied to all pixels at once, so a pixel sees exactly the sequence of
binary64 operations the header writes down; the cases (a bad count, n_b == 0, n_a == 0, the pooled pixel) are selected afterwards with
np.where, which keeps bits.  A NaN the arithmetic makes has no specified sign or payload (inf - inf is a negative NaN on one machine and a
positive one on another): `same` compares bit for bit except that a NaN equals a NaN.  Nothing here reads the C++ or the kernel."""
import numpy as np

F, D = np.float32, np.float64
TWO53 = 2 ** 53


def layout(primary_components=4, normals=False, samples=True):
    """-> (xstride, normals_offset, m2_offset, samples_offset) of a film with the m2 channel, as Film lays a pixel out (0 = no such channel);
    samples=True is the accumulator (and an adaptive frame film)"""
    m2 = primary_components + (3 if normals else 0)
    return m2 + 3 + (1 if samples else 0), primary_components if normals else 0, m2, m2 + 3 if samples else 0


def same(a, b):
    """bit for bit, except that a NaN matches a NaN"""
    a = np.ascontiguousarray(a, F); b = np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def counts(acc, frame, offs_a, offs_b, spp_b):
    """-> n_a, n_b (...,) f64 and the masks bad, skip, copy, pool of the rule's four cases"""
    n_a = acc[..., offs_a[2]].astype(D)
    n_b = frame[..., offs_b[2]].astype(D) if offs_b[2] else np.full(frame.shape[:-1], D(spp_b))
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(n_a) & np.isfinite(n_b) & (n_a >= 0) & (n_b >= 0))
    skip = ~bad & (n_b == 0)
    copy = ~bad & ~skip & (n_a == 0)
    return n_a, n_b, bad, skip, copy, ~bad & ~skip & ~copy


def accumulate(acc, frame, offs_a, offs_b, spp_b=0):
    """acc (..., xstride_a) f32, frame (..., xstride_b) f32; offs = (normals_offset, m2_offset, samples_offset) of each -> the new acc"""
    acc = np.asarray(acc, F); frame = np.asarray(frame, F)
    (no_a, mo_a, so_a), (no_b, mo_b, so_b) = offs_a, offs_b
    out = acc.copy()
    n_a, n_b, bad, skip, copy, pool = counts(acc, frame, offs_a, offs_b, spp_b)
    V_a, V_b = acc[..., 0:3].astype(D), frame[..., 0:3].astype(D)
    m2_a, m2_b = acc[..., mo_a:mo_a + 3].astype(D), frame[..., mo_b:mo_b + 3].astype(D)
    na, nb = n_a[..., None], n_b[..., None]
    with np.errstate(all="ignore"):
        n = na + nb
        Q_a = (m2_a * na) * na
        Q_b = (m2_b * nb) * nb
        d = V_b - V_a
        V = (V_a + (d * nb) / n).astype(F)
        Q = (Q_a + Q_b) + ((d * d) * (na * nb)) / n
        m2 = ((Q / n) / n).astype(F)
        samples = n[..., 0].astype(F)
        nb32 = n_b.astype(F)
    nan = F(np.nan)
    c3 = lambda m: m[..., None]
    out[..., 0:3] = np.where(c3(bad), nan, np.where(c3(copy), frame[..., 0:3], np.where(c3(pool), V, acc[..., 0:3])))
    out[..., mo_a:mo_a + 3] = np.where(c3(bad), nan, np.where(c3(copy), frame[..., mo_b:mo_b + 3], np.where(c3(pool), m2, acc[..., mo_a:mo_a + 3])))
    out[..., so_a] = np.where(bad, nan, np.where(copy, nb32, np.where(pool, samples, acc[..., so_a])))
    if no_a and no_b:
        N_b = frame[..., no_b:no_b + 3]
        takes = (copy | pool) & (N_b != 0).any(-1)
        out[..., no_a:no_a + 3] = np.where(c3(takes), N_b, acc[..., no_a:no_a + 3])
    return out


def valid_pixels(film, offs):
    """-> (valid (...,) bool, n (...,) f64) of a film with a samples channel, as the summary counts them"""
    _, mo, so = offs
    n = film[..., so].astype(D)
    m2 = film[..., mo:mo + 3]
    with np.errstate(all="ignore"):
        return np.isfinite(film[..., 0:3]).all(-1) & np.isfinite(m2).all(-1) & (m2 >= 0).all(-1) & np.isfinite(n) & (n >= 2), n


def summary(film, offs, tau, floor=0.0):
    """the counters of phx_accumulate_summary of the pooled film `film`"""
    film = np.asarray(film, F)
    _, mo, so = offs
    valid, n = valid_pixels(film, offs)
    tau, floor = D(F(tau)), D(F(floor))
    with np.errstate(all="ignore"):
        q = n / (n - D(1))
        L = film[..., mo:mo + 3].astype(D) * q[..., None]
        b = tau * (np.fabs(film[..., 0:3].astype(D)) + floor)
        ok = (L <= b * b).all(-1)
    total = sum(int(min(v, TWO53)) for v in n[valid].ravel().tolist()) % (1 << 64)
    return {"pixels": int(valid.size), "invalid": int((~valid).sum()), "converged": int((valid & ok).sum()), "samples": total}


SPECIALS = ["n_a == 0", "n_b == 0", "both zero", "count 1", "count 2", "count 2^24 - 1", "NaN count", "negative count", "infinite count", "NaN colour",
            "inf colour", "m2 == 0", "m2 < 0", "d == 0", "zero normal", "half-zero normal"]


def synthetic_films(shape, primary_components=4, normals=False, frame_samples=False, spp_b=8, seed=0):
    """Two films that reach every branch of the rule: colours over ten decades, sample counts of 2 .. 64, and, where the film has 32 pixels
    or more, one pixel for each of SPECIALS (a frame film without "samples" cannot have n_b == 0 or a bad n_b: those pixels then carry the
    case on acc's side where it has one).  shape: (H, W) -> (acc, frame, offs_a, offs_b), offs = (normals, m2, samples offset)."""
    rng = np.random.default_rng([seed, shape[0], shape[1], primary_components, int(normals), int(frame_samples)])
    xa, no_a, mo_a, so_a = layout(primary_components, normals, True)
    xb, no_b, mo_b, so_b = layout(primary_components, normals, frame_samples)
    npix = shape[0] * shape[1]

    def film(xstride, no, mo, so, top):
        f = np.zeros((npix, xstride), F)
        colour = np.abs(rng.uniform(0.1, 2.0, (npix, 3)) * 10.0 ** rng.integers(-5, 6, (npix, 1)))
        f[:, 0:3] = colour
        if primary_components == 4:
            f[:, 3] = rng.random(npix)
        f[:, mo:mo + 3] = (rng.uniform(0.0, 0.5, (npix, 3)) * colour) ** 2
        if normals:
            nrm = rng.standard_normal((npix, 3))
            f[:, no:no + 3] = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
        if so:
            f[:, so] = rng.integers(2, top + 1, npix)
        return f
    acc = film(xa, no_a, mo_a, so_a, 64)
    frame = film(xb, no_b, mo_b, so_b, 16)
    if npix >= 32:
        at = dict(zip(SPECIALS, rng.choice(npix, len(SPECIALS), replace=False)))
        acc[at["n_a == 0"]] = 0
        acc[at["both zero"]] = 0
        for name, v in (("count 1", 1.0), ("count 2", 2.0), ("count 2^24 - 1", 2.0 ** 24 - 1), ("NaN count", np.nan), ("infinite count", np.inf)):
            acc[at[name], so_a] = v
        if so_b:
            frame[at["n_b == 0"], so_b] = 0
            frame[at["both zero"], so_b] = 0
            frame[at["negative count"], so_b] = -3.0
            frame[at["count 1"], so_b] = 1.0
        else:
            acc[at["negative count"], so_a] = -3.0
        frame[at["NaN colour"], 1] = np.nan
        acc[at["inf colour"], 2] = np.inf
        acc[at["m2 == 0"], mo_a:mo_a + 3] = 0; frame[at["m2 == 0"], mo_b:mo_b + 3] = 0
        frame[at["m2 == 0"], 0:3] = acc[at["m2 == 0"], 0:3]  # equal samples throughout: the pooled m2 is 0 too
        frame[at["m2 < 0"], mo_b + 1] = -abs(frame[at["m2 < 0"], mo_b + 1]) - F(1e-3)
        frame[at["d == 0"], 0:3] = acc[at["d == 0"], 0:3]
        if normals:
            frame[at["zero normal"], no_b:no_b + 3] = 0
            frame[at["half-zero normal"], no_b:no_b + 3] = (0.0, 1.0, 0.0)
    return acc.reshape(shape + (xa,)), frame.reshape(shape + (xb,)), (no_a, mo_a, so_a), (no_b, mo_b, so_b)
