"""The first-hit guide film's sums (phx_guides in include/phx_xpu.h) in numpy fp32 and the guided denoiser's rule (phx_denoise_guides) in float64
numpy, operation by operation.  It extends tests/denoise64.py by import: init_state, the kernels and the gathers are that file's, and with
flags == 0 the call IS denoise64.denoise.  As there, the taps are an explicit loop in the rule's order, every line is one IEEE operation applied to
all pixels at once, and a skipped tap leaves the accumulators as they are.  Nothing here reads the C++ or the kernels."""
import numpy as np

import denoise64 as dn

F, D = np.float32, np.float64
DEMODULATE, PLANE = 1, 2
GUIDE_FLOATS = 8


# ---- the guide film ---------------------------------------------------------------------------------------------------------------------------
def guide_sums(samples):
    """samples: per camera sample, in sample order, a tuple (albedo (..., 3) f32, hit (...) bool, o (..., 3) f32, d (..., 3) f32, t (...) f32); the
    albedo of a sample is read as given (the caller has put (1, 1, 1) where the rule says so), position and distance count where hit.
    -> the guide film (..., 8) f32 by the header's expressions: fp32 sums in sample order from 0, X_c = o_c + t * d_c."""
    G = len(samples)
    shape = np.asarray(samples[0][1]).shape
    a_sum = np.zeros(shape + (3,), F); x_sum = np.zeros(shape + (3,), F); t_sum = np.zeros(shape, F); hits = np.zeros(shape, np.uint32)
    for albedo, hit, o, d, t in samples:
        albedo, o, d, t = (np.asarray(v, F) for v in (albedo, o, d, t))
        hit = np.asarray(hit, bool)
        a_sum = (a_sum + albedo).astype(F)
        with np.errstate(all="ignore"):
            X = (o + (d * t[..., None]).astype(F)).astype(F)
            x_sum = np.where(hit[..., None], (x_sum + X).astype(F), x_sum)
            t_sum = np.where(hit, (t_sum + t).astype(F), t_sum)
        hits = hits + hit.astype(np.uint32)
    inv_g = F(1.0) / F(G)
    fh = hits.astype(F)
    out = np.zeros(shape + (GUIDE_FLOATS,), F)
    out[..., 0:3] = a_sum * inv_g
    out[..., 3] = fh * inv_g
    with np.errstate(all="ignore"):
        out[..., 4:7] = np.where((hits > 0)[..., None], x_sum / fh[..., None], F(0))
        out[..., 7] = np.where(hits > 0, t_sum / fh, F(0))
    return out


# ---- the guided filter ------------------------------------------------------------------------------------------------------------------------
def albedo_divisor(guides, albedo_floor):
    """D_c = max((double)albedo_c, (double)albedo_floor)"""
    return np.maximum(np.asarray(guides, F)[..., 0:3].astype(D), D(F(albedo_floor)))


def init_state(film, guides, flags, spp, normals_offset, m2_offset, samples_offset, albedo_floor):
    """denoise64.init_state with the guides: valid also needs the 8 guide floats finite; under DEMODULATE C and V are the demodulated ones"""
    film = np.asarray(film, F); guides = np.asarray(guides, F)
    C, V, N, valid, n = dn.init_state(film, spp, normals_offset, m2_offset, samples_offset)
    valid = valid & np.isfinite(guides[..., 0:GUIDE_FLOATS]).all(-1)
    if flags & DEMODULATE:
        Dv = albedo_divisor(guides, albedo_floor)
        m2 = film[..., m2_offset:m2_offset + 3]
        with np.errstate(all="ignore"):
            q = n / (n - D(1))
            C = (film[..., 0:3].astype(D) / Dv).astype(F)
            V = ((m2.astype(D) * q[..., None]) / (Dv * Dv)).astype(F)
        C = np.where(valid[..., None], C, film[..., 0:3])
    V = np.where(valid[..., None], V, F(0))
    return C, V, N, valid, n


def plane_weight(N, guides, step, dx, dy, tol_scale):
    """w_x of the tap (dx, dy) at step `step` for every pixel p: (H, W) f64"""
    Nd = N.astype(D)
    X = guides[..., 4:7].astype(D); cov = guides[..., 3]; dist = guides[..., 7].astype(D)
    Xq = dn._gather(X, step * dx, step * dy)[1]
    covq = dn._gather(cov, step * dx, step * dy)[1]
    with np.errstate(all="ignore"):
        r = (Nd[..., 0] * (Xq[..., 0] - X[..., 0]) + Nd[..., 1] * (Xq[..., 1] - X[..., 1])) + Nd[..., 2] * (Xq[..., 2] - X[..., 2])
        tol = tol_scale * dist
        u = np.fabs(r) / tol
        t = D(1) - u * u
        w = np.where(tol == 0, np.where(r == 0, D(1), D(0)), np.where(u < 1, t * t, D(0)))
    p_open, q_open = cov == 0, covq == 0
    return np.where(p_open | q_open, np.where(p_open & q_open, D(1), D(0)), w)


def iterate(C, V, N, valid, step, sigma_l, normal_power_log2, guides=None, tol_scale=None, weights=None):
    """denoise64.iterate with w = ((h * w_n) * w_l) * w_x on the non-centre taps (guides and tol_scale given: PLANE); without them it is that function"""
    if guides is None:
        return dn.iterate(C, V, N, valid, step, sigma_l, normal_power_log2, weights)
    Cd, Vd, Nd = C.astype(D), V.astype(D), N.astype(D)
    sigma = D(F(sigma_l))
    K3, K5, _gather = dn.K3, dn.K5, dn._gather
    with np.errstate(all="ignore"):
        l = dn.luminance(Cd)
        e = dn.deviation(V)
        sum_g = np.zeros(l.shape, D); sum_gee = np.zeros(l.shape, D)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inside, eq = _gather(e, dx, dy)
                ok = inside & _gather(valid, dx, dy)[1]
                g = K3[dy + 1] * K3[dx + 1]
                sum_gee = np.where(ok, sum_gee + (g * eq) * eq, sum_gee)
                sum_g = np.where(ok, sum_g + g, sum_g)
        sig = sigma * np.sqrt(sum_gee / sum_g)
        p_missed = (N == 0).all(-1)
        W = np.zeros(l.shape, D); A = np.zeros(Cd.shape, D); B = np.zeros(Cd.shape, D)
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                inside, Cq = _gather(Cd, step * dx, step * dy)
                ok = inside & _gather(valid, step * dx, step * dy)[1]
                Vq = _gather(Vd, step * dx, step * dy)[1]
                h = K5[dy + 2] * K5[dx + 2]
                if dx == 0 and dy == 0:
                    w = np.full(l.shape, h)
                else:
                    Nq = _gather(Nd, step * dx, step * dy)[1]
                    d = (Nd[..., 0] * Nq[..., 0] + Nd[..., 1] * Nq[..., 1]) + Nd[..., 2] * Nq[..., 2]
                    d = np.where(d > 0, d, D(0))
                    for _ in range(normal_power_log2):
                        d = d * d
                    w_n = np.where(p_missed & (Nq == 0).all(-1), D(1), d)
                    lq = dn.luminance(Cq)
                    u = np.fabs(lq - l) / sig
                    t = D(1) - u * u
                    w_l = np.where(sig == 0, np.where(lq == l, D(1), D(0)), np.where(u < 1, t * t, D(0)))
                    w = ((h * w_n) * w_l) * plane_weight(N, guides, step, dx, dy, tol_scale)
                if weights is not None:
                    weights.append((dy, dx, ok, w))
                W = np.where(ok, W + w, W)
                A = np.where(ok[..., None], A + w[..., None] * (Cq - Cd), A)
                B = np.where(ok[..., None], B + (w * w)[..., None] * Vq, B)
        Cn = (Cd + A / W[..., None]).astype(F)
        Vn = (B / (W * W)[..., None]).astype(F)
    return np.where(valid[..., None], Cn, C), np.where(valid[..., None], Vn, V)


def denoise(film, spp, normals_offset, m2_offset, samples_offset=0, iterations=5, sigma_l=4.0, normal_power_log2=7,
            guides=None, flags=0, albedo_floor=0.01, sigma_x=1.0, plane_scale=1.0):
    """film (H, W, xstride) f32, guides (H, W, >= 8) f32 -> the denoised film, a new array.  flags == 0 (or no guides): denoise64.denoise."""
    if guides is None or not flags:
        return dn.denoise(film, spp, normals_offset, m2_offset, samples_offset, iterations, sigma_l, normal_power_log2)
    if flags & PLANE and not normals_offset:
        raise ValueError("PLANE needs the film's normals")
    film = np.asarray(film, F); guides = np.asarray(guides, F)
    out = film.copy()
    if iterations == 0:
        return out
    C, V, N, valid, n = init_state(film, guides, flags, spp, normals_offset, m2_offset, samples_offset, albedo_floor)
    tol_scale = D(F(sigma_x)) * D(F(plane_scale))
    for i in range(iterations):
        if flags & PLANE:
            C, V = iterate(C, V, N, valid, 1 << i, sigma_l, normal_power_log2, guides, tol_scale)
        else:
            C, V = dn.iterate(C, V, N, valid, 1 << i, sigma_l, normal_power_log2)
    with np.errstate(all="ignore"):
        r = ((n - D(1)) / n)[..., None]
        if flags & DEMODULATE:
            Dv = albedo_divisor(guides, albedo_floor)
            primary = (C.astype(D) * Dv).astype(F)
            m2 = (((V.astype(D) * Dv) * Dv) * r).astype(F)
        else:
            primary = C
            m2 = (V.astype(D) * r).astype(F)
    out[..., 0:3] = np.where(valid[..., None], primary, film[..., 0:3])
    out[..., m2_offset:m2_offset + 3] = np.where(valid[..., None], m2, film[..., m2_offset:m2_offset + 3])
    return out


def synthetic_guides(height, width, seed=0, xstride=GUIDE_FLOATS):
    """A guide film that reaches every branch: albedo over three decades with values below any sensible floor, pixels of coverage 0 (position and
    distance 0) and of partial coverage, positions on two planes and scattered off them, a zero distance on a covered pixel, and (where the film is
    large enough) one NaN and one Inf.  -> (H, W, xstride) f32"""
    rng = np.random.default_rng([seed, height, width, 19])
    g = np.zeros((height, width, xstride), F)
    yy, xx = np.mgrid[0:height, 0:width]
    g[..., 0:3] = 10.0 ** rng.uniform(-3, 0, (height, width, 3))
    g[..., 0:3][rng.random((height, width)) < 0.1] = 1.0
    cov = rng.choice([0.0, 0.25, 1.0], (height, width), p=[0.15, 0.15, 0.7])
    g[..., 3] = cov
    depth = np.where((xx * 2) // max(width, 1) == 0, 4.0, 4.5) + 0.002 * rng.standard_normal((height, width)) * (rng.random((height, width)) < 0.5)
    g[..., 4] = (xx - width / 2) * 0.01 * depth; g[..., 5] = (yy - height / 2) * 0.01 * depth; g[..., 6] = -depth
    g[..., 7] = depth
    g[..., 4:8][cov == 0] = 0.0
    if xstride > GUIDE_FLOATS:
        g[..., GUIDE_FLOATS:] = rng.random((height, width, xstride - GUIDE_FLOATS))
    flat = g.reshape(-1, xstride)
    npix = height * width
    if npix >= 16:
        spots = rng.choice(npix, 3, replace=False)
        flat[spots[0], 1] = np.nan
        flat[spots[1], 6] = np.inf
        flat[spots[2], 3] = 1.0; flat[spots[2], 7] = 0.0  # covered, at distance 0: tol == 0
    return g
