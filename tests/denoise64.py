"""The film denoiser's rule (phx_denoise in include/phx_xpu.h) restated in float64 numpy, operation by operation.

The taps are an explicit loop in the rule's order (dy outer, dx inner): there is no np.sum over taps, because the order of the additions IS
the rule.  What is vectorised is the film: every line below is one IEEE operation applied to all pixels at once, so a pixel sees exactly the
sequence of binary64 operations the header writes down.  A skipped tap (outside the film, or invalid) leaves the accumulators as they are
(np.where keeps the old value); it does not add a zero.  Nothing here reads the C++ or the kernels."""
import numpy as np

F, D = np.float32, np.float64
K3 = (D(0.25), D(0.5), D(0.25))
K5 = (D(0.0625), D(0.25), D(0.375), D(0.25), D(0.0625))


def layout(primary_components=4, normals=False, adaptive=False):
    """-> (xstride, normals_offset, m2_offset, samples_offset) of a film with the m2 channel, as Film lays a pixel out (0 = no such channel)"""
    m2 = primary_components + (3 if normals else 0)
    return m2 + 3 + (1 if adaptive else 0), primary_components if normals else 0, m2, m2 + 3 if adaptive else 0


def luminance(c):
    return (D(0.2126) * c[..., 0] + D(0.7152) * c[..., 1]) + D(0.0722) * c[..., 2]


def deviation(V):
    """e_x from the fp32 variances V (..., 3)"""
    s = np.sqrt(V.astype(D))
    return (D(0.2126) * s[..., 0] + D(0.7152) * s[..., 1]) + D(0.0722) * s[..., 2]


def init_state(film, spp, normals_offset, m2_offset, samples_offset):
    """-> C (H, W, 3) f32, V (H, W, 3) f32, N (H, W, 3) f32, valid (H, W) bool, n (H, W) f64"""
    film = np.asarray(film, F)
    C = film[..., 0:3].copy()
    m2 = film[..., m2_offset:m2_offset + 3]
    N = film[..., normals_offset:normals_offset + 3].copy() if normals_offset else np.zeros(C.shape, F)
    n = film[..., samples_offset].astype(D) if samples_offset else np.full(C.shape[:2], D(spp))
    with np.errstate(all="ignore"):
        valid = (np.isfinite(C).all(-1) & np.isfinite(m2).all(-1) & np.isfinite(N).all(-1) & (m2 >= 0).all(-1) & np.isfinite(n) & (n >= 2))
        q = n / (n - D(1))
        V = (m2.astype(D) * q[..., None]).astype(F)
    V[~valid] = 0
    return C, V, N, valid, n


def _gather(a, dx, dy):
    """-> (inside (H, W) bool, a at (y + dy, x + dx), clamped where that is outside)"""
    H, W = a.shape[:2]
    yy = np.arange(H)[:, None] + dy
    xx = np.arange(W)[None, :] + dx
    inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    return inside, a[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]


def iterate(C, V, N, valid, step, sigma_l, normal_power_log2, weights=None):
    """One iteration at step `step`: the state (C, V) f32 -> the next (C', V') f32; invalid pixels keep theirs.
    weights: a list that receives (dy, dx, ok, w) per tap, for tests that recompute a result from the weights."""
    Cd, Vd, Nd = C.astype(D), V.astype(D), N.astype(D)
    sigma = D(F(sigma_l))
    with np.errstate(all="ignore"):
        l = luminance(Cd)
        e = deviation(V)
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
                    lq = luminance(Cq)
                    u = np.fabs(lq - l) / sig
                    t = D(1) - u * u
                    w_l = np.where(sig == 0, np.where(lq == l, D(1), D(0)), np.where(u < 1, t * t, D(0)))
                    w = (h * w_n) * w_l
                if weights is not None:
                    weights.append((dy, dx, ok, w))
                W = np.where(ok, W + w, W)
                A = np.where(ok[..., None], A + w[..., None] * (Cq - Cd), A)
                B = np.where(ok[..., None], B + (w * w)[..., None] * Vq, B)
        Cn = (Cd + A / W[..., None]).astype(F)
        Vn = (B / (W * W)[..., None]).astype(F)
    return np.where(valid[..., None], Cn, C), np.where(valid[..., None], Vn, V)


def denoise(film, spp, normals_offset, m2_offset, samples_offset=0, iterations=5, sigma_l=4.0, normal_power_log2=7):
    """film (H, W, xstride) f32 -> the denoised film, a new array"""
    film = np.asarray(film, F)
    out = film.copy()
    if iterations == 0:
        return out
    C, V, N, valid, n = init_state(film, spp, normals_offset, m2_offset, samples_offset)
    for i in range(iterations):
        C, V = iterate(C, V, N, valid, 1 << i, sigma_l, normal_power_log2)
    with np.errstate(all="ignore"):
        m2 = (V.astype(D) * ((n - D(1)) / n)[..., None]).astype(F)
    out[..., 0:3] = np.where(valid[..., None], C, film[..., 0:3])
    out[..., m2_offset:m2_offset + 3] = np.where(valid[..., None], m2, film[..., m2_offset:m2_offset + 3])
    return out


def synthetic_film(height, width, primary_components=4, normals=False, adaptive=False, spp=16, seed=0):
    """A film that reaches every branch of the rule: colours over ten decades with exact zeros, normals in three clusters plus missed pixels,
    m2 with zeros, one NaN, one Inf and one negative m2, "samples" between 2 and spp and one pixel with 1 (where the film is large enough to
    hold them apart; a 1 x 1 film is one ordinary pixel).  -> (film (H, W, xstride) f32, (normals_offset, m2_offset, samples_offset))"""
    rng = np.random.default_rng([seed, height, width, primary_components, int(normals), int(adaptive)])
    xstride, no, mo, so = layout(primary_components, normals, adaptive)
    film = np.zeros((height, width, xstride), F)
    yy, xx = np.mgrid[0:height, 0:width]
    region = ((xx * 3) // max(width, 1) + (yy * 2) // max(height, 1)) % 3       # three surfaces, in blocks
    base = np.array([[0.8, 0.4, 0.1], [0.05, 0.3, 0.6], [2.0, 2.0, 2.0]])[region]
    decade = 10.0 ** rng.integers(-5, 6, (height, width, 1))                      # ten decades
    smooth = rng.random((height, width, 1)) < 0.7                                 # mostly one decade, so that neighbours DO mix
    colour = base * np.where(smooth, 1.0, decade) * (1.0 + 0.2 * rng.standard_normal((height, width, 3)))
    colour = np.abs(colour)
    colour[rng.random((height, width)) < 0.05] = 0.0                              # exact zeros
    film[..., 0:3] = colour
    if primary_components == 4:
        film[..., 3] = rng.random((height, width))
    rel = rng.uniform(0.0, 0.5, (height, width, 3))
    m2 = (rel * colour) ** 2
    m2[rng.random((height, width)) < 0.1] = 0.0                                   # m2 with zeros
    film[..., mo:mo + 3] = m2
    if normals:
        axes = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]])[region]
        nrm = axes + 0.02 * rng.standard_normal((height, width, 3))
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        nrm[rng.random((height, width)) < 0.1] = 0.0                              # missed pixels
        film[..., no:no + 3] = nrm
    if adaptive:
        film[..., so] = rng.integers(2, spp + 1, (height, width))
    flat = film.reshape(-1, xstride)
    npix = height * width
    if npix >= 16:  # the special pixels, apart from each other
        spots = rng.choice(npix, 4, replace=False)
        flat[spots[0], 1] = np.nan
        flat[spots[1], mo] = np.inf
        flat[spots[2], mo + 2] = -abs(flat[spots[2], mo + 2]) - F(1e-3)
        if adaptive:
            flat[spots[3], so] = 1.0
    return film, (no, mo, so)
