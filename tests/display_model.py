"""The display pass's rule (phx_display in include/phx_xpu.h) as a model: numpy fp32 in the rule's order, the oracle's powf_
(orc_exp_log_pow, which tests/test_oracle_math.py pins) and Python integers for the exposure.  It shares no code with csrc/display_rule.h;
tests/test_display.py holds that header, compiled for the host, to this model bit for bit, and tests/test_gpu_display.py the device."""
import numpy as np

F, D = np.float32, np.float64
DITHER, AUTO = 1, 2
CLAMP, REINHARD, ACES = 0, 1, 2
TONES = {"clamp": CLAMP, "reinhard": REINHARD, "aces": ACES}
INVALID, UNLIT = 256, 257  # what bins() answers for a pixel in no bin
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.float32)
DEFAULTS = dict(scale=1.0, tone=ACES, white=4.0, flags=DITHER, key=0.18, low_q16=32768, high_q16=62259, min_scale=2.0 ** -12, max_scale=2.0 ** 12)


def powf(x, y):
    """the oracle's powf_ on fp32 arrays of one shape"""
    from oracle import oracle as orc
    x = np.ascontiguousarray(x, F)
    y = np.ascontiguousarray(np.broadcast_to(F(y), x.shape), F)
    e, l, p = np.empty(x.size, F), np.empty(x.size, F), np.empty(x.size, F)
    with np.errstate(all="ignore"):
        orc.load().orc_exp_log_pow(x.size, orc._fp(x.ravel()), orc._fp(y.ravel()), orc._fp(e), orc._fp(l), orc._fp(p))
    return p.reshape(x.shape)


def bins(rgb):
    """rgb (..., 3) f32 -> per pixel its bin 0 .. 255, INVALID or UNLIT"""
    rgb = np.asarray(rgb, F)
    r, g, b = (rgb[..., c].astype(D) for c in range(3))
    with np.errstate(all="ignore"):
        Y = ((D(0.2126) * r + D(0.7152) * g) + D(0.0722) * b).astype(F)
    k = np.clip((np.ascontiguousarray(Y).view(np.uint32) >> 20).astype(np.int64) - 888, 0, 255)
    k = np.where(Y <= 0, UNLIT, k)
    return np.where(np.isfinite(rgb).all(axis=-1), k, INVALID)


def histogram(rgb):
    """-> (the 256 counts as Python integers, invalid, unlit)"""
    c = np.bincount(bins(rgb).ravel(), minlength=258)
    return [int(v) for v in c[:256]], int(c[INVALID]), int(c[UNLIT])


def exposure(h, fallback, key, low_q16, high_q16, min_scale, max_scale):
    """the exposure rule on 256 integer counts -> (scale f32, from_histogram)"""
    N = sum(h)
    if N == 0:
        return F(fallback), 0
    c_lo, c_hi = (N * low_q16) >> 16, (N * high_q16 + 65535) >> 16
    C = W = S = 0
    for k in range(256):
        w = min(C + h[k], c_hi) - max(C, c_lo)
        if w > 0:
            W += w
            S += w * (2 * k + 1)
        C += h[k]
    assert S < 2 ** 53 and 16 * W < 2 ** 53
    p = F(float(S) / float(16 * W) - 16.0)
    Ybar = powf(np.array([2.0], F), p)[0]
    with np.errstate(all="ignore"):
        return np.minimum(np.maximum(F(key) / Ybar, F(min_scale)), F(max_scale)), 1


def tone_curve(x, tone, white):
    if tone == REINHARD:
        w = F(white)
        return (x * (F(1) + x / (w * w))) / (F(1) + x)
    if tone == ACES:
        return (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
    assert tone == CLAMP
    return x


def codes(v, scale, tone, white, d):
    """the codes (uint8) of the values v (f32, any shape) under one scale; d: 0.5, or an array that broadcasts against v"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        x = F(scale) * v
        x = np.where(x > 0, x, F(0))
        x = np.minimum(x, F(65536))
        t = np.fmin(tone_curve(x, tone, white), F(1))
        e = np.where(t <= F(0.0031308), F(12.92) * t, F(1.055) * powf(t, F(1) / F(2.4)) - F(0.055))
        q = F(255) * e + np.asarray(d, F)
    assert q.dtype == F and (q >= 0).all() and (q < 256).all()
    return q.astype(np.int32).astype(np.uint8)


def dither_plane(height, width, on):
    """d of every pixel (height, width, 1)"""
    if not on:
        return np.full((height, width, 1), 0.5, F)
    y, x = np.mgrid[0:height, 0:width]
    return ((BAYER[y & 3, x & 3] + F(0.5)) / F(16))[..., None]


def display(film, scale=1.0, tone=ACES, white=4.0, flags=DITHER, key=0.18, low_q16=32768, high_q16=62259, min_scale=2.0 ** -12, max_scale=2.0 ** 12):
    """film (H, W, >= 3) f32 -> (image (H, W, 4) uint8, summary): what phx_dev_film_display writes and reports for these settings; the
    summary as HipDevice.display gives it, with the 256 counts under "histogram" """
    film = np.asarray(film, F)
    H, W = film.shape[:2]
    rgb = film[..., :3]
    h, invalid, unlit = histogram(rgb)
    s, from_histogram = (F(scale), 0)
    if flags & AUTO:
        s, from_histogram = exposure(h, scale, key, low_q16, high_q16, min_scale, max_scale)
    image = np.full((H, W, 4), 255, np.uint8)
    image[..., :3] = codes(rgb, s, tone, white, dither_plane(H, W, flags & DITHER))
    return image, dict(pixels=H * W, invalid=invalid, unlit=unlit, counted=sum(h), scale=float(s), from_histogram=from_histogram,
                       histogram=np.array(h, np.uint64))


def srgb_decode(code):
    """the inverse transfer function of code / 255, in binary64 (a property's input, no part of the rule)"""
    c = np.asarray(code, D) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def synthetic_film(shape, xstride=4, seed=1, special=True):
    """(H, W, xstride) f32: log-uniform radiance over 2^-18 .. 2^6 (past the histogram's low end), floats behind the colour that no call may
    read (NaN), and, when the film has room, one pixel of every special kind: NaN, +inf, -inf, negative, zero, -0, huge and tiny"""
    H, W = shape
    rng = np.random.default_rng(seed)
    film = np.full((H, W, xstride), np.nan, F)
    film[..., :3] = np.exp2(rng.uniform(-18.0, 6.0, (H, W, 3))).astype(F)
    flat = film.reshape(-1, xstride)
    kinds = [(np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (-1, -2, -3), (0, 0, 0), (-0.0, 0.5, 0.25), (1e30, 1e-30, 3.4e38), (1e-40, 1e-42, 0), (-5, 0.001, 0.001)]
    if special and len(flat) >= 3 * len(kinds):
        where = rng.choice(len(flat), len(kinds), replace=False)
        for i, k in zip(where, kinds):
            flat[i, :3] = k
    return film
