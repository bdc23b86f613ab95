"""The float64 model of reprojection (phx_reproject in include/phx_xpu.h states the rule; csrc/reproject.hip is held to this bit for bit).

numpy only, no code shared with the library.  Every operation is one binary64 operation in the header's order: numpy evaluates a * b + c as
two rounded operations, never as an fma."""
import math

import numpy as np

F, D = np.float32, np.float64


class Camera:
    """a camera as the rule derives it from (to_world 4 x 4 fp32, fov fp32, film width, film height); None from derive() when refused"""

    def __init__(self, o, inv, zoom, ratio, w, h):
        self.o, self.inv, self.zoom, self.ratio, self.w, self.h = o, inv, zoom, ratio, w, h


def derive(to_world, fov, width, height):
    M = np.asarray(to_world, F).reshape(4, 4).astype(D)
    (a, b, c), (d, e, f), (g, h, k) = M[0, :3], M[1, :3], M[2, :3]
    with np.errstate(all="ignore"):
        A, B, Cc = e * k - f * h, f * g - d * k, d * h - e * g
        det = (a * A + b * B) + c * Cc
        if not np.isfinite(det) or det == 0.0 or width == 0 or height == 0:
            return None
        inv = np.array([[A / det, (c * h - b * k) / det, (b * f - c * e) / det],
                        [B / det, (a * k - c * g) / det, (c * d - a * f) / det],
                        [Cc / det, (b * g - a * h) / det, (a * e - b * d) / det]], D)
    o = M[3, :3].copy()
    fov = float(D(F(fov)))
    zoom = 1.12 * math.tan(fov * 0.5) if math.isfinite(fov) else math.nan  # (math.tan raises on an infinity where libm returns a NaN)
    if not (np.isfinite(inv).all() and np.isfinite(o).all() and math.isfinite(zoom) and zoom != 0.0):
        return None
    return Camera(o, inv, D(zoom), D(width) / D(height), D(width), D(height))


def project(K, X):
    """X (..., 3) f64 -> (in front of the camera, fx, fy)"""
    with np.errstate(all="ignore"):
        dx, dy, dz = X[..., 0] - K.o[0], X[..., 1] - K.o[1], X[..., 2] - K.o[2]
        c = [(dx * K.inv[0, j] + dy * K.inv[1, j]) + dz * K.inv[2, j] for j in range(3)]
        front = c[2] < 0.0
        t = -c[2]
        fx = ((c[0] / t) / (K.ratio * K.zoom) + 0.5) * K.w
        fy = (0.5 - (c[1] / t) / K.zoom) * K.h
    return front, fx, fy


def valid_pixels(acc, offs):
    """phx_denoise's definition with the pixel's own samples"""
    no, mo, so = offs
    n = acc[..., so].astype(D)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(acc[..., 0:3]).all(-1) & np.isfinite(acc[..., mo:mo + 3]).all(-1) & np.isfinite(acc[..., no:no + 3]).all(-1) &
                (acc[..., mo:mo + 3] >= 0).all(-1) & np.isfinite(n) & (n >= 2.0))


def reproject(acc, guides_from, guides_to, cam_from, cam_to, offs, sigma_plane=1.0, sigma_dist=4.0, max_history=64):
    """acc (H, W, xa) f32, guides_* (H, W, >= 8) f32, cam_* Camera, offs = (normals, m2, samples) offsets
    -> (acc_to (H, W, xa) f32, summary dict)"""
    acc, gf, gt = np.asarray(acc, F), np.asarray(guides_from, F), np.asarray(guides_to, F)
    H, W, xa = acc.shape
    no, mo, so = offs
    sp, sd, mh = D(F(sigma_plane)), D(F(sigma_dist)), D(max_history)
    out = np.zeros_like(acc)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        geometry = gt[..., 3] > 0
        X = gt[..., 4:7].astype(D)
        fa, fxa, fya = project(cam_from, X)
        fb, fxb, fyb = project(cam_to, X)
        sx, sy = xs.astype(D) + (fxa - fxb), ys.astype(D) + (fya - fyb)
        inside = geometry & fa & fb & (sx > -1.0) & (sx < D(W)) & (sy > -1.0) & (sy < D(H))
        sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
        x0, y0 = np.floor(sx), np.floor(sy)
        tx, ty = sx - x0, sy - y0
        plane_scale = cam_from.zoom / cam_from.h
        ok_pixel = valid_pixels(acc, offs) & np.isfinite(gf[..., 0:8]).all(-1) & (gf[..., 3] > 0)
        taps = []
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            w = (tx if k & 1 else 1.0 - tx) * (ty if k >> 1 else 1.0 - ty)
            counts = inside & (w > 0.0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            ix, iy = np.where(counts, qx, 0).astype(np.int64), np.where(counts, qy, 0).astype(np.int64)
            counts &= ok_pixel[iy, ix]
            a, g = acc[iy, ix], gf[iy, ix]
            dX = X - g[..., 4:7].astype(D)
            N = a[..., no:no + 3].astype(D)
            tol = plane_scale * g[..., 7].astype(D)
            r = (N[..., 0] * dX[..., 0] + N[..., 1] * dX[..., 1]) + N[..., 2] * dX[..., 2]
            dd = (dX[..., 0] * dX[..., 0] + dX[..., 1] * dX[..., 1]) + dX[..., 2] * dX[..., 2]
            lim = sd * tol
            counts &= (np.abs(r) <= sp * tol) & (dd <= lim * lim)
            taps.append((counts, w, a))
        # sums that start at their first term
        def total(terms):
            s, started = None, np.zeros((H, W), bool)
            for counts, t in terms:
                s = np.where(counts, t, 0.0) if s is None else np.where(counts, np.where(started, s + t, t), s)
                started = started | counts
            return s
        wsum = total([(c, w) for c, w, _ in taps])
        reused = np.any([c for c, _, _ in taps], axis=0)
        u = [w / wsum for _, w, _ in taps]
        n = total([(c, ui * a[..., so].astype(D)) for (c, _, a), ui in zip(taps, u)])
        V = [total([(c, ui * a[..., ch].astype(D)) for (c, _, a), ui in zip(taps, u)]) for ch in range(3)]
        m = [total([(c, (ui * ui) * a[..., mo + ch].astype(D)) for (c, _, a), ui in zip(taps, u)]) for ch in range(3)]
        n_out = np.where(n < mh, n, mh)
        bites = n > n_out
        m = [np.where(bites, mc * (n / n_out), mc) for mc in m]
        # every other float: the counting tap of largest weight, ties to the first
        wbest = np.zeros((H, W), D)
        for counts, w, a in taps:
            better = counts & (w > wbest)
            out[better] = a[better]
            wbest = np.where(better, w, wbest)
        for ch in range(3):
            out[..., ch] = np.where(reused, V[ch].astype(F), F(0))
            out[..., mo + ch] = np.where(reused, m[ch].astype(F), F(0))
        out[..., so] = np.where(reused, n_out.astype(F), F(0))
        out[~reused] = 0
    summary = {"pixels": H * W, "reused": int(reused.sum()), "no_geometry": int((~geometry).sum()), "disoccluded": int((geometry & ~reused).sum()),
               "samples": int(sum(int(v) for v in out[..., so][reused].astype(D)))}
    return out, summary


def same(a, b):
    """bit for bit, a NaN matching a NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
