"""A float64 numpy model of the outlier clamp (phx_outlier_clamp in include/phx_xpu.h states the rule operation by operation),
written from the rule's text and sharing no code with the library.  Every pixel is computed at once, tap by tap in tap order, so each
pixel's sums run in the order the rule gives; numpy's float64 +, -, *, / and sqrt are IEEE operations, as the device's are.  The device is
held to this model bit for bit (tests/test_gpu_outlier_clamp.py)."""
import numpy as np

F, D = np.float32, np.float64
EXCLUDE_CENTRE, UPPER_ONLY = 1, 2
CLASSES = ("skipped", "unbounded", "inside", "clamped")


def taps_of(radius, flags):
    """the window's offsets (dx, dy) in tap order: dy outer, dx inner"""
    r = int(radius)
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if not (flags & EXCLUDE_CENTRE and dx == 0 and dy == 0)]


def bounds(A_rgb_shape, B, radius, gamma, floor, trim, flags):
    """-> (k, lo, hi): the number of taps left (H, W) and the bounds (H, W, 3) of every pixel, from film B's "primary" rgb"""
    H, W = A_rgb_shape[:2]
    r = int(radius)
    pad = np.full((H + 2 * r, W + 2 * r, 3), np.nan, D)   # outside the film: a tap that does not count, like a non-finite one
    pad[r:r + H, r:r + W] = B[..., :3].astype(D)
    taps = taps_of(radius, flags)
    val = np.stack([pad[r + dy:r + dy + H, r + dx:r + dx + W] for dx, dy in taps])              # (T, H, W, 3)
    counts = np.isfinite(val).all(-1)                                                           # (T, H, W)
    with np.errstate(invalid="ignore"):
        lum = (0.2126 * val[..., 0] + 0.7152 * val[..., 1]) + 0.0722 * val[..., 2]
    for _ in range(int(trim)):
        l = np.where(counts, lum, -np.inf)
        first = np.argmax(l, axis=0)                      # the largest, among equals the earliest in tap order
        drop = counts.any(0)
        ys, xs = np.nonzero(drop)
        counts[first[ys, xs], ys, xs] = False
    k = counts.sum(0)
    g, fl = D(F(gamma)), D(F(floor))
    with np.errstate(invalid="ignore", divide="ignore"):
        total = np.zeros((H, W, 3), D)
        for t in range(len(taps)):
            total = np.where(counts[t][..., None], total + val[t], total)
        mu = total / k[..., None]
        spread = np.zeros((H, W, 3), D)
        for t in range(len(taps)):
            d = val[t] - mu
            spread = np.where(counts[t][..., None], spread + d * d, spread)
        s = spread / k[..., None]
        w = g * np.sqrt(s) + fl
        return k, mu - w, mu + w


def clamp(A, B, m2_offset, samples_offset, radius=2, gamma=4.0, floor=0.0, trim=2, min_taps=4, flags=EXCLUDE_CENTRE | UPPER_ONLY, clamped_history=0):
    """films A (H, W, xa) and B (H, W, xb) f32 -> (out, summary, classes): out of A's shape; classes (H, W) indexes CLASSES"""
    A = np.ascontiguousarray(A, F)
    out = A.copy()
    a = A[..., :3].astype(D)
    skipped = ~np.isfinite(a).all(-1)
    n = None
    if samples_offset:
        n = A[..., samples_offset].astype(D)
        with np.errstate(invalid="ignore"):
            skipped |= ~(np.isfinite(n) & (n > 0))
    k, lo, hi = bounds(a.shape, B, radius, gamma, floor, trim, flags)
    unbounded = ~skipped & (k < int(min_taps))
    live = ~skipped & ~unbounded
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        up = live[..., None] & (a > hi)
        down = live[..., None] & ~up & (a < lo) if not flags & UPPER_ONLY else np.zeros_like(up)
        new = np.where(up, hi.astype(F), np.where(down, lo.astype(F), A[..., :3]))
        cl = up | down
        out[..., :3][cl] = new[cl]
        any_ = cl.any(-1)
        applied = np.zeros_like(cl)
        v = None
        if m2_offset:
            v = A[..., m2_offset:m2_offset + 3].astype(D)
            f = new.astype(D) / a
            applied = cl & (a != 0) & (f >= 0) & (f < 1)
            v = np.where(applied, (v * f) * f, v)
        capped = np.zeros_like(any_)
        if clamped_history > 0:
            ch = D(int(clamped_history))
            capped = any_ & (n > ch)
            out[..., samples_offset][capped] = F(ch)
            if m2_offset:
                v = np.where(capped[..., None], v * (n / ch)[..., None], v)
                applied = applied | capped[..., None]
        if m2_offset:
            out[..., m2_offset:m2_offset + 3][applied] = v.astype(F)[applied]
    classes = np.where(skipped, 0, np.where(unbounded, 1, np.where(any_, 3, 2)))
    summary = {"pixels": int(classes.size), "skipped": int(skipped.sum()), "unbounded": int(unbounded.sum()), "inside": int((classes == 2).sum()),
               "clamped": int((classes == 3).sum()), "capped": int(capped.sum())}
    return out, summary, classes


def same(a, b):
    """bit for bit"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
