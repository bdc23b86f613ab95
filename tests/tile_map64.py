"""The rule of the tile map (phx_tile_map in include/phx_xpu.h) restated in float64 numpy: a plain loop over the tiles of the grid, and inside
a tile every line is one IEEE operation applied to the tile's pixels at once, so a pixel sees exactly the sequence of binary64 operations the
header writes down.  Every per-tile quantity is an integer count or a maximum of non-negative non-NaN floats, so no order of reduction shows.
Nothing here reads the C++ or the kernel."""
import numpy as np

F, D = np.float32, np.float64
TWO53 = 2 ** 53

# a phx_tile_record as numpy reads it (40 bytes)
RECORD = np.dtype([("x", np.uint32), ("y", np.uint32), ("w", np.uint32), ("h", np.uint32), ("invalid", np.uint32), ("starved", np.uint32),
                   ("converged", np.uint32), ("worst", np.float32), ("samples", np.uint64)])
assert RECORD.itemsize == 40


def grid(width, height, tile_width, tile_height):
    """-> the tiles (x, y, w, h) of the grid in the records' order: rows top to bottom, tiles left to right"""
    tx, ty = -(-width // tile_width), -(-height // tile_height)
    return [(i * tile_width, j * tile_height, min(tile_width, width - i * tile_width), min(tile_height, height - j * tile_height))
            for j in range(ty) for i in range(tx)]


def pixels(film, m2_offset, samples_offset, tau, floor):
    """film (..., xstride) f32 -> per pixel: valid, starved, converged (bool) and r (f32; 0 where the pixel is not valid), n (f64)"""
    film = np.asarray(film, F)
    V, m = film[..., 0:3].astype(D), film[..., m2_offset:m2_offset + 3].astype(D)
    n = film[..., samples_offset].astype(D)
    tau, floor = D(F(tau)), D(F(floor))
    with np.errstate(all="ignore"):
        valid = np.isfinite(V).all(-1) & np.isfinite(m).all(-1) & (m >= 0).all(-1) & np.isfinite(n) & (n >= 2)
        starved = np.isfinite(n) & (n >= 0) & (n < 2)
        q = n / (n - D(1))
        L = m * q[..., None]
        den = np.fabs(V) + floor
        b = tau * den
        ok = (L <= b * b).all(-1)
        r_c = np.where(den > 0, np.sqrt(L) / den, np.where(L == 0, D(0), D(np.inf)))
        r = np.where(valid, r_c.max(-1), D(0)).astype(F)
    return valid, starved, valid & ok, r, n


def tile_map(film, m2_offset, samples_offset, tile_width, tile_height, tau, floor=0.0):
    """film (H, W, xstride) f32 -> (records (tiles,) RECORD, summary dict): phx_dev_film_tile_map's outputs"""
    film = np.asarray(film, F)
    H, W = film.shape[:2]
    tiles = grid(W, H, tile_width, tile_height)
    records = np.zeros(len(tiles), RECORD)
    n_open = 0
    for k, (x, y, w, h) in enumerate(tiles):
        valid, starved, converged, r, n = pixels(film[y:y + h, x:x + w], m2_offset, samples_offset, tau, floor)
        rec = records[k]
        rec["x"], rec["y"], rec["w"], rec["h"] = x, y, w, h
        rec["invalid"], rec["starved"], rec["converged"] = int((~valid).sum()), int(starved.sum()), int(converged.sum())
        rec["samples"] = sum(int(min(v, TWO53)) for v in n[valid].ravel().tolist()) % (1 << 64)
        rec["worst"] = r[valid].max() if valid.any() else F(0.0)  # (+0.0: the r of a pixel is never -0.0)
        n_open += int(is_open(rec))
    total = lambda f: int(sum(int(v) for v in records[f])) % (1 << 64)
    return records, {"pixels": W * H, "invalid": total("invalid"), "converged": total("converged"), "samples": total("samples"),
                     "tiles": len(tiles), "open": n_open}


def is_open(rec, coverage=1.0):
    """coverage == 1: the rule's open tile.  coverage < 1 is the progressive loop's: closed once converged >= coverage * (w * h - invalid) and
    starved == 0"""
    valid = int(rec["w"]) * int(rec["h"]) - int(rec["invalid"])
    if coverage >= 1.0:
        return int(rec["converged"]) < valid or int(rec["starved"]) > 0
    return not (int(rec["converged"]) >= coverage * valid and int(rec["starved"]) == 0)


def open_tiles(records, coverage=1.0):
    return [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in records if is_open(r, coverage)]


def same_records(a, b):
    """bit for bit, `worst` included"""
    return a.dtype == b.dtype == RECORD and a.shape == b.shape and a.tobytes() == b.tobytes()


SPECIALS = ["NaN colour", "inf m2", "m2 < 0", "n == 0", "n == 1", "n == 2", "n == 2^60", "NaN count", "negative count", "den == 0, L == 0", "den == 0, L > 0",
            "m2 == 0", "huge r"]


def synthetic_film(shape, xstride=8, m2_offset=4, samples_offset=7, seed=0, specials=True):
    """An accumulator film (H, W, xstride) that reaches every branch of the rule: colours over ten decades, relative errors on both sides of
    any sensible tau, counts of 2 .. 64, foreign floats in every float outside the seven that are read, and, where the film has 32 pixels or
    more, one pixel for each of SPECIALS -> (film, {special: (y, x)})"""
    H, W = shape
    rng = np.random.default_rng([seed, H, W, xstride, m2_offset, samples_offset])
    npix = H * W
    f = rng.uniform(-1e6, 1e6, (npix, xstride)).astype(F)  # the foreign floats
    foreign = [c for c in range(3, xstride) if not (m2_offset <= c < m2_offset + 3) and c != samples_offset]
    if foreign:
        f[rng.random(npix) < 0.1, foreign[0]] = np.nan  # a NaN nobody reads
    colour = rng.uniform(0.1, 2.0, (npix, 3)) * 10.0 ** rng.integers(-5, 6, (npix, 1)) * rng.choice([-1.0, 1.0], (npix, 3), p=[0.1, 0.9])
    f[:, 0:3] = colour
    f[:, m2_offset:m2_offset + 3] = (10.0 ** rng.uniform(-3, 0, (npix, 3)) * colour) ** 2
    f[:, samples_offset] = rng.integers(2, 65, npix)
    at = {}
    if specials and npix >= 32:
        at = dict(zip(SPECIALS, (int(v) for v in rng.choice(npix, len(SPECIALS), replace=False))))
        f[at["NaN colour"], 1] = np.nan
        f[at["inf m2"], m2_offset + 2] = np.inf
        f[at["m2 < 0"], m2_offset] = -1e-3
        for name, v in (("n == 0", 0.0), ("n == 1", 1.0), ("n == 2", 2.0), ("n == 2^60", 2.0 ** 60), ("NaN count", np.nan), ("negative count", -3.0)):
            f[at[name], samples_offset] = v
        f[at["n == 0"], 0:3] = np.nan  # starved whatever the other floats hold
        f[at["den == 0, L == 0"], 0:3] = 0; f[at["den == 0, L == 0"], m2_offset:m2_offset + 3] = 0
        f[at["den == 0, L > 0"], 0] = 0
        f[at["m2 == 0"], m2_offset:m2_offset + 3] = 0
        f[at["huge r"], 2] = 1e-30; f[at["huge r"], m2_offset + 2] = 1e30  # sqrt(L) / den is finite in binary64 and rounds to +inf in fp32
        at = {k: divmod(v, W) for k, v in at.items()}
    return f.reshape(H, W, xstride), at
