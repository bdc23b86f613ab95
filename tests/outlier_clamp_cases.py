"""Films for the tests of the outlier clamp (tests/test_outlier_clamp.py on the model alone, tests/test_gpu_outlier_clamp.py on the device):
the layouts, heavy-tailed random films with every kind of special pixel, and the synthetic firefly film of DESIGN 23's payoff figure."""
import numpy as np

F, D = np.float32, np.float64

# name -> (xstride_a, m2_offset_a, samples_offset_a): 3 and 4 components, with and without normals, "m2" and "samples", and a wide pixel
# whose channels lie in another order
LAYOUTS = {
    "x6": (6, 3, 0),        # rgb, m2
    "x7": (7, 3, 6),        # rgb, m2, samples
    "x10": (10, 7, 0),      # rgba, normals, m2
    "x11": (11, 7, 10),     # rgba, normals, m2, samples: an accumulator
    "x24": (24, 17, 5),     # samples before m2, and floats of other channels between them
    "x4": (4, 0, 0),        # rgba alone
    "x5": (5, 0, 4),        # rgba, samples, no m2
}
SIZES = [(1, 1), (7, 1), (1, 7), (16, 16), (17, 15), (33, 18), (37, 29)]   # (width, height) around the kernel's 16 x 16 tile and its halo of 1 .. 3


def heavy(rng, W, H, xstride, m2_offset=0, samples_offset=0, specials=True):
    """a film (H, W, xstride) f32 whose every float is set: rgb log-normal over five decades with one pixel in 16 a spike and one in 8 of
    another sign, m2 positive, samples a small count; with `specials` also pixels that are NaN, inf, zero, -0, and samples of 0, -1, NaN"""
    film = rng.normal(size=(H, W, xstride)).astype(F)
    rgb = np.exp(rng.normal(0.0, 2.5, (H, W, 3)))
    rgb *= np.where(rng.random((H, W, 1)) < 1 / 16, 1e3, 1.0)
    rgb *= np.where(rng.random((H, W, 3)) < 1 / 8, -1.0, 1.0)
    film[..., :3] = rgb
    if m2_offset:
        film[..., m2_offset:m2_offset + 3] = np.exp(rng.normal(0.0, 2.0, (H, W, 3)))
    if samples_offset:
        film[..., samples_offset] = rng.choice([1, 2, 4, 16, 37, 64, 1000], (H, W))
    if specials:
        n = H * W
        flat = film.reshape(n, xstride)
        for i, (ch, v) in zip(rng.permutation(n)[:max(n // 6, 1)], [(0, np.nan), (1, np.inf), (2, -np.inf), (0, 0.0), (1, -0.0), (2, 0.0)] * n):
            flat[i, ch] = v
        if samples_offset:
            for i, v in zip(rng.permutation(n)[:max(n // 8, 1)], [0.0, -1.0, np.nan, np.inf, 0.5, 3.0] * n):
                flat[i, samples_offset] = v
    return film


def fireflies(seed, W=128, H=128, spp=16, rate=1e-4, worth=1000.0):
    """DESIGN 23's synthetic film -> (film (H, W, 3) f32, truth (H, W, 3)): a horizontal ramp from 0.5 to 1.5, each pixel the mean of `spp`
    exponential samples of that mean, one sample in 1 / rate a firefly worth `worth` times the mean instead"""
    rng = np.random.default_rng(seed)
    truth = np.broadcast_to(np.linspace(0.5, 1.5, W)[None, :, None], (H, W, 3)).copy()
    s = rng.exponential(1.0, (H, W, spp)) * truth[..., :1]
    hot = rng.random((H, W, spp)) < rate
    s = np.where(hot, worth * truth[..., :1], s)
    film = np.repeat(s.mean(-1, keepdims=True), 3, -1).astype(F)
    return film, truth


def mse(film, truth):
    d = film[..., :3].astype(D) - truth
    return float((d * d).mean())
