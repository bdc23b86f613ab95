"""Cases and helpers of the frame driver's tests (test_frame_cases.py on the oracle alone, test_gpu_frame_shapes.py and
test_gpu_film_sinks.py on the device): films of odd shapes rendered by the oracle strip by strip, and caller-made tile lists.

The oracle, like the reference, takes tile WIDTHS that are multiples of 8 with at most 1024 pixels; it does not restrict the film, and
tiles may overlap.  With the counter sampler a pixel's samples depend on the pixel, the sample index and the seed alone, so a film of
any width >= 8 is the union of 8-wide strips at x = 0, 8, ... and a last one at W - 8 that overlaps its neighbour when 8 does not divide
W.  Under the device's tie rule (set_tie_rule(1): of two triangles hit at the same distance the lower index wins, whatever the order in
which a traversal meets them) a pixel is the same in every strip that holds it, which oracle_film_by_strips asserts bit for bit."""
import numpy as np

DEPTH, SEED = 4, 3
SPPS = (1, 5, 17)  # packets of one, several and many samples per pixel
FILMS = ((17, 13), (67, 5), (100, 3))


def soup(w, h, fov=1.9):
    from phosphorus_mk2_amd import scenes
    return scenes.soup(3000, width=w, height=h, fov=fov)


def cornell(w, h, fov=1.9):
    from phosphorus_mk2_amd import scenes
    return scenes.cornell(w, h, fov)


# "_narrow": through a narrow lens.  A one-row film looks UP by half its single row's height; with the scenes' own field of view (1.9)
# and 8 : 1 pixels that is past everything.
SCENES = {"soup": soup, "cornell": cornell,
          "soup_narrow": lambda w, h: soup(w, h, 0.3), "cornell_narrow": lambda w, h: cornell(w, h, 0.3)}

# (scene, width, height, spp) of every film compared with the oracle.  test_frame_cases.py requires of each that the reference traces
# shadow rays and has a lit pixel; a shape that does not (a 9 x 1 film of either scene traces none) is no case.
ODD_FILMS = [(s, w, h, spp) for s in ("soup", "cornell") for (w, h) in FILMS for spp in SPPS]
# 8 x 1: the one film below 9 pixels wide that the oracle renders (one strip), through the narrow lens
TINY_ORACLE_FILMS = [("cornell_narrow", 8, 1, 5), ("soup_narrow", 8, 1, 5)]
ORACLE_CASES = ODD_FILMS + TINY_ORACLE_FILMS

TINY_FILMS = ((1, 1), (3, 2), (7, 5), (1, 40), (5, 1), (8, 1))
TINY_SPPS = (1, 5)


# ---- the oracle, strip by strip ---------------------------------------------------------------------------------------------------
def strip_positions(width):
    """x of the 8-wide strips that cover `width` columns: 0, 8, ... and, when 8 does not divide width, width - 8"""
    assert width >= 8
    xs = list(range(0, width - 7, 8))
    if width % 8:
        xs.append(width - 8)
    return xs


def strip_tiles(width, height):
    return [(x, 0, 8, height) for x in strip_positions(width)]


RAY_KEYS = ("camera_samples", "rays_closest", "rays_shadow", "rays_masked")


def oracle_film_by_strips(orc, scene, spp, depth, seed, normals=False):
    """-> (film (H, W, 4), normals (H, W, 3) or None, counts) of `scene` at any film width >= 8, one oracle render per strip of
    strip_tiles().  The columns two strips share must agree bit for bit.

    counts sums RAY_KEYS over ALL the strips, so the rays of a column that two strips share are counted twice: it is what a device frame
    over the same tile list (strip_tiles) must count, and it is NOT the count of a frame that renders every pixel once.  (The once-only
    count cannot be had from the oracle: every window it renders is 8 columns wide, and sums over 8-wide windows do not determine the sum
    over the last width % 8 columns.)  On a film whose width is a multiple of 8 nothing overlaps and counts is the frame's."""
    W, H = scene.camera.width, scene.camera.height
    assert 8 * H <= 1024
    film = np.zeros((H, W, 4), np.float32)
    nrm = np.zeros((H, W, 3), np.float32) if normals else None
    done = np.zeros(W, bool)
    counts = dict.fromkeys(RAY_KEYS, 0)
    orc.set_tie_rule(1)
    try:
        O = orc.Oracle(scene, spp=spp, pps=1, depth=depth)
        for (x, y, w, h) in strip_tiles(W, H):
            res = O.render(rng=orc.RNG_COUNTER, seed=seed, threads=1, tiles=[(x, y, w, h)], normals=normals)
            f, st = res[0], res[1]
            outside = np.ones(W, bool); outside[x:x + w] = False
            assert not f[:, outside].any(), "the oracle wrote outside its tile"
            seen = done[x:x + w]
            assert np.array_equal(f[:, x:x + w][:, seen].view(np.uint32), film[:, x:x + w][:, seen].view(np.uint32)), \
                f"strip at x = {x}: columns shared with the previous strip differ"
            film[:, x:x + w] = f[:, x:x + w]
            if normals:
                assert np.array_equal(res[2][:, x:x + w][:, seen].view(np.uint32), nrm[:, x:x + w][:, seen].view(np.uint32))
                nrm[:, x:x + w] = res[2][:, x:x + w]
            done[x:x + w] = True
            for k in RAY_KEYS:
                counts[k] += st[k]
        O.close()
    finally:
        orc.set_tie_rule(0)
    assert done.all()
    return film, nrm, counts


_films = {}


def oracle_case(orc, scene_name, w, h, spp, depth=DEPTH, seed=SEED, normals=False):
    """oracle_film_by_strips of a case of the table, rendered once per session and shared (callers leave the arrays unchanged)"""
    key = (scene_name, w, h, spp, depth, seed, normals)
    if key not in _films:
        film, nrm, counts = oracle_film_by_strips(orc, SCENES[scene_name](w, h), spp, depth, seed, normals)
        film.setflags(write=False)
        if nrm is not None:
            nrm.setflags(write=False)
        _films[key] = (film, nrm, counts)
    return _films[key]


# ---- tile lists ---------------------------------------------------------------------------------------------------------------------
# Each maker: (W, H) -> (tiles [(x, y, w, h)], cover (H, W) int: how often the list claims to cover each pixel).  The claim is written
# down per pixel, independently of the list (test_frame_cases.py paints the list and compares).
def _shuffled(tiles, seed):
    order = np.random.default_rng(seed).permutation(len(tiles))
    return [tiles[i] for i in order]


def grid(W, H, tw, th):
    """tw x th tiles in row order, ragged at the right and bottom edges"""
    return [(x, y, min(tw, W - x), min(th, H - y)) for y in range(0, H, th) for x in range(0, W, tw)]


def shuffled_strips(W, H):
    """8 x 1 strips (the last of a row narrower when 8 does not divide W) in a random order"""
    return _shuffled(grid(W, H, 8, 1), 1), np.ones((H, W), np.int64)


def per_pixel(W, H):
    return _shuffled(grid(W, H, 1, 1), 2), np.ones((H, W), np.int64)


def ragged_5x3(W, H):
    return grid(W, H, 5, 3), np.ones((H, W), np.int64)


def mixed(W, H):
    """rectangles of many sizes: the film is cut in two at a random place, again and again, down to pieces of at most 40 pixels or one
    pixel wide or high; 1 x n, n x 1 and 1 x 1 pieces occur"""
    rng = np.random.default_rng(3)
    out, todo = [], [(0, 0, W, H)]
    while todo:
        x, y, w, h = todo.pop()
        if w * h <= 40 and rng.random() < 0.5 or (w == 1 and h == 1):
            out.append((x, y, w, h))
        elif w > 1 and (h == 1 or rng.random() < 0.6):
            c = int(rng.integers(1, w))
            todo += [(x, y, c, h), (x + c, y, w - c, h)]
        else:
            c = int(rng.integers(1, h))
            todo += [(x, y, w, c), (x, y + c, w, h - c)]
    return _shuffled(out, 4), np.ones((H, W), np.int64)


def whole(W, H):
    return [(0, 0, W, H)], np.ones((H, W), np.int64)


def covered_twice(W, H):
    """the 5 x 3 grid and, in the middle of the list, a 7 x 4 tile across the film's centre that covers 28 pixels (fewer on a film
    below 7 x 4) a second time"""
    tiles = grid(W, H, 5, 3)
    x0, y0 = max(0, W // 2 - 3), max(0, H // 2 - 2)
    extra = (x0, y0, min(7, W - x0), min(4, H - y0))
    tiles.insert(len(tiles) // 2, extra)
    yy, xx = np.mgrid[0:H, 0:W]
    cover = 1 + ((xx >= W // 2 - 3) & (xx < W // 2 + 4) & (yy >= H // 2 - 2) & (yy < H // 2 + 2)).astype(np.int64)
    return tiles, cover


def partial(W, H):
    """the 5 x 3 grid without the tiles whose column + row index is a multiple of 3: two thirds of the film"""
    tiles = [t for t in grid(W, H, 5, 3) if (t[0] // 5 + t[1] // 3) % 3 != 0]
    yy, xx = np.mgrid[0:H, 0:W]
    return tiles, ((xx // 5 + yy // 3) % 3 != 0).astype(np.int64)


TILINGS = {"shuffled_strips": shuffled_strips, "per_pixel": per_pixel, "ragged_5x3": ragged_5x3, "mixed": mixed, "whole": whole,
           "covered_twice": covered_twice, "partial": partial}
TILING_FILMS = (("soup", 72, 40), ("soup", 17, 13))


def shifted_pair(W, H):
    """two partial tile lists A and B of the same number of tiles of the same sizes in the same order, B's shifted by (3, 2): lists
    that differ in their positions alone.  A: one tile in each 6 x 5 cell of a lattice, its size by turns.  -> ((A, cover A), (B, cover B))"""
    sizes = [(4, 3), (2, 1), (1, 4), (5, 1), (3, 3)]
    cells = [(x, y) for y in range(0, H - 2 - 4, 5) for x in range(0, W - 3 - 5, 6)]
    A = [(x, y) + sizes[i % len(sizes)] for i, (x, y) in enumerate(cells)]
    B = [(x + 3, y + 2, w, h) for (x, y, w, h) in A]
    return (A, paint(A, W, H)), (B, paint(B, W, H))


def paint(tiles, W, H):
    """how often the list covers each pixel; a tile must lie inside the film"""
    cover = np.zeros((H, W), np.int64)
    for (x, y, w, h) in tiles:
        assert w > 0 and h > 0 and 0 <= x and x + w <= W and 0 <= y and y + h <= H, (x, y, w, h)
        cover[y:y + h, x:x + w] += 1
    return cover


# ---- device frames into every sink (GPU tests) ----------------------------------------------------------------------------------------
SENTINEL = 12345.0  # finite and odd: no film value, and not the zeros a fresh film holds
HOST_SINKS = ("add_tile", "native")


def default_tiles(xpu, W, H, rank=0, world=1):
    """the 32-pixel grid of Tiles.make as a list, in queue order"""
    q, out = xpu.Tiles.make(W, H, 32, rank, world), []
    while (t := q.next()) is not None:
        out.append(t)
    return out


class DeviceFilm:
    """A film in device memory, (H, W, xstride) float32, from the HIP runtime that the library itself runs on (hipMalloc through ctypes).
    Not a torch tensor: torch's ROCm wheel brings a HIP runtime of its own, which finds no GPU in a process where the library's runtime has
    opened the device first -- and in a pytest session some earlier test has.  bench.py initialises torch first; that order, with a torch
    tensor as the film, is test_gpu_film_sinks.py's child process."""
    H2D, D2H = 1, 2

    def __init__(self, xpu, shape, fill):
        import ctypes as C
        xpu.load_library()  # the runtime is in the process from here on: the soname below names that copy
        self._hip, self._C = C.CDLL("libamdhip64.so.7"), C
        self.shape, self.nbytes = tuple(shape), int(np.prod(shape)) * 4
        p = C.c_void_p()
        self._ok(self._hip.hipMalloc(C.byref(p), C.c_size_t(self.nbytes)), "hipMalloc")
        self.ptr = p.value
        self.fill(fill)

    def _ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    def fill(self, value):
        C, host = self._C, np.full(self.shape, value, np.float32)
        self._ok(self._hip.hipMemcpy(C.c_void_p(self.ptr), host.ctypes.data_as(C.c_void_p), C.c_size_t(self.nbytes), self.H2D), "hipMemcpy")
        # the copy is the null stream's; a frame runs on the device object's own, which does not wait for it
        self._ok(self._hip.hipStreamSynchronize(C.c_void_p(None)), "hipStreamSynchronize")

    def numpy(self):
        C, host = self._C, np.empty(self.shape, np.float32)  # (after join(): the frame's stream has been synchronised)
        self._ok(self._hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), C.c_size_t(self.nbytes), self.D2H), "hipMemcpy")
        return host

    def free(self):
        if self.ptr:
            self._hip.hipFree(self._C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def frame(xpu, dev, scene, seed, tiles=None, host=None, device=False, components=4, normals=False, tensor=None, rank=0, world=1):
    """One frame of `dev` (preprocessed with `scene`).  tiles: a list for CallbackTiles, or None for the native queue of (rank, world).
    host: None, "add_tile" or "native" -- a Film prefilled with SENTINEL; device: a DeviceFilm prefilled with SENTINEL, made and freed
    here, or `tensor`: the caller's DeviceFilm as it is.  -> (host array or None, device film as an array or None, stats)"""
    W, H = scene.camera.width, scene.camera.height
    xs = components + (3 if normals else 0)
    film = None
    if host is not None:
        assert host in HOST_SINKS
        film = xpu.Film(W, H, components, normals)
        film.data[:] = SENTINEL
    mine = tensor is None and device
    if mine:
        tensor = DeviceFilm(xpu, (H, W, xs), SENTINEL)
    if tensor is not None:
        assert tensor.shape == (H, W, xs) and tensor.ptr  # what the scatter writes into
    queue = xpu.Tiles.make(W, H, 32, rank, world) if tiles is None else xpu.CallbackTiles(tiles)
    try:
        dev.start(scene, xpu.FrameState(seed, queue, film, device_film_ptr=None if tensor is None else tensor.ptr, native_sink=host == "native",
                                        primary_components=components, normals=normals))
        dev.join()
        return (None if film is None else film.data), (None if tensor is None else tensor.numpy()), dev.stats()
    finally:
        if mine:
            tensor.free()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_cover(film, full, cover):
    """film: a sink that held SENTINEL everywhere before a frame over a tile list with this cover.  Covered pixels are `full`'s, over the
    whole pixel; the others still hold the sentinel in every component."""
    covered = cover > 0
    assert film.shape == full.shape
    assert same_bits(film[covered], full[covered])
    assert (film[~covered] == np.float32(SENTINEL)).all()
    assert not (full == np.float32(SENTINEL)).any()


def current_hip_device(xpu):
    """hipGetDevice of the calling thread, asked of the HIP runtime that the library itself runs on: the symbol is looked up through the
    library's own handle, which finds it in the runtime the library was linked against, whatever its version (a pytest session may hold
    torch's copy of the runtime as well)"""
    import ctypes as C
    dev = C.c_int(-1)
    rc = xpu.load_library().hipGetDevice(C.byref(dev))
    if rc != 0:
        raise RuntimeError(f"hipGetDevice failed: {rc}")
    return dev.value
