"""What is known of a film without a device library: the pixel's layout, the in-memory film sinks, the settings structs of the
film passes (include/phx_xpu.h) with their argument refusals, and the tile map's grid.  Pure arithmetic over numpy and the ABI's structs:
device.py, the binding, calls the library with these."""
import collections
import math
import threading

import numpy as np

from . import abi

FilmLayout = collections.namedtuple("FilmLayout", "normals_offset m2_offset samples_offset xstride")


def film_layout(primary_components=4, normals=False, moments=False, samples=False):
    """The channel order of a film's pixel, derived here and nowhere else: "primary", then "normals" (3 floats), "m2" (3 floats) and "samples"
    (1 float), each only when asked for -> (normals_offset, m2_offset, samples_offset, xstride); the offset of a channel that is not there
    is 0, as in the structs of include/phx_xpu.h."""
    xstride, offsets = primary_components, []
    for there, floats in ((normals, 3), (moments, 3), (samples, 1)):
        offsets.append(xstride if there else 0)
        xstride += floats if there else 0
    return FilmLayout(offsets[0], offsets[1], offsets[2], xstride)


class Film:
    """An in-memory film sink: film_t<>::add_tile copies a tile's render buffer into a full frame
    (what film::file_t / the Blender sink do, src/film/file.cpp:27-41)."""

    def __init__(self, width, height, primary_components=4, normals=False, moments=False, adaptive=False):
        if adaptive and not moments:
            raise ValueError("a film of adaptive sampling needs moments=True (phx_dev_start refuses the frame otherwise)")
        self.width, self.height = width, height
        self.primary_components, self.normals, self.moments, self.adaptive = primary_components, normals, moments, adaptive
        # channel "m2" (phx_frame.moments_channel), when asked for, sits behind "primary" and "normals"; channel "samples" (adaptive sampling:
        # the device adds it to every frame started while HipDevice.set_adaptive is on) behind "m2".  A film without them says where they would be
        widest = film_layout(primary_components, normals, True, True)
        self.m2_offset, self.samples_offset = widest.m2_offset, widest.samples_offset
        self.xstride = film_layout(primary_components, normals, moments, adaptive).xstride
        self.data = np.zeros((height, width, self.xstride), np.float32)
        self.tiles = 0
        self._lock = threading.Lock()

    def add_tile(self, x, y, w, h, buffer, xstride, ystride):
        src = np.ctypeslib.as_array(buffer, shape=(h * ystride,)).reshape(h, w, xstride)
        with self._lock:
            self.data[y:y + h, x:x + w, :] = src
            self.tiles += 1

    @property
    def primary(self):
        return self.data[..., :3]

    @property
    def m2(self):
        """channel "m2": per pixel and colour the centred second moment of the samples the film summed (see film_variance)"""
        if not self.moments:
            raise AttributeError("this film was made without moments=True")
        return self.data[..., self.m2_offset:self.m2_offset + 3]

    @property
    def samples(self):
        """channel "samples": (float)n per pixel, the samples the pixel took under adaptive sampling"""
        if not self.adaptive:
            raise AttributeError("this film was made without adaptive=True")
        return self.data[..., self.samples_offset]


class BottomUpFilm(Film):
    """The Blender-style sink (plugins/blender/sink.cpp:34-69): the host's (0,0) is the BOTTOM-left pixel, so a tile lands at
    row `height - h - y` with its rows reversed, and the alpha of channel "primary" is set to one (sink.cpp:61-63).
    Needs the add_tile callback path (FrameState.native_sink = False): the flip happens per tile, as in the reference."""

    def add_tile(self, x, y, w, h, buffer, xstride, ystride):
        src = np.ctypeslib.as_array(buffer, shape=(h * ystride,)).reshape(h, w, xstride)
        inv_y = self.height - h - y
        with self._lock:
            self.data[inv_y:inv_y + h, x:x + w, :] = src[::-1]
            if self.primary_components == 4:
                self.data[inv_y:inv_y + h, x:x + w, 3] = 1.0
            self.tiles += 1


def film_variance(data, spp, primary_components=4, normals=False, adaptive=False):
    """The unbiased estimate of the variance of every pixel's film value from a film rendered with moments=True: data (..., xstride) as
    render() returns it -> m2 * S / (S - 1) in float64, shape (..., 3); S = spp.  The film value is a SUM of S samples y_s (each carries the
    film's 1 / (spp * pps)), and m2 is their centred sum of squares, so S / (S - 1) * m2 estimates S * var(y).  spp == 1 says nothing: inf.
    adaptive=True: a film of adaptive sampling (one more float per pixel, "samples"): m2 * n / (n - 1) from the pixel's OWN n, which holds
    after the rescale of a pixel that stopped as well; inf where n <= 1.  spp is not used then."""
    data = np.asarray(data)
    lay = film_layout(primary_components, normals, True, adaptive)
    if data.shape[-1] != lay.xstride:
        raise ValueError(f"film_variance: a film with the m2 channel has {lay.xstride} floats per pixel, this one {data.shape[-1]}")
    m2 = data[..., lay.m2_offset:lay.m2_offset + 3].astype(np.float64)
    if adaptive:
        n = data[..., lay.samples_offset].astype(np.float64)[..., None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 1, m2 * (n / (n - 1.0)), np.inf)
    if spp <= 1:
        return np.full(m2.shape, np.inf)
    return m2 * (spp / (spp - 1.0))


def guide_plane_scale(camera):
    """phx_denoise_guides.plane_scale of a camera (CameraDesc): the world size of one film pixel at unit distance.  The film's height at unit
    distance is the camera kernel's zoom, 1.12 * tan(fov / 2) (camera.hpp:113)."""
    return 1.12 * math.tan(0.5 * float(camera.fov)) / float(camera.height)


def denoise_settings(shape, spp, primary_components=4, normals=False, adaptive=False, iterations=5, sigma_l=4.0, normal_power_log2=7):
    """abi.Denoise for a film of `shape` (H, W, xstride) with the channels derived as Film derives them: "normals" behind "primary", "m2"
    behind them, "samples" behind "m2".  ValueError for a film without the channel m2 (render it with moments=True)."""
    if len(shape) != 3:
        raise ValueError("denoise: the film must be (height, width, xstride)")
    H, W, xstride = (int(v) for v in shape)
    normals_offset, m2_offset, samples_offset, want = film_layout(primary_components, normals, True, adaptive)
    if xstride != want:
        raise ValueError(f"denoise: a film with the m2 channel has {want} floats per pixel in this layout, this one {xstride} "
                         "(the denoiser needs a film rendered with moments=True)")
    return abi.Denoise(width=W, height=H, xstride=xstride, normals_offset=normals_offset, m2_offset=m2_offset,
                       samples_offset=samples_offset, spp=int(spp), iterations=int(iterations), sigma_l=float(sigma_l),
                       normal_power_log2=int(normal_power_log2), on_device=0)


def accumulator(width, height, primary_components=4, normals=False):
    """A zeroed film in the accumulator's layout (HipDevice.accumulate): "primary", "normals" when asked for, "m2" and always "samples", which
    is the layout of an adaptive film, so HipDevice.denoise(..., adaptive=True) and film_variance(..., adaptive=True) read it as it is
    -> (H, W, xstride) f32.  Accumulating a frame into it is the copy."""
    return Film(width, height, primary_components, normals, True, True).data


def accumulate_settings(shape_a, shape_b, spp, primary_components=4, normals=False, frame_adaptive=False, threshold=0.0, floor=0.0):
    """abi.Accumulate for an accumulator of shape_a and a frame film of shape_b (H, W, xstride each) with the channels derived as Film derives
    them; both films have the same primary_components and normals, the accumulator always has "samples", the frame film when frame_adaptive.
    ValueError for films of different sizes or without the channel m2 (render the frame with moments=True)."""
    if len(shape_a) != 3 or len(shape_b) != 3:
        raise ValueError("accumulate: both films must be (height, width, xstride)")
    (H, W, xa), (Hb, Wb, xb) = ((int(v) for v in s) for s in (shape_a, shape_b))
    if (H, W) != (Hb, Wb):
        raise ValueError(f"accumulate: the accumulator is {W} x {H} pixels, the frame film {Wb} x {Hb}")
    a, b = film_layout(primary_components, normals, True, True), film_layout(primary_components, normals, True, frame_adaptive)
    if xa != a.xstride:
        raise ValueError(f"accumulate: an accumulator has {a.xstride} floats per pixel in this layout (xpu.accumulator), this one {xa}")
    if xb != b.xstride:
        raise ValueError(f"accumulate: a frame film with the m2 channel has {b.xstride} floats per pixel in this layout, this one {xb} "
                         "(accumulation needs frames rendered with moments=True)")
    return abi.Accumulate(width=W, height=H, xstride_a=xa, normals_offset_a=a.normals_offset, m2_offset_a=a.m2_offset, samples_offset_a=a.samples_offset,
                          xstride_b=xb, normals_offset_b=b.normals_offset, m2_offset_b=b.m2_offset, samples_offset_b=b.samples_offset,
                          spp_b=int(spp), on_device=0, tau=float(threshold), floor=float(floor))


# a phx_tile_record as numpy reads it (40 bytes, abi.TileRecord)
TILE_RECORD = np.dtype([("x", np.uint32), ("y", np.uint32), ("w", np.uint32), ("h", np.uint32), ("invalid", np.uint32), ("starved", np.uint32),
                        ("converged", np.uint32), ("worst", np.float32), ("samples", np.uint64)])


def tile_map_settings(shape, tile_size=32, threshold=0.0, floor=0.0, primary_components=4, normals=False):
    """abi.TileMap for an accumulator film of `shape` (H, W, xstride) with the channels derived as Film derives them (xpu.accumulator's
    layout) and a grid of tile_size x tile_size tiles (an int, or (tile_width, tile_height)).  ValueError for a film of another layout."""
    if len(shape) != 3:
        raise ValueError("tile_map: the film must be (height, width, xstride)")
    H, W, xs = (int(v) for v in shape)
    lay = film_layout(primary_components, normals, True, True)
    if xs != lay.xstride:
        raise ValueError(f"tile_map: an accumulator has {lay.xstride} floats per pixel in this layout (xpu.accumulator), this one {xs}")
    tw, th = tile_extent(tile_size)
    return abi.TileMap(width=W, height=H, xstride=xs, m2_offset=lay.m2_offset, samples_offset=lay.samples_offset, tile_width=tw, tile_height=th,
                       on_device=0, tau=float(threshold), floor=float(floor))


def tile_extent(tile_size):
    """tile_size, an int or (tile_width, tile_height) -> (tile_width, tile_height)"""
    return (int(tile_size),) * 2 if np.isscalar(tile_size) else tuple(int(v) for v in tile_size)


def tile_counts(width, height, tile_width, tile_height):
    """the tiles a row and a column of the grid over a width x height film hold"""
    return -(-width // tile_width), -(-height // tile_height)


def tile_list(records, keep=slice(None)):
    """TILE_RECORD entries (those of the mask or slice `keep`) -> list of (x, y, w, h), in the records' order: what Tiles.from_list takes"""
    return [tuple(t) for t in np.stack([records[f] for f in ("x", "y", "w", "h")], 1)[keep].tolist()]


def open_tiles(records, coverage=1.0):
    """The tiles of a tile map's records a progressive frame still renders -> list of (x, y, w, h), in the records' order.  coverage == 1: the
    open tiles as phx_tile_map defines them; coverage < 1 closes a tile once converged >= coverage * (w * h - invalid) and starved == 0."""
    converged, starved = records["converged"].astype(np.int64), records["starved"]
    valid = records["w"].astype(np.int64) * records["h"] - records["invalid"]
    if coverage >= 1.0:
        is_open = (converged < valid) | (starved > 0)
    else:
        is_open = ~((converged >= float(coverage) * valid) & (starved == 0))
    return tile_list(records, is_open)


def tile_map_grid(width, height, tile_size):
    """The tile map's grid without a film: TILE_RECORD entries with only x, y, w, h set, in the records' order (phx_tile_map states it)"""
    tw, th = tile_extent(tile_size)
    tx, ty = tile_counts(width, height, tw, th)
    out = np.zeros(tx * ty, TILE_RECORD)
    x, y = np.tile(np.arange(tx) * tw, ty), np.repeat(np.arange(ty) * th, tx)  # rows top to bottom, tiles left to right
    out["x"], out["y"], out["w"], out["h"] = x, y, np.minimum(tw, width - x), np.minimum(th, height - y)
    return out


def pack_camera(camera):
    """abi.Camera of a CameraDesc, field by field as SceneDesc.pack fills the scene's"""
    c = abi.Camera()
    c.to_world[:] = [float(x) for x in camera.to_world.reshape(-1)]
    c.fov, c.focal_distance, c.aperture_radius = camera.fov, camera.focal_distance, camera.aperture_radius
    c.film_width, c.film_height = camera.width, camera.height
    return c


def reproject_settings(shape_a, shape_gf, shape_gt, camera_from, camera_to, sigma_plane=1.0, sigma_dist=4.0, max_history=64, primary_components=4):
    """abi.Reproject for an accumulator film of shape_a (H, W, xstride) WITH normals, laid out as xpu.accumulator(W, H, primary_components,
    True) lays it out, and two guide films (H, W, >= 8) of one stride.  ValueError for films of different sizes, an accumulator without
    normals or guide films of different strides."""
    if len(shape_a) != 3 or len(shape_gf) != 3 or len(shape_gt) != 3:
        raise ValueError("reproject: the films must be (height, width, xstride)")
    H, W, xa = (int(v) for v in shape_a)
    if tuple(shape_gf[:2]) != (H, W) or tuple(shape_gt[:2]) != (H, W):
        raise ValueError(f"reproject: the accumulator is {W} x {H} pixels, the guide films {shape_gf[1]} x {shape_gf[0]} and {shape_gt[1]} x {shape_gt[0]}")
    if int(shape_gf[2]) != int(shape_gt[2]):
        raise ValueError(f"reproject: the two guide films must have one stride, not {shape_gf[2]} and {shape_gt[2]}")
    normals_offset, m2_offset, samples_offset, want = film_layout(primary_components, True, True, True)
    if xa != want:
        raise ValueError(f"reproject: an accumulator with normals has {want} floats per pixel in this layout "
                         f"(xpu.accumulator(..., normals=True): the plane test reads them), this one {xa}")
    q = abi.Reproject(width=W, height=H, xstride_a=xa, normals_offset_a=normals_offset, m2_offset_a=m2_offset, samples_offset_a=samples_offset,
                      xstride_g=int(shape_gf[2]), on_device=0, to=pack_camera(camera_to), sigma_plane=float(sigma_plane), sigma_dist=float(sigma_dist),
                      max_history=int(max_history))
    setattr(q, "from", pack_camera(camera_from))
    return q


def outlier_clamp_settings(shape_a, shape_b, radius=2, gamma=4.0, floor=0.0, trim=2, min_taps=4, exclude_centre=True, upper_only=True, clamped_history=0,
                           primary_components=4, normals=False, moments=True, samples=False, m2_offset=None, samples_offset=None):
    """abi.OutlierClamp for a film of shape_a and a reference film of shape_b (H, W, xstride each) in host memory.  The film's "m2" and
    "samples" are where Film puts them for primary_components, normals, moments and samples ("samples" behind "m2", so an accumulator is
    moments=True, samples=True), unless m2_offset / samples_offset say otherwise (0: none).  ValueError for films of different sizes or a
    film narrower than the derived layout."""
    if len(shape_a) != 3 or len(shape_b) != 3:
        raise ValueError("clamp_outliers: both films must be (height, width, xstride)")
    (H, W, xa), (Hb, Wb, xb) = ((int(v) for v in s) for s in (shape_a, shape_b))
    if (H, W) != (Hb, Wb):
        raise ValueError(f"clamp_outliers: the film is {W} x {H} pixels, the reference film {Wb} x {Hb}")
    derived = film_layout(primary_components, normals, moments, samples)
    behind = film_layout(primary_components, normals).xstride  # "primary" and "normals": what the film holds at least
    m2_offset = derived.m2_offset if m2_offset is None else m2_offset
    samples_offset = derived.samples_offset if samples_offset is None else samples_offset
    if max(behind, m2_offset + 3 if m2_offset else 0, samples_offset + 1 if samples_offset else 0) > xa:
        raise ValueError(f"clamp_outliers: this layout needs {max(behind, m2_offset + 3, samples_offset + 1)} floats per pixel, the film has {xa}")
    return abi.OutlierClamp(width=W, height=H, xstride_a=xa, m2_offset_a=int(m2_offset), samples_offset_a=int(samples_offset), xstride_b=xb, on_device=0,
                            flags=(abi.OUTLIER_EXCLUDE_CENTRE if exclude_centre else 0) | (abi.OUTLIER_UPPER_ONLY if upper_only else 0),
                            radius=int(radius), trim=int(trim), min_taps=int(min_taps), gamma=float(gamma), floor=float(floor),
                            clamped_history=int(clamped_history))


TONES = {"clamp": abi.TONE_CLAMP, "reinhard": abi.TONE_REINHARD, "aces": abi.TONE_ACES}


def display_settings(shape, exposure=1.0, tone="aces", white=4.0, dither=True, key=0.18, percentiles=(0.5, 0.95), scale_range=(2.0 ** -12, 2.0 ** 12),
                     fallback=1.0):
    """abi.Display for a film of `shape` (H, W, xstride) in host memory and a tightly packed host image (HipDevice.display sets on_device and
    image_pitch).  exposure: the multiplier, or "auto", which reads key, percentiles (fractions, held in units of 1 / 65536), scale_range
    and `fallback`, the multiplier of a film without a lit pixel.  ValueError for a shape that is no film or an unknown tone."""
    if len(shape) != 3:
        raise ValueError("display: the film must be (height, width, xstride)")
    H, W, xstride = (int(v) for v in shape)
    if tone not in TONES:
        raise ValueError(f"display: tone must be one of {sorted(TONES)}, not {tone!r}")
    auto = isinstance(exposure, str)
    if auto and exposure != "auto":
        raise ValueError(f'display: exposure must be a number or "auto", not {exposure!r}')
    lo, hi = (int(round(float(v) * 65536.0)) for v in percentiles)
    return abi.Display(width=W, height=H, xstride=xstride, image_pitch=0, on_device=0,
                       flags=(abi.DISPLAY_DITHER if dither else 0) | (abi.DISPLAY_AUTO_EXPOSURE if auto else 0), tone=TONES[tone],
                       scale=float(fallback if auto else exposure), white=float(white), key=float(key), low_q16=lo, high_q16=hi,
                       min_scale=float(scale_range[0]), max_scale=float(scale_range[1]))
