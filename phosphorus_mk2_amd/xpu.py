"""Host-side mirror of the reference's device interface over the C ABI (include/phx_xpu.h).

    reference (C++)                                   here
    -----------------------------------------------   -------------------------------------------
    xpu_t::discover(options)      src/xpu.cpp:7-9     HipDevice.discover(options)
    T::make(options)              src/xpu/cpu.hpp:35  HipDevice.make(options)
    xpu_t::preprocess(scene)      src/xpu.hpp:20      HipDevice.preprocess(scene)
    xpu_t::start(scene, frame)    src/xpu.hpp:26      HipDevice.start(scene, frame)   (non-blocking)
    xpu_t::join()                 src/xpu.hpp:32      HipDevice.join()
    frame_state_t{sampler,tiles,film} state.hpp:18    FrameState(sampler_seed, tiles, film)
    job::tiles_t::make/next       jobs/tiles.hpp      Tiles.make(...) / Tiles.next()
    film_t<>::add_tile            film.hpp:12-15      Film.add_tile(...)

The compute path is libphx_hip.so (hand-written HIP for gfx950).  There is no CPU fallback: if the
library is missing or no MI355X is visible, construction raises.

The mirror itself is device.py (the binding) over film.py (what is known of a film without a library); this module re-exports both and holds
what a host does WITH a device: the frame of session_t::render and the loops over frames, cameras and scenes.
"""
import numpy as np

from . import abi  # noqa: F401  (xpu.abi is part of this module's surface, as the names below are)
from .device import LIB_PATH, CallbackTiles, DeviceError, FrameState, HipDevice, Options, Tiles, load_library  # noqa: F401
from .film import (TILE_RECORD, TONES, BottomUpFilm, Film, accumulate_settings, accumulator, denoise_settings, display_settings,  # noqa: F401
                   film_layout, film_variance, guide_plane_scale, open_tiles, outlier_clamp_settings, pack_camera, reproject_settings,
                   tile_list, tile_map_grid, tile_map_settings)


# ---- the steps the loops below share ------------------------------------------------------------------------------------------------------
def _one_device(spp, pps, depth, **options):
    """the device of a loop, to be used as `with _one_device(...) as dev:`: it is closed however the loop ends"""
    return HipDevice.make(Options(samples_per_pixel=spp, paths_per_sample=pps, path_depth=depth, **options))


def _frame(dev, scene_desc, seed, film, tiles, native_sink=True):
    """one frame of the preprocessed scene into `film`, from start to join"""
    dev.start(scene_desc, FrameState(seed, tiles, film, native_sink=native_sink))
    dev.join()


def _denoise_plan(denoise):
    """A loop's denoise= -> (the settings of HipDevice.denoise with those of the entry `guides` merged in, whether there is that entry, its
    `samples` for HipDevice.render_guides); (None, False, None) without denoise.  When the guide film is rendered is the caller's business."""
    if denoise is None:
        return None, False, None
    settings = dict(denoise)
    gset = settings.pop("guides", None)
    if gset is None:
        return settings, False, None
    gset = dict(gset)
    samples = gset.pop("samples", 4)
    settings.update(gset)
    return settings, True, samples


def _shown(dev, display, out, *rest):
    """what a loop yields: (out, *rest), and with display= the image of `out` behind them"""
    return (out, *rest) if display is None else (out, *rest, dev.display(out, **display))


def display(film, **settings):
    """HipDevice.display on a device made for the call (no scene is needed) and closed behind it: film (H, W, xstride) f32 -> (H, W, 4) uint8,
    or (image, summary) with summary=True."""
    with _one_device(1, 1, 1) as dev:
        return dev.display(film, **settings)


def render_progressive(scene_desc, spp, frames, seed=1, stop=None, denoise=None, adaptive=None, pps=1, depth=9, normals=False, tile_size=32,
                       display=None, despeckle=None, tiles=None, **options):
    """Progressive rendering on ONE device: the scene is preprocessed once, then frame k = 0, 1, ... is rendered at `spp` samples
    with sampler seed (seed + k) mod 2^64 and moments=True and pooled into an accumulator film (HipDevice.accumulate).  A generator: after
    every frame it yields (film, summary, frames_done); film is the accumulator (H, W, xstride) f32 in xpu.accumulator's layout, a view that
    the next frame changes: copy it to keep it.  It ends after `frames`, or, with stop=dict(threshold=, floor=0.0, coverage=0.95), once
    pixels - invalid > 0 and converged >= coverage * (pixels - invalid) of the summary (HipDevice.accumulate states the criterion); summary is
    None without stop.
    denoise: a dict of HipDevice.denoise's settings; the yielded film then is a denoised COPY, the accumulator itself is never filtered.
    Its entry guides=dict(samples=4, ...) renders the guide film once, with the first frame's seed.  adaptive: a dict of
    HipDevice.set_adaptive's arguments for every frame.  display: a dict of HipDevice.display's settings ({} for the defaults); the generator
    then yields (film, summary, frames_done, image), the image (or (image, summary) under summary=True) of the film it yields: with denoise,
    of the denoised copy.  despeckle: a dict of HipDevice.clamp_outliers' settings (radius=, gamma=, floor=, trim=, min_taps=;
    {} for the defaults): every frame film is then clamped in place against its own neighbourhoods, the centre excluded and upper only,
    before it is pooled (biased: the fireflies' energy is gone).
    tiles: dict(size=32, coverage=1.0, min_frames=1) stops converged TILES; it needs stop.  Frames 0 .. min_frames - 1 render
    every tile; before each later frame HipDevice.tile_map reads the accumulator with stop's threshold and floor, and the frame renders only
    the tiles that are open (coverage < 1 closes a tile once converged >= coverage * (w * h - invalid) and starved == 0: open_tiles).  The
    loop then also ends once no tile is open.  A closed tile is never looked at again, and neighbouring tiles end with different "samples".
    The frame films carry "samples", so that an unrendered pixel holds n_b == 0 and accumulate leaves it alone: without adaptive= the device
    is set to set_adaptive(0, 0, max(spp, 2), 1), one round that ends at spp and takes no decision.  summary gains tiles, tiles_open (of
    the frame just rendered) and rendered_pixels (the frame's).  tiles= with despeckle= raises ValueError: the clamp's window would read the
    black pixels of unrendered neighbouring tiles as taps.
    options: further Options fields (samples_in_flight=, light_sampling=, ...)."""
    if frames < 1:
        raise ValueError("render_progressive: frames must be at least 1")
    stop = dict(stop) if stop is not None else None
    coverage = float(stop.pop("coverage", 0.95)) if stop is not None else None
    if stop is not None and "threshold" not in stop:
        raise ValueError("render_progressive: stop needs a threshold")
    if tiles is not None:
        if stop is None:
            raise ValueError("render_progressive: tiles= needs stop: the tile map reads its threshold and floor")
        if despeckle is not None:
            raise ValueError("render_progressive: despeckle= cannot be combined with tiles=: the clamp would read unrendered neighbouring tiles as taps")
        tiles = dict(tiles)
        map_size, tile_coverage, min_frames = int(tiles.pop("size", 32)), float(tiles.pop("coverage", 1.0)), int(tiles.pop("min_frames", 1))
        if tiles:
            raise ValueError(f"render_progressive: tiles= does not know {sorted(tiles)}")
        if min_frames < 1:
            raise ValueError("render_progressive: tiles' min_frames must be at least 1")
    by_tiles = tiles is not None
    with_samples = adaptive is not None or by_tiles  # the frame films carry "samples"; the accumulator always does
    pixel = dict(primary_components=4, normals=normals)  # of both: "m2" is always there
    with _one_device(spp, pps, depth, **options) as dev:
        if adaptive is not None:
            dev.set_adaptive(**adaptive)
        elif by_tiles:  # only marks samples = spp: one round that ends at spp, no decision is ever taken
            dev.set_adaptive(threshold=0.0, floor=0.0, min_samples=max(spp, 2), step=1)
        dev.preprocess(scene_desc)
        W, H = scene_desc.camera.width, scene_desc.camera.height
        acc = accumulator(W, H, **pixel)
        settings, guided, guide_samples = _denoise_plan(denoise)
        guides = dev.render_guides(seed, min(int(guide_samples), spp)) if guided else None  # once, before the frames
        for k in range(frames):
            film = Film(W, H, moments=True, adaptive=with_samples, **pixel)
            if not by_tiles:
                queue = Tiles.make(W, H, tile_size)
            else:
                if k < min_frames:
                    records = tile_map_grid(W, H, map_size)
                    frame_tiles = tile_list(records)
                else:
                    records, _ = dev.tile_map(acc, map_size, stop["threshold"], stop.get("floor", 0.0), summary=False, **pixel)
                    frame_tiles = open_tiles(records, tile_coverage)
                    if not frame_tiles:
                        return
                queue = Tiles.from_list(frame_tiles, W, H)
            _frame(dev, scene_desc, (seed + k) % (1 << 64), film, queue)
            if despeckle is not None:  # (never by tiles, so with_samples says whether adaptive= is on)
                dev.clamp_outliers(film.data, **{**despeckle, "exclude_centre": True, "upper_only": True, "moments": True, "samples": with_samples,
                                                 "summary": False, **pixel})
            _, summary = dev.accumulate(acc, film.data, spp, frame_adaptive=with_samples, **pixel, **(stop or {}))
            if by_tiles:
                summary.update(tiles=len(records), tiles_open=len(frame_tiles), rendered_pixels=sum(t[2] * t[3] for t in frame_tiles))
            out = acc if settings is None else dev.denoise(acc, spp, adaptive=True, guides=guides, **pixel, **settings)
            yield _shown(dev, display, out, summary, k + 1)
            valid = summary["pixels"] - summary["invalid"] if summary is not None else 0
            if valid > 0 and summary["converged"] >= coverage * valid:  # (a film without one valid pixel, as any film of 1 spp, has not converged)
                return


def render_camera_path(scene_desc, cameras, spp, frames_per_camera=1, seed=1, guide_samples=4, reproject=None, denoise=None, display=None,
                       pps=1, depth=9, tile_size=32, history_clamp=None, **options):
    """A camera path through a static scene on ONE device: the scene is preprocessed once; then, per camera of `cameras`
    (CameraDescs of the scene's film size): set_camera; the guide film (guide_samples samples, the seed of the camera's first frame); from
    the second camera on the accumulator is carried over by HipDevice.reproject (`reproject`: a dict of its settings, sigma_plane=,
    sigma_dist=, max_history=); then frames_per_camera frames of `spp` samples with seeds (seed + k) mod 2^64, k counting frames over the
    whole path, each pooled by HipDevice.accumulate.  A generator: after every frame it yields (film, summary, frames_done, reprojection),
    as render_progressive yields (summary is None: there is no stop) plus the summary of the reprojection that led to this camera (None at
    the first); with display, (..., reprojection, image).  film is the accumulator (H, W, 11) f32 in xpu.accumulator's layout with
    normals, replaced at every camera: copy it to keep it.  denoise, display, options: as for render_progressive; the guided denoiser
    reads this camera's guide film (no entry `guides` is needed: guides=dict(...) carries its settings).  history_clamp: a dict of
    HipDevice.clamp_outliers' settings (radius=, gamma=, floor=, trim=, min_taps=, clamped_history=; {} for the defaults): from the second
    camera on the reprojected accumulator is clamped, two-sided and with the centre included, against the neighbourhoods of that camera's
    first frame film before that frame is pooled."""
    if frames_per_camera < 1:
        raise ValueError("render_camera_path: frames_per_camera must be at least 1")
    pixel = dict(primary_components=4, normals=True)  # of the accumulator and of the frame films, which carry "m2" and no "samples"
    with _one_device(spp, pps, depth, **options) as dev:
        dev.preprocess(scene_desc)
        W, H = scene_desc.camera.width, scene_desc.camera.height
        acc = accumulator(W, H, **pixel)
        settings, guided, _ = _denoise_plan(denoise)  # (the entry's `samples` is not read: the guide film is each camera's, of guide_samples)
        k, previous, guides_before = 0, None, None
        for camera in cameras:
            dev.set_camera(camera)
            guides = dev.render_guides((seed + k) % (1 << 64), min(int(guide_samples), spp))  # once per camera
            moved = None
            if previous is not None:
                acc, moved = dev.reproject(acc, guides_before, guides, previous, camera, **(reproject or {}))
            for first in [True] + [False] * (frames_per_camera - 1):
                film = Film(W, H, moments=True, adaptive=False, **pixel)
                _frame(dev, scene_desc, (seed + k) % (1 << 64), film, Tiles.make(W, H, tile_size))
                k += 1
                if history_clamp is not None and previous is not None and first:
                    dev.clamp_outliers(acc, film.data, **{**history_clamp, "exclude_centre": False, "upper_only": False, "moments": True, "samples": True,
                                                          "summary": False, **pixel})
                dev.accumulate(acc, film.data, spp, frame_adaptive=False, **pixel)
                if settings is None:
                    out = acc
                else:
                    out = dev.denoise(acc, spp, adaptive=True, guides=guides if guided else None, **pixel,
                                      **({"plane_scale": guide_plane_scale(camera), **settings} if guided else settings))
                yield _shown(dev, display, out, None, k, moved)
            previous, guides_before = camera, guides


def render_animation(scene_descs, spp, mode="refit", rebuild_every=0, denoise=None, display=None, seed=1, pps=1, depth=9, tile_size=32, **options):
    """Moving geometry on ONE device: the first scene of `scene_descs` is preprocessed, every later one — the same scene
    with moved vertices — is taken by HipDevice.update_geometry(mode); with rebuild_every = k > 0 every k-th update is a "rebuild"
    whatever `mode` says.  One FRESH film of `spp` samples is rendered per scene, with sampler seed `seed`: nothing is accumulated or
    reprojected across geometry (a film of the old geometry says nothing about the new one).  A generator: per scene it yields (film,
    summary, index) — film (H, W, 10) f32 with normals and moments, summary the update's dict (None for the first scene) — and with
    display (..., image).  denoise, display: dicts of HipDevice.denoise's and HipDevice.display's settings; options: xpu.Options'."""
    pixel = dict(primary_components=4, normals=True, adaptive=False)  # of every film, which carries "m2"
    with _one_device(spp, pps, depth, **options) as dev:
        for index, scene_desc in enumerate(scene_descs):
            summary = None
            if index == 0:
                dev.preprocess(scene_desc)
            else:
                summary = dev.update_geometry(scene_desc, "rebuild" if rebuild_every > 0 and index % rebuild_every == 0 else mode)
            W, H = scene_desc.camera.width, scene_desc.camera.height
            film = Film(W, H, moments=True, **pixel)
            _frame(dev, scene_desc, seed, film, Tiles.make(W, H, tile_size))
            out = film.data if denoise is None else dev.denoise(film.data, spp, **pixel, **denoise)
            yield _shown(dev, display, out, summary, index)


def render_on(devices, scene_desc, seed=1, normals=False, tile_size=32, native_sink=True, rank=0, world=1, moments=False, adaptive=False):
    """The reference's frame on SEVERAL devices in one process (src/core.cpp:103-115): every device is started on the SAME tile
    queue and the SAME film and joined in turn; no collective.  `devices` must have been preprocessed with `scene_desc`.
    adaptive=True only sizes the film for the channel "samples": the caller has set every device (HipDevice.set_adaptive).
    Returns (film array, [stats per device])."""
    W, H = scene_desc.camera.width, scene_desc.camera.height
    tiles = Tiles.make(W, H, tile_size, rank, world)
    film = Film(W, H, primary_components=4, normals=normals, moments=moments, adaptive=bool(adaptive))
    for d in devices:
        d.start(scene_desc, FrameState(seed, tiles, film, native_sink=native_sink))
    for d in devices:
        d.join()
    return film.data, [d.stats() for d in devices]


def render(scene_desc, spp=16, pps=1, depth=9, seed=1, normals=False, tile_size=32, rank=0, world=1, callback_tiles=False,
           samples_in_flight=0, tiles_per_batch=0, native_sink=False, bvh_builder="auto", light_sampling="reference",
           light_selection="uniform", environment_sampling=False, moments=False, adaptive=None, denoise=None, progressive=None):
    """Convenience: the call sequence of session_t::render (plugins/blender/session.cpp:73-94):
    make -> preprocess -> tiles_t::make -> start -> join on ONE device.  Returns (film array HxWxC, stats).
    adaptive: a dict of HipDevice.set_adaptive's arguments (threshold=..., floor=, min_samples=, step=) turns adaptive sampling on; the film then
    needs moments=True and carries the channel "samples".
    denoise: a dict of HipDevice.denoise's settings (iterations=, sigma_l=, normal_power_log2=; {} for the defaults) filters the film that is
    returned; it needs moments=True.  Its entry guides=dict(samples=4, demodulate=True, plane=False, albedo_floor=, sigma_x=) renders the
    first-hit guide film with the frame's seed (HipDevice.render_guides) and runs the guided filter; plane=True needs normals=True.
    progressive: dict(frames=, stop=None, tiles=None) drains render_progressive (frames of spp samples at seeds seed, seed + 1, ... pooled into
    one film, until `frames` are done or stop's coverage is met) and returns (the last film it yields, in xpu.accumulator's layout, the last
    summary or None); it needs moments=True and renders the whole film on one device."""
    if denoise is not None and not moments:
        raise ValueError("denoise needs moments=True: the filter's yardstick is the film's m2 channel")
    if progressive is not None:
        if not moments:
            raise ValueError("progressive needs moments=True: frames are pooled by their m2 channel")
        if callback_tiles or (rank, world) != (0, 1):
            raise ValueError("progressive renders whole films on one device: no callback_tiles, rank or world")
        last = None
        for last in render_progressive(scene_desc, spp, int(progressive["frames"]), seed, progressive.get("stop"), denoise, adaptive, pps, depth, normals,
                                       tile_size, tiles=progressive.get("tiles"), samples_in_flight=samples_in_flight, tiles_per_batch=tiles_per_batch, bvh_builder=bvh_builder,
                                       light_sampling=light_sampling, light_selection=light_selection, environment_sampling=environment_sampling):
            pass
        return np.array(last[0]), last[1]
    opts = Options(samples_per_pixel=spp, paths_per_sample=pps, path_depth=depth, samples_in_flight=samples_in_flight,
                   tiles_per_batch=tiles_per_batch, bvh_builder=bvh_builder, light_sampling=light_sampling, light_selection=light_selection,
                   environment_sampling=environment_sampling)
    # ONE device, on the caller's current GPU (device_ordinal -1): discover() is for hosts that drive every GPU (render_on) and
    # would build a context, a stream and the kernel attributes on each of them only to use the first
    pixel = dict(primary_components=4, normals=normals, adaptive=adaptive is not None)
    with HipDevice.make(opts) as dev:
        if adaptive is not None:
            dev.set_adaptive(**adaptive)
        dev.preprocess(scene_desc)
        W, H = scene_desc.camera.width, scene_desc.camera.height
        tiles = Tiles.make(W, H, tile_size, rank, world)
        if callback_tiles:
            tiles = CallbackTiles(iter(tiles.next, None))  # the native queue, drained into a Python one
        film = Film(W, H, moments=moments, **pixel)
        _frame(dev, scene_desc, seed, film, tiles, native_sink)
        settings, guided, guide_samples = _denoise_plan(denoise)
        if settings is None:
            return film.data, dev.stats()
        guides = dev.render_guides(seed, min(int(guide_samples), spp)) if guided else None  # behind the frame
        return dev.denoise(film.data, spp, guides=guides, **pixel, **settings), dev.stats()
