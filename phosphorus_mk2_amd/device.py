"""The binding of the C ABI (include/phx_xpu.h): the loader of libphx_hip.so, Options, the tile queues, FrameState and HipDevice,
one method per entry point.  xpu.py's docstring holds the table of what mirrors what of the reference.  The structs a film pass takes
are made by film.py; here they meet the caller's host arrays or device addresses and the library."""
import ctypes as C
import os
import threading

import numpy as np

from . import abi
from .film import (TILE_RECORD, accumulate_settings, denoise_settings, display_settings, guide_plane_scale, outlier_clamp_settings, pack_camera,
                   reproject_settings, tile_counts, tile_map_settings)

_HERE = os.path.dirname(os.path.abspath(__file__))
# PHX_LIB selects another build of the same library (A/B experiments: scripts/ab.sh builds variants with extra -D flags)
LIB_PATH = os.environ.get("PHX_LIB") or os.path.join(_HERE, "libphx_hip.so")
_lib = None


class DeviceError(RuntimeError):
    pass


def load_library():
    """Load the in-tree HIP extension.  Raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DeviceError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback path")
        _lib = abi.declare(C.CDLL(LIB_PATH))
        _lib.phx_abi_sizeof.argtypes = [C.c_int]
        _lib.phx_abi_sizeof.restype = C.c_uint32
    return _lib


def _check(lib, rc, what):
    if rc != abi.PHX_OK:
        raise DeviceError(f"{what} failed ({rc}): {lib.phx_last_error().decode()}")


class Options:
    """parsed_options_t (src/options.hpp:6-43) plus the device knobs."""

    def __init__(self, samples_per_pixel=16, paths_per_sample=16, path_depth=9, single_threaded=False, host_only=False,
                 render_normals=False, verbose=False, device_ordinal=-1, samples_in_flight=0, tiles_per_batch=0, bvh_builder="auto",
                 light_sampling="reference", light_selection="uniform", environment_sampling=False):
        self.samples_per_pixel = samples_per_pixel
        self.paths_per_sample = paths_per_sample
        self.path_depth = path_depth
        self.single_threaded = single_threaded
        self.host_only = host_only
        self.render_normals = render_normals
        self.verbose = verbose
        self.device_ordinal = device_ordinal
        self.samples_in_flight = samples_in_flight
        self.tiles_per_batch = tiles_per_batch
        self.bvh_builder = bvh_builder  # "host": binned SAH on the host cores; "device": LBVH built on the GPU; "auto": by scene size
        # "reference": next-event estimation picks a light's triangle by index, as the reference does (biased for lights of unequal triangles);
        # "area": by the light's area CDF (unbiased; the scene is shaded by k_shade_g).  An int is passed through as it is.
        self.light_sampling = light_sampling
        # "uniform": next-event estimation chooses among the lights uniformly; "power": by area x luminance of the emission (bit 8 of the packed
        # word, abi.LIGHT_SELECT_BY_POWER), which needs light_sampling "area"
        self.light_selection = light_selection
        # True: next-event estimation samples the environment image too (bit 9, abi.LIGHT_INCLUDE_ENVIRONMENT), which needs light_selection
        # "power" and an environment material with an image
        self.environment_sampling = environment_sampling

    def pack(self):
        o = abi.Options()
        o.samples_per_pixel, o.paths_per_sample, o.path_depth = self.samples_per_pixel, self.paths_per_sample, self.path_depth
        o.single_threaded, o.host_only = int(self.single_threaded), int(self.host_only)
        o.render_normals, o.verbose = int(self.render_normals), int(self.verbose)
        o.device_ordinal, o.samples_in_flight, o.tiles_per_batch = self.device_ordinal, self.samples_in_flight, self.tiles_per_batch
        o.bvh_builder = {"auto": abi.BVH_AUTO, "host": abi.BVH_HOST_SAH, "device": abi.BVH_DEVICE_LBVH}[self.bvh_builder]
        ls = self.light_sampling
        o.light_sampling = ls if isinstance(ls, int) else {"reference": abi.LIGHTS_REFERENCE, "area": abi.LIGHTS_BY_AREA}[ls]
        if {"uniform": False, "power": True}[self.light_selection]:
            if o.light_sampling != abi.LIGHTS_BY_AREA:
                raise ValueError('light_selection="power" needs light_sampling="area"')
            o.light_sampling |= abi.LIGHT_SELECT_BY_POWER
        if self.environment_sampling:
            if not o.light_sampling & abi.LIGHT_SELECT_BY_POWER:
                raise ValueError('environment_sampling=True needs light_selection="power"')
            o.light_sampling |= abi.LIGHT_INCLUDE_ENVIRONMENT
        return o


class Tiles:
    """job::tiles_t: precomputed tile_size x tile_size tiles behind an atomic cursor; `rank`/`world`
    keep only the tiles of one GPU (tile (tx, ty) -> rank (tx + s*ty) % world, see dist.tile_shift) for the multi-GPU shard."""

    def __init__(self, handle, lib, width, height):
        self._h, self._lib, self.width, self.height = handle, lib, width, height

    @staticmethod
    def make(width, height, tile_size=32, rank=0, world=1):
        lib = load_library()
        h = lib.phx_tiles_make(width, height, tile_size, rank, world)
        if not h:
            raise DeviceError(lib.phx_last_error().decode())
        return Tiles(h, lib, width, height)

    @staticmethod
    def from_list(tiles, width, height):
        """A native queue of the caller's own tiles (x, y, w, h) in the caller's order (phx_tiles_make_list): the open tiles of a tile map,
        say.  The list is copied; an empty one gives a queue that is drained at once.  width, height: the film's, as make() keeps them."""
        lib = load_library()
        arr = np.ascontiguousarray(np.asarray(list(tiles), np.int64).reshape(-1, 4).astype(np.uint32))  # x, y, w, h: a phx_tile each
        h = lib.phx_tiles_make_list(arr.ctypes.data_as(C.POINTER(abi.Tile)), len(arr))
        if not h:
            raise DeviceError(lib.phx_last_error().decode())
        return Tiles(h, lib, width, height)

    def next(self):
        t = abi.Tile()
        if self._lib.phx_tiles_next(self._h, C.byref(t)):
            return (t.x, t.y, t.w, t.h)
        return None

    def reset(self):
        self._lib.phx_tiles_reset(self._h)

    def __len__(self):
        return self._lib.phx_tiles_count(self._h)

    def __del__(self):
        try:
            if self._h:
                self._lib.phx_tiles_free(self._h)
                self._h = None
        except Exception:
            pass


class CallbackTiles:
    """A tile queue implemented in Python (any object with next() -> (x,y,w,h) | None): exercises the
    phx_next_tile_fn callback path exactly like a foreign host's own job::tiles_t would."""

    def __init__(self, tiles):
        self._tiles = list(tiles)
        self._i = 0
        self._lock = threading.Lock()

    def next(self):
        with self._lock:
            if self._i < len(self._tiles):
                self._i += 1
                return self._tiles[self._i - 1]
        return None


def _f32p(a):
    return a.ctypes.data_as(abi.f32p)


def _u32p(a):
    return a.ctypes.data_as(abi.u32p)


def _film_shape(film, on_device):  # a device-resident film is given by its shape, or by an array of it
    return tuple(film) if on_device and not hasattr(film, "shape") else film.shape


def _writable_f32(a):  # an array a film call can work on in place
    return isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable


def _in_place(a):  # the array a film call changes and returns: a itself where that can be, else a copy
    return a if _writable_f32(a) else np.array(a, np.float32, order="C")


def _read_only(film, device_ptr):
    """a film a call only reads -> (its address, what keeps that address alive until the call is over): the device address, or the host
    array as C-contiguous float32"""
    if device_ptr is not None:
        return int(device_ptr), None
    keep = np.ascontiguousarray(film, np.float32)
    return keep.ctypes.data, keep


def _summary(struct, wanted=True):  # -> (the summary struct a call fills, its reference), or (None, None)
    s = struct() if wanted else None
    return s, (C.byref(s) if wanted else None)


def _summary_dict(s):  # a summary struct of counts, or None
    return None if s is None else {k: int(getattr(s, k)) for k, _ in s._fields_}


class FrameState:
    """frame_state_t (src/state.hpp:18-31).  `sampler_seed` replaces the shared sampler_t."""

    def __init__(self, sampler_seed, tiles, film, device_film_ptr=None, native_sink=False, primary_components=4, normals=False, moments=False,
                 adaptive=False):
        self.sampler_seed, self.tiles, self.film, self.device_film_ptr = sampler_seed, tiles, film, device_film_ptr
        self.native_sink = native_sink  # fill film.data from C (phx_frame.host_film) instead of one Python add_tile call per tile
        # the pixel layout of device_film_ptr when there is no `film` to take it from (a film's own layout wins)
        self.primary_components, self.normals, self.moments = primary_components, normals, moments
        # the frame's pixels carry the channel "samples": what the device writes while HipDevice.set_adaptive is on.  It says how the CALLER
        # sized device_film_ptr; the device itself goes by its own setting (phx_frame has no word for it)
        self.adaptive = adaptive


class HipDevice:
    """The gfx950 device behind the xpu_t interface."""

    def __init__(self, handle, lib, options):
        self._h, self._lib, self.options = handle, lib, options
        self._keep = None
        self._scene = None
        self._camera = None  # the camera of the last set_camera behind the last preprocess; None: the scene's own
        self._adaptive = False  # set_adaptive is on: this device's frames carry the channel "samples"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def discover(options):
        """xpu_t::discover (src/xpu.cpp:7-9): one device object per usable gfx950 GPU — all of them are meant to drain the frame's
        one tile queue into its one film (src/core.cpp:103-115, see render_on).  An explicit `options.device_ordinal >= 0` restricts
        the list to that GPU (what one rank of a one-process-per-GPU job wants)."""
        lib = load_library()
        o = options.pack()
        n = C.c_int(0)
        rc = lib.phx_discover(C.byref(o), C.byref(n))
        if options.host_only:
            return []
        _check(lib, rc, "phx_discover")
        if options.device_ordinal >= 0 or n.value == 1:
            return [HipDevice.make(options)]
        devs = []
        for i in range(n.value):
            oi = Options(**{**options.__dict__, "device_ordinal": i})
            devs.append(HipDevice.make(oi))
        return devs

    @staticmethod
    def make(options):
        lib = load_library()
        o = options.pack()
        h = lib.phx_dev_make(C.byref(o))
        if not h:
            raise DeviceError("phx_dev_make: " + lib.phx_last_error().decode())
        return HipDevice(h, lib, options)

    def preprocess(self, scene_desc):
        s, keep = scene_desc.pack()
        _check(self._lib, self._lib.phx_dev_preprocess(self._h, C.byref(s)), "phx_dev_preprocess")
        self._scene, self._camera = scene_desc, None

    def set_camera(self, camera):
        """Replaces the camera of the preprocessed scene and nothing else (phx_dev_set_camera): camera is a CameraDesc of the
        preprocessed scene's film size.  Every later frame and guide film is what a device preprocessed with the scene under this camera
        renders, bit for bit, at none of preprocess's cost.  The scene description is not changed: start() still takes the one that was
        preprocessed."""
        c = pack_camera(camera)
        _check(self._lib, self._lib.phx_dev_set_camera(self._h, C.byref(c)), "phx_dev_set_camera")
        self._camera = camera

    def update_geometry(self, scene_desc, mode="refit"):
        """New vertex positions and normals for the preprocessed scene (phx_dev_update_geometry): scene_desc is the
        preprocessed scene with moved vertices (scenes.transformed, scenes.wobbled, or a SceneDesc of the caller's with the same faces,
        face sets, materials and textures).  mode "refit" keeps the tree's topology and recomputes its boxes; "rebuild" builds a new
        tree.  Either way the next frame is, bit for bit, what a device freshly preprocessed with scene_desc renders, and no material,
        texture or environment table is read or uploaded again.  The camera stays the device's (the last set_camera's, else the
        preprocessed scene's).  start() takes scene_desc from now on; films accumulated before the update are stale.  -> the summary as a
        dict: mode, triangles, nodes, levels, lights, light_triangles, bounds (6 floats), delta."""
        modes = {"refit": abi.UPDATE_REFIT, "rebuild": abi.UPDATE_REBUILD}
        if mode not in modes:
            raise ValueError(f"update_geometry: mode must be one of {sorted(modes)}, not {mode!r}")
        s, keep = scene_desc.pack()
        u, out = abi.GeometryUpdate(mode=modes[mode]), abi.GeometrySummary()
        _check(self._lib, self._lib.phx_dev_update_geometry(self._h, C.byref(s), C.byref(u), C.byref(out)), "phx_dev_update_geometry")
        self._scene = scene_desc
        return {k: (list(getattr(out, k)) if k == "bounds" else getattr(out, k)) for k, _ in out._fields_}

    def update_geometry_times(self):
        """milliseconds of the last update_geometry(), host clock: dict of flatten (the host's pass over the moved scene), upload, device
        (the refit or rebuild and the tables' kernels, to the last synchronise) and call"""
        return self._times("phx_dev_update_geometry_times", 4, ("flatten", "upload", "device", "call"))

    def start(self, scene_desc, frame):
        assert scene_desc is self._scene, "start() must get the scene that was preprocessed"
        f = abi.Frame()
        tiles = frame.tiles
        if isinstance(tiles, Tiles):  # native queue: no Python in the loop
            f.tiles_user = tiles._h
            f.next_tile = C.cast(self._lib.phx_tiles_next, C.c_void_p)
            cb_next = None
        else:
            def _next(user, out):
                t = tiles.next()
                if t is None:
                    return 0
                out[0].x, out[0].y, out[0].w, out[0].h = t
                return 1
            cb_next = abi.NEXT_TILE_FN(_next)
            f.next_tile = C.cast(cb_next, C.c_void_p)
        cb_add = None
        if frame.film is not None:
            film = frame.film

            def _add(user, x, y, w, h, buf, xs, ys):
                film.add_tile(x, y, w, h, buf, xs, ys)
            if frame.native_sink:
                f.host_film = film.data.ctypes.data
            else:
                cb_add = abi.ADD_TILE_FN(_add)
                f.add_tile = C.cast(cb_add, C.c_void_p)
            f.primary_components = film.primary_components
            f.normals_channel = 1 if film.normals else 0
            moments = getattr(film, "moments", False)
        else:
            f.primary_components = frame.primary_components
            f.normals_channel = 1 if frame.normals else 0
            moments = frame.moments
        # the device writes xstride floats per pixel by ITS setting: a sink sized otherwise would be overrun (or left with holes)
        sized_for = bool(getattr(frame.film, "adaptive", False)) if frame.film is not None else bool(frame.adaptive)
        if sized_for != self._adaptive and moments == 1:
            raise ValueError(f"the film is sized {'with' if sized_for else 'without'} the channel \"samples\", but adaptive sampling is "
                             f"{'on' if self._adaptive else 'off'} for this device (HipDevice.set_adaptive; Film(..., adaptive=True))")
        f.moments_channel = int(moments)  # False / True; another int is passed through as it is (and refused by phx_dev_start)
        if frame.device_film_ptr:
            f.device_film = frame.device_film_ptr
        f.sampler_seed = frame.sampler_seed
        self._keep = (f, cb_next, cb_add, frame)
        _check(self._lib, self._lib.phx_dev_start(self._h, C.byref(f)), "phx_dev_start")

    def join(self):
        rc = self._lib.phx_dev_join(self._h)
        self._keep = None
        _check(self._lib, rc, "phx_dev_join")

    def stats(self):
        st = abi.Stats()
        _check(self._lib, self._lib.phx_dev_get_stats(self._h, C.byref(st)), "phx_dev_get_stats")
        out = {}
        for k, _ in st._fields_:
            if k == "reserved":
                continue
            v = getattr(st, k)
            out[k] = list(v) if hasattr(v, "__len__") else v
        return out

    def set_adaptive(self, threshold, floor=0.0, min_samples=16, step=16):
        """Adaptive sampling for every frame this device starts from now on (phx_dev_set_adaptive; include/phx_xpu.h states the rule): a
        pixel stops once the standard error of its extrapolated value is at most threshold * (|value| + floor), tested after min_samples
        samples and then every `step`.  Such a frame needs a film with moments=True, adaptive=True.  set_adaptive(None) turns it off."""
        if threshold is None:
            _check(self._lib, self._lib.phx_dev_set_adaptive(self._h, None), "phx_dev_set_adaptive")
            self._adaptive = False
            return
        a = abi.Adaptive(threshold=threshold, floor=floor, min_samples=min_samples, step=step)
        _check(self._lib, self._lib.phx_dev_set_adaptive(self._h, C.byref(a)), "phx_dev_set_adaptive")
        self._adaptive = True

    def render_guides(self, seed, samples, device_ptr=None):
        """The first-hit guide film of the preprocessed scene (phx_dev_render_guides; include/phx_xpu.h states the rule): per pixel
        albedo rgb, coverage, position xyz, distance over the first `samples` camera samples of a frame with sampler seed `seed` (1 <= samples <=
        the device's samples_per_pixel) -> (H, W, 8) f32.  device_ptr: the address of a device-resident W * H * 8 fp32 film to fill instead;
        the call then returns None."""
        g = abi.Guides(sampler_seed=int(seed), samples=int(samples), on_device=0 if device_ptr is None else 1)
        if device_ptr is not None:
            _check(self._lib, self._lib.phx_dev_render_guides(self._h, C.byref(g), device_ptr), "phx_dev_render_guides")
            return None
        if self._scene is None:
            _check(self._lib, self._lib.phx_dev_render_guides(self._h, C.byref(g), None), "phx_dev_render_guides")  # the device says why: no scene
        H, W = self._scene.camera.height, self._scene.camera.width
        out = np.zeros((H, W, abi.GUIDE_FLOATS), np.float32)
        _check(self._lib, self._lib.phx_dev_render_guides(self._h, C.byref(g), out.ctypes.data), "phx_dev_render_guides")
        return out

    def _times(self, getter, n, keys=None):
        """a phx_dev_*_times getter of n doubles -> dict by keys, or the list"""
        ms = (C.c_double * n)()
        _check(self._lib, getattr(self._lib, getter)(self._h, ms), getter)
        return list(ms) if keys is None else dict(zip(keys, ms))

    def guides_times(self):
        """milliseconds of the last render_guides(): dict of kernel (HIP events) and call (host clock)"""
        return self._times("phx_dev_guides_times", 2, ("kernel", "call"))

    def denoise(self, data, spp, primary_components=4, normals=False, adaptive=False, iterations=5, sigma_l=4.0, normal_power_log2=7, device_ptr=None,
                guides=None, demodulate=True, plane=False, albedo_floor=0.01, sigma_x=1.0, plane_scale=None, guides_ptr=None):
        """The film denoiser (phx_dev_denoise; include/phx_xpu.h states the rule): an edge-avoiding a-trous filter of a finished film
        whose yardstick is the film's own error estimate, so the film must have been rendered with moments=True.  data (H, W, xstride) f32 as
        render() returns it -> a new array of the same shape: "primary" filtered, "m2" the filtered value's variance estimate (read it with
        film_variance as before), every other float untouched.  primary_components, normals and adaptive say how the pixel is laid out, as for
        Film.  device_ptr: the address of a device-resident film of that layout, denoised IN PLACE; `data` then is only its shape (H, W,
        xstride), and the call returns None.  Needs no scene; call it after join(), and after dist.reduce_film on several GPUs.
        guides: a guide film (H, W, >= 8) f32 as render_guides returns it (guides_ptr: its device address, with device_ptr, `guides` then its
        shape) turns the guided filter on (phx_dev_denoise_guided): demodulate divides the first hit's albedo (floored at
        albedo_floor) out before filtering and multiplies it back; plane (needs normals) also rejects taps farther than sigma_x pixels'
        worth of surface from the pixel's tangent plane, plane_scale being the world size of a pixel at unit distance (guide_plane_scale;
        default: that of the last preprocessed scene's camera)."""
        shape = _film_shape(data, device_ptr is not None)
        q = denoise_settings(shape, spp, primary_components, normals, adaptive, iterations, sigma_l, normal_power_log2)
        if guides is None and guides_ptr is None:
            gref = None
        else:
            gshape = _film_shape(guides, guides_ptr is not None)
            if len(gshape) != 3 or tuple(gshape[:2]) != tuple(shape[:2]):
                raise ValueError(f"denoise: the guide film must be (height, width, >= 8) over the film's pixels, not {tuple(gshape)}")
            if plane and plane_scale is None:
                if self._scene is None:
                    raise ValueError("denoise: plane=True needs plane_scale (guide_plane_scale(camera)) on a device without a preprocessed scene")
                plane_scale = guide_plane_scale(self._camera or self._scene.camera)
            gaddr, keep = _read_only(guides, guides_ptr)
            g = abi.DenoiseGuides(guides=gaddr, xstride=int(gshape[2]),
                                  flags=(abi.GUIDE_DEMODULATE if demodulate else 0) | (abi.GUIDE_PLANE if plane else 0),
                                  albedo_floor=float(albedo_floor), sigma_x=float(sigma_x), plane_scale=float(plane_scale if plane_scale is not None else 0.0))
            gref = C.byref(g)
        call = (lambda a, b: self._lib.phx_dev_denoise(self._h, C.byref(q), a, b)) if gref is None else \
               (lambda a, b: self._lib.phx_dev_denoise_guided(self._h, C.byref(q), gref, a, b))
        what = "phx_dev_denoise" if gref is None else "phx_dev_denoise_guided"
        if device_ptr is not None:
            if gref is not None and guides_ptr is None:
                raise ValueError("denoise: a device-resident film needs device-resident guides (guides_ptr)")
            q.on_device = 1
            _check(self._lib, call(device_ptr, device_ptr), what)
            return None
        if guides_ptr is not None:
            raise ValueError("denoise: device-resident guides (guides_ptr) need a device-resident film (device_ptr)")
        src = np.ascontiguousarray(data, np.float32)
        out = np.empty_like(src)
        _check(self._lib, call(src.ctypes.data, out.ctypes.data), what)
        return out

    def denoise_times(self):
        """HIP-event milliseconds of the last denoise(): dict of pack, iterations (list of 8, 0 for those not run), unpack, call (host clock)"""
        ms = self._times("phx_dev_denoise_times", 11)
        return {"pack": ms[0], "iterations": ms[1:9], "unpack": ms[9], "call": ms[10]}

    def accumulate(self, acc, frame_film, spp, primary_components=4, normals=False, frame_adaptive=False, threshold=None, floor=0.0, device_ptrs=None):
        """Film accumulation across frames (phx_dev_film_accumulate; include/phx_xpu.h states the rule): frame_film, a finished film
        of `spp` samples rendered with moments=True (frame_adaptive: under adaptive sampling, so that it carries its own "samples"), is pooled
        into acc, a film in the accumulator's layout (accumulator(): the layout of an adaptive film) -> (acc, summary).  A C-contiguous float32
        acc is pooled in place and returned; anything else is copied first.  summary is None unless threshold is given: then a dict of pixels,
        invalid, converged (valid pixels whose standard error is at most threshold * (|value| + floor)) and samples, counted on the pooled
        film.  The frames must come from different seeds.  device_ptrs: (acc address, frame film address) of device-resident films of these
        layouts; acc and frame_film then are only their shapes (H, W, xstride), and the call returns (None, summary).  Needs no scene; call it
        after join(), and after dist.reduce_film on several GPUs."""
        on_device = device_ptrs is not None
        q = accumulate_settings(_film_shape(acc, on_device), _film_shape(frame_film, on_device), spp, primary_components, normals, frame_adaptive,
                                0.0 if threshold is None else threshold, floor)
        s, sref = _summary(abi.AccumulateSummary, threshold is not None)
        if on_device:
            q.on_device = 1
            pa, pb = (int(p) for p in device_ptrs)
            out = None
        else:
            out = _in_place(acc)
            keep = np.ascontiguousarray(frame_film, np.float32)
            pa, pb = out.ctypes.data, keep.ctypes.data
        _check(self._lib, self._lib.phx_dev_film_accumulate(self._h, C.byref(q), pa, pb, sref), "phx_dev_film_accumulate")
        return out, _summary_dict(s)

    def accumulate_times(self):
        """milliseconds of the last accumulate(): dict of kernel (HIP events) and call (host clock)"""
        return self._times("phx_dev_accumulate_times", 2, ("kernel", "call"))

    def tile_map(self, acc, tile_size=32, threshold=0.0, floor=0.0, primary_components=4, normals=False, device_ptr=None, summary=True):
        """The tile map (phx_dev_film_tile_map; include/phx_xpu.h states the rule): acc, a film in the accumulator's layout
        (accumulator()), is read, and every tile of the tile_size x tile_size grid over it (an int, or (tile_width, tile_height)) gets a record
        -> (records, summary).  records: a numpy structured array (TILE_RECORD: x, y, w, h, invalid, starved, converged, worst, samples), one
        entry per tile, rows top to bottom, tiles left to right: for a square tile the list Tiles.make(W, H, tile_size) serves.  A tile is
        open when converged < w * h - invalid or starved > 0; `converged` counts the valid pixels whose standard error is at most
        threshold * (|value| + floor), as accumulate()'s summary does.  summary: a dict of pixels, invalid, converged, samples, tiles and
        open (None with summary=False).  device_ptr: the address of a device-resident film; acc then is only its shape (H, W, xstride), and
        40 bytes a tile come back instead of the film.  Needs no scene; it changes no film."""
        q = tile_map_settings(_film_shape(acc, device_ptr is not None), tile_size, threshold, floor, primary_components, normals)
        q.on_device = 0 if device_ptr is None else 2
        film, keep = _read_only(acc, device_ptr)
        tx, ty = tile_counts(q.width, q.height, q.tile_width, q.tile_height)
        records = np.zeros(tx * ty, TILE_RECORD)
        s, sref = _summary(abi.TileMapSummary, summary)
        _check(self._lib, self._lib.phx_dev_film_tile_map(self._h, C.byref(q), film, records.ctypes.data, sref), "phx_dev_film_tile_map")
        return records, _summary_dict(s)

    def tile_map_times(self):
        """milliseconds of the last tile_map(): dict of kernel (HIP events) and call (host clock)"""
        return self._times("phx_dev_tile_map_times", 2, ("kernel", "call"))

    def reproject(self, acc, guides_from, guides_to, camera_from, camera_to, sigma_plane=1.0, sigma_dist=4.0, max_history=64, primary_components=4,
                  summary=True, device_ptrs=None):
        """Reprojection (phx_dev_film_reproject; include/phx_xpu.h states the rule): acc, an accumulator film with normals
        (accumulator(..., normals=True)) under camera_from, is carried to camera_to by the two cameras' guide films (render_guides under
        each) -> (film, summary): a new film of acc's layout, in which a pixel whose first hit was seen before holds the bilinear mix of the
        old pixels that are the same surface (to within sigma_plane pixels' worth of surface off the tangent plane and sigma_dist of
        distance), its "samples" capped at max_history, and every other pixel is zero, so that accumulate() starts it afresh.  summary: a
        dict of pixels, reused, no_geometry, disoccluded and samples (None with summary=False).  The defaults are settings, not
        measurements.  device_ptrs: (acc, guides_from, guides_to, out) addresses of device-resident films; acc, guides_from and guides_to
        then are only their shapes, and the call returns (None, summary).  Needs no scene."""
        on_device = device_ptrs is not None
        shapes = [_film_shape(a, on_device) for a in (acc, guides_from, guides_to)]
        q = reproject_settings(shapes[0], shapes[1], shapes[2], camera_from, camera_to, sigma_plane, sigma_dist, max_history, primary_components)
        s, sref = _summary(abi.ReprojectSummary, summary)
        if on_device:
            q.on_device = 1
            ptrs, out, keep = [int(p) for p in device_ptrs], None, None
        else:
            keep = [np.ascontiguousarray(a, np.float32) for a in (acc, guides_from, guides_to)]
            out = np.empty(shapes[0], np.float32)
            ptrs = [k.ctypes.data for k in keep] + [out.ctypes.data]
        _check(self._lib, self._lib.phx_dev_film_reproject(self._h, C.byref(q), *ptrs, sref), "phx_dev_film_reproject")
        return out, _summary_dict(s)

    def reproject_times(self):
        """milliseconds of the last reproject(): dict of kernel (HIP events) and call (host clock)"""
        return self._times("phx_dev_reproject_times", 2, ("kernel", "call"))

    def clamp_outliers(self, film, ref=None, radius=2, gamma=4.0, floor=0.0, trim=2, min_taps=4, exclude_centre=True, upper_only=True, clamped_history=0,
                       primary_components=4, normals=False, moments=True, samples=False, m2_offset=None, samples_offset=None, summary=True, out=None,
                       device_ptrs=None):
        """The outlier clamp (phx_dev_film_outlier_clamp; include/phx_xpu.h states the rule): every colour of every pixel of film is
        clamped to mean +- (gamma standard deviations + floor) of the (2 radius + 1)^2 window around the same pixel of ref ("primary" rgb of
        it; None: film itself), the `trim` brightest taps left out, a pixel with fewer than min_taps taps left alone -> (film, summary).
        The defaults are the despeckle of a frame film against itself: the centre excluded, upper only.  For a history clamp pass the
        reprojected accumulator as film, the new camera's first frame film as ref, exclude_centre=False, upper_only=False and
        clamped_history, the most samples a clamped pixel may go on claiming (0: no cap; needs samples).  "m2" is scaled with a clamped
        colour.  The clamp is BIASED: it removes the energy the outliers carried.  The defaults are settings, not measurements.
        film's layout is derived as Film derives it from primary_components, normals, moments and samples, or given by m2_offset and
        samples_offset (0: none).  A C-contiguous float32 film is clamped in place and returned; anything else is copied first; out: an
        array of film's shape that receives the result instead (it may be ref), film is then left alone.  summary: a dict of pixels,
        skipped, unbounded, inside, clamped and capped (None with summary=False).  device_ptrs: (film, ref, out) addresses of
        device-resident films (ref may be film's, out may be film's or ref's); film and ref then are only their shapes, and the call
        returns (None, summary).  Needs no scene."""
        on_device = device_ptrs is not None
        shape_a = _film_shape(film, on_device)
        shape_b = shape_a if ref is None else _film_shape(ref, on_device)
        q = outlier_clamp_settings(shape_a, shape_b, radius, gamma, floor, trim, min_taps, exclude_centre, upper_only, clamped_history, primary_components,
                                   normals, moments, samples, m2_offset, samples_offset)
        s, sref = _summary(abi.OutlierClampSummary, summary)
        if on_device:
            q.on_device = 1
            (pa, pb, po), res, keep = (int(p) for p in device_ptrs), None, None
        else:
            if out is not None and (not _writable_f32(out) or out.shape != tuple(shape_a)):
                raise ValueError("clamp_outliers: out must be a writable C-contiguous float32 array of film's shape")
            if out is None:
                src = res = _in_place(film)
            else:
                src, res = np.ascontiguousarray(film, np.float32), out
            keep = src if ref is None or ref is film else out if ref is out else np.ascontiguousarray(ref, np.float32)
            pa, pb, po = src.ctypes.data, keep.ctypes.data, res.ctypes.data
        _check(self._lib, self._lib.phx_dev_film_outlier_clamp(self._h, C.byref(q), pa, pb, po, sref), "phx_dev_film_outlier_clamp")
        return res, _summary_dict(s)

    def outlier_clamp_times(self):
        """milliseconds of the last clamp_outliers(): dict of kernel (HIP events) and call (host clock)"""
        return self._times("phx_dev_outlier_clamp_times", 2, ("kernel", "call"))

    def display(self, film, exposure=1.0, tone="aces", white=4.0, dither=True, key=0.18, percentiles=(0.5, 0.95), scale_range=(2.0 ** -12, 2.0 ** 12),
                summary=False, device_ptr=None, image_on_host=True, image_ptr=None, image_pitch=0, fallback=1.0):
        """The display pass (phx_dev_film_display; include/phx_xpu.h states the rule): film (H, W, xstride) f32 of any layout, of
        which "primary" rgb is read, -> an (H, W, 4) uint8 image R, G, B, 255: radiance times the exposure, through the tone curve ("clamp",
        "reinhard" with its `white`, "aces") and the sRGB transfer function, rounded to 8 bits with a 4 x 4 ordered dither (dither=False:
        plain rounding).  exposure: the multiplier, or "auto": the device takes it from the film's own luminance histogram, so that the
        logarithmic mean between the two `percentiles` lands on `key`, within scale_range; a film without a lit pixel is shown at `fallback`.
        summary=True: -> (image, summary), a dict of pixels, invalid, unlit, counted, scale,
        from_histogram and histogram, the 256 counts.
        device_ptr: the address of a device-resident film; `film` then is only its shape (H, W, xstride).  With image_on_host (the preview:
        4 bytes a pixel come back instead of the film) the image is returned as above; otherwise image_ptr is the address of a
        device-resident image of image_pitch bytes a row (0: 4 * W), and None is returned in the image's place.  Needs no scene."""
        shape = _film_shape(film, device_ptr is not None)
        q = display_settings(shape, exposure, tone, white, dither, key, percentiles, scale_range, fallback)
        s, h = (abi.DisplaySummary(), (C.c_uint64 * 256)()) if summary else (None, None)
        if device_ptr is not None and not image_on_host:
            if image_ptr is None:
                raise ValueError("display: a device-resident image needs its address (image_ptr)")
            q.on_device, q.image_pitch = 1, int(image_pitch)
            src, out, dst = int(device_ptr), None, int(image_ptr)
        else:
            if image_ptr is not None:
                raise ValueError("display: image_ptr is a device address: it needs device_ptr and image_on_host=False")
            q.on_device = 0 if device_ptr is None else 2
            out = np.empty((q.height, q.width, 4), np.uint8)
            (src, keep), dst = _read_only(film, device_ptr), out.ctypes.data
        _check(self._lib, self._lib.phx_dev_film_display(self._h, C.byref(q), src, dst, C.byref(s) if summary else None, h), "phx_dev_film_display")
        if not summary:
            return out
        info = {k: int(getattr(s, k)) for k in ("pixels", "invalid", "unlit", "counted", "from_histogram")}
        info.update(scale=float(s.scale), histogram=np.array(h[:], np.uint64))
        return out, info

    def display_times(self):
        """milliseconds of the last display(): dict of histogram (with the exposure) and encode (HIP events) and call (host clock)"""
        return self._times("phx_dev_display_times", 3, ("histogram", "encode", "call"))

    # ---- stage-level hooks (parity tests) -------------------------------------------------------
    def adaptive_select(self, acc, samples_done, spp, threshold, floor=0.0, min_samples=16, step=16, active=None, num_active=None):
        """The selection of adaptive sampling behind a round that ended at samples_done of spp samples, on the caller's data
        (phx_dev_adaptive_select): acc (rows, 7) f32 = primary rgb, m2 rgb, samples; active: ascending row indices, or None for rows
        0 .. num_active - 1 (default: every row) -> (the new acc, survivors (k,) u32: the rows that go on, in the order of active).  Needs no scene."""
        out = np.array(acc, np.float32, order="C").reshape(-1, 7)
        if active is not None:
            active = np.ascontiguousarray(active, np.uint32)
            num_active = len(active)
        elif num_active is None:
            num_active = len(out)
        a = abi.Adaptive(threshold=threshold, floor=floor, min_samples=min_samples, step=step)
        surv = np.zeros(max(num_active, 1), np.uint32); n = C.c_uint32(0)
        _check(self._lib, self._lib.phx_dev_adaptive_select(self._h, num_active, None if active is None else _u32p(active), len(out), _f32p(out),
                                                            int(samples_done), int(spp), C.byref(a), _u32p(surv), C.byref(n)), "phx_dev_adaptive_select")
        return out, surv[:n.value].copy()

    def trace(self, o, d, tmax, shadow=False):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = len(tmax)
        t = np.zeros(n, np.float32); u = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        prim = np.zeros(n, np.uint32); hit = np.zeros(n, np.uint8)
        _check(self._lib, self._lib.phx_dev_trace(self._h, n, _f32p(o), _f32p(d), _f32p(tmax), 1 if shadow else 0, _f32p(t), _f32p(u), _f32p(v),
                                                  _u32p(prim), hit.ctypes.data_as(abi.u8p)), "phx_dev_trace")
        return {"t": t, "u": u, "v": v, "prim": prim, "hit": hit.astype(bool)}

    def bsdf_f(self, material, n, wi, wo):
        n = np.ascontiguousarray(n, np.float32); wi = np.ascontiguousarray(wi, np.float32); wo = np.ascontiguousarray(wo, np.float32)
        out = np.zeros_like(wi)
        _check(self._lib, self._lib.phx_dev_bsdf_f(self._h, material, len(wi), _f32p(n), _f32p(wi), _f32p(wo), _f32p(out)), "phx_dev_bsdf_f")
        return out

    def film_moments(self, radiance, acc, samples_done, inv):
        """One pass of the film stage of a frame with moments=True on the caller's data (phx_dev_film_moments): radiance (pixels, samples, 4)
        f32, the samples samples_done .. samples_done + samples - 1 of every pixel; acc (pixels, 6) f32 = primary rgb and m2 rgb as the passes
        before left them (zeros before the first) -> the new (pixels, 6).  Needs no scene."""
        radiance = np.ascontiguousarray(radiance, np.float32)
        if radiance.ndim != 3 or radiance.shape[2] != 4:
            raise ValueError("film_moments: radiance must be (pixels, samples, 4)")
        out = np.array(acc, np.float32, order="C").reshape(-1, 6)
        if len(out) != radiance.shape[0]:
            raise ValueError("film_moments: acc must have one row of 6 per pixel")
        _check(self._lib, self._lib.phx_dev_film_moments(self._h, radiance.shape[0], radiance.shape[1], int(samples_done), float(inv), _f32p(radiance), _f32p(out)),
               "phx_dev_film_moments")
        return out

    def bsdf_sample(self, material, n, wi, u2):
        n = np.ascontiguousarray(n, np.float32); wi = np.ascontiguousarray(wi, np.float32); u2 = np.ascontiguousarray(u2, np.float32)
        k = len(wi)
        wo = np.zeros((k, 3), np.float32); f = np.zeros((k, 3), np.float32); pdf = np.zeros(k, np.float32); fl = np.zeros(k, np.uint32)
        _check(self._lib, self._lib.phx_dev_bsdf_sample(self._h, material, k, _f32p(n), _f32p(wi), _f32p(u2), _f32p(wo), _f32p(f), _f32p(pdf),
                                                        _u32p(fl)), "phx_dev_bsdf_sample")
        return wo, f, pdf, fl

    def lobe_weights(self, material, n, wi, st=None):
        """The closure weights of material `material` as the shade kernel resolves them at n hits (shading normal n, view direction wi =
        hits.wi, texture coordinates st): (w (n, MAX_LOBES, 3) f32, kept (n,) u32 with bit k set where baked lobe k is there at the hit).
        st may be omitted for a scene without textured or masked lobes."""
        n = np.ascontiguousarray(n, np.float32).reshape(-1, 3); wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        k = len(wi)
        st = np.zeros((k, 2), np.float32) if st is None else np.ascontiguousarray(st, np.float32).reshape(-1, 2)
        if len(n) != k or len(st) != k:
            raise ValueError("lobe_weights: n, wi and st must have one row per item")
        w = np.zeros((k, abi.MAX_LOBES, 3), np.float32); kept = np.zeros(k, np.uint32)
        _check(self._lib, self._lib.phx_dev_lobe_weights(self._h, material, k, _f32p(n), _f32p(wi), _f32p(st), _f32p(w), _u32p(kept)),
               "phx_dev_lobe_weights")
        return w, kept

    def light_sample(self, u3):
        """Next-event estimation's light sample as the shade kernel draws it, in this device's light_sampling mode: u3 (n, 3) = (pick, lu,
        lv) per item -> dict of light (n,) u32, tri (n,) u32 (index inside the light, face order), bary (n, 2) f32 (bu, bv), P (n, 3) f32 and
        pdf (n,) f32 (the light's lpdf).  phx_dev_light_sample."""
        u3 = np.ascontiguousarray(u3, np.float32).reshape(-1, 3)
        k = len(u3)
        light = np.zeros(k, np.uint32); tri = np.zeros(k, np.uint32)
        bary = np.zeros((k, 2), np.float32); P = np.zeros((k, 3), np.float32); pdf = np.zeros(k, np.float32)
        _check(self._lib, self._lib.phx_dev_light_sample(self._h, k, _f32p(u3), _u32p(light), _u32p(tri), _f32p(bary), _f32p(P), _f32p(pdf)), "phx_dev_light_sample")
        return {"light": light, "tri": tri, "bary": bary, "P": P, "pdf": pdf}

    def light_emission(self, u3):
        """The emission next-event estimation uses at the light samples of light_sample(u3): u3 (n, 3) = (pick, lu, lv) per item -> dict of
        st (n, 2) f32, the sampled point's texture coordinates by the rule of phx_material.emission_uv_texture, and e (n, 3) f32, the light's
        emission times its image's texel there.  A light without an image: its constant emission and st = (0, 0).  phx_dev_light_emission."""
        u3 = np.ascontiguousarray(u3, np.float32).reshape(-1, 3)
        k = len(u3)
        st = np.zeros((k, 2), np.float32); e = np.zeros((k, 3), np.float32)
        _check(self._lib, self._lib.phx_dev_light_emission(self._h, k, _f32p(u3), _f32p(st), _f32p(e)), "phx_dev_light_emission")
        return {"st": st, "e": e}

    def environment_sample(self, u3):
        """Next-event estimation's environment sample under environment_sampling, as the shade kernel draws it: u3 (n, 3) = (pick, lu, lv) per
        item -> dict of light (n,) u32 (== the number of mesh lights for an environment pick; every other output is zero for a mesh pick),
        texel (n, 2) u32 (i, j), st (n, 2) f32, dir (n, 3) f32, pdf (n,) f32 = p_env * pdf_omega (0: no shadow ray) and e (n, 3) f32, the
        environment's emission in that direction.  phx_dev_environment_sample."""
        u3 = np.ascontiguousarray(u3, np.float32).reshape(-1, 3)
        k = len(u3)
        light = np.zeros(k, np.uint32); texel = np.zeros((k, 2), np.uint32)
        st = np.zeros((k, 2), np.float32); d = np.zeros((k, 3), np.float32); pdf = np.zeros(k, np.float32); e = np.zeros((k, 3), np.float32)
        _check(self._lib, self._lib.phx_dev_environment_sample(self._h, k, _f32p(u3), _u32p(light), _u32p(texel), _f32p(st), _f32p(d), _f32p(pdf), _f32p(e)),
               "phx_dev_environment_sample")
        return {"light": light, "texel": texel, "st": st, "dir": d, "pdf": pdf, "e": e}

    def texture_lookup(self, texture, st):
        """The shade kernel's image lookup on the device: texture `texture` (0-based index into SceneDesc.textures of the preprocessed
        scene, which must have a textured lobe) at st (n, 2) -> rgb (n, 3) f32."""
        st = np.ascontiguousarray(st, np.float32).reshape(-1, 2)
        out = np.zeros((len(st), 3), np.float32)
        _check(self._lib, self._lib.phx_dev_texture_lookup(self._h, texture, len(st), _f32p(st), _f32p(out)),
               "phx_dev_texture_lookup")
        return out

    def environment_lookup(self, dirs):
        """The shade kernel's environment on a miss, on the device: e = emission * texel(s, t) of the preprocessed scene's environment
        image at directions dirs (n, 3) -> rgb (n, 3) f32 (phx_dev_environment_lookup; DeviceError when the environment has no image)."""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros((len(dirs), 3), np.float32)
        _check(self._lib, self._lib.phx_dev_environment_lookup(self._h, len(dirs), _f32p(dirs), _f32p(out)),
               "phx_dev_environment_lookup")
        return out

    def bvh_pool(self):
        """the acceleration structure as the kernels read it: (uint32 array [elements, 16], grid lo[3], grid cell[3]) — phx_dev_copy_bvh"""
        n = C.c_uint64(0); grid = np.zeros(6, np.float32)
        _check(self._lib, self._lib.phx_dev_copy_bvh(self._h, None, 0, C.byref(n), _f32p(grid)), "phx_dev_copy_bvh")
        pool = np.zeros(n.value // 4, np.uint32)
        _check(self._lib, self._lib.phx_dev_copy_bvh(self._h, pool.ctypes.data_as(C.c_void_p), n.value, C.byref(n), _f32p(grid)), "phx_dev_copy_bvh")
        return pool.reshape(-1, 16), grid[:3].copy(), grid[3:].copy()

    def close(self):
        """~xpu_t: joins a frame that is still running (its callbacks may fire until then: they are kept alive up to here)"""
        if self._h:
            self._lib.phx_dev_destroy(self._h)
            self._h = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
