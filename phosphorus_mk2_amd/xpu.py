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
"""
import ctypes as C
import math
import os
import threading

import numpy as np

from . import abi

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


def film_layout(primary_components=4, normals=False, moments=False, samples=False):
    """The channel order of a film's pixel, derived here and nowhere else: "primary", then "normals" (3 floats), "m2" (3 floats) and "samples"
    (1 float), each only when asked for -> (normals_offset, m2_offset, samples_offset, xstride); the offset of a channel that is not there
    is 0, as in the structs of include/phx_xpu.h."""
    xstride, offsets = primary_components, []
    for there, floats in ((normals, 3), (moments, 3), (samples, 1)):
        offsets.append(xstride if there else 0)
        xstride += floats if there else 0
    return offsets[0], offsets[1], offsets[2], xstride


def _film_shape(film, on_device):  # a device-resident film is given by its shape, or by an array of it
    return tuple(film) if on_device and not hasattr(film, "shape") else film.shape


def _writable_f32(a):  # an array a film call can work on in place
    return isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable


def _summary_dict(s):  # a summary struct of counts, or None
    return None if s is None else {k: int(getattr(s, k)) for k, _ in s._fields_}


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
        _, self.m2_offset, self.samples_offset, _ = film_layout(primary_components, normals, True, True)
        self.xstride = film_layout(primary_components, normals, moments, adaptive)[3]
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
            gref, keep = None, None
        else:
            gshape = _film_shape(guides, guides_ptr is not None)
            if len(gshape) != 3 or tuple(gshape[:2]) != tuple(shape[:2]):
                raise ValueError(f"denoise: the guide film must be (height, width, >= 8) over the film's pixels, not {tuple(gshape)}")
            if plane and plane_scale is None:
                if self._scene is None:
                    raise ValueError("denoise: plane=True needs plane_scale (guide_plane_scale(camera)) on a device without a preprocessed scene")
                plane_scale = guide_plane_scale(self._camera or self._scene.camera)
            keep = None if guides_ptr is not None else np.ascontiguousarray(guides, np.float32)
            g = abi.DenoiseGuides(guides=guides_ptr if guides_ptr is not None else keep.ctypes.data, xstride=int(gshape[2]),
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
        s = abi.AccumulateSummary() if threshold is not None else None
        sref = C.byref(s) if s is not None else None
        if on_device:
            q.on_device = 1
            pa, pb = (int(p) for p in device_ptrs)
            out = keep = None
        else:
            out = acc if _writable_f32(acc) else np.array(acc, np.float32, order="C")
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
        keep = None if device_ptr is not None else np.ascontiguousarray(acc, np.float32)
        tx, ty = -(-q.width // q.tile_width), -(-q.height // q.tile_height)
        records = np.zeros(tx * ty, TILE_RECORD)
        s = abi.TileMapSummary() if summary else None
        _check(self._lib, self._lib.phx_dev_film_tile_map(self._h, C.byref(q), int(device_ptr) if device_ptr is not None else keep.ctypes.data,
                                                          records.ctypes.data, C.byref(s) if summary else None), "phx_dev_film_tile_map")
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
        s = abi.ReprojectSummary() if summary else None
        if on_device:
            q.on_device = 1
            ptrs, out, keep = [int(p) for p in device_ptrs], None, None
        else:
            keep = [np.ascontiguousarray(a, np.float32) for a in (acc, guides_from, guides_to)]
            out = np.empty(shapes[0], np.float32)
            ptrs = [k.ctypes.data for k in keep] + [out.ctypes.data]
        _check(self._lib, self._lib.phx_dev_film_reproject(self._h, C.byref(q), ptrs[0], ptrs[1], ptrs[2], ptrs[3], C.byref(s) if s is not None else None),
               "phx_dev_film_reproject")
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
        s = abi.OutlierClampSummary() if summary else None
        if on_device:
            q.on_device = 1
            (pa, pb, po), res, keep = (int(p) for p in device_ptrs), None, None
        else:
            if out is not None and (not _writable_f32(out) or out.shape != tuple(shape_a)):
                raise ValueError("clamp_outliers: out must be a writable C-contiguous float32 array of film's shape")
            if out is None:
                src = res = film if _writable_f32(film) else np.array(film, np.float32, order="C")
            else:
                src, res = np.ascontiguousarray(film, np.float32), out
            keep = src if ref is None or ref is film else out if ref is out else np.ascontiguousarray(ref, np.float32)
            pa, pb, po = src.ctypes.data, keep.ctypes.data, res.ctypes.data
        _check(self._lib, self._lib.phx_dev_film_outlier_clamp(self._h, C.byref(q), pa, pb, po, C.byref(s) if s is not None else None),
               "phx_dev_film_outlier_clamp")
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
            keep = None if device_ptr is not None else np.ascontiguousarray(film, np.float32)
            out = np.empty((q.height, q.width, 4), np.uint8)
            src, dst = int(device_ptr) if device_ptr is not None else keep.ctypes.data, out.ctypes.data
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
        up = lambda x: x.ctypes.data_as(abi.u32p)
        _check(self._lib, self._lib.phx_dev_adaptive_select(self._h, num_active, None if active is None else up(active), len(out), out.ctypes.data_as(abi.f32p),
                                                            int(samples_done), int(spp), C.byref(a), up(surv), C.byref(n)), "phx_dev_adaptive_select")
        return out, surv[:n.value].copy()

    def trace(self, o, d, tmax, shadow=False):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = len(tmax)
        t = np.zeros(n, np.float32); u = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        prim = np.zeros(n, np.uint32); hit = np.zeros(n, np.uint8)
        fp = lambda a: a.ctypes.data_as(abi.f32p)
        _check(self._lib, self._lib.phx_dev_trace(self._h, n, fp(o), fp(d), fp(tmax), 1 if shadow else 0, fp(t), fp(u), fp(v),
                                                  prim.ctypes.data_as(abi.u32p), hit.ctypes.data_as(abi.u8p)), "phx_dev_trace")
        return {"t": t, "u": u, "v": v, "prim": prim, "hit": hit.astype(bool)}

    def bsdf_f(self, material, n, wi, wo):
        n = np.ascontiguousarray(n, np.float32); wi = np.ascontiguousarray(wi, np.float32); wo = np.ascontiguousarray(wo, np.float32)
        out = np.zeros_like(wi)
        fp = lambda a: a.ctypes.data_as(abi.f32p)
        _check(self._lib, self._lib.phx_dev_bsdf_f(self._h, material, len(wi), fp(n), fp(wi), fp(wo), fp(out)), "phx_dev_bsdf_f")
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
        fp = lambda a: a.ctypes.data_as(abi.f32p)
        _check(self._lib, self._lib.phx_dev_film_moments(self._h, radiance.shape[0], radiance.shape[1], int(samples_done), float(inv), fp(radiance), fp(out)),
               "phx_dev_film_moments")
        return out

    def bsdf_sample(self, material, n, wi, u2):
        n = np.ascontiguousarray(n, np.float32); wi = np.ascontiguousarray(wi, np.float32); u2 = np.ascontiguousarray(u2, np.float32)
        k = len(wi)
        wo = np.zeros((k, 3), np.float32); f = np.zeros((k, 3), np.float32); pdf = np.zeros(k, np.float32); fl = np.zeros(k, np.uint32)
        fp = lambda a: a.ctypes.data_as(abi.f32p)
        _check(self._lib, self._lib.phx_dev_bsdf_sample(self._h, material, k, fp(n), fp(wi), fp(u2), fp(wo), fp(f), fp(pdf),
                                                        fl.ctypes.data_as(abi.u32p)), "phx_dev_bsdf_sample")
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
        fp = lambda a: a.ctypes.data_as(abi.f32p)
        _check(self._lib, self._lib.phx_dev_lobe_weights(self._h, material, k, fp(n), fp(wi), fp(st), fp(w), kept.ctypes.data_as(abi.u32p)),
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
        fp = lambda a: a.ctypes.data_as(abi.f32p)
        up = lambda a: a.ctypes.data_as(abi.u32p)
        _check(self._lib, self._lib.phx_dev_light_sample(self._h, k, fp(u3), up(light), up(tri), fp(bary), fp(P), fp(pdf)), "phx_dev_light_sample")
        return {"light": light, "tri": tri, "bary": bary, "P": P, "pdf": pdf}

    def light_emission(self, u3):
        """The emission next-event estimation uses at the light samples of light_sample(u3): u3 (n, 3) = (pick, lu, lv) per item -> dict of
        st (n, 2) f32, the sampled point's texture coordinates by the rule of phx_material.emission_uv_texture, and e (n, 3) f32, the light's
        emission times its image's texel there.  A light without an image: its constant emission and st = (0, 0).  phx_dev_light_emission."""
        u3 = np.ascontiguousarray(u3, np.float32).reshape(-1, 3)
        k = len(u3)
        st = np.zeros((k, 2), np.float32); e = np.zeros((k, 3), np.float32)
        fp = lambda a: a.ctypes.data_as(abi.f32p)
        _check(self._lib, self._lib.phx_dev_light_emission(self._h, k, fp(u3), fp(st), fp(e)), "phx_dev_light_emission")
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
        fp = lambda a: a.ctypes.data_as(abi.f32p)
        up = lambda a: a.ctypes.data_as(abi.u32p)
        _check(self._lib, self._lib.phx_dev_environment_sample(self._h, k, fp(u3), up(light), up(texel), fp(st), fp(d), fp(pdf), fp(e)),
               "phx_dev_environment_sample")
        return {"light": light, "texel": texel, "st": st, "dir": d, "pdf": pdf, "e": e}

    def texture_lookup(self, texture, st):
        """The shade kernel's image lookup on the device: texture `texture` (0-based index into SceneDesc.textures of the preprocessed
        scene, which must have a textured lobe) at st (n, 2) -> rgb (n, 3) f32."""
        st = np.ascontiguousarray(st, np.float32).reshape(-1, 2)
        out = np.zeros((len(st), 3), np.float32)
        _check(self._lib, self._lib.phx_dev_texture_lookup(self._h, texture, len(st), st.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p)),
               "phx_dev_texture_lookup")
        return out

    def environment_lookup(self, dirs):
        """The shade kernel's environment on a miss, on the device: e = emission * texel(s, t) of the preprocessed scene's environment
        image at directions dirs (n, 3) -> rgb (n, 3) f32 (phx_dev_environment_lookup; DeviceError when the environment has no image)."""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros((len(dirs), 3), np.float32)
        _check(self._lib, self._lib.phx_dev_environment_lookup(self._h, len(dirs), dirs.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p)),
               "phx_dev_environment_lookup")
        return out

    def bvh_pool(self):
        """the acceleration structure as the kernels read it: (uint32 array [elements, 16], grid lo[3], grid cell[3]) — phx_dev_copy_bvh"""
        n = C.c_uint64(0); grid = np.zeros(6, np.float32)
        _check(self._lib, self._lib.phx_dev_copy_bvh(self._h, None, 0, C.byref(n), grid.ctypes.data_as(abi.f32p)), "phx_dev_copy_bvh")
        pool = np.zeros(n.value // 4, np.uint32)
        _check(self._lib, self._lib.phx_dev_copy_bvh(self._h, pool.ctypes.data_as(C.c_void_p), n.value, C.byref(n), grid.ctypes.data_as(abi.f32p)), "phx_dev_copy_bvh")
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


def film_variance(data, spp, primary_components=4, normals=False, adaptive=False):
    """The unbiased estimate of the variance of every pixel's film value from a film rendered with moments=True: data (..., xstride) as
    render() returns it -> m2 * S / (S - 1) in float64, shape (..., 3); S = spp.  The film value is a SUM of S samples y_s (each carries the
    film's 1 / (spp * pps)), and m2 is their centred sum of squares, so S / (S - 1) * m2 estimates S * var(y).  spp == 1 says nothing: inf.
    adaptive=True: a film of adaptive sampling (one more float per pixel, "samples"): m2 * n / (n - 1) from the pixel's OWN n, which holds
    after the rescale of a pixel that stopped as well; inf where n <= 1.  spp is not used then."""
    data = np.asarray(data)
    _, off, samples_offset, want = film_layout(primary_components, normals, True, adaptive)
    if data.shape[-1] != want:
        raise ValueError(f"film_variance: a film with the m2 channel has {want} floats per pixel, this one {data.shape[-1]}")
    m2 = data[..., off:off + 3].astype(np.float64)
    if adaptive:
        n = data[..., samples_offset].astype(np.float64)[..., None]
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
    no, m2_offset, samples_offset, want_a = film_layout(primary_components, normals, True, True)
    if xa != want_a:
        raise ValueError(f"accumulate: an accumulator has {want_a} floats per pixel in this layout (xpu.accumulator), this one {xa}")
    _, _, samples_offset_b, want = film_layout(primary_components, normals, True, frame_adaptive)
    if xb != want:
        raise ValueError(f"accumulate: a frame film with the m2 channel has {want} floats per pixel in this layout, this one {xb} "
                         "(accumulation needs frames rendered with moments=True)")
    return abi.Accumulate(width=W, height=H, xstride_a=xa, normals_offset_a=no, m2_offset_a=m2_offset, samples_offset_a=samples_offset,
                          xstride_b=xb, normals_offset_b=no, m2_offset_b=m2_offset, samples_offset_b=samples_offset_b,
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
    _, m2_offset, samples_offset, want = film_layout(primary_components, normals, True, True)
    if xs != want:
        raise ValueError(f"tile_map: an accumulator has {want} floats per pixel in this layout (xpu.accumulator), this one {xs}")
    tw, th = (int(tile_size),) * 2 if np.isscalar(tile_size) else (int(v) for v in tile_size)
    return abi.TileMap(width=W, height=H, xstride=xs, m2_offset=m2_offset, samples_offset=samples_offset, tile_width=tw, tile_height=th,
                       on_device=0, tau=float(threshold), floor=float(floor))


def open_tiles(records, coverage=1.0):
    """The tiles of a tile map's records a progressive frame still renders -> list of (x, y, w, h), in the records' order.  coverage == 1: the
    open tiles as phx_tile_map defines them; coverage < 1 closes a tile once converged >= coverage * (w * h - invalid) and starved == 0."""
    converged, starved = records["converged"].astype(np.int64), records["starved"]
    valid = records["w"].astype(np.int64) * records["h"] - records["invalid"]
    if coverage >= 1.0:
        is_open = (converged < valid) | (starved > 0)
    else:
        is_open = ~((converged >= float(coverage) * valid) & (starved == 0))
    return [tuple(t) for t in np.stack([records[f] for f in ("x", "y", "w", "h")], 1)[is_open].tolist()]


def tile_map_grid(width, height, tile_size):
    """The tile map's grid without a film: TILE_RECORD entries with only x, y, w, h set, in the records' order (phx_tile_map states it)"""
    tw, th = (int(tile_size),) * 2 if np.isscalar(tile_size) else (int(v) for v in tile_size)
    tx, ty = -(-width // tw), -(-height // th)
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
    _, derived_m2, derived_samples, _ = film_layout(primary_components, normals, moments, samples)
    behind = film_layout(primary_components, normals)[3]  # "primary" and "normals": what the film holds at least
    m2_offset = derived_m2 if m2_offset is None else m2_offset
    samples_offset = derived_samples if samples_offset is None else samples_offset
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


def display(film, **settings):
    """HipDevice.display on a device made for the call (no scene is needed) and closed behind it: film (H, W, xstride) f32 -> (H, W, 4) uint8,
    or (image, summary) with summary=True."""
    dev = HipDevice.make(Options(samples_per_pixel=1, paths_per_sample=1, path_depth=1))
    try:
        return dev.display(film, **settings)
    finally:
        dev.close()


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
    dev = HipDevice.make(Options(samples_per_pixel=spp, paths_per_sample=pps, path_depth=depth, **options))
    try:
        if adaptive is not None:
            dev.set_adaptive(**adaptive)
        elif by_tiles:  # only marks samples = spp: one round that ends at spp, no decision is ever taken
            dev.set_adaptive(threshold=0.0, floor=0.0, min_samples=max(spp, 2), step=1)
        dev.preprocess(scene_desc)
        W, H = scene_desc.camera.width, scene_desc.camera.height
        acc = accumulator(W, H, 4, normals)
        settings, guides = None, None
        if denoise is not None:
            settings = dict(denoise)
            gset = settings.pop("guides", None)
            if gset is not None:
                gset = dict(gset)
                guides = dev.render_guides(seed, min(int(gset.pop("samples", 4)), spp))
                settings.update(gset)
        with_samples = adaptive is not None or by_tiles
        for k in range(frames):
            film = Film(W, H, 4, normals, True, with_samples)
            queue, frame_tiles = None, None
            if by_tiles:
                if k < min_frames:
                    records = tile_map_grid(W, H, map_size)
                    frame_tiles = [tuple(t) for t in np.stack([records[f] for f in ("x", "y", "w", "h")], 1).tolist()]
                else:
                    records, _ = dev.tile_map(acc, map_size, stop["threshold"], stop.get("floor", 0.0), 4, normals, summary=False)
                    frame_tiles = open_tiles(records, tile_coverage)
                    if not frame_tiles:
                        return
                queue = Tiles.from_list(frame_tiles, W, H)
            dev.start(scene_desc, FrameState((seed + k) % (1 << 64), queue if by_tiles else Tiles.make(W, H, tile_size), film, native_sink=True))
            dev.join()
            if despeckle is not None:
                dev.clamp_outliers(film.data, **{**despeckle, "exclude_centre": True, "upper_only": True, "primary_components": 4, "normals": normals,
                                                 "moments": True, "samples": adaptive is not None, "summary": False})
            _, summary = dev.accumulate(acc, film.data, spp, 4, normals, with_samples, **(stop or {}))
            if by_tiles:
                summary.update(tiles=len(records), tiles_open=len(frame_tiles), rendered_pixels=sum(t[2] * t[3] for t in frame_tiles))
            out = acc if settings is None else dev.denoise(acc, spp, 4, normals, True, guides=guides, **settings)
            if display is None:
                yield out, summary, k + 1
            else:
                yield out, summary, k + 1, dev.display(out, **display)
            valid = summary["pixels"] - summary["invalid"] if summary is not None else 0
            if valid > 0 and summary["converged"] >= coverage * valid:  # (a film without one valid pixel, as any film of 1 spp, has not converged)
                return
    finally:
        dev.close()


def render_camera_path(scene_desc, cameras, spp, frames_per_camera=1, seed=1, guide_samples=4, reproject=None, denoise=None, display=None,
                       pps=1, depth=9, tile_size=32, history_clamp=None, **options):
    """A camera path through a static scene on ONE device: the scene is preprocessed once; then, per camera of `cameras`
    (CameraDescs of the scene's film size): set_camera; the guide film (guide_samples samples, the seed of the camera's first frame); from
    the second camera on the accumulator is carried over by HipDevice.reproject (`reproject`: a dict of its settings, sigma_plane=,
    sigma_dist=, max_history=); then frames_per_camera frames of `spp` samples with seeds (seed + k) mod 2^64, k counting frames over the
    whole path, each pooled by HipDevice.accumulate.  A generator: after every frame it yields (film, summary, frames_done, reprojection),
    as render_progressive yields (summary is None: there is no stop) plus the summary of the reprojection that led to this camera (None at
    the first); with display, (..., reprojection, image).  film is the accumulator (H, W, 14) f32 in xpu.accumulator's layout with
    normals, replaced at every camera: copy it to keep it.  denoise, display, options: as for render_progressive; the guided denoiser
    reads this camera's guide film (no entry `guides` is needed: guides=dict(...) carries its settings).  history_clamp: a dict of
    HipDevice.clamp_outliers' settings (radius=, gamma=, floor=, trim=, min_taps=, clamped_history=; {} for the defaults): from the second
    camera on the reprojected accumulator is clamped, two-sided and with the centre included, against the neighbourhoods of that camera's
    first frame film before that frame is pooled."""
    if frames_per_camera < 1:
        raise ValueError("render_camera_path: frames_per_camera must be at least 1")
    dev = HipDevice.make(Options(samples_per_pixel=spp, paths_per_sample=pps, path_depth=depth, **options))
    try:
        dev.preprocess(scene_desc)
        W, H = scene_desc.camera.width, scene_desc.camera.height
        acc = accumulator(W, H, 4, True)
        settings, guided = None, False
        if denoise is not None:
            settings = dict(denoise)
            gset = settings.pop("guides", None)
            if gset is not None:
                gset = dict(gset)
                gset.pop("samples", None)
                settings.update(gset)
                guided = True
        k, previous, guides_before = 0, None, None
        for camera in cameras:
            dev.set_camera(camera)
            guides = dev.render_guides((seed + k) % (1 << 64), min(int(guide_samples), spp))
            moved = None
            if previous is not None:
                acc, moved = dev.reproject(acc, guides_before, guides, previous, camera, **(reproject or {}))
            for first in [True] + [False] * (frames_per_camera - 1):
                film = Film(W, H, 4, True, True, False)
                dev.start(scene_desc, FrameState((seed + k) % (1 << 64), Tiles.make(W, H, tile_size), film, native_sink=True))
                dev.join()
                k += 1
                if history_clamp is not None and previous is not None and first:
                    dev.clamp_outliers(acc, film.data, **{**history_clamp, "exclude_centre": False, "upper_only": False, "primary_components": 4,
                                                          "normals": True, "moments": True, "samples": True, "summary": False})
                dev.accumulate(acc, film.data, spp, 4, True, False)
                if settings is None:
                    out = acc
                else:
                    out = dev.denoise(acc, spp, 4, True, True, guides=guides if guided else None,
                                      **({"plane_scale": guide_plane_scale(camera), **settings} if guided else settings))
                if display is None:
                    yield out, None, k, moved
                else:
                    yield out, None, k, moved, dev.display(out, **display)
            previous, guides_before = camera, guides
    finally:
        dev.close()


def render_animation(scene_descs, spp, mode="refit", rebuild_every=0, denoise=None, display=None, seed=1, pps=1, depth=9, tile_size=32, **options):
    """Moving geometry on ONE device: the first scene of `scene_descs` is preprocessed, every later one — the same scene
    with moved vertices — is taken by HipDevice.update_geometry(mode); with rebuild_every = k > 0 every k-th update is a "rebuild"
    whatever `mode` says.  One FRESH film of `spp` samples is rendered per scene, with sampler seed `seed`: nothing is accumulated or
    reprojected across geometry (a film of the old geometry says nothing about the new one).  A generator: per scene it yields (film,
    summary, index) — film (H, W, 11) f32 with normals and moments, summary the update's dict (None for the first scene) — and with
    display (..., image).  denoise, display: dicts of HipDevice.denoise's and HipDevice.display's settings; options: xpu.Options'."""
    dev = HipDevice.make(Options(samples_per_pixel=spp, paths_per_sample=pps, path_depth=depth, **options))
    try:
        for index, scene_desc in enumerate(scene_descs):
            summary = None
            if index == 0:
                dev.preprocess(scene_desc)
            else:
                summary = dev.update_geometry(scene_desc, "rebuild" if rebuild_every > 0 and index % rebuild_every == 0 else mode)
            W, H = scene_desc.camera.width, scene_desc.camera.height
            film = Film(W, H, 4, True, True, False)
            dev.start(scene_desc, FrameState(seed, Tiles.make(W, H, tile_size), film, native_sink=True))
            dev.join()
            out = film.data if denoise is None else dev.denoise(film.data, spp, 4, True, False, **denoise)
            if display is None:
                yield out, summary, index
            else:
                yield out, summary, index, dev.display(out, **display)
    finally:
        dev.close()


def render_on(devices, scene_desc, seed=1, normals=False, tile_size=32, native_sink=True, rank=0, world=1, moments=False, adaptive=False):
    """The reference's frame on SEVERAL devices in one process (src/core.cpp:103-115): every device is started on the SAME tile
    queue and the SAME film and joined in turn; no collective.  `devices` must have been preprocessed with `scene_desc`.
    adaptive=True only sizes the film for the channel "samples": the caller has set every device (HipDevice.set_adaptive).
    Returns (film array, [stats per device])."""
    W, H = scene_desc.camera.width, scene_desc.camera.height
    tiles = Tiles.make(W, H, tile_size, rank, world)
    film = Film(W, H, 4, normals, moments, bool(adaptive))
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
    dev = HipDevice.make(opts)
    try:
        if adaptive is not None:
            dev.set_adaptive(**adaptive)
        dev.preprocess(scene_desc)
        W, H = scene_desc.camera.width, scene_desc.camera.height
        tiles = Tiles.make(W, H, tile_size, rank, world)
        if callback_tiles:
            lst = []
            while True:
                t = tiles.next()
                if t is None:
                    break
                lst.append(t)
            tiles = CallbackTiles(lst)
        film = Film(W, H, 4, normals, moments, adaptive is not None)
        dev.start(scene_desc, FrameState(seed, tiles, film, native_sink=native_sink))
        dev.join()
        if denoise is not None:
            denoise = dict(denoise)
            gset = denoise.pop("guides", None)
            if gset is not None:
                gset = dict(gset)
                denoise.update(guides=dev.render_guides(seed, min(int(gset.pop("samples", 4)), spp)), **gset)
            return dev.denoise(film.data, spp, 4, normals, adaptive is not None, **denoise), dev.stats()
        return film.data, dev.stats()
    finally:
        dev.close()
