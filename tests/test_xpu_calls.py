"""The Python host layer's device calls, in order, without a device: tests/fake_phx.py stands in for the library, the loops of
phosphorus_mk2_amd/xpu.py run on it, and what they called, with what, is compared with sequences written out here.  Nothing is rendered;
what a device computes from these calls is held to its models in the tests marked gpu."""
import dataclasses

import numpy as np
import pytest

import fake_phx
from phosphorus_mk2_amd import abi, scenes, xpu

F = np.float32
W = H = 16
SPP = 4
FRAME = ["tiles_make", "start", "join"]
POOL = FRAME + ["film_accumulate"]
STOP = dict(threshold=0.05, floor=0.01, coverage=0.95)


@pytest.fixture
def scene():
    return scenes.cornell(W, H)


def converged_from(frame, pixels=W * H, converged=250):
    """a script of phx_dev_film_accumulate: the summary says `converged` of `pixels` from its frame-th call on, none before"""
    def script(n, args):
        if args[4] is not None:
            fake_phx.fill_summary(args, 4, pixels=pixels, invalid=0, converged=converged if n >= frame else 0)
    return script


def makes_and_destroys(fake):
    return fake.names().count("make"), fake.names().count("destroy")


# ---- render_progressive ----------------------------------------------------------------------------------------------------------------------
def test_progressive_plain(monkeypatch, scene):
    fake = fake_phx.install(monkeypatch)
    got = list(xpu.render_progressive(scene, SPP, 3, seed=2 ** 64 - 1))
    assert fake.names() == ["make", "preprocess"] + POOL * 3 + ["destroy"]
    frames, pools = [a[1] for a in fake.args("start")], fake.args("film_accumulate")
    assert [f.sampler_seed for f in frames] == [2 ** 64 - 1, 0, 1]
    assert all(f.moments_channel == 1 and f.normals_channel == 0 and f.primary_components == 4 and not f.add_tile for f in frames)
    assert [f.host_film for f in frames] == [p[3] for p in pools] and all(f.host_film for f in frames)
    assert [f.tiles_user for f in frames] == [0x2000, 0x3000, 0x4000] and fake.args("tiles_make") == [(W, H, 32, 0, 1)] * 3
    assert {p[2] for p in pools} == {got[0][0].ctypes.data} and all(g[0] is got[0][0] for g in got)
    assert all(p[4] is None for p in pools) and all(p[1].spp_b == SPP and p[1].samples_offset_b == 0 and p[1].on_device == 0 for p in pools)
    assert [(len(g), g[1], g[2]) for g in got] == [(3, None, 1), (3, None, 2), (3, None, 3)] and got[0][0].shape == (H, W, 8)


def test_progressive_stops_behind_the_frame_that_converged(monkeypatch, scene):
    fake = fake_phx.install(monkeypatch, phx_dev_film_accumulate=converged_from(2))
    got = list(xpu.render_progressive(scene, SPP, 5, stop=STOP))
    assert fake.names() == ["make", "preprocess"] + POOL * 2 + ["destroy"]
    assert [g[2] for g in got] == [1, 2] and got[1][1] == {"pixels": 256, "invalid": 0, "converged": 250, "samples": 0} and got[0][1]["converged"] == 0
    for _, q, _, _, summary in fake.args("film_accumulate"):
        assert (q.tau, q.floor) == (F(0.05), F(0.01)) and isinstance(summary, abi.AccumulateSummary)


def test_progressive_adaptive_and_despeckle(monkeypatch, scene):
    fake = fake_phx.install(monkeypatch)
    got = list(xpu.render_progressive(scene, SPP, 2, adaptive=dict(threshold=0.1, floor=0.02, min_samples=2, step=2), despeckle={}))
    assert fake.names() == ["make", "set_adaptive", "preprocess"] + (FRAME + ["film_outlier_clamp", "film_accumulate"]) * 2 + ["destroy"]
    a = fake.args("set_adaptive")[0][1]
    assert (a.threshold, a.floor, a.min_samples, a.step) == (F(0.1), F(0.02), 2, 2)
    for frame, clamp, pool in zip(fake.args("start"), fake.args("film_outlier_clamp"), fake.args("film_accumulate")):
        q = clamp[1]
        assert q.flags == abi.OUTLIER_EXCLUDE_CENTRE | abi.OUTLIER_UPPER_ONLY and clamp[2] == clamp[3] == clamp[4] == frame[1].host_film
        assert (q.xstride_a, q.m2_offset_a, q.samples_offset_a, q.xstride_b) == (8, 4, 7, 8) and clamp[5] is None
        assert pool[3] == frame[1].host_film and pool[1].samples_offset_b == 7 and pool[1].xstride_b == 8
    assert len(got) == 2


def test_progressive_guided_denoise_and_display(monkeypatch, scene):
    fake = fake_phx.install(monkeypatch)
    got = list(xpu.render_progressive(scene, SPP, 2, seed=11, normals=True, denoise=dict(iterations=3, guides=dict(samples=9, plane=True)), display={}))
    assert fake.names() == ["make", "preprocess", "render_guides"] + (POOL + ["denoise_guided", "film_display"]) * 2 + ["destroy"]
    (_, g, guide_film), = fake.args("render_guides")
    assert (g.sampler_seed, g.samples, g.on_device) == (11, 4, 0) and guide_film
    for pool, den, dis, out in zip(fake.args("film_accumulate"), fake.args("denoise_guided"), fake.args("film_display"), got):
        _, q, guides, src, dst = den
        assert src == pool[2] and dst != src and dis[2] == dst == out[0].ctypes.data and dis[4] is None and dis[5] is None
        assert (q.iterations, q.spp, q.xstride, q.normals_offset, q.m2_offset, q.samples_offset, q.on_device) == (3, SPP, 11, 4, 7, 10, 0)
        assert guides.guides == guide_film and guides.flags == abi.GUIDE_DEMODULATE | abi.GUIDE_PLANE and guides.xstride == 8
        assert guides.plane_scale == F(xpu.guide_plane_scale(scene.camera)) > 0
        assert len(out) == 4 and out[3].shape == (H, W, 4) and out[3].dtype == np.uint8 and out[3].ctypes.data == dis[3]


GRID = [(0, 0, 8, 8), (8, 0, 8, 8), (0, 8, 8, 8), (8, 8, 8, 8)]


def leaves_open(*per_call):
    """a script of phx_dev_film_tile_map: its n-th call leaves the tiles of per_call[n - 1] open (indices into the grid)"""
    return lambda n, args: fake_phx.write_tile_records(args, [0 if k in per_call[n - 1] else 64 for k in range(4)])


def test_progressive_by_tiles(monkeypatch, scene):
    fake = fake_phx.install(monkeypatch, phx_dev_film_accumulate=converged_from(99), phx_dev_film_tile_map=leaves_open((2, 1), ()))
    got = list(xpu.render_progressive(scene, SPP, 5, stop=STOP, tiles=dict(size=8, min_frames=1)))
    by_list = ["tiles_make_list", "start", "join", "film_accumulate"]
    assert fake.names() == ["make", "set_adaptive", "preprocess"] + by_list + ["film_tile_map"] + by_list + ["film_tile_map", "destroy"]
    a = fake.args("set_adaptive")[0][1]
    assert (a.threshold, a.floor, a.min_samples, a.step) == (0.0, 0.0, 4, 1)
    assert fake.tile_lists == [GRID, [GRID[1], GRID[2]]] and [a[1] for a in fake.args("tiles_make_list")] == [4, 2]
    for _, q, film, records, summary in fake.args("film_tile_map"):
        assert summary is None and film == got[0][0].ctypes.data and records and q.on_device == 0
        assert (q.tile_width, q.tile_height, q.tau, q.floor, q.xstride, q.m2_offset, q.samples_offset) == (8, 8, F(0.05), F(0.01), 8, 4, 7)
    assert [f[1].moments_channel for f in fake.args("start")] == [1, 1] and all(p[1].samples_offset_b == 7 for p in fake.args("film_accumulate"))
    assert [(g[1]["tiles"], g[1]["tiles_open"], g[1]["rendered_pixels"], g[2]) for g in got] == [(4, 4, 256, 1), (4, 2, 128, 2)]


@pytest.mark.parametrize("kwargs,match", [
    (dict(frames=0), "frames must be at least 1"),
    (dict(stop=dict(floor=0.1)), "stop needs a threshold"),
    (dict(tiles=dict(size=8)), "tiles= needs stop"),
    (dict(stop=STOP, tiles={}, despeckle={}), "despeckle= cannot be combined with tiles="),
    (dict(stop=STOP, tiles=dict(sizes=8)), r"tiles= does not know \['sizes'\]"),
    (dict(stop=STOP, tiles=dict(min_frames=0)), "min_frames must be at least 1"),
])
def test_progressive_refuses_at_the_first_next_and_before_any_call(monkeypatch, scene, kwargs, match):
    fake = fake_phx.install(monkeypatch)
    gen = xpu.render_progressive(scene, SPP, **{"frames": 2, **kwargs})
    assert fake.calls == []
    with pytest.raises(ValueError, match=match):
        next(gen)
    assert fake.calls == []


@pytest.mark.parametrize("kwargs,match", [
    (dict(denoise={}), "denoise needs moments=True"),
    (dict(progressive=dict(frames=2)), "progressive needs moments=True"),
    (dict(moments=True, progressive=dict(frames=2), callback_tiles=True), "no callback_tiles, rank or world"),
    (dict(moments=True, progressive=dict(frames=2), rank=1, world=2), "no callback_tiles, rank or world"),
    (dict(moments=True, progressive=dict(frames=0)), "frames must be at least 1"),
    (dict(moments=True, progressive=dict(frames=2, tiles={})), "tiles= needs stop"),
])
def test_render_refuses_before_any_call(monkeypatch, scene, kwargs, match):
    fake = fake_phx.install(monkeypatch)
    with pytest.raises(ValueError, match=match):
        xpu.render(scene, spp=SPP, **kwargs)
    assert fake.calls == []


# ---- render_camera_path ----------------------------------------------------------------------------------------------------------------------
def test_camera_path(monkeypatch, scene):
    fake = fake_phx.install(monkeypatch)
    cameras = [scene.camera, dataclasses.replace(scene.camera, fov=1.2), dataclasses.replace(scene.camera, fov=0.7)]
    got = list(xpu.render_camera_path(scene, cameras, SPP, frames_per_camera=2, seed=7, guide_samples=3, reproject=dict(max_history=24), history_clamp={},
                                      denoise=dict(guides=dict(plane=True, samples=7)), display={}))
    shown = ["denoise_guided", "film_display"]
    first, later = ["set_camera", "render_guides"], ["set_camera", "render_guides", "film_reproject"]
    assert fake.names() == (["make", "preprocess"] + first + (POOL + shown) * 2
                            + (later + FRAME + ["film_outlier_clamp", "film_accumulate"] + shown + POOL + shown) * 2 + ["destroy"])
    assert [(a[1].fov, a[1].film_width) for a in fake.args("set_camera")] == [(F(c.fov), W) for c in cameras]
    guides = fake.args("render_guides")
    assert [(g[1].sampler_seed, g[1].samples) for g in guides] == [(7, 3), (9, 3), (11, 3)]
    assert [f[1].sampler_seed for f in fake.args("start")] == [7, 8, 9, 10, 11, 12]
    frames, pools, moves, clamps, dens = (fake.args(n) for n in ("start", "film_accumulate", "film_reproject", "film_outlier_clamp", "denoise_guided"))
    assert all(f[1].normals_channel == 1 and f[1].moments_channel == 1 for f in frames)
    assert all(p[3] == f[1].host_film and p[1].samples_offset_b == 0 and p[1].xstride_b == 10 and p[4] is None for p, f in zip(pools, frames))
    # the accumulator of camera k's pools: the film render_camera_path made, then what each reprojection wrote
    assert pools[0][2] == pools[1][2] == moves[0][2] and [p[2] for p in pools[2:]] == [moves[0][5]] * 2 + [moves[1][5]] * 2 and moves[1][2] == moves[0][5]
    assert all(m[5] != m[2] for m in moves)
    for k, move in enumerate(moves):
        _, q, _, gf, gt, _, summary = move
        assert (gf, gt) == (guides[k][2], guides[k + 1][2]) and isinstance(summary, abi.ReprojectSummary)
        assert (q.max_history, getattr(q, "from").fov, q.to.fov, q.xstride_a, q.on_device) == (24, F(cameras[k].fov), F(cameras[k + 1].fov), 11, 0)
    for clamp, move, frame in zip(clamps, moves, (frames[2], frames[4])):
        q = clamp[1]
        assert q.flags == 0 and clamp[2] == clamp[4] == move[5] and clamp[3] == frame[1].host_film and clamp[5] is None
        assert (q.xstride_a, q.m2_offset_a, q.samples_offset_a, q.xstride_b) == (11, 7, 10, 10)
    for k, (den, pool, out) in enumerate(zip(dens, pools, got)):
        camera = k // 2
        assert den[3] == pool[2] and den[2].guides == guides[camera][2] and den[2].plane_scale == F(xpu.guide_plane_scale(cameras[camera]))
        assert den[2].flags == abi.GUIDE_DEMODULATE | abi.GUIDE_PLANE and (den[1].normals_offset, den[1].samples_offset, den[1].iterations) == (4, 10, 5)
        assert len(out) == 5 and out[1] is None and out[2] == k + 1 and out[0].ctypes.data == den[4] and out[4].shape == (H, W, 4)
        assert (out[3] is None) == (camera == 0) and (camera == 0 or set(out[3]) == {"pixels", "reused", "no_geometry", "disoccluded", "samples"})
    assert len({F(xpu.guide_plane_scale(c)) for c in cameras}) == 3


# ---- render_animation ------------------------------------------------------------------------------------------------------------------------
def test_animation(monkeypatch):
    fake = fake_phx.install(monkeypatch)
    path = [scenes.cornell(W, H) for _ in range(5)]
    got = list(xpu.render_animation(path, SPP, mode="refit", rebuild_every=2, denoise={}, display={}, seed=3))
    shown = ["denoise", "film_display"]
    assert fake.names() == ["make", "preprocess"] + FRAME + shown + (["update_geometry"] + FRAME + shown) * 4 + ["destroy"]
    assert [u[2].mode for u in fake.args("update_geometry")] == [abi.UPDATE_REFIT, abi.UPDATE_REBUILD, abi.UPDATE_REFIT, abi.UPDATE_REBUILD]
    assert [f[1].sampler_seed for f in fake.args("start")] == [3] * 5
    for frame, den, dis, out in zip(fake.args("start"), fake.args("denoise"), fake.args("film_display"), got):
        assert den[2] == frame[1].host_film and den[3] == dis[2] == out[0].ctypes.data and den[1].samples_offset == 0 and den[1].xstride == 10
        assert frame[1].normals_channel == 1 and frame[1].moments_channel == 1
    assert [(len(g), g[2], g[1] is None) for g in got] == [(4, 0, True)] + [(4, k, False) for k in (1, 2, 3, 4)]


# ---- render and render_on --------------------------------------------------------------------------------------------------------------------
def test_render_with_callback_tiles_an_add_tile_sink_and_guides(monkeypatch, scene):
    fake = fake_phx.install(monkeypatch)
    film, stats = xpu.render(scene, spp=SPP, seed=5, rank=1, world=2, callback_tiles=True, native_sink=False, moments=True,
                             adaptive=dict(threshold=0.1), denoise=dict(guides=dict(samples=2)))
    assert fake.names() == ["make", "set_adaptive", "preprocess", "tiles_make", "tiles_next", "start", "join", "render_guides", "denoise_guided",
                            "get_stats", "destroy"]
    (_, frame), = fake.args("start")
    assert frame.add_tile and not frame.host_film and not frame.tiles_user and frame.next_tile and (frame.sampler_seed, frame.moments_channel) == (5, 1)
    assert fake.args("tiles_make") == [(W, H, 32, 1, 2)]
    g = fake.args("render_guides")[0][1]
    assert (g.sampler_seed, g.samples) == (5, 2)
    den = fake.args("denoise_guided")[0]
    assert den[2].guides == fake.args("render_guides")[0][2] and den[2].flags == abi.GUIDE_DEMODULATE and den[1].samples_offset == 7 and den[4] == film.ctypes.data
    assert film.shape == (H, W, 8) and stats["tiles"] == 0


def test_render_progressive_through_render_is_the_direct_call(monkeypatch, scene):
    script = lambda: dict(phx_dev_film_accumulate=converged_from(99), phx_dev_film_tile_map=leaves_open((0, 3)))
    fake = fake_phx.install(monkeypatch, **script())
    film, summary = xpu.render(scene, spp=SPP, seed=5, moments=True, tile_size=16, samples_in_flight=3, progressive=dict(frames=2, stop=STOP, tiles=dict(size=8)))
    through = fake_phx.trace(fake)
    fake = fake_phx.install(monkeypatch, **script())
    direct = list(xpu.render_progressive(scene, SPP, 2, 5, STOP, tile_size=16, tiles=dict(size=8), samples_in_flight=3))
    assert through == fake_phx.trace(fake) and through[1] == [GRID, [GRID[0], GRID[3]]]
    assert [n for n, _ in through[0]].count("phx_dev_start") == 2 and through[0][0][1][0]["samples_in_flight"] == 3
    assert summary == direct[-1][1] and summary["tiles_open"] == 2 and film.shape == (H, W, 8)


def test_render_on_starts_every_device_then_joins_them(monkeypatch, scene):
    fake = fake_phx.install(monkeypatch)
    devs = [xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP)) for _ in range(2)]
    for d in devs:
        d.preprocess(scene)
    film, stats = xpu.render_on(devs, scene, seed=2)
    for d in devs:
        d.close()
    assert fake.names() == ["make", "make", "preprocess", "preprocess", "tiles_make", "start", "start", "join", "join", "get_stats", "get_stats",
                            "destroy", "destroy"]
    starts = fake.args("start")
    assert [s[0] for s in starts] == [j[0] for j in fake.args("join")] == [0x1000, 0x2000]
    assert starts[0][1].host_film == starts[1][1].host_film == film.ctypes.data and starts[0][1].tiles_user == starts[1][1].tiles_user == 0x3000
    assert len(stats) == 2


# ---- a device's lifetime ---------------------------------------------------------------------------------------------------------------------
def test_a_failing_call_still_destroys_the_device(monkeypatch, scene):
    fake = fake_phx.install(monkeypatch, phx_dev_film_accumulate=lambda n, args: 2 if n == 2 else None)
    gen = xpu.render_progressive(scene, SPP, 3)
    next(gen)
    with pytest.raises(xpu.DeviceError, match=r"phx_dev_film_accumulate failed \(2\)"):
        next(gen)
    assert makes_and_destroys(fake) == (1, 1) and fake.names()[-1] == "destroy"


@pytest.mark.parametrize("loop", ["progressive", "camera_path", "animation"])
def test_closing_the_generator_destroys_the_device(monkeypatch, scene, loop):
    fake = fake_phx.install(monkeypatch)
    gen = {"progressive": lambda: xpu.render_progressive(scene, SPP, 3), "camera_path": lambda: xpu.render_camera_path(scene, [scene.camera] * 2, SPP),
           "animation": lambda: xpu.render_animation([scene, scene], SPP)}[loop]()
    next(gen)
    assert makes_and_destroys(fake) == (1, 0)
    gen.close()
    assert makes_and_destroys(fake) == (1, 1) and fake.names()[-1] == "destroy"


def test_display_of_an_unknown_tone_destroys_its_device(monkeypatch):
    fake = fake_phx.install(monkeypatch)
    with pytest.raises(ValueError, match="tone must be one of"):
        xpu.display(np.zeros((4, 4, 4), F), tone="filmic")
    assert fake.names() == ["make", "destroy"]
    image = xpu.display(np.zeros((4, 4, 4), F))
    assert fake.names() == ["make", "destroy", "make", "film_display", "destroy"] and image.shape == (4, 4, 4)


# ---- HipDevice's film methods: host and device operands --------------------------------------------------------------------------------------
A, B, O, G = 0xa0000, 0xb0000, 0xc0000, 0xd0000  # device addresses (nothing reads them)


@pytest.fixture
def dev(monkeypatch):
    fake = fake_phx.install(monkeypatch)
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP))
    del fake.calls[:]
    yield d, fake
    d.close()


def test_denoise_operands(dev):
    d, fake = dev
    film, guides = np.zeros((H, W, 7), F), np.zeros((H, W, 8), F)
    out = d.denoise(film, SPP)
    assert d.denoise((H, W, 7), SPP, device_ptr=A) is None
    out_g = d.denoise(film, SPP, guides=guides, plane_scale=0.5)
    assert d.denoise((H, W, 7), SPP, device_ptr=A, guides=(H, W, 8), guides_ptr=G) is None
    assert fake.names() == ["denoise", "denoise", "denoise_guided", "denoise_guided"]
    (_, q, src, dst), (_, qd, srcd, dstd) = fake.args("denoise")
    assert (src, dst, q.on_device) == (film.ctypes.data, out.ctypes.data, 0) and src != dst and (srcd, dstd, qd.on_device) == (A, A, 1)
    (_, q, g, src, dst), (_, qd, gd, srcd, dstd) = fake.args("denoise_guided")
    assert (src, dst, q.on_device, g.guides) == (film.ctypes.data, out_g.ctypes.data, 0, guides.ctypes.data) and (srcd, dstd, qd.on_device, gd.guides) == (A, A, 1, G)
    del fake.calls[:]
    for kwargs, match in ((dict(guides=np.zeros((H, W + 1, 8), F)), "the guide film must be"), (dict(guides=guides, plane=True), "plane=True needs plane_scale"),
                          (dict(device_ptr=A, guides=guides), "needs device-resident guides"), (dict(guides=(H, W, 8), guides_ptr=G), "need a device-resident film")):
        with pytest.raises(ValueError, match=match):
            d.denoise(film, SPP, **kwargs)
    with pytest.raises(ValueError, match="floats per pixel"):
        d.denoise(np.zeros((H, W, 4), F), SPP)
    assert fake.calls == []


def test_accumulate_operands(dev):
    d, fake = dev
    acc, frame = xpu.accumulator(W, H), np.zeros((H, W, 7), F)
    got, summary = d.accumulate(acc, frame, SPP)
    assert got is acc and summary is None
    got, summary = d.accumulate(acc[:, :, ::-1][:, :, ::-1].astype(np.float64), frame, SPP, threshold=0.1)   # no float32 film: a copy is pooled
    assert got is not acc and got.dtype == F and summary == {"pixels": 0, "invalid": 0, "converged": 0, "samples": 0}
    assert d.accumulate((H, W, 8), (H, W, 7), SPP, device_ptrs=(A, B)) == (None, None)
    host, copied, device = fake.args("film_accumulate")
    assert (host[2], host[3], host[4], host[1].on_device) == (acc.ctypes.data, frame.ctypes.data, None, 0)
    assert copied[2] == got.ctypes.data and isinstance(copied[4], abi.AccumulateSummary) and copied[1].tau == F(0.1)
    assert (device[2], device[3], device[4], device[1].on_device) == (A, B, None, 1)
    del fake.calls[:]
    with pytest.raises(ValueError, match="the accumulator is"):
        d.accumulate(acc, np.zeros((H, W + 1, 7), F), SPP)
    assert fake.calls == []


def test_tile_map_operands(dev):
    d, fake = dev
    acc = xpu.accumulator(W, H)
    records, summary = d.tile_map(acc, 8, 0.1)
    assert len(records) == 4 and summary == dict.fromkeys(("pixels", "invalid", "converged", "samples", "tiles", "open"), 0)
    records, summary = d.tile_map((H, W, 8), (8, 5), device_ptr=A, summary=False)
    assert len(records) == 2 * 4 and summary is None
    host, device = fake.args("film_tile_map")
    assert (host[2], host[1].on_device, host[1].tile_width, host[1].tile_height) == (acc.ctypes.data, 0, 8, 8) and isinstance(host[4], abi.TileMapSummary)
    assert (device[2], device[3], device[4], device[1].on_device, device[1].tile_height) == (A, records.ctypes.data, None, 2, 5)
    del fake.calls[:]
    with pytest.raises(ValueError, match="an accumulator has 8 floats"):
        d.tile_map(np.zeros((H, W, 7), F))
    assert fake.calls == []


def test_reproject_operands(dev, scene):
    d, fake = dev
    acc, gf, gt, cam = xpu.accumulator(W, H, 4, True), np.zeros((H, W, 8), F), np.zeros((H, W, 8), F), scene.camera
    out, summary = d.reproject(acc, gf, gt, cam, cam)
    assert out.shape == acc.shape and out is not acc and set(summary) == {"pixels", "reused", "no_geometry", "disoccluded", "samples"}
    assert d.reproject((H, W, 11), (H, W, 8), (H, W, 8), cam, cam, summary=False, device_ptrs=(A, B, G, O)) == (None, None)
    host, device = fake.args("film_reproject")
    assert host[2:6] == (acc.ctypes.data, gf.ctypes.data, gt.ctypes.data, out.ctypes.data) and host[1].on_device == 0 and isinstance(host[6], abi.ReprojectSummary)
    assert device[2:7] == (A, B, G, O, None) and device[1].on_device == 1
    del fake.calls[:]
    with pytest.raises(ValueError, match="one stride"):
        d.reproject(acc, gf, np.zeros((H, W, 9), F), cam, cam)
    assert fake.calls == []


def test_clamp_outliers_operands(dev):
    d, fake = dev
    film, ref, out = np.zeros((H, W, 7), F), np.ones((H, W, 7), F), np.zeros((H, W, 7), F)
    assert d.clamp_outliers(film)[0] is film                                  # in place, against itself
    got, summary = d.clamp_outliers(film, ref, summary=False)                  # in place, against another film
    assert got is film and summary is None
    assert d.clamp_outliers(film, out=out)[0] is out                           # ref=None: film itself, though the result goes elsewhere
    assert d.clamp_outliers(film, out, out=out)[0] is out                      # ref is out
    assert d.clamp_outliers(film, film, out=out)[0] is out                     # ref is film
    assert d.clamp_outliers((H, W, 7), (H, W, 4), device_ptrs=(A, B, O))[0] is None
    calls = fake.args("film_outlier_clamp")
    f, r, o = film.ctypes.data, ref.ctypes.data, out.ctypes.data
    assert [c[2:5] for c in calls] == [(f, f, f), (f, r, f), (f, f, o), (f, o, o), (f, f, o), (A, B, O)]
    assert [c[1].on_device for c in calls] == [0, 0, 0, 0, 0, 1] and calls[1][5] is None and isinstance(calls[0][5], abi.OutlierClampSummary)
    assert calls[5][1].xstride_b == 4
    del fake.calls[:]
    for bad in (np.zeros((H, W, 8), F), np.zeros((H, W, 7), np.float64), out[:, ::2]):
        with pytest.raises(ValueError, match="out must be a writable C-contiguous float32 array of film's shape"):
            d.clamp_outliers(film, out=bad)
    with pytest.raises(ValueError, match="the film is 16 x 16 pixels, the reference film 15 x 16"):
        d.clamp_outliers(film, np.zeros((H, W - 1, 7), F))
    assert fake.calls == []


def test_display_operands(dev):
    d, fake = dev
    film = np.zeros((H, W, 4), F)
    image = d.display(film)
    preview, info = d.display((H, W, 4), device_ptr=A, summary=True)
    assert d.display((H, W, 4), device_ptr=A, image_on_host=False, image_ptr=O, image_pitch=128) is None
    host, device, resident = fake.args("film_display")
    assert (host[2], host[3], host[4], host[5], host[1].on_device, host[1].image_pitch) == (film.ctypes.data, image.ctypes.data, None, None, 0, 0)
    assert (device[2], device[3], device[1].on_device) == (A, preview.ctypes.data, 2) and isinstance(device[4], abi.DisplaySummary) and device[5]
    assert (resident[2], resident[3], resident[1].on_device, resident[1].image_pitch) == (A, O, 1, 128)
    assert info["pixels"] == 0 and info["histogram"].shape == (256,) and image.shape == preview.shape == (H, W, 4)
    del fake.calls[:]
    for kwargs, match in ((dict(device_ptr=A, image_on_host=False), "needs its address"), (dict(image_ptr=O), "image_ptr is a device address"),
                          (dict(device_ptr=A, image_ptr=O), "image_ptr is a device address"), (dict(exposure="manual"), 'a number or "auto"')):
        with pytest.raises(ValueError, match=match):
            d.display(film, **kwargs)
    assert fake.calls == []


def test_the_fake_answers_every_export():
    fake = fake_phx.FakePhx()
    assert all(callable(getattr(fake, name)) for name in abi.EXPORTS) and isinstance(fake.phx_tiles_next, abi.NEXT_TILE_FN)
    assert fake.phx_last_error() == b"" and fake.phx_dev_make(None) == 0x1000 and fake.phx_dev_join(0x1000) == abi.PHX_OK
    with pytest.raises(AttributeError):
        fake.phx_no_such_call
