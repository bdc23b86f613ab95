"""The tile map on the device (phx_dev_film_tile_map, csrc/tile_map.hip) against the float64 model of tests/tile_map64.py, bit for bit, records
and summary, `worst` compared as bits: film shapes around and below the tile, tile shapes from 4 x 4 to 256 x 256, pixel layouts through the
raw C call, host and device memory; the refusals and the call's state; frames over a tile list (phx_tiles_make_list) in every sink; the
frame films that carry "samples" without adaptive sampling; and render_progressive(tiles=) and the plain-C example against the chain of the
models."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import accumulate64 as ac
import frame_cases as FC
import tile_map64 as tm
from conftest import ROOT, bits_equal
from test_tile_map import LOOP_DEPTH, LOOP_FLOOR, LOOP_H, LOOP_SPP, LOOP_TAU, LOOP_TILE, LOOP_TILES_PER_FRAME, LOOP_W, OFFS_ACC, model_chain

pytestmark = pytest.mark.gpu

F = np.float32
PHX_OK, PHX_ERR_ARG, PHX_ERR_STATE = 0, 1, 4  # include/phx_xpu.h
TAU, FLOOR = 0.1, 0.0  # floor 0: a black colour with m2 > 0 has den == 0 and r = +inf (the layouts run with a floor)
SHAPES = [(1, 1), (1, 9), (9, 1), (37, 29), (65, 67), (300, 260)]  # (width, height)
TILES = [(4, 4), (8, 8), (16, 4), (32, 32), (64, 64)]             # (tile_width, tile_height)


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


@pytest.fixture(scope="module")
def dev(xpu):
    """a device without a scene: the call needs none"""
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=LOOP_SPP, paths_per_sample=1, path_depth=LOOP_DEPTH))
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def film_of(width, height, xstride=8, m2_offset=4, samples_offset=7):
    """-> the synthetic film of this shape and layout, read-only and shared"""
    film, at = tm.synthetic_film((height, width), xstride, m2_offset, samples_offset)
    film.setflags(write=False)
    return film, at


@functools.lru_cache(maxsize=None)
def want_of(width, height, tw, th, xstride=8, m2_offset=4, samples_offset=7, tau=TAU, floor=FLOOR):
    records, summary = tm.tile_map(film_of(width, height, xstride, m2_offset, samples_offset)[0], m2_offset, samples_offset, tw, th, tau, floor)
    records.setflags(write=False)
    return records, summary


def check(records, summary, want, what):
    want_records, want_summary = want
    assert records.dtype == tm.RECORD and records.shape == want_records.shape, what
    if records.tobytes() != want_records.tobytes():
        for k, (g, w) in enumerate(zip(records, want_records)):
            assert g.tobytes() == w.tobytes(), f"{what}: record {k} is {g}, the model's {w}"
    assert summary == want_summary, what


@pytest.mark.parametrize("tw,th", TILES, ids=[f"{a}x{b}" for a, b in TILES])
@pytest.mark.parametrize("width,height", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_device_is_the_model(dev, width, height, tw, th):
    """host film, host records (on_device = 0), the accumulator's own layout of 8 floats"""
    film, at = film_of(width, height)
    records, summary = dev.tile_map(film, (tw, th), TAU, FLOOR)
    check(records, summary, want_of(width, height, tw, th), f"{width} x {height} in tiles of {tw} x {th}")
    if width * height >= 32:
        assert summary["invalid"] == 7 and 0 < summary["converged"] < summary["pixels"] - 7 and np.isposinf(records["worst"]).any()


def test_a_thread_owns_many_pixels_and_every_edge_tile_is_ragged(dev):
    """300 x 260 in tiles of 256 x 256: four workgroups of 256 x 256, 44 x 256, 256 x 4 and 44 x 4 pixels, 256 pixels a thread in the first"""
    film, _ = film_of(300, 260)
    records, summary = dev.tile_map(film, 256, TAU, FLOOR)
    check(records, summary, want_of(300, 260, 256, 256), "300 x 260 in tiles of 256")
    assert [(int(r["w"]), int(r["h"])) for r in records] == [(256, 256), (44, 256), (256, 4), (44, 4)]


def test_more_workgroups_than_summary_slots(dev):
    """65 x 67 at tile 8: 81 workgroups on 64 summary slots, 17 of them added to twice"""
    slots = int(re.search(r"PHX_SUMMARY_SLOTS = (\d+)", open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "kernels.h")).read()).group(1))
    want = want_of(65, 67, 8, 8)
    assert len(want[0]) == 81 > slots == 64
    for tau, floor in ((0.0, 0.0), (1e9, 1.0)):
        records, summary = dev.tile_map(film_of(65, 67)[0], 8, tau, floor)
        check(records, summary, want_of(65, 67, 8, 8, tau=tau, floor=floor), f"81 workgroups at tau {tau}")
    assert summary["open"] < summary["tiles"]


def raw_call(xpu, dev, film_ptr, records_ptr, shape, m2_offset, samples_offset, tw, th, on_device, tau=TAU, floor=FLOOR, summary=True):
    H, W, xs = shape
    q = xpu.abi.TileMap(width=W, height=H, xstride=xs, m2_offset=m2_offset, samples_offset=samples_offset, tile_width=tw, tile_height=th,
                        on_device=on_device, tau=tau, floor=floor)
    s = xpu.abi.TileMapSummary()
    rc = dev._lib.phx_dev_film_tile_map(dev._h, C.byref(q), film_ptr, records_ptr, C.byref(s) if summary else None)
    return rc, {k: int(getattr(s, k)) for k, _ in s._fields_}


LAYOUTS = [(7, 3, 6), (7, 4, 3), (8, 4, 7), (11, 7, 3), (11, 4, 10), (24, 20, 12), (24, 3, 23)]  # (xstride, m2_offset, samples_offset)


@pytest.mark.parametrize("xstride,m2_offset,samples_offset", LAYOUTS, ids=[f"{a}-{b}-{c}" for a, b, c in LAYOUTS])
def test_layouts_through_the_c_call(xpu, dev, xstride, m2_offset, samples_offset):
    """xstrides 7, 8, 11 and 24, the channels in either order, foreign floats (NaNs among them) in every float the rule does not read"""
    film, _ = film_of(65, 67, xstride, m2_offset, samples_offset)
    records = np.zeros(9 * 17, tm.RECORD)
    rc, summary = raw_call(xpu, dev, film.ctypes.data, records.ctypes.data, film.shape, m2_offset, samples_offset, 8, 4, 0, 0.3, 0.001)
    assert rc == PHX_OK, dev._lib.phx_last_error()
    check(records, summary, want_of(65, 67, 8, 4, xstride, m2_offset, samples_offset, 0.3, 0.001), f"xstride {xstride}, m2 at {m2_offset}, samples at {samples_offset}")


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("on_device", [1, 2])
def test_device_resident_films(xpu, dev, on_device, misaligned):
    """the film in device memory, once 4 bytes past a 16-byte boundary; the records in device memory (1) or on the host (2).  The film is read only."""
    film, _ = film_of(65, 67, 11, 7, 10)  # xpu.accumulator's layout with normals
    want = want_of(65, 67, 16, 4, 11, 7, 10)
    pad = 1 if misaligned else 0
    df = FC.DeviceFilm(xpu, (film.size + pad,), np.concatenate([np.full(pad, FC.SENTINEL, F), film.ravel()]))
    dr = FC.DeviceFilm(xpu, (len(want[0]) * 10 + 2,), FC.SENTINEL)  # a word of sentinel on either side of the records (8-byte aligned behind two words)
    try:
        if on_device == 1:
            rc, summary = raw_call(xpu, dev, df.ptr + 4 * pad, dr.ptr + 8, film.shape, 7, 10, 16, 4, 1)
            assert rc == PHX_OK, dev._lib.phx_last_error()
            words = dr.numpy()
            assert (words[:2] == F(FC.SENTINEL)).all()  # nothing before the records
            records = np.frombuffer(words[2:].tobytes(), tm.RECORD)
        else:
            records, summary = dev.tile_map(film.shape, (16, 4), TAU, FLOOR, 4, True, device_ptr=df.ptr + 4 * pad)
        check(records, summary, want, f"on_device {on_device}, misaligned {misaligned}")
        assert df.numpy()[pad:].tobytes() == film.tobytes() and (df.numpy()[:pad] == F(FC.SENTINEL)).all()
    finally:
        df.free(); dr.free()


def test_without_a_summary_the_records_are_the_same(dev):
    records, summary = dev.tile_map(film_of(37, 29)[0], 8, TAU, FLOOR, summary=False)
    assert summary is None
    assert records.tobytes() == want_of(37, 29, 8, 8)[0].tobytes()


# ---- refusals and state ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_records_untouched_and_the_device_usable(xpu, dev):
    film, _ = film_of(37, 29)
    lib = dev._lib
    records = np.zeros(20, tm.RECORD)
    records["invalid"] = 77
    before = records.tobytes()
    s = xpu.abi.TileMapSummary(pixels=7)
    for kw, field in ((dict(tile_width=3), "tile_width"), (dict(tile_height=1025), "tile_height"), (dict(tau=-1.0), "tau"), (dict(floor=float("nan")), "floor"),
                      (dict(on_device=3), "on_device"), (dict(samples_offset=5), "samples_offset"), (dict(m2_offset=0), "m2_offset"), (dict(xstride=25), "xstride")):
        q = xpu.tile_map_settings(film.shape, 8, TAU, FLOOR)
        for k, v in kw.items():
            setattr(q, k, v)
        assert lib.phx_dev_film_tile_map(dev._h, C.byref(q), film.ctypes.data, records.ctypes.data, C.byref(s)) == PHX_ERR_ARG
        assert lib.phx_last_error().decode() == f"tile_map: {field} is outside its range (phx_tile_map)"
    q = xpu.tile_map_settings(film.shape, 8, TAU, FLOOR)
    q.reserved[2] = 1
    assert lib.phx_dev_film_tile_map(dev._h, C.byref(q), film.ctypes.data, records.ctypes.data, C.byref(s)) == PHX_ERR_ARG and "reserved" in lib.phx_last_error().decode()
    q = xpu.tile_map_settings(film.shape, 8, TAU, FLOOR)
    for a, r, field in ((None, records.ctypes.data, "acc"), (film.ctypes.data, None, "records"), (film.ctypes.data, film.ctypes.data + 64, "records")):
        assert lib.phx_dev_film_tile_map(dev._h, C.byref(q), a, r, C.byref(s)) == PHX_ERR_ARG and field in lib.phx_last_error().decode()
    assert lib.phx_dev_film_tile_map(dev._h, None, film.ctypes.data, records.ctypes.data, None) == PHX_ERR_ARG
    assert lib.phx_dev_tile_map_times(dev._h, None) == PHX_ERR_ARG
    with pytest.raises(ValueError, match="xpu.accumulator"):
        dev.tile_map(film[..., :7], 8, TAU, FLOOR)
    assert records.tobytes() == before and (s.pixels, s.invalid, s.converged, s.samples, s.tiles, s.open) == (7, 0, 0, 0, 0, 0)
    bytes_before = dev.stats()["device_bytes"]
    got, summary = dev.tile_map(film, 8, TAU, FLOOR)
    check(got, summary, want_of(37, 29, 8, 8), "after the refusals")
    assert dev.stats()["device_bytes"] == bytes_before
    t = dev.tile_map_times()
    assert set(t) == {"kernel", "call"} and 0 < t["kernel"] <= t["call"]
    # a refused call behind a successful one leaves the times and the caller's current device alone
    current = FC.current_hip_device(xpu)
    q.on_device = 3
    assert lib.phx_dev_film_tile_map(dev._h, C.byref(q), film.ctypes.data, records.ctypes.data, None) == PHX_ERR_ARG
    assert dev.tile_map_times() == t and FC.current_hip_device(xpu) == current


SPP, DEPTH, W, H = LOOP_SPP, LOOP_DEPTH, LOOP_W, LOOP_H


@pytest.fixture(scope="module")
def scene():
    return FC.SCENES["cornell"](W, H)


@pytest.fixture(scope="module")
def frames(xpu, scene):
    """the device's uniform films of seeds 1, 2, 3 with the m2 channel (H, W, 7), read-only"""
    out = {seed: xpu.render(scene, seed=seed, spp=SPP, depth=DEPTH, moments=True)[0] for seed in (1, 2, 3)}
    for f in out.values():
        f.setflags(write=False)
    assert out[1].shape == (H, W, 7) and not bits_equal(out[1], out[2])
    return out


@pytest.fixture(scope="module")
def marking(xpu, scene):
    """a device with the scene whose frames only mark samples = spp: set_adaptive(0, 0, max(spp, 2), 1)"""
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=DEPTH))
    d.set_adaptive(threshold=0.0, floor=0.0, min_samples=max(SPP, 2), step=1)
    d.preprocess(scene)
    yield d
    d.close()


def test_a_call_between_start_and_join_is_refused_and_disturbs_nothing(xpu, scene, frames):
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=DEPTH))
    acc0 = ac.accumulate(xpu.accumulator(W, H), frames[1], OFFS_ACC, (0, 4, 0), SPP)
    tensor = FC.DeviceFilm(xpu, (H, W, 7), FC.SENTINEL)
    try:
        d.preprocess(scene)

        def start():
            d.start(scene, xpu.FrameState(2, xpu.Tiles.make(W, H, 32), None, device_film_ptr=tensor.ptr, primary_components=4, normals=False, moments=True))
        start()
        records = np.zeros(20, tm.RECORD)
        rc, _ = raw_call(xpu, d, acc0.ctypes.data, records.ctypes.data, acc0.shape, 4, 7, 8, 8, 0)
        msg = d._lib.phx_last_error().decode()
        d.join()
        assert rc == PHX_ERR_STATE and "frame" in msg and not records.tobytes().strip(b"\0")
        assert bits_equal(tensor.numpy(), frames[2])  # the frame then completes as ever
        before = d.stats()["device_bytes"]
        got, summary = d.tile_map(acc0, 8, LOOP_TAU, LOOP_FLOOR)
        want = tm.tile_map(acc0, 4, 7, 8, 8, LOOP_TAU, LOOP_FLOOR)
        check(got, summary, want, "behind the frame")
        assert d.stats()["device_bytes"] == before and summary["open"] == LOOP_TILES_PER_FRAME[1]
        tensor.fill(FC.SENTINEL)
        start(); d.join()
        assert bits_equal(tensor.numpy(), frames[2]) and d.stats()["device_bytes"] == before  # and a later frame is what it was
    finally:
        tensor.free()
        d.close()


# ---- frames that carry "samples", and frames over a tile list -----------------------------------------------------------------------------
def marked_frame(xpu, d, scene, seed, tiles, sink):
    """one frame of the marking device over `tiles` (None: the whole film) into a zeroed film of 8 floats a pixel -> (H, W, 8)"""
    queue = xpu.Tiles.make(W, H, 32) if tiles is None else xpu.Tiles.from_list(tiles, W, H)
    if sink == "device":
        tensor = FC.DeviceFilm(xpu, (H, W, 8), 0.0)
        try:
            d.start(scene, xpu.FrameState(seed, queue, None, device_film_ptr=tensor.ptr, primary_components=4, normals=False, moments=True, adaptive=True))
            d.join()
            return tensor.numpy()
        finally:
            tensor.free()
    film = xpu.Film(W, H, 4, False, True, True)
    d.start(scene, xpu.FrameState(seed, queue, film, native_sink=sink == "native"))
    d.join()
    return film.data


def test_a_marking_frame_is_the_uniform_frame_with_samples(xpu, scene, frames, marking):
    """set_adaptive(0, 0, max(spp, 2), 1): primary, m2 (and with normals=True the normals) are the plain moments=True frame's bit for bit, and
    samples == spp everywhere"""
    got = marked_frame(xpu, marking, scene, 2, None, "native")
    assert bits_equal(got[..., 0:7], frames[2]) and (got[..., 7] == SPP).all()
    plain = xpu.render(scene, seed=3, spp=SPP, depth=DEPTH, moments=True, normals=True)[0]
    film = xpu.Film(W, H, 4, True, True, True)
    marking.start(scene, xpu.FrameState(3, xpu.Tiles.make(W, H, 32), film, native_sink=True))
    marking.join()
    assert plain.shape == (H, W, 10) and bits_equal(film.data[..., 0:10], plain) and (film.data[..., 10] == SPP).all() and plain[..., 4:7].any()


@pytest.mark.parametrize("sink", ["native", "device", "add_tile"])
def test_a_frame_over_a_tile_list_is_the_full_frame_inside_and_zero_outside(xpu, scene, frames, marking, sink):
    tiles = tm.grid(W, H, 8, 8)
    assert len(tiles) == 20
    subset = [tiles[k] for k in (13, 2, 19)]  # in the caller's order; 19 is the ragged corner
    got = marked_frame(xpu, marking, scene, 1, subset, sink)
    inside = np.zeros((H, W), bool)
    for x, y, w, h in subset:
        inside[y:y + h, x:x + w] = True
    assert bits_equal(got[inside][:, 0:7], frames[1][inside]) and (got[inside][:, 7] == SPP).all()
    assert not got[~inside].view(np.uint32).any()  # all zero, samples included
    assert marking.stats()["tiles"] == 3


def test_an_empty_tile_list_renders_nothing(xpu, scene, marking):
    got = marked_frame(xpu, marking, scene, 1, [], "native")
    assert not got.view(np.uint32).any() and marking.stats()["tiles"] == 0 and marking.stats()["camera_samples"] == 0


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
def test_render_progressive_by_tiles_is_the_chain_of_the_models(xpu, scene, frames):
    """every yield equals: render, tile_map64, filter, pool, with the model's tile lists; rendered_pixels falls; closed tiles keep their bits"""
    chain = model_chain([frames[s] for s in (1, 2, 3)], LOOP_TAU, LOOP_FLOOR)
    assert [len(t) for t, _ in chain] == LOOP_TILES_PER_FRAME
    got = [(film.copy(), summary, done) for film, summary, done in
           xpu.render_progressive(scene, SPP, 3, seed=1, depth=DEPTH, stop=dict(threshold=LOOP_TAU, floor=LOOP_FLOOR, coverage=1.0), tiles=dict(size=LOOP_TILE))]
    assert [g[2] for g in got] == [1, 2, 3]
    for k, (film, summary, _) in enumerate(got):
        tiles, acc = chain[k]
        assert bits_equal(film, acc), f"after frame {k + 1}"
        want = ac.summary(acc, OFFS_ACC, LOOP_TAU, LOOP_FLOOR)
        want.update(tiles=20, tiles_open=len(tiles), rendered_pixels=sum(w * h for _, _, w, h in tiles))
        assert summary == want, f"after frame {k + 1}"
    rendered = [g[1]["rendered_pixels"] for g in got]
    assert rendered[0] == W * H > rendered[1] > rendered[2] > 0
    for k in (1, 2):
        closed = np.ones((H, W), bool)
        for x, y, w, h in chain[k][0]:
            closed[y:y + h, x:x + w] = False
        assert closed.any() and got[k][0][closed].tobytes() == got[k - 1][0][closed].tobytes()
        assert not bits_equal(got[k][0][~closed], got[k - 1][0][~closed])
    # render(progressive=dict(tiles=)) passes it through
    film, summary = xpu.render(scene, seed=1, spp=SPP, depth=DEPTH, moments=True,
                               progressive=dict(frames=2, stop=dict(threshold=LOOP_TAU, floor=LOOP_FLOOR, coverage=1.0), tiles=dict(size=LOOP_TILE)))
    assert bits_equal(film, got[1][0]) and summary == got[1][1]


def test_render_progressive_ends_when_no_tile_is_open(xpu, scene, frames):
    """tiles close at half their pixels while stop asks for every pixel: the loop ends because no tile is open, before `frames` and before
    stop's coverage is met; and with min_frames = 2 the second frame renders every tile whatever the map says"""
    stop = dict(threshold=LOOP_TAU, floor=LOOP_FLOOR, coverage=1.0)
    chain = model_chain([frames[s] for s in (1, 2, 3)], LOOP_TAU, LOOP_FLOOR, coverage=0.5)
    assert 1 <= len(chain) < 3
    got = [(film.copy(), summary, done) for film, summary, done in xpu.render_progressive(scene, SPP, 3, seed=1, depth=DEPTH, stop=stop, tiles=dict(size=LOOP_TILE, coverage=0.5))]
    assert len(got) == len(chain) and all(bits_equal(g[0], c[1]) for g, c in zip(got, chain))
    last = got[-1][1]
    assert last["converged"] < last["pixels"] - last["invalid"]  # stop's own rule did not end it
    chain2 = model_chain([frames[s] for s in (1, 2, 3)], LOOP_TAU, LOOP_FLOOR, min_frames=2)
    got2 = [(film.copy(), summary) for film, summary, _ in xpu.render_progressive(scene, SPP, 3, seed=1, depth=DEPTH, stop=stop, tiles=dict(size=LOOP_TILE, min_frames=2))]
    assert [s["tiles_open"] for _, s in got2] == [len(t) for t, _ in chain2] and got2[1][1]["tiles_open"] == 20 > got2[2][1]["tiles_open"]
    assert all(bits_equal(g[0], c[1]) for g, c in zip(got2, chain2))


def test_without_tiles_the_loop_is_what_it_was(xpu, scene, frames):
    """the three-frame chain of tests/test_gpu_accumulate.py, with a stop: films, summaries and the yield's shape"""
    got = [(film.copy(), summary, done) for film, summary, done in xpu.render_progressive(scene, SPP, 3, seed=1, depth=DEPTH, stop=dict(threshold=LOOP_TAU, floor=LOOP_FLOOR, coverage=1.0))]
    acc = np.zeros((H, W, 8), F)
    for k, seed in enumerate((1, 2, 3)):
        acc = ac.accumulate(acc, frames[seed], OFFS_ACC, (0, 4, 0), SPP)
        assert bits_equal(got[k][0], acc) and got[k][1] == ac.summary(acc, OFFS_ACC, LOOP_TAU, LOOP_FLOOR) and got[k][2] == k + 1
        assert set(got[k][1]) == {"pixels", "invalid", "converged", "samples"}


def test_despeckle_with_tiles_raises(xpu, scene):
    with pytest.raises(ValueError, match="despeckle"):
        next(xpu.render_progressive(scene, SPP, 2, stop=dict(threshold=0.1), tiles=dict(size=8), despeckle={}))


def test_the_c_example_renders_the_open_tiles(xpu, tmp_path):
    """examples/render_room.c `progressive 3 tiles TAU`: the three `tiles:` lines of the model chain on the room's own frames (seeds 7, 8, 9,
    8 spp, tiles of 32 on 128 x 96: 12 tiles), and the accumulator on file"""
    from test_gpu_parity import _room_scene
    exe = os.path.join(ROOT, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "examples")], check=True)
    tau, floor = 0.7, 0.01  # the example's floor; at this tau the room's frames render 12, 11 and 8 of its 12 tiles
    out = str(tmp_path / "room.f32")
    r = subprocess.run([exe, out, "host-bvh", "progressive", "3", "tiles", str(tau)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [tuple(int(v) for v in l) for l in re.findall(r"tiles: frame (\d+) open (\d+) of (\d+) rendered (\d+) pixels", r.stdout)]
    full = [xpu.render(_room_scene(), spp=8, pps=1, depth=5, seed=seed, native_sink=True, bvh_builder="host", moments=True)[0] for seed in (7, 8, 9)]
    acc = np.zeros((96, 128, 8), F)
    want = []
    for k, frame in enumerate(full):
        tiles = tm.grid(128, 96, 32, 32) if k == 0 else tm.open_tiles(tm.tile_map(acc, 4, 7, 32, 32, tau, floor)[0])
        want.append((k + 1, len(tiles), 12, sum(w * h for _, _, w, h in tiles)))
        if not tiles:
            break
        film = np.zeros((96, 128, 8), F)
        for x, y, w, h in tiles:
            film[y:y + h, x:x + w, 0:7] = frame[y:y + h, x:x + w]
            film[y:y + h, x:x + w, 7] = 8
        acc = ac.accumulate(acc, film, OFFS_ACC, OFFS_ACC)
    assert lines == want and len(lines) == 3 and 12 == want[0][1] > want[1][1] > want[2][1] > 0
    assert bits_equal(np.fromfile(out, F).reshape(96, 128, 4), acc[..., :4])
    assert len(re.findall(r"progressive: frame \d+ seed \d+", r.stdout)) == sum(1 for w in want if w[1])
