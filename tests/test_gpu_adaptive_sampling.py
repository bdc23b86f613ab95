"""Adaptive sampling on the device (phx_dev_set_adaptive; the selection kernels of film_hooks.hip) against the float64 restatement of
tests/adaptive64.py, bit for bit: the selection alone through its parity hook on sizes around its 64-lane waves, its 256-row blocks and
the second level of its scan; whole frames against the restatement of the oracle's per-sample films (tests/test_adaptive_sampling.py
pins the frames and asserts that some of their pixels stop early and some do not), in every sink and pixel layout; off means off; the
refusals; two devices on one queue, two ranks through dist.reduce_film, and the plain-C host."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import adaptive64 as A
import frame_cases as FC
from conftest import ROOT, bits_equal
from phosphorus_mk2_amd import scenes
from test_adaptive_sampling import DEPTH, EARLY, F, MIN_SAMPLES, SEED, SETTINGS, SPP, STEP, check_condition, oracle_samples, restated

pytestmark = pytest.mark.gpu

PHX_OK, PHX_ERR_ARG, PHX_ERR_STATE = 0, 1, 4  # include/phx_xpu.h


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


def make_dev(xpu, scene=None, spp=SPP, flight=0, tpb=0, **kw):
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=spp, paths_per_sample=1, path_depth=DEPTH, samples_in_flight=flight, tiles_per_batch=tpb, **kw))
    if scene is not None:
        dev.preprocess(scene)
    return dev


def set_pinned(dev, which):
    tau, floor = SETTINGS[which]
    dev.set_adaptive(tau, floor, MIN_SAMPLES, STEP)


def frame(xpu, dev, scene, sink="native", components=4, normals=False, moments=True, adaptive=True, seed=SEED):
    """one frame into a sink prefilled with a sentinel -> (film (H, W, xstride), stats); sink: "add_tile", "native" or "device" """
    W, H = scene.camera.width, scene.camera.height
    film, tensor = None, None
    if sink == "device":
        xs = components + (3 if normals else 0) + (3 if moments else 0) + (1 if adaptive else 0)
        tensor = FC.DeviceFilm(xpu, (H, W, xs), FC.SENTINEL)
    else:
        film = xpu.Film(W, H, components, normals, moments, adaptive)
        film.data[:] = FC.SENTINEL
    try:
        dev.start(scene, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, device_film_ptr=tensor.ptr if tensor else None, native_sink=sink == "native",
                                        primary_components=components, normals=normals, moments=moments, adaptive=adaptive))
        dev.join()
        return (tensor.numpy() if tensor else film.data), dev.stats()
    finally:
        if tensor:
            tensor.free()


def counters(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms") and k != "device_bytes"}


def check_film(film, r, components, normals):
    """every channel of an adaptive frame against the restatement `r`, bit for bit"""
    off = components + (3 if normals else 0)
    assert film.shape == r["samples"].shape + (off + 4,)
    assert bits_equal(film[..., :3], r["primary"])
    if components == 4:
        assert (film[..., 3].view(np.uint32) == 0).all()  # the fourth component of "primary" is never written
    if normals:
        assert bits_equal(film[..., components:off], r["normals"])
    assert bits_equal(film[..., off:off + 3], r["m2"])
    assert bits_equal(film[..., off + 3], r["samples"])


# ---- 1. the selection through its hook -----------------------------------------------------------------------------------------------------------
TAU = 0.1
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 70000)
PATTERNS = ("all_stop", "none_stop", "alternating", "first_and_last", "specials", "decades")


def hook_rows(pattern, n, seed):
    """n rows of (primary rgb, m2 rgb, samples): which of them stop at TAU follows from the pattern whatever samples_done and the floor are,
    but for "specials" and "decades", where the restatement decides"""
    rng = np.random.default_rng(seed)
    acc = np.zeros((n, 7), F)
    f = (0.05 + rng.random((n, 3))).astype(F)
    noisy = (f.astype(np.float64) ** 2 * 1e4).astype(F)  # L >= 1e4 f^2 against b^2 = (0.1 (f + g))^2 <= 0.02 f^2 (g < 0.02 <= 0.4 f): never stops; m2 = 0 always does
    acc[:, :3] = f
    if pattern == "none_stop":
        acc[:, 3:6] = noisy
    elif pattern == "alternating":
        acc[1::2, 3:6] = noisy[1::2]
    elif pattern == "first_and_last":
        acc[[0, -1], 3:6] = noisy[[0, -1]]
    elif pattern == "specials":
        acc[:, 3:6] = (f * f * F(1e-3) * rng.random((n, 3))).astype(F)
        kind = rng.integers(0, 8, n)
        acc[kind == 0, 1] = np.nan; acc[kind == 1, 4] = np.nan
        acc[kind == 2, 0] = np.inf; acc[kind == 3, 5] = np.inf; acc[kind == 4, 2] = -np.inf
        acc[kind == 5, :6] = 0; acc[kind == 6, :3] = 0          # all zeros: stops; a black pixel with spread: does not without a floor
    elif pattern == "decades":
        f = (10.0 ** rng.uniform(-5, 5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
        acc[:, :3] = f
        acc[:, 3:6] = (f.astype(np.float64) ** 2 * 10.0 ** rng.uniform(-4, 0, (n, 3))).astype(F)
    acc[:, 6] = 77
    return acc


@pytest.fixture(scope="module")
def hook_dev(xpu):
    dev = make_dev(xpu)  # no scene: the selection reads none
    yield dev
    dev.close()


@pytest.mark.parametrize("n", SIZES)
def test_the_hook_is_the_restatement(hook_dev, n):
    saw = {"stop": 0, "go": 0}
    for p, pattern in enumerate(PATTERNS):
        for done in (2, 8, 31):
            for floor in (0.0, 0.02):
                for strided in (False, True):
                    if strided:  # every second row of a larger table, from row 1; the rows between would stop if they were decided
                        acc = hook_rows("all_stop", 2 * n + 3, 7 * n + p)
                        active = np.arange(1, 2 * n + 1, 2, dtype=np.uint32)
                        acc[active] = hook_rows(pattern, n, 1000 * n + 10 * p + done)
                    else:
                        acc, active = hook_rows(pattern, n, 1000 * n + 10 * p + done), None
                    got, surv = hook_dev.adaptive_select(acc, done, SPP, TAU, floor, 2, 1, active=active)
                    want, wsurv = A.select(acc, active, done, SPP, TAU, floor)
                    tag = (n, pattern, done, floor, strided)
                    assert surv.dtype == np.uint32 and np.array_equal(surv, wsurv), (tag, len(surv), len(wsurv))
                    assert bits_equal(got, want), (tag, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4])
                    rows = np.arange(n) if active is None else active
                    if pattern == "all_stop":
                        assert len(surv) == 0 and (got[rows, 6] == done).all()
                    if pattern == "none_stop":
                        assert np.array_equal(surv, rows) and bits_equal(got, acc)
                    if pattern == "alternating":
                        assert np.array_equal(surv, rows[1::2])
                    if pattern == "first_and_last":
                        assert np.array_equal(surv, np.unique(rows[[0, -1]]))
                    if strided:
                        rest = np.ones(len(acc), bool); rest[active] = False
                        assert bits_equal(got[rest], acc[rest])  # rows outside `active`: not decided, not touched
                    saw["stop"] += n - len(surv); saw["go"] += len(surv)
    assert saw["stop"] and saw["go"]


def test_the_hook_and_the_setting_check_their_arguments(xpu):
    sc = scenes.cornell(32, 32)
    dev = make_dev(xpu, sc, spp=8)
    lib, h, abi = dev._lib, dev._h, xpu.abi
    try:
        want, _ = frame(xpu, dev, sc, moments=True, adaptive=False)
        acc = hook_rows("decades", 4, 1); surv = np.zeros(4, np.uint32); n = C.c_uint32(99)
        fp, up = acc.ctypes.data_as(abi.f32p), lambda a: a.ctypes.data_as(abi.u32p)
        ok = abi.Adaptive(threshold=0.1, floor=0.0, min_samples=8, step=8)

        def select(active=None, num_active=4, num_rows=4, acc_p=fp, done=8, spp=32, a=ok, surv_p=up(surv), n_p=C.byref(n)):
            return lib.phx_dev_adaptive_select(h, num_active, None if active is None else up(active), num_rows, acc_p, done, spp, None if a is None else C.byref(a), surv_p, n_p)

        def still_renders():
            again, _ = frame(xpu, dev, sc, moments=True, adaptive=False)
            assert bits_equal(again, want)

        def bad(**kw):
            a = abi.Adaptive(threshold=0.1, floor=0.0, min_samples=8, step=8)
            for k, v in kw.items():
                if k == "reserved":
                    a.reserved[v] = 1
                else:
                    setattr(a, k, v)
            return a
        before = acc.copy()
        refusals = [dict(acc_p=None), dict(a=None), dict(surv_p=None), dict(n_p=None), dict(done=1), dict(done=32), dict(done=33),
                    dict(active=np.array([0, 1, 2, 4], np.uint32)), dict(active=np.array([0, 2, 1, 3], np.uint32)), dict(num_active=5),
                    dict(a=bad(reserved=0)), dict(a=bad(reserved=3)), dict(a=bad(threshold=float("nan"))), dict(a=bad(threshold=-1.0)),
                    dict(a=bad(floor=float("inf"))), dict(a=bad(floor=-0.5)), dict(a=bad(min_samples=1)), dict(a=bad(step=0))]
        for kw in refusals:
            assert select(**kw) == PHX_ERR_ARG, kw
            assert lib.phx_last_error() and bits_equal(acc, before)
            still_renders()
        assert select() == PHX_OK and n.value <= 4
        # the setting: the same ranges, the field named, and the previous setting stays in force
        dev.set_adaptive(1e9, 0.0, 2, 1)  # everything stops after two samples
        first, _ = frame(xpu, dev, sc)
        assert (first[..., 7] == 2).all()
        for field, a in (("reserved", bad(reserved=2)), ("threshold", bad(threshold=float("nan"))), ("threshold", bad(threshold=-1.0)),
                         ("floor", bad(floor=float("-inf"))), ("min_samples", bad(min_samples=1)), ("min_samples", bad(min_samples=0)), ("step", bad(step=0))):
            assert lib.phx_dev_set_adaptive(h, C.byref(a)) == PHX_ERR_ARG and field in lib.phx_last_error().decode(), field
            again, _ = frame(xpu, dev, sc)
            assert bits_equal(again, first)
        dev.set_adaptive(None)
        still_renders()
    finally:
        dev.close()


# ---- 2. frames against the restatement of the oracle's per-sample films ------------------------------------------------------------------------------
@pytest.mark.parametrize("flight", [0, 3])
@pytest.mark.parametrize("which", ["cornell", "general"])
def test_a_frame_is_the_restatement_of_the_oracles_samples(xpu, orc, which, flight):
    sc, y, nrm, ref, ost = oracle_samples(orc, which)
    r = restated(orc, which, flight)
    check_condition(r)
    dev = make_dev(xpu, sc, flight=flight)
    try:
        uniform, st_u = frame(xpu, dev, sc, normals=True, adaptive=False)
        set_pinned(dev, which)
        film, st = frame(xpu, dev, sc, normals=True)
    finally:
        dev.close()
    check_film(film, r, 4, True)
    assert st["shade_general"] == (which == "general") and st["paths_in_flight"] == 32 * 32 * (flight or 8)
    assert st["camera_samples"] == int(film[..., 10].astype(np.float64).sum()) == int(r["samples"].astype(np.float64).sum()) < st_u["camera_samples"] == 32 * 32 * SPP
    assert 0 < st["rays_closest"] < st_u["rays_closest"] and st["rays_shadow"] < st_u["rays_shadow"]
    # the pixels that took every sample hold the uniform frame's primary and normals (which are the oracle's); their m2 is the one of THIS
    # pass schedule (check_film above), which re-centres at other samples than the uniform frame's passes do
    never = r["stop_round"] < 0
    assert bits_equal(film[never][:, :7], uniform[never][:, :7]) and bits_equal(uniform[..., :3], ref[..., :3]) and st_u["rays_closest"] == ost["rays_closest"]
    assert not bits_equal(film[~never][:, :3], uniform[~never][:, :3])
    assert np.isfinite(xpu.film_variance(film, SPP, normals=True, adaptive=True)).all()


@pytest.fixture(scope="module")
def ragged(xpu, orc):
    """cornell at 40 x 24 under 32-pixel tiles (partial tiles, the narrow ones 8 wide), a floor above zero: the devices and the restatement"""
    sc, y, nrm, ref, ost = oracle_samples(orc, "cornell40")
    r = restated(orc, "cornell40")
    check_condition(r)
    devs = {tpb: make_dev(xpu, sc, tpb=tpb) for tpb in (0, 1)}
    for d in devs.values():
        set_pinned(d, "cornell40")
    yield sc, devs, r
    for d in devs.values():
        d.close()


@pytest.mark.parametrize("components,normals", [(3, False), (4, False), (3, True), (4, True)])
def test_every_sink_and_layout_holds_the_same_channels(xpu, ragged, components, normals):
    sc, devs, r = ragged
    total = int(r["samples"].astype(np.float64).sum())
    for tpb in (0, 1):
        for sink in ("add_tile", "native", "device"):
            film, st = frame(xpu, devs[tpb], sc, sink, components, normals)
            check_film(film, r, components, normals)
            assert st["camera_samples"] == total and st["tiles"] == 2, (sink, tpb)


# ---- 3. off means off ------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(xpu):
    sc = scenes.cornell(32, 32)
    dev = make_dev(xpu, sc)
    try:
        plain, st_plain = frame(xpu, dev, sc, normals=True, adaptive=False)
        set_pinned(dev, "cornell")
        on, _ = frame(xpu, dev, sc, normals=True)
        assert on.shape == (32, 32, 11) and (on[..., 10] < SPP).any()
        dev.set_adaptive(None)
        off, st_off = frame(xpu, dev, sc, normals=True, adaptive=False)
        assert off.shape == (32, 32, 10) and bits_equal(off, plain) and counters(st_off) == counters(st_plain)
        bare, _ = frame(xpu, dev, sc, moments=False, adaptive=False)  # and the frame without any of the channels
        assert bare.shape == (32, 32, 4) and bits_equal(bare, plain[..., :4])
        for ms in (SPP, SPP + 1):  # no decision before the last sample: the plain frame, and every pixel says spp
            dev.set_adaptive(1e9, 0.0, ms, STEP)
            late, st_late = frame(xpu, dev, sc, normals=True)
            assert bits_equal(late[..., :10], plain) and (late[..., 10] == SPP).all()
            assert all(st_late[k] == st_plain[k] for k in FC.RAY_KEYS) and st_late["paths_in_flight"] == st_plain["paths_in_flight"]
    finally:
        dev.close()


# ---- 4. call order and the required channel ------------------------------------------------------------------------------------------------------------
def test_the_setting_needs_the_m2_channel_and_an_idle_device(xpu):
    sc = scenes.cornell(32, 32)
    dev = make_dev(xpu, sc, spp=8)
    try:
        dev.set_adaptive(0.1, 0.0, 4, 2)
        want, _ = frame(xpu, dev, sc)
        with pytest.raises(xpu.DeviceError, match="moments_channel") as e:
            frame(xpu, dev, sc, moments=False, adaptive=False)
        assert f"({PHX_ERR_ARG})" in str(e.value)
        again, _ = frame(xpu, dev, sc)
        assert bits_equal(again, want) and (want[..., 7] < 8).any()
        # between start and join the setting cannot change
        film = xpu.Film(32, 32, 4, False, True, True)
        dev.start(sc, xpu.FrameState(SEED, xpu.Tiles.make(32, 32, 32), film, native_sink=True))
        a = xpu.abi.Adaptive(threshold=0.5, floor=0.0, min_samples=2, step=1)
        rc_set, rc_off = dev._lib.phx_dev_set_adaptive(dev._h, C.byref(a)), dev._lib.phx_dev_set_adaptive(dev._h, None)
        dev.join()
        assert rc_set == PHX_ERR_STATE and rc_off == PHX_ERR_STATE and bits_equal(film.data, want)
        third, _ = frame(xpu, dev, sc)
        assert bits_equal(third, want)  # the setting is the one from before
    finally:
        dev.close()


# ---- 5. devices and ranks ----------------------------------------------------------------------------------------------------------------------------
W2, H2 = 72, 40  # 6 tiles to share


def test_two_devices_on_one_queue_give_the_one_device_film(xpu):
    sc = scenes.cornell(W2, H2)
    devs = [make_dev(xpu, sc, tpb=1), make_dev(xpu, sc, tpb=1)]
    try:
        for d in devs:
            set_pinned(d, "cornell")
        one, st1 = xpu.render_on(devs[:1], sc, seed=SEED, moments=True, adaptive=True)
        one = one.copy()
        two, sts = xpu.render_on(devs, sc, seed=SEED, moments=True, adaptive=True)
    finally:
        for d in devs:
            d.close()
    assert one.shape == (H2, W2, 8) and bits_equal(one, two) and sum(st["tiles"] for st in sts) == 6
    n = one[..., 7]
    assert set(np.unique(n)) == set(EARLY) | {SPP} and sum(st["camera_samples"] for st in sts) == st1[0]["camera_samples"] == int(n.astype(np.float64).sum())


def _rank(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    import torch
    from phosphorus_mk2_amd import dist as pdist
    from phosphorus_mk2_amd import xpu
    pdist.init_process_group("gloo", rank, world)
    sc = scenes.cornell(W2, H2)
    dev = make_dev(xpu, sc, device_ordinal=0)
    set_pinned(dev, "cornell")
    film = xpu.Film(W2, H2, 4, False, True, True)  # zero-initialised
    dev.start(sc, xpu.FrameState(SEED, xpu.Tiles.make(W2, H2, 32, rank, world), film, native_sink=True)); dev.join()
    taken = dev.stats()["camera_samples"]
    dev.close()
    t = torch.from_numpy(film.data)
    pdist.reduce_film(t, dst=0)  # ranks own disjoint pixels: every channel, "samples" too, sums with zeros
    taken = pdist.sum_over_ranks(taken)
    if rank == 0:
        np.savez(out_path, film=t.numpy(), taken=taken)
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_through_reduce_film_give_the_one_device_film(xpu, tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "r0.npz")
    mp.start_processes(_rank, args=(2, 29500 + (os.getpid() % 2000), out), nprocs=2, join=True, start_method="spawn")
    got = np.load(out)
    sc = scenes.cornell(W2, H2)
    tau, floor = SETTINGS["cornell"]
    full, st = xpu.render(sc, spp=SPP, pps=1, depth=DEPTH, seed=SEED, native_sink=True, moments=True, adaptive=dict(threshold=tau, floor=floor, min_samples=MIN_SAMPLES, step=STEP))
    assert full.shape == (H2, W2, 8) and bits_equal(got["film"], full) and got["taken"] == st["camera_samples"] == full[..., 7].astype(np.float64).sum()
    assert (full[..., 7] < SPP).mean() > 0.1 and (full[..., 7] == SPP).mean() > 0.1


# ---- 6. the plain-C host -------------------------------------------------------------------------------------------------------------------------------
def test_the_c_example_prints_the_mean_samples_and_writes_h_w_4(xpu, tmp_path):
    import re
    import subprocess
    from test_gpu_parity import _room_scene
    exe = os.path.join(ROOT, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "examples")], check=True)
    out = str(tmp_path / "room.f32")
    r = subprocess.run([exe, out, "adaptive", "0.2", "host-bvh"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    film_c = np.fromfile(out, np.float32).reshape(96, 128, 4)
    film, st = xpu.render(_room_scene(), spp=8, pps=1, depth=5, seed=7, native_sink=True, bvh_builder="host", moments=True,
                          adaptive=dict(threshold=0.2, floor=0.0, min_samples=4, step=2))
    assert film.shape == (96, 128, 8) and bits_equal(film[..., :4], film_c) and film_c[..., :3].max() > 0.05
    mean = film[..., 7].astype(np.float64).mean()
    m = re.search(r"adaptive: mean samples per pixel ([0-9.]+) of 8 \(camera_samples (\d+)\)", r.stdout)
    assert m and abs(float(m.group(1)) - mean) <= 5e-5 and int(m.group(2)) == st["camera_samples"] == int(film[..., 7].astype(np.float64).sum())
    assert 4 <= mean < 8 and "error estimate:" in r.stdout
