"""The per-pixel error estimate on the device (phx_frame.moments_channel, k_film_moments) against the float64 restatement of
tests/test_film_moments.py, bit for bit: the kernel alone through its parity hook on shapes around its 64 x 16 tile, whole frames against
the oracle's per-sample films, every sink and pixel layout, two devices on one queue, the refused word, and the estimate itself against
the closed-form variance of scenes.sun_floor."""
import numpy as np
import pytest

import frame_cases as FC
from conftest import bits_equal
from phosphorus_mk2_amd import scenes
from test_film_moments import D, DEPTH, F, SEED, SPP, cornell_samples, general_samples, moments_of, moments_pass, oracle_samples, radiance_to_y

pytestmark = pytest.mark.gpu

PHX_OK, PHX_ERR_ARG = 0, 1  # include/phx_xpu.h


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


def frame(xpu, dev, scene, sink="native", components=4, normals=False, moments=True, seed=SEED, tile_size=32):
    """one frame into a sink prefilled with a sentinel -> (film (H, W, xstride), stats); sink: "add_tile", "native" or "device" """
    W, H = scene.camera.width, scene.camera.height
    film, tensor = None, None
    if sink == "device":
        xs = components + (3 if normals else 0) + (3 if moments else 0)
        tensor = FC.DeviceFilm(xpu, (H, W, xs), FC.SENTINEL)
    else:
        film = xpu.Film(W, H, components, normals, moments)
        film.data[:] = FC.SENTINEL
    try:
        dev.start(scene, xpu.FrameState(seed, xpu.Tiles.make(W, H, tile_size), film, device_film_ptr=tensor.ptr if tensor else None,
                                        native_sink=sink == "native", primary_components=components, normals=normals, moments=moments))
        dev.join()
        return (tensor.numpy() if tensor else film.data), dev.stats()
    finally:
        if tensor:
            tensor.free()


def counters(st):
    """every counter of phx_stats: not the times, and not device_bytes (the memory the object holds: the batch buffer grows by the channel)"""
    return {k: v for k, v in st.items() if not k.endswith("_ms") and k != "device_bytes"}


# ---- 1. the kernel through its hook ------------------------------------------------------------------------------------------------------------
NS = (1, 2, 15, 16, 17, 33)


def hook_radiance(P, S, seed, constant):
    """(P, S, 4): random over ten decades with zeros, the fourth float (which the film never reads) not zero; pixel `constant` has one value"""
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.uniform(-5, 5, (P, S, 4))).astype(F)
    x[rng.random((P, S, 4)) < 0.1] = 0
    x[..., 3] = 7.0
    if constant is not None:
        x[constant, :, :3] = [0.375, 2.0, 1e-3]
    return x


def run_chain(dev, x, passes, inv):
    """the hook pass after pass on one acc -> [acc after each call]"""
    acc, s0, out = np.zeros((x.shape[0], 6), F), 0, []
    for ns in passes:
        acc = dev.film_moments(x[:, s0:s0 + ns], acc, s0, inv)
        out.append(acc)
        s0 += ns
    return out


def model_chain(x, passes, inv):
    y = radiance_to_y(x[..., :3], inv)
    f, m2, s0, out = np.zeros((x.shape[0], 3), F), np.zeros((x.shape[0], 3), F), 0, []
    for ns in passes:
        f, m2 = moments_pass(f, m2, y[:, s0:s0 + ns], s0)
        out.append(np.concatenate([f, m2], axis=1))
        s0 += ns
    return out


@pytest.fixture(scope="module")
def hook_dev(xpu):
    dev = make_dev(xpu)  # no scene: the film stage reads none
    yield dev
    dev.close()


@pytest.mark.parametrize("pps", [1, 16])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_the_hook_is_the_restatement(hook_dev, P, pps):
    """chains of three calls on one acc: (ns, 5, ns) has samples_done 0, ns, ns + 5 and (5, ns, ns) has 0, 5, 5 + ns, for every ns"""
    for ns in NS:
        for chain, passes in enumerate([(ns, 5, ns), (5, ns, ns)]):
            S = sum(passes)
            inv = F(1.0) / F(S * pps)
            constant = min(1, P - 1) if (P > 1 or chain == 0) else None
            x = hook_radiance(P, S, 1000 * P + 10 * ns + chain, constant)
            got, want = run_chain(hook_dev, x, passes, inv), model_chain(x, passes, inv)
            for k, (g, w) in enumerate(zip(got, want)):
                assert bits_equal(g, w), (P, pps, ns, passes, k, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:4])
            assert (got[-1][:, 3:] > 0).sum() >= (P - 1) * 3 and np.isfinite(got[-1]).all()
            if constant is not None:
                assert (got[0][constant, 3:].view(np.uint32) == 0).all()  # all samples equal, one pass: +0.0 exactly
                if ns == 1 and chain == 0:
                    assert (got[0][:, 3:].view(np.uint32) == 0).all()     # one sample: +0.0 everywhere
            if P >= 63 and ns in (16, 17):
                # one NaN and one infinite sample, in later passes of the chain: their pixels' m2 is not finite from there on, in that colour;
                # every other value is the clean run's
                bad = x.copy()
                pn, pi = 5, P - 2
                bad[pn, passes[0] + 1, 1] = np.nan
                bad[pi, S - 1, 2] = np.inf
                dirty = run_chain(hook_dev, bad, passes, inv)
                assert bits_equal(dirty[0], got[0])
                for k in (1, 2):
                    same = np.ones((P, 6), bool)
                    same[pn, [1, 4]] = False
                    assert not np.isfinite(dirty[k][pn, 4]) and not np.isfinite(dirty[k][pn, 1])
                    if k == 2:
                        same[pi, [2, 5]] = False
                        assert not np.isfinite(dirty[k][pi, 5]) and np.isposinf(dirty[k][pi, 2])
                    assert np.array_equal(dirty[k].view(np.uint32)[same], got[k].view(np.uint32)[same])


def test_the_hook_checks_its_arguments(xpu, hook_dev):
    lib, h = hook_dev._lib, hook_dev._h
    acc = np.zeros((2, 6), F); x = np.ones((2, 3, 4), F)
    fp = lambda a: a.ctypes.data_as(xpu.abi.f32p)
    assert lib.phx_dev_film_moments(h, 2, 3, 0, 1.0, None, fp(acc)) == PHX_ERR_ARG
    assert lib.phx_dev_film_moments(h, 2, 3, 0, 1.0, fp(x), None) == PHX_ERR_ARG
    assert lib.phx_dev_film_moments(h, 1 << 16, 1 << 15, 0, 1.0, fp(x), fp(acc)) == PHX_ERR_ARG  # 2^31 samples: refused before anything is read
    assert lib.phx_dev_film_moments(h, 0, 3, 0, 1.0, None, None) == PHX_OK and not acc.any()
    assert bits_equal(hook_dev.film_moments(x, acc, 0, 0.5), np.array([[1.5, 1.5, 1.5, 0, 0, 0]] * 2, F))


# ---- 2. frames against the oracle's per-sample films ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flight,passes", [(0, (8,)), (3, (3, 3, 2))])
@pytest.mark.parametrize("which", ["cornell", "general"])
def test_a_frame_is_the_restatement_of_the_oracles_samples(xpu, orc, which, flight, passes):
    sc, y, ref, ost = cornell_samples(orc) if which == "cornell" else general_samples(orc)
    f, m2 = moments_of(y, passes)
    fin = np.isfinite(y).all((2, 3))
    assert fin.mean() > 0.99 and (m2[fin] > 0).any(-1).mean() >= 0.1  # the condition: at least one pixel in ten has m2 > 0
    dev = make_dev(xpu, sc, flight=flight)
    try:
        on, st_on = frame(xpu, dev, sc)
        off, st_off = frame(xpu, dev, sc, moments=False)
    finally:
        dev.close()
    assert on.shape == (32, 32, 7) and off.shape == (32, 32, 4)
    assert st_on["paths_in_flight"] == 32 * 32 * passes[0] and st_on["shade_general"] == (which == "general")
    assert bits_equal(on[..., :4], off) and counters(st_on) == counters(st_off)
    assert all(st_on[k] == ost[k] for k in FC.RAY_KEYS)
    assert bits_equal(on[..., :3][fin], ref[..., :3][fin]) and bits_equal(f[fin], ref[..., :3][fin])
    assert bits_equal(on[..., 4:][fin], m2[fin])
    assert (~np.isfinite(on[..., 4:][~fin])).any(-1).all()


def test_one_sample_per_pixel_is_all_zero(xpu):
    sc = scenes.cornell(32, 32)
    dev = make_dev(xpu, sc, spp=1)
    try:
        on, st = frame(xpu, dev, sc)
    finally:
        dev.close()
    assert on[..., :3].any() and np.isfinite(on).all() and st["camera_samples"] == 1024
    assert (on[..., 4:].view(np.uint32) == 0).all()


# ---- 4. sinks and shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(xpu, orc):
    """cornell at 40 x 24 under 32-pixel tiles (partial tiles, the narrow ones 8 wide: what the oracle renders too): the devices, the
    channel by the restatement and the films without the channel, per layout"""
    sc = scenes.cornell(40, 24)
    y, ref, ost = oracle_samples(orc, sc)
    _, m2 = moments_of(y)
    assert np.isfinite(y).all() and (m2 > 0).any(-1).mean() >= 0.1
    devs = {tpb: make_dev(xpu, sc, tpb=tpb) for tpb in (0, 1)}
    plain = {}

    def without(components, normals):
        if (components, normals) not in plain:
            plain[(components, normals)] = frame(xpu, devs[0], sc, "add_tile", components, normals, moments=False)
        return plain[(components, normals)]
    yield sc, devs, m2, ref, ost, without
    for d in devs.values():
        d.close()


@pytest.mark.parametrize("components,normals", [(3, False), (4, False), (3, True), (4, True)])
def test_every_sink_and_layout_holds_the_same_channel(xpu, ragged, components, normals):
    sc, devs, m2, ref, ost, without = ragged
    off = components + (3 if normals else 0)
    base, st_base = without(components, normals)
    assert base.shape == (24, 40, off) and bits_equal(base[..., :3], ref[..., :3])
    if normals:
        assert base[..., components:].any()
    for tpb in (0, 1):
        for sink in ("add_tile", "native", "device"):
            film, st = frame(xpu, devs[tpb], sc, sink, components, normals)
            assert film.shape == (24, 40, off + 3), (sink, tpb)
            assert bits_equal(film[..., :off], base), (sink, tpb)       # primary, alpha and normals: the frame without the channel
            assert bits_equal(film[..., off:], m2), (sink, tpb)         # the channel, at its offset, the same floats everywhere
            assert all(st[k] == ost[k] == st_base[k] for k in FC.RAY_KEYS) and st["tiles"] == 2 == st_base["tiles"]


# ---- 5. two devices on one queue ----------------------------------------------------------------------------------------------------------------
def test_two_devices_on_one_queue_give_the_one_device_film(xpu):
    sc = scenes.cornell(72, 40)  # 6 tiles to share, one per batch: a device that took them all at once would leave the other none
    devs = [make_dev(xpu, sc, tpb=1), make_dev(xpu, sc, tpb=1)]
    try:
        one, _ = xpu.render_on(devs[:1], sc, seed=SEED, moments=True)
        one = one.copy()
        two, sts = xpu.render_on(devs, sc, seed=SEED, normals=False, moments=True)
        plain, _ = xpu.render_on(devs[:1], sc, seed=SEED)
    finally:
        for d in devs:
            d.close()
    assert one.shape == (40, 72, 7) and bits_equal(one, two) and bits_equal(one[..., :4], plain)
    assert (one[..., 4:] > 0).any(-1).mean() >= 0.1 and sum(st["tiles"] for st in sts) == 6


# ---- 6. the refused word ------------------------------------------------------------------------------------------------------------------------
def test_any_other_word_is_refused_and_the_device_stays_usable(xpu):
    sc = scenes.cornell(32, 32)
    dev = make_dev(xpu, sc)
    try:
        want, _ = frame(xpu, dev, sc)
        for word in (2, 0xffffffff):
            with pytest.raises(xpu.DeviceError, match="moments_channel") as e:
                frame(xpu, dev, sc, moments=word)
            assert f"({PHX_ERR_ARG})" in str(e.value)
            again, _ = frame(xpu, dev, sc)
            assert bits_equal(again, want)
    finally:
        dev.close()


# ---- 7. the estimate is right -------------------------------------------------------------------------------------------------------------------
def test_the_estimate_is_the_closed_form_variance_on_sun_floor(xpu):
    """scenes.sun_floor under environment sampling: every pixel draws from the same one-sample distribution, whose variance var_nee the float64
    model of tests/test_gpu_environment_sampling.py gives in closed form.  Each of the 1024 pixels estimates it by S^2 m2 / (S - 1); their mean
    must lie within 4 standard errors (taken from their own spread) of the model, and that standard error must be below 5 % of var_nee."""
    from test_environment_sampling import EnvTable
    from test_gpu_environment_sampling import AREA_POWER_ENV, sun_floor_model
    S = 256
    sc = scenes.sun_floor()
    film, st = xpu.render(sc, spp=S, pps=1, depth=2, seed=SEED, moments=True, **AREA_POWER_ENV)
    plain, st_plain = xpu.render(sc, spp=S, pps=1, depth=2, seed=SEED, **AREA_POWER_ENV)
    assert film.shape == (32, 32, 7) and bits_equal(film[..., :4], plain) and counters(st) == counters(st_plain)
    _, var_nee, _ = sun_floor_model(EnvTable(sc), sc.textures[0].texels)
    est = (xpu.film_variance(film, S) * S).reshape(-1, 3)  # S^2 m2 / (S - 1): the film's variance is S x the variance of y = x / S
    mean, se = est.mean(0), est.std(0, ddof=1) / np.sqrt(len(est))
    print(f"one-sample variance: model {var_nee}, mean of {len(est)} estimates {mean}, standard error {se} ({se / var_nee} of the model), z {(mean - var_nee) / se}")
    assert len(est) == 1024 and np.isfinite(est).all()
    assert (se < 0.05 * var_nee).all()
    assert (np.abs(mean - var_nee) < 4 * se).all()


# ---- the plain-C host ------------------------------------------------------------------------------------------------------------------------
def test_the_c_example_prints_the_estimate_and_writes_the_same_film(xpu, tmp_path):
    """examples/render_room.c with the keyword error-estimate (anywhere behind the film's name): the file is still H x W x 4 and the same floats,
    and the printed mean relative standard error is the one film_variance gives for the room through the Python mirror"""
    import os
    import re
    import subprocess
    from conftest import ROOT
    from test_gpu_parity import _room_scene
    exe = os.path.join(ROOT, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "examples")], check=True)
    films = []
    for args in (["host-bvh"], ["error-estimate", "host-bvh"]):
        out = str(tmp_path / f"room{len(films)}.f32")
        r = subprocess.run([exe, out] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        films.append(np.fromfile(out, np.float32).reshape(96, 128, 4))
        assert ("error estimate:" in r.stdout) == (len(films) == 2)
    assert bits_equal(films[0], films[1]) and films[0][..., :3].max() > 0.05
    film, _ = xpu.render(_room_scene(), spp=8, pps=1, depth=5, seed=7, native_sink=True, bvh_builder="host", moments=True)
    assert bits_equal(film[..., :4], films[0])
    v, var = film[..., :3].astype(D), xpu.film_variance(film, 8)
    want = (np.sqrt(var[v > 0]) / v[v > 0]).mean()
    m = re.search(r"mean relative standard error ([0-9.]+) over (\d+) lit values", r.stdout)
    assert m and int(m.group(2)) == (v > 0).sum() and abs(float(m.group(1)) - want) <= 1e-4 and want > 0.01
