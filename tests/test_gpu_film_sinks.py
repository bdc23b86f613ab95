"""The frame's four film sinks against each other and the oracle: the add_tile callback, the host film filled from C (native_sink), the
device-resident film that bench.py times (k_scatter_film, the sink-less branch of render_batch) and the last two together.  Every
comparison is bit equality over the whole pixel -- alpha and the normals channel included -- and every sink starts from a sentinel, so
a pixel that was not written, written at another place or added to instead of replaced shows."""
import numpy as np
import pytest

import frame_cases as F
from phosphorus_mk2_amd import scenes

pytestmark = pytest.mark.gpu

SPP, DEPTH = 5, 4
SCENES = {
    "soup": lambda: scenes.soup(3000, width=72, height=40),   # 3 x 2 tiles, ragged on both axes
    "cornell": lambda: scenes.cornell(48, 40),                # 2 x 2 tiles
    "blobs": lambda: scenes.smooth_blobs(width=40, height=24),  # interpolated normals and silhouettes against the walls
}
LAYOUTS = [(3, False), (4, False), (3, True), (4, True)]  # xstride 3, 4, 6, 7


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


@pytest.fixture(scope="module")
def rig(xpu, orc):
    """one device object per (scene, samples in flight, tiles per batch), one scene object per scene, one oracle film per (scene, seed)"""
    made, devs, refs, hosts = {}, {}, {}, {}

    class Rig:
        def scene(self, name):
            if name not in made:
                made[name] = SCENES[name]()
            return made[name]

        def dev(self, name, flight=0, tpb=0, fresh=None):
            key = (name, flight, tpb, fresh)
            if key not in devs:
                d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=DEPTH, samples_in_flight=flight, tiles_per_batch=tpb))
                d.preprocess(self.scene(name))
                devs[key] = d
            return devs[key]

        def oracle(self, name, seed):
            if (name, seed) not in refs:
                orc.set_tie_rule(1)
                try:
                    refs[(name, seed)] = orc.Oracle(self.scene(name), spp=SPP, pps=1, depth=DEPTH).render(rng=orc.RNG_COUNTER, seed=seed, threads=4, normals=True)
                finally:
                    orc.set_tie_rule(0)
            return refs[(name, seed)]

        def host(self, name, seed, components=4, normals=False):
            """the whole frame through add_tile on the plain device: (film, stats), compared with the oracle once"""
            key = (name, seed, components, normals)
            if key not in hosts:
                film, _, st = F.frame(xpu, self.dev(name), self.scene(name), seed, host="add_tile", components=components, normals=normals)
                ref, ost, nref = self.oracle(name, seed)
                assert F.same_bits(film[..., :3], ref[..., :3])
                assert all(st[k] == ost[k] for k in F.RAY_KEYS) and ost["rays_shadow"] > 0
                if normals:
                    assert F.same_bits(film[..., components:], nref) and nref.any()
                film.setflags(write=False)
                hosts[key] = (film, st)
            return hosts[key]
    yield Rig()
    for d in devs.values():
        d.close()


def counts(st):
    return {k: st[k] for k in F.RAY_KEYS + ("tiles",)}


@pytest.mark.parametrize("components,normals", LAYOUTS)
@pytest.mark.parametrize("name", list(SCENES))
def test_four_sinks_agree_and_the_callback_film_is_the_oracles(xpu, rig, name, components, normals):
    sc, dev = rig.scene(name), rig.dev(name)
    a, st_a = rig.host(name, 7, components, normals)
    assert a.shape[-1] == components + (3 if normals else 0)
    if components == 4:
        assert (a[..., 3] == 0).all()  # film_t<>::add_tile leaves alpha alone: the render buffer's zero
    b, _, st_b = F.frame(xpu, dev, sc, 7, host="native", components=components, normals=normals)
    _, c, st_c = F.frame(xpu, dev, sc, 7, device=True, components=components, normals=normals)
    d_host, d_dev, st_d = F.frame(xpu, dev, sc, 7, host="native", device=True, components=components, normals=normals)
    for other in (b, c, d_host, d_dev):
        assert F.same_bits(a, other)
    for st in (st_b, st_c, st_d):
        assert counts(st) == counts(st_a)


@pytest.mark.parametrize("flight,tpb", [(0, 0), (1, 0), (2, 0), (0, 1), (0, 3), (2, 1)])
@pytest.mark.parametrize("name,components,normals", [("soup", 4, False), ("cornell", 3, True), ("blobs", 4, True)])
def test_a_rank_of_two_writes_its_tiles_alone_into_the_device_film(xpu, rig, name, components, normals, flight, tpb):
    """several passes (5 samples, 1 or 2 in flight) and several batches (1 or 3 tiles each: one scatter per batch)"""
    sc, dev = rig.scene(name), rig.dev(name, flight, tpb)
    W, H = sc.camera.width, sc.camera.height
    full, st_full = rig.host(name, 7, components, normals)
    covers, total = [], dict.fromkeys(F.RAY_KEYS + ("tiles",), 0)
    for r in (0, 1):
        tiles = F.default_tiles(xpu, W, H, r, 2)
        covers.append(F.paint(tiles, W, H))
        _, film, st = F.frame(xpu, dev, sc, 7, device=True, components=components, normals=normals, rank=r, world=2)
        F.check_cover(film, full, covers[-1])
        assert st["tiles"] == len(tiles) > 0
        for k in total:
            total[k] += st[k]
    assert (covers[0] + covers[1] == 1).all()  # disjoint and complete
    assert total == counts(st_full)
    # the two ranks' frames into ONE film: the full frame
    both = F.DeviceFilm(xpu, (H, W, full.shape[-1]), F.SENTINEL)
    for r in (0, 1):
        _, film, _ = F.frame(xpu, dev, sc, 7, tensor=both, components=components, normals=normals, rank=r, world=2)
    both.free()
    assert F.same_bits(film, full)
    # and the whole frame at once on this device
    _, film, st = F.frame(xpu, dev, sc, 7, device=True, components=components, normals=normals)
    assert F.same_bits(film, full) and counts(st) == counts(st_full)


@pytest.mark.parametrize("name,components,normals", [("soup", 4, False), ("blobs", 3, True)])
def test_a_frame_replaces_the_device_film(xpu, rig, name, components, normals):
    sc, dev = rig.scene(name), rig.dev(name)
    W, H = sc.camera.width, sc.camera.height
    first, _ = rig.host(name, 7, components, normals)
    second, _ = rig.host(name, 8, components, normals)
    assert not F.same_bits(first, second)
    t = F.DeviceFilm(xpu, (H, W, first.shape[-1]), F.SENTINEL)
    for want, seed in ((first, 7), (second, 8), (first, 7), (first, 7)):
        _, film, _ = F.frame(xpu, dev, sc, seed, tensor=t, components=components, normals=normals)
        assert F.same_bits(film, want)
    t.free()


def test_two_devices_with_frames_in_flight_over_two_device_films(xpu, rig):
    """bench.py's second protocol: two device objects on one scene, frame i on device i & 1 into film i % 2, started before frame i - 1 is
    joined"""
    name = "soup"
    sc = rig.scene(name)
    W, H = sc.camera.width, sc.camera.height
    want, st_want = rig.host(name, 7)
    devs = [rig.dev(name, fresh=0), rig.dev(name, fresh=1)]
    tiles = [xpu.Tiles.make(W, H, 32), xpu.Tiles.make(W, H, 32)]
    films = [F.DeviceFilm(xpu, (H, W, 4), F.SENTINEL) for _ in range(2)]
    seen = []

    def go(i):
        tiles[i & 1].reset()
        devs[i & 1].start(sc, xpu.FrameState(7, tiles[i & 1], None, device_film_ptr=films[i % 2].ptr))

    def done(i):
        devs[i & 1].join()
        seen.append((i, films[i % 2].numpy(), devs[i & 1].stats()))
        films[i % 2].fill(F.SENTINEL)  # the next frame into this film starts from the sentinel again

    n = 4
    for i in range(n):
        if i >= 2:
            done(i - 2)
        go(i)
    for i in range(n - 2, n):
        done(i)
    assert [i for i, _, _ in seen] == list(range(n))
    for i, film, st in seen:
        assert F.same_bits(film, want), i
        assert counts(st) == counts(st_want), i


def test_torch_tensor_as_the_device_film(xpu, rig, tmp_path):
    """bench.py's own arrangement, which needs a process of its own (torch first, see frame_cases.DeviceFilm): a torch tensor prefilled
    with the sentinel as FrameState's device_film_ptr, without a layout (bench.py's call) and with the normals channel"""
    import os
    import subprocess
    import sys
    out = str(tmp_path / "films.npz")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_film_child.py")
    r = subprocess.run([sys.executable, child, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    sc = rig.scene("soup")
    W, H = sc.camera.width, sc.camera.height
    for key, seed, normals in (("seed7", 7, False), ("seed8", 8, False), ("seed7_normals", 7, True)):
        want, st = rig.host("soup", seed, 4, normals)
        assert F.same_bits(got[key], want), key
        assert list(got[key + "_rays"]) == list(counts(st).values()), key
    want, _ = rig.host("soup", 7)
    tiles = F.default_tiles(xpu, W, H, 0, 2)
    F.check_cover(got["rank0"], want, F.paint(tiles, W, H))
    assert got["rank0_rays"][-1] == len(tiles)
