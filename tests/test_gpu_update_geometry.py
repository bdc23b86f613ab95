"""Geometry updates on the device (phx_dev_update_geometry).

  identity    update_geometry(the same scene) leaves bvh_pool() byte for byte what preprocess made, the grid included
  model       after each motion of tests/test_bvh_refit.py the pool equals tests/refit_model.py byte for byte, on device-built and host-built trees
  film        a frame after an update equals, bit for bit, the frame of a device freshly preprocessed with the moved scene: film, normals and
              every ray counter, under refit and under rebuild, and again after the update back (the original film); device_bytes is
              unchanged by a refit, equals the fresh device's after a rebuild, and is the original amount after the update back
  example     examples/render_room.c `animate K` prints an update line per frame and writes the fresh film of the last position
  refusals    leave the next frame the old scene's; an update while a frame runs is PHX_ERR_STATE and the frame completes
  animation   xpu.render_animation yields the fresh-preprocess film of every scene
  switch      a preprocess of another scene after a rebuild, and a refit after that, render what a fresh device renders: the steps preprocess
              and an update share (scene_commit.cpp) leave nothing of the scene before
  refused     a rebuild refused while committing (the fault-injection twin) leaves the device without a scene until a preprocess succeeds;
              one whose device build fails recoverably under the auto builder falls back to the host builder and renders the fresh film

A differing pixel is a finding to trace to its ray (scripts/pixel_*_probe.py), never a tolerance."""
import numpy as np
import pytest

import bvh_model as M
import refit_model as R
from conftest import bits_equal, tri_abc
from test_bvh_refit import CASES, MOTIONS, check_refitted, moved
from test_gpu_bvh_builder import _case, scene_of

pytestmark = pytest.mark.gpu

F = np.float32
W_, H_, SPP = 48, 32, 8
COUNTERS = ("camera_samples", "rays_closest", "rays_shadow", "rays_masked")


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


def make(xpu, **options):
    return xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=5, **options))


def frame(xpu, dev, sc, seed=3):
    """one frame with normals -> (film (H, W, 7) f32, the ray counters)"""
    W, H = sc.camera.width, sc.camera.height
    film = xpu.Film(W, H, 4, True)
    dev.start(sc, xpu.FrameState(seed, xpu.Tiles.make(W, H, 16), film, native_sink=True))
    dev.join()
    st = dev.stats()
    return film.data.copy(), {k: st[k] for k in COUNTERS}


# ---- identity and the model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["device", "host"])
def tree_dev(xpu, request):
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, bvh_builder=request.param))
    yield d, request.param
    d.close()


@pytest.mark.parametrize("name", CASES)
def test_refit_is_the_builder_and_the_model(tree_dev, name):
    """identity first, then every motion in turn, each refit starting from the pool the last one left (the refit reads topology alone)"""
    dev, builder = tree_dev
    sc, abc, material = _case(name)
    dev.preprocess(sc)
    st = dev.stats()
    assert st["bvh_built_on_device"] == (1 if builder == "device" else 0)
    counts = (st["bvh_nodes"], st["triangles"], st["bvh_depth"])
    pool, glo, gcell = dev.bvh_pool()
    bytes_before = st["device_bytes"]
    for motion in MOTIONS:
        new = moved(abc, motion, seed=len(abc))
        summary = dev.update_geometry(scene_of(new)[0], "refit")
        got, hlo, hcell = dev.bvh_pool()
        if motion == "identity":
            assert np.array_equal(got, pool) and bits_equal(hlo, glo) and bits_equal(hcell, gcell), "the identity refit changed the builder's pool"
        want, mlo, mcell = R.refit(pool, glo, gcell, new)
        assert bits_equal(hlo, mlo) and bits_equal(hcell, mcell), f"{motion}: the grid of the new bounds"
        diff = np.nonzero((got != want).any(1))[0]
        assert len(diff) == 0, f"{motion}: {len(diff)} of {len(pool)} pool elements differ from the model, the first at {diff[:4].tolist()}"
        check_refitted(got, hlo, hcell, new, material, counts)
        boxes = M.leaf_boxes(new)
        assert summary["mode"] == 0 and summary["triangles"] == len(abc) and summary["nodes"] == counts[0] and summary["levels"] == counts[2]
        assert bits_equal(np.array(summary["bounds"], F), np.concatenate([boxes.glo, boxes.ghi])) and bits_equal(F(summary["delta"]), F(boxes.delta))
        assert dev.stats()["device_bytes"] == bytes_before
        pool, glo, gcell = got, hlo, hcell
    t = dev.update_geometry_times()
    assert set(t) == {"flatten", "upload", "device", "call"} and t["call"] >= t["device"] > 0.0


# ---- the film -----------------------------------------------------------------------------------------------------------------------------------
def rigid(angle, t, scale=(1.0, 1.0, 1.0)):
    c, s = np.cos(angle), np.sin(angle)
    m = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) * np.asarray(scale)[None, :]
    return np.concatenate([m, np.asarray(t, np.float64)[:, None]], 1).astype(F)


def smooth_showroom():
    """showroom(2000) with smooth spheres: per-vertex normals from each sphere's centre"""
    from phosphorus_mk2_amd import scenes
    sc = scenes.showroom(2000, width=W_, height=H_)
    for m in sc.meshes[6:]:
        n = m.vertices - m.vertices.mean(0, keepdims=True)
        m.normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
        m.smooth = np.ones(len(m.faces), np.uint8)
    return sc


def textured_room():
    """a floor with an image on its lobe, a lamp with an image on its emission (both with UVs) and a grey block between them"""
    from phosphorus_mk2_amd import abi, scenes
    rng = np.random.default_rng(5)
    quad = lambda pts, mat, uv: scenes.MeshDesc(vertices=np.array(pts, F), faces=np.array([[0, 1, 2], [0, 2, 3]], np.uint32), sets=[(mat, np.array([0, 1], np.uint32))],
                                                uvs=np.array(uv, F))
    uv = [(0, 0), (1, 0), (1, 1), (0, 1)]
    floor = quad([(-2, -1, -1), (2, -1, -1), (2, -1, -5), (-2, -1, -5)], 0, [(0, 0), (3, 0), (3, 3), (0, 3)])
    lamp = quad([(-0.6, 1.2, -2.4), (-0.6, 1.2, -3.6), (0.6, 1.2, -3.6), (0.6, 1.2, -2.4)], 1, uv)
    c = rng.uniform(-0.5, 0.5, (40, 1, 3)) + np.array([0.0, -0.3, -3.0])
    block = scenes.MeshDesc(vertices=(c + rng.uniform(-0.25, 0.25, (40, 3, 3))).astype(F).reshape(-1, 3), faces=np.arange(120, dtype=np.uint32).reshape(-1, 3),
                            sets=[(2, np.arange(40, dtype=np.uint32))])
    mats = [scenes.MaterialDesc(lobes=[scenes.LobeDesc(abi.LOBE_DIFFUSE, (0.8, 0.8, 0.8), texture=1)]),
            scenes.MaterialDesc([], (6.0, 5.0, 4.0), True, emission_uv_texture=2), scenes.diffuse(0.6, 0.6, 0.6)]
    tex = [scenes.TextureDesc(rng.uniform(0.1, 1.0, (8, 8, 3)).astype(F)), scenes.TextureDesc(rng.uniform(0.2, 1.0, (4, 4, 3)).astype(F))]
    return scenes.SceneDesc([floor, lamp, block], mats, scenes.CameraDesc(W_, H_), name="textured_room", textures=tex)


def sky_room():
    """the Cornell box without its ceiling under an image sky: mesh lights and the environment are both sampled"""
    from phosphorus_mk2_amd import abi, scenes
    sc = scenes.cornell(W_, H_)
    del sc.meshes[1]
    sc.materials.append(scenes.MaterialDesc(lobes=[], emission=(1.0, 1.0, 1.0), emission_texture=1, emission_mapping=abi.ENV_LATLONG_Y_UP))
    sc.environment_material = len(sc.materials) - 1
    sc.textures = [scenes.TextureDesc(scenes.sun_and_sky(sun=50.0), abi.TEX_CLOSEST, abi.WRAP_PERIODIC, abi.WRAP_CLAMP)]
    return sc


def _film_case(name):
    """-> (scene, moved scene, options)"""
    from phosphorus_mk2_amd import scenes
    lamp_move = rigid(0.4, (0.3, -0.15, 0.2), scale=(1.8, 1.0, 0.6))  # the lamp turns, moves and is stretched: another area, another pdf
    if name == "cornell":
        sc = scenes.cornell(W_, H_)
        return sc, scenes.transformed(sc, {2: rigid(0.0, (0.0, 0.0, 0.4)), 5: rigid(0.3, (0.2, -0.1, 0.0))}), {}
    if name == "showroom_smooth":
        sc = smooth_showroom()
        return sc, scenes.transformed(sc, {k: rigid(0.5, (0.1, 0.05, -0.1)) for k in range(6, 18)}), {}
    if name == "glass_blobs":
        sc = scenes.glass_blobs(W_, H_)
        return sc, scenes.wobbled(sc, 0.02, seed=1), {}
    if name == "textured":
        sc = textured_room()
        return sc, scenes.transformed(sc, {1: lamp_move, 2: rigid(0.7, (0.2, 0.1, 0.3))}), {}
    if name.startswith("lamp_"):
        options = {"lamp_reference": {}, "lamp_area": dict(light_sampling="area"), "lamp_power": dict(light_sampling="area", light_selection="power"),
                   "lamp_env": dict(light_sampling="area", light_selection="power", environment_sampling=True)}[name]
        sc = sky_room() if name == "lamp_env" else scenes.cornell(W_, H_)
        return sc, scenes.transformed(sc, {len(sc.meshes) - 1: lamp_move}), options
    raise KeyError(name)


FILM_CASES = ["cornell", "showroom_smooth", "glass_blobs", "textured", "lamp_reference", "lamp_area", "lamp_power", "lamp_env"]


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("name", FILM_CASES)
def test_film_after_an_update_is_a_fresh_preprocess(xpu, name, mode):
    sc, new, options = _film_case(name)
    assert not np.array_equal(tri_abc(sc), tri_abc(new))
    a, b = make(xpu, **options), make(xpu, **options)
    try:
        a.preprocess(sc)
        film0, rays0 = frame(xpu, a, sc)
        before = a.stats()["device_bytes"]
        summary = a.update_geometry(new, mode)
        assert summary["mode"] == (0 if mode == "refit" else 1) and summary["triangles"] == new.num_triangles
        if mode == "refit":
            assert a.stats()["device_bytes"] == before, "a refit changed what the device holds"
        b.preprocess(new)
        film_a, rays_a = frame(xpu, a, new)
        film_b, rays_b = frame(xpu, b, new)
        differ = np.argwhere((film_a.view(np.uint32) != film_b.view(np.uint32)).any(-1))
        assert len(differ) == 0, f"{len(differ)} pixels differ from the fresh preprocess, the first at (y, x) {differ[:4].tolist()}"
        assert rays_a == rays_b
        assert not np.array_equal(film_a, film0), "the moved scene renders the old film: the test's motion shows nowhere"
        if mode == "rebuild":  # the builders are deterministic: after a rebuild and a frame the device holds what the fresh one holds, to the byte
            assert a.stats()["device_bytes"] == b.stats()["device_bytes"], "a rebuild left more (or less) on the device than a fresh preprocess"
        if name == "cornell":  # set_camera and render_guides behave as on the fresh device
            from phosphorus_mk2_amd import scenes
            cam = scenes.CameraDesc(W_, H_, 1.7, np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0.1, 0.05, 0.2, 1]], F))
            a.set_camera(cam); b.set_camera(cam)
            assert bits_equal(a.render_guides(3, 4), b.render_guides(3, 4))
            fa, ra = frame(xpu, a, new); fb, rb = frame(xpu, b, new)
            assert bits_equal(fa, fb) and ra == rb
            a.set_camera(sc.camera)
        a.update_geometry(sc, mode)  # and back
        film1, rays1 = frame(xpu, a, sc)
        assert bits_equal(film1, film0) and rays1 == rays0, "the update back does not restore the original film"
        assert a.stats()["device_bytes"] == before, "there and back left the device with another amount of memory"
    finally:
        a.close(); b.close()


# ---- refusals, state, animation ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_old_scene_and_a_running_frame_is_left_alone(xpu):
    from dataclasses import replace
    from phosphorus_mk2_amd import scenes
    sc = scenes.cornell(W_, H_)
    dev = make(xpu)
    try:
        with pytest.raises(xpu.DeviceError, match=r"\(4\).*before preprocess"):
            dev.update_geometry(sc)
        dev.preprocess(sc)
        film0, rays0 = frame(xpu, dev, sc)
        fewer = replace(sc, meshes=sc.meshes[:2] + sc.meshes[3:])
        nan = scenes.transformed(sc, {0: rigid(0.0, (0.0, float("nan"), 0.0))})
        other = replace(sc, meshes=[replace(sc.meshes[0], sets=[(1, sc.meshes[0].sets[0][1])])] + sc.meshes[1:])
        for bad, why in ((fewer, "triangle count"), (nan, "not finite"), (other, "material word")):
            with pytest.raises(xpu.DeviceError, match=r"\(1\).*" + why):
                dev.update_geometry(bad)
            film, rays = frame(xpu, dev, sc)
            assert bits_equal(film, film0) and rays == rays0, f"a refused update ({why}) changed the next frame"
        with pytest.raises(ValueError):
            dev.update_geometry(sc, "rebuilt")
        # an update while a frame runs
        film = xpu.Film(W_, H_, 4, True)
        dev.start(sc, xpu.FrameState(3, xpu.Tiles.make(W_, H_, 16), film, native_sink=True))
        with pytest.raises(xpu.DeviceError, match=r"\(4\).*while a frame is running"):
            dev.update_geometry(scenes.wobbled(sc, 0.01))
        dev.join()
        assert bits_equal(film.data, film0)
    finally:
        dev.close()


def test_a_scene_switch_after_updates_leaves_nothing_behind(xpu):
    """textured room -> rebuilt -> Cornell (no image, no UV, another light count) -> refitted: every film, guide film and ray counter is the
    fresh device's.  (device_bytes is not compared: buffers grow only across a preprocess.)"""
    room, room_moved, _ = _film_case("textured")
    box, box_moved, _ = _film_case("cornell")
    a, b = make(xpu), make(xpu)
    try:
        a.preprocess(room)
        a.update_geometry(room_moved, "rebuild")
        for scene, arrive in ((box, lambda: a.preprocess(box)), (box_moved, lambda: a.update_geometry(box_moved, "refit"))):
            arrive()
            b.preprocess(scene)
            film_a, rays_a = frame(xpu, a, scene)
            film_b, rays_b = frame(xpu, b, scene)
            differ = np.argwhere((film_a.view(np.uint32) != film_b.view(np.uint32)).any(-1))
            assert len(differ) == 0, f"{len(differ)} pixels differ from the fresh device, the first at (y, x) {differ[:4].tolist()}"
            assert rays_a == rays_b
            assert bits_equal(a.render_guides(3, 4), b.render_guides(3, 4))
    finally:
        a.close(); b.close()


def test_a_rebuild_refused_while_committing_leaves_the_device_without_a_scene(xpu):
    """As test_gpu_parity.py's test_a_preprocess_that_fails_while_committing_..., for the update's rebuild: the device builder's fatal error,
    forced in the fault-injection twin (libphx_hip_hooks.so), comes after the old pool is gone, so start and a further update answer
    PHX_ERR_STATE (4) until a preprocess succeeds.  Under the auto builder a recoverable failure falls back to the host builder instead: the
    film does not depend on the tree, so it is the product library's of a fresh preprocess.  Refused calls; nothing faults."""
    import hashlib, json, os, subprocess, sys
    from conftest import ROOT
    from phosphorus_mk2_amd import scenes
    hooks = os.path.join(ROOT, "phosphorus_mk2_amd", "libphx_hip_hooks.so")
    assert os.path.exists(hooks), "build() makes the fault-injection twin"
    code = ("import hashlib, json, os, sys; sys.path.insert(0, %r)\n"
            "from phosphorus_mk2_amd import scenes, xpu\n"
            "a = scenes.soup(500, width=32, height=32); moved = scenes.wobbled(a, 0.02, seed=1)\n"
            "def device(builder):\n"
            "    return xpu.HipDevice.make(xpu.Options(samples_per_pixel=4, paths_per_sample=1, path_depth=5, bvh_builder=builder))\n"
            "def frame(dev, sc):\n"
            "    film = xpu.Film(32, 32, 4)\n"
            "    dev.start(sc, xpu.FrameState(1, xpu.Tiles.make(32, 32, 32), film)); dev.join()\n"
            "    return film.data.copy()\n"
            "def refused(call):\n"
            "    try:\n"
            "        call()\n"
            "    except xpu.DeviceError as e:\n"
            "        return str(e)\n"
            "    return 'NOT REFUSED'\n"
            "dev = device('device')\n"
            "dev.preprocess(a)\n"
            "first = frame(dev, a)\n"
            "print('LIT', bool(first[..., :3].max() > 0.05))\n"
            "os.environ['PHX_TEST_FAIL_DEVICE_BUILD'] = 'fatal'\n"
            "print('REBUILD', refused(lambda: dev.update_geometry(moved, 'rebuild')))\n"
            "print('START', refused(lambda: frame(dev, a)))\n"
            "print('REFIT', refused(lambda: dev.update_geometry(moved, 'refit')))\n"
            "del os.environ['PHX_TEST_FAIL_DEVICE_BUILD']\n"
            "dev.preprocess(a)\n"
            "print('AGAIN', first.tobytes() == frame(dev, a).tobytes())\n"
            "dev.close()\n"
            "dev = device('auto')\n"
            "dev.preprocess(a)\n"
            "print('DEVICE_BUILT', dev.stats()['bvh_built_on_device'])\n"
            "os.environ['PHX_TEST_FAIL_DEVICE_BUILD'] = 'recoverable'\n"
            "print('FELL_BACK', refused(lambda: dev.update_geometry(moved, 'rebuild')), dev.stats()['bvh_built_on_device'])\n"
            "film = frame(dev, moved); st = dev.stats()\n"
            "print('FILM', hashlib.sha1(film.tobytes()).hexdigest(), json.dumps([st[k] for k in %r]))\n"
            "dev.close()\n") % (ROOT, COUNTERS)
    env = {k: v for k, v in os.environ.items() if k != "PHX_TEST_FAIL_DEVICE_BUILD"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(env, PHX_LIB=hooks))
    assert r.returncode == 0, (r.stdout, r.stderr[-800:])
    out = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in r.stdout.splitlines() if " " in l}
    assert out["LIT"] == "True"
    assert "(2)" in out["REBUILD"] and "device BVH build" in out["REBUILD"]  # PHX_ERR_DEVICE
    assert "phx_dev_start failed (4)" in out["START"] and "start before preprocess" in out["START"]
    assert "(4)" in out["REFIT"] and "before preprocess" in out["REFIT"]
    assert out["AGAIN"] == "True"
    assert out["DEVICE_BUILT"] == "1" and out["FELL_BACK"] == "NOT REFUSED 0" and "fell back to the host builder" in r.stderr
    # the product library's fresh preprocess of the moved scene
    moved = scenes.wobbled(scenes.soup(500, width=32, height=32), 0.02, seed=1)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=4, paths_per_sample=1, path_depth=5))
    try:
        dev.preprocess(moved)
        film = xpu.Film(32, 32, 4)
        dev.start(moved, xpu.FrameState(1, xpu.Tiles.make(32, 32, 32), film)); dev.join()
        st = dev.stats()
        assert st["bvh_built_on_device"] == 1
        assert out["FILM"] == hashlib.sha1(film.data.tobytes()).hexdigest() + " " + json.dumps([st[k] for k in COUNTERS])
    finally:
        dev.close()


def test_render_animation_yields_the_fresh_films(xpu):
    from phosphorus_mk2_amd import scenes
    sc = scenes.cornell(W_, H_)
    path = [sc, scenes.transformed(sc, {5: rigid(0.2, (0.1, -0.1, 0.0))}), scenes.transformed(sc, {5: rigid(0.4, (0.2, -0.2, 0.1)), 2: rigid(0.0, (0.0, 0.0, 0.3))})]
    films = [(np.array(f), s, k) for f, s, k in xpu.render_animation(path, SPP, mode="refit", rebuild_every=2, seed=3, depth=5)]
    assert [k for _, _, k in films] == [0, 1, 2] and films[0][1] is None and films[1][1]["mode"] == 0 and films[2][1]["mode"] == 1
    for (film, _, _), scene in zip(films, path):
        dev = make(xpu)
        try:
            dev.preprocess(scene)
            W, H = scene.camera.width, scene.camera.height
            fresh = xpu.Film(W, H, 4, True, True, False)
            dev.start(scene, xpu.FrameState(3, xpu.Tiles.make(W, H, 32), fresh, native_sink=True))
            dev.join()
            assert bits_equal(film, fresh.data)
        finally:
            dev.close()


def test_render_animation_denoises_the_fresh_films_and_displays_that(xpu):
    """denoise={} and display={} on 32 x 32 films of 4 samples: each yielded film is the denoise of the scene's fresh frame, each image its display"""
    from phosphorus_mk2_amd import scenes
    sc = scenes.cornell(32, 32)
    path = [sc, scenes.transformed(sc, {5: rigid(0.2, (0.1, -0.1, 0.0))}), scenes.transformed(sc, {5: rigid(0.4, (0.2, -0.2, 0.1)), 2: rigid(0.0, (0.0, 0.0, 0.3))})]
    got = [(np.array(f), image) for f, _, _, image in xpu.render_animation(path, 4, mode="refit", denoise={}, display={}, seed=3, depth=5)]
    assert len(got) == 3
    for (film, image), scene in zip(got, path):
        dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=4, paths_per_sample=1, path_depth=5))
        try:
            dev.preprocess(scene)
            fresh = xpu.Film(32, 32, 4, True, True, False)
            dev.start(scene, xpu.FrameState(3, xpu.Tiles.make(32, 32, 32), fresh, native_sink=True))
            dev.join()
            want = dev.denoise(fresh.data, 4, 4, True, False)
            assert bits_equal(film, want) and not bits_equal(want, fresh.data)
            assert image.shape == (32, 32, 4) and np.array_equal(image, dev.display(want))
        finally:
            dev.close()


def test_plain_c_host_animates(xpu, tmp_path):
    """examples/render_room.c `animate 2`: one `update:` line per frame, and the film on file is the fresh film of the room with its two tilted
    triangles (vertices 12 .. 17) moved by 0.8 along x, the last of the two positions"""
    import os
    import re
    import subprocess
    from test_gpu_parity import _room_scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(root, "examples")], check=True)
    out = str(tmp_path / "room.f32")
    r = subprocess.run([exe, out, "animate", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [bool(re.fullmatch(r"update: frame %d refit \d+\.\d{3} ms" % (k + 1), l)) for k, l in enumerate(lines[0::2])] == [True, True], r.stdout
    assert all(l.startswith(f"animate: frame {k + 1} triangles 8 nodes 1 levels 1 ") for k, l in enumerate(lines[1::2])) and len(lines) == 4
    sc = _room_scene()
    sc.meshes[0].vertices[12:18, 0] = (sc.meshes[0].vertices[12:18, 0] + F(F(F(0.8) * F(2.0)) / F(2.0))).astype(F)
    film, _ = xpu.render(sc, spp=8, pps=1, depth=5, seed=7, native_sink=True)
    assert bits_equal(np.fromfile(out, np.float32).reshape(96, 128, 4), film)
