"""Synthetic inputs are reproducible functions of (N, seed) — the generator is committed, not the data."""
import hashlib

import numpy as np


def test_soup_is_deterministic_and_matches_its_spec():
    from phosphorus_mk2_amd import scenes
    a = scenes.soup(1000, seed=1234); b = scenes.soup(1000, seed=1234); c = scenes.soup(1000, seed=1235)
    va, vb, vc = a.meshes[0].vertices, b.meshes[0].vertices, c.meshes[0].vertices
    assert np.array_equal(va, vb) and not np.array_equal(va, vc)
    assert hashlib.sha1(va.tobytes()).hexdigest() == hashlib.sha1(scenes.soup(1000).meshes[0].vertices.tobytes()).hexdigest()
    e = 2 * 1000 ** (-1 / 3)
    tri = va.reshape(-1, 3, 3)
    assert tri[..., 0].min() >= -0.98 - e - 1e-5 and tri[..., 0].max() <= 0.98 + e + 1e-5
    assert tri[..., 2].min() >= -2.5 - 0.98 - e - 1e-5 and tri[..., 2].max() <= -2.5 + 0.98 + e + 1e-5
    assert a.num_triangles == 1002 and len(a.materials) == 2 and a.materials[1].is_emitter
    # prefix property: the first triangles do not depend on N only through the scale e
    big = scenes.soup(2000).meshes[0].vertices.reshape(-1, 3, 3)
    assert big.shape[0] == 2000


def test_cornell_normals_face_inwards():
    from phosphorus_mk2_amd import scenes
    sc = scenes.cornell()
    centre = np.array([0, 0, -2.5])
    for m in sc.meshes:
        v = m.vertices
        for f in m.faces:
            n = np.cross(v[f[1]] - v[f[0]], v[f[2]] - v[f[0]])
            assert np.dot(n, centre - v[f[0]]) > 0
    assert sc.num_triangles == 12


def test_pack_round_trip():
    from phosphorus_mk2_amd import scenes
    sc = scenes.multi_material_soup(100)
    s, keep = sc.pack()
    assert s.num_meshes == 2 and s.num_materials == 17
    assert s.meshes[0].num_faces == 100 and s.meshes[0].num_sets == 16
    assert s.materials[4].lobes[0].type == 16 and abs(s.materials[4].lobes[0].xalpha - 0.09) < 1e-7
    assert s.camera.film_width == 1280 and abs(s.camera.fov - 1.9) < 1e-6


def test_deep_comb_matches_its_spec():
    """scenes.deep_comb: triangle i lies in the plane x = ratio^i, faces the camera at the origin (geometric normal -x), is 0.5 x_i across and
    centred on the axis (so every one subtends the same angle); the lamp behind the camera faces +x; the camera looks down +x"""
    from phosphorus_mk2_amd import abi, scenes
    sc = scenes.deep_comb()
    assert sc.num_triangles == 402 and len(sc.meshes) == 2 and (sc.camera.width, sc.camera.height) == (64, 48)
    assert abs(sc.camera.fov - 0.6) < 1e-7
    tri = sc.meshes[0].vertices[sc.meshes[0].faces].astype(np.float64)  # (400, 3, 3)
    x = 1.08 ** np.arange(400)
    assert np.allclose(tri[..., 0], x[:, None], rtol=1e-6, atol=0)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (n[:, 0] < 0).all() and np.allclose(n[:, 1:] / -n[:, :1], 0, atol=1e-6)
    side = np.linalg.norm(tri - np.roll(tri, 1, axis=1), axis=2)
    assert np.allclose(side / x[:, None], 0.5, rtol=1e-5)
    assert np.allclose(tri.mean(1)[:, 1:] / x[:, None], 0, atol=1e-6)  # centred on the axis
    lamp = sc.meshes[1].vertices[sc.meshes[1].faces].astype(np.float64)
    assert (lamp[..., 0] == np.float32(-0.3)).all()
    assert (np.cross(lamp[:, 1] - lamp[:, 0], lamp[:, 2] - lamp[:, 0])[:, 0] > 0).all() and sc.materials[1].is_emitter
    assert [l.type for l in sc.materials[0].lobes] == [abi.LOBE_REFRACTION, abi.LOBE_REFLECTION]  # glass(1.45)
    assert np.allclose(np.array([0, 0, -1], np.float32) @ sc.camera.to_world[:3, :3], [1, 0, 0])  # row-vector convention
    bare = scenes.deep_comb(200, 1.2, lamp=False, material=scenes.diffuse(0.5, 0.5, 0.5))
    assert bare.num_triangles == 200 and len(bare.meshes) == 1 and bare.materials[0].lobes[0].type == abi.LOBE_DIFFUSE
    assert np.isclose(bare.meshes[0].vertices[:, 0].max(), 1.2 ** 199, rtol=1e-6)
    o, d, tm = scenes.deep_comb_rays(1000, 200, 1.2, seed=3)
    assert o.shape == d.shape == (1000, 3) and (d == [1, 0, 0]).all() and (tm == np.finfo(np.float32).max).all()
