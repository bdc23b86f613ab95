"""Image textures on the device (k_shade_g<., ., ., TEX>, phx_dev_texture_lookup).  The oracle knows no textures: the device's lookup is
compared with the numpy restatement below, and a textured film with the oracle's film of the same geometry whose materials carry the
texel already multiplied into their weight (fp32), which is what the device must compute per hit."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


# ---- numpy restatement of the lookup (include/phx_xpu.h: phx_texture) --------------------------------------------------------------
def _wrap(i, n, mode):
    from phosphorus_mk2_amd import abi
    if mode == abi.WRAP_PERIODIC:
        return np.mod(i, n), np.zeros(i.shape, bool)
    if mode == abi.WRAP_CLAMP:
        return np.clip(i, 0, n - 1), np.zeros(i.shape, bool)
    out = (i < 0) | (i > n - 1)
    return np.where(out, 0, i), out


def np_lookup(tex, st):
    """fp32, operation by operation: x = s*W - 0.5, y = t*H - 0.5, bilinear c = t00 + fx (t10 - t00), d = t01 + fx (t11 - t01),
    c + fy (d - c); closest (floor(s W), floor(t H)); non-finite or |s W|, |t H| > 2^24: black"""
    from phosphorus_mk2_amd import abi
    img = tex.texels
    H, W = img.shape[:2]
    st = np.asarray(st, F).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        sw = st[:, 0] * F(W); th = st[:, 1] * F(H)
        ok = (np.abs(sw) <= F(16777216.0)) & (np.abs(th) <= F(16777216.0))
        sw = np.where(ok, sw, F(0)); th = np.where(ok, th, F(0))

    def texel(i, j):
        x, ox = _wrap(i, W, tex.swrap); y, oy = _wrap(j, H, tex.twrap)
        return np.where((ox | oy)[:, None], F(0), img[y, x])

    if tex.filter == abi.TEX_CLOSEST:
        out = texel(np.floor(sw).astype(np.int64), np.floor(th).astype(np.int64))
    else:
        x = sw - F(0.5); y = th - F(0.5)
        x0 = np.floor(x); y0 = np.floor(y)
        fx = (x - x0)[:, None]; fy = (y - y0)[:, None]
        i = x0.astype(np.int64); j = y0.astype(np.int64)
        t00, t10, t01, t11 = texel(i, j), texel(i + 1, j), texel(i, j + 1), texel(i + 1, j + 1)
        c = t00 + fx * (t10 - t00)
        d = t01 + fx * (t11 - t01)
        out = c + fy * (d - c)
    return np.where(ok[:, None], out, F(0)).astype(F)


def _textured_cornell(textures, width=16, height=16):
    """the Cornell box whose grey walls carry texture 1 (a scene with a textured lobe uploads the whole texture table)"""
    from phosphorus_mk2_amd import scenes
    sc = scenes.cornell(width, height)
    sc.textures = list(textures)
    sc.materials[0].lobes[0].texture = 1
    return sc


def test_lookup_is_bit_equal_to_the_restatement(xpu):
    from phosphorus_mk2_amd import abi, scenes
    rng = np.random.default_rng(11)
    images = [rng.uniform(0.0, 1.0, (3, 4, 3)).astype(F), rng.uniform(-1.0, 2.0, (1, 7, 3)).astype(F),
              rng.uniform(0.0, 1.0, (6, 1, 3)).astype(F), rng.uniform(0.0, 1.0, (5, 9, 3)).astype(F)]
    modes = [(w, w) for w in (abi.WRAP_PERIODIC, abi.WRAP_CLAMP, abi.WRAP_BLACK)] + [(abi.WRAP_PERIODIC, abi.WRAP_BLACK), (abi.WRAP_BLACK, abi.WRAP_CLAMP)]
    texs = [scenes.TextureDesc(img, f, sw, tw) for img in images for f in (abi.TEX_LINEAR, abi.TEX_CLOSEST) for sw, tw in modes]
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2))
    try:
        dev.preprocess(_textured_cornell(texs))
        eps = np.finfo(F).eps
        special = np.array([0.0, 1.0, 1.0 - eps / 2, 1.0 - eps, -0.0, np.nan, np.inf, -np.inf, 1e9, -1e9, 0.5, -1.0, 2.0], F)
        for k, tex in enumerate(texs):
            H, W = tex.texels.shape[:2]
            centres = np.stack(np.meshgrid((np.arange(-W, 2 * W) + F(0.5)) / F(W), (np.arange(-H, 2 * H) + F(0.5)) / F(H)), -1).reshape(-1, 2)
            edges = np.stack(np.meshgrid(np.arange(-W, 2 * W + 1) / F(W), np.arange(-H, 2 * H + 1) / F(H)), -1).reshape(-1, 2)
            grid = np.stack(np.meshgrid(special, special), -1).reshape(-1, 2)
            st = np.concatenate([rng.uniform(-3.0, 3.0, (100_000, 2)), centres, edges, grid]).astype(F)
            got = dev.texture_lookup(k, st)
            want = np_lookup(tex, st)
            assert bits_equal(got, want), (k, tex.filter, tex.swrap, tex.twrap, tex.texels.shape)
            assert np.isfinite(got).all()
    finally:
        dev.close()


# ---- the textured box against the oracle --------------------------------------------------------------------------------------------
TEX43 = np.array([[[0.9, 0.2, 0.1], [0.1, 0.8, 0.2], [0.2, 0.3, 0.9], [0.7, 0.7, 0.2]],
                  [[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.9, 0.5, 0.7], [0.3, 0.9, 0.9]],
                  [[0.6, 0.1, 0.8], [0.95, 0.9, 0.85], [0.25, 0.6, 0.4], [0.8, 0.4, 0.3]]], F)  # (H 3, W 4); texel (0, 1) is black


def _bake(lobe, texel):
    from phosphorus_mk2_amd import scenes
    w = tuple(F(a) * F(b) for a, b in zip(lobe.weight, texel))
    return scenes.LobeDesc(lobe.type, w, lobe.alpha, lobe.eta, lobe.xalpha, lobe.yalpha, lobe.refract, lobe.r, lobe.fac_mode, lobe.fac_ior,
                           lobe.pre_weight, 0)


def _bake_material(m, texel):
    """the material with every textured lobe's weight multiplied by `texel`; a textured lobe whose weight is all zero is not there"""
    from phosphorus_mk2_amd import scenes
    lobes = []
    for l in m.lobes:
        if not l.texture:
            lobes.append(l)
            continue
        b = _bake(l, texel)
        if any(x != 0 for x in b.weight):
            lobes.append(b)
    return scenes.MaterialDesc(lobes, m.emission, m.is_emitter)


def grid_box(per_vertex=True, nx=8, ny=6, width=64, height=48, lens=False, glass=True):
    """(textured scene, baked scene): the Cornell box whose back wall is a grid of nx x ny quads, each quad's UV triangles strictly inside
    one texel of TEX43 (CLOSEST).  Materials on the grid, by quad: textured Lambert; Lambert + glossy with the Lambert textured (it drops
    on the black texel); Blender's glass node with its refraction colour textured (per-hit Fresnel x texture).  The baked scene has
    the same face sets in the same order, each with the material of its texel baked in.  glass=False leaves the glass material out: no
    closure weight of the scene then depends on the hit (k_shade_g<false, ., ., true>, TEX without PERHIT)."""
    from phosphorus_mk2_amd import abi, scenes
    D, MF = abi.LOBE_DIFFUSE, abi.LOBE_MICROFACET
    box = scenes.cornell(width, height)
    back = box.meshes.pop(2)  # the plain back wall goes; the grid takes its place
    assert back.vertices[:, 2].max() == -3.5
    tex_mats = [scenes.MaterialDesc([scenes.LobeDesc(D, (0.8, 0.75, 0.7), texture=1)]),
                scenes.MaterialDesc([scenes.LobeDesc(D, (0.7, 0.7, 0.7), texture=1), scenes.LobeDesc(MF, (0.3, 0.3, 0.3), xalpha=0.09, yalpha=0.09)])]
    if glass:
        glass = scenes.glass(1.45, 0.0, (0.95, 0.98, 0.95), (1.0, 1.0, 1.0))
        assert glass.lobes[0].type == abi.LOBE_REFRACTION and glass.lobes[0].fac_mode != 0
        glass.lobes[0].texture = 1
        tex_mats.append(glass)
    base = len(box.materials)
    mats_t = box.materials + tex_mats
    mats_b = list(box.materials)
    verts, faces, uvs, sets_t, sets_b = [], [], [], [], []
    x0, x1, y0, y1, z = -1.0, 1.0, -1.0, 1.0, -3.5
    for qy in range(ny):
        for qx in range(nx):
            a = (x0 + (x1 - x0) * qx / nx, y0 + (y1 - y0) * qy / ny)
            b = (x0 + (x1 - x0) * (qx + 1) / nx, y0 + (y1 - y0) * (qy + 1) / ny)
            v = len(verts)
            verts += [(a[0], a[1], z), (b[0], a[1], z), (b[0], b[1], z), (a[0], b[1], z)]
            f = len(faces)
            faces += [(v, v + 1, v + 2), (v, v + 2, v + 3)]
            i, j = qx % 4, (qx + qy) % 3  # texel of this quad: column i, row j
            s0, s1, t0, t1 = (i + 0.25) / 4, (i + 0.75) / 4, (j + 0.75) / 3, (j + 0.25) / 3
            corner = [(s0, t0), (s1, t0), (s1, t1), (s0, t1)]
            if per_vertex:
                uvs += corner
            else:
                uvs += [corner[0], corner[1], corner[2], corner[0], corner[2], corner[3]]
            k = (qx * 7 + qy * 3) % len(tex_mats)
            sets_t.append((base + k, np.array([f, f + 1], np.uint32)))
            mats_b.append(_bake_material(tex_mats[k], TEX43[j, i]))
            sets_b.append((len(mats_b) - 1, np.array([f, f + 1], np.uint32)))
    flags = abi.MESH_NORMALS_PER_VERTEX | (abi.MESH_UV_PER_VERTEX if per_vertex else 0)
    grid_t = scenes.MeshDesc(np.array(verts, F), np.array(faces, np.uint32), sets_t, flags=flags, uvs=np.array(uvs, F))
    grid_b = scenes.MeshDesc(np.array(verts, F), np.array(faces, np.uint32), sets_b, flags=flags)
    st = scenes.SceneDesc(box.meshes[:2] + [grid_t] + box.meshes[2:], mats_t, box.camera, textures=[scenes.TextureDesc(TEX43, abi.TEX_CLOSEST)])
    sb = scenes.SceneDesc(box.meshes[:2] + [grid_b] + box.meshes[2:], mats_b, scenes.CameraDesc(width, height, box.camera.fov))
    if lens:
        for s in (st, sb):
            s.camera.aperture_radius, s.camera.focal_distance = 0.03, 3.0
    return st, sb


def _compare_with_oracle(xpu, orc, st, sb, spp, seed, **kw):
    film, s = xpu.render(st, spp=spp, pps=1, depth=9, seed=seed, **kw)
    orc.set_tie_rule(1)  # the grid's quads share edges: the lower primitive index wins a tie, as on the device
    try:
        ref, ost = orc.Oracle(sb, spp=spp, pps=1, depth=9).render(rng=orc.RNG_COUNTER, seed=seed, threads=8)
    finally:
        orc.set_tie_rule(0)
    assert (s["rays_closest"], s["rays_shadow"], s["rays_masked"]) == (ost["rays_closest"], ost["rays_shadow"], ost["rays_masked"])
    assert np.isfinite(film).all() and film[..., :3].max() > 0.05
    assert bits_equal(film[..., :3], ref[..., :3])
    return film, s


@pytest.mark.parametrize("per_vertex,flight,lens", [(True, 0, False), (False, 0, False), (True, 4, False), (False, 0, True)])
def test_closest_texels_match_the_baked_oracle_scene(xpu, orc, per_vertex, flight, lens):
    st, sb = grid_box(per_vertex, lens=lens)
    film, s = _compare_with_oracle(xpu, orc, st, sb, spp=16, seed=5, samples_in_flight=flight)
    assert s["shade_general"] == 1


def test_uniform_linear_texture_on_the_closure_zoo(xpu, orc):
    """every lobe of the 16 recipes textured by a constant LINEAR / PERIODIC image at random UVs: each lookup returns the constant bit
    for bit, so the film is the oracle's with the constant multiplied into every weight"""
    from phosphorus_mk2_amd import abi, scenes
    st = scenes.multi_material_soup(3000, width=64, height=64)
    sb = scenes.multi_material_soup(3000, width=64, height=64)
    c = np.array([0.8, 0.6, 0.9], F)
    st.textures = [scenes.TextureDesc(np.broadcast_to(c, (5, 7, 3)).copy(), abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_PERIODIC)]
    rng = np.random.default_rng(3)
    for m in st.meshes:
        m.uvs = rng.uniform(-2.0, 2.0, (len(m.vertices), 2)).astype(F)
    for i, m in enumerate(st.materials):
        if m.is_emitter:
            continue
        for l in m.lobes:
            l.texture = 1
        sb.materials[i] = _bake_material(m, c)
    _compare_with_oracle(xpu, orc, st, sb, spp=8, seed=2)


def test_bilinear_filter_and_uv_interpolation_end_to_end(xpu, orc):
    """one textured Lambert quad facing one emitter quad, nothing else (no path has three events: roulette never acts).  At spp 1 the
    textured film divided by the untextured one is, per pixel whose camera ray hits the quad, the texel at the ray's (s, t) — computed
    here from the hit the device's own trace returns and the numpy lookup.  Once with the UVs turned by 90 degrees, so that swapped
    s / t or flipped rows cannot pass."""
    from phosphorus_mk2_amd import abi, scenes
    W = H = 32  # one tile: orc.camera_rays takes at most 1024 rays
    yy, xx = np.meshgrid(np.linspace(0, 1, 5, dtype=F), np.linspace(0, 1, 6, dtype=F), indexing="ij")
    img = np.stack([0.2 + 0.7 * xx, 0.2 + 0.7 * yy, 0.3 + 0.5 * ((np.arange(5)[:, None] + np.arange(6)[None, :]) % 2)], -1).astype(F)
    quad_v = np.array([(-2, -2, -3), (2, -2, -3), (2, 2, -3), (-2, 2, -3)], F)
    light_v = np.array([(1.2, -0.5, -0.5), (1.2, 0.5, -0.5), (2.2, 0.5, -0.5), (2.2, -0.5, -0.5)], F)  # out of the camera's view, facing the quad
    f2 = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    for rot in (False, True):
        uv = np.array([(-0.2, 1.3), (1.4, 1.3), (1.4, -0.1), (-0.2, -0.1)], F)
        if rot:
            uv = np.stack([uv[:, 1], F(1) - uv[:, 0]], 1)

        def scene(textured):
            mats = [scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_DIFFUSE, (0.8, 0.8, 0.8), texture=1 if textured else 0)]), scenes.emitter(3.0, 3.0, 3.0)]
            meshes = [scenes.MeshDesc(quad_v, f2, [(0, np.arange(2, dtype=np.uint32))], uvs=uv),
                      scenes.MeshDesc(light_v, f2, [(1, np.arange(2, dtype=np.uint32))])]
            return scenes.SceneDesc(meshes, mats, scenes.CameraDesc(W, H, 1.2),
                                    textures=[scenes.TextureDesc(img, abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_CLAMP)] if textured else [])
        st, su = scene(True), scene(False)
        ft, s_t = xpu.render(st, spp=1, pps=1, depth=9, seed=9)
        fu, s_u = xpu.render(su, spp=1, pps=1, depth=9, seed=9)
        assert s_t["rays_closest"] == s_u["rays_closest"] and s_t["rays_shadow"] == s_u["rays_shadow"]
        o, d = orc.Oracle(su, spp=1, pps=1, depth=9).camera_rays((0, 0, W, H), 0, seed=9)
        dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=9))
        try:
            dev.preprocess(st)
            h = dev.trace(o, d, np.full(len(o), np.finfo(F).max, F))
        finally:
            dev.close()
        on_quad = h["prim"] <= 1  # triangles 0, 1: the quad (mesh order)
        assert on_quad.sum() > W * H // 4
        p = h["prim"][on_quad].astype(np.int64); u = h["u"][on_quad]; v = h["v"][on_quad]
        tri = f2[p]
        w = (F(1) - u) - v
        s_ = (w * uv[tri[:, 0], 0] + u * uv[tri[:, 1], 0]) + v * uv[tri[:, 2], 0]
        t_ = (w * uv[tri[:, 0], 1] + u * uv[tri[:, 1], 1]) + v * uv[tri[:, 2], 1]
        want = np_lookup(st.textures[0], np.stack([s_, t_], 1)).astype(np.float64)
        a = ft[..., :3].reshape(-1, 3)[on_quad].astype(np.float64); b = fu[..., :3].reshape(-1, 3)[on_quad].astype(np.float64)
        lit = (b > 0).all(1)
        assert lit.mean() > 0.9
        ratio = a[lit] / b[lit]
        assert (np.abs(ratio - want[lit]) <= 2e-6 * np.abs(want[lit])).all(), (rot, np.abs(ratio / want[lit] - 1).max())


# ---- untextured scenes are untouched --------------------------------------------------------------------------------------------------
def test_uvs_without_a_textured_lobe_change_nothing(xpu):
    from phosphorus_mk2_amd import scenes
    a = scenes.multi_material_soup(3000, width=64, height=48)
    b = scenes.multi_material_soup(3000, width=64, height=48)
    rng = np.random.default_rng(5)
    for m in b.meshes:
        m.uvs = rng.uniform(0.0, 1.0, (len(m.vertices), 2)).astype(F)
    b.textures = [scenes.TextureDesc(np.ones((2, 2, 3), F))]  # a texture table no lobe uses
    fa, sa = xpu.render(a, spp=8, pps=1, depth=9, seed=3)
    fb, sb_ = xpu.render(b, spp=8, pps=1, depth=9, seed=3)
    assert bits_equal(fa, fb) and sa["rays_closest"] == sb_["rays_closest"] and sa["rays_shadow"] == sb_["rays_shadow"]
    assert sa["shade_general"] == sb_["shade_general"] == 1
    assert sa["device_bytes"] == sb_["device_bytes"]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_bad_texture_inputs_are_refused_and_the_device_stays_usable(xpu):
    from phosphorus_mk2_amd import abi, scenes
    good = _textured_cornell([scenes.TextureDesc(TEX43, abi.TEX_LINEAR)], 32, 32)
    good.meshes[0].uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)

    def out_of_range(s):
        s.materials[1].lobes[0].texture = 2

    def on_emitter(s):
        s.materials[3].lobes = [scenes.LobeDesc(abi.LOBE_DIFFUSE, (1, 1, 1), texture=1)]

    def on_environment(s):
        s.materials.append(scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_DIFFUSE, (1, 1, 1), texture=1)], emission=(0.1, 0.1, 0.1)))
        s.environment_material = len(s.materials) - 1

    def zero_size(s):
        s.textures.append(scenes.TextureDesc(np.zeros((0, 4, 3), F)))

    def too_large(s):
        s.textures.append(scenes.TextureDesc(np.zeros((1, 70000, 3), F)))

    def uv_index(s):
        s.meshes[0].uvs = s.meshes[0].uvs[:3]  # per vertex: vertex 3 has no UV

    def uv_index_corner(s):
        s.meshes[1].uvs = np.zeros((5, 2), F)  # per face corner: 6 are needed
        s.meshes[1].flags &= ~abi.MESH_UV_PER_VERTEX

    import copy
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=4, paths_per_sample=1, path_depth=9))
    try:
        def frame():
            film = xpu.Film(32, 32, 4)
            dev.start(good, xpu.FrameState(1, xpu.Tiles.make(32, 32, 32), film)); dev.join()
            return film.data.copy()
        dev.preprocess(good)
        ref = frame()
        assert ref[..., :3].max() > 0.05
        for bad in (out_of_range, on_emitter, on_environment, zero_size, too_large, uv_index, uv_index_corner):
            s = copy.deepcopy(good)
            bad(s)
            with pytest.raises(xpu.DeviceError) as e:
                dev.preprocess(s)
            assert "(1)" in str(e.value) and len(str(e.value).split(":", 1)[1].strip()) > 5, bad.__name__  # PHX_ERR_ARG with a message
            dev.preprocess(good)
            assert bits_equal(frame(), ref), bad.__name__
    finally:
        dev.close()
