"""Image masks on closure mixes on the device (k_shade_g<PERHIT, ., ., TEX, ., MASK>, phx_dev_lobe_weights).  The oracle knows no masks:
the device's per-hit weights are compared bit for bit with the numpy restatement below (include/phx_xpu.h: phx_lobe.fac_mode), and a
masked film with the oracle's film of the same geometry whose materials have the mix already resolved into constant weights (fp32, in
the device's order), which is what the device must compute per hit.  Self-contained: own fixtures, own restatement."""
import copy

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


# ---- numpy restatement, fp32, operation by operation -----------------------------------------------------------------------------------
def _wrap(i, n, mode):
    from phosphorus_mk2_amd import abi
    if mode == abi.WRAP_PERIODIC:
        return np.mod(i, n), np.zeros(i.shape, bool)
    if mode == abi.WRAP_CLAMP:
        return np.clip(i, 0, n - 1), np.zeros(i.shape, bool)
    out = (i < 0) | (i > n - 1)
    return np.where(out, 0, i), out


def np_lookup(tex, st):
    """phx_texture: x = s*W - 0.5, y = t*H - 0.5, bilinear c = t00 + fx (t10 - t00), d = t01 + fx (t11 - t01), c + fy (d - c); closest
    (floor(s W), floor(t H)); |s W|, |t H| > 2^24: black"""
    from phosphorus_mk2_amd import abi
    img = tex.texels
    H, W = img.shape[:2]
    st = np.asarray(st, F).reshape(-1, 2)
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


def np_luminance(c):
    """fac = (c.r * 0.2126f + c.g * 0.7152f) + c.b * 0.0722f"""
    c = np.asarray(c, F)
    return ((c[..., 0] * F(0.2126) + c[..., 1] * F(0.7152)) + c[..., 2] * F(0.0722)).astype(F)


def np_masked_weight(lobe, textures, st):
    """w = (pre_weight * term) * (weight (*) colour texel) of a masked lobe at every st, and whether the lobe is there (w not all zero)"""
    from phosphorus_mk2_amd import abi
    st = np.asarray(st, F).reshape(-1, 2)
    w0 = np.broadcast_to(np.array(lobe.weight, F), (len(st), 3))
    if lobe.texture:
        w0 = w0 * np_lookup(textures[lobe.texture - 1], st)
    fac = np_luminance(np_lookup(textures[lobe.fac_texture - 1], st))
    term = fac if lobe.fac_mode == abi.FAC_TEX_B else F(1.0) - fac
    w = (np.array(lobe.pre_weight, F)[None, :] * term[:, None]) * w0
    return w.astype(F), (w != 0).any(1)


def resolve(mat, mask_texel, colour_texel=None):
    """the material a hit sees where its masks read `mask_texel` and its colour textures `colour_texel`: constant FAC_NONE weights in the
    device's order, zero-weight lobes removed (written out here; not the package's helper)"""
    from phosphorus_mk2_amd import abi, scenes
    fac = np_luminance(np.asarray(mask_texel, F))
    lobes = []
    for l in mat.lobes:
        if l.fac_mode not in (abi.FAC_TEX_A, abi.FAC_TEX_B):
            assert not l.texture
            lobes.append(copy.deepcopy(l))
            continue
        w0 = [F(x) for x in l.weight]
        if l.texture:
            w0 = [F(x * F(c)) for x, c in zip(w0, colour_texel)]
        term = fac if l.fac_mode == abi.FAC_TEX_B else F(F(1.0) - fac)
        w = tuple(float(F(F(F(p) * term) * x)) for p, x in zip(l.pre_weight, w0))
        if any(x != 0.0 for x in w):
            lobes.append(scenes.LobeDesc(l.type, w, l.alpha, l.eta, l.xalpha, l.yalpha, l.refract, l.r))
    return scenes.MaterialDesc(lobes, mat.emission, mat.is_emitter)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


# ---- 4. the hook against the restatement -----------------------------------------------------------------------------------------------
def test_lobe_weights_are_bit_equal_to_the_restatement(xpu):
    from phosphorus_mk2_amd import abi, scenes
    L = scenes.LobeDesc
    rng = np.random.default_rng(21)
    bw = (rng.uniform(0, 1, (4, 6, 1)) < 0.5).astype(F).repeat(3, axis=2)  # black and white: luminance exactly 0 / 1
    images = [rng.uniform(0.0, 1.0, (3, 4, 3)).astype(F), bw, rng.uniform(-0.5, 1.8, (5, 2, 3)).astype(F)]  # the last leaves [0, 1]: fac is not clamped
    texs = [scenes.TextureDesc(img, f, w, w) for img in images for f in (abi.TEX_LINEAR, abi.TEX_CLOSEST)
            for w in (abi.WRAP_PERIODIC, abi.WRAP_CLAMP, abi.WRAP_BLACK)]
    texs.append(scenes.TextureDesc(images[0], abi.TEX_LINEAR, abi.WRAP_BLACK, abi.WRAP_PERIODIC))
    sc = scenes.cornell(16, 16)
    base = len(sc.materials)
    glass = scenes.glass(1.45, 0.0, (0.95, 0.98, 0.95), (1.0, 1.0, 1.0)).lobes
    for k in range(len(texs)):
        j = (k + 5) % len(texs)
        sc.materials.append(scenes.MaterialDesc([  # mask only
            L(abi.LOBE_DIFFUSE, (0.8, 0.7, 0.6), fac_mode=abi.FAC_TEX_A, pre_weight=(0.9, 0.5, 0.3), fac_texture=k + 1),
            L(abi.LOBE_MICROFACET, (0.5, 0.4, 0.3), xalpha=0.09, yalpha=0.09, fac_mode=abi.FAC_TEX_B, pre_weight=(0.9, 0.5, 0.3), fac_texture=k + 1)]))
        sc.materials.append(scenes.MaterialDesc([  # mask + colour texture, beside a constant lobe
            L(abi.LOBE_TRANSPARENT, (1.0, 1.0, 1.0), fac_mode=abi.FAC_TEX_A, fac_texture=k + 1),
            L(abi.LOBE_SHEEN, (0.2, 0.2, 0.2), r=0.4),
            L(abi.LOBE_DIFFUSE, (0.7, 0.9, 0.8), fac_mode=abi.FAC_TEX_B, texture=j + 1, fac_texture=k + 1)]))
    # Fresnel lobes and masked lobes side by side, and the same glass lobes alone
    sc.materials.append(scenes.MaterialDesc(copy.deepcopy(glass) + copy.deepcopy(sc.materials[base].lobes)))
    sc.materials.append(scenes.MaterialDesc(copy.deepcopy(glass)))
    sc.textures = texs
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2))
    try:
        with pytest.raises(xpu.DeviceError) as e:
            dev.lobe_weights(0, np.zeros((1, 3), F), np.zeros((1, 3), F), np.zeros((1, 2), F))
        assert "(4)" in str(e.value)  # PHX_ERR_STATE before preprocess
        dev.preprocess(sc)
        with pytest.raises(xpu.DeviceError) as e:
            dev.lobe_weights(len(sc.materials), np.zeros((1, 3), F), np.zeros((1, 3), F), np.zeros((1, 2), F))
        assert "(1)" in str(e.value)  # PHX_ERR_ARG
        for hook in (lambda: dev.bsdf_f(base, np.zeros((1, 3), F), np.zeros((1, 3), F), np.zeros((1, 3), F)),
                     lambda: dev.bsdf_sample(base, np.zeros((1, 3), F), np.zeros((1, 3), F), np.zeros((1, 2), F))):
            with pytest.raises(xpu.DeviceError) as e:  # the hooks without (s, t) cannot resolve a mask
                hook()
            assert "(1)" in str(e.value)
        dropped = 0
        for k, tex in enumerate(texs):
            H, W = tex.texels.shape[:2]
            centres = np.stack(np.meshgrid((np.arange(-W, 2 * W) + F(0.5)) / F(W), (np.arange(-H, 2 * H) + F(0.5)) / F(H)), -1).reshape(-1, 2)
            edges = np.stack(np.meshgrid(np.arange(-W, 2 * W + 1) / F(W), np.arange(-H, 2 * H + 1) / F(H)), -1).reshape(-1, 2)
            st = np.concatenate([rng.uniform(0.0, 1.0, (20_000, 2)), rng.uniform(-3.0, 3.0, (20_000, 2)), centres, edges]).astype(F)
            n, wi = _unit(rng, len(st)), _unit(rng, len(st))
            for mi in (base + 2 * k, base + 2 * k + 1):
                m = sc.materials[mi]
                got, kept = dev.lobe_weights(mi, n, wi, st)
                assert got.shape == (len(st), abi.MAX_LOBES, 3) and not got[:, len(m.lobes):].any()
                want_kept = np.zeros(len(st), np.uint32)
                for i, l in enumerate(m.lobes):
                    if l.fac_mode == abi.FAC_NONE:
                        w, there = np.broadcast_to(np.array(l.weight, F), (len(st), 3)), np.ones(len(st), bool)
                    else:
                        w, there = np_masked_weight(l, texs, st)
                    assert bits_equal(got[:, i], w), (mi, i, tex.filter, tex.swrap)
                    want_kept |= there.astype(np.uint32) << np.uint32(i)
                    dropped += int((~there).sum())
                assert np.array_equal(kept, want_kept), (mi, tex.filter, tex.swrap)
        assert dropped > 1000  # the black-and-white image and the BLACK wrap do drop lobes
        # Fresnel lobes are what they are without a mask beside them; the masked lobes behind them are what they are alone
        st = rng.uniform(-1.0, 2.0, (50_000, 2)).astype(F)
        n, wi = _unit(rng, len(st)), _unit(rng, len(st))
        both, kb = dev.lobe_weights(len(sc.materials) - 2, n, wi, st)
        alone, ka = dev.lobe_weights(len(sc.materials) - 1, n, wi, st)
        masked, km = dev.lobe_weights(base, n, wi, st)
        assert bits_equal(both[:, :2], alone[:, :2]) and bits_equal(both[:, 2:4], masked[:, :2])
        assert np.array_equal(kb & 3, ka) and np.array_equal(kb >> 2, km)
        assert np.isfinite(alone[:, :2]).all() and (alone[:, :2] != 0).any() and len(np.unique(alone[:, 0, 0])) > 1000  # the factor does depend on the hit
    finally:
        dev.close()


def test_lobe_weights_of_a_scene_without_images(xpu):
    """untextured scenes take st as unused: constant lobes come back as baked, glass lobes as with any st"""
    from phosphorus_mk2_amd import scenes
    sc = scenes.glass_blobs(16, 16)
    rng = np.random.default_rng(4)
    n, wi = _unit(rng, 4096), _unit(rng, 4096)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2))
    try:
        dev.preprocess(sc)
        a, ka = dev.lobe_weights(1, n, wi)
        b, kb = dev.lobe_weights(1, n, wi, rng.uniform(-5, 5, (4096, 2)).astype(F))
        assert bits_equal(a, b) and np.array_equal(ka, kb) and (a[:, :2] != 0).any() and not a[:, 2:].any()
        c, kc = dev.lobe_weights(0, n, wi)
        m = sc.materials[0]
        assert all(bits_equal(c[:, i], np.broadcast_to(np.array(l.weight, F), (4096, 3))) for i, l in enumerate(m.lobes))
        assert (kc == (1 << len(m.lobes)) - 1).all()
    finally:
        dev.close()


# ---- 5. the masked atlas against the oracle ----------------------------------------------------------------------------------------------
# (H 3, W 4) CLOSEST mask: luminances exactly 0 (black), exactly 1 (white), greys that come back exactly and coloured texels in between
MASK43 = np.array([[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.25, 0.25, 0.25], [0.9, 0.2, 0.1]],
                   [[0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [0.1, 0.8, 0.2], [1.0, 1.0, 1.0]],
                   [[0.75, 0.75, 0.75], [0.3, 0.9, 0.9], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]], F)
COLOUR43 = np.array([[[0.9, 0.2, 0.1], [0.1, 0.8, 0.2], [0.2, 0.3, 0.9], [0.7, 0.7, 0.2]],
                     [[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.9, 0.5, 0.7], [0.3, 0.9, 0.9]],
                     [[0.6, 0.1, 0.8], [0.95, 0.9, 0.85], [0.25, 0.6, 0.4], [0.8, 0.4, 0.3]]], F)  # texel (1, 0) is black


def test_the_atlas_holds_the_luminances_the_cases_need():
    lum = np_luminance(MASK43)
    assert (lum == 0).sum() == 3 and (lum == 1).sum() == 3 and ((lum > 0) & (lum < 1)).sum() == 6
    assert lum[0, 2] == F(0.25) and lum[1, 0] == F(0.5) and lum[2, 0] == F(0.75)


def atlas_box(per_vertex=True, nx=8, ny=6, width=64, height=48, lens=False):
    """(masked scene, baked scene): the Cornell box whose back wall is a grid of nx x ny quads, each quad's UV triangles strictly inside
    one texel of MASK43 / COLOUR43 (both CLOSEST, both 4 x 3).  Materials by quad: mix(diffuse, glossy, mask) under a constant weight;
    mix(transparent, diffuse, mask), a cut-out; a masked mix whose diffuse side carries a colour texture.  The baked scene has the same
    face sets in the same order, each with the material its texels give, FAC_NONE."""
    from phosphorus_mk2_amd import abi, scenes
    L = scenes.LobeDesc
    box = scenes.cornell(width, height)
    back = box.meshes.pop(2)
    assert back.vertices[:, 2].max() == -3.5
    pre = (0.9, 0.8, 0.7)
    masked = [scenes.MaterialDesc([L(abi.LOBE_DIFFUSE, (0.8, 0.75, 0.7), fac_mode=abi.FAC_TEX_A, pre_weight=pre, fac_texture=1),
                                   L(abi.LOBE_MICROFACET, (0.6, 0.6, 0.6), xalpha=0.09, yalpha=0.09, fac_mode=abi.FAC_TEX_B, pre_weight=pre, fac_texture=1)]),
              scenes.MaterialDesc([L(abi.LOBE_TRANSPARENT, (1.0, 1.0, 1.0), fac_mode=abi.FAC_TEX_A, fac_texture=1),
                                   L(abi.LOBE_DIFFUSE, (0.7, 0.8, 0.7), fac_mode=abi.FAC_TEX_B, fac_texture=1)]),
              scenes.MaterialDesc([L(abi.LOBE_DIFFUSE, (0.9, 0.9, 0.9), fac_mode=abi.FAC_TEX_A, texture=2, fac_texture=1),
                                   L(abi.LOBE_REFLECTION, (0.8, 0.8, 0.8), fac_mode=abi.FAC_TEX_B, fac_texture=1)])]
    base = len(box.materials)
    mats_t = box.materials + masked
    mats_b = list(box.materials)
    verts, faces, uvs, sets_t, sets_b, cases = [], [], [], [], [], set()
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
            uvs += corner if per_vertex else [corner[0], corner[1], corner[2], corner[0], corner[2], corner[3]]
            k = (qx // 4 + 2 * (qy // 3)) % len(masked)  # every texel meets every material (nx = 8, ny = 6: each texel is on four quads)
            lum, lobes = np_luminance(MASK43[j, i]), [l.type for l in resolve(masked[k], MASK43[j, i], COLOUR43[j, i]).lobes]
            cases.add((k, "black" if lum == 0 else "white" if lum == 1 else "between", tuple(lobes)))
            sets_t.append((base + k, np.array([f, f + 1], np.uint32)))
            mats_b.append(resolve(masked[k], MASK43[j, i], COLOUR43[j, i]))
            sets_b.append((len(mats_b) - 1, np.array([f, f + 1], np.uint32)))
    flags = abi.MESH_NORMALS_PER_VERTEX | (abi.MESH_UV_PER_VERTEX if per_vertex else 0)
    grid_t = scenes.MeshDesc(np.array(verts, F), np.array(faces, np.uint32), sets_t, flags=flags, uvs=np.array(uvs, F))
    grid_b = scenes.MeshDesc(np.array(verts, F), np.array(faces, np.uint32), sets_b, flags=flags)
    st = scenes.SceneDesc(box.meshes[:2] + [grid_t] + box.meshes[2:], mats_t, box.camera,
                          textures=[scenes.TextureDesc(MASK43, abi.TEX_CLOSEST), scenes.TextureDesc(COLOUR43, abi.TEX_CLOSEST)])
    sb = scenes.SceneDesc(box.meshes[:2] + [grid_b] + box.meshes[2:], mats_b, scenes.CameraDesc(width, height, box.camera.fov))
    if lens:
        for s in (st, sb):
            s.camera.aperture_radius, s.camera.focal_distance = 0.03, 3.0
    # every case is on the wall: each material with B dropped by luminance 0, with A dropped by luminance 1 and with both sides kept, and
    # the textured diffuse side dropped by its black colour texel under a mask that keeps it
    for k, m in enumerate(masked):
        ta, tb = m.lobes[0].type, m.lobes[1].type
        assert {(k, "black", (ta,)), (k, "white", (tb,)), (k, "between", (ta, tb))} <= cases, (k, sorted(cases))
    assert (2, "between", (abi.LOBE_REFLECTION,)) in cases
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
def test_closest_mask_texels_match_the_baked_oracle_scene(xpu, orc, per_vertex, flight, lens):
    st, sb = atlas_box(per_vertex, lens=lens)
    film, s = _compare_with_oracle(xpu, orc, st, sb, spp=16, seed=5, samples_in_flight=flight)
    assert s["shade_general"] == 1


# ---- 6. an all-black mask is A alone, an all-white one B alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0.0, 1.0])
def test_a_uniform_black_or_white_mask_is_one_side_alone(xpu, level):
    from phosphorus_mk2_amd import abi, scenes
    L = scenes.LobeDesc
    A = [L(abi.LOBE_DIFFUSE, (0.73, 0.73, 0.73)), L(abi.LOBE_SHEEN, (0.2, 0.1, 0.3), r=0.4)]
    B = [L(abi.LOBE_MICROFACET, (0.8, 0.7, 0.3), xalpha=0.09, yalpha=0.09)]
    rng = np.random.default_rng(8)
    masked, plain = scenes.cornell(64, 64), scenes.cornell(64, 64)
    for m in masked.meshes:
        m.uvs = rng.uniform(-2.0, 2.0, (len(m.vertices), 2)).astype(F)
    masked.textures = [scenes.TextureDesc(np.full((3, 5, 3), level, F), abi.TEX_LINEAR)]
    masked.materials[0] = scenes.MaterialDesc([copy.deepcopy(l) for l in A + B])
    for l in masked.materials[0].lobes[:2]:
        l.fac_mode, l.fac_texture = abi.FAC_TEX_A, 1
    masked.materials[0].lobes[2].fac_mode, masked.materials[0].lobes[2].fac_texture = abi.FAC_TEX_B, 1
    plain.materials[0] = scenes.MaterialDesc(copy.deepcopy(A if level == 0.0 else B))
    fm, sm = xpu.render(masked, spp=16, pps=1, depth=9, seed=4)
    fp, sp = xpu.render(plain, spp=16, pps=1, depth=9, seed=4)
    assert (sm["rays_closest"], sm["rays_shadow"], sm["rays_masked"]) == (sp["rays_closest"], sp["rays_shadow"], sp["rays_masked"])
    assert np.isfinite(fm).all() and fm[..., :3].max() > 0.05 and bits_equal(fm, fp)


# ---- 7. the closure zoo under a constant LINEAR mask -------------------------------------------------------------------------------------
def test_constant_linear_mask_on_the_closure_zoo(xpu, orc):
    """every lobe of the 16 recipes under a masked mix whose image is constant (LINEAR / PERIODIC, random UVs): each lookup returns the
    constant bit for bit, so the film is the oracle's with the resolved weights"""
    from phosphorus_mk2_amd import abi, scenes
    st = scenes.multi_material_soup(3000, width=64, height=64)
    sb = scenes.multi_material_soup(3000, width=64, height=64)
    c = np.array([0.8, 0.6, 0.9], F)
    st.textures = [scenes.TextureDesc(np.broadcast_to(c, (5, 7, 3)).copy(), abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_PERIODIC)]
    rng = np.random.default_rng(3)
    for m in st.meshes:
        m.uvs = rng.uniform(-2.0, 2.0, (len(m.vertices), 2)).astype(F)
    n = 0
    for i, m in enumerate(st.materials):
        if m.is_emitter:
            continue
        for k, l in enumerate(m.lobes):
            assert l.fac_mode == abi.FAC_NONE
            l.fac_mode, l.fac_texture, l.pre_weight = (abi.FAC_TEX_B if (i + k) % 2 else abi.FAC_TEX_A), 1, (0.9, 0.8, 0.95)
            n += 1
        sb.materials[i] = resolve(m, c)
        assert len(sb.materials[i].lobes) == len(m.lobes)
    assert n >= 16
    _compare_with_oracle(xpu, orc, st, sb, spp=8, seed=2)


# ---- 8. scenes without masked or textured lobes are untouched --------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["zoo", "glass"])
def test_a_texture_table_without_a_masked_lobe_changes_nothing(xpu, scene):
    from phosphorus_mk2_amd import scenes
    make = (lambda: scenes.multi_material_soup(3000, width=64, height=48)) if scene == "zoo" else (lambda: scenes.glass_blobs(64, 48))
    a, b = make(), make()
    rng = np.random.default_rng(5)
    for m in b.meshes:
        m.uvs = rng.uniform(0.0, 1.0, (len(m.vertices), 2)).astype(F)
    b.textures = [scenes.TextureDesc(np.ones((2, 2, 3), F)), scenes.TextureDesc(np.zeros((1, 3, 3), F))]  # a table no lobe uses
    fa, sa = xpu.render(a, spp=8, pps=1, depth=9, seed=3)
    fb, sb_ = xpu.render(b, spp=8, pps=1, depth=9, seed=3)
    assert bits_equal(fa, fb) and sa["rays_closest"] == sb_["rays_closest"] and sa["rays_shadow"] == sb_["rays_shadow"]
    assert sa["shade_general"] == sb_["shade_general"] == 1
    assert sa["device_bytes"] == sb_["device_bytes"]  # neither the table nor the UVs were uploaded
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2))
    try:
        dev.preprocess(b)
        with pytest.raises(xpu.DeviceError):  # no table on the device: the lookup hook has nothing to read
            dev.texture_lookup(0, np.zeros((1, 2), F))
    finally:
        dev.close()


def test_a_masked_scene_counts_its_table_in_device_bytes(xpu):
    from phosphorus_mk2_amd import abi, scenes
    stats = []
    for size in (1, 64):  # a mask-only scene (no colour texture anywhere) uploads the table: 16 bytes per texel
        sc = scenes.cornell(32, 32)
        sc.textures = [scenes.TextureDesc(np.full((size, size, 3), 0.5, F))]
        sc.materials[0].lobes[0].fac_mode, sc.materials[0].lobes[0].fac_texture = abi.FAC_TEX_A, 1
        stats.append(xpu.render(sc, spp=1, pps=1, depth=3, seed=1)[1])
    assert stats[1]["device_bytes"] == stats[0]["device_bytes"] + (64 * 64 - 1) * 16 and stats[0]["shade_general"] == stats[1]["shade_general"] == 1


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def test_bad_mask_inputs_are_refused_and_the_device_stays_usable(xpu):
    from phosphorus_mk2_amd import abi, scenes
    good = scenes.cornell(32, 32)
    good.textures = [scenes.TextureDesc(MASK43, abi.TEX_LINEAR)]
    good.meshes[0].uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)
    good.materials[0].lobes[0].fac_mode, good.materials[0].lobes[0].fac_texture = abi.FAC_TEX_A, 1
    masked = lambda: scenes.LobeDesc(abi.LOBE_DIFFUSE, (1, 1, 1), fac_mode=abi.FAC_TEX_B, fac_texture=1)

    def index_zero(s):
        s.materials[1].lobes[0].fac_mode, s.materials[1].lobes[0].fac_texture = abi.FAC_TEX_B, 0

    def index_past_the_table(s):
        s.materials[1].lobes[0].fac_mode, s.materials[1].lobes[0].fac_texture = abi.FAC_TEX_A, 2

    def upper_bits_without_a_tex_mode(s):
        s.materials[1].lobes[0].fac_mode, s.materials[1].lobes[0].fac_texture = abi.FAC_MIX_B, 1

    def upper_bits_on_fac_none(s):
        s.materials[1].lobes[0].fac_mode, s.materials[1].lobes[0].fac_texture = abi.FAC_NONE, 1

    def unknown_mode(s):
        s.materials[1].lobes[0].fac_mode, s.materials[1].lobes[0].fac_texture = 5, 1

    def unknown_mode_without_index(s):
        s.materials[1].lobes[0].fac_mode = 255

    def on_emitter(s):
        s.materials[3].lobes = [masked()]

    def on_environment(s):
        s.materials.append(scenes.MaterialDesc([masked()], emission=(0.1, 0.1, 0.1)))
        s.environment_material = len(s.materials) - 1

    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=4, paths_per_sample=1, path_depth=9))
    try:
        def frame():
            film = xpu.Film(32, 32, 4)
            dev.start(good, xpu.FrameState(1, xpu.Tiles.make(32, 32, 32), film)); dev.join()
            return film.data.copy()
        dev.preprocess(good)
        ref = frame()
        assert ref[..., :3].max() > 0.05
        assert good.materials[3].is_emitter
        for bad in (index_zero, index_past_the_table, upper_bits_without_a_tex_mode, upper_bits_on_fac_none, unknown_mode, unknown_mode_without_index,
                    on_emitter, on_environment):
            s = copy.deepcopy(good)
            bad(s)
            with pytest.raises(xpu.DeviceError) as e:
                dev.preprocess(s)
            assert "(1)" in str(e.value) and len(str(e.value).split(":", 1)[1].strip()) > 5, bad.__name__  # PHX_ERR_ARG with a message
            dev.preprocess(good)
            assert bits_equal(frame(), ref), bad.__name__
    finally:
        dev.close()
