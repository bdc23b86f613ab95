"""Every shade kernel on a scene that selects it.  launch_shade (shade_general.hip) picks one of 36 instantiations -- 12 families (k_shade<2>,
k_shade<1> and k_shade_g with PERHIT / TEX / ENV / MASK) times the pass (a later bounce, camera rays through a pinhole, camera rays
through a lens) -- and phx_stats::shade_kernels names the ones a frame launched.  One table: each family on a pinhole and on a lens
camera, each case against the CPU oracle's film of the same scene with its images baked in (the oracle knows neither textures nor
masks nor environment images), bit for bit, with the launched kernels pinned exactly and every feature of the family shown to reach the
film.  No comparison here carries a tolerance."""
import copy

import numpy as np
import pytest

from conftest import aim_camera, bits_equal
from phosphorus_mk2_amd import abi, scenes
from test_gpu_environment import BH, BW, _blocks, _far_geometry, _with_constant_env, _with_env, np_env_st, open_box
from test_gpu_masks import atlas_box
from test_gpu_parity import _with_lens
from test_gpu_textures import grid_box

F = np.float32
W, H, SPP, DEPTH, SEED = 64, 48, 16, 9, 5
LENS = (0.03, 3.0)  # aperture radius, focal distance
# The environment image is constant: emission x texel is the oracle's constant environment, exact in fp32 (powers of two).  The image is the
# LAST texture of its scene and its texel occurs in no other one: a kernel that read env_tex or a lobe's texture from the wrong slot changes
# the film.
ENV_EMISSION, ENV_TEXEL = np.array([2.0, 0.5, 4.0], F), np.array([0.125, 3.0, 0.1875], F)
ENV = ENV_EMISSION * ENV_TEXEL
assert ENV.tolist() == [0.25, 1.5, 0.75]
SEEN_FRACTION = 0.25  # an environment counts as seen when it changes at least a quarter of the film's pixels


def _lambert_soup():
    """several Lambert lobes on one material and nothing but Lambert lobes: sc.diffuse_only == 1"""
    D = abi.LOBE_DIFFUSE
    mats = [scenes.MaterialDesc([scenes.LobeDesc(D, (0.4, 0.3, 0.2)), scenes.LobeDesc(D, (0.2, 0.3, 0.4))]), scenes.diffuse(0.73, 0.73, 0.73)]
    return scenes.soup(3000, width=W, height=H, materials=mats)


def _same(sc):
    return sc, copy.deepcopy(sc)


# base scene -> (the device's scene, the oracle's scene with the images baked in)
BASES = {
    "cornell": lambda: _same(scenes.cornell(W, H)),
    "lambert_soup": lambda: _same(_lambert_soup()),
    "zoo_soup": lambda: _same(scenes.multi_material_soup(3000, width=W, height=H)),
    "glass_blobs": lambda: _same(scenes.glass_blobs(W, H)),
    "open_box": lambda: _same(open_box(W, H)),
    "grid": lambda: grid_box(True, width=W, height=H, glass=False),
    "grid_glass": lambda: grid_box(True, width=W, height=H),
    "atlas": lambda: atlas_box(True, width=W, height=H),
}
# 1-based index of the colour image / the mask image in the base's textures
COLOUR_TEXTURE = {"grid": 1, "grid_glass": 1, "atlas": 2}
MASK_TEXTURE = {"atlas": 1}
G = abi.SHADE_FAMILY_GENERAL
PERHIT, TEX, ENVF = abi.SHADE_G_PERHIT, abi.SHADE_G_TEX, abi.SHADE_G_ENV
# name: (family, base scene, with the environment image, the features whose removal must change the film)
FAMILIES = {
    "lambert1": (abi.SHADE_FAMILY_LAMBERT1, "cornell", False, ()),                               # k_shade<2>
    "lambert": (abi.SHADE_FAMILY_LAMBERT, "lambert_soup", False, ()),                            # k_shade<1>
    "general": (G, "zoo_soup", False, ()),                                                       # k_shade_g<false>
    "perhit": (G + PERHIT, "glass_blobs", False, ()),                                            # k_shade_g<true>
    "tex": (G + TEX, "grid", False, ("texture",)),
    "tex_perhit": (G + (TEX | PERHIT), "grid_glass", False, ("texture",)),
    "env": (G + ENVF, "open_box", True, ("environment",)),
    "env_perhit": (G + (ENVF | PERHIT), "glass_blobs", True, ("environment",)),
    "env_tex": (G + (ENVF | TEX), "grid", True, ("environment", "texture")),
    "env_tex_perhit": (G + (ENVF | TEX | PERHIT), "grid_glass", True, ("environment", "texture")),
    "mask": (abi.SHADE_FAMILY_MASK, "atlas", False, ("mask", "texture")),
    "mask_env": (abi.SHADE_FAMILY_MASK_ENV, "atlas", True, ("environment", "mask", "texture")),
}
CASES = [(name, lens) for name in FAMILIES for lens in (False, True)]


def family_flags(family):
    """the template flags of a family, by the layout include/phx_xpu.h states"""
    if family < G:
        return set()
    if family >= abi.SHADE_FAMILY_MASK:
        return {"perhit", "texture", "mask"} | ({"environment"} if family == abi.SHADE_FAMILY_MASK_ENV else set())
    return {n for n, b in (("perhit", PERHIT), ("texture", TEX), ("environment", ENVF)) if (family - G) & b}


def expected_kernels(family, lens):
    """a frame of depth 9 launches the family's camera-ray kernel (its lens twin under a lens) once per pass and its later-bounce kernel
    for every further step, and nothing else"""
    first = abi.SHADE_PASS_LENS if lens else abi.SHADE_PASS_CAMERA
    return (1 << abi.shade_kernel_bit(family, first)) | (1 << abi.shade_kernel_bit(family, abi.SHADE_PASS_LATER))


def test_the_table_reaches_every_shade_kernel():
    """CPU only: the union of the table's expected bits is all of phx_stats::shade_kernels' 36.  An instantiation added to launch_shade
    (PHX_SHADE_KERNELS grows with it) without a case here fails this test."""
    assert len(FAMILIES) == abi.SHADE_FAMILIES and sorted(f[0] for f in FAMILIES.values()) == list(range(abi.SHADE_FAMILIES))
    union, total = 0, 0
    for name, lens in CASES:
        bits = expected_kernels(FAMILIES[name][0], lens)
        assert bin(bits).count("1") == 2
        union |= bits
        total += 1
    missing = ((1 << abi.SHADE_KERNELS) - 1) & ~union
    assert union == (1 << abi.SHADE_KERNELS) - 1, f"no case for {abi.shade_kernel_names(missing)}"
    assert total == 2 * abi.SHADE_FAMILIES
    for name, (family, base, env, features) in FAMILIES.items():  # the table's scenes and features are the family's
        flags = family_flags(family)
        assert env == ("environment" in flags) == ("environment" in features), name
        assert ("texture" in flags) == ("texture" in features) == (base in COLOUR_TEXTURE), name
        assert ("mask" in flags) == ("mask" in features) == (base in MASK_TEXTURE), name
        assert ("perhit" in flags) == (base in ("glass_blobs", "grid_glass", "atlas")), name


def _decoys():
    """two images no lobe reads, in front of the environment image of a scene without textures: the image is then texture 3, not 1"""
    return [scenes.TextureDesc(np.full((1, 1, 3), (0.9, 0.1, 0.4), F)), scenes.TextureDesc(np.full((2, 3, 3), (0.4, 0.7, 5.0), F))]


def build(name, lens, without=None):
    """(the device's scene, the oracle's scene) of family `name`; `without` removes one feature from the device's scene: no environment,
    the colour image white, the mask image a constant 0.5, or the lens closed"""
    family, base, env, features = FAMILIES[name]
    assert without is None or without == "lens" or without in features
    st, sb = BASES[base]()
    if without == "texture":
        t = st.textures[COLOUR_TEXTURE[base] - 1]
        t.texels = np.ones_like(t.texels)
    if without == "mask":
        t = st.textures[MASK_TEXTURE[base] - 1]
        t.texels = np.full_like(t.texels, 0.5)
    if env and without != "environment":
        if not st.textures:
            st.textures = _decoys()
        st = _with_env(st, np.broadcast_to(ENV_TEXEL, (2, 4, 3)).copy(), ENV_EMISSION)
        assert st.materials[st.environment_material].emission_texture == len(st.textures) >= 2
        assert all((t.texels != ENV_TEXEL).any(-1).all() for t in st.textures[:-1])
        sb = _with_constant_env(sb, ENV)
    if lens and without != "lens":
        for s in (st, sb):
            _with_lens(s, *LENS)
    assert not sb.textures  # the oracle reads no image
    return st, sb


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


@pytest.fixture(scope="module")
def device_film(xpu):
    """device films by (family, lens, removed feature), each rendered once; the same film under two keys (a family without its
    environment is another family's case) is rendered twice: a device frame takes milliseconds"""
    done = {}

    def get(name, lens, without=None):
        key = (name, False, None) if without == "lens" else (name, lens, without)  # the lens closed: the family's pinhole case
        if key not in done:
            done[key] = xpu.render(build(name, lens, without)[0], spp=SPP, pps=1, depth=DEPTH, seed=SEED)
        return done[key]
    return get


@pytest.fixture(scope="module")
def oracle_film(orc):
    """oracle films by (base scene, environment, lens), each rendered once, under the device's tie rule (the grids' quads share edges: of
    two triangles met at bitwise the same distance the lower primitive index wins)"""
    orc.set_tie_rule(1)
    done = {}

    def get(name, lens, without=None):
        family, base, env, _ = FAMILIES[name]
        assert without in (None, "environment")
        key = (base, env and without is None, lens)
        if key not in done:
            done[key] = orc.Oracle(build(name, lens, without)[1], spp=SPP, pps=1, depth=DEPTH).render(rng=orc.RNG_COUNTER, seed=SEED, threads=8)
        return done[key]
    yield get
    orc.set_tie_rule(0)


def _pixels_differing(a, b):
    return float((a[..., :3].view(np.uint32) != b[..., :3].view(np.uint32)).any(-1).mean())


def _check_kernels(st, family, lens):
    got, want = st["shade_kernels"], expected_kernels(family, lens)
    return [] if got == want else [f"launched {abi.shade_kernel_names(got)}, expected {abi.shade_kernel_names(want)}"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,lens", CASES, ids=[f"{n}-{'lens' if l else 'pinhole'}" for n, l in CASES])
def test_family_matches_the_baked_oracle_scene(device_film, oracle_film, name, lens):
    """Every check of a case is made before any is reported, so that one wrong dispatch shows both as the kernel's name and as the film it
    spoils."""
    family, base, env, features = FAMILIES[name]
    film, st = device_film(name, lens)
    ref, ost = oracle_film(name, lens)
    rgb = np.ascontiguousarray(film[..., :3])
    failed = _check_kernels(st, family, lens)
    for k in ("camera_samples", "rays_closest", "rays_shadow", "rays_masked"):
        if st[k] != ost[k]:
            failed.append(f"{k}: {st[k]}, the oracle's {ost[k]}")
    if not (np.isfinite(film).all() and np.isfinite(ref[..., :3]).all()):
        failed.append("the film is not finite")
    if not rgb.max() > 0.05:
        failed.append(f"the film is dark: max {rgb.max()}")
    if not bits_equal(rgb, ref[..., :3]):
        failed.append(f"the film differs from the oracle's in {_pixels_differing(film, ref):.1%} of the pixels")
    # every feature of the family reaches the film
    for feature in features + (("lens",) if lens else ()):
        other, ost_ = device_film(name, lens, feature)
        changed = _pixels_differing(film, other)
        print(f"{name} lens={lens}: without its {feature} {changed:.1%} of the pixels change")
        if feature == "environment":
            oracle_changed = _pixels_differing(ref, oracle_film(name, lens, feature)[0])
            if not (changed >= SEEN_FRACTION and oracle_changed >= SEEN_FRACTION):
                failed.append(f"the environment changes {changed:.1%} of the pixels ({oracle_changed:.1%} of the oracle's), not {SEEN_FRACTION:.0%}")
        elif not changed > 0:
            failed.append(f"the film is the same without its {feature}")
    assert not failed, f"{name}, {'lens' if lens else 'pinhole'}:\n" + "\n".join(failed)


# ---- a non-constant image through the MASK + ENV camera kernels ---------------------------------------------------------------------------
def _masked_far_geometry():
    """test_gpu_environment.py's far geometry (no view below reaches it) with an image mask on its walls: the scene's flags select
    MASK + ENV, and every camera ray takes the miss branch.  The mask is texture 1, the environment's blocks texture 2."""
    sc = _far_geometry()
    sc.textures = [scenes.TextureDesc(np.full((1, 1, 3), 0.5, F), abi.TEX_CLOSEST)]
    L = scenes.LobeDesc
    sc.materials[0] = scenes.MaterialDesc([L(abi.LOBE_DIFFUSE, (0.73, 0.73, 0.73), fac_mode=abi.FAC_TEX_A, fac_texture=1),
                                           L(abi.LOBE_MICROFACET, (0.6, 0.6, 0.6), xalpha=0.09, yalpha=0.09, fac_mode=abi.FAC_TEX_B, fac_texture=1)])
    return sc


def blocks_seen(orc, base, mapping, spp, seed):
    """(good, block): the pixels all of whose camera rays (the camera model's, from the oracle: pinhole or lens) map inside one CLOSEST
    block of the BW x BH image, at least 2e-3 from its edges in s and t, and that block's index"""
    w, h = base.camera.width, base.camera.height
    O = orc.Oracle(base, spp=spp, pps=1, depth=DEPTH)
    block = np.full(w * h, -1); good = np.ones(w * h, bool)
    for s in range(spp):
        o, d = O.camera_rays((0, 0, w, h), s, seed=seed)
        st, ok = np_env_st(d, mapping)
        st = st.astype(np.float64)
        x, y = st[:, 0] * BW, st[:, 1] * BH
        i, j = np.floor(x) % BW, np.floor(y)
        margin = 2e-3 * np.array([BW, BH])
        inside = ok & (x - np.floor(x) > margin[0]) & (np.ceil(x) - x > margin[0]) & (y - np.floor(y) > margin[1]) & (np.ceil(y) - y > margin[1])
        k = (j * BW + i).astype(np.int64)
        good &= inside & ((block < 0) | (block == k))
        block = np.where(good, k, -1)
    return good, block


@pytest.mark.gpu
@pytest.mark.parametrize("mapping,yaw,pitch,lens", [(0, 2.2, -0.3, False), (1, -0.8, 0.5, True)])
def test_mask_env_camera_kernels_see_the_right_block(xpu, orc, mapping, yaw, pitch, lens):
    """test_gpu_environment.py::test_camera_sees_the_right_block through k_shade_g<true, true, LENS, true, true, true>: a pixel whose
    every camera ray maps inside one block has the oracle's film value under that block's colour as the constant environment"""
    w = h = 32
    spp, seed = 8, 2
    img = _blocks()
    plain = aim_camera(_far_geometry(), yaw, pitch)
    masked = aim_camera(_masked_far_geometry(), yaw, pitch)
    if lens:
        _with_lens(plain, *LENS); _with_lens(masked, *LENS)
    sc = _with_env(masked, img, (1.0, 1.0, 1.0), mapping, abi.TEX_CLOSEST)
    assert sc.materials[sc.environment_material].emission_texture == 2
    film, st = xpu.render(sc, spp=spp, pps=1, depth=DEPTH, seed=seed)
    failed = _check_kernels(st, abi.SHADE_FAMILY_MASK_ENV, lens)
    good, block = blocks_seen(orc, plain, mapping, spp, seed)
    assert good.sum() >= w * h // 3 and len(np.unique(block[good])) >= 3, (good.sum(), np.unique(block[good]))
    got = film[..., :3].reshape(-1, 3)
    for k in np.unique(block[good]):
        ref, ost = orc.Oracle(_with_constant_env(plain, img[k // BW, k % BW]), spp=spp, pps=1, depth=DEPTH).render(rng=orc.RNG_COUNTER, seed=seed, threads=8)
        sel = good & (block == k)
        if (st["rays_closest"], st["rays_shadow"], st["rays_masked"]) != (ost["rays_closest"], ost["rays_shadow"], ost["rays_masked"]):
            failed.append(f"block {k}: ray counts {st['rays_closest']}, {st['rays_shadow']}, {st['rays_masked']} are not the oracle's")
        assert ost["rays_closest"] == w * h * spp and ost["rays_shadow"] == 0  # every camera ray misses and ends its path
        if not bits_equal(got[sel], ref[..., :3].reshape(-1, 3)[sel]):
            failed.append(f"block {k} ({img[k // BW, k % BW]}): {(got[sel] != ref[..., :3].reshape(-1, 3)[sel]).any(1).sum()} of {sel.sum()} pixels differ")
    assert not failed, "\n".join(failed)
