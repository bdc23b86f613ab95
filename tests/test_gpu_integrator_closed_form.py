"""The device's integrator on the furnace scenes of tests/test_integrator_closed_form.py, checked on two counts: film and ray counts are
bit-equal to the CPU oracle's (under the device's tie rule), and both are within the CPU file's tolerances of the float64 model
(tests/integrator64.py) -- the recorded standard errors, never a spread of the device's own film -- so that this file stands on its own.

The cavity's answer depends neither on the camera nor on the kernel that shades it, so one scene reaches every shade path (launch_shade,
shade_general.hip); each case's docstring entry names the DevScene state that selects it."""
import copy
from dataclasses import replace

import numpy as np
import pytest

import integrator64 as I
import test_integrator_closed_form as T
from conftest import bits_equal
from phosphorus_mk2_amd import abi, scenes

pytestmark = pytest.mark.gpu

RHO, DEPTH = "colour", 5  # two rounds of roulette


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


@pytest.fixture(scope="module")
def oracle(orc):
    """oracle films by key, each rendered once, with the device's tie rule (a ray through a shared edge of the sphere meets two facets
    at bitwise the same distance)"""
    orc.set_tie_rule(1)
    done = {}

    def get(key, make, depth, spp=T.SPP):
        if key not in done:
            film, st = orc.Oracle(make(), spp=spp, pps=1, depth=depth).render(rng=orc.RNG_COUNTER, seed=T.SEED, threads=8)
            done[key] = (film, st)
        return done[key]
    yield get
    orc.set_tie_rule(0)


def device(xpu, sc, depth, spp=T.SPP, **kw):
    return xpu.render(sc, spp=spp, pps=1, depth=depth, seed=T.SEED, **kw)


def same(film, st, ref, ost):
    for k in ("camera_samples", "rays_closest", "rays_shadow", "rays_masked"):
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert np.isfinite(film[..., :3]).all() and bits_equal(film[..., :3], ref[..., :3])


def f64(film):
    return film[..., :3].astype(np.float64)


def _lens(sc):
    sc.camera.aperture_radius, sc.camera.focal_distance = 0.05, 1.0
    return sc


def _env_image(sc, emission, texel, shape=(2, 4)):
    """sc with a constant lat-long image of `texel` on its (new or existing) environment material, emission x texel = the constant E"""
    sc = copy.deepcopy(sc)
    sc.textures = list(sc.textures) + [scenes.TextureDesc(np.full(shape + (3,), texel, np.float32), abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_CLAMP)]
    env = scenes.MaterialDesc([], tuple(emission), emission_texture=len(sc.textures), emission_mapping=abi.ENV_LATLONG_Y_UP)
    if sc.environment_material >= 0:
        sc.materials[sc.environment_material] = env
    else:
        sc.materials.append(env); sc.environment_material = len(sc.materials) - 1
    return sc


def _constant_env(sc, e):
    sc = copy.deepcopy(sc)
    sc.materials.append(scenes.MaterialDesc([], tuple(e))); sc.environment_material = len(sc.materials) - 1
    return sc


GGX, GLASS = scenes.closure_zoo()[4], scenes.glass()
HALF_4X4 = scenes.TextureDesc(np.full((4, 4, 3), 0.5, np.float32), abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_PERIODIC)
HALF_1X1 = scenes.TextureDesc(np.full((1, 1, 3), 0.5, np.float32), abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_PERIODIC)
TEXTURED = scenes.MaterialDesc([replace(GGX.lobes[0], texture=1)])
TEXTURED_GLASS = scenes.MaterialDesc([replace(GLASS.lobes[0], texture=1), GLASS.lobes[1]])
LAMBERT1, GENERAL = abi.SHADE_FAMILY_LAMBERT1, abi.SHADE_FAMILY_GENERAL


def K(family, lens=False):
    """the two kernels a frame of this family launches: the camera rays' (through a pinhole or a lens) and the later bounces'"""
    first = abi.SHADE_PASS_LENS if lens else abi.SHADE_PASS_CAMERA
    return (1 << abi.shade_kernel_bit(family, first)) | (1 << abi.shade_kernel_bit(family, abi.SHADE_PASS_LATER))


# name: (scene, the oracle's scene (None: the same; textures and environment images baked in), render options,
#        the shade kernels of the frame (phx_stats::shade_kernels: the instantiation the comment above the entry names and its later-bounce twin),
#        the standard error's key in SE_VARIANT (None: the plain cavity's, whose film this one must repeat bit for bit),
#        the key under which cases with the same oracle film share it)
CAVITIES = {
    # k_shade<2>: sc.diffuse_only == 2 (every material has at most one Lambert lobe, no textures)
    "plain": (lambda: I.cavity(), None, {}, K(LAMBERT1), None, "plain"),
    "plain_host_builder": (lambda: I.cavity(), None, {"bvh_builder": "host"}, K(LAMBERT1), None, "plain"),
    "plain_device_builder": (lambda: I.cavity(), None, {"bvh_builder": "device"}, K(LAMBERT1), None, "plain"),
    "plain_3_in_flight": (lambda: I.cavity(), None, {"samples_in_flight": 3}, K(LAMBERT1), None, "plain"),
    # k_shade<2, true, true>: the same with sc.aperture_radius != 0 on the camera rays' pass
    "plain_lens": (lambda: _lens(I.cavity()), None, {}, K(LAMBERT1, True), "lens", "lens"),
    # k_shade_g<false>: sc.diffuse_only == 0 (a GGX lobe exists), sc.any_per_hit == 0, sc.any_tex == 0
    "hidden_ggx": (lambda: I.cavity(hidden=GGX), None, {}, K(GENERAL), None, "hidden_ggx"),
    "hidden_ggx_3_in_flight": (lambda: I.cavity(hidden=GGX), None, {"samples_in_flight": 3, "bvh_builder": "host"}, K(GENERAL), None, "hidden_ggx"),
    # k_shade_g<false, true, true>: the thin lens on the general kernel
    "hidden_ggx_lens": (lambda: _lens(I.cavity(hidden=GGX)), None, {}, K(GENERAL, True), "lens", "hidden_ggx_lens"),
    # k_shade_g<true> (PERHIT): sc.any_per_hit == 1 (the glass node's Fresnel mix)
    "hidden_glass": (lambda: I.cavity(hidden=GLASS), None, {}, K(GENERAL + abi.SHADE_G_PERHIT), None, "hidden_glass"),
    # k_shade_g<false, ., ., true> (TEX): sc.any_tex & SC_TEX_LOBES -- the texture is on the hidden triangle; the device takes no textured lobe
    # on an emitter (phx_xpu.h), so the wall's rho cannot be split into weight x texel: test_lambert_floor_under_the_environment does that
    "texture_kernel": (lambda: I.cavity(hidden=TEXTURED, textures=[HALF_4X4]), lambda: I.cavity(hidden=GGX), {}, K(GENERAL + abi.SHADE_G_TEX), None, "hidden_ggx"),
    # k_shade_g<true, ., ., true> (PERHIT + TEX)
    "texture_kernel_per_hit": (lambda: I.cavity(hidden=TEXTURED_GLASS, textures=[HALF_4X4]), lambda: I.cavity(hidden=GLASS), {}, K(GENERAL + (abi.SHADE_G_TEX | abi.SHADE_G_PERHIT)), None, "hidden_glass"),
    # k_shade_g<false, ., ., false, true> (ENV): sc.any_tex & SC_TEX_ENV, an environment image that no path of the closed cavity sees
    "environment_image": (lambda: _env_image(I.cavity(), (8.0, 8.0, 8.0), 0.5), lambda: _constant_env(I.cavity(), (4.0, 4.0, 4.0)), {}, K(GENERAL + abi.SHADE_G_ENV), None, "constant_environment"),
    # k_shade_g<false, ., ., true, true> (TEX + ENV)
    "texture_kernel_and_environment_image": (lambda: _env_image(I.cavity(hidden=TEXTURED, textures=[HALF_4X4]), (8.0, 8.0, 8.0), 0.5),
                                             lambda: _constant_env(I.cavity(), (4.0, 4.0, 4.0)), {}, K(GENERAL + (abi.SHADE_G_TEX | abi.SHADE_G_ENV)), None, "constant_environment"),
    # a ragged film: 24 x 13 is one partial 32 x 32 tile (the oracle, like the reference, takes tile widths that are multiples of 8 only)
    "film_24x13": (lambda: I.cavity(width=24, height=13), None, {}, K(LAMBERT1), "film_24x13", "film_24x13"),
    "film_24x13_hidden_ggx": (lambda: I.cavity(width=24, height=13, hidden=GGX), None, {"samples_in_flight": 3}, K(GENERAL), "film_24x13", "film_24x13_hidden_ggx"),
}
# relative standard errors (r, g, b) of the film mean of the variants whose camera or film differs from the plain cavity's (colour, depth 5,
# 256 spp, seed 5), measured on the CPU oracle like SE_MEAN
SE_VARIANT = {
    "lens": (1.50e-03, 5.19e-04, 2.17e-04),
    "film_24x13": (1.40e-03, 4.75e-04, 2.09e-04),
}


@pytest.mark.parametrize("name", list(CAVITIES))
def test_cavity_on_every_shade_path(xpu, oracle, name):
    """The coloured cavity at depth 5 through each shade kernel.  The comment above each entry of CAVITIES names the instantiation and the
    DevScene state that selects it in launch_shade (shade_general.hip): sc.diffuse_only == 2 -> k_shade<2>; 0 -> k_shade_g, <PERHIT> with
    sc.any_per_hit, <TEX> / <ENV> with sc.any_tex & SC_TEX_LOBES / SC_TEX_ENV, the LENS twins with sc.aperture_radius != 0 on the camera
    rays' pass.  Stats' shade_kernels names the instantiations the frame launched: exactly the entry's two."""
    make, make_ref, opts, kernels, se_key, ref_key = CAVITIES[name]
    sc = make()
    film, st = device(xpu, sc, DEPTH, **opts)
    assert st["shade_kernels"] == kernels, (abi.shade_kernel_names(st["shade_kernels"]), abi.shade_kernel_names(kernels))
    assert st["shade_general"] == (0 if kernels in (K(LAMBERT1), K(LAMBERT1, True)) else 1)
    ref, ost = oracle(ref_key, make_ref or make, DEPTH)
    same(film, st, ref, ost)
    T.check_cavity(f64(film), st, RHO, 1, DEPTH, se=None if se_key is None else SE_VARIANT[se_key])
    if se_key is None:  # the hidden triangle, the texture and the unseen environment change no path: the plain cavity's film
        plain, _ = oracle("plain", lambda: I.cavity(), DEPTH)
        assert bits_equal(film[..., :3], plain[..., :3])


def test_cavity_on_an_odd_film(xpu):
    """17 x 13: a partial tile whose width is no multiple of 8, here against the model alone.  (The oracle, like the reference, SURVEY A-2,
    restricts the width of a TILE to multiples of 8, not the film's: it renders such a film as overlapping 8-wide strips, and
    test_gpu_frame_shapes.py compares films of this shape with it bit for bit.)  The standard error is the 16 x 16 film's scaled by
    sqrt(256 / 221): the same cavity, the same samples per pixel, pixels independent of each other."""
    for hidden, general in ((None, 0), (GGX, 1)):
        film, st = device(xpu, I.cavity(width=17, height=13, hidden=hidden), DEPTH)
        assert st["shade_general"] == general and st["camera_samples"] == 17 * 13 * T.SPP and np.isfinite(film).all()
        T.check_cavity(f64(film), st, RHO, 1, DEPTH, se=np.asarray(T.SE_MEAN[(RHO, 1, DEPTH)]) * np.sqrt(256.0 / 221.0))
        first, _ = device(xpu, I.cavity(width=24, height=13, hidden=hidden), DEPTH)
        assert not bits_equal(film[:, :16, :3], first[:, :16, :3])  # another film, not a crop


@pytest.mark.parametrize("depth", T.DEPTHS)
@pytest.mark.parametrize("rho", list(T.RHO))
def test_cavity_at_every_depth(xpu, oracle, rho, depth):
    """k_shade<2>: the depth cut, the roulette's survival chain and the film mean at the CPU file's depths"""
    film, st = device(xpu, I.cavity(T.RHO[rho]), depth)
    ref, ost = oracle(("depth", rho, depth), lambda: I.cavity(T.RHO[rho]), depth)
    same(film, st, ref, ost)
    T.check_cavity(f64(film), st, rho, 1, depth)


@pytest.mark.parametrize("rho,lo,hi,spp", T.INCREMENTS)
def test_cavity_increment_between_depths(xpu, rho, lo, hi, spp):
    a, _ = device(xpu, I.cavity(T.RHO[rho]), hi, spp=spp)
    b, _ = device(xpu, I.cavity(T.RHO[rho]), lo, spp=spp)
    T.check_increment(f64(a), f64(b), rho, 1, lo, hi)


@pytest.mark.parametrize("rho,nsets,depth", T.MULTI)
def test_cavity_cut_into_several_lights(xpu, oracle, rho, nsets, depth):
    """several lights of unequal area (pdf = 1 / (nlights x the set's area)), on k_shade<2> and, with the hidden GGX triangle, on k_shade_g"""
    for hidden in (None, GGX):
        film, st = device(xpu, I.cavity(T.RHO[rho], nsets=nsets, hidden=hidden), depth)
        ref, ost = oracle(("multi", rho, nsets, depth), lambda: I.cavity(T.RHO[rho], nsets=nsets), depth)
        same(film, st, ref, ost)
        T.check_cavity(f64(film), st, rho, nsets, depth)


def test_wall_emission_is_exact(xpu):
    """emission on a material that also has lobes, on k_shade<2> and k_shade_g"""
    for hidden in (None, GGX):
        film, _ = device(xpu, I.cavity((0.0, 0.0, 0.0), hidden=hidden), 4, spp=4)
        assert (film[..., :3] == np.array(I.LE_CAVITY, np.float32)).all()


# ---- under the uniform environment ------------------------------------------------------------------------------------------------------------
def _jitter(orc, spp):
    return T.jitter_table(orc, spp)


def _double(rho, texture):
    """Lambert rho as weight 2 rho x a texel of 0.5: the product is exact in fp32"""
    return scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_DIFFUSE, tuple(2.0 * r for r in rho), texture=texture)])


# name: (textures, the environment as an image, shade_general).  The floor's rho is weight x texel where there is a texture: a 1 x 1 image, or
# a 4 x 4 LINEAR one with PERIODIC wrap under UVs that run over [-0.7, 1.8]^2 -- filtering across the wrap edge must return the constant
FLOORS = {
    "constant": ((), False, 0),                      # k_shade<2>: sc.diffuse_only == 2
    "environment_image": ((), True, 1),              # k_shade_g<false, ., ., false, true> (ENV): sc.any_tex == SC_TEX_ENV, seen by every path
    "texture_1x1": ((HALF_1X1,), False, 1),          # k_shade_g<false, ., ., true> (TEX): sc.any_tex == SC_TEX_LOBES
    "texture_4x4": ((HALF_4X4,), False, 1),
    "texture_4x4_environment_image": ((HALF_4X4,), True, 1),  # k_shade_g<false, ., ., true, true> (TEX + ENV)
}


@pytest.mark.parametrize("depth", [1, 2, 5])
@pytest.mark.parametrize("name", list(FLOORS))
def test_lambert_floor_under_the_environment(xpu, orc, oracle, depth, name):
    """zero variance: rho E on the floor, E past its edge, 0 at depth 1.  The oracle knows neither textures nor environment images: its
    scene has them baked in (rho, and the constant E = emission 2 E x texel 0.5)."""
    textures, image, general = FLOORS[name]
    base = I.floor_under_environment(scenes.diffuse(*I.RHO_COLOUR), pitch=T.PITCH)
    sc = I.floor_under_environment(_double(I.RHO_COLOUR, 1), pitch=T.PITCH, textures=textures) if textures else base
    if image:
        sc = _env_image(sc, tuple(2.0 * e for e in I.ENV), 0.5)
    film, st = device(xpu, sc, depth, spp=64)
    assert st["shade_general"] == general
    ref, ost = oracle(("floor", depth), lambda: base, depth, spp=64)
    same(film, st, ref, ost)
    T.check_floor(f64(film), st, _jitter(orc, 64), depth, 64)


def test_planar_mirror(xpu, orc, oracle):
    make = lambda: I.floor_under_environment(scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_REFLECTION, (T.MIRROR,) * 3)]), pitch=T.PITCH)
    film, st = device(xpu, make(), 3, spp=64)
    same(film, st, *oracle("mirror", make, 3, spp=64))
    T.check_mirror(f64(film), st, _jitter(orc, 64))


@pytest.mark.parametrize("k,depth,spp", T.SHEET_CASES)
def test_transparent_sheets(xpu, orc, oracle, k, depth, spp):
    make = lambda: I.sheets_before_environment(k, scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_TRANSPARENT, T.SHEET)]))
    film, st = device(xpu, make(), depth, spp=spp)
    same(film, st, *oracle(("sheets", k, depth), make, depth, spp=spp))
    T.check_sheets(f64(film), st, _jitter(orc, spp), k, depth)


@pytest.mark.parametrize("name", list(T.lobe_materials()))
def test_one_lobe_floor(xpu, orc, oracle, name):
    make = lambda: I.floor_under_environment(T.lobe_materials()[name], pitch=0.5)
    film, st = device(xpu, make(), 2, spp=T.LOBE_SPP[name])
    same(film, st, *oracle(("lobe", name), make, 2, spp=T.LOBE_SPP[name]))
    T.check_lobe_floor(f64(film), st, _jitter(orc, T.LOBE_SPP[name]), name)
