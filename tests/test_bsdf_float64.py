"""A. The float64 model of the closure layer (tests/bsdf64.py) against the CPU oracle (oracle/obsdf.h) on the sweep: every material of
bsdf64.sweep_scenes() on every input set of bsdf64.edge_inputs(), f and sample's wo / f / pdf / flags, within the tolerances that
tests/test_gpu_bsdf_float64.py holds the device to (bsdf64.compare).  The model shares no code with the oracle or the device, so a
transcription error that the oracle shares with the device (which is bit-equal to it) fails here.  Plus the host maps and the quirk
switches of the model itself, pinned as numbers."""
import numpy as np
import pytest

import bsdf64 as M
from phosphorus_mk2_amd import abi


@pytest.fixture(scope="module")
def sweep(orc):
    return [(sc, mats, orc.Oracle(sc, spp=1)) for sc, mats in M.sweep_scenes()]


def check_sweep(sweep, f_of, sample_of):
    """every material of the sweep on every input row -> (failures, excluded fraction); f_of(i) / sample_of(i): the implementation under test"""
    n, wi, wo, u2, sets = M.all_inputs()
    fails, rows, excluded, nonfinite = [], 0, 0, 0
    for k, (sc, mats, impl) in enumerate(sweep):
        L5 = M.sheen_L5_of(sc.materials)
        for idx, name in mats:
            r = M.compare(M.Model(sc.materials[idx], L5), n, wi, wo, u2, f_of(impl, idx), sample_of(impl, idx))
            rows += 2 * r["rows"]; excluded += r["f_excluded_rows"] + r["s_excluded_rows"]; nonfinite += r["nonfinite_allowed"]
            for what in ("bad_f", "bad_s"):
                if len(r[what]):
                    fails.append((name, what, len(r[what]), sorted(set(sets[r[what]]))))
    return fails, excluded / rows


def test_model_matches_the_oracle_on_the_sweep(sweep):
    fails, frac = check_sweep(sweep, lambda O, i: (lambda *a: O.bsdf_f(i, *a)), lambda O, i: (lambda *a: O.bsdf_sample(i, *a)))
    print(f"excluded by input predicates: {100 * frac:.3f} % of the rows")
    assert not fails, fails
    assert frac < 0.01


def test_host_parameter_maps():
    # roughness_to_alpha is not monotonic and never reaches its 1e-4 clamp: roughness 0 (log(1e-5)) is alpha 0.296, the minimum 0.0093
    assert M.roughness_to_alpha(0.0) == pytest.approx(0.2961, abs=1e-4)
    r = np.exp(np.linspace(np.log(1e-5), 0.0, 20001))
    a = np.array([M.roughness_to_alpha(x) for x in r])
    assert a.min() == pytest.approx(0.0093, abs=1e-4) and r[a.argmin()] == pytest.approx(1.5e-4, rel=0.1)
    assert M.roughness_to_alpha(4.0) == 1.0 and M.roughness_to_alpha(0.09) == pytest.approx(0.4349, abs=1e-4)
    # Oren-Nayar reads alpha as degrees: 90 -> sigma = pi / 2
    A, B = M.oren_nayar_ab(90.0)
    s2 = (np.pi / 2) ** 2
    assert A == pytest.approx(1 - s2 / (2 * (s2 + 0.33))) and B == pytest.approx(0.45 * s2 / (s2 + 0.09))
    # L5 is the first sheen lobe's of the table
    from phosphorus_mk2_amd import scenes
    sh = lambda r: scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_SHEEN, r=r)])
    assert M.sheen_L5_of([scenes.diffuse(1, 1, 1), sh(0.3), sh(0.7)]) == M.sheen_L(0.5, float(np.float32(0.3)))


def test_sheen_r0_is_nan_everywhere_and_so_is_the_oracle(sweep):
    """sheen_bsdf_node's default roughness 0: D = (2 + 1/r) sin^(1/r) / (2 pi) = inf * 0 for every direction (sheen.hpp:40-48 has the
    same expression): f is NaN wherever the lobe is evaluated, on the oracle as in the model."""
    sc, mats, O = next(s for s in sweep if s[1][0][1] == "sheen_r0")
    rng = np.random.default_rng(3)
    unit = lambda k: M._unit(rng.normal(size=(k, 3)))
    n, wi, wo = unit(2000), unit(2000), unit(2000)
    lit = ((n * wi).sum(1) * (n * wo).sum(1)) > 0
    fo, fm = O.bsdf_f(0, n, wi, wo), M.Model(sc.materials[0], M.sheen_L5_of(sc.materials)).f(n, wi, wo)
    assert np.isnan(fo[lit]).all() and np.isnan(fm[lit]).all() and (fo[~lit] == 0).all() and (fm[~lit] == 0).all()


def test_quirk_switches_change_what_they_name():
    """each quirk switch of the model that matters off rounding edges is live: turning it off changes f or sample on random inputs
    (wh_zero and pdf_side_world differ from the textbook only on rounding edges: an exactly-zero component, a non-orthonormal frame)"""
    from phosphorus_mk2_amd import scenes
    rng = np.random.default_rng(7)
    unit = lambda k: M._unit(rng.normal(size=(k, 3)))
    n, wi, wo, u2 = unit(4000), unit(4000), unit(4000), rng.random((4000, 2)).astype(np.float32)
    wi = np.where(((n * wi).sum(1, keepdims=True) < 0), -wi, wi).astype(np.float32)
    mats = {"fresnel_half": M.sweep_materials()[8][1], "g1_world": scenes.closure_zoo()[8], "lambda_alpha": M.sweep_materials()[13][1],
            "pdf_precedence": M.sweep_materials()[18][1], "jacobian_eta": M.sweep_materials()[18][1], "diffuse_pdf_wi": scenes.closure_zoo()[9],
            "on_degrees": M.sweep_materials()[2][1]}
    for q, mat in mats.items():
        on, off = M.Model(mat), M.Model(mat, quirks=M.ALL - {q})
        a, b = on.sample(n, wi, u2), off.sample(n, wi, u2)
        fa, fb = on.f(n, wo, wi), off.f(n, wo, wi)
        F = M.frame(M.f64(n))
        pa = [M.lobe_eval(l, F, M.f64(wi), M.f64(wo), 0.0, on.q)[1] for l in on.lobes]  # the pdf eval() gives the matched-lobe average
        pb = [M.lobe_eval(l, F, M.f64(wi), M.f64(wo), 0.0, off.q)[1] for l in off.lobes]
        changed = not (np.allclose(a[2], b[2], equal_nan=True) and np.allclose(a[1], b[1], equal_nan=True) and np.allclose(fa, fb, equal_nan=True)
                       and all(np.allclose(x, y, equal_nan=True) for x, y in zip(pa, pb)))
        assert changed, q
