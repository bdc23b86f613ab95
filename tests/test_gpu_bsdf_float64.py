"""The device's closure layer (phx_dev_bsdf_f / phx_dev_bsdf_sample) on the sweep of tests/bsdf64.py:
B  bit-equal to the CPU oracle on every sweep material and edge input (test_bsdf_known_answers does this for the zoo points only);
C  within the stated tolerances of the float64 model, outside the documented input predicates (bsdf64.compare);
D  each non-delta single-lobe sampler draws with the density the model says it does (chi-square against bin masses integrated from the
   model's true density), reports the model's quirk pdf, and the ratio reported / true is the model's quirk factor;
E  E[f cos / pdf] of the device's samples is what float64 quadrature of the model predicts (the bias of a quirky pdf included), and the
   sampler's f (n.wo) is bsdf_f(light = wo, view = wi) for the reciprocal lobes;
F  the delta lobes and the glass node's mix factor against float64 geometry and Fresnel."""
import math

import numpy as np
import pytest

import bsdf64 as M
from conftest import bits_equal
from phosphorus_mk2_amd import abi
from test_bsdf_float64 import check_sweep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sweep(orc):
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    out = []
    for sc, mats in M.sweep_scenes():
        dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2))
        dev.preprocess(sc)
        out.append((sc, mats, dev, orc.Oracle(sc, spp=1)))
    yield out
    for _, _, dev, _ in out:
        dev.close()


def same(a, b):
    """bit-equal, NaN matching NaN whatever its payload (the device's and the host's default NaNs differ)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_B_device_is_bit_equal_to_the_oracle_on_the_sweep(sweep):
    n, wi, wo, u2, _ = M.all_inputs()
    for sc, mats, dev, O in sweep:
        for idx, name in mats:
            assert same(dev.bsdf_f(idx, n, wi, wo), O.bsdf_f(idx, n, wi, wo)), f"bsdf_f {name}"
            for a, b, what in zip(dev.bsdf_sample(idx, n, wi, u2), O.bsdf_sample(idx, n, wi, u2), ("wo", "f", "pdf", "flags")):
                assert same(a, b), f"sample {what} {name}"


def test_C_device_matches_the_float64_model_on_the_sweep(sweep):
    fails, frac = check_sweep([(sc, mats, dev) for sc, mats, dev, _ in sweep], lambda d, i: (lambda *a: d.bsdf_f(i, *a)),
                              lambda d, i: (lambda *a: d.bsdf_sample(i, *a)))
    print(f"excluded by input predicates: {100 * frac:.3f} % of the rows")
    assert not fails, fails
    assert frac < 0.01


# ---- D / E: sampling density and albedo ----------------------------------------------------------------------------------------------
N_SAMPLES = 1 << 20
ANGLES = (0.0, 30.0, 60.0, 80.0, 89.0)
AZIMUTHS = (0.3, 2.0)
NB = 16  # bins per coordinate
NQ = 32  # quadrature points per bin and coordinate: 16 leaves errors of ~0.3 % in the bin masses (normal incidence, and 89 degrees
#          where the visible normals reach the horizon), which 2^20 stratified samples resolve


def stratified(k, seed):
    side = int(round(math.sqrt(k)))
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    u = (np.stack([i.ravel(), j.ravel()], 1) + rng.random((side * side, 2))) / side
    return np.minimum(u, 1.0 - 2.0 ** -24).astype(np.float32)


def density_cases(sweep):
    """(name, material index, device, oracle, model) of every non-delta single-lobe material of the sweep"""
    for sc, mats, dev, O in sweep:
        L5 = M.sheen_L5_of(sc.materials)
        for idx, name in mats:
            m = sc.materials[idx]
            if len(m.lobes) != 1 or m.lobes[0].fac_mode != abi.FAC_NONE:
                continue
            l = m.lobes[0]
            if l.type in (abi.LOBE_REFLECTION, abi.LOBE_REFRACTION, abi.LOBE_TRANSPARENT) or (l.refract and np.float32(l.eta) == 1.0):
                continue
            yield name, idx, dev, O, M.Model(m, L5)


class Coords:
    """bins of the sampled directions: a map of the sample onto [0, 1)^2, its inverse with the Jacobian, for the model's quadrature.
    Cosine-weighted lobes: (sin^2 theta_o, phi_o), where the true density is uniform.  GGX: the microfacet normal that takes wi to wo,
    as (2/pi atan |m|, phi of m) of its unit-roughness slopes m = (-h.x / (h.y ax), -h.z / (h.y ay)): the bins follow the lobe at
    every roughness and are the images of rectangles in slope space."""

    def __init__(self, model, li):
        self.model, self.l, self.li = model, model.lobes[0], li
        self.ggx = self.l.type == abi.LOBE_MICROFACET

    def forward(self, lo):
        if not self.ggx:
            return 1.0 - lo[:, 1] ** 2, (np.arctan2(lo[:, 2], lo[:, 0]) + np.pi) / (2 * np.pi)
        h = self.model.half_vector(np.broadcast_to(self.li, lo.shape), lo)
        mx, my = -h[:, 0] / h[:, 1] / self.l.ax, -h[:, 2] / h[:, 1] / self.l.ay
        return (2 / np.pi) * np.arctan(np.hypot(mx, my)), (np.arctan2(my, mx) + np.pi) / (2 * np.pi)

    def quadrature(self):
        """-> (x, y, lo at the quadrature points, h, weight = true density of the DRAW (wo for cosine-weighted, the microfacet normal for
        GGX) times the area element where the sampler accepts it, the mass it rejects) on an NB NQ x NB NQ midpoint grid"""
        g = (np.arange(NB * NQ) + 0.5) / (NB * NQ)
        x, y = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
        li = np.broadcast_to(self.li, (len(x), 3))
        phi = 2 * np.pi * y - np.pi
        dA = 1.0 / (NB * NQ) ** 2
        if not self.ggx:
            s = x
            lo = np.stack([np.sqrt(s) * np.cos(phi), np.sqrt(1 - s), np.sqrt(s) * np.sin(phi)], 1)
            return x, y, lo, None, np.pi / lo[:, 1] * (lo[:, 1] / np.pi) * dA, 0.0  # dw = pi / cos ds dy, density cos / pi
        rho = np.tan(np.pi / 2 * x)
        m1, m2 = rho * np.cos(phi), rho * np.sin(phi)
        h = M.normalize(np.stack([-self.l.ax * m1, np.ones_like(m1), -self.l.ay * m2], 1))
        jac = h[:, 1] ** 3 * self.l.ax * self.l.ay * rho * (np.pi / 2) * (1 + rho * rho) * 2 * np.pi  # dw_h / (dx dy)
        p = M.ggx_true_density(self.l.ax, self.l.ay, li, h)
        iw = M.dot(li, h)
        if not self.l.refract:
            lo = -li + (2 * iw)[:, None] * h
            ok = lo[:, 1] > 0
        else:
            e = np.where(li[:, 1] > 0, 1.0 / self.l.eta, self.l.eta)
            s2t = e * e * np.maximum(0.0, 1 - iw * iw)
            ok = s2t < 1
            lo = -e[:, None] * li + (e * iw - np.sqrt(np.maximum(0.0, 1 - s2t)))[:, None] * h
        return x, y, lo, h, np.where(ok & (iw > 0), p * jac * dA, 0.0), float(np.where(~ok & (iw > 0), p * jac * dA, 0.0).sum())


def chi2_p(obs, exp):
    """chi-square of counts against expectations, bins of expectation < 20 pooled (the pooled bin expects at least 1e-5 of the samples:
    fp32 directions on the edge of the support, where the model's density drops to 0, land there); Wilson-Hilferty p-value"""
    low = exp < 20
    o = np.append(obs[~low], obs[low].sum()); e = np.append(exp[~low], max(exp[low].sum(), 1e-5 * obs.sum()))
    x2, k = float(((o - e) ** 2 / e).sum()), len(o) - 1
    z = ((x2 / k) ** (1 / 3) - (1 - 2 / (9 * k))) / math.sqrt(2 / (9 * k))
    return x2, k, 0.5 * math.erfc(z / math.sqrt(2))


def run_case(sampler, model, theta, azim, seed):
    """-> dict of the case: p-value, pointwise pdf error, quirk-factor error, estimator mean vs prediction"""
    n = np.tile(np.array([[0, 1, 0]], np.float32), (N_SAMPLES, 1))
    F1 = M.frame(np.array([[0.0, 1.0, 0.0]]))
    t, a = np.radians(theta), azim
    li = np.array([[np.sin(t) * np.cos(a), np.cos(t), np.sin(t) * np.sin(a)]])
    wi1 = M.to_world(F1, li).astype(np.float32)
    li = M.to_local(F1, wi1.astype(np.float64))  # the fp32 direction the device sees
    wi = np.tile(wi1, (N_SAMPLES, 1))
    wo, f, pdf, fl = sampler(n, wi, stratified(N_SAMPLES, seed))
    live = pdf > 0
    lo = M.to_local(F1, wo[live].astype(np.float64))
    C = Coords(model, li)
    x, y = C.forward(lo)
    bins = np.minimum((x * NB).astype(int), NB - 1) * NB + np.minimum((y * NB).astype(int), NB - 1)
    obs = np.append(np.bincount(bins, minlength=NB * NB).astype(float), float((~live).sum()))
    qx, qy, qlo, qh, w, rejected = C.quadrature()
    qb = np.minimum((qx * NB).astype(int), NB - 1) * NB + np.minimum((qy * NB).astype(int), NB - 1)
    mass = np.bincount(qb, weights=w, minlength=NB * NB)
    exp = np.append(mass, rejected) * N_SAMPLES
    x2, k, p = chi2_p(obs, exp)
    # pointwise: the reported pdf is the model's quirk pdf at the sampled wo; reported / true is the model's quirk factor
    sub = np.nonzero(live)[0][:: max(1, live.sum() // 8192)]
    n1 = n[:len(sub)]
    rep_m = model.reported_pdf(n1, wi[sub], wo[sub])
    true_m = model.true_pdf(n1, wi[sub], wo[sub])
    # the model's pdf takes wh from the fp32 wo, and D is steep at small alpha (roughness 1e-3 needs 1.7e-4): 1e-3 relative; for refraction
    # li.wh + eta lo.wh amplifies that rounding by kappa^2 (C's REFRACT_COND term), and beyond kappa 1e3 (|eta - 1| ~ 1e-4 at some wo)
    # the fp32 pdf is not resolved at all
    kappa = M.refract_condition(model, n1, wi[sub], wo[sub])
    ok = (true_m > 0) & (kappa < 1e3)
    tol = (1e-3 + M.REFRACT_COND * kappa[ok] ** 2) * np.abs(rep_m[ok]) + 1e-6 * np.abs(rep_m[ok]).max(initial=0.0)
    pt_err = float(np.max(np.abs(pdf[sub][ok] - rep_m[ok]) / tol, initial=0.0))  # <= 1: within the stated bound
    factor = pdf[sub][ok] / true_m[ok]
    # E: E[f cos / pdf] against the quadrature of the model (what the quirk pdf makes of the estimator), and the unbiased albedo
    w0 = model.lobes[0].weight[0]
    est = np.zeros(N_SAMPLES)
    est[live] = f[live, 0] / w0 * np.abs(wo[live, 1]) / pdf[live]
    wo_q = M.to_world(F1, qlo).astype(np.float32)
    nq = np.tile(np.array([[0, 1, 0]], np.float32), (len(qlo), 1))
    wiq = np.tile(wi1, (len(qlo), 1))
    good = w > 0
    g = np.zeros(len(qlo))
    Fq = M.frame(M.f64(nq[good]))
    fq = M.lobe_eval(model.lobes[0], Fq, M.f64(wiq[good]), M.f64(wo_q[good]), model.L5, model.q)[0]  # the sampler's f (view, sampled)
    g[good] = fq * np.abs(M.f64(wo_q[good])[:, 1]) / model.reported_pdf(nq[good], wiq[good], wo_q[good])
    predicted = float((g * w).sum())
    return {"x2": x2, "dof": k, "p": p, "pointwise": pt_err, "factor": (float(factor.min()), float(np.median(factor)), float(factor.max())),
            "est": float(est.mean()), "sigma": float(est.std() / math.sqrt(N_SAMPLES)), "predicted": predicted}


def test_D_E_sampling_density_and_albedo(sweep):
    cases = [(name, idx, dev, model, th, az) for name, idx, dev, O, model in density_cases(sweep) for th in ANGLES
             for az in (AZIMUTHS if model.lobes[0].ax != model.lobes[0].ay else AZIMUTHS[:1])]  # azimuth matters to anisotropic lobes only
    alpha = 1e-3 / len(cases)  # one significance for all cases together (Bonferroni)
    bad = []
    for c, (name, idx, dev, model, th, az) in enumerate(cases):
        r = run_case(lambda *a: dev.bsdf_sample(idx, *a), model, th, az, seed=c)
        print(f"{name:24s} {th:4.0f} {az:3.1f}  chi2 {r['x2']:8.1f}/{r['dof']:3d} p {r['p']:.2e}  pdf err / bound {r['pointwise']:.1e}  "
              f"reported/true {r['factor'][0]:.4f} {r['factor'][1]:.4f} {r['factor'][2]:.4f}  E[f cos/pdf] {r['est']:.5f} +- {r['sigma']:.1e} "
              f"predicted {r['predicted']:.5f}")
        # sheen r < 0.01 seen at >= 80 degrees: D ~ sin^(1/r) theta_h is a spike at the horizon that 2^20 samples hit a few times and the
        # quadrature grid does not resolve -- neither the sample mean nor its sigma is a usable bound there (the histogram and the pdf are)
        resolved = not (model.lobes[0].type == abi.LOBE_SHEEN and model.lobes[0].r < 0.01 and th >= 80.0)
        if r["p"] < alpha or r["pointwise"] > 1.0 or \
                (resolved and abs(r["est"] - r["predicted"]) > 6 * r["sigma"] + 2e-3 * abs(r["predicted"]) + 1e-6):  # 1e-6: a prediction of
            # ~1e-19 where no sample reaches (sheen r = 1e-3 below 80 degrees) has sigma 0
            bad.append((name, th, az, r))
    assert not bad, bad


def test_E_sampler_f_is_bsdf_f_for_the_reciprocal_lobes(sweep):
    """Lambert, Oren-Nayar, GGX reflect and sheen: the sampler's f (n.wo) equals bsdf_f(light = wo, view = wi) within 2 ulp.  GGX refract
    picks eta by li.y, so f(wo -> wi) is the model's f with the roles swapped (its own tolerance, C)."""
    rng = np.random.default_rng(17)
    k = 8192
    unit = lambda m: M._unit(rng.normal(size=(m, 3)))
    n = unit(k)
    wi = unit(k)
    wi = np.where((n * wi).sum(1, keepdims=True) < 0, -wi, wi).astype(np.float32)  # the view above the surface: the sample reflects
    u2 = rng.random((k, 2)).astype(np.float32)
    for name, idx, dev, O, model in density_cases(sweep):
        wo, f, pdf, fl = dev.bsdf_sample(idx, n, wi, u2)
        live = (pdf > 0) & np.isfinite(f).all(1) & ~M.sheen_nonfinite_inputs(model, n, wi, wo)
        if not live.any():  # sheen r = 0: f is NaN everywhere (test_sheen_r0_is_nan_everywhere_and_so_is_the_oracle)
            continue
        cos =(n[:, 0] * wo[:, 0] + n[:, 1] * wo[:, 1] + n[:, 2] * wo[:, 2]).astype(np.float32)
        g = dev.bsdf_f(idx, n, wo, wi)
        if model.lobes[0].refract:
            fm = model.f(n[live], wo[live], wi[live])  # the relation: f(wo -> wi) is the model's f with the roles swapped, C's tolerance
            rt = M.RTOL + M._cos_terms(M.f64(n[live]), M.f64(wi[live]), M.f64(wo[live])) + \
                M.REFRACT_COND * M.refract_condition(model, n[live], wo[live], wi[live]) ** 2 + M.fresnel_condition(model, n[live], wo[live], wi[live])
            assert M._close(g[live], fm, M._peak(fm), rt).all(), name
            continue
        lhs = (f * cos[:, None]).astype(np.float32)
        ul = np.abs(lhs[live].view(np.int32).astype(np.int64) - g[live].view(np.int32).astype(np.int64))
        # the Cook-Torrance f takes its Fresnel at lo.wh, lo = the view in bsdf_f and the sampled direction in sample: the two cosines
        # differ by rounding, which dielectric(c, 0.5) amplifies by ~1 / |c^2 - 3/4| (bsdf64.fresnel_condition) -- there, that bound
        rel = np.abs(lhs[live].astype(np.float64) - g[live]) / np.maximum(np.abs(g[live].astype(np.float64)), 1e-30)
        fc = 4 * M.fresnel_condition(model, n[live], wi[live], wo[live])[:, None]
        assert ((ul <= 2) | (rel <= fc)).all(), (name, int(ul.max()))
        print(f"{name:24s} {live.sum():5d} samples: within 2 ulp {100 * (ul <= 2).all(1).mean():.2f} %, the rest within the Fresnel bound")


# ---- F: delta lobes ------------------------------------------------------------------------------------------------------------------
def test_F_delta_lobes_against_float64_geometry(sweep):
    sc, mats, dev, O = sweep[0]
    idx = {name: i for i, name in mats}
    rng = np.random.default_rng(23)
    k = 1 << 14
    n = M._unit(rng.normal(size=(k, 3)))
    wi = M._unit(rng.normal(size=(k, 3)))
    u2 = rng.random((k, 2)).astype(np.float32)
    n64, wi64 = M.f64(n), M.f64(wi)
    c = M.dot(n64, wi64)
    # mirror
    wo, f, pdf, fl = dev.bsdf_sample(idx["reflection"], n, wi, u2)
    assert np.abs(wo - (-wi64 + 2 * c[:, None] * n64)).max() < 8 * M.U * 4 and (pdf == 1).all() and (f == np.float32(0.9)).all()
    # transparent: straight through, bit for bit
    wo, f, pdf, fl = dev.bsdf_sample(idx["transparent"], n, wi, u2)
    assert bits_equal(wo, -wi) and (fl == abi.BSDF_TRANSMIT).all() and (pdf == 1).all()
    # the eta == 1 microfacet pass-through
    wo, f, pdf, fl = dev.bsdf_sample(idx["ggx_refract_eta1"], n, wi, u2)
    assert bits_equal(wo, -wi) and (pdf == 1).all() and (f == np.float32(0.9)).all() and (fl == abi.BSDF_TRANSMIT).all()
    # refraction: Snell, coplanarity, the other side; black exactly outside a rounding band around the critical angle
    for e in M.SWEEP_ETA:
        wo, f, pdf, fl = dev.bsdf_sample(idx[f"refraction_eta{e:g}"], n, wi, u2)
        eta = np.where(c > 0, 1.0 / float(np.float32(e)), float(np.float32(e)))
        arg = 1.0 - eta * eta * (1.0 - c * c)
        band = M.BAND * (1.0 + eta * eta)
        assert (f[arg < -band] == 0).all() and (f[arg > band] > 0).all(), e
        live = arg > band
        wo64 = wo[live].astype(np.float64)
        ct = M.dot(n64[live], wo64)
        sin_t, sin_i = np.sqrt(np.maximum(0, 1 - ct * ct)), np.sqrt(np.maximum(0, 1 - c[live] ** 2))
        assert np.allclose(sin_t, eta[live] * sin_i, atol=1e-5), e
        assert np.abs(M.dot(np.cross(n64[live], wi64[live]), wo64)).max() < 1e-5, e
        assert (ct * c[live] < 0).all() or e == 1.0, e
        assert np.allclose(np.linalg.norm(wo64, axis=1), 1, atol=1e-5), e
    # the glass node's mix factor: u = 0.75 picks the mirror (lobe 1 of 2, or the only lobe where the refraction's weight is 0)
    cosv = np.linspace(-1, 1, k)
    for ior in M.SWEEP_GLASS_IOR:
        if ior == 1.0:
            continue  # fac = 0 for every cos: the mirror is dropped (f = the refraction)
        n1 = np.tile(np.array([[0, 1, 0]], np.float32), (k, 1))
        v = M._unit(np.stack([np.sqrt(1 - cosv ** 2), cosv, np.zeros(k)], 1))
        u = np.tile(np.array([[0.75, 0.5]], np.float32), (k, 1))
        wo, f, pdf, fl = dev.bsdf_sample(idx[f"glass_ior{ior:g}"], n1, v, u)
        fac = M.fresnel_mix_factor(float(np.float32(ior)), M.f64(n1), M.f64(v))
        mirror = fl == (abi.BSDF_REFLECT | abi.BSDF_SPECULAR)
        assert mirror.mean() > 0.5, ior
        assert np.allclose(f[mirror, 0], fac[mirror], rtol=1e-4, atol=1e-6), ior
