"""Adaptive sampling (phx_adaptive in include/phx_xpu.h) restated in float64 numpy, operation by operation as the header writes it:
the rounds, the decision, the rescale and the pass schedule.  Per-sample fp32 films come in -- y_s = fp32(x_s * inv), the very values the
film adds -- and `primary`, `m2`, `samples` and the round at which each pixel stopped come out.  The passes are replayed exactly as the
restatement of the m2 channel replays them (tests/test_film_moments.py: moments_pass, the re-centring at every pass included).  Nothing here
reads the device's sources."""
import numpy as np

from test_film_moments import moments_pass

F, D = np.float32, np.float64


def round_ends(spp, min_samples, step):
    """e_0 = min(min_samples, spp), e_{j+1} = min(e_j + step, spp)"""
    assert spp >= 1 and min_samples >= 2 and step >= 1
    ends = [min(min_samples, spp)]
    while ends[-1] < spp:
        ends.append(min(ends[-1] + step, spp))
    return ends


def round_passes(samples, flight=0):
    """the passes of one round of `samples` samples: one, or -- samples_in_flight set -- passes of at most `flight`"""
    if not flight:
        return [samples]
    S = min(flight, samples)
    return [min(S, samples - s0) for s0 in range(0, samples, S)]


def stops(f, m2, n, spp, tau, a):
    """the decision after a round that ended at n < spp: f, m2 (..., 3) float32 -> (...) bool.  A NaN compares false."""
    f, m2 = np.asarray(f, F), np.asarray(m2, F)
    tau, a = D(F(tau)), D(F(a))
    with np.errstate(invalid="ignore", over="ignore"):
        q = D(n) / D(n - 1)
        g = (a * D(n)) / D(spp)
        L = m2.astype(D) * q
        b = tau * (np.abs(f.astype(D)) + g)
        ok = L <= b * b
    return ok.all(-1)


def rescaled(f, m2, n, spp):
    """a pixel that stops at n, rescaled once -> (primary, m2) float32"""
    k = D(spp) / D(n)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(f, F).astype(D) * k).astype(F), ((np.asarray(m2, F).astype(D) * k) * k).astype(F)


def select(acc, active, n, spp, tau, a):
    """phx_dev_adaptive_select: acc (rows, 7) float32 = primary rgb, m2 rgb, samples; active = ascending row indices or None for all rows.
    -> (acc after the selection, the rows that go on in the order of `active`).  Rows that go on and rows outside `active` are unchanged."""
    out = np.array(acc, F).reshape(-1, 7)
    active = np.arange(len(out), dtype=np.uint32) if active is None else np.asarray(active, np.uint32)
    rows = out[active]
    stop = stops(rows[:, :3], rows[:, 3:6], n, spp, tau, a)
    f, m2 = rescaled(rows[stop, :3], rows[stop, 3:6], n, spp)
    done = active[stop]
    out[done, :3], out[done, 3:6], out[done, 6] = f, m2, F(n)
    return out, active[~stop].copy()


def adaptive_film(y, tau, floor, min_samples, step, flight=0, normals=None):
    """The frame of adaptive sampling from its per-sample films.  y (..., spp, 3) float32; normals (..., spp, 3) float32 per sample, all
    zero where the camera ray of that sample hit nothing, or None.
    -> dict: primary, m2 (..., 3) float32; samples (...) float32; stop_round (...) int, the index of the round after which the pixel
    stopped, -1 for a pixel that took every sample; normals (..., 3) float32 when given: the last sample with a hit among those the pixel took."""
    y = np.asarray(y, F)
    spp, shape = y.shape[-2], y.shape[:-2]
    f, m2 = np.zeros(shape + (3,), F), np.zeros(shape + (3,), F)
    samples = np.full(shape, F(spp), F)
    stop_round = np.full(shape, -1, np.int64)
    active = np.ones(shape, bool)
    nrm = None if normals is None else np.zeros(shape + (3,), F)
    begin = 0
    for j, end in enumerate(round_ends(spp, min_samples, step)):
        s0 = begin
        for ns in round_passes(end - begin, flight):
            fa, ma = moments_pass(f[active], m2[active], y[active][..., s0:s0 + ns, :], s0)
            f[active], m2[active] = fa, ma
            if nrm is not None:
                for s in range(s0, s0 + ns):
                    hit = active & (np.asarray(normals, F)[..., s, :] != 0).any(-1)
                    nrm[hit] = normals[..., s, :][hit]
            s0 += ns
        begin = end
        if end == spp:
            break
        stop = np.zeros(shape, bool)
        stop[active] = stops(f[active], m2[active], end, spp, tau, floor)
        f[stop], m2[stop] = rescaled(f[stop], m2[stop], end, spp)
        samples[stop] = F(end)
        stop_round[stop] = j
        active &= ~stop
    out = {"primary": f, "m2": m2, "samples": samples, "stop_round": stop_round}
    if nrm is not None:
        out["normals"] = nrm
    return out
