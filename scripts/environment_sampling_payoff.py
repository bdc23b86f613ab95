"""What sampling the environment buys where the sky holds a small sun: the OPEN showroom of DESIGN 10 (scenes.environment_showroom) under
scenes.procedural_sky with a sun of a few texels (--sun-radius), rendered on one GPU at equal sample counts under

    power    light_sampling 0x101: the sun is found only by BSDF samples that happen to escape towards it
    env      light_sampling 0x301 (environment_sampling=True): next-event estimation samples the image

Per mode: a reference, the mean of two frames at --ref-spp (seeds 1 and 2), and, per entry of --spp, --frames frames of other seeds whose
mean squared error against THAT MODE's reference is reported (each estimator is held to its own limit; the two references' distance from one
another is printed as a check: where a lobe's sampling pdf is one of DESIGN 4.11's quirks their expectations differ by that bias), with
phx_stats' frame_ms.  Error figures: the plain MSE over the film's RGB; the relative MSE (error^2 / (reference^2 + 1e-4)); and both again
with the --trim largest pixel errors left out (default 0.1 %), as scripts/light_selection_payoff.py does.  The last line is one JSON record.

    python scripts/environment_sampling_payoff.py [--spp 16 64 256] [--ref-spp 2048] [--out profiles/r13_environment_sampling_payoff.log]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=500_000)
    ap.add_argument("--sun-radius", type=float, default=0.006, help="radians; a texel of the 2048 x 1024 sky is 0.003 wide")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--trim", type=float, default=0.001, help="share of the pixels, the ones with the largest error, left out of the trimmed figures")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r13_environment_sampling_payoff.log"))
    a = ap.parse_args()
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    sc = scenes.environment_showroom(a.triangles, a.width, a.height)
    sky = scenes.procedural_sky(2048, 1024, sun_radius=a.sun_radius)
    sc.textures[sc.materials[sc.environment_material].emission_texture - 1].texels = sky
    sun_texels = int((sky[..., 0] > 100.0).sum())
    W, H = sc.camera.width, sc.camera.height
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def frames(kw, spp, seeds):
        dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=spp, paths_per_sample=1, path_depth=9, **kw))
        try:
            dev.preprocess(sc)
            out = []
            for seed in seeds:
                film = xpu.Film(W, H, 4)
                dev.start(sc, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, native_sink=True))
                dev.join()
                out.append((film.data[..., :3].astype(np.float64), dev.stats()))
            return out
        finally:
            dev.close()

    modes = {"power": {"light_sampling": "area", "light_selection": "power"},
             "env": {"light_sampling": "area", "light_selection": "power", "environment_sampling": True}}
    out = {"scene": f"{sc.name} {W}x{H} depth 9, a sun of {sun_texels} texels", "ref_spp": a.ref_spp, "modes": {}}
    refs = {}
    for m, kw in modes.items():
        (r1, st1), (r2, st) = frames(kw, a.ref_spp, [1, 2])
        ref = 0.5 * (r1 + r2)
        assert np.nanmax(ref) > 0.05
        refs[m] = ref
        say(f"{m:>6} reference: 2 x {a.ref_spp} spp, frames {st1['frame_ms']:.1f} (the process's first) and {st['frame_ms']:.1f} ms, film mean {np.nanmean(ref, (0, 1))}, "
            f"shadow rays {st['rays_shadow']} of {st['rays_closest']} closest-hit rays, pixels not finite {int((~np.isfinite(ref).all(-1)).sum())}")
        out["modes"][m] = {"ref_frame_ms": [st1["frame_ms"], st["frame_ms"]], "ref_mean": np.nanmean(ref, (0, 1)).tolist(), "spp": {}}
    # the closed room's glass yields a few non-finite pixels (as the reference's films do): a pixel counts where both references are finite
    ok = np.isfinite(refs["power"]).all(-1) & np.isfinite(refs["env"]).all(-1)
    out["pixels_compared"] = int(ok.sum())

    def errors(f, ref):
        keep = ok & np.isfinite(f).all(-1)
        d = f[keep] - ref[keep]
        se, rel = (d * d).mean(-1), (d * d / (ref[keep] ** 2 + 1e-4)).mean(-1)  # per pixel
        n = len(se) - int(round(a.trim * len(se)))
        return {"mse": float(se.mean()), "rel_mse": float(rel.mean()), "mse_trimmed": float(np.sort(se)[:n].mean()), "rel_mse_trimmed": float(np.sort(rel)[:n].mean())}
    KEYS = ("mse", "rel_mse", "mse_trimmed", "rel_mse_trimmed")
    out["refs"] = errors(refs["power"], refs["env"])
    say(f"{out['pixels_compared']} of {W * H} pixels compared; the two references differ by " + ", ".join(f"{k} {out['refs'][k]:.3e}" for k in KEYS) +
        f"; film means' ratio {refs['power'][ok].mean(0) / refs['env'][ok].mean(0)}")
    for spp in a.spp:
        for m, kw in modes.items():
            rows = frames(kw, spp, [100 + k for k in range(a.frames + 1)])[1:]  # the first frame warms the device up
            errs = [errors(f, refs[m]) for f, _ in rows]
            ms = [st["frame_ms"] for _, st in rows]
            rec = {k: float(np.median([e[k] for e in errs])) for k in KEYS}
            rec.update({"frame_ms": float(np.median(ms)), "frame_ms_all": ms, "all": errs})
            out["modes"][m]["spp"][str(spp)] = rec
            say(f"{spp:5d} spp {m:>6}: " + "  ".join(f"{k} {rec[k]:.4e}" for k in KEYS) + f"  frame {rec['frame_ms']:8.1f} ms   (medians of {a.frames} frames)")
        u, p = out["modes"]["power"]["spp"][str(spp)], out["modes"]["env"]["spp"][str(spp)]
        say(f"{spp:5d} spp: BSDF sampling over environment sampling: " + ", ".join(f"{k} x {u[k] / p[k]:.2f}" for k in KEYS) + f", frame time x {u['frame_ms'] / p['frame_ms']:.3f}")
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
