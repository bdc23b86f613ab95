"""What adaptive sampling buys: scenes.bmw_showroom (the closed showroom, general closures) and scenes.sun_floor() under light_sampling 0x301
(every pixel has the same expectation; the sun makes the samples heavy-tailed), on one GPU.  Per scene: a reference, one uniform frame at
--ref-factor x the spp (at least 16 x); the uniform frame at full spp; per threshold of --tau the adaptive frame (min_samples = step = --step)
and the uniform frame whose spp is the adaptive frame's mean samples per pixel, rounded.  Reported per frame: phx_stats' frame_ms (the best
of --frames after a warm-up frame), the mean samples per pixel, the MSE over the film's RGB against the reference (pixels finite in both),
and for the adaptive frames the measured bias: the film's mean minus the reference's, per colour, in standard errors of that difference
(the per-pixel variances by film_variance from each film's own m2 channel, summed over the pixels).  The last line is one JSON record.

    python scripts/adaptive_sampling_payoff.py [--tau 0.05 0.1 0.2] [--out profiles/r16_adaptive_sampling_payoff.log]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tau", type=float, nargs="+", default=[0.05, 0.1, 0.2])
    ap.add_argument("--floor", type=float, default=0.0)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--ref-factor", type=int, default=16)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--triangles", type=int, default=200_000)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--floor-size", type=int, default=256, help="the sun_floor film is this many pixels square")
    ap.add_argument("--scenes", nargs="+", default=["sun_floor", "bmw_showroom"])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r16_adaptive_sampling_payoff.log"))
    a = ap.parse_args()
    assert a.ref_factor >= 16
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cases = {"sun_floor": (lambda: scenes.sun_floor(a.floor_size, a.floor_size), dict(light_sampling="area", light_selection="power", environment_sampling=True), 2),
             "bmw_showroom": (lambda: scenes.bmw_showroom(a.triangles, a.width, a.height), {}, 9)}
    out = {"spp": a.spp, "ref_spp": a.spp * a.ref_factor, "min_samples": a.step, "step": a.step, "floor": a.floor, "scenes": {}}
    for name in a.scenes:
        make, kw, depth = cases[name]
        sc = make()
        W, H = sc.camera.width, sc.camera.height

        def frames(spp, seed, adaptive=None, n=1):
            """-> (film data (H, W, 7 or 8) of the last frame, the best frame_ms of n frames behind a warm-up frame, stats)"""
            dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=spp, paths_per_sample=1, path_depth=depth, **kw))
            try:
                if adaptive is not None:
                    dev.set_adaptive(adaptive, a.floor, a.step, a.step)
                dev.preprocess(sc)
                best = None
                for k in range(n + 1):
                    film = xpu.Film(W, H, 4, False, True, adaptive is not None)
                    dev.start(sc, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, native_sink=True))
                    dev.join()
                    st = dev.stats()
                    if k and (best is None or st["frame_ms"] < best):
                        best = st["frame_ms"]
                return film.data, best, st
            finally:
                dev.close()

        ref, _, st = frames(a.spp * a.ref_factor, 1, n=0)
        ref_rgb = ref[..., :3].astype(np.float64)
        ref_var = xpu.film_variance(ref, a.spp * a.ref_factor)
        say(f"{name}: {W}x{H} depth {depth}, reference {a.spp * a.ref_factor} spp uniform (seed 1, {st['frame_ms']:.1f} ms with the process's start), film mean {np.nanmean(ref_rgb, (0, 1))}")
        rec = {"film": [W, H], "depth": depth, "rows": []}

        def report(label, data, ms, st, adaptive):
            rgb = data[..., :3].astype(np.float64)
            ok = np.isfinite(rgb).all(-1) & np.isfinite(ref_rgb).all(-1)
            d = rgb[ok] - ref_rgb[ok]
            n = data[..., 7].astype(np.float64) if adaptive else None
            row = {"frame": label, "frame_ms": ms, "mean_samples": float(n.mean()) if adaptive else float(st["camera_samples"]) / (W * H), "mse": float((d * d).mean()),
                   "rel_mse": float((d * d / (ref_rgb[ok] ** 2 + 1e-4)).mean()), "rays": st["rays_closest"] + st["rays_shadow"], "pixels_compared": int(ok.sum())}
            text = f"  {label:>28}: frame {ms:8.2f} ms  mean samples {row['mean_samples']:7.2f}  MSE {row['mse']:.4e}  relative MSE {row['rel_mse']:.4e}  rays {row['rays']}"
            if adaptive:
                var = xpu.film_variance(data, a.spp, adaptive=True)
                fin = ok & np.isfinite(var).all(-1) & np.isfinite(ref_var).all(-1)
                diff = rgb[fin].mean(0) - ref_rgb[fin].mean(0)
                se = np.sqrt(var[fin].sum(0) + ref_var[fin].sum(0)) / fin.sum()
                row.update({"bias": diff.tolist(), "bias_se": se.tolist(), "bias_z": (diff / se).tolist(), "bias_relative": (diff / ref_rgb[fin].mean(0)).tolist(),
                            "stopped_early": float((n < a.spp).mean())})
                text += f"  stopped early {row['stopped_early']:.3f}  bias {diff} = {diff / se} standard errors ({100 * diff / ref_rgb[fin].mean(0)} % of the mean)"
            say(text)
            rec["rows"].append(row)
            return row

        data, ms, st = frames(a.spp, 100, n=a.frames)
        full = report(f"uniform {a.spp} spp", data, ms, st, False)
        for tau in a.tau:
            data, ms, st = frames(a.spp, 100, adaptive=tau, n=a.frames)
            assert st["camera_samples"] == int(data[..., 7].astype(np.float64).sum())
            ad = report(f"adaptive tau {tau}", data, ms, st, True)
            eq = max(1, int(round(ad["mean_samples"])))
            data, ms, st = frames(eq, 100, n=a.frames)
            un = report(f"uniform {eq} spp (equal samples)", data, ms, st, False)
            say(f"  tau {tau}: against the full frame: time x {ad['frame_ms'] / full['frame_ms']:.3f}, MSE x {ad['mse'] / full['mse']:.3f}; against equal samples: time x "
                f"{ad['frame_ms'] / un['frame_ms']:.3f}, MSE x {ad['mse'] / un['mse']:.3f}, relative MSE x {ad['rel_mse'] / un['rel_mse']:.3f}")
        out["scenes"][name] = rec
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
