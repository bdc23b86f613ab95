"""What stopping converged tiles buys (render_progressive(tiles=)): scenes.bmw_showroom (200 000 triangles, 960 x 540) and
scenes.sun_floor(), 16 spp a frame, on one GPU.  Per scene: a reference, one uniform frame of --ref-spp samples (2 048); then the same
stop=dict(threshold=, floor=, coverage=) without and with tiles=dict(size=, coverage=, min_frames=), up to --frames frames, --reps times,
interleaved, each loop in a fresh child process (so that no loop inherits another's warm device); with --parent PATH the loop without tiles
also runs on that checkout's package, interleaved with the two, which is the comparison against the loop as it was.
Reported per loop: frames, the pixels rendered in all, the time of the frames (wall clock around each step of the generator: the frame, the
pooling and, with tiles, the tile map and the download of its records; the first step also holds the device's start and preprocess and is
given apart), MSE and trimmed MSE (the largest 0.1 % of the squared errors left out) over the film's RGB against the reference, the bias of
the film's mean in standard errors of the difference (per-pixel variances by film_variance from each film's own m2 channel), and with tiles
the share of tiles open per frame.  The last line is one JSON record.

    python scripts/tile_map_payoff.py [--tau 0.1] [--parent PATH] [--out profiles/r26_tile_map_payoff.log]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPP = 16


def scene_of(name, a, scenes):
    if name == "sun_floor":
        return scenes.sun_floor(a.floor_size, a.floor_size), dict(light_sampling="area", light_selection="power", environment_sampling=True), 2
    return scenes.bmw_showroom(a.triangles, a.width, a.height), {}, 9


def child(a):
    """one reference frame or one loop, on the package of a.tree -> one JSON line on stdout"""
    sys.path.insert(0, a.tree)
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    sc, kw, depth = scene_of(a.scene, a, scenes)
    W, H = sc.camera.width, sc.camera.height
    if a.child == "reference":
        film, st = xpu.render(sc, spp=a.ref_spp, depth=depth, seed=1, moments=True, native_sink=True, **kw)
        np.save(a.file, film)
        print(json.dumps({"frame_ms": st["frame_ms"], "film": [W, H], "depth": depth}))
        return
    ref = np.load(a.file)
    stop = dict(threshold=a.tau, floor=a.floor, coverage=a.coverage)
    more = dict(tiles=dict(size=a.tile, coverage=a.tile_coverage, min_frames=a.min_frames)) if a.child == "tiles" else {}
    steps, opened, rendered, film, summary = [], [], 0, None, None
    t0 = time.perf_counter()
    for film, summary, done in xpu.render_progressive(sc, SPP, a.frames, seed=100, stop=stop, depth=depth, **more, **kw):
        t1 = time.perf_counter()
        steps.append(1e3 * (t1 - t0))
        rendered += summary.get("rendered_pixels", W * H)
        if "tiles" in summary:
            opened.append(summary["tiles_open"] / summary["tiles"])
        t0 = time.perf_counter()
    film = np.array(film)
    rgb, ref_rgb = film[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    ok = np.isfinite(rgb).all(-1) & np.isfinite(ref_rgb).all(-1)
    d2 = ((rgb[ok] - ref_rgb[ok]) ** 2).ravel()
    var, ref_var = xpu.film_variance(film, 0, adaptive=True), xpu.film_variance(ref, a.ref_spp)
    fin = ok & np.isfinite(var).all(-1) & np.isfinite(ref_var).all(-1)
    diff = rgb[fin].mean(0) - ref_rgb[fin].mean(0)
    se = np.sqrt(var[fin].sum(0) + ref_var[fin].sum(0)) / fin.sum()
    n = film[..., 7].astype(np.float64)
    print(json.dumps({"frames": len(steps), "rendered_pixels": rendered, "first_step_ms": steps[0], "later_steps_ms": sum(steps[1:]), "steps_ms": steps,
                      "mse": float(d2.mean()), "trimmed_mse": float(np.sort(d2)[:max(1, int(0.999 * d2.size))].mean()), "bias_z": (diff / se).tolist(),
                      "mean_samples": float(n.mean()), "min_samples": float(n.min()), "max_samples": float(n.max()), "tiles_open_share": opened,
                      "converged": summary["converged"], "valid": summary["pixels"] - summary["invalid"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tau", type=float, default=0.1)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--coverage", type=float, default=0.95, help="stop's coverage")
    ap.add_argument("--tile", type=int, default=32)
    ap.add_argument("--tile-coverage", type=float, default=0.95)
    ap.add_argument("--min-frames", type=int, default=2)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--triangles", type=int, default=200_000)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--floor-size", type=int, default=256, help="the sun_floor film is this many pixels square")
    ap.add_argument("--scenes", nargs="+", default=["sun_floor", "bmw_showroom"])
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its loop without tiles runs interleaved with this tree's")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r26_tile_map_payoff.log"))
    ap.add_argument("--child", default=None, choices=["reference", "plain", "tiles"])
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--scene", default=None)
    ap.add_argument("--file", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(kind, scene, file, tree=HERE):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--tree", tree, "--scene", scene, "--file", file]
        for k in ("tau", "floor", "coverage", "tile", "tile_coverage", "min_frames", "frames", "ref_spp", "triangles", "width", "height", "floor_size"):
            cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        if r.returncode != 0:
            sys.exit(f"{kind} on {scene} ended with {r.returncode}: nothing more is started on the GPU\n{r.stderr[-2000:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])
    out = {"spp": SPP, "ref_spp": a.ref_spp, "stop": dict(threshold=a.tau, floor=a.floor, coverage=a.coverage),
           "tiles": dict(size=a.tile, coverage=a.tile_coverage, min_frames=a.min_frames), "frames": a.frames, "scenes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for scene in a.scenes:
            file = os.path.join(tmp, scene + ".npy")
            r = run("reference", scene, file)
            say(f"{scene}: {r['film'][0]}x{r['film'][1]} depth {r['depth']}, reference {a.ref_spp} spp uniform (seed 1, {r['frame_ms']:.0f} ms); {SPP} spp a frame, stop {out['stop']}, tiles {out['tiles']}")
            loops = [("parent", "plain", a.parent)] if a.parent else []
            loops += [("plain", "plain", HERE), ("tiles", "tiles", HERE)]
            rec = {name: [] for name, _, _ in loops}
            for rep in range(a.reps):
                for name, kind, tree in loops:
                    r = run(kind, scene, file, tree)
                    rec[name].append(r)
                    share = " ".join(f"{v:.2f}" for v in r["tiles_open_share"])
                    say(f"  {name:>6} run {rep + 1}: {r['frames']:2d} frames, {r['rendered_pixels']:9d} pixels rendered, first step {r['first_step_ms']:8.1f} ms, later steps {r['later_steps_ms']:8.1f} ms, "
                        f"MSE {r['mse']:.4e} trimmed {r['trimmed_mse']:.4e}, bias {['%.2f' % z for z in r['bias_z']]} se, samples {r['min_samples']:.0f} .. {r['max_samples']:.0f} (mean {r['mean_samples']:.1f}), "
                        f"converged {r['converged']} of {r['valid']}" + (f", tiles open per frame: {share}" if share else ""))
            best = {name: min(r["later_steps_ms"] for r in runs) for name, runs in rec.items()}
            say(f"  best later-steps time: " + ", ".join(f"{k} {v:.1f} ms" for k, v in best.items()) + f"; tiles / plain = {best['tiles'] / best['plain']:.3f}, "
                f"pixels rendered tiles / plain = {rec['tiles'][0]['rendered_pixels'] / rec['plain'][0]['rendered_pixels']:.3f}")
            out["scenes"][scene] = rec
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
