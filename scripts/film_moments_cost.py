"""What the per-pixel error estimate (phx_frame.moments_channel, k_film_moments instead of k_film) costs on the bench frame: BASELINE
configs[1] (Soup 100 k, 1280 x 720, 256 spp, depth 9) on one GPU into a device-resident film, as bench.py renders it, with the channel

    off      moments = False: k_film
    on       moments = True:  k_film_moments, 3 more floats per pixel in the batch buffer and the film

each in a process of its own, --rounds times, interleaved (off, on, off, ...), so that drift of the machine lands on both alike.  Before any
time is printed the script asserts that `primary` (hashed) and the ray counts are the same in every run, off and on, and that the channel
is there when asked for.  Prints phx_stats' frame_ms and the begin-pass + film launches' share of shade_ms (shade_ms - shade_kernel_ms:
the HIP-event time of the Launch::Pass launches, of which the film kernel is all but the one-thread k_begin_pass) of every run, each
mode's best, median and range, and one JSON line.

    python scripts/film_moments_cost.py [--rounds 3] [--frames 3] [--out profiles/r15_film_moments_cost.log]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("frame_ms", "pass_ms", "shade_kernel_ms", "trace_ms")


def one(a):
    """a child process: one device, one warm-up frame, a.frames timed ones; prints one JSON line"""
    sys.path.insert(0, HERE)
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    hip = C.CDLL("libamdhip64.so.7")  # the runtime the library runs on
    on = a.one == "on"
    sc = scenes.soup(a.triangles, width=a.width, height=a.height)
    W, H, xs = a.width, a.height, 4 + (3 if on else 0)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.spp, paths_per_sample=1, path_depth=9))
    ptr = C.c_void_p()
    try:
        dev.preprocess(sc)
        assert hip.hipMalloc(C.byref(ptr), C.c_size_t(W * H * xs * 4)) == 0
        best, first = None, None
        for k in range(a.frames + 1):  # the first frame warms up and is not counted; its film (seed 1) is hashed
            dev.start(sc, xpu.FrameState(1 + k, xpu.Tiles.make(W, H, 32), None, device_film_ptr=ptr.value, moments=on))
            dev.join()
            st = dev.stats()
            st["pass_ms"] = st["shade_ms"] - st["shade_kernel_ms"]
            if k == 0:
                film = np.empty((H, W, xs), np.float32)
                assert hip.hipMemcpy(film.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(film.nbytes), 2) == 0
                first = {"primary_sha": hashlib.sha256(np.ascontiguousarray(film[..., :4]).tobytes()).hexdigest()[:16], "rays_closest": st["rays_closest"],
                         "rays_shadow": st["rays_shadow"], "rays_masked": st["rays_masked"], "camera_samples": st["camera_samples"],
                         "film_mean": float(film[..., :3].mean()),
                         "m2_positive": float((film[..., 4:] > 0).any(-1).mean()) if on else None,
                         "mean_relative_standard_error": float(np.mean(np.sqrt(xpu.film_variance(film, a.spp)[film[..., :3] > 0]) / film[..., :3][film[..., :3] > 0])) if on else None}
            if k and (best is None or st["frame_ms"] < best["frame_ms"]):
                best = st
        print(json.dumps({"mode": a.one, **{key: best[key] for key in KEYS}, "device_bytes": best["device_bytes"], "paths_in_flight": best["paths_in_flight"], **first}))
    finally:
        dev.close()
        if ptr.value:
            hip.hipFree(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r15_film_moments_cost.log"))
    ap.add_argument("--one", choices=["off", "on"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    modes = ["off", "on"]
    runs = {m: [] for m in modes}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for r in range(a.rounds):
        for m in modes:
            env = {k: v for k, v in os.environ.items() if k != "PHX_LIB"}
            cmd = [sys.executable, os.path.abspath(__file__), "--one", m, "--triangles", str(a.triangles), "--width", str(a.width),
                   "--height", str(a.height), "--spp", str(a.spp), "--frames", str(a.frames)]
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
            if p.returncode:
                sys.exit(f"{m}, round {r}: exit status {p.returncode}\n{p.stdout}\n{p.stderr}")  # nothing more is started on the GPU
            row = json.loads(p.stdout.strip().splitlines()[-1])
            runs[m].append(row)
            say(f"round {r} {m:>3}: frame {row['frame_ms']:8.2f} ms  begin-pass + film {row['pass_ms']:7.3f} ms  k_shade {row['shade_kernel_ms']:7.2f} ms  trace {row['trace_ms']:7.2f} ms  "
                f"{(row['rays_closest'] + row['rays_shadow']) / row['frame_ms'] / 1e3:8.1f} Mrays/s  {row['device_bytes']:12d} B  primary {row['primary_sha']}")
    # before any comparison: one `primary` and one set of ray counts, off and on
    pictures = {(row["primary_sha"], row["camera_samples"], row["rays_closest"], row["rays_shadow"], row["rays_masked"]) for m in modes for row in runs[m]}
    assert len(pictures) == 1, f"the runs rendered different primary channels or ray counts: {pictures}"
    assert all(row["film_mean"] > 0.05 for m in modes for row in runs[m]) and all(row["m2_positive"] > 0.1 for row in runs["on"])
    say(f"channel on: {runs['on'][0]['m2_positive']:.3f} of the pixels have m2 > 0; mean relative standard error of the lit values {runs['on'][0]['mean_relative_standard_error']:.4f}")
    out = {"scene": f"soup({a.triangles}) {a.width}x{a.height} {a.spp} spp depth 9, device-resident film", "same_primary_and_ray_counts": True, "runs": runs}
    for key in KEYS:
        for m in modes:
            v = [row[key] for row in runs[m]]
            out[f"{m}_{key}"] = {"best": min(v), "median": sorted(v)[len(v) // 2], "range": max(v) - min(v)}
        s = "  ".join(f"{m} best {out[f'{m}_{key}']['best']:.3f} median {out[f'{m}_{key}']['median']:.3f} range {out[f'{m}_{key}']['range']:.3f}" for m in modes)
        say(f"{key:>16}: {s}")
    out["on_vs_off"] = {}
    for key in KEYS:
        d = out[f"on_{key}"]["median"] - out[f"off_{key}"]["median"]
        rng = out[f"off_{key}"]["range"]
        out["on_vs_off"][key] = {"median_difference_ms": d, "percent": 100.0 * d / out[f"off_{key}"]["median"], "off_range_ms": rng, "within_range": bool(abs(d) <= rng)}
        say(f"channel on against off, {key}: {d:+.3f} ms ({100.0 * d / out[f'off_{key}']['median']:+.2f} %) between the medians; off's own range is {rng:.3f} ms: "
            f"{'within' if abs(d) <= rng else 'OUTSIDE'} it")
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
