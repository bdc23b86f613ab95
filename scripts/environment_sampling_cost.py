"""What sampling the environment costs, with the bit clear and with it set: the OPEN showroom of DESIGN 10 (scenes.environment_showroom: 500 k
triangles under the 2048 x 1024 procedural sky) at BASELINE config-3 size (1920 x 1080, 1024 spp, depth 9), rendered on one GPU by

    parent   the parent commit's tree and library, light_sampling 0x101 (--parent-root: a checkout of that commit with its library built)
    power    this tree, light_sampling 0x101 ("area" + "power"): the ENV kernels with the new branch not taken
    env      this tree, light_sampling 0x301 (environment_sampling=True)

each in a process of its own, --rounds times, interleaved (parent, power, env, parent, ...), so that drift of the machine lands on all
three alike.  parent and power must deliver one film and one set of ray counts, which is asserted before any time is printed; "power against
parent" is the cost of k_shade_g<.., ENV>'s changed code with the bit clear, held against the parent's own run-to-run range.  "env against
power" is what the samples cost: one more table search and image lookup per hit, and a shadow ray to infinity for most of them.
Prints phx_stats' frame_ms, shade_kernel_ms (k_shade_g) and trace_ms of every run, each mode's best, median and range, and one JSON line.

    python scripts/environment_sampling_cost.py --parent-root DIR [--rounds 3] [--frames 2] [--out profiles/r13_environment_sampling_cost.log]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("frame_ms", "shade_kernel_ms", "trace_ms")


def one(a):
    """a child process: one device, one warm-up frame, a.frames timed ones; prints one JSON line"""
    sys.path.insert(0, a.root)
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    sc = scenes.environment_showroom(a.triangles, a.width, a.height)
    kw = {"light_sampling": "area", "light_selection": "power"}
    if a.one == "env":
        kw["environment_sampling"] = True
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.spp, paths_per_sample=1, path_depth=9, **kw))
    try:
        dev.preprocess(sc)
        W, H = sc.camera.width, sc.camera.height
        best, first = None, None
        for k in range(a.frames + 1):  # the first frame warms up and is not counted; its film (seed 1) is hashed
            film = xpu.Film(W, H, 4)
            dev.start(sc, xpu.FrameState(1 + k, xpu.Tiles.make(W, H, 32), film, native_sink=True))
            dev.join()
            st = dev.stats()
            if k == 0:
                first = {"film_sha": hashlib.sha256(np.ascontiguousarray(film.data[..., :3]).tobytes()).hexdigest()[:16], "rays_closest": st["rays_closest"],
                         "rays_shadow": st["rays_shadow"], "film_max": float(np.nanmax(film.data[..., :3]))}
            if k and (best is None or st["frame_ms"] < best["frame_ms"]):
                best = st
        print(json.dumps({"mode": a.one, **{key: best[key] for key in KEYS}, "shade_general": best["shade_general"],
                          "rays": best["rays_closest"] + best["rays_shadow"], "device_bytes": best["device_bytes"], **first}))
    finally:
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r13_environment_sampling_cost.log"))
    ap.add_argument("--one", choices=["parent", "power", "env"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    modes = (["parent"] if a.parent_root else []) + ["power", "env"]
    runs = {m: [] for m in modes}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for r in range(a.rounds):
        for m in modes:
            root = os.path.abspath(a.parent_root) if m == "parent" else HERE
            env = {k: v for k, v in os.environ.items() if k != "PHX_LIB"}
            cmd = [sys.executable, os.path.abspath(__file__), "--one", m, "--root", root, "--triangles", str(a.triangles), "--width", str(a.width),
                   "--height", str(a.height), "--spp", str(a.spp), "--frames", str(a.frames)]
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
            if p.returncode:
                sys.exit(f"{m}, round {r}: exit status {p.returncode}\n{p.stdout}\n{p.stderr}")  # nothing more is started on the GPU
            row = json.loads(p.stdout.strip().splitlines()[-1])
            runs[m].append(row)
            say(f"round {r} {m:>6}: frame {row['frame_ms']:9.1f} ms  k_shade_g {row['shade_kernel_ms']:9.1f} ms  k_trace {row['trace_ms']:9.1f} ms  "
                f"{row['rays'] / row['frame_ms'] / 1e3:8.1f} Mrays/s  {row['device_bytes']:12d} B  film {row['film_sha']}")
    # before any comparison: one picture with the bit clear, in the parent and in this tree
    pictures = {(row["film_sha"], row["rays_closest"], row["rays_shadow"]) for m in modes if m != "env" for row in runs[m]}
    assert len(pictures) == 1, f"the bit-clear modes rendered different films or ray counts: {pictures}"
    assert len({(row["film_sha"], row["rays_shadow"]) for row in runs["env"]}) == 1 and runs["env"][0]["film_sha"] != runs["power"][0]["film_sha"]
    assert all(row["film_max"] > 0.05 and row["shade_general"] == 1 for m in modes for row in runs[m])
    out = {"scene": f"environment_showroom({a.triangles}) {a.width}x{a.height} {a.spp} spp depth 9", "same_film_with_the_bit_clear": True, "runs": runs}
    for key in KEYS:
        for m in modes:
            v = [row[key] for row in runs[m]]
            out[f"{m}_{key}"] = {"best": min(v), "median": sorted(v)[len(v) // 2], "range": max(v) - min(v)}
        s = "  ".join(f"{m} best {out[f'{m}_{key}']['best']:.1f} median {out[f'{m}_{key}']['median']:.1f} range {out[f'{m}_{key}']['range']:.1f}" for m in modes)
        say(f"{key:>16}: {s}")

    def against(x, y, what):
        out[f"{x}_vs_{y}"] = {}
        for key in KEYS:
            d = out[f"{x}_{key}"]["median"] - out[f"{y}_{key}"]["median"]
            rng = out[f"{y}_{key}"]["range"]
            out[f"{x}_vs_{y}"][key] = {"median_difference_ms": d, "percent": 100.0 * d / out[f"{y}_{key}"]["median"], f"{y}_range_ms": rng, "within_range": bool(abs(d) <= rng)}
            say(f"{what}, {key}: {d:+.2f} ms ({100.0 * d / out[f'{y}_{key}']['median']:+.2f} %) between the medians; {y}'s own range is {rng:.2f} ms: "
                f"{'within' if abs(d) <= rng else 'OUTSIDE'} it")
    if a.parent_root:
        against("power", "parent", "bit clear against the parent")
    against("env", "power", "bit set against clear")
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
