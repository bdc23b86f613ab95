"""What the pick of a light's triangle by area costs: the closed showroom at BASELINE config-3 size (scenes.bmw_showroom: 500 k triangles,
1920 x 1080, 1024 spp, depth 9) rendered on one GPU by

    parent   the parent commit's tree and library (--parent-root: a checkout of that commit with its library built)
    off      this tree, light_sampling = "reference" (zero-filled options)
    on       this tree, light_sampling = "area"

each in a process of its own, --rounds times, interleaved (parent, off, on, parent, off, on, ...), so that drift of the machine lands
on all three alike.  The showroom's lamps are quads of two equal triangles: off and on must deliver the same film and ray counts, which
is asserted before any time is printed (the cost is that of the table, the branch and k_shade_g's changed code, not of other paths).
Prints phx_stats' frame_ms, shade_kernel_ms (k_shade_g) and trace_ms of every run, each mode's best and range, and one JSON line.

    python scripts/light_sampling_cost.py --parent-root DIR [--rounds 3] [--frames 2] [--out profiles/r10_light_sampling_cost.log]

(The parent's library cannot be selected with PHX_LIB under this tree's loader, which declares phx_dev_light_sample: the parent runs
from its own checkout.  Without --parent-root only off and on are measured.)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(a):
    """a child process: one device, one warm-up frame, a.frames timed ones; prints one JSON line"""
    sys.path.insert(0, a.root)
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    sc = scenes.bmw_showroom(a.triangles, a.width, a.height)
    kw = {"light_sampling": "area"} if a.one == "on" else {}
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
        print(json.dumps({"mode": a.one, "frame_ms": best["frame_ms"], "trace_ms": best["trace_ms"], "shade_kernel_ms": best["shade_kernel_ms"],
                          "shade_general": best["shade_general"], "rays": best["rays_closest"] + best["rays_shadow"], "device_bytes": best["device_bytes"], **first}))
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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r10_light_sampling_cost.log"))
    ap.add_argument("--one", choices=["parent", "off", "on"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    modes = (["parent"] if a.parent_root else []) + ["off", "on"]
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
                f"{row['rays'] / row['frame_ms'] / 1e3:8.1f} Mrays/s  {row['device_bytes'] / 2**20:9.1f} MiB  film {row['film_sha']}")
    # before any comparison: one picture in all modes (the showroom's lamps are pairs of equal triangles)
    pictures = {(row["film_sha"], row["rays_closest"], row["rays_shadow"]) for m in modes for row in runs[m]}
    assert len(pictures) == 1, f"the modes rendered different films or ray counts: {pictures}"
    assert all(row["film_max"] > 0.05 and row["shade_general"] == 1 for m in modes for row in runs[m])
    out = {"scene": f"bmw_showroom({a.triangles}) {a.width}x{a.height} {a.spp} spp depth 9", "same_film_in_every_mode": True, "runs": runs}
    for key in ("frame_ms", "shade_kernel_ms", "trace_ms"):
        for m in modes:
            v = [row[key] for row in runs[m]]
            out[f"{m}_{key}"] = {"best": min(v), "median": sorted(v)[len(v) // 2], "range": max(v) - min(v)}
        s = "  ".join(f"{m} best {out[f'{m}_{key}']['best']:.1f} median {out[f'{m}_{key}']['median']:.1f} range {out[f'{m}_{key}']['range']:.1f}" for m in modes)
        say(f"{key:>16}: {s}")
    pct = lambda x, y, key: 100.0 * (out[f"{x}_{key}"]["median"] / out[f"{y}_{key}"]["median"] - 1.0)
    out["on_vs_off_pct"] = {key: pct("on", "off", key) for key in ("frame_ms", "shade_kernel_ms", "trace_ms")}
    say(f"option on against off (medians): frame {out['on_vs_off_pct']['frame_ms']:+.2f} %  k_shade_g {out['on_vs_off_pct']['shade_kernel_ms']:+.2f} %  k_trace {out['on_vs_off_pct']['trace_ms']:+.2f} %")
    if a.parent_root:
        out["off_vs_parent_pct"] = {key: pct("off", "parent", key) for key in ("frame_ms", "shade_kernel_ms", "trace_ms")}
        d = out["off_median_minus_parent_median_frame_ms"] = out["off_frame_ms"]["median"] - out["parent_frame_ms"]["median"]
        out["off_within_parent_range"] = bool(d <= out["parent_frame_ms"]["range"])
        say(f"option off against the parent (medians): frame {out['off_vs_parent_pct']['frame_ms']:+.2f} %  k_shade_g {out['off_vs_parent_pct']['shade_kernel_ms']:+.2f} %  "
            f"k_trace {out['off_vs_parent_pct']['trace_ms']:+.2f} %; frame {d:+.1f} ms against the parent's own range of {out['parent_frame_ms']['range']:.1f} ms: "
            f"{'within' if out['off_within_parent_range'] else 'OUTSIDE'} it")
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
