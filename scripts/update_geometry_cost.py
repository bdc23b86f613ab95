#!/usr/bin/env python
"""What a geometry update costs against a fresh preprocess, and what a refitted tree costs the traversal.

    python scripts/update_geometry_cost.py [--scenes soup100k,soup1m,bmw500k,textured500k] [--runs 5] [--parent DIR] [--variants parent,preprocess]
                                           [--motions rigid] [--out profiles/NAME.log]

Per scene, every variant in a fresh process of its own, the variants alternating run by run; medians with the spread (min .. max):

  preprocess(moved)        the yardstick: phx_stats.preprocess_ms of a device that is handed the moved scene
  parent                   the same on another checkout of the project (--parent DIR, its library built: the commit this one is compared
                           with), run by that checkout's own Python package: preprocess is not meant to change
  parent-rebuild, parent-refit   the two updates on that checkout likewise (rigid move only), each run just before this tree's
  update(rebuild)          HipDevice.update_geometry(moved, "rebuild"): the call's four timers
  update(refit)            HipDevice.update_geometry(moved, "refit"): the call's four timers
  trace after refit / rebuild   phx_stats.trace_ms of one frame (the kernels' HIP events) for a rigid move of one object and for wobbles of
                           1 %, 5 % and 20 % of the scene's extent, on the refitted and on the rebuilt tree

Measured and reported, never asserted.  A child prints one JSON line; the parent prints the table and, with --out, writes it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("PHX_COST_TREE") or ROOT)  # (a child measuring the parent checkout imports that checkout's package)

SCENES = {"soup100k": ("soup", 100_000), "soup1m": ("soup", 1_000_000), "bmw500k": ("bmw_showroom", 500_000), "textured500k": ("textured_showroom", 500_000)}
MOTIONS = ["rigid", "wobble1", "wobble5", "wobble20"]
VARIANTS = ["parent", "preprocess", "parent-rebuild", "rebuild", "parent-refit", "refit"]  # in the order they alternate in
W, H, SPP = 640, 360, 4


def scene_of(name):
    from phosphorus_mk2_amd import scenes
    kind, n = SCENES[name]
    return getattr(scenes, kind)(n, width=W, height=H)


def moved_scene(sc, motion):
    """(numpy alone, so that a checkout without scenes.transformed / scenes.wobbled moves the scene the same way)"""
    import dataclasses
    import numpy as np
    v = np.concatenate([m.vertices for m in sc.meshes])
    extent = float((v.max(0) - v.min(0)).max())
    meshes = list(sc.meshes)
    if motion == "rigid":  # the largest mesh moves by a tenth of the scene's extent
        k = max(range(len(meshes)), key=lambda i: len(meshes[i].faces))
        meshes[k] = dataclasses.replace(meshes[k], vertices=(meshes[k].vertices + np.array([0.1 * extent, 0, 0], np.float32)).astype(np.float32))
    else:
        rng = np.random.default_rng(1)
        a = 0.01 * float(motion[6:]) * extent
        meshes = [dataclasses.replace(m, vertices=(m.vertices + rng.uniform(-a, a, m.vertices.shape).astype(np.float32)).astype(np.float32)) for m in meshes]
    return dataclasses.replace(sc, meshes=meshes)


def child(name, variant, motion):
    from phosphorus_mk2_amd import xpu
    sc = scene_of(name)
    new = moved_scene(sc, motion)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=5))
    out = {"scene": name, "variant": variant, "motion": motion}
    try:
        mode = variant.split("-")[-1]  # (parent-rebuild, parent-refit: the parent checkout's update)
        if mode in ("preprocess", "parent"):
            dev.preprocess(sc)  # warm: code objects, allocations
            dev.preprocess(new)
            out["ms"] = dev.stats()["preprocess_ms"]
        else:
            dev.preprocess(sc)
            dev.update_geometry(sc, mode)  # warm
            dev.update_geometry(new, mode)
            out.update(dev.update_geometry_times()); out["ms"] = out["call"]
        frames = []
        for seed in (1, 2, 3):
            film = xpu.Film(W, H, 4, False)
            dev.start(new, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, native_sink=True))
            dev.join()
            frames.append(dev.stats()["trace_ms"])
        out["trace_ms"] = statistics.median(frames[1:])
    finally:
        dev.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="soup100k,soup1m,bmw500k")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--parent", help="another checkout of the project, built: its preprocess and its updates are timed beside this one's")
    ap.add_argument("--variants", default=",".join(VARIANTS), help="which of them to run")
    ap.add_argument("--motions", default=",".join(MOTIONS), help="which of them to run")
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    lines = []

    def say(text):
        print(text, flush=True); lines.append(text)
    fmt = lambda xs: f"{statistics.median(xs):9.3f} ({min(xs):.3f} .. {max(xs):.3f})"
    for name in a.scenes.split(","):
        results = {}
        for motion in MOTIONS:
            # the preprocess's time does not depend on the motion: it is measured under the rigid move; the wobbles compare the two updates' trees
            variants = [v for v in VARIANTS if v in a.variants.split(",") and (a.parent or not v.startswith("parent")) and (motion == "rigid" or v in ("rebuild", "refit"))]
            if motion not in a.motions.split(","):
                continue
            for run in range(a.runs):
                for variant in variants:  # alternating: one of each per round
                    env = dict(os.environ, PHX_COST_TREE=os.path.abspath(a.parent)) if variant.startswith("parent") else None
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, variant, motion], capture_output=True, text=True, timeout=600, env=env)
                    got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                    if r.returncode != 0 or not got:
                        say(f"{name} {variant} {motion}: child failed ({r.returncode}): {r.stderr[-300:]}")
                        return 1
                    results.setdefault((variant, motion), []).append(json.loads(got[0][7:]))
                    print(f"  {name} {motion} run {run + 1} {variant}: {results[(variant, motion)][-1]['ms']:.3f} ms", file=sys.stderr, flush=True)  # progress
        say(f"== {name}: {W} x {H}, {SPP} spp, depth 5; ms, median (min .. max)")
        for motion in MOTIONS:
            for variant in VARIANTS:
                if (variant, motion) not in results:
                    continue
                rs = results[(variant, motion)]
                text = f"{motion:9s} {variant:14s} n={len(rs)} call {fmt([r['ms'] for r in rs])}  trace/frame {fmt([r['trace_ms'] for r in rs])}"
                if variant.endswith(("rebuild", "refit")):
                    text += "  flatten {} upload {} device {}".format(*(fmt([r[k] for r in rs]) for k in ("flatten", "upload", "device")))
                say(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
