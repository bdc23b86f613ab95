"""What a camera move costs (phx_dev_set_camera) beside the only way there was before it, a full phx_dev_preprocess with the new camera:
the bench scene (scenes.soup of --triangles triangles at 1280 x 720), --calls of each on one device, host clock around the call (preprocess
also by its own phx_stats.preprocess_ms and bvh_build_ms).  After the timed calls the script checks what the tests check at small sizes: a
frame behind set_camera(B) equals a frame behind preprocess(scene with B), bit for bit.

    python scripts/set_camera_cost.py [--calls 10] [--out profiles/r22_set_camera_cost.log]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r22_set_camera_cost.log"))
    a = ap.parse_args()
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    sc = scenes.soup(a.triangles, seed=1234, width=a.width, height=a.height)
    M = sc.camera.to_world.copy()
    M[3, :3] += (0.05, 0.02, -0.03)
    cams = [sc.camera, dataclasses.replace(sc.camera, to_world=M)]
    scs = [sc, dataclasses.replace(sc, camera=cams[1])]
    W, H = a.width, a.height
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.spp, paths_per_sample=1, path_depth=9))

    def frame(scene):
        film = xpu.Film(W, H, 4, False, False, False)
        dev.start(scene, xpu.FrameState(1, xpu.Tiles.make(W, H, 32), film, native_sink=True))
        dev.join()
        return film.data
    try:
        pre, own, bvh, setc = [], [], [], []
        for k in range(a.calls + 1):  # the first of each is the warm-up
            t0 = time.perf_counter()
            dev.preprocess(scs[k & 1])
            t1 = time.perf_counter()
            st = dev.stats()
            if k:
                pre.append(1e3 * (t1 - t0)); own.append(st["preprocess_ms"]); bvh.append(st["bvh_build_ms"])
        for k in range(a.calls + 1):
            t0 = time.perf_counter()
            dev.set_camera(cams[k & 1])
            t1 = time.perf_counter()
            if k:
                setc.append(1e3 * (t1 - t0))
        med = lambda v: sorted(v)[len(v) // 2]
        say(f"soup of {a.triangles} triangles, {W}x{H}: {a.calls} calls each")
        say(f"  preprocess with the new camera (the scene packed and handed over): {med(pre):.2f} ms ({min(pre):.2f} - {max(pre):.2f}); "
            f"its own clock {med(own):.2f} ms, of which the tree {med(bvh):.2f} ms")
        say(f"  set_camera (the camera packed and handed over): {med(setc):.4f} ms ({min(setc):.4f} - {max(setc):.4f});  preprocess / set_camera = {med(pre) / med(setc):.0f}")
        dev.preprocess(scs[0])
        dev.set_camera(cams[1])
        moved = frame(scs[0]).copy()
        dev.preprocess(scs[1])
        fresh = frame(scs[1])
        same = bool(np.array_equal(moved.view(np.uint32), fresh.view(np.uint32)))
        say(f"  a frame of {a.spp} spp behind set_camera equals the frame behind a fresh preprocess bit for bit: {same}")
        say(json.dumps({"triangles": a.triangles, "film": [W, H], "preprocess_ms": med(pre), "preprocess_own_ms": med(own), "bvh_build_ms": med(bvh),
                        "set_camera_ms": med(setc), "frames_equal": same}))
        if not same:
            sys.exit("the frames differ")
    finally:
        dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
