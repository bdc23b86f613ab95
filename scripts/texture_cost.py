"""What the texel gathers cost: the closed showroom at BASELINE config-3 size (scenes.textured_showroom: 500 k triangles, 1920 x 1080,
1024 spp, depth 9) rendered twice on one GPU — once with procedural 2048^2 LINEAR textures on its diffuse recipes, once with the same
scene whose textures are 1 x 1 images of their means (the same kernel, k_shade_g<., ., ., TEX>, whose lookups then hit one texel).
Prints phx_stats' shade_kernel_ms, trace_ms and frame_ms of each, and the untextured bmw_showroom for scale; one JSON line at the end.

    python scripts/texture_cost.py [--spp 1024] [--tex 2048] [--frames 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(xpu, sc, spp, frames):
    opts = xpu.Options(samples_per_pixel=spp, paths_per_sample=1, path_depth=9)
    dev = xpu.HipDevice.make(opts)
    try:
        t0 = time.perf_counter()
        dev.preprocess(sc)
        pre = time.perf_counter() - t0
        W, H = sc.camera.width, sc.camera.height
        best = None
        for k in range(frames + 1):  # the first frame warms up (allocations, code objects) and is not counted
            film = xpu.Film(W, H, 4)
            dev.start(sc, xpu.FrameState(1 + k, xpu.Tiles.make(W, H, 32), film, native_sink=True))
            dev.join()
            st = dev.stats()
            if k and (best is None or st["frame_ms"] < best["frame_ms"]):
                best = st
        import numpy as np
        return {"scene": sc.name, "frame_ms": best["frame_ms"], "trace_ms": best["trace_ms"], "shade_kernel_ms": best["shade_kernel_ms"],
                "shade_ms": best["shade_ms"], "rays": best["rays_closest"] + best["rays_shadow"], "device_bytes": best["device_bytes"],
                "preprocess_s": pre, "film_mean": float(np.nanmean(film.data[..., :3]))}
    finally:
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--tex", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=2)
    a = ap.parse_args()
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    rows = []
    for sc in (scenes.textured_showroom(a.triangles, a.width, a.height, a.tex),
               scenes.textured_showroom(a.triangles, a.width, a.height, a.tex, baked=True),
               scenes.bmw_showroom(a.triangles, a.width, a.height)):
        r = run(xpu, sc, a.spp, a.frames)
        rows.append(r)
        print(f"{r['scene']:>32}: frame {r['frame_ms']:9.1f} ms  trace {r['trace_ms']:9.1f} ms  shade kernels {r['shade_kernel_ms']:9.1f} ms  "
              f"{r['rays'] / r['frame_ms'] / 1e3:8.1f} Mrays/s  {r['device_bytes'] / 2**20:8.1f} MiB", flush=True)
    t, b = rows[0], rows[1]
    out = {"textured": t, "baked_1x1": b, "untextured": rows[2],
           "texel_gather_cost": {"frame_pct": 100.0 * (t["frame_ms"] / b["frame_ms"] - 1.0),
                                 "shade_kernel_pct": 100.0 * (t["shade_kernel_ms"] / b["shade_kernel_ms"] - 1.0),
                                 "shade_kernel_ms": t["shade_kernel_ms"] - b["shade_kernel_ms"]}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
