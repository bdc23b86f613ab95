"""What image masks on closure mixes cost: the closed showroom at BASELINE config-3 size (scenes.masked_showroom: 500 k triangles,
1920 x 1080, 1024 spp, depth 9), its six diffuse recipes turned into mix(diffuse, glossy, mask), rendered on one GPU in three modes:

    image      procedural 2048^2 LINEAR masks                      k_shade_g<PERHIT, ., ., TEX, ., MASK>, lookups all over the images
    one_texel  1 x 1 masks holding each image's mean               the same kernels, every lookup hits one texel
    baked      the mix each 1 x 1 mask gives as constant weights   the kernels of an unmasked scene (FAC_NONE lobes, no image, no UVs)

"image vs one_texel" is the texel gathers, "one_texel vs baked" the MASK instantiations themselves.  The baked scene's weights are
computed in fp32 in the device's order from each mask's one texel (scenes.resolve_masks), so the one_texel and baked films must be
bit-identical: that is asserted before any time is printed.  Prints phx_stats' frame_ms, shade_kernel_ms and trace_ms of each mode and
one JSON line at the end.

    python scripts/mask_cost.py [--spp 1024] [--tex 2048] [--frames 2]
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
        best, first = None, None
        for k in range(frames + 1):  # the first frame warms up (allocations, code objects) and is not counted; its film and ray counts (seed 1) are kept
            film = xpu.Film(W, H, 4)
            dev.start(sc, xpu.FrameState(1 + k, xpu.Tiles.make(W, H, 32), film, native_sink=True))
            dev.join()
            st = dev.stats()
            if k == 0:
                first = (film.data.copy(), st["rays_closest"], st["rays_shadow"])
            if k and (best is None or st["frame_ms"] < best["frame_ms"]):
                best = st
        return {"scene": sc.name, "frame_ms": best["frame_ms"], "trace_ms": best["trace_ms"], "shade_kernel_ms": best["shade_kernel_ms"],
                "shade_ms": best["shade_ms"], "rays": best["rays_closest"] + best["rays_shadow"], "device_bytes": best["device_bytes"],
                "preprocess_s": pre}, first
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
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    rows, films = {}, {}
    for mode in ("image", "one_texel", "baked"):
        rows[mode], films[mode] = run(xpu, scenes.masked_showroom(a.triangles, a.width, a.height, a.tex, mode), a.spp, a.frames)
        if mode == "baked":  # before any time is printed: the constant masks and their baked mix are the same picture, bit for bit
            (fo, *ro), (fb, *rb) = films["one_texel"], films["baked"]  # the frames of seed 1
            assert ro == rb, f"one_texel and baked ray counts differ: {ro} / {rb}"
            differ = int((fo.view(np.uint32) != fb.view(np.uint32)).any(-1).sum())
            assert differ == 0, f"one_texel and baked films differ in {differ} pixels"
            assert np.nanmax(fb[..., :3]) > 0.05  # lit (the closed room has the reference's few non-finite pixels: scripts/nonfinite_probe.py)
    for mode, r in rows.items():
        print(f"{r['scene']:>36}: frame {r['frame_ms']:9.1f} ms  trace {r['trace_ms']:9.1f} ms  shade kernels {r['shade_kernel_ms']:9.1f} ms  "
              f"{r['rays'] / r['frame_ms'] / 1e3:8.1f} Mrays/s  {r['device_bytes'] / 2**20:8.1f} MiB", flush=True)
    pct = lambda x, y, k: 100.0 * (rows[x][k] / rows[y][k] - 1.0)
    out = dict(rows)
    out["one_texel_film_equals_baked_film"] = True
    out["texel_gather_cost"] = {"frame_pct": pct("image", "one_texel", "frame_ms"), "shade_kernel_pct": pct("image", "one_texel", "shade_kernel_ms"),
                                "trace_pct": pct("image", "one_texel", "trace_ms")}
    out["mask_instantiation_cost"] = {"frame_pct": pct("one_texel", "baked", "frame_ms"), "shade_kernel_pct": pct("one_texel", "baked", "shade_kernel_ms"),
                                      "trace_pct": pct("one_texel", "baked", "trace_ms")}
    out["feature_cost"] = {"frame_pct": pct("image", "baked", "frame_ms"), "shade_kernel_pct": pct("image", "baked", "shade_kernel_ms")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
