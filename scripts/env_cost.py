"""What the environment lookup costs: the open showroom lit through its open side by a lat-long sky (scenes.environment_showroom:
500 k triangles, 1920 x 1080, 1024 spp, depth 9, BASELINE config-3 size) rendered three times on one GPU — with a procedural 2048 x 1024
HDR sky, with a 1 x 1 image of the sky's mean (the same kernels, k_shade_g<.., ENV>, whose lookups then read one texel) and with the
sky's mean as a constant environment (the kernels without the lookup).  Prints phx_stats' frame_ms, trace_ms and shade_kernel_ms of
each; one JSON line at the end.

    python scripts/env_cost.py [--spp 1024] [--sky 2048] [--frames 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from texture_cost import run  # noqa: E402  (the same timing loop: the first frame warms up, the fastest of the rest is kept)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--sky", type=int, default=2048, help="sky width (height = width / 2)")
    ap.add_argument("--frames", type=int, default=2)
    a = ap.parse_args()
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    rows = []
    for mode in ("image", "mean", "constant"):
        sc = scenes.environment_showroom(a.triangles, a.width, a.height, (a.sky, a.sky // 2), mode=mode)
        r = run(xpu, sc, a.spp, a.frames)
        rows.append(r)
        print(f"{r['scene']:>40}: frame {r['frame_ms']:9.1f} ms  trace {r['trace_ms']:9.1f} ms  shade kernels {r['shade_kernel_ms']:9.1f} ms  "
              f"{r['rays'] / r['frame_ms'] / 1e3:8.1f} Mrays/s  {r['device_bytes'] / 2**20:8.1f} MiB", flush=True)
    i, m, c = rows
    out = {"sky": i, "mean_1x1": m, "constant": c,
           "lookup_cost_vs_1x1": {"frame_pct": 100.0 * (i["frame_ms"] / m["frame_ms"] - 1.0),
                                  "shade_kernel_pct": 100.0 * (i["shade_kernel_ms"] / m["shade_kernel_ms"] - 1.0)},
           "env_kernels_vs_constant": {"frame_pct": 100.0 * (m["frame_ms"] / c["frame_ms"] - 1.0),
                                       "shade_kernel_pct": 100.0 * (m["shade_kernel_ms"] / c["shade_kernel_ms"] - 1.0)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
