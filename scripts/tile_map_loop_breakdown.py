"""Where a progressive step's time goes, with and without tiles=: the loop of render_progressive by hand on scenes.sun_floor and
scenes.bmw_showroom (200 000 triangles, 960 x 540), 16 spp a frame, stop tau 0.1 floor 0.01 coverage 0.95, tiles of 32 at coverage 0.95 from the
third frame on, with a timer round every piece of a step: the tile map (a host accumulator: its upload included), the open list and its queue,
the frame film's allocation, the frame (wall clock and phx_stats' frame_ms), the pooling.  Plain, tiles, plain, tiles; sums over the frames
behind the first, and the first four and last three frames of each loop.

    python scripts/tile_map_loop_breakdown.py > profiles/r26_loop_breakdown.log      # on an MI355X
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from phosphorus_mk2_amd import scenes, xpu
SPP, TAU, FLOOR = 16, 0.1, 0.01
def run(name, sc, depth, kw, by_tiles, frames=24, cov=0.95, min_frames=2):
    W, H = sc.camera.width, sc.camera.height
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=depth, **kw))
    T = dict(map=0.0, queue=0.0, film=0.0, frame_wall=0.0, frame_ms=0.0, pool=0.0); rows = []
    try:
        if by_tiles: dev.set_adaptive(threshold=0.0, floor=0.0, min_samples=SPP, step=1)
        dev.preprocess(sc)
        acc = xpu.accumulator(W, H)
        for k in range(frames):
            t = [time.perf_counter()]
            if by_tiles and k >= min_frames:
                rec, _ = dev.tile_map(acc, 32, TAU, FLOOR, summary=False); t.append(time.perf_counter())
                tl = xpu.open_tiles(rec, cov)
                if not tl: break
                q = xpu.Tiles.from_list(tl, W, H)
            else:
                t.append(time.perf_counter()); q = xpu.Tiles.make(W, H, 32)
            t.append(time.perf_counter())
            film = xpu.Film(W, H, 4, False, True, by_tiles); t.append(time.perf_counter())
            dev.start(sc, xpu.FrameState(100 + k, q, film, native_sink=True)); dev.join(); t.append(time.perf_counter())
            fm = dev.stats()["frame_ms"]
            _, s = dev.accumulate(acc, film.data, SPP, 4, False, by_tiles, threshold=TAU, floor=FLOOR); t.append(time.perf_counter())
            d = [1e3 * (b - a) for a, b in zip(t, t[1:])]
            if k >= 1:
                for key, v in zip(("map", "queue", "film", "frame_wall", "pool"), d): T[key] += v
                T["frame_ms"] += fm
            rows.append((len(q), round(fm, 2), [round(v, 2) for v in d]))
            valid = s["pixels"] - s["invalid"]
            if valid > 0 and s["converged"] >= 0.95 * valid: break
    finally:
        dev.close()
    print(name, "tiles" if by_tiles else "plain", "frames", len(rows), "sums over frames 2..: ", {k: round(v, 1) for k, v in T.items()}, flush=True)
    for r in rows[:4] + rows[-3:]: print("   tiles, frame_ms, [map, queue, film, frame wall, pool] ms:", r, flush=True)
cases = [("sun_floor", scenes.sun_floor(256, 256), 2, dict(light_sampling="area", light_selection="power", environment_sampling=True)),
         ("bmw_showroom", scenes.bmw_showroom(200_000, 960, 540), 9, {})]
for name, sc, depth, kw in cases:
    for by_tiles in (False, True, False, True):
        run(name, sc, depth, kw, by_tiles)
