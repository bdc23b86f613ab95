"""What the tile map costs (phx_dev_film_tile_map): one call on a device-resident accumulator at 1280 x 720 and at 3840 x 2160, in
tiles of 16, 32 and 64 pixels, in two layouts: "plain", an accumulator of 8 floats a pixel (primary rgba, m2, samples), what render_progressive
maps by default, and "normals", 11 floats.  The records stay on the device (on_device = 1): what is timed is the kernel and the call, not a
download of 40 bytes a tile.

The kernel's time (phx_dev_tile_map_times: HIP events around the one launch) is put against
  (a) the byte model: the kernel reads 7 floats a pixel, 28 bytes, if only the floats it uses counted, and the whole film, 4 * xstride = 32 /
      44 bytes a pixel, if every 128-byte line it touches is fetched whole, which at these strides is every line; it writes 40 bytes a tile;
  (b) a device-to-device copy (hipMemcpyAsync, HIP events around it) that moves the film's number of bytes over the memory bus: a copy of B
      bytes reads B and writes B, so B = half the film; and
  (c) k_accumulate's own figure for the same accumulator and a uniform frame film of one float less (phx_dev_accumulate_times), which moves
      4 * (2 * xstride + xstride - 1) bytes a pixel.
Calls alternate (tile map, copy, accumulate, tile map, ...): --warmup of each, then --calls timed of each; medians and ranges.  PHX_LIB selects
another build of the library (the LDS-staged kernel: -DPHX_TILE_MAP_STAGED=1, csrc/tile_map.hip).

    python scripts/tile_map_cost.py [--calls 40] [--out profiles/r26_tile_map_cost.log]
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"720p": (1280, 720), "2160p": (3840, 2160)}
LAYOUTS = {"plain": (8, False), "normals": (11, True)}  # xstride of the accumulator, the normals channel
SPP = 16


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--layouts", nargs="+", default=list(LAYOUTS), choices=list(LAYOUTS))
    ap.add_argument("--tiles", nargs="+", type=int, default=[16, 32, 64])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r26_tile_map_cost.log"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    from phosphorus_mk2_amd import xpu
    lib = xpu.load_library()
    try:
        hip = C.CDLL("libamdhip64.so.7")  # the runtime the library runs on: the copy already in the process
    except OSError:
        hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p

    def ok(rc, what):
        if rc != 0:
            sys.exit(f"{what} failed: {rc}")  # nothing more is started on the GPU
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"library: {os.path.basename(xpu.LIB_PATH)}")
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=4))
    ev = [vp(), vp()]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)), "hipEventCreate")
    out = {"library": os.path.basename(xpu.LIB_PATH), "cases": {}}
    fmt = lambda m: f"{m['median']:.4f} ({m['min']:.4f} - {m['max']:.4f})"
    try:
        for layout, name in ((l, s) for l in a.layouts for s in a.sizes):
            XA, normals = LAYOUTS[layout]
            W, H = SIZES[name]
            npix = W * H
            rng = np.random.default_rng(1)
            _, mo, so, _ = xpu.film_layout(4, normals, True, True)
            acc = rng.uniform(0.1, 1.0, (npix, XA)).astype(np.float32)
            acc[:, mo:mo + 3] *= 0.01
            acc[:, so] = SPP
            frame = rng.uniform(0.1, 1.0, (npix, XA - 1)).astype(np.float32)
            film_bytes = acc.nbytes
            bytes_copy = film_bytes // 2
            max_records = -(-W // min(a.tiles)) * -(-H // min(a.tiles))
            pa, pb, pc, pd, pr = vp(), vp(), vp(), vp(), vp()
            for p, n in ((pa, acc.nbytes), (pb, frame.nbytes), (pc, bytes_copy), (pd, bytes_copy), (pr, max_records * 40)):
                ok(hip.hipMalloc(C.byref(p), C.c_size_t(n)), "hipMalloc")
            try:
                ok(hip.hipMemcpy(pb, frame.ctypes.data_as(vp), C.c_size_t(frame.nbytes), 1), "hipMemcpy")
                ok(hip.hipMemset(pc, 0, C.c_size_t(bytes_copy)), "hipMemset")
                for ts in a.tiles:
                    ok(hip.hipMemcpy(pa, acc.ctypes.data_as(vp), C.c_size_t(acc.nbytes), 1), "hipMemcpy")  # (the accumulate calls below pool into it)
                    ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
                    q = xpu.tile_map_settings((H, W, XA), ts, 0.05, 0.01, 4, normals)
                    q.on_device = 1
                    s = xpu.abi.TileMapSummary()
                    kernel, call, copy, pool = [], [], [], []
                    for k in range(a.warmup + a.calls):
                        ok(lib.phx_dev_film_tile_map(dev._h, C.byref(q), pa, pr, C.byref(s)), "phx_dev_film_tile_map")
                        t = dev.tile_map_times()
                        ok(hip.hipEventRecord(ev[0], None), "hipEventRecord")
                        ok(hip.hipMemcpyAsync(pd, pc, C.c_size_t(bytes_copy), 3, None), "hipMemcpyAsync")
                        ok(hip.hipEventRecord(ev[1], None), "hipEventRecord")
                        ok(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
                        ms = C.c_float(0.0)
                        ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
                        dev.accumulate((H, W, XA), (H, W, XA - 1), SPP, 4, normals, False, threshold=0.05, floor=0.01, device_ptrs=(pa.value, pb.value))
                        if k >= a.warmup:
                            kernel.append(t["kernel"]); call.append(t["call"]); copy.append(ms.value); pool.append(dev.accumulate_times()["kernel"])
                    tiles = -(-W // ts) * -(-H // ts)
                    assert s.pixels == npix and s.tiles == tiles and s.invalid == 0, (s.pixels, s.tiles, s.invalid)
                    rec = {"pixels": npix, "tiles": tiles, "bytes_used": 28 * npix, "bytes_lines": film_bytes, "bytes_copy_moved": 2 * bytes_copy}
                    for key, v in (("kernel_ms", kernel), ("call_ms", call), ("copy_ms", copy), ("accumulate_kernel_ms", pool)):
                        rec[key] = {"median": median(v), "min": min(v), "max": max(v)}
                    rec["kernel_GBps_lines"] = film_bytes / rec["kernel_ms"]["median"] / 1e6
                    rec["copy_GBps"] = 2 * bytes_copy / rec["copy_ms"]["median"] / 1e6
                    rec["kernel_over_copy"] = rec["kernel_ms"]["median"] / rec["copy_ms"]["median"]
                    rec["kernel_over_accumulate"] = rec["kernel_ms"]["median"] / rec["accumulate_kernel_ms"]["median"]
                    say(f"{layout} ({XA} floats) {name:>5} tiles of {ts:2d}: {npix} pixels, {tiles} tiles, {film_bytes / 1e6:.1f} MB of film ({28 * npix / 1e6:.1f} MB used)")
                    say(f"       kernel {fmt(rec['kernel_ms'])} ms = {rec['kernel_GBps_lines']:.0f} GB/s of whole lines;  call {fmt(rec['call_ms'])} ms")
                    say(f"       copy of {bytes_copy / 1e6:.1f} MB (the film's bytes moved) {fmt(rec['copy_ms'])} ms = {rec['copy_GBps']:.0f} GB/s;  kernel / copy = {rec['kernel_over_copy']:.2f}")
                    say(f"       k_accumulate on the same accumulator {fmt(rec['accumulate_kernel_ms'])} ms;  kernel / k_accumulate = {rec['kernel_over_accumulate']:.2f}")
                    out["cases"][f"{layout} {name} {ts}"] = rec
            finally:
                for p in (pa, pb, pc, pd, pr):
                    if p.value:
                        hip.hipFree(p)
    finally:
        dev.close()
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
