"""What film accumulation costs (phx_dev_film_accumulate): one call on device-resident films at 1280 x 720 and at 3840 x 2160, with the
summary (--no-summary: without), in two layouts: "normals", an accumulator of 11 floats a pixel (primary rgba, normals, m2, samples) and a uniform
frame film of 10; and "plain", without the normals, 8 and 7 floats: what render_progressive and the C example pool by default, and the stride (8) at
which a thread's reads of its own pixel meet 8-way LDS bank conflicts.

The kernel's time (phx_dev_accumulate_times: HIP events around the one launch) is put against
  (a) the byte model: the kernel reads both films and writes the accumulator, 4 * (xstride_a + xstride_b) + 4 * xstride_a = 128 / 92 bytes a
      pixel, nothing twice; and
  (b) a device-to-device copy (hipMemcpyAsync, HIP events around it) that moves the SAME number of bytes over the memory bus: a copy of B bytes
      reads B and writes B, so B = 64 / 46 bytes a pixel.
Calls alternate (accumulate, copy, accumulate, ...): --warmup of each, then --calls timed of each; medians and ranges.  The films are far larger
than the last-level cache at 2160p (700 / 500 MB) and are not at 720p (81 / 55 MB), which the copy shares with the kernel.

    python scripts/accumulate_cost.py [--calls 40] [--out profiles/r20_accumulate_cost.log]
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"720p": (1280, 720), "2160p": (3840, 2160)}
LAYOUTS = {"normals": (11, 10, True), "plain": (8, 7, False)}  # xstride of the accumulator, of the frame film, the normals channel
SPP = 16


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--no-summary", action="store_true", help="pass no summary: the kernel then skips the counters and their arithmetic")
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--layouts", nargs="+", default=list(LAYOUTS), choices=list(LAYOUTS))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r20_accumulate_cost.log"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
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
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=4))
    ev = [vp(), vp()]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)), "hipEventCreate")
    out = {"summary": "off" if a.no_summary else "on", "sizes": {}}
    try:
        for layout, name in ((l, s) for l in a.layouts for s in a.sizes):
            XA, XB, normals = LAYOUTS[layout]
            W, H = SIZES[name]
            npix = W * H
            rng = np.random.default_rng(1)
            frame = rng.uniform(0.1, 1.0, (npix, XB)).astype(np.float32)
            acc = np.zeros((npix, XA), np.float32)
            bytes_kernel = npix * (4 * (XA + XB) + 4 * XA)
            bytes_copy = bytes_kernel // 2
            pa, pb, pc, pd = vp(), vp(), vp(), vp()
            for p, n in ((pa, acc.nbytes), (pb, frame.nbytes), (pc, bytes_copy), (pd, bytes_copy)):
                ok(hip.hipMalloc(C.byref(p), C.c_size_t(n)), "hipMalloc")
            try:
                ok(hip.hipMemcpy(pa, acc.ctypes.data_as(vp), C.c_size_t(acc.nbytes), 1), "hipMemcpy")
                ok(hip.hipMemcpy(pb, frame.ctypes.data_as(vp), C.c_size_t(frame.nbytes), 1), "hipMemcpy")
                ok(hip.hipMemset(pc, 0, C.c_size_t(bytes_copy)), "hipMemset")
                ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
                kernel, call, copy = [], [], []
                for k in range(a.warmup + a.calls):
                    _, s = dev.accumulate((H, W, XA), (H, W, XB), SPP, 4, normals, False, threshold=None if a.no_summary else 0.05, floor=0.01, device_ptrs=(pa.value, pb.value))
                    t = dev.accumulate_times()
                    ok(hip.hipEventRecord(ev[0], None), "hipEventRecord")
                    ok(hip.hipMemcpyAsync(pd, pc, C.c_size_t(bytes_copy), 3, None), "hipMemcpyAsync")
                    ok(hip.hipEventRecord(ev[1], None), "hipEventRecord")
                    ok(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
                    ms = C.c_float(0.0)
                    ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
                    if k >= a.warmup:
                        kernel.append(t["kernel"]); call.append(t["call"]); copy.append(ms.value)
                assert a.no_summary or s["pixels"] == npix and s["invalid"] == 0 and s["samples"] == npix * SPP * (a.warmup + a.calls), s
                rec = {"pixels": npix, "bytes_kernel": bytes_kernel, "bytes_copy_moved": 2 * bytes_copy}
                for key, v in (("kernel_ms", kernel), ("call_ms", call), ("copy_ms", copy)):
                    rec[key] = {"median": median(v), "min": min(v), "max": max(v)}
                rec["kernel_GBps"] = bytes_kernel / rec["kernel_ms"]["median"] / 1e6
                rec["copy_GBps"] = 2 * bytes_copy / rec["copy_ms"]["median"] / 1e6
                rec["kernel_over_copy"] = rec["kernel_ms"]["median"] / rec["copy_ms"]["median"]
                fmt = lambda m: f"{m['median']:.4f} ({m['min']:.4f} - {m['max']:.4f})"
                say(f"{layout} ({XA} + {XB} floats) {name:>5}: {npix} pixels, {bytes_kernel / 1e6:.1f} MB over the bus ({bytes_kernel // npix} B a pixel)")
                say(f"       kernel {fmt(rec['kernel_ms'])} ms = {rec['kernel_GBps']:.0f} GB/s;  call {fmt(rec['call_ms'])} ms")
                say(f"       copy of {bytes_copy / 1e6:.1f} MB (the same bytes moved) {fmt(rec['copy_ms'])} ms = {rec['copy_GBps']:.0f} GB/s;  kernel / copy = {rec['kernel_over_copy']:.2f}")
                out["sizes"][f"{layout} {name}"] = rec
            finally:
                for p in (pa, pb, pc, pd):
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
