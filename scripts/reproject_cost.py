"""What reprojection costs (phx_dev_film_reproject): one call on device-resident films at 1280 x 720 and at 3840 x 2160, with the summary
(--no-summary: without).  The accumulator has 11 floats a pixel (primary rgba, normals, m2, samples), the guide films 8.  The inputs are
synthetic and cheap to make: a floor and a back wall traced in numpy under two cameras a small step apart (tests/reproject_cases.py), so
nearly every pixel takes the full path, four taps and a mix.

The kernel's time (phx_dev_reproject_times: HIP events around the one launch) is put against
  (a) the byte model: the kernel reads the old accumulator and both guide films and writes the new accumulator, 4 * (11 + 8 + 8) + 4 * 11 =
      152 bytes a pixel, were every byte read once (the four taps of neighbouring pixels overlap: what is read twice is meant to come from
      L1 / L2); and
  (b) a device-to-device copy (hipMemcpyAsync, HIP events around it) that moves the SAME number of bytes over the memory bus: 76 read, 76 written.
Calls alternate (reproject, copy, ...): --warmup of each, then --calls timed of each; medians and ranges.

    python scripts/reproject_cost.py [--calls 40] [--out profiles/r22_reproject_cost.log]
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"720p": (1280, 720), "2160p": (3840, 2160)}
XA, XG = 11, 8


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--no-summary", action="store_true", help="pass no summary: the kernel then skips the counters")
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r22_reproject_cost.log"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import numpy as np
    import reproject_cases as RC
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
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=16, paths_per_sample=1, path_depth=4))
    ev = [vp(), vp()]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)), "hipEventCreate")
    out = {"summary": "off" if a.no_summary else "on", "sizes": {}}
    try:
        for name in a.sizes:
            W, H = SIZES[name]
            npix = W * H
            cam_a, cam_b = RC.camera(W, H), RC.camera(W, H, origin=(0.06, 0.02, 0.03), m3=RC.rot_y(0.004))
            world = [RC.FLOOR, RC.OPEN_WALL[0]]
            (gf, normals), (gt, _) = RC.trace(world, cam_a), RC.trace(world, cam_b)
            acc = np.random.default_rng(1).uniform(0.1, 1.0, (H, W, XA)).astype(np.float32)
            acc[..., 4:7], acc[..., 10] = normals, 16.0
            bytes_kernel = npix * (4 * (XA + 2 * XG) + 4 * XA)
            bytes_copy = bytes_kernel // 2
            ptrs = [vp() for _ in range(6)]  # acc_from, guides_from, guides_to, acc_to, copy source, copy destination
            for p, n in zip(ptrs, (acc.nbytes, gf.nbytes, gt.nbytes, acc.nbytes, bytes_copy, bytes_copy)):
                ok(hip.hipMalloc(C.byref(p), C.c_size_t(n)), "hipMalloc")
            try:
                for p, x in zip(ptrs, (acc, gf, gt)):
                    ok(hip.hipMemcpy(p, x.ctypes.data_as(vp), C.c_size_t(x.nbytes), 1), "hipMemcpy")
                ok(hip.hipMemset(ptrs[4], 0, C.c_size_t(bytes_copy)), "hipMemset")
                ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
                kernel, call, copy = [], [], []
                for k in range(a.warmup + a.calls):
                    _, s = dev.reproject(acc.shape, gf.shape, gt.shape, cam_a, cam_b, summary=not a.no_summary, device_ptrs=[p.value for p in ptrs[:4]])
                    t = dev.reproject_times()
                    ok(hip.hipEventRecord(ev[0], None), "hipEventRecord")
                    ok(hip.hipMemcpyAsync(ptrs[5], ptrs[4], C.c_size_t(bytes_copy), 3, None), "hipMemcpyAsync")
                    ok(hip.hipEventRecord(ev[1], None), "hipEventRecord")
                    ok(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
                    ms = C.c_float(0.0)
                    ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
                    if k >= a.warmup:
                        kernel.append(t["kernel"]); call.append(t["call"]); copy.append(ms.value)
                rec = {"pixels": npix, "bytes_kernel": bytes_kernel, "bytes_copy_moved": 2 * bytes_copy, "summary": s}
                for key, v in (("kernel_ms", kernel), ("call_ms", call), ("copy_ms", copy)):
                    rec[key] = {"median": median(v), "min": min(v), "max": max(v)}
                rec["kernel_GBps"] = bytes_kernel / rec["kernel_ms"]["median"] / 1e6
                rec["copy_GBps"] = 2 * bytes_copy / rec["copy_ms"]["median"] / 1e6
                rec["kernel_over_copy"] = rec["kernel_ms"]["median"] / rec["copy_ms"]["median"]
                fmt = lambda m: f"{m['median']:.4f} ({m['min']:.4f} - {m['max']:.4f})"
                say(f"{name:>5}: {npix} pixels, {bytes_kernel / 1e6:.1f} MB by the byte model ({bytes_kernel // npix} B a pixel); summary {s}")
                say(f"       kernel {fmt(rec['kernel_ms'])} ms = {rec['kernel_GBps']:.0f} GB/s of the byte model;  call {fmt(rec['call_ms'])} ms")
                say(f"       copy of {bytes_copy / 1e6:.1f} MB (the same bytes moved) {fmt(rec['copy_ms'])} ms = {rec['copy_GBps']:.0f} GB/s;  kernel / copy = {rec['kernel_over_copy']:.2f}")
                out["sizes"][name] = rec
            finally:
                for p in ptrs:
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
