"""What the outlier clamp costs (phx_dev_film_outlier_clamp): one call on device-resident films at 1280 x 720 and at 3840 x 2160, radius 1
to 3, with the summary, in its two uses:
  despeckle   a frame film of 7 floats a pixel (primary rgba, m2) against itself, in place, the centre excluded and upper only, trim 2.  The
              call copies the film first (film_out is ref): the copy is in the call's time, not in the kernel's
  history     an accumulator of 11 floats a pixel (primary rgba, normals, m2, samples) in place against a frame film of 10, two-sided, the
              centre included, trim 0, clamped_history 8
The films are synthetic and cheap to make: log-normal colours with one pixel in 4096 a spike, so that, as on a real film, few pixels are
clamped and the kernel writes little.

The kernel's time (phx_dev_outlier_clamp_times: HIP events around the one launch) is put against
  (a) the byte model: every float of ref once (the halo's share of a tile, (16 + 2 r)^2 / 256, is meant to come from L2) and, where film is
      not ref, every float of film once (a pixel's floats share cache lines with its neighbours'); what is written is left out; and
  (b) a device-to-device copy (hipMemcpyAsync, HIP events around it) that moves the SAME number of bytes over the memory bus: half read,
      half written.
Calls alternate (clamp, copy, ...): --warmup of each, then --calls timed of each; medians and ranges.

    python scripts/outlier_clamp_cost.py [--calls 40] [--out profiles/r23_outlier_clamp_cost.log]
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"720p": (1280, 720), "2160p": (3840, 2160)}


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r23_outlier_clamp_cost.log"))
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

    def film_of(rng, W, H, x, samples_at=0):
        f = np.exp(rng.normal(0.0, 0.5, (H, W, x))).astype(np.float32)
        f[..., :3] *= np.where(rng.random((H, W, 1)) < 1 / 4096, 1000.0, 1.0).astype(np.float32)
        if samples_at:
            f[..., samples_at] = 64.0
        return f
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=16, paths_per_sample=1, path_depth=4))
    ev = [vp(), vp()]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)), "hipEventCreate")
    out = {"sizes": {}}
    try:
        for name in a.sizes:
            W, H = SIZES[name]
            npix = W * H
            rng = np.random.default_rng(1)
            frame7, acc11, frame10 = film_of(rng, W, H, 7), film_of(rng, W, H, 11, 10), film_of(rng, W, H, 10)
            uses = {"despeckle": dict(film=frame7, ref=None, bytes=npix * 4 * 7,
                                      kw=dict(gamma=4.0, trim=2, min_taps=4, exclude_centre=True, upper_only=True, m2_offset=4, samples_offset=0)),
                    "history": dict(film=acc11, ref=frame10, bytes=npix * 4 * (11 + 10),
                                    kw=dict(gamma=4.0, trim=0, min_taps=4, exclude_centre=False, upper_only=False, clamped_history=8, m2_offset=7, samples_offset=10))}
            out["sizes"][name] = {}
            for use, u in uses.items():
                bytes_kernel = u["bytes"]
                bytes_copy = bytes_kernel // 2
                hosts = [u["film"]] + ([u["ref"]] if u["ref"] is not None else [])
                ptrs = [vp() for _ in range(len(hosts) + 2)]  # film [, ref], copy source, copy destination
                for p, n in zip(ptrs, [h.nbytes for h in hosts] + [bytes_copy, bytes_copy]):
                    ok(hip.hipMalloc(C.byref(p), C.c_size_t(n)), "hipMalloc")
                try:
                    ok(hip.hipMemset(ptrs[-2], 0, C.c_size_t(bytes_copy)), "hipMemset")
                    film_ptr = ptrs[0].value
                    ref_ptr = ptrs[1].value if u["ref"] is not None else film_ptr
                    shape_b = u["ref"].shape if u["ref"] is not None else u["film"].shape
                    for radius in (1, 2, 3):
                        kernel, call, copy = [], [], []
                        for k in range(a.warmup + a.calls):
                            for p, h in zip(ptrs, hosts):   # the call is in place: every call starts from the same films
                                ok(hip.hipMemcpy(p, h.ctypes.data_as(vp), C.c_size_t(h.nbytes), 1), "hipMemcpy")
                            ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
                            _, s = dev.clamp_outliers(u["film"].shape, shape_b, radius, device_ptrs=[film_ptr, ref_ptr, film_ptr], **u["kw"])
                            t = dev.outlier_clamp_times()
                            ok(hip.hipEventRecord(ev[0], None), "hipEventRecord")
                            ok(hip.hipMemcpyAsync(ptrs[-1], ptrs[-2], C.c_size_t(bytes_copy), 3, None), "hipMemcpyAsync")
                            ok(hip.hipEventRecord(ev[1], None), "hipEventRecord")
                            ok(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
                            ms = C.c_float(0.0)
                            ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
                            if k >= a.warmup:
                                kernel.append(t["kernel"]); call.append(t["call"]); copy.append(ms.value)
                        rec = {"pixels": npix, "radius": radius, "bytes_kernel": bytes_kernel, "bytes_copy_moved": 2 * bytes_copy, "summary": s}
                        for key, v in (("kernel_ms", kernel), ("call_ms", call), ("copy_ms", copy)):
                            rec[key] = {"median": median(v), "min": min(v), "max": max(v)}
                        rec["kernel_GBps"] = bytes_kernel / rec["kernel_ms"]["median"] / 1e6
                        rec["copy_GBps"] = 2 * bytes_copy / rec["copy_ms"]["median"] / 1e6
                        rec["kernel_over_copy"] = rec["kernel_ms"]["median"] / rec["copy_ms"]["median"]
                        fmt = lambda m: f"{m['median']:.4f} ({m['min']:.4f} - {m['max']:.4f})"
                        say(f"{name:>5} {use:>9} radius {radius}: {bytes_kernel / 1e6:.1f} MB by the byte model ({bytes_kernel // npix} B a pixel); clamped {s['clamped']} of {s['pixels']}")
                        say(f"       kernel {fmt(rec['kernel_ms'])} ms = {rec['kernel_GBps']:.0f} GB/s of the byte model;  call {fmt(rec['call_ms'])} ms;  "
                            f"copy of the same bytes {fmt(rec['copy_ms'])} ms = {rec['copy_GBps']:.0f} GB/s;  kernel / copy = {rec['kernel_over_copy']:.2f}")
                        out["sizes"][name][f"{use} r{radius}"] = rec
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
