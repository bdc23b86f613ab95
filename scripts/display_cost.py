"""What the display pass costs (phx_dev_film_display): one call on device-resident films at 1280 x 720 and at 3840 x 2160, in the 7-float
layout (primary rgba, m2: what render() gives with moments=True) and the 8-float one (an accumulator's: the stride at which a wave's lanes lie
32 bytes apart), with the exposure taken from the film (histogram + exposure + encode) into a device-resident image.

The two stages' times (phx_dev_display_times: HIP events around histogram + exposure and around the encode) are put against
  (a) the byte model: the histogram reads the film, 4 * xstride bytes a pixel; the encode reads it again and writes 4 bytes a pixel; and
  (b) device-to-device copies (hipMemcpyAsync, HIP events around them) that move the SAME number of bytes over the memory bus: a copy of B bytes
      reads B and writes B, so B = 2 * xstride bytes a pixel for the histogram and 2 * xstride + 2 for the encode.
Calls alternate (display, the two copies, display, ...): --warmup of each, then --calls timed of each; medians and ranges.

Then the figure the pass exists for, at 2160p: the whole call with the film in device memory and the image on the host (on_device = 2: 4 bytes a
pixel come back) against reading the film itself back (hipMemcpy to host memory, 4 * xstride bytes a pixel), both on the host's clock.

    python scripts/display_cost.py [--calls 40] [--out profiles/r21_display_cost.log]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"720p": (1280, 720), "2160p": (3840, 2160)}
LAYOUTS = (7, 8)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r21_display_cost.log"))
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
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=1))
    ev = [vp(), vp(), vp()]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)), "hipEventCreate")
    out = {"sizes": {}}
    fmt = lambda m: f"{m['median']:.4f} ({m['min']:.4f} - {m['max']:.4f})"
    stat = lambda v: {"median": median(v), "min": min(v), "max": max(v)}
    try:
        for xs, name in ((x, s) for x in LAYOUTS for s in a.sizes):
            W, H = SIZES[name]
            npix = W * H
            rng = np.random.default_rng(1)
            film = np.zeros((npix, xs), np.float32)
            film[:, :3] = np.exp2(rng.uniform(-8.0, 4.0, (npix, 3))).astype(np.float32)  # a lit film over twelve stops
            bytes_h, bytes_e = npix * 4 * xs, npix * (4 * xs + 4)
            pf, pi, pc, pd = vp(), vp(), vp(), vp()
            for p, n in ((pf, film.nbytes), (pi, npix * 4), (pc, bytes_e // 2), (pd, bytes_e // 2)):
                ok(hip.hipMalloc(C.byref(p), C.c_size_t(n)), "hipMalloc")
            try:
                ok(hip.hipMemcpy(pf, film.ctypes.data_as(vp), C.c_size_t(film.nbytes), 1), "hipMemcpy")
                ok(hip.hipMemset(pc, 0, C.c_size_t(bytes_e // 2)), "hipMemset")
                ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
                hist, enc, call, copy_h, copy_e = [], [], [], [], []
                for k in range(a.warmup + a.calls):
                    _, s = dev.display((H, W, xs), "auto", "aces", summary=True, device_ptr=pf.value, image_on_host=False, image_ptr=pi.value)
                    t = dev.display_times()
                    ok(hip.hipEventRecord(ev[0], None), "hipEventRecord")
                    ok(hip.hipMemcpyAsync(pd, pc, C.c_size_t(bytes_h // 2), 3, None), "hipMemcpyAsync")
                    ok(hip.hipEventRecord(ev[1], None), "hipEventRecord")
                    ok(hip.hipMemcpyAsync(pd, pc, C.c_size_t(bytes_e // 2), 3, None), "hipMemcpyAsync")
                    ok(hip.hipEventRecord(ev[2], None), "hipEventRecord")
                    ok(hip.hipEventSynchronize(ev[2]), "hipEventSynchronize")
                    m0, m1 = C.c_float(0.0), C.c_float(0.0)
                    ok(hip.hipEventElapsedTime(C.byref(m0), ev[0], ev[1]), "hipEventElapsedTime")
                    ok(hip.hipEventElapsedTime(C.byref(m1), ev[1], ev[2]), "hipEventElapsedTime")
                    if k >= a.warmup:
                        hist.append(t["histogram"]); enc.append(t["encode"]); call.append(t["call"]); copy_h.append(m0.value); copy_e.append(m1.value)
                assert s["pixels"] == npix and s["invalid"] == 0 and s["counted"] == npix and s["from_histogram"] == 1, s
                rec = {"pixels": npix, "xstride": xs, "scale": s["scale"], "bytes_histogram": bytes_h, "bytes_encode": bytes_e,
                       "histogram_ms": stat(hist), "encode_ms": stat(enc), "call_ms": stat(call), "copy_histogram_ms": stat(copy_h), "copy_encode_ms": stat(copy_e)}
                rec["histogram_over_copy"] = rec["histogram_ms"]["median"] / rec["copy_histogram_ms"]["median"]
                rec["encode_over_copy"] = rec["encode_ms"]["median"] / rec["copy_encode_ms"]["median"]
                say(f"xstride {xs} {name:>5}: {npix} pixels; the histogram reads {bytes_h / 1e6:.1f} MB, the encode moves {bytes_e / 1e6:.1f} MB ({4 * xs + 4} B a pixel)")
                say(f"       histogram + exposure {fmt(rec['histogram_ms'])} ms = {bytes_h / rec['histogram_ms']['median'] / 1e6:.0f} GB/s;  "
                    f"copy of the same bytes {fmt(rec['copy_histogram_ms'])} ms;  ratio {rec['histogram_over_copy']:.2f}")
                say(f"       encode               {fmt(rec['encode_ms'])} ms = {bytes_e / rec['encode_ms']['median'] / 1e6:.0f} GB/s;  "
                    f"copy of the same bytes {fmt(rec['copy_encode_ms'])} ms;  ratio {rec['encode_over_copy']:.2f}")
                say(f"       call (device-resident image) {fmt(rec['call_ms'])} ms")
                if name == "2160p":  # the preview against the read-back it replaces
                    host = np.empty_like(film)
                    preview, back = [], []
                    for k in range(a.warmup + a.calls):
                        dev.display((H, W, xs), "auto", "aces", device_ptr=pf.value)
                        t = dev.display_times()["call"]
                        t0 = time.perf_counter()
                        ok(hip.hipMemcpy(host.ctypes.data_as(vp), pf, C.c_size_t(film.nbytes), 2), "hipMemcpy")
                        t1 = time.perf_counter()
                        if k >= a.warmup:
                            preview.append(t); back.append(1e3 * (t1 - t0))
                    rec["preview_call_ms"], rec["film_readback_ms"] = stat(preview), stat(back)
                    say(f"       preview (on_device = 2: the image, {npix * 4 / 1e6:.1f} MB, to the host) call {fmt(rec['preview_call_ms'])} ms;  "
                        f"reading the film back ({film.nbytes / 1e6:.1f} MB) {fmt(rec['film_readback_ms'])} ms")
                out["sizes"][f"xstride {xs} {name}"] = rec
            finally:
                for p in (pf, pi, pc, pd):
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
