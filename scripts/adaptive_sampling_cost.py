"""What the round structure of adaptive sampling costs by itself: the bench frame -- BASELINE configs[1] (Soup 100 k, 1280 x 720, 256 spp,
depth 9) on one GPU into a device-resident film with moments=True -- with the setting

    off      one pass of 256 samples per batch
    on       min_samples = 64, step = 64 and a threshold so small (--threshold, 1e-30) that no lit pixel stops: four rounds of 64 samples,
             a selection and a host synchronisation behind each of the first three, batches sized for 64 samples a pixel

each in a process of its own, --rounds times, interleaved (off, on, off, ...), so that drift of the machine lands on both alike.  A pixel
whose first 64 samples are all equal (a black one: every camera ray missed; one that looks straight at the emitter) stops whatever the threshold, so before any time is printed the
script asserts, on the frame of seed 1: `primary` of every pixel that took all its samples is the `off` frame's, bit for bit; camera_samples
is the sum of the channel "samples"; and the four ray counts are the `off` frame's when no pixel stopped -- when some did, every sample not
taken is at least one closest-hit ray less, and no count is above the `off` frame's.  Prints phx_stats' frame_ms of every run, each mode's
best, median and range, and one JSON line.

    python scripts/adaptive_sampling_cost.py [--rounds 3] [--frames 3] [--out profiles/r16_adaptive_sampling_cost.log]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("frame_ms", "pass_ms", "shade_kernel_ms", "trace_ms")
COUNTS = ("camera_samples", "rays_closest", "rays_shadow", "rays_masked")


def one(a):
    """a child process: one device, one warm-up frame (seed 1, whose film is saved), a.frames timed ones; prints one JSON line"""
    sys.path.insert(0, HERE)
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    hip = C.CDLL("libamdhip64.so.7")  # the runtime the library runs on
    on = a.one == "on"
    sc = scenes.soup(a.triangles, width=a.width, height=a.height)
    W, H, xs = a.width, a.height, 7 + (1 if on else 0)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.spp, paths_per_sample=1, path_depth=9))
    ptr = C.c_void_p()
    try:
        if on:
            dev.set_adaptive(a.threshold, 0.0, a.min_samples, a.step)
        dev.preprocess(sc)
        assert hip.hipMalloc(C.byref(ptr), C.c_size_t(W * H * xs * 4)) == 0
        best, first = None, None
        for k in range(a.frames + 1):
            dev.start(sc, xpu.FrameState(1 + k, xpu.Tiles.make(W, H, 32), None, device_film_ptr=ptr.value, moments=True, adaptive=on))
            dev.join()
            st = dev.stats()
            st["pass_ms"] = st["shade_ms"] - st["shade_kernel_ms"]
            if k == 0:
                film = np.empty((H, W, xs), np.float32)
                assert hip.hipMemcpy(film.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(film.nbytes), 2) == 0
                np.save(a.film, film)
                first = {key: st[key] for key in COUNTS}
            if k and (best is None or st["frame_ms"] < best["frame_ms"]):
                best = st
        print(json.dumps({"mode": a.one, **{key: best[key] for key in KEYS}, "device_bytes": best["device_bytes"], "paths_in_flight": best["paths_in_flight"],
                          "tiles": best["tiles"], "trace_launches": best["trace_launches"], **first}))
    finally:
        dev.close()
        if ptr.value:
            hip.hipFree(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--min-samples", type=int, default=64)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=1e-30)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r16_adaptive_sampling_cost.log"))
    ap.add_argument("--one", choices=["off", "on"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--film", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    import numpy as np
    modes = ["off", "on"]
    runs = {m: [] for m in modes}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            for m in modes:
                env = {k: v for k, v in os.environ.items() if k != "PHX_LIB"}
                film = os.path.join(tmp, f"{m}{r}.npy")
                cmd = [sys.executable, os.path.abspath(__file__), "--one", m, "--film", film, "--triangles", str(a.triangles), "--width", str(a.width), "--height", str(a.height),
                       "--spp", str(a.spp), "--frames", str(a.frames), "--min-samples", str(a.min_samples), "--step", str(a.step), "--threshold", repr(a.threshold)]
                p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
                if p.returncode:
                    sys.exit(f"{m}, round {r}: exit status {p.returncode}\n{p.stdout}\n{p.stderr}")  # nothing more is started on the GPU
                row = json.loads(p.stdout.strip().splitlines()[-1])
                row["film"] = film
                runs[m].append(row)
                say(f"round {r} {m:>3}: frame {row['frame_ms']:8.2f} ms  begin-pass + film + selection {row['pass_ms']:7.3f} ms  k_shade {row['shade_kernel_ms']:7.2f} ms  trace {row['trace_ms']:7.2f} ms  "
                    f"{row['paths_in_flight']:10d} paths in flight  {row['tiles']} tiles, {row['trace_launches']} k_trace launches  {row['device_bytes']:12d} B")
        # before any comparison: what the rule promises of the pixels that never stop
        off, on = np.load(runs["off"][0]["film"]), np.load(runs["on"][0]["film"])
        for m in modes:
            for row in runs[m][1:]:
                assert np.array_equal(np.load(row["film"]).view(np.uint32), (off if m == "off" else on).view(np.uint32)), f"{m}: two runs rendered different films"
                assert all(row[k] == runs[m][0][k] for k in COUNTS)
    n = on[..., 7]
    never = n == a.spp
    stopped = int((~never).sum())
    skipped = int((a.spp - n.astype(np.float64)).sum())
    o, w = runs["off"][0], runs["on"][0]
    assert np.array_equal(on[never][:, :4].view(np.uint32), off[never][:, :4].view(np.uint32)), "primary of a pixel that never stopped differs"
    assert w["camera_samples"] == int(n.astype(np.float64).sum()) == o["camera_samples"] - skipped
    lit_stopped = int(((~never) & (off[..., :3] != 0).any(-1)).sum())
    # (a lit pixel can stop under any threshold only if its first min_samples samples are equal to the bit, m2 = +0.0: one that looks straight at the emitter)
    assert (on[~never][:, 4:7].view(np.uint32) == 0).all(), "a pixel with m2 > 0 stopped: the threshold is not small enough"
    if stopped == 0:
        assert all(w[k] == o[k] for k in COUNTS)
    else:
        assert o["rays_closest"] - w["rays_closest"] >= skipped and all(w[k] <= o[k] for k in COUNTS)
    say(f"{int(never.sum())} of {never.size} pixels took all {a.spp} samples and hold the off frame's primary bit for bit; {stopped} pixels whose first {a.min_samples} samples are "
        f"all equal (m2 = +0.0) stopped, {lit_stopped} of them lit, {skipped} samples not taken; ray counts off {[o[k] for k in COUNTS]} on {[w[k] for k in COUNTS]}")
    for m in modes:
        for row in runs[m]:
            del row["film"]
    out = {"scene": f"soup({a.triangles}) {a.width}x{a.height} {a.spp} spp depth 9, device-resident film, moments on; adaptive min_samples {a.min_samples} step {a.step} threshold {a.threshold}",
           "pixels_never_stopped": int(never.sum()), "pixels_stopped": stopped, "samples_not_taken": skipped, "runs": runs}
    for key in KEYS:
        for m in modes:
            v = [row[key] for row in runs[m]]
            out[f"{m}_{key}"] = {"best": min(v), "median": sorted(v)[len(v) // 2], "range": max(v) - min(v)}
        say(f"{key:>16}: " + "  ".join(f"{m} best {out[f'{m}_{key}']['best']:.3f} median {out[f'{m}_{key}']['median']:.3f} range {out[f'{m}_{key}']['range']:.3f}" for m in modes))
    out["on_vs_off"] = {}
    for key in KEYS:
        d = out[f"on_{key}"]["median"] - out[f"off_{key}"]["median"]
        rng = out[f"off_{key}"]["range"]
        out["on_vs_off"][key] = {"median_difference_ms": d, "percent": 100.0 * d / out[f"off_{key}"]["median"], "off_range_ms": rng, "within_range": bool(abs(d) <= rng)}
        say(f"rounds on against off, {key}: {d:+.3f} ms ({100.0 * d / out[f'off_{key}']['median']:+.2f} %) between the medians; off's own range is {rng:.3f} ms: "
            f"{'within' if abs(d) <= rng else 'OUTSIDE'} it")
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
