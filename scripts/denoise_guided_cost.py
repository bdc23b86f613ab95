"""What the first-hit guides and the guided filter cost (phx_dev_render_guides, phx_dev_denoise_guided): the bench scene -- Soup 100 k,
256 spp, depth 9 -- rendered on one GPU into a device-resident film with normals and moments (10 floats a pixel) at 1280 x 720 and at 3840 x 2160.

Per size a process of its own, --rounds times, interleaved (720p, 2160p, 720p, ...).  A process renders the frame twice and keeps the second one's
primary_ms (the packet walk of its camera rays: spp samples a pixel) and frame_ms; renders the guide film into device memory at each G of --guides,
--warmup times and then --calls timed times (phx_dev_guides_times: the kernel by HIP events, the call on the host's clock with the tables' upload in
it); then denoises the film with 5 iterations unguided, demodulated, and demodulated with the plane test, each --calls times after --warmup
(phx_dev_denoise_times).  A process reports medians over its calls, the script the median and the range over the processes.

The guide kernel is put against the frame's own camera-ray walk per sample: multiple = (kernel ms / G) / (primary_ms / spp).
Bytes of state a pixel and iteration, compulsory (denoise_cost.py keeps the unguided model): 96 unguided and demodulated, 112 with the plane test
(x: 16 more read); gathered per tap 48, and 16 more with the plane test (x of q).

    python scripts/denoise_guided_cost.py [--rounds 3] [--calls 5] [--out profiles/r19_denoise_guided_cost.log]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"720p": (1280, 720), "2160p": (3840, 2160)}
STATE_BYTES = {"unguided": 96, "demodulate": 96, "demodulate+plane": 112}
GATHER_BYTES = {"unguided": 25 * 48 + 9 * 24, "demodulate": 25 * 48 + 9 * 24, "demodulate+plane": 25 * 64 + 9 * 24}


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def one(a):
    """a child process: the frame, the guide passes, the three filters; prints one JSON line"""
    sys.path.insert(0, HERE)
    from phosphorus_mk2_amd import abi, scenes, xpu
    xpu.load_library()
    hip = C.CDLL("libamdhip64.so.7")  # the runtime the library runs on
    W, H = SIZES[a.one]
    xs = 10
    sc = scenes.soup(a.triangles, width=W, height=H)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.spp, paths_per_sample=1, path_depth=9))
    src, dst, gbuf = C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        dev.preprocess(sc)
        nbytes = W * H * xs * 4
        for p, n in ((src, nbytes), (dst, nbytes), (gbuf, W * H * 8 * 4)):
            assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
        for k in range(2):
            dev.start(sc, xpu.FrameState(1, xpu.Tiles.make(W, H, 32), None, device_film_ptr=src.value, primary_components=4, normals=True, moments=True))
            dev.join()
        st = dev.stats()
        row = {"size": a.one, "pixels": W * H, "frame_ms": st["frame_ms"], "primary_ms": st["primary_ms"], "primary_ms_per_sample": st["primary_ms"] / a.spp, "guides": {},
               "denoise": {}}
        for G in a.guides:
            t = []
            for k in range(a.warmup + a.calls):
                dev.render_guides(1, G, device_ptr=gbuf.value)
                if k >= a.warmup:
                    t.append(dev.guides_times())
            kern, call = median([x["kernel"] for x in t]), median([x["call"] for x in t])
            row["guides"][str(G)] = {"kernel": kern, "call": call, "kernel_per_sample": kern / G, "multiple_of_primary": (kern / G) / row["primary_ms_per_sample"]}
        dev.render_guides(1, 4, device_ptr=gbuf.value)  # the guides the filters below read
        q = xpu.denoise_settings((H, W, xs), a.spp, 4, True, False, iterations=a.iterations)
        q.on_device = 1
        for name, flags in (("unguided", 0), ("demodulate", 1), ("demodulate+plane", 3)):
            g = abi.DenoiseGuides(guides=gbuf.value, xstride=8, flags=flags, albedo_floor=0.01, sigma_x=1.0, plane_scale=xpu.guide_plane_scale(sc.camera))
            t = []
            for k in range(a.warmup + a.calls):
                rc = dev._lib.phx_dev_denoise_guided(dev._h, C.byref(q), C.byref(g), src.value, dst.value)
                assert rc == 0, dev._lib.phx_last_error()
                if k >= a.warmup:
                    t.append(dev.denoise_times())
            its = [median([x["iterations"][i] for x in t]) for i in range(a.iterations)]
            row["denoise"][name] = {"pack": median([x["pack"] for x in t]), "unpack": median([x["unpack"] for x in t]), "iterations": its,
                                    "kernels": median([x["pack"] + x["unpack"] + sum(x["iterations"]) for x in t]), "call": median([x["call"] for x in t])}
        print(json.dumps(row))
    finally:
        dev.close()
        for p in (src, dst, gbuf):
            if p.value:
                hip.hipFree(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--guides", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r19_denoise_guided_cost.log"))
    ap.add_argument("--one", choices=list(SIZES), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    runs = {s: [] for s in a.sizes}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for r in range(a.rounds):
        for s in a.sizes:
            env = {k: v for k, v in os.environ.items() if k != "PHX_LIB"}
            cmd = [sys.executable, os.path.abspath(__file__), "--one", s, "--triangles", str(a.triangles), "--spp", str(a.spp), "--iterations", str(a.iterations),
                   "--warmup", str(a.warmup), "--calls", str(a.calls), "--guides"] + [str(g) for g in a.guides]
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=400)
            if p.returncode:
                sys.exit(f"{s}, round {r}: exit status {p.returncode}\n{p.stdout}\n{p.stderr}")  # nothing more is started on the GPU
            row = json.loads(p.stdout.strip().splitlines()[-1])
            runs[s].append(row)
            say(f"round {r} {s:>5}: frame {row['frame_ms']:8.2f} ms, primary {row['primary_ms']:.3f} ms = {row['primary_ms_per_sample']:.4f} a sample;  guides " +
                ", ".join(f"G={G}: kernel {v['kernel']:.3f} call {v['call']:.3f} (x {v['multiple_of_primary']:.2f})" for G, v in row["guides"].items()) + ";  denoise " +
                ", ".join(f"{n}: call {v['call']:.3f} kernels {v['kernels']:.3f}" for n, v in row["denoise"].items()))
    out = {"scene": f"soup({a.triangles}) {a.spp} spp depth 9, device-resident film of 10 floats a pixel, {a.iterations} iterations", "runs": runs, "sizes": {}}

    def mmm(v):
        return {"median": median(v), "min": min(v), "max": max(v)}
    fmt = lambda m: f"{m['median']:.3f} ({m['min']:.3f} - {m['max']:.3f})"
    for s in a.sizes:
        rec = {"frame_ms": mmm([r["frame_ms"] for r in runs[s]]), "primary_ms_per_sample": mmm([r["primary_ms_per_sample"] for r in runs[s]]), "guides": {}, "denoise": {}}
        say(f"{s}: frame {fmt(rec['frame_ms'])} ms;  camera-ray walk {rec['primary_ms_per_sample']['median']:.4f} ms a sample")
        for G in (str(g) for g in a.guides):
            rec["guides"][G] = {k: mmm([r["guides"][G][k] for r in runs[s]]) for k in ("kernel", "call", "kernel_per_sample", "multiple_of_primary")}
            say(f"  guides G={G:>2}: kernel {fmt(rec['guides'][G]['kernel'])} ms, call {fmt(rec['guides'][G]['call'])} ms;  a sample {rec['guides'][G]['kernel_per_sample']['median']:.4f} ms = "
                f"{fmt(rec['guides'][G]['multiple_of_primary'])} x the frame's walk")
        for n in STATE_BYTES:
            rec["denoise"][n] = {"call": mmm([r["denoise"][n]["call"] for r in runs[s]]), "kernels": mmm([r["denoise"][n]["kernels"] for r in runs[s]]),
                                 "pack": mmm([r["denoise"][n]["pack"] for r in runs[s]]), "unpack": mmm([r["denoise"][n]["unpack"] for r in runs[s]]),
                                 "iterations": [mmm([r["denoise"][n]["iterations"][i] for r in runs[s]]) for i in range(a.iterations)],
                                 "state_bytes": STATE_BYTES[n], "gather_bytes": GATHER_BYTES[n]}
            say(f"  denoise {n:>16}: call {fmt(rec['denoise'][n]['call'])} ms, kernels {fmt(rec['denoise'][n]['kernels'])} = pack {rec['denoise'][n]['pack']['median']:.3f} + " +
                " + ".join(f"{m['median']:.3f}" for m in rec["denoise"][n]["iterations"]) + f" + unpack {rec['denoise'][n]['unpack']['median']:.3f};  state {STATE_BYTES[n]} B, gather {GATHER_BYTES[n]} B a pixel")
        g4, un = rec["guides"].get("4"), rec["denoise"]["unguided"]
        if g4:
            say(f"  G=4 guide call {g4['call']['median']:.3f} ms against the unguided {a.iterations}-iteration denoise call {un['call']['median']:.3f} ms: "
                f"{'MORE than the whole denoise call' if g4['call']['median'] > un['call']['median'] else 'less than the denoise call'}")
        out["sizes"][s] = rec
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
