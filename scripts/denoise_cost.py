"""What the film denoiser costs (phx_dev_denoise): the bench scene -- Soup 100 k, 256 spp, depth 9 -- rendered on one GPU into a
device-resident film with normals and moments (10 floats a pixel) at 1280 x 720 and at 3840 x 2160, then denoised with 5 iterations from that
film into a second device film, so that every call does the same work.

Per size a process of its own, --rounds times, interleaved (720p, 2160p, 720p, ...).  A process renders one frame, makes --warmup calls and
then --calls timed ones; a call's figures are the library's own HIP events (phx_dev_denoise_times: pack, each iteration, unpack) and its host
clock around the whole call, allocation and release of the working memory included.  A process reports the median over its calls, the script
the median and the range over the processes, next to the frame's time.

Per iteration the achieved bytes/s against a byte model kept here (bytes per valid pixel and iteration):
    compulsory   read  c 16 + v 16 + n 16 + e 8, write c 16 + v 16 + e 8                      =   96
    gather       25 taps x (n 16 + c 16 + v 16) + 9 yardstick neighbours x (n 16 + e 8)       = 1416
and the binary64 operations by a count of the rule: 25 taps x 40 + 9 x 4 + 30 = 1066 a pixel.  The ceilings they are put against are those of
MI355X_MICROARCH.md: HBM 6.29 TB/s measured for the compulsory bytes, the L2's 34.5 TB/s for the gather (which the vector L1 serves first).

    python scripts/denoise_cost.py [--rounds 3] [--calls 10] [--out profiles/r18_denoise_cost.log]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPULSORY_BYTES, GATHER_BYTES, FLOPS = 96, 25 * 48 + 9 * 24, 25 * 40 + 9 * 4 + 30
HBM_TBS, L2_TBS = 6.29, 34.5
SIZES = {"720p": (1280, 720), "2160p": (3840, 2160)}


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def one(a):
    """a child process: one frame, then the calls; prints one JSON line"""
    sys.path.insert(0, HERE)
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    hip = C.CDLL("libamdhip64.so.7")  # the runtime the library runs on
    W, H = SIZES[a.one]
    xs = 10
    sc = scenes.soup(a.triangles, width=W, height=H)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.spp, paths_per_sample=1, path_depth=9))
    src, dst = C.c_void_p(), C.c_void_p()
    try:
        dev.preprocess(sc)
        nbytes = W * H * xs * 4
        assert hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)) == 0
        frame_ms = []
        for k in range(2):
            dev.start(sc, xpu.FrameState(1, xpu.Tiles.make(W, H, 32), None, device_film_ptr=src.value, primary_components=4, normals=True, moments=True))
            dev.join()
            frame_ms.append(dev.stats()["frame_ms"])
        q = xpu.denoise_settings((H, W, xs), a.spp, 4, True, False, iterations=a.iterations)
        q.on_device = 1
        rows = []
        for k in range(a.warmup + a.calls):
            rc = dev._lib.phx_dev_denoise(dev._h, C.byref(q), src.value, dst.value)
            assert rc == 0, dev._lib.phx_last_error()
            if k >= a.warmup:
                rows.append(dev.denoise_times())
        film = np.empty((H, W, xs), np.float32)
        assert hip.hipMemcpy(film.ctypes.data_as(C.c_void_p), src, C.c_size_t(nbytes), 2) == 0
        out = np.empty_like(film)
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), dst, C.c_size_t(nbytes), 2) == 0
        m2 = film[..., 7:10]
        valid = int((np.isfinite(film[..., :10]).all(-1) & (m2 >= 0).all(-1)).sum())
        changed = int((out[..., :3] != film[..., :3]).any(-1).sum())
        print(json.dumps({"size": a.one, "pixels": W * H, "valid_pixels": valid, "pixels_changed": changed, "frame_ms": frame_ms[1],
                          "pack": median([r["pack"] for r in rows]), "unpack": median([r["unpack"] for r in rows]),
                          "iterations": [median([r["iterations"][i] for r in rows]) for i in range(a.iterations)],
                          "kernels": median([r["pack"] + r["unpack"] + sum(r["iterations"]) for r in rows]), "call": median([r["call"] for r in rows]),
                          "mean_m2_before": float(m2.astype(np.float64).mean()), "mean_m2_after": float(out[..., 7:10].astype(np.float64).mean())}))
    finally:
        dev.close()
        for p in (src, dst):
            if p.value:
                hip.hipFree(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r18_denoise_cost.log"))
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
                   "--warmup", str(a.warmup), "--calls", str(a.calls)]
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=400)
            if p.returncode:
                sys.exit(f"{s}, round {r}: exit status {p.returncode}\n{p.stdout}\n{p.stderr}")  # nothing more is started on the GPU
            row = json.loads(p.stdout.strip().splitlines()[-1])
            runs[s].append(row)
            say(f"round {r} {s:>5}: frame {row['frame_ms']:8.2f} ms  call {row['call']:7.3f} ms  kernels {row['kernels']:7.3f} ms = pack {row['pack']:.3f} + "
                f"{' + '.join(f'{v:.3f}' for v in row['iterations'])} + unpack {row['unpack']:.3f}  ({row['valid_pixels']} of {row['pixels']} pixels valid, "
                f"{row['pixels_changed']} changed, mean m2 {row['mean_m2_before']:.4g} -> {row['mean_m2_after']:.4g})")
    out = {"scene": f"soup({a.triangles}) {a.spp} spp depth 9, device-resident film of 10 floats a pixel, {a.iterations} iterations", "runs": runs, "sizes": {}}
    for s in a.sizes:
        rec = {}
        for key in ("frame_ms", "call", "kernels", "pack", "unpack"):
            v = [row[key] for row in runs[s]]
            rec[key] = {"median": median(v), "min": min(v), "max": max(v)}
        px = runs[s][0]["valid_pixels"]
        rec["iterations"] = []
        for i in range(a.iterations):
            v = [row["iterations"][i] for row in runs[s]]
            ms = median(v)
            rec["iterations"].append({"step": 1 << i, "median": ms, "min": min(v), "max": max(v), "compulsory_TBs": px * COMPULSORY_BYTES / ms / 1e9,
                                      "gather_TBs": px * GATHER_BYTES / ms / 1e9, "binary64_TFLOPs": px * FLOPS / ms / 1e9})
        out["sizes"][s] = rec
        say(f"{s}: frame {rec['frame_ms']['median']:.2f} ms ({rec['frame_ms']['min']:.2f} - {rec['frame_ms']['max']:.2f});  call {rec['call']['median']:.3f} ms "
            f"({rec['call']['min']:.3f} - {rec['call']['max']:.3f}) = {100 * rec['call']['median'] / rec['frame_ms']['median']:.2f} % of the frame;  kernels "
            f"{rec['kernels']['median']:.3f} ms ({rec['kernels']['min']:.3f} - {rec['kernels']['max']:.3f});  pack {rec['pack']['median']:.3f}  unpack {rec['unpack']['median']:.3f}")
        for it in rec["iterations"]:
            say(f"  step {it['step']:3d}: {it['median']:.3f} ms ({it['min']:.3f} - {it['max']:.3f})  compulsory {it['compulsory_TBs']:.3f} TB/s = "
                f"{100 * it['compulsory_TBs'] / HBM_TBS:.1f} % of HBM's {HBM_TBS};  gather {it['gather_TBs']:.2f} TB/s = {100 * it['gather_TBs'] / L2_TBS:.1f} % of the L2's {L2_TBS};  "
                f"binary64 {it['binary64_TFLOPs']:.2f} TFLOP/s")
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
