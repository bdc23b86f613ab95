"""What an image on a lamp's emission costs: the closed showroom at BASELINE config-3 size (scenes.bmw_showroom: 500 k triangles,
1920 x 1080, 1024 spp, depth 9) rendered on one GPU three ways

    image     its lamps carry a procedural 2048^2 LINEAR image on their emission (phx_material.emission_uv_texture, UVs over [0, 1]^2)
    mean      the same scene with a 1 x 1 image of that image's mean: the same kernels and branches, every lookup on one texel
    constant  the lamps as they are: no image, the scene's own kernels (k_shade_g<PERHIT> without TEX)

each in a process of its own, --rounds times, interleaved (image, mean, constant, image, ...), so that drift of the machine lands on
all three alike.  "image" against "mean" is the cost of the texel gathers at hits and light samples; "mean" against "constant" is the cost
of routing the scene to the TEX kernels (corner UVs requested with every hit) plus the lookups themselves.  Prints phx_stats' frame_ms,
shade_kernel_ms (k_shade_g) and trace_ms of every run, each mode's median and range, and one JSON line.

    python scripts/emission_texture_cost.py [--rounds 3] [--frames 2] [--tex 2048] [--out profiles/r11_emission_texture_cost.log]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["image", "mean", "constant"]


def lamp_scene(a, mode):
    import numpy as np
    from phosphorus_mk2_amd import abi, scenes
    sc = scenes.bmw_showroom(a.triangles, a.width, a.height)
    if mode == "constant":
        return sc
    img = scenes.procedural_texture(a.tex, 11)
    mean = img.reshape(-1, 3).mean(0, dtype=np.float64).astype(np.float32).reshape(1, 1, 3)
    sc.textures = [scenes.TextureDesc(img if mode == "image" else mean, abi.TEX_LINEAR)]
    lamps = 0
    for m in sc.meshes:
        if any(sc.materials[mat].is_emitter for mat, _ in m.sets):
            assert len(m.faces) == 2 and len(m.vertices) == 4, "the showroom's lamps are quads"
            m.uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
            m.flags |= abi.MESH_UV_PER_VERTEX
            lamps += 1
    assert lamps
    for mat in sc.materials:
        if mat.is_emitter:
            mat.emission_uv_texture = 1
    sc.name += "_lamp_" + mode
    return sc


def one(a):
    """a child process: one device, one warm-up frame, a.frames timed ones; prints one JSON line"""
    sys.path.insert(0, HERE)
    import numpy as np
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    sc = lamp_scene(a, a.one)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.spp, paths_per_sample=1, path_depth=9))
    try:
        dev.preprocess(sc)
        W, H = sc.camera.width, sc.camera.height
        best, first = None, None
        for k in range(a.frames + 1):  # the first frame warms up and is not counted
            film = xpu.Film(W, H, 4)
            dev.start(sc, xpu.FrameState(1 + k, xpu.Tiles.make(W, H, 32), film, native_sink=True))
            dev.join()
            st = dev.stats()
            if k == 0:
                first = {"rays_closest": st["rays_closest"], "rays_shadow": st["rays_shadow"], "film_mean": [float(x) for x in np.nanmean(film.data[..., :3], (0, 1))]}
            if k and (best is None or st["frame_ms"] < best["frame_ms"]):
                best = st
        print(json.dumps({"mode": a.one, "frame_ms": best["frame_ms"], "trace_ms": best["trace_ms"], "shade_kernel_ms": best["shade_kernel_ms"],
                          "shade_kernels": best["shade_kernels"], "rays": best["rays_closest"] + best["rays_shadow"], "device_bytes": best["device_bytes"], **first}))
    finally:
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--tex", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r11_emission_texture_cost.log"))
    ap.add_argument("--one", choices=MODES, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    runs = {m: [] for m in MODES}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for r in range(a.rounds):
        for m in MODES:
            env = {k: v for k, v in os.environ.items() if k != "PHX_LIB"}
            cmd = [sys.executable, os.path.abspath(__file__), "--one", m, "--triangles", str(a.triangles), "--width", str(a.width), "--height", str(a.height),
                   "--spp", str(a.spp), "--tex", str(a.tex), "--frames", str(a.frames)]
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
            if p.returncode:
                sys.exit(f"{m}, round {r}: exit status {p.returncode}\n{p.stdout}\n{p.stderr}")  # nothing more is started on the GPU
            row = json.loads(p.stdout.strip().splitlines()[-1])
            runs[m].append(row)
            say(f"round {r} {m:>8}: frame {row['frame_ms']:9.1f} ms  k_shade_g {row['shade_kernel_ms']:9.1f} ms  k_trace {row['trace_ms']:9.1f} ms  "
                f"{row['rays'] / row['frame_ms'] / 1e3:8.1f} Mrays/s  {row['device_bytes'] / 2**20:9.1f} MiB  kernels {row['shade_kernels']:#x}  film mean {row['film_mean']}")
    # the three modes trace the same paths (an emission changes no ray); image and mean run the same kernels, constant the scene's own
    assert len({(row["rays_closest"], row["rays_shadow"]) for m in MODES for row in runs[m]}) == 1, "the modes traced different rays"
    assert len({row["shade_kernels"] for m in ("image", "mean") for row in runs[m]}) == 1
    assert runs["constant"][0]["shade_kernels"] != runs["image"][0]["shade_kernels"]
    out = {"scene": f"bmw_showroom({a.triangles}) {a.width}x{a.height} {a.spp} spp depth 9, lamp image {a.tex}^2 LINEAR", "runs": runs}
    for key in ("frame_ms", "shade_kernel_ms", "trace_ms"):
        for m in MODES:
            v = [row[key] for row in runs[m]]
            out[f"{m}_{key}"] = {"best": min(v), "median": sorted(v)[len(v) // 2], "range": max(v) - min(v)}
        say(f"{key:>16}: " + "  ".join(f"{m} median {out[f'{m}_{key}']['median']:.1f} range {out[f'{m}_{key}']['range']:.1f}" for m in MODES))
    pct = lambda x, y, key: 100.0 * (out[f"{x}_{key}"]["median"] / out[f"{y}_{key}"]["median"] - 1.0)
    for x, y in (("image", "mean"), ("mean", "constant"), ("image", "constant")):
        out[f"{x}_vs_{y}_pct"] = {key: pct(x, y, key) for key in ("frame_ms", "shade_kernel_ms", "trace_ms")}
        say(f"{x} against {y} (medians): frame {out[f'{x}_vs_{y}_pct']['frame_ms']:+.2f} %  k_shade_g {out[f'{x}_vs_{y}_pct']['shade_kernel_ms']:+.2f} %  "
            f"k_trace {out[f'{x}_vs_{y}_pct']['trace_ms']:+.2f} %")
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
