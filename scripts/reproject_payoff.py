"""What reprojection buys behind a camera move (phx_dev_film_reproject): scenes.bmw_showroom and scenes.textured_showroom at 960 x 540 on one
GPU.  Camera B is camera A moved by a small orbit step (--angle radians about a pivot --pivot units in front of A).  Per scene:
  reference    one frame at --ref-spp samples under B (seed 1), on a device preprocessed with B
  history      --history frames of --spp samples under A (seeds 100, 101, ...), pooled
  the move     set_camera(B), the guide films of A and B (--guides samples), the reprojection of the history (max_history --max-history), one
               frame of --spp samples under B (seed 200)
and two films at the same cost in new samples: "restart" is that one frame alone, "reproject + one frame" is it pooled into the reprojected
history.  Reported per film as scripts/denoise_guided_payoff.py reports them: the MSE over RGB against the reference (pixels finite in all
films), the same without the 0.1 % largest per-pixel errors, and the shift of the film mean; then the share of pixels reused, and the mean's
shift over the reused pixels by the class of the material the pixel's centre ray meets first under B (phx_dev_trace): diffuse only, some
glossy or specular lobe, emitter.  The last line is one JSON record.

    python scripts/reproject_payoff.py [--spp 16] [--history 4] [--out profiles/r22_reproject_payoff.log]
"""
import argparse
import dataclasses
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--history", type=int, default=4)
    ap.add_argument("--max-history", type=int, default=64)
    ap.add_argument("--guides", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--angle", type=float, default=0.02)
    ap.add_argument("--pivot", type=float, default=4.0)
    ap.add_argument("--triangles", type=int, default=200_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--scenes", nargs="+", default=["bmw_showroom", "textured_showroom"])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r22_reproject_payoff.log"))
    a = ap.parse_args()
    import numpy as np
    from phosphorus_mk2_amd import abi, scenes, xpu
    xpu.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cases = {"textured_showroom": lambda: scenes.textured_showroom(a.triangles, a.width, a.height, a.tex_size),
             "bmw_showroom": lambda: scenes.bmw_showroom(a.triangles, a.width, a.height)}
    depth = 9
    out = {"spp": a.spp, "history_frames": a.history, "ref_spp": a.ref_spp, "angle": a.angle, "scenes": {}}
    for name in a.scenes:
        sc = cases[name]()
        W, H = sc.camera.width, sc.camera.height
        cam_a = sc.camera
        M = cam_a.to_world.astype(np.float64)
        c, s = math.cos(a.angle), math.sin(a.angle)
        R = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
        pivot = M[3, :3] - a.pivot * M[2, :3]             # the camera looks down its -z
        Mb = M.copy()
        Mb[:3, :3] = M[:3, :3] @ R
        Mb[3, :3] = pivot + (M[3, :3] - pivot) @ R
        cam_b = dataclasses.replace(cam_a, to_world=Mb.astype(np.float32))
        sc_b = dataclasses.replace(sc, camera=cam_b)

        def frame(dev, scene, seed):
            film = xpu.Film(W, H, 4, True, True, False)
            dev.start(scene, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, native_sink=True))
            dev.join()
            return film.data
        dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.ref_spp, paths_per_sample=1, path_depth=depth))
        try:
            dev.preprocess(sc_b)
            ref = frame(dev, sc_b, 1).copy()
            # the material class under every pixel's centre ray, camera B
            zoom = 1.12 * math.tan(0.5 * float(np.float32(cam_b.fov)))
            ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
            d = np.stack([(xs / W - 0.5) * (W / H) * zoom, (0.5 - ys / H) * zoom, -np.ones_like(xs)], -1) @ Mb[:3, :3]
            d /= np.linalg.norm(d, axis=-1, keepdims=True)
            hit = dev.trace(np.broadcast_to(Mb[3, :3], d.shape).reshape(-1, 3), d.reshape(-1, 3), np.full(W * H, 3.0e38, np.float32))
        finally:
            dev.close()
        prim_material = np.concatenate([np.full(len(faces), mat, np.int64) for m in sc.meshes for mat, faces in m.sets])

        def material_class(m):
            if m.is_emitter:
                return 2
            return 0 if all(l.type in (abi.LOBE_DIFFUSE, abi.LOBE_OREN_NAYAR) for l in m.lobes) else 1
        classes = np.array([material_class(m) for m in sc.materials])
        pixel_class = np.where(hit["hit"], classes[prim_material[np.minimum(hit["prim"], len(prim_material) - 1)]], 3).reshape(H, W)

        dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.spp, paths_per_sample=1, path_depth=depth))
        try:
            dev.preprocess(sc)
            acc = xpu.accumulator(W, H, 4, True)
            for k in range(a.history):
                dev.accumulate(acc, frame(dev, sc, 100 + k), a.spp, 4, True, False)
            guides_a = dev.render_guides(100, min(a.guides, a.spp))
            dev.set_camera(cam_b)
            guides_b = dev.render_guides(200, min(a.guides, a.spp))
            carried, moved = dev.reproject(acc, guides_a, guides_b, cam_a, cam_b, max_history=a.max_history)
            times = dev.reproject_times()
            one = frame(dev, sc, 200)
            restart, _ = dev.accumulate(xpu.accumulator(W, H, 4, True), one, a.spp, 4, True, False)
            pooled, _ = dev.accumulate(carried.copy(), one, a.spp, 4, True, False)
        finally:
            dev.close()
        ref_rgb = ref[..., :3].astype(np.float64)
        films = {"restart": restart[..., :3].astype(np.float64), "reproject + one frame": pooled[..., :3].astype(np.float64)}
        ok = np.isfinite(ref_rgb).all(-1)
        for rgb in films.values():
            ok &= np.isfinite(rgb).all(-1)
        reused = carried[..., 10] > 0
        say(f"{name}: {W}x{H} depth {depth}, reference {a.ref_spp} spp under B; history {a.history} x {a.spp} spp under A; orbit step {a.angle} rad about {a.pivot} units")
        say(f"  reprojection: {moved}; reused {100.0 * moved['reused'] / moved['pixels']:.1f} % of the pixels; call {times['call']:.2f} ms (host films), kernel {times['kernel']:.3f} ms")
        rec = {"film": [W, H], "summary": moved, "reused_share": moved["reused"] / moved["pixels"], "films": {}, "classes": {}}
        for label, rgb in films.items():
            e = ((rgb[ok] - ref_rgb[ok]) ** 2).sum(-1) / 3.0
            keep = np.sort(e)[:len(e) - max(1, int(round(0.001 * len(e))))]
            rec["films"][label] = {"mse": float(e.mean()), "trimmed_mse": float(keep.mean()), "mean_shift": float(rgb[ok].mean() / ref_rgb[ok].mean() - 1.0)}
        p = rec["films"]["restart"]
        for label, f in rec["films"].items():
            say(f"    {label:>22}: MSE {f['mse']:.4e} (x {f['mse'] / p['mse']:.3f} of restart);  without the 0.1 % worst pixels {f['trimmed_mse']:.4e} "
                f"(x {f['trimmed_mse'] / p['trimmed_mse']:.3f});  film mean {100 * f['mean_shift']:+.2f} % off the reference's")
        for k, cname in enumerate(("diffuse only", "glossy or specular lobe", "emitter", "nothing")):
            sel = ok & reused & (pixel_class == k)
            if sel.sum() < 100:
                continue
            shifts = {label: float(rgb[sel].mean() / ref_rgb[sel].mean() - 1.0) for label, rgb in films.items()}
            mses = {label: float((((rgb[sel] - ref_rgb[sel]) ** 2).sum(-1) / 3.0).mean()) for label, rgb in films.items()}
            rec["classes"][cname] = {"pixels": int(sel.sum()), "mean_shift": shifts, "mse": mses}
            say(f"    reused pixels on {cname:>24}: {int(sel.sum()):7d};  mean off the reference's: restart {100 * shifts['restart']:+.2f} %, "
                f"reproject + one frame {100 * shifts['reproject + one frame']:+.2f} %;  MSE x {mses['reproject + one frame'] / mses['restart']:.3f} of restart")
        out["scenes"][name] = rec
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
