"""What the outlier clamp buys in the two cases it was built for (phx_dev_film_outlier_clamp): scenes.textured_showroom and
scenes.bmw_showroom at 960 x 540 on one GPU.
  history clamp   scripts/reproject_payoff.py's orbit step: --history frames of --spp samples under camera A, pooled; camera B is A
                  moved by --angle radians about a pivot --pivot units in front of it; the history is reprojected to B and one frame of --spp
                  samples under B is pooled into it, without and with the clamp of the reprojected history against that frame (two-sided,
                  the centre included; --history-clamp radius gamma trim clamped_history).  "restart" is that one frame alone.
  despeckle       scripts/denoise_guided_payoff.py's frame: one frame of --spp samples under A, denoised guided + plane, without and
                  with the despeckle of the frame before the filter (the centre excluded, upper only; --despeckle radius gamma trim).
Reported per film: the MSE over RGB against a reference of --ref-spp samples under the same camera (pixels finite in all films), the same
without the 0.1 % largest per-pixel errors, and the film mean against the reference's: the energy the clamp removed.  The last line is one
JSON record.

    python scripts/outlier_clamp_payoff.py [--spp 16] [--history 4] [--out profiles/r23_outlier_clamp_payoff.log]
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
    ap.add_argument("--history-clamp", type=float, nargs=4, default=[1, 3.0, 0, 8], metavar=("RADIUS", "GAMMA", "TRIM", "CLAMPED_HISTORY"))
    ap.add_argument("--despeckle", type=float, nargs=3, default=[2, 4.0, 2], metavar=("RADIUS", "GAMMA", "TRIM"))
    ap.add_argument("--scenes", nargs="+", default=["textured_showroom", "bmw_showroom"])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r23_outlier_clamp_payoff.log"))
    a = ap.parse_args()
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cases = {"textured_showroom": lambda: scenes.textured_showroom(a.triangles, a.width, a.height, a.tex_size),
             "bmw_showroom": lambda: scenes.bmw_showroom(a.triangles, a.width, a.height)}
    depth = 9
    hc = dict(radius=int(a.history_clamp[0]), gamma=a.history_clamp[1], trim=int(a.history_clamp[2]), min_taps=4, clamped_history=int(a.history_clamp[3]))
    ds = dict(radius=int(a.despeckle[0]), gamma=a.despeckle[1], trim=int(a.despeckle[2]), min_taps=4)
    out = {"spp": a.spp, "history_frames": a.history, "ref_spp": a.ref_spp, "angle": a.angle, "history_clamp": hc, "despeckle": ds, "scenes": {}}

    def report(films, ref, first):
        """films: label -> (H, W, >= 3); -> label -> {mse, trimmed_mse, mean_shift}, said against the film `first`"""
        ref_rgb = ref[..., :3].astype(np.float64)
        rgbs = {k: v[..., :3].astype(np.float64) for k, v in films.items()}
        ok = np.isfinite(ref_rgb).all(-1)
        for rgb in rgbs.values():
            ok &= np.isfinite(rgb).all(-1)
        rec = {}
        for label, rgb in rgbs.items():
            e = ((rgb[ok] - ref_rgb[ok]) ** 2).sum(-1) / 3.0
            keep = np.sort(e)[:len(e) - max(1, int(round(0.001 * len(e))))]
            rec[label] = {"mse": float(e.mean()), "trimmed_mse": float(keep.mean()), "mean_shift": float(rgb[ok].mean() / ref_rgb[ok].mean() - 1.0)}
        p = rec[first]
        for label, f in rec.items():
            say(f"    {label:>36}: MSE {f['mse']:.4e} (x {f['mse'] / p['mse']:.3f} of {first});  without the 0.1 % worst pixels {f['trimmed_mse']:.4e} "
                f"(x {f['trimmed_mse'] / p['trimmed_mse']:.3f});  film mean {100 * f['mean_shift']:+.2f} % off the reference's")
        return rec

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

        def frame(dev, seed):
            film = xpu.Film(W, H, 4, True, True, False)
            dev.start(sc, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, native_sink=True))
            dev.join()
            return film.data
        dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.ref_spp, paths_per_sample=1, path_depth=depth))
        try:
            dev.preprocess(sc)
            ref_a = frame(dev, 1).copy()
            dev.set_camera(cam_b)
            ref_b = frame(dev, 1).copy()
        finally:
            dev.close()
        dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=a.spp, paths_per_sample=1, path_depth=depth))
        try:
            dev.preprocess(sc)
            # despeckle before the guided + plane filter, camera A
            plain = frame(dev, 100).copy()
            guides_a = dev.render_guides(100, min(a.guides, a.spp))
            speckless, s_ds = dev.clamp_outliers(plain.copy(), normals=True, **ds)
            t_ds = dev.outlier_clamp_times()
            filtered = dev.denoise(plain, a.spp, 4, True, False, guides=guides_a, plane=True)
            filtered_ds = dev.denoise(speckless, a.spp, 4, True, False, guides=guides_a, plane=True)
            # the orbit step
            acc = xpu.accumulator(W, H, 4, True)
            for k in range(a.history):
                dev.accumulate(acc, frame(dev, 100 + k), a.spp, 4, True, False)
            dev.set_camera(cam_b)
            guides_b = dev.render_guides(200, min(a.guides, a.spp))
            carried, moved = dev.reproject(acc, guides_a, guides_b, cam_a, cam_b, max_history=a.max_history)
            one = frame(dev, 200)
            restart, _ = dev.accumulate(xpu.accumulator(W, H, 4, True), one, a.spp, 4, True, False)
            pooled, _ = dev.accumulate(carried.copy(), one, a.spp, 4, True, False)
            clamped, s_hc = dev.clamp_outliers(carried.copy(), one, exclude_centre=False, upper_only=False, normals=True, samples=True, **hc)
            t_hc = dev.outlier_clamp_times()
            pooled_hc, _ = dev.accumulate(clamped, one, a.spp, 4, True, False)
        finally:
            dev.close()
        say(f"{name}: {W}x{H} depth {depth}, references {a.ref_spp} spp under A and B; {a.spp} spp a frame")
        say(f"  despeckle {ds} before guided + plane denoise, camera A: {s_ds}; call {t_ds['call']:.2f} ms (host films), kernel {t_ds['kernel']:.3f} ms")
        rec = {"film": [W, H], "despeckle_summary": s_ds, "history_clamp_summary": s_hc, "reprojection": moved}
        rec["despeckle"] = report({"plain": plain, "despeckled": speckless, "guided + plane": filtered, "despeckled, guided + plane": filtered_ds}, ref_a, "plain")
        f0, f1 = rec["despeckle"]["guided + plane"], rec["despeckle"]["despeckled, guided + plane"]
        say(f"    despeckle before the filter: MSE x {f1['mse'] / f0['mse']:.3f}, trimmed x {f1['trimmed_mse'] / f0['trimmed_mse']:.3f} of the filter alone; "
            f"energy lost by the despeckle {-100 * (rec['despeckle']['despeckled']['mean_shift'] - rec['despeckle']['plain']['mean_shift']):.2f} % of the film mean")
        say(f"  history clamp {hc}, orbit step {a.angle} rad about {a.pivot} units, history {a.history} x {a.spp} spp: reprojection {moved}")
        say(f"    clamp: {s_hc}; call {t_hc['call']:.2f} ms (host films), kernel {t_hc['kernel']:.3f} ms")
        rec["history"] = report({"restart": restart, "reproject + one frame": pooled, "reproject + clamp + one frame": pooled_hc}, ref_b, "restart")
        h0, h1 = rec["history"]["reproject + one frame"], rec["history"]["reproject + clamp + one frame"]
        say(f"    clamp against no clamp: MSE x {h1['mse'] / h0['mse']:.3f}, trimmed x {h1['trimmed_mse'] / h0['trimmed_mse']:.3f}; "
            f"energy lost by the clamp {-100 * (h1['mean_shift'] - h0['mean_shift']):.2f} % of the film mean")
        out["scenes"][name] = rec
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
