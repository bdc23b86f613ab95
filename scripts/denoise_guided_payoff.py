"""What the guided filter buys (phx_dev_denoise_guided): scenes.textured_showroom (image textures on its surfaces) and scenes.bmw_showroom
(untextured: what demodulation costs where it has nothing to gain), both at 960 x 540 with the normals channel, on one GPU.  Per scene: a
reference, one uniform frame at --ref-spp samples (seed 1); then at each spp of --spp a uniform frame (seed 100), its guide film (--guides samples
a pixel, the frame's seed) and four films: plain, denoised unguided (phx_dev_denoise's defaults), guided (demodulated) and guided + plane.
Reported per film as scripts/denoise_payoff.py reports them: the MSE over the film's RGB against the reference (pixels finite in all films), the
same with the 0.1 % largest per-pixel squared errors of that film left out, and the bias of the film mean in standard errors of the difference
(per-pixel variances by film_variance from the PLAIN film's and the reference's own m2 channels).  The last line is one JSON record.

    python scripts/denoise_guided_payoff.py [--spp 16 64] [--guides 4] [--out profiles/r19_denoise_guided_payoff.log]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--guides", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--triangles", type=int, default=200_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--scenes", nargs="+", default=["textured_showroom", "bmw_showroom"])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r19_denoise_guided_payoff.log"))
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
    out = {"ref_spp": a.ref_spp, "guide_samples": a.guides, "scenes": {}}
    for name in a.scenes:
        sc = cases[name]()
        W, H = sc.camera.width, sc.camera.height

        def frame(spp, seed, filters=False):
            """-> (film data, frame_ms of the second of two frames, {name: (film, call ms)}, guide call ms)"""
            dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=spp, paths_per_sample=1, path_depth=depth))
            try:
                dev.preprocess(sc)
                for k in range(2):
                    film = xpu.Film(W, H, 4, True, True, False)
                    dev.start(sc, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, native_sink=True))
                    dev.join()
                ms = dev.stats()["frame_ms"]
                films, gms = {}, None
                if filters:
                    for k in range(2):
                        guides = dev.render_guides(seed, min(a.guides, spp))
                    gms = dev.guides_times()
                    for label, kw in (("unguided", {}), ("guided", dict(guides=guides)), ("guided+plane", dict(guides=guides, plane=True))):
                        for k in range(2):
                            den = dev.denoise(film.data, spp, 4, True, False, **kw)
                        films[label] = (den, dev.denoise_times()["call"])
                return film.data, ms, films, gms
            finally:
                dev.close()

        ref, ms, _, _ = frame(a.ref_spp, 1)
        ref_rgb = ref[..., :3].astype(np.float64)
        ref_var = xpu.film_variance(ref, a.ref_spp, normals=True)
        say(f"{name}: {W}x{H} depth {depth}, reference {a.ref_spp} spp uniform (seed 1, {ms:.1f} ms), film mean {np.nanmean(ref_rgb, (0, 1))}")
        rec = {"film": [W, H], "depth": depth, "rows": []}
        for spp in a.spp:
            data, ms, films, gms = frame(spp, 100, True)
            var = xpu.film_variance(data, spp, normals=True)
            rgbs = {"plain": data[..., :3].astype(np.float64)}
            rgbs.update({k: v[0][..., :3].astype(np.float64) for k, v in films.items()})
            ok = np.isfinite(ref_rgb).all(-1) & np.isfinite(var).all(-1) & np.isfinite(ref_var).all(-1)
            for rgb in rgbs.values():
                ok &= np.isfinite(rgb).all(-1)
            se = np.sqrt(var[ok].sum(0) + ref_var[ok].sum(0)) / ok.sum()
            row = {"spp": spp, "frame_ms": ms, "guide_kernel_ms": gms["kernel"], "guide_call_ms": gms["call"], "pixels_compared": int(ok.sum()), "films": {}}
            say(f"  uniform {spp} spp: frame {ms:.2f} ms, guides (G = {min(a.guides, spp)}, host film) kernel {gms['kernel']:.3f} ms, call {gms['call']:.2f} ms")
            for label, rgb in rgbs.items():
                e = ((rgb[ok] - ref_rgb[ok]) ** 2).sum(-1) / 3.0  # per pixel
                keep = np.sort(e)[:len(e) - max(1, int(round(0.001 * len(e))))]
                z = (rgb[ok].mean(0) - ref_rgb[ok].mean(0)) / se
                row["films"][label] = {"mse": float(e.mean()), "trimmed_mse": float(keep.mean()), "bias_z": z.tolist(),
                                       "mean_shift": float(rgb[ok].mean() / ref_rgb[ok].mean() - 1.0), "call_ms": films[label][1] if label in films else 0.0}
            p = row["films"]["plain"]
            for label, f in row["films"].items():
                say(f"    {label:>13}: MSE {f['mse']:.4e} (x {f['mse'] / p['mse']:.3f} of plain);  without the 0.1 % worst pixels {f['trimmed_mse']:.4e} (x {f['trimmed_mse'] / p['trimmed_mse']:.3f});  "
                    f"bias of the mean in standard errors {np.round(f['bias_z'], 2)} ({100 * f['mean_shift']:+.2f} % of the mean);  call {f['call_ms']:.2f} ms")
            u, g = row["films"]["unguided"], row["films"]["guided"]
            say(f"    guided / unguided: MSE x {g['mse'] / u['mse']:.3f}, trimmed x {g['trimmed_mse'] / u['trimmed_mse']:.3f};  guided+plane / unguided: MSE x "
                f"{row['films']['guided+plane']['mse'] / u['mse']:.3f}, trimmed x {row['films']['guided+plane']['trimmed_mse'] / u['trimmed_mse']:.3f}")
            rec["rows"].append(row)
        out["scenes"][name] = rec
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
