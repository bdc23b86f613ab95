"""What the film denoiser buys (phx_dev_denoise): scenes.sun_floor under light_sampling 0x301 (every pixel has the same
expectation; the sun makes the samples heavy-tailed) and scenes.bmw_showroom (200 000 triangles, general closures), both at 960 x 540 with
the normals channel, on one GPU.  Per scene: a reference, one uniform frame at --ref-spp samples (seed 1); then at each spp of --spp a
uniform frame and a frame of adaptive sampling at --tau (min_samples = step = spp / 4), seed 100, each denoised with the default settings
(5 iterations, sigma_l 4, normal power 2^7).  Reported per frame, plain and denoised: the MSE over the film's RGB against the reference
(pixels finite in all three), the same with the 0.1 % largest per-pixel squared errors of that film left out, denoised over plain, and the
bias of the film mean: the film's mean minus the reference's, per colour, in standard errors of that difference (per-pixel variances by
film_variance from the PLAIN film's and the reference's own m2 channels, summed over the pixels: the denoised film's m2 understates its
error and is not used for this).  Also the frame's time and the call's (host film: the upload and the download are in it) with its stages.
The last line is one JSON record.

    python scripts/denoise_payoff.py [--spp 16 64] [--tau 0.1] [--out profiles/r18_denoise_payoff.log]
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
    ap.add_argument("--tau", type=float, default=0.1)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--triangles", type=int, default=200_000)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--scenes", nargs="+", default=["sun_floor", "bmw_showroom"])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r18_denoise_payoff.log"))
    a = ap.parse_args()
    import numpy as np
    from phosphorus_mk2_amd import scenes, xpu
    xpu.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cases = {"sun_floor": (lambda: scenes.sun_floor(a.width, a.height), dict(light_sampling="area", light_selection="power", environment_sampling=True), 2),
             "bmw_showroom": (lambda: scenes.bmw_showroom(a.triangles, a.width, a.height), {}, 9)}
    out = {"ref_spp": a.ref_spp, "tau": a.tau, "scenes": {}}
    for name in a.scenes:
        make, kw, depth = cases[name]
        sc = make()
        W, H = sc.camera.width, sc.camera.height

        def frame(spp, seed, adaptive=False, denoise=False):
            """-> (film data, frame_ms of the second of two frames, the denoised film or None, the call's times)"""
            dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=spp, paths_per_sample=1, path_depth=depth, **kw))
            try:
                if adaptive:
                    dev.set_adaptive(a.tau, 0.0, max(2, spp // 4), max(1, spp // 4))
                dev.preprocess(sc)
                for k in range(2):
                    film = xpu.Film(W, H, 4, True, True, adaptive)
                    dev.start(sc, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32), film, native_sink=True))
                    dev.join()
                ms = dev.stats()["frame_ms"]
                den, times = None, None
                if denoise:
                    for k in range(2):
                        den = dev.denoise(film.data, spp, 4, True, adaptive)
                    times = dev.denoise_times()
                return film.data, ms, den, times
            finally:
                dev.close()

        ref, ms, _, _ = frame(a.ref_spp, 1)
        ref_rgb = ref[..., :3].astype(np.float64)
        ref_var = xpu.film_variance(ref, a.ref_spp, normals=True)
        say(f"{name}: {W}x{H} depth {depth}, reference {a.ref_spp} spp uniform (seed 1, {ms:.1f} ms), film mean {np.nanmean(ref_rgb, (0, 1))}")
        rec = {"film": [W, H], "depth": depth, "rows": []}
        for spp in a.spp:
            for adaptive in (False, True):
                data, ms, den, times = frame(spp, 100, adaptive, True)
                plain_rgb, den_rgb = data[..., :3].astype(np.float64), den[..., :3].astype(np.float64)
                var = xpu.film_variance(data, spp, normals=True, adaptive=adaptive)
                ok = np.isfinite(plain_rgb).all(-1) & np.isfinite(den_rgb).all(-1) & np.isfinite(ref_rgb).all(-1) & np.isfinite(var).all(-1) & np.isfinite(ref_var).all(-1)

                def errors(rgb):
                    e = ((rgb[ok] - ref_rgb[ok]) ** 2).sum(-1) / 3.0  # per pixel
                    keep = np.sort(e)[:len(e) - max(1, int(round(0.001 * len(e))))]
                    return float(e.mean()), float(keep.mean())
                (mse_p, trim_p), (mse_d, trim_d) = errors(plain_rgb), errors(den_rgb)
                se = np.sqrt(var[ok].sum(0) + ref_var[ok].sum(0)) / ok.sum()
                z_p = (plain_rgb[ok].mean(0) - ref_rgb[ok].mean(0)) / se
                z_d = (den_rgb[ok].mean(0) - ref_rgb[ok].mean(0)) / se
                shift = float(den_rgb[ok].mean() / ref_rgb[ok].mean() - 1.0)
                label = f"{'adaptive tau ' + str(a.tau) if adaptive else 'uniform'} {spp} spp"
                row = {"frame": label, "spp": spp, "adaptive": adaptive, "frame_ms": ms, "denoise_call_ms": times["call"],
                       "denoise_kernels_ms": times["pack"] + times["unpack"] + sum(times["iterations"]), "mse_plain": mse_p, "mse_denoised": mse_d,
                       "mse_ratio": mse_d / mse_p, "trimmed_mse_plain": trim_p, "trimmed_mse_denoised": trim_d, "trimmed_mse_ratio": trim_d / trim_p,
                       "bias_z_plain": z_p.tolist(), "bias_z_denoised": z_d.tolist(), "mean_shift_denoised": shift, "pixels_compared": int(ok.sum()),
                       "mean_samples": float(data[..., 10].astype(np.float64).mean()) if adaptive else float(spp)}
                rec["rows"].append(row)
                say(f"  {label:>26}: frame {ms:7.2f} ms, denoise call {row['denoise_call_ms']:.2f} ms (kernels {row['denoise_kernels_ms']:.2f});  mean samples {row['mean_samples']:.2f};  "
                    f"MSE {mse_p:.4e} -> {mse_d:.4e} (x {mse_d / mse_p:.3f});  without the 0.1 % worst pixels {trim_p:.4e} -> {trim_d:.4e} (x {trim_d / trim_p:.3f});  "
                    f"bias of the mean in standard errors: plain {np.round(z_p, 2)}, denoised {np.round(z_d, 2)} ({100 * shift:+.2f} % of the mean)")
        out["scenes"][name] = rec
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
