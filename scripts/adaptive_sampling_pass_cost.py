"""What a pass costs on scenes.bmw_showroom(200 000) at 960 x 540, 128 spp, with and without adaptive sampling: the uniform frame in one pass and in
passes of 16 and 64 samples (samples_in_flight), adaptive sampling with a threshold of 0 (only pixels whose samples are all equal stop) in rounds of
16 and 64, and with tau 0.2 in rounds of 16/16, 32/32 and 16/48.  Prints phx_stats of the best of two frames behind a warm-up frame.  Run on an MI355X;
profiles/r16_adaptive_sampling_pass_cost.log is its output."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phosphorus_mk2_amd import scenes, xpu

xpu.load_library()
sc = scenes.bmw_showroom(200_000, 960, 540)
W, H = 960, 540
for label, flight, ad in (("uniform, one pass", 0, None), ("uniform, samples_in_flight 16", 16, None), ("uniform, samples_in_flight 64", 64, None),
                          ("adaptive tau 0, 16/16", 0, (0.0, 16, 16)), ("adaptive tau 0, 64/64", 0, (0.0, 64, 64)), ("adaptive tau 0.2, 16/16", 0, (0.2, 16, 16)),
                          ("adaptive tau 0.2, 32/32", 0, (0.2, 32, 32)), ("adaptive tau 0.2, 16/48", 0, (0.2, 16, 48))):
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=128, paths_per_sample=1, path_depth=9, samples_in_flight=flight))
    try:
        if ad:
            dev.set_adaptive(ad[0], 0.0, ad[1], ad[2])
        dev.preprocess(sc)
        best = None
        for k in range(3):
            film = xpu.Film(W, H, 4, False, True, ad is not None)
            dev.start(sc, xpu.FrameState(100, xpu.Tiles.make(W, H, 32), film, native_sink=True))
            dev.join()
            st = dev.stats()
            if k and (best is None or st["frame_ms"] < best["frame_ms"]):
                best = st
        n = film.data[..., 7].mean() if ad else 128.0
        print(f"{label:>32}: frame {best['frame_ms']:7.2f} ms  trace {best['trace_ms']:7.2f}  shade {best['shade_ms']:7.2f} (kernels {best['shade_kernel_ms']:7.2f})  "
              f"k_trace launches {best['trace_launches']:4d}  mean samples {n:6.2f}  rays {best['rays_closest'] + best['rays_shadow']}", flush=True)
    finally:
        dev.close()
