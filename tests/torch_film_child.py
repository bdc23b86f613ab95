"""Child process of test_gpu_film_sinks.py::test_torch_tensor_as_the_device_film: bench.py's order -- torch initialises the GPU first, then
the library renders into a torch tensor's memory.  usage: python torch_film_child.py OUT.npz   (films and counts for the parent to judge)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SENTINEL, SPP, DEPTH = 12345.0, 5, 4


def main(out):
    import torch
    torch.cuda.set_device(0)
    from phosphorus_mk2_amd import scenes, xpu
    W, H = 72, 40
    sc = scenes.soup(3000, width=W, height=H)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=DEPTH, device_ordinal=torch.cuda.current_device()))
    dev.preprocess(sc)
    res = {}

    def frame(key, seed, film, rank=0, world=1, **layout):
        torch.cuda.synchronize()  # the fill ran on torch's stream
        dev.start(sc, xpu.FrameState(seed, xpu.Tiles.make(W, H, 32, rank, world), None, device_film_ptr=film.data_ptr(), **layout))
        dev.join()
        res[key] = film.cpu().numpy()
        res[key + "_rays"] = np.array([dev.stats()[k] for k in ("camera_samples", "rays_closest", "rays_shadow", "rays_masked", "tiles")], np.int64)

    film = torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
    frame("rank0", 7, film, 0, 2)        # the sentinel stays outside rank 0's tiles
    frame("seed7", 7, film)              # bench.py's frame: no layout given
    frame("seed8", 8, film)              # replaced, not added to
    film7 = torch.full((H, W, 7), SENTINEL, dtype=torch.float32, device="cuda")
    frame("seed7_normals", 7, film7, primary_components=4, normals=True)
    dev.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
