"""Generates tests/golden/ref_live_vectors.npz from oracle/_ref/libphx_ref_subset.so (the reference's own object code, see
make_ref_subset_vectors.py): the inputs and the reference's outputs of tests/test_oracle_pins.py::test_live_ref_subset_if_present, so
that the test runs where the reference is not at hand and checks the live library against them where it is:

    make -C oracle ref && python tests/golden/make_ref_live_vectors.py
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libphx_ref_subset.so"))
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
rng = np.random.default_rng(7)
cosi = rng.uniform(-1, 1, 4096).astype(np.float32); eta = rng.uniform(0.3, 3.0, 4096).astype(np.float32)
fres = np.zeros(4096, np.float32)
lib.ref_fresnel_dielectric(4096, fp(cosi), fp(eta), fp(fres))
x = rng.uniform(0.01, 100, 8).astype(np.float32); rcp = np.zeros(8, np.float32)
lib.ref_rcp8(fp(x), fp(rcp))
np.savez(os.path.join(ROOT, "tests", "golden", "ref_live_vectors.npz"), cosi=cosi, eta=eta, fresnel=fres, rcp_in=x, rcp=rcp)
