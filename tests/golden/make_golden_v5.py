#!/usr/bin/env python
"""Fifth batch of golden vectors: THE WHOLE NETWORK ABOVE WIDTH 64.

  net72_*  StyleNBodyEmulatorVelCore.apply on a (1,3,104,104,104) input, mid_chan 72, z = 0.5, Om = 0.3 -> (1,3,8,8,8)
           displacement and velocity.  72 channels pad to 80 (a half-empty last 16-channel chunk), the decoder blocks are
           144 -> 144 -> 72 (nine chunks, three cout tiles with a ragged last one): the width at which the engine leaves the
           Winograd-z kernel in its decoders, the one-launch up-sampling and the one-pass head kernel
           (tests/wide_cases.py).  Float64 oracle (torch-CPU convolution core, pinned against the NumPy tap-wise GEMM in
           tests/test_oracle_pins.py), seeded inputs; stored as float64 like net64_* of golden_v1.npz.
           See make_golden.py for why the oracle and not the reference produces them.

Run from the repository root:  python tests/golden/make_golden_v5.py      (about a minute on 8 cores)
"""

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import cosmology as C, layers as L, model as M, params as P  # noqa: E402

Z, OM = 0.5, 0.3
DZ, VF = float(C.growth_factor(Z, OM)), float(C.vel_norm(Z, OM))
SEED_PARAMS, SEED_INPUT, MID, N = 7205, 72, 72, 104


def main():
    t = time.time()
    p = P.synthetic_params(seed=SEED_PARAMS, mid_chan=MID)
    x = np.random.default_rng(SEED_INPUT).standard_normal((1, 3, N, N, N)).astype(np.float32)
    with L.backend('torch'):
        d, v = M.forward(p, x, OM, DZ, VF)
    out = {"net72_disp": d[0], "net72_vel": v[0], "net72_meta": np.array([SEED_PARAMS, SEED_INPUT, MID, N, N, N])}
    np.savez_compressed(os.path.join(HERE, "golden_v5.npz"), **out)
    print("wrote golden_v5.npz:", {k: np.asarray(a).shape for k, a in out.items()}, "%.0f s" % (time.time() - t))


if __name__ == "__main__":
    main()
