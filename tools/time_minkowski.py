#!/usr/bin/env python
"""Time density.minkowski_functionals on one MI355X: n^3 fields (default 256^3, 512^3, 1024^3) with T = 41 and T = 1024
thresholds, standardization on and off, for three fields made on the device:

  grf        Gaussian random field (P(k) ~ k^-1.5 exp(-(k R)^2), R = 4 cells), smooth over a few cells
  constant   every voxel 1.0: every lane of a wave adds to one histogram bin (the worst case for LDS contention)
  cic        the CIC-painted, deconvolved delta of a Zel'dovich-like displacement of min(n, 512)^3 particles

Per case: the device time of the moments (nbe_field_moments) and of the counts pass (nbe_minkowski_counts), by HIP
events, the whole call (host clock, NumPy results back), and the HBM floor of the three reads of the field (two moment
passes and the counts pass) at the achievable 6.3 TB/s.  For comparison it times the tool's own NumPy restatement, one
mask and its periodic shifts per threshold, at a CPU-sized mesh and extrapolates in n^3 T.

    python tools/time_minkowski.py --out profiles/minkowski_timing_512.json
"""

import argparse
import ctypes as C
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, density as D  # noqa: E402
from time_density import gaussian_displacement  # noqa: E402

HBM = 6.3e12


def grf(n, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    dk = torch.fft.rfftn(torch.randn((n, n, n), generator=g, device=dev, dtype=torch.float32))
    f = torch.fft.fftfreq(n, device=dev)
    fz = torch.fft.rfftfreq(n, device=dev)
    k2 = f[:, None, None] ** 2 + f[None, :, None] ** 2 + fz[None, None, :] ** 2
    k2[0, 0, 0] = 1.0
    amp = k2.pow(-0.375) * torch.exp(-k2 * (2 * np.pi * 4.0) ** 2 / 2)
    amp[0, 0, 0] = 0.0
    x = torch.fft.irfftn(dk * amp, s=(n, n, n))
    return (x / x.std()).contiguous()


def make_field(kind, n, dev):
    if kind == "grf":
        return grf(n, 1, dev)
    if kind == "constant":
        return torch.ones((n, n, n), dtype=torch.float32, device=dev)
    npart = min(n, 512)
    disp = gaussian_displacement(npart, 1000.0, 6.0, 2, dev)
    out = D.paint_density(disp, 1000.0, n, 2, deconvolve=True)
    del disp
    return out


def time_kernels(x, T, standardize, reps):
    """ms of the moments launches and of the counts launch (medians of reps, device events)."""
    l = _lib.lib()
    dev = x.device
    n = int(x.shape[0])
    s = D._stream(dev)
    thr = torch.linspace(-3, 3, T, device=dev, dtype=torch.float32) if T != 41 else \
        torch.from_numpy(np.linspace(-3, 3, 41, dtype=np.float32)).to(dev)
    mom = torch.empty(D._MOMENT_WORDS, dtype=torch.float64, device=dev)
    hist = torch.zeros(4 * (T + 1) + 1, dtype=torch.int64, device=dev)
    tm, tc = [], []
    for r in range(reps + 1):
        hist.zero_()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _lib.check(l.nbe_field_moments(D._ptr(x), n, D._ptr(mom), s))
        e[1].record()
        _lib.check(l.nbe_minkowski_counts(D._ptr(x), n, D._ptr(thr), T, D._ptr(mom) if standardize else None,
                                          D._ptr(hist), s))
        e[2].record()
        torch.cuda.synchronize()
        if r:
            tm.append(e[0].elapsed_time(e[1]))
            tc.append(e[1].elapsed_time(e[2]))
    total = int(hist[:-1].view(4, T + 1).sum(1)[3])
    assert total == n ** 3, "cube count %d != n^3" % total
    return float(np.median(tm)), float(np.median(tc))


def time_call(x, T, standardize, reps):
    thr = np.linspace(-3, 3, T, dtype=np.float32)
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.minkowski_functionals(x, 1000.0, thresholds=thr, standardize=standardize)
        if r:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def numpy_counts(w, thresholds):
    """One mask per threshold and the periodic shifts of the cubical-complex definition (include/nbe.h)."""
    def any_of(m, shifts):
        o = np.zeros_like(m)
        for s in shifts:
            o |= np.roll(m, s, axis=(0, 1, 2))
        return int(o.sum())
    E = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
    out = []
    for t in thresholds:
        m = w >= t
        n2 = sum(any_of(m, [(0, 0, 0), E[a]]) for a in range(3))
        n1 = 0
        for a in range(3):
            b, c = [E[i] for i in range(3) if i != a]
            n1 += any_of(m, [(0, 0, 0), b, c, tuple(p + q for p, q in zip(b, c))])
        out.append((any_of(m, list(itertools.product((0, 1), repeat=3))), n1, n2, int(m.sum())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--fields", default="grf,constant,cic")
    ap.add_argument("--thresholds", default="41,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-n", type=int, default=128, help="mesh of the NumPy timing (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        for kind in a.fields.split(","):
            x = make_field(kind, n, dev)
            for T in [int(v) for v in a.thresholds.split(",")]:
                for stdz in (True, False):
                    m_ms, c_ms = time_kernels(x, T, stdz, a.reps)
                    call = time_call(x, T, stdz, a.reps)
                    floor_us = 3 * 4.0 * n ** 3 / HBM * 1e6
                    row = dict(field=kind, n=n, T=T, standardize=stdz, moments_ms=m_ms, counts_ms=c_ms,
                               kernels_ms=m_ms + c_ms, call_ms=call, hbm_floor_us=floor_us,
                               counts_floor_us=floor_us / 3, kernels_over_floor=(m_ms + c_ms) * 1e3 / floor_us)
                    rows.append(row)
                    print("%-8s %4d^3 T=%4d std=%d: moments %7.3f ms, counts %7.3f ms, call %8.2f ms; "
                          "HBM floor %6.1f us (3 reads), kernels %.1fx the floor, counts pass %.1fx one read"
                          % (kind, n, T, stdz, m_ms, c_ms, call, floor_us, row["kernels_over_floor"],
                             c_ms * 1e3 / (floor_us / 3)), flush=True)
            del x
            torch.cuda.empty_cache()
    cpu = []
    if a.cpu_n:
        w = grf(a.cpu_n, 3, dev).cpu().numpy()
        thr = np.linspace(-3, 3, 41, dtype=np.float32)
        t0 = time.perf_counter()
        numpy_counts(w, thr)
        dt = time.perf_counter() - t0
        for n, T in ((512, 41), (512, 1024), (1024, 41)):
            ex = dt * (n / a.cpu_n) ** 3 * T / 41
            cpu.append(dict(n=a.cpu_n, T=41, seconds=dt, at_n=n, at_T=T, extrapolated_seconds=ex,
                            extrapolated="linear in n^3 T (not measured)"))
            print("numpy restatement %d^3 T=41: %.3f s measured; %d^3 T=%d extrapolated (unmeasured): %.1f s"
                  % (a.cpu_n, dt, n, T, ex), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(),
               lib=os.path.basename(_lib.LIB_PATH), rows=rows,
               numpy_cpu=cpu)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
