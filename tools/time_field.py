#!/usr/bin/env python
"""Time density.paint_field and the line-of-sight shift of density.paint_density on one MI355X, with the fields of
tools/time_density.py: N^3 particles (default 512^3) with a 3-D rms displacement of 6 Mpc/h (realistic) and 18 Mpc/h
(clustered) in a 1000 Mpc/h box, painted into 256^3, 512^3 and 1024^3 meshes with NGP / CIC / TSC / PCS.  The quantity
is a second Gaussian field of three components with an rms of 300 per component (a velocity in km/s).

Per case, in one run: paint_density as it was (the comparison), paint_density with a shift along axis 2, paint_field with
C = 1 and C = 3 ("density") and C = 3 ("mean"); every number is the median wall time of whole calls on tensors (allocation,
range pass and conversion included) after one warm-up call.  Also nbe_paint_fields alone (HIP events) for C = 0, 1 and 3,
the share of 8^3-particle tiles on the direct path, and the ratio of a C = 3 call to four paint_density calls.

    python tools/time_field.py --out profiles/field_timing_512.json
"""

import argparse
import ctypes as C
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


def wall_ms(fn, reps):
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def kernel_ms(x, q, v, L, res, worder, reps):
    """ms of nbe_paint_fields alone (median of reps) for the channels of q (None: masses only, shifted by v), and the
    tiles on the direct path."""
    l = _lib.lib()
    dev = x.device
    n = tuple(int(d) for d in x.shape[1:])
    nchan = 0 if q is None else int(q.shape[0])
    mesh = torch.zeros((res,) * 3, dtype=torch.int64, device=dev)
    qmesh = torch.zeros((max(nchan, 1),) + (res,) * 3, dtype=torch.int64, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    exps = (C.c_int * 4)(*([int(np.frexp(float(q.abs().max()))[1]) if nchan else 0] * 4))   # one exponent fits all
    s = D._stream(dev)
    times = []
    for r in range(reps + 1):
        mesh.zero_()
        qmesh.zero_()
        stats.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(l.nbe_paint_fields(D._ptr(x), 0, D._ptr(q) if nchan else None, 0, nchan, exps,
                                      D._ptr(v) if v is not None else None, 0, 2, 0.01, D._i64(n),
                                      (C.c_double * 3)(L, L, L), D._i64((res,) * 3), worder, D._ptr(mesh),
                                      D._ptr(qmesh) if nchan else None, D._ptr(stats), s))
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    assert int(mesh.sum()) == n[0] * n[1] * n[2] * (1 << 22), "mass not conserved"
    return float(np.median(times)), int(stats[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--res", default="256,512,1024")
    ap.add_argument("--worders", default="1,2,3,4")
    ap.add_argument("--boxsize", type=float, default=1000.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = a.boxsize
    res_list = [int(v) for v in a.res.split(",")]
    worders = [int(v) for v in a.worders.split(",")]
    base = gaussian_displacement(a.n, L, 6.0, 1, dev)
    vel = gaussian_displacement(a.n, L, 300.0 * np.sqrt(3.0), 3, dev)
    tiles = ((a.n + 7) // 8) ** 3
    rows = []
    for case, scale in (("realistic", 1.0), ("clustered", 3.0)):
        x = (base * scale).contiguous()
        for res in res_list:
            for p in worders:
                row = dict(case=case, rms3d_mpc_h=6.0 * scale, n=a.n, res=res, worder=p, mas=D.WORDERS[p])
                row["paint_density_ms"] = wall_ms(lambda: D.paint_density(x, L, res, p, deconvolve=False), a.reps)
                row["paint_density_shift_ms"] = wall_ms(
                    lambda: D.paint_density(x, L, res, p, deconvolve=False, velocity=vel, los=2, velocity_to_length=0.01),
                    a.reps)
                row["paint_field_c1_density_ms"] = wall_ms(lambda: D.paint_field(x, vel[2], L, res, p), a.reps)
                row["paint_field_c3_density_ms"] = wall_ms(lambda: D.paint_field(x, vel, L, res, p), a.reps)
                row["paint_field_c3_mean_ms"] = wall_ms(lambda: D.paint_field(x, vel, L, res, p, normalize="mean"), a.reps)
                row["kernel_c0_shift_ms"], direct_shift = kernel_ms(x, None, vel[2].contiguous(), L, res, p, a.reps)
                row["kernel_c1_ms"], _ = kernel_ms(x, vel[2:3].contiguous(), None, L, res, p, a.reps)
                row["kernel_c3_ms"], direct = kernel_ms(x, vel, None, L, res, p, a.reps)
                row["direct_tile_share"] = direct / tiles
                row["direct_tile_share_shift"] = direct_shift / tiles
                row["c3_over_four_paints"] = row["paint_field_c3_density_ms"] / (4.0 * row["paint_density_ms"])
                rows.append(row)
                print("%-9s %4d^3 -> %4d^3 %s: paint_density %7.2f ms, shifted %7.2f ms, field C=1 %7.2f ms, C=3 %7.2f ms "
                      "(mean %7.2f ms) = %.2f x four paints; kernel C=0/1/3 %7.2f / %7.2f / %7.2f ms, direct tiles %.2f %%"
                      % (case, a.n, res, D.WORDERS[p], row["paint_density_ms"], row["paint_density_shift_ms"],
                         row["paint_field_c1_density_ms"], row["paint_field_c3_density_ms"], row["paint_field_c3_mean_ms"],
                         row["c3_over_four_paints"], row["kernel_c0_shift_ms"], row["kernel_c1_ms"], row["kernel_c3_ms"],
                         100 * row["direct_tile_share"]), flush=True)
        del x
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
