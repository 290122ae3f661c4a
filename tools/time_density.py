#!/usr/bin/env python
"""Time density.paint_density on one MI355X: N^3 particles (default 512^3) painted into 256^3, 512^3 and 1024^3 meshes
with NGP / CIC / TSC / PCS, with and without the window deconvolution, for two displacement fields made on the device
with torch.fft:

  realistic   Zel'dovich-like displacement of a Gaussian random field (P(k) ~ k^-1.5 exp(-(k R)^2), R = 2 Mpc/h),
              3-D rms 6 Mpc/h in a 1000 Mpc/h box
  clustered   the same field times 3 (3-D rms 18 Mpc/h): strong shell crossing, dense caustics, larger tile spreads

Per case: the paint kernel alone (HIP events around nbe_paint_mesh), the whole paint_density call with and without
deconvolution, the 64-bit atomic adds into the mesh (counted in a separate run) and the rate of added bytes, and the share
of 8^3-particle tiles whose footprint did not fit LDS (direct global-atomic path).  For comparison it times a NumPy float64
np.add.at painting at a CPU-sized lattice and extrapolates linearly in particles x contributions.

    python tools/time_density.py --out profiles/density_timing.json
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

import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, density as D  # noqa: E402


def gaussian_displacement(n, L, rms3d, seed, dev):
    """(3, n, n, n) float32 displacement psi_k = i k / k^2 delta_k of a Gaussian field, scaled to a 3-D rms of rms3d."""
    g = torch.Generator(device=dev).manual_seed(seed)
    white = torch.randn((n, n, n), generator=g, device=dev, dtype=torch.float32)
    dk = torch.fft.rfftn(white)
    kF = 2 * np.pi / L
    f = torch.fft.fftfreq(n, d=1.0 / n, device=dev) * kF
    fz = torch.fft.rfftfreq(n, d=1.0 / n, device=dev) * kF
    kx, ky, kz = f[:, None, None], f[None, :, None], fz[None, None, :]
    k2 = kx * kx + ky * ky + kz * kz
    k2[0, 0, 0] = 1.0
    amp = k2.pow(-0.375) * torch.exp(-k2 * 4.0 / 2)          # sqrt(P), P ~ k^-1.5 exp(-k^2 R^2), R = 2 Mpc/h
    amp[0, 0, 0] = 0.0
    dk = dk * amp
    out = torch.empty((3, n, n, n), device=dev, dtype=torch.float32)
    for c, kc in enumerate((kx, ky, kz)):
        out[c] = torch.fft.irfftn(1j * kc / k2 * dk, s=(n, n, n))
    out *= rms3d / float(out.pow(2).sum(0).mean().sqrt())
    return out.contiguous()


def time_paint_kernel(x, L, res, worder, reps):
    """ms of nbe_paint_mesh alone (median of reps) and (direct tiles, total tiles, atomic adds)."""
    l = _lib.lib()
    dev = x.device
    n = tuple(int(v) for v in x.shape[1:])
    mesh = torch.zeros((res,) * 3, dtype=torch.int64, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    s = D._stream(dev)
    args = lambda count: (D._ptr(x), 0, D._i64(n), (C.c_double * 3)(L, L, L), D._i64((res,) * 3), worder, count,
                          D._ptr(mesh), D._ptr(stats), s)
    times = []
    for r in range(reps + 1):
        mesh.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(l.nbe_paint_mesh(*args(0)))
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    stats.zero_()
    mesh.zero_()
    _lib.check(l.nbe_paint_mesh(*args(1)))
    torch.cuda.synchronize()
    st = stats.cpu()
    atomics = int(st[2:4].view(torch.int64)[0])
    tiles = int(np.prod([(v + 7) // 8 for v in n]))
    assert int(mesh.sum()) == n[0] * n[1] * n[2] * (1 << 22), "mass not conserved"
    del mesh
    return float(np.median(times)), int(st[0]), tiles, atomics


def time_call(x, L, res, worder, deconvolve, reps):
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.paint_density(x, L, res, worder, deconvolve=deconvolve)
        torch.cuda.synchronize()
        if r:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def numpy_paint(disp, L, res, p):
    """float64 np.add.at painting (the CPU route the density module replaces)."""
    n = disp.shape[1]
    u = [(np.indices((n,) * 3)[c].ravel() * (res / n) + disp[c].ravel().astype(np.float64) * (res / L)) for c in range(3)]
    j0 = [np.floor(uc + 1.0 - 0.5 * p).astype(np.int64) for uc in u]
    mesh = np.zeros((res,) * 3)
    for a in range(p):
        for b in range(p):
            for c in range(p):
                w = np.ones_like(u[0])
                for ax, t in enumerate((a, b, c)):
                    x = np.abs(u[ax] - (j0[ax] + t))
                    w = w * {1: np.ones_like(x), 2: 1 - x,
                             3: np.where(x < 0.5, 0.75 - x * x, 0.5 * (1.5 - x) ** 2),
                             4: np.where(x < 1, (4 - 6 * x * x + 3 * x ** 3) / 6, (2 - x) ** 3 / 6)}[p]
                np.add.at(mesh, (np.mod(j0[0] + a, res), np.mod(j0[1] + b, res), np.mod(j0[2] + c, res)), w)
    return mesh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--res", default="256,512,1024")
    ap.add_argument("--worders", default="1,2,3,4")
    ap.add_argument("--boxsize", type=float, default=1000.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=64, help="lattice of the NumPy timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = a.boxsize
    res_list = [int(v) for v in a.res.split(",")]
    worders = [int(v) for v in a.worders.split(",")]
    base = gaussian_displacement(a.n, L, 6.0, 1, dev)
    rows = []
    for case, scale in (("realistic", 1.0), ("clustered", 3.0)):
        x = (base * scale).contiguous()
        for res in res_list:
            for p in worders:
                k_ms, direct, tiles, atomics = time_paint_kernel(x, L, res, p, a.reps)
                row = dict(case=case, rms3d_mpc_h=6.0 * scale, n=a.n, res=res, worder=p, mas=D.WORDERS[p],
                           paint_kernel_ms=k_ms, paint_density_ms=time_call(x, L, res, p, False, a.reps),
                           paint_density_deconv_ms=time_call(x, L, res, p, True, a.reps),
                           atomic_adds=atomics, atomic_bytes_per_s=atomics * 8 / (k_ms * 1e-3),
                           direct_tile_share=direct / tiles)
                rows.append(row)
                print("%-9s %4d^3 -> %4d^3 %s: kernel %8.2f ms, paint %8.2f ms, +deconv %8.2f ms, %.3g atomics "
                      "(%.2f TB/s of added bytes), direct tiles %.2f %%"
                      % (case, a.n, res, D.WORDERS[p], k_ms, row["paint_density_ms"], row["paint_density_deconv_ms"],
                         atomics, row["atomic_bytes_per_s"] / 1e12, 100 * row["direct_tile_share"]), flush=True)
        del x
    # NumPy float64 reference at a CPU-sized lattice, extrapolated in particles x contributions
    cpu = []
    small = gaussian_displacement(a.cpu_n, L, 6.0, 2, dev).cpu().numpy()
    for p in (2, 4):
        t0 = time.perf_counter()
        numpy_paint(small, L, a.cpu_n, p)
        dt = time.perf_counter() - t0
        extrap = dt * (a.n / a.cpu_n) ** 3
        cpu.append(dict(worder=p, mas=D.WORDERS[p], n=a.cpu_n, res=a.cpu_n, seconds=dt,
                        extrapolated_seconds_at_n=extrap, extrapolated="linear in particles (not measured)"))
        print("numpy np.add.at %s %d^3 -> %d^3: %.3f s measured; %d^3 extrapolated (unmeasured): %.1f s"
              % (D.WORDERS[p], a.cpu_n, a.cpu_n, dt, a.n, extrap), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), rows=rows, numpy_cpu=cpu)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
