#!/usr/bin/env python
"""Time density.bispectrum, density.field_statistics and density.field_pdf on one MI355X: n^3 fields (default 256^3,
512^3, 1024^3), the reference's two configurations (k1 = k2 = 0.1 and k1 = 0.05, k2 = 0.1 h/Mpc in a 1000 Mpc/h box,
theta = linspace(0, pi, 25)), for two fields made on the device:

  grf   Gaussian random field (P(k) ~ k^-1.5 exp(-(k R)^2), R = 4 cells)
  cic   the CIC-painted, deconvolved delta of a Zel'dovich-like displacement of min(n, 512)^3 particles

Per case: the whole call (host clock, NumPy results back) and, by HIP events inside the call, the rfftn, the shell filter
(nbe_shell_filter), the batched irfftn, the triple sums (nbe_triple_sums) and the integer triangle count
(nbe_triangle_counts); the bytes the two bandwidth-shaped kernels move over their time against the achievable 6.3 TB/s;
the shell batch the planner took.  The exact integer triangle counts are compared with the float64 estimate
n^6 sum_x G1 G2 G3 from complex128 transforms of the shell indicators on the device at a few angles.  The one-point
calls are timed at the same sizes.  For comparison it times the float64 NumPy restatement (tests/bk_ref.py, FFT form)
at a CPU-sized mesh; anything derived from that for other sizes is marked "extrapolated, not measured".

    python tools/time_bispectrum.py --out profiles/bispectrum_timing_512.json
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, density as D  # noqa: E402
from time_minkowski import make_field  # noqa: E402

HBM = 6.3e12
L = 1000.0
CONFIGS = ((0.1, 0.1), (0.05, 0.1))
THETA = np.linspace(0.0, np.pi, 25)
PHASES = ("rfftn", "shell_filter", "irfftn", "triple_sums", "triangle_counts", "other")


def time_bispectrum(x, k1, k2, reps):
    n = int(x.shape[0])
    calls, phases = [], []
    out = None
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = D.bispectrum(x, L, k1, k2, THETA)
        dt = (time.perf_counter() - t0) * 1e3
        tm = {}
        D.bispectrum(x, L, k1, k2, THETA, _timings=tm)
        if r:
            calls.append(dt)
            phases.append(tm)
    med = {p: float(np.median([t.get(p, 0.0) for t in phases])) for p in PHASES}
    batch = int(phases[-1]["batch"])
    T = len(THETA)
    nbatches = 1 + -(-T // batch)
    half = 8.0 * n * n * (n // 2 + 1)
    filter_bytes = (nbatches + 2 + T) * half                       # the spectrum once per batch, every filtered spectrum
    groups = sum(-(-min(batch, T - t0) // 8) for t0 in range(0, T, batch))
    triple_bytes = (2 * groups + T) * 4.0 * n ** 3                  # F1 and F2 once per group of 8, every F3 once
    row = dict(n=n, k1=k1, k2=k2, T=T, call_ms=float(np.median(calls)), batch=batch, **{p + "_ms": med[p] for p in PHASES})
    row.update(filter_bytes=filter_bytes, triple_bytes=triple_bytes,
               filter_tb_s=filter_bytes / (med["shell_filter"] * 1e-3) / 1e12,
               triple_tb_s=triple_bytes / (med["triple_sums"] * 1e-3) / 1e12,
               filter_over_hbm=med["shell_filter"] * 1e-3 / (filter_bytes / HBM),
               triple_over_hbm=med["triple_sums"] * 1e-3 / (triple_bytes / HBM),
               kernels_over_transforms=(med["shell_filter"] + med["triple_sums"]) / (med["rfftn"] + med["irfftn"]),
               ntriangles_min=int(out["ntriangles"].min()), ntriangles_max=int(out["ntriangles"].max()))
    return row, out


def indicator_counts(n, k1, k2, picks, dev):
    """n^6 sum_x G1 G2 G3 at the angles `picks` through complex128 transforms of the shell indicators on the device."""
    kF = 2.0 * np.pi / L
    ka = np.concatenate([[k1 / kF, k2 / kF], D.bispectrum_kappa3(k1 / kF, k2 / kF, THETA[picks])])
    lo2, hi2 = D.bispectrum_shell_bounds(ka, 1.0)
    f = torch.fft.fftfreq(n, 1.0 / n, device=dev, dtype=torch.float64).round().to(torch.int64)
    fz = torch.arange(n // 2 + 1, device=dev, dtype=torch.int64)
    q = f[:, None, None] ** 2 + f[None, :, None] ** 2 + fz[None, None, :] ** 2

    def G(i):
        ind = ((q >= int(lo2[i])) & (q < int(hi2[i]))).to(torch.complex128)
        return torch.fft.irfftn(ind, s=(n, n, n))

    g12 = G(0) * G(1)
    return [float((g12 * G(2 + j)).sum()) * float(n) ** 6 for j in range(len(picks))]


def time_onepoint(x, reps):
    l = _lib.lib()
    dev = x.device
    s = D._stream(dev)
    count = x.numel()
    lo, hi = (float(v) for v in torch.aminmax(x))
    edges = D.pdf_edges(lo, hi, 120)
    ed = torch.from_numpy(edges).to(dev)
    mom = torch.empty(D._MOMENT4_WORDS, dtype=torch.float64, device=dev)
    cd = torch.zeros(122, dtype=torch.int64, device=dev)
    tm, th, c1, c2 = [], [], [], []
    for r in range(reps + 1):
        cd.zero_()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _lib.check(l.nbe_field_moments4(D._ptr(x), count, D._ptr(mom), s))
        e[1].record()
        _lib.check(l.nbe_field_histogram(D._ptr(x), count, lo, hi, D._ptr(ed), 120, D._ptr(cd), s))
        e[2].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.field_statistics(x)
        t1 = time.perf_counter()
        D.field_pdf(x, lo, hi, 120)
        t2 = time.perf_counter()
        if r:
            tm.append(e[0].elapsed_time(e[1]))
            th.append(e[1].elapsed_time(e[2]))
            c1.append((t1 - t0) * 1e3)
            c2.append((t2 - t1) * 1e3)
    assert int(cd[:120].sum()) == count
    read = 4.0 * count / HBM * 1e3
    return dict(moments4_ms=float(np.median(tm)), histogram_ms=float(np.median(th)), statistics_call_ms=float(np.median(c1)),
                pdf_call_ms=float(np.median(c2)), one_read_ms=read, top_bin_share=float(cd[:120].max()) / count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--fields", default="grf,cic")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=128, help="mesh of the NumPy timing (0: skip)")
    ap.add_argument("--onepoint-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows, onepoint, counts = [], [], []
    for n in [int(v) for v in a.sizes.split(",")]:
        for kind in a.fields.split(","):
            x = make_field(kind, n, dev)
            op = dict(field=kind, n=n, **time_onepoint(x, a.reps))
            onepoint.append(op)
            print("%-4s %4d^3 one-point: moments %7.3f ms (2 reads), histogram %7.3f ms (one read %.3f ms, top bin holds "
                  "%.0f %%); field_statistics %.2f ms, field_pdf %.2f ms"
                  % (kind, n, op["moments4_ms"], op["histogram_ms"], op["one_read_ms"], 100 * op["top_bin_share"],
                     op["statistics_call_ms"], op["pdf_call_ms"]), flush=True)
            if a.onepoint_only:
                continue
            for k1, k2 in CONFIGS:
                row, out = time_bispectrum(x, k1, k2, a.reps)
                row["field"] = kind
                rows.append(row)
                print("%-4s %4d^3 k1 %.2f k2 %.2f: call %8.2f ms; rfftn %7.2f, filter %7.2f (%.2f TB/s), irfftn %7.2f, "
                      "triple sums %7.2f (%.2f TB/s), triangle count %6.2f, other %6.2f ms; batch %d; kernels / "
                      "transforms %.2f; N_tri %d .. %d"
                      % (kind, n, k1, k2, row["call_ms"], row["rfftn_ms"], row["shell_filter_ms"], row["filter_tb_s"],
                         row["irfftn_ms"], row["triple_sums_ms"], row["triple_tb_s"], row["triangle_counts_ms"],
                         row["other_ms"], row["batch"], row["kernels_over_transforms"], row["ntriangles_min"],
                         row["ntriangles_max"]), flush=True)
                if kind == a.fields.split(",")[0]:
                    picks = np.array([0, 12, 23])
                    est = indicator_counts(n, k1, k2, picks, dev)
                    for p, e in zip(picks, est):
                        exact = int(out["ntriangles"][p])
                        counts.append(dict(n=n, k1=k1, k2=k2, theta_index=int(p), ntriangles=exact, float64_estimate=e,
                                           distance=abs(e - exact)))
                        print("     N_tri theta[%d]: %d exact; complex128 indicator estimate off by %.3g"
                              % (p, exact, abs(e - exact)), flush=True)
            del x
            torch.cuda.empty_cache()
    cpu = []
    if a.cpu_n and not a.onepoint_only:
        import bk_ref
        x = make_field("grf", a.cpu_n, dev).cpu().numpy()
        # k = 0.1 h/Mpc closes on a 128^3 mesh in a 250 Mpc/h box, not in this one: kappa = 3.98 (the cost does not depend on it)
        kappa = 0.1 * 250.0 / (2.0 * np.pi)
        t0 = time.perf_counter()
        bk_ref.fft_form(x, kappa, kappa, THETA, 1.0)
        dt = time.perf_counter() - t0
        for n in (512, 1024):
            cpu.append(dict(n=a.cpu_n, T=25, seconds=dt, at_n=n, extrapolated_seconds=dt * (n / a.cpu_n) ** 3,
                            extrapolated="extrapolated, not measured: linear in n^3, one thread"))
            print("numpy float64 restatement (FFT form) %d^3 T=25: %.2f s measured; %d^3: %.0f s extrapolated, not "
                  "measured" % (a.cpu_n, dt, n, dt * (n / a.cpu_n) ** 3), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), lib=os.path.basename(_lib.LIB_PATH),
               boxsize=L, rows=rows, onepoint=onepoint, triangle_counts=counts, numpy_cpu=cpu)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
