#!/usr/bin/env python
"""Time the input path (lpt.zeldovich_displacement, lpt.resize_density) on one MI355X.

Cases: zeldovich_displacement at 256^3, 512^3 and 1024^3; resize_density 256^3 -> 512^3 with every upsampling method and
512^3 -> 256^3 with every downsampling method, on a Gaussian field with a red spectrum in a 1000 Mpc/h box.

Per case, in one run: the whole call on a device tensor (HIP events, median of --reps after a warm-up call), and its
stages timed on their own: the rocFFT transforms through torch.fft, and every kernel of csrc/nbe_lpt.hip through the C
ABI.  Beside each kernel stands the time its bytes would take at the copy bandwidth of this device in this run: a
device-to-device copy_ of a buffer of half the kernel's traffic, which reads and writes as many bytes as the kernel
does.  For scale, the float64 NumPy restatement (tests/lpt_ref.py) is timed on the host at 128^3, labelled as such.

    python tools/time_lpt.py --out profiles/lpt_timing_512.json > profiles/lpt_timing_512.txt
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, lpt as T  # noqa: E402
from jax_nbody_emulator_with_dj_amd.density import _ptr, _stream  # noqa: E402

L = 1000.0


def event_ms(fn, reps):
    """Median HIP-event time of fn() over reps calls after one warm-up call."""
    times = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def copy_ms(nbytes, reps, dev):
    """A device-to-device copy_ of nbytes: reads nbytes and writes nbytes."""
    a = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    a.zero_()
    return event_ms(lambda: b.copy_(a), reps)


def red_field(n, seed, dev):
    """A Gaussian field with |delta_k| ~ 1 / |m|, unit variance, made on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    w = torch.fft.rfftn(torch.randn((n, n, n), generator=g, device=dev))
    m = torch.fft.fftfreq(n, 1.0 / n, device=dev)
    q = m[:, None, None] ** 2 + m[None, :, None] ** 2 + m[None, None, :n // 2 + 1] ** 2
    x = torch.fft.irfftn(w / torch.sqrt(torch.clamp(q, min=1.0)), s=(n, n, n))
    return (x / x.std()).contiguous()


def kernel_row(name, fn, traffic_bytes, reps, dev):
    ms = event_ms(fn, reps)
    at_copy = copy_ms(traffic_bytes // 2, reps, dev)
    return dict(stage=name, kind="kernel", ms=ms, traffic_bytes=int(traffic_bytes), copy_ms=at_copy, ratio=ms / at_copy)


def fft_row(name, fn, reps):
    return dict(stage=name, kind="rocFFT", ms=event_ms(fn, reps))


def spec_bytes(n, count=1):
    return 8 * count * n * n * (n // 2 + 1)


def zeldovich_case(n, reps, dev):
    l = _lib.lib()
    x = red_field(n, n, dev)
    row = dict(case="zeldovich_displacement", n=n, call_ms=event_ms(lambda: T.zeldovich_displacement(x, L), reps))
    spec = T._half_spectrum(x)
    psi_k = T._empty_spectrum(n, dev, (3,))
    s = _stream(dev)
    stages = [fft_row("rfftn", lambda: torch.fft.rfftn(x), reps),
              kernel_row("nbe_zeldovich_spectrum",
                         lambda: _lib.check(l.nbe_zeldovich_spectrum(_ptr(spec), n, L, 1.0, _ptr(psi_k), s)),
                         spec_bytes(n, 4), reps, dev),
              fft_row("irfftn x3 (batched)", lambda: torch.fft.irfftn(psi_k, s=(n, n, n), dim=(1, 2, 3)), reps)]
    row["stages"] = stages
    return row


def resize_case(n_in, n_out, method, table, reps, dev):
    l = _lib.lib()
    x = red_field(n_in, n_in + n_out, dev)
    up = n_out > n_in
    kw = dict(boxsize=L, upsample_method=method if up else "fourier", downsample_method="gaussian" if up else method)
    if method == "mode_inject":
        kw.update(k_target=table[0], pk_target=table[1], seed=1)
    row = dict(case="resize_density", n_in=n_in, n_out=n_out, method=method,
               call_ms=event_ms(lambda: T.resize_density(x, n_out, **kw), reps))
    s = _stream(dev)
    stages = []
    if method in ("fourier", "mode_inject"):
        spec = T._half_spectrum(x)
        out = T._empty_spectrum(n_out, dev)
        stages.append(fft_row("rfftn %d^3" % n_in, lambda: torch.fft.rfftn(x), reps))
        if method == "fourier":
            # upwards only the modes of the source band are read; downwards only those of the destination band
            traffic = spec_bytes(n_out) + spec_bytes(min(n_in, n_out))
            stages.append(kernel_row("nbe_spectrum_resize",
                                     lambda: _lib.check(l.nbe_spectrum_resize(_ptr(spec), n_in, _ptr(out), n_out, 0, s)),
                                     traffic, reps, dev))
        else:
            kd, pd = torch.from_numpy(table[0]).to(dev), torch.from_numpy(table[1]).to(dev)
            stages.append(kernel_row("nbe_spectrum_inject",
                                     lambda: _lib.check(l.nbe_spectrum_inject(_ptr(spec), n_in, _ptr(out), n_out, _ptr(kd),
                                                                              _ptr(pd), int(table[0].size), table[2],
                                                                              table[3], L, 1, s)),
                                     spec_bytes(n_out) + spec_bytes(n_in), reps, dev))
        stages.append(fft_row("irfftn %d^3" % n_out, lambda: torch.fft.irfftn(out, s=(n_out,) * 3), reps))
    elif method == "linear":
        out = torch.empty((n_out,) * 3, dtype=torch.float32, device=dev)
        stages.append(kernel_row("nbe_trilinear_upsample",
                                 lambda: _lib.check(l.nbe_trilinear_upsample(_ptr(x), n_in, _ptr(out), n_out, s)),
                                 4 * (n_in ** 3 + n_out ** 3), reps, dev))
    else:
        if method == "gaussian":
            spec = T._half_spectrum(x)
            stages.append(fft_row("rfftn %d^3" % n_in, lambda: torch.fft.rfftn(x), reps))
            stages.append(kernel_row("nbe_gaussian_filter",
                                     lambda: _lib.check(l.nbe_gaussian_filter(_ptr(spec), n_in, 1.0 / n_out, s)),
                                     2 * spec_bytes(n_in), reps, dev))
            stages.append(fft_row("irfftn %d^3" % n_in, lambda: torch.fft.irfftn(spec, s=(n_in,) * 3), reps))
        out = torch.empty((n_out,) * 3, dtype=torch.float32, device=dev)
        stages.append(kernel_row("nbe_block_average",
                                 lambda: _lib.check(l.nbe_block_average(_ptr(x), n_in, _ptr(out), n_out, s)),
                                 4 * (n_in ** 3 + n_out ** 3), reps, dev))
    row["stages"] = stages
    return row


def host_restatement(n):
    """Seconds of the float64 NumPy restatement on the host CPU, for scale only."""
    import lpt_ref as R
    x = R.red_field(n, 1)
    out = {}
    for name, fn in (("zeldovich_displacement", lambda: R.zeldovich_displacement(x, L)),
                     ("gaussian_smooth", lambda: R.gaussian_smooth(x, L, 8.0)),
                     ("block_average to n/2", lambda: R.block_average(x, n // 2))):
        t0 = time.perf_counter()
        fn()
        out[name] = time.perf_counter() - t0
    return out


def show(row):
    head = ("zeldovich_displacement %d^3" % row["n"]) if row["case"] == "zeldovich_displacement" else \
        "resize_density %d^3 -> %d^3 %s" % (row["n_in"], row["n_out"], row["method"])
    fft = sum(s["ms"] for s in row["stages"] if s["kind"] == "rocFFT")
    ker = sum(s["ms"] for s in row["stages"] if s["kind"] == "kernel")
    print("%-46s call %9.3f ms; stages alone: rocFFT %9.3f ms, kernels %8.3f ms" % (head, row["call_ms"], fft, ker))
    for s in row["stages"]:
        if s["kind"] == "kernel":
            print("    %-28s %9.3f ms; %6.2f GB at copy bandwidth %9.3f ms (%.2f x)"
                  % (s["stage"], s["ms"], s["traffic_bytes"] / 1e9, s["copy_ms"], s["ratio"]))
        else:
            print("    %-28s %9.3f ms (rocFFT)" % (s["stage"], s["ms"]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zeldovich", default="256,512,1024")
    ap.add_argument("--coarse", type=int, default=256)
    ap.add_argument("--fine", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-n", type=int, default=128, dest="host_n")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    k = np.geomspace(np.pi / L, 0.7 * np.pi * a.fine / L, 256)
    table = T._validate_table(k, 2.0e4 * (k / 0.1) ** -1.7)
    rows = []
    big = 1 << 30
    rows_copy = copy_ms(big, a.reps, dev)
    print("device-to-device copy_ of 1 GiB: %.3f ms = %.2f TB/s of traffic (read + write)"
          % (rows_copy, 2 * big / rows_copy / 1e9))
    for n in [int(v) for v in a.zeldovich.split(",") if v]:
        rows.append(zeldovich_case(n, a.reps, dev))
        show(rows[-1])
        torch.cuda.empty_cache()
    for method in T.UPSAMPLE_METHODS:
        rows.append(resize_case(a.coarse, a.fine, method, table, a.reps, dev))
        show(rows[-1])
    for method in T.DOWNSAMPLE_METHODS:
        rows.append(resize_case(a.fine, a.coarse, method, table, a.reps, dev))
        show(rows[-1])
    host = host_restatement(a.host_n)
    for name, sec in host.items():
        print("host CPU, float64 NumPy restatement at %d^3 (for scale only): %-24s %8.3f s" % (a.host_n, name, sec))
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps,
               copy_1gib_ms=rows_copy, rows=rows, host_restatement=dict(n=a.host_n, seconds=host))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
