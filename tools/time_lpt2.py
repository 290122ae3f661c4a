#!/usr/bin/env python
"""Time second-order LPT (lpt.lpt2_displacement) on one MI355X.

Cases: lpt2_displacement at 256^3, 512^3 and 1024^3, without and with dealiasing (the source on the mesh of 3 n / 2), on
a Gaussian field with a red spectrum in a 1000 Mpc/h box, and zeldovich_displacement on the same field in the same run.

Per size: the whole calls on a device tensor (HIP events, median of --reps after a warm-up call), the rocFFT transforms
alone through torch.fft, and each kernel the call runs through the C ABI.  Beside each kernel stands a device-to-device
copy_ of half the kernel's traffic, which reads and writes as many bytes as the kernel does.  A case that does not fit
the device's memory is recorded as such.

    python tools/time_lpt2.py --out profiles/lpt2_timing_512.json > profiles/lpt2_timing_512.txt

--first-order times zeldovich_displacement and linear_ics(order=1) alone and prints one line each with --label in front;
it also runs on a library from before second order (NBE_LIB), which is how profiles/lpt2_zeldovich_ab.txt was made.
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, lpt as T  # noqa: E402
from jax_nbody_emulator_with_dj_amd.density import _ptr, _stream  # noqa: E402
from time_lpt import L, copy_ms, event_ms, fft_row, kernel_row, red_field, spec_bytes  # noqa: E402


def call_ms(fn, reps):
    """event_ms, or the reason the call cannot run (memory)."""
    try:
        return event_ms(fn, reps), None
    except (_lib.NBEError, torch.cuda.OutOfMemoryError) as e:
        torch.cuda.empty_cache()
        return None, str(e).splitlines()[0]


def kernels_and_transforms(n, p, x, reps, dev):
    """The stages of lpt2_displacement at n with the source on the p^3 mesh, each alone."""
    l = _lib.lib()
    s = _stream(dev)
    spec = T._half_spectrum(x)
    hk = T._empty_spectrum(n, dev, (6,))
    psi_k = T._empty_spectrum(n, dev, (3,))
    stages = [fft_row("rfftn %d^3" % n, lambda: torch.fft.rfftn(x), reps),
              kernel_row("nbe_lpt2_hessian_spectrum",
                         lambda: _lib.check(l.nbe_lpt2_hessian_spectrum(_ptr(spec), n, 0, 6, _ptr(hk), 0, s)),
                         spec_bytes(n, 7), reps, dev)]
    if p != n:
        up = T._empty_spectrum(p, dev)
        stages.append(kernel_row("nbe_spectrum_resize %d -> %d" % (n, p),
                                 lambda: _lib.check(l.nbe_spectrum_resize(_ptr(hk[0]), n, _ptr(up), p, 0, s)),
                                 spec_bytes(p) + spec_bytes(n), reps, dev))
        stages.append(fft_row("irfftn %d^3 (one of six)" % p,
                              lambda: torch.fft.irfftn(up[None], s=(p, p, p), dim=(1, 2, 3)), reps))
        del up
    else:
        stages.append(fft_row("irfftn %d^3 x6 (batched)" % n,
                              lambda: torch.fft.irfftn(hk, s=(n, n, n), dim=(1, 2, 3)), reps))
    del hk
    hess = torch.randn((6, p, p, p), dtype=torch.float32, device=dev)
    out = torch.empty((p, p, p), dtype=torch.float32, device=dev)
    stages.append(kernel_row("nbe_lpt2_source %d^3" % p,
                             lambda: _lib.check(l.nbe_lpt2_source(_ptr(hess), p, _ptr(out), 0, s)),
                             7 * 4 * p ** 3, reps, dev))
    del hess
    stages.append(fft_row("rfftn %d^3" % p, lambda: torch.fft.rfftn(out), reps))
    if p != n:
        s_p = T._half_spectrum(out)
        down = T._empty_spectrum(n, dev)
        stages.append(kernel_row("nbe_spectrum_resize %d -> %d" % (p, n),
                                 lambda: _lib.check(l.nbe_spectrum_resize(_ptr(s_p), p, _ptr(down), n, 0, s)),
                                 2 * spec_bytes(n), reps, dev))
        del s_p, down
    del out
    s_k = spec.clone()
    stages.append(kernel_row("nbe_lpt2_spectrum",
                             lambda: _lib.check(l.nbe_lpt2_spectrum(_ptr(spec), _ptr(s_k), n, L, 1.0, 3.0 / 7.0, _ptr(psi_k),
                                                                    0, s)),
                             spec_bytes(n, 5), reps, dev))
    stages.append(fft_row("irfftn %d^3 x3 (batched)" % n,
                          lambda: torch.fft.irfftn(psi_k, s=(n, n, n), dim=(1, 2, 3)), reps))
    return stages


def size_case(n, reps, dev):
    x = red_field(n, n, dev)
    row = dict(n=n, zeldovich_ms=event_ms(lambda: T.zeldovich_displacement(x, L), reps), cases=[])
    for dealias in (False, True):
        p = 3 * n // 2 if dealias else n
        if p > T.MAX_N:
            row["cases"].append(dict(dealias=dealias, p=p, call_ms=None, why="3 n / 2 = %d is above %d" % (p, T.MAX_N)))
            continue
        ms, why = call_ms(lambda: T.lpt2_displacement(x, L, dealias=dealias), reps)
        case = dict(dealias=dealias, p=p, call_ms=ms, why=why)
        torch.cuda.empty_cache()
        if ms is not None:
            case["stages"] = kernels_and_transforms(n, p, x, reps, dev)
        row["cases"].append(case)
        torch.cuda.empty_cache()
    return row


def show(row):
    n = row["n"]
    print("zeldovich_displacement %d^3: call %9.3f ms" % (n, row["zeldovich_ms"]))
    for c in row["cases"]:
        head = "lpt2_displacement %d^3%s" % (n, ", dealias (source at %d^3)" % c["p"] if c["dealias"] else "")
        if c["call_ms"] is None:
            print("%s: does not run: %s" % (head, c["why"]))
            continue
        fft = sum(s["ms"] for s in c["stages"] if s["kind"] == "rocFFT")
        ker = sum(s["ms"] for s in c["stages"] if s["kind"] == "kernel")
        print("%s: call %9.3f ms (%.2f x zeldovich_displacement); stages below, each once: rocFFT %9.3f ms, kernels %8.3f ms"
              % (head, c["call_ms"], c["call_ms"] / row["zeldovich_ms"], fft, ker))
        for s in c["stages"]:
            if s["kind"] == "kernel":
                print("    %-34s %9.3f ms; %6.2f GB at copy bandwidth %9.3f ms (%.2f x)"
                      % (s["stage"], s["ms"], s["traffic_bytes"] / 1e9, s["copy_ms"], s["ratio"]))
            else:
                print("    %-34s %9.3f ms (rocFFT)" % (s["stage"], s["ms"]))
    sys.stdout.flush()


def first_order(sizes, reps, dev, label):
    """zeldovich_displacement and linear_ics(order=1), which second order must not move: one line a case."""
    k = np.geomspace(np.pi / L, 0.7 * np.pi * max(sizes) / L, 256)
    pk = 2.0e4 * (k / 0.1) ** -1.7
    for n in sizes:
        x = red_field(n, n, dev)
        z = event_ms(lambda: T.zeldovich_displacement(x, L), reps)
        del x
        torch.cuda.empty_cache()
        ics = event_ms(lambda: T.linear_ics(n, L, k, pk, 7), reps)
        torch.cuda.empty_cache()
        print("%s: %4d^3: zeldovich_displacement %9.3f ms, linear_ics(order=1) %9.3f ms" % (label, n, z, ics))
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--first-order", action="store_true", dest="first_order")
    ap.add_argument("--label", default="run")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sizes = [int(v) for v in a.sizes.split(",") if v]
    if a.first_order:
        if os.environ.get("NBE_LIB"):                       # a library from before second order has no such symbols
            for name in [s for s in _lib.SIGNATURES if s.startswith("nbe_lpt2_")]:
                del _lib.SIGNATURES[name]
        first_order(sizes, a.reps, dev, a.label)
        return
    big = 1 << 30
    rows_copy = copy_ms(big, a.reps, dev)
    print("device-to-device copy_ of 1 GiB: %.3f ms = %.2f TB/s of traffic (read + write)"
          % (rows_copy, 2 * big / rows_copy / 1e9))
    rows = []
    for n in sizes:
        rows.append(size_case(n, a.reps, dev))
        show(rows[-1])
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, copy_1gib_ms=rows_copy,
               rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
