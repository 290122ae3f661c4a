#!/usr/bin/env python
"""Time the anisotropic two-point calls (density.power_spectrum_multipoles, density.power_spectrum_wedges,
lpt.divergence) on one MI355X.

At 256^3, 512^3 and 1024^3, on a Gaussian field with a red spectrum in a 1000 Mpc/h box, in one run:

- the whole calls on a device tensor (HIP events, median of --reps after a warm-up call): power_spectrum, whose code this
  work does not touch, so its figure is the parent's, then power_spectrum_multipoles, power_spectrum_wedges(nmu=5) and
  divergence, each with its ratio to power_spectrum;
- the rocFFT rfftn on its own;
- every entry point on its own through the C ABI, beside a device-to-device copy_ of the bytes it reads.  The shell-sum
  entry points read the spectrum once per pass (the max pass, then one sum pass per chunk of mu bins) and write a few
  kilobytes; nbe_power_spectrum stands beside them for scale.  nbe_divergence_spectrum reads three spectra and writes one.

    python tools/time_aniso.py --out profiles/aniso_timing_512.json > profiles/aniso_timing_512.txt
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, density as D, lpt as T  # noqa: E402
from jax_nbody_emulator_with_dj_amd.density import _ptr, _stream  # noqa: E402
from time_lpt import copy_ms, event_ms, red_field, spec_bytes  # noqa: E402

L = 1000.0
NMU = 5
LDS_BYTES = 65536                           # csrc/nbe_density.hip, nbe_power_wedges: the image of one launch


def wedge_launches(n, nmu):
    nb = n // 2 + 1
    per = ((LDS_BYTES - 4 * nb) // 32) // nb
    return -(-nmu // per)


def kernel_row(name, fn, passes, read_bytes, reps, dev):
    ms = event_ms(fn, reps)
    at_copy = copy_ms(read_bytes, reps, dev)
    return dict(stage=name, passes=passes, ms=ms, read_bytes=int(read_bytes), copy_ms=at_copy, ratio=ms / at_copy)


def case(n, reps, dev):
    l = _lib.lib()
    x = red_field(n, n, dev)
    v = torch.stack([red_field(n, n + c, dev) for c in (1, 2, 3)]).contiguous()
    calls = dict(power_spectrum=event_ms(lambda: D.power_spectrum(x, L), reps),
                 power_spectrum_multipoles=event_ms(lambda: D.power_spectrum_multipoles(x, L, los=2), reps),
                 power_spectrum_wedges=event_ms(lambda: D.power_spectrum_wedges(x, L, los=2, nmu=NMU), reps),
                 divergence=event_ms(lambda: T.divergence(v, L), reps))
    row = dict(n=n, nmu=NMU, call_ms=calls, call_ratio={k: t / calls["power_spectrum"] for k, t in calls.items()},
               rfftn_ms=event_ms(lambda: torch.fft.rfftn(x), reps))
    s = _stream(dev)
    nb = n // 2 + 1
    a = T._half_spectrum(x)
    binmax = torch.zeros(nb, dtype=torch.int32, device=dev)
    sums = torch.zeros(4 * NMU * nb, dtype=torch.int64, device=dev)      # sums only grow: the time does not depend on them
    launches = wedge_launches(n, NMU)
    stages = [kernel_row("nbe_power_spectrum", lambda: _lib.check(l.nbe_power_spectrum(
                  _ptr(a), None, n, _ptr(binmax), _ptr(sums), s)), 2, 2 * spec_bytes(n), reps, dev),
              kernel_row("nbe_power_multipoles", lambda: _lib.check(l.nbe_power_multipoles(
                  _ptr(a), None, n, 2, _ptr(binmax), _ptr(sums), s)), 2, 2 * spec_bytes(n), reps, dev),
              kernel_row("nbe_power_wedges", lambda: _lib.check(l.nbe_power_wedges(
                  _ptr(a), None, n, 2, NMU, 0, _ptr(binmax), _ptr(sums), s)), 1 + launches, (1 + launches) * spec_bytes(n),
                  reps, dev)]
    del a, binmax, sums
    spec = torch.fft.rfftn(v, dim=(1, 2, 3)).contiguous()
    out = T._empty_spectrum(n, dev)
    stages.append(kernel_row("nbe_divergence_spectrum", lambda: _lib.check(l.nbe_divergence_spectrum(
        _ptr(spec), n, L, _ptr(out), s)), 1, spec_bytes(n, 3), reps, dev))
    row["stages"] = stages
    return row


def show(row):
    c, r = row["call_ms"], row["call_ratio"]
    print("%d^3: power_spectrum %9.3f ms (rfftn alone %9.3f ms)" % (row["n"], c["power_spectrum"], row["rfftn_ms"]))
    for name in ("power_spectrum_multipoles", "power_spectrum_wedges", "divergence"):
        print("    %-34s %9.3f ms = %5.2f x power_spectrum"
              % (name + ("(nmu=%d)" % row["nmu"] if name.endswith("wedges") else ""), c[name], r[name]))
    for s in row["stages"]:
        print("    %-26s %9.3f ms, %2d pass%s; copy_ of the %6.2f GB it reads %9.3f ms (%.2f x)"
              % (s["stage"], s["ms"], s["passes"], "" if s["passes"] == 1 else "es", s["read_bytes"] / 1e9, s["copy_ms"],
                 s["ratio"]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    big = 1 << 30
    one = copy_ms(big, a.reps, dev)
    print("device-to-device copy_ of 1 GiB: %.3f ms = %.2f TB/s of traffic (read + write)" % (one, 2 * big / one / 1e9))
    rows = []
    for n in [int(v) for v in a.sizes.split(",") if v]:
        rows.append(case(n, a.reps, dev))
        show(rows[-1])
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, copy_1gib_ms=one,
               rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
