#!/usr/bin/env python
"""Time the draw of the linear field (lpt.gaussian_field, lpt.linear_ics, lpt.colour_noise) on one MI355X.

Cases: the three calls at 256^3, 512^3 and 1024^3 with a power-law table of 256 points in a 1000 Mpc/h box.

Per case, in one run: the whole call (HIP events, median of --reps after a warm-up call) and its stages timed on their
own: the rocFFT transforms through torch.fft and the kernels of csrc/nbe_lpt.hip through the C ABI, each kernel beside a
device-to-device copy_ of a buffer of half its traffic, which reads and writes as many bytes as the kernel does.

Two comparisons are made in the same run:
(a) nbe_gaussian_spectrum against nbe_spectrum_inject with n_in = 2, the kernel that did the same arithmetic before (all
    but the 6 modes of the half spectrum inside the sphere |m| <= 1 are drawn), in time per drawn mode.  The two are timed alternately in --rounds
    rounds, each round a median of --reps, so that the spread between rounds of one kernel stands beside the difference
    between the two.
(b) the whole linear_ics call against the sum of its irfftn calls timed alone.

    python tools/time_ic.py --out profiles/ic_timing_512.json > profiles/ic_timing_512.txt
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
from time_lpt import copy_ms, event_ms, fft_row, kernel_row, spec_bytes  # noqa: E402

L = 1000.0
SEED = 1


def modes(n):
    return n * n * (n // 2 + 1)


def draw_call(l, out, n, table, kd, pd, flags, s):
    return lambda: _lib.check(l.nbe_gaussian_spectrum(_ptr(out), n, _ptr(kd), _ptr(pd), int(table[0].size), table[2],
                                                      table[3], L, 1.0, SEED, flags, 0, s))


def size_case(n, table, reps, rounds, dev):
    l = _lib.lib()
    s = _stream(dev)
    k, pk = table[0], table[1]
    kd, pd = torch.from_numpy(k).to(dev), torch.from_numpy(pk).to(dev)
    spec = T._empty_spectrum(n, dev)
    row = dict(n=n)

    # the kernels, each beside the copy of its bytes
    draw = draw_call(l, spec, n, table, kd, pd, 0, s)
    stages = [kernel_row("nbe_gaussian_spectrum", draw, spec_bytes(n), reps, dev),
              kernel_row("nbe_gaussian_spectrum fixed", draw_call(l, spec, n, table, kd, pd, T.FIXED_AMPLITUDE, s),
                         spec_bytes(n), reps, dev),
              kernel_row("nbe_gaussian_spectrum white", draw_call(l, spec, n, table, kd, pd, T.WHITE_NOISE, s),
                         spec_bytes(n), reps, dev),
              kernel_row("nbe_spectrum_colour",
                         lambda: _lib.check(l.nbe_spectrum_colour(_ptr(spec), n, _ptr(kd), _ptr(pd), int(k.size), table[2],
                                                                  table[3], L, 1e-4, s)), 2 * spec_bytes(n), reps, dev)]
    draw()                                                      # the colour pass ran in place (scale 1e-4: no overflow)
    psi_k = T._empty_spectrum(n, dev, (3,))
    stages.append(kernel_row("nbe_zeldovich_spectrum",
                             lambda: _lib.check(l.nbe_zeldovich_spectrum(_ptr(spec), n, L, 1.0, _ptr(psi_k), s)),
                             spec_bytes(n, 4), reps, dev))

    # (a) the draw against the injection kernel at n_in = 2, alternately
    src = torch.fft.rfftn(torch.randn((2, 2, 2), device=dev)).contiguous()
    out = T._empty_spectrum(n, dev)
    inject = lambda: _lib.check(l.nbe_spectrum_inject(_ptr(src), 2, _ptr(out), n, _ptr(kd), _ptr(pd), int(k.size), table[2],
                                                      table[3], L, SEED, s))
    a_draw, a_inject = [], []
    for _ in range(rounds):
        a_draw.append(event_ms(draw, reps))
        a_inject.append(event_ms(inject, reps))
    # n_in = 2 keeps the sphere 4 |m|^2 <= 4: m = 0, (+-1, 0, 0), (0, +-1, 0) and (0, 0, 1) of the half spectrum
    drawn = dict(draw=modes(n) - 1, inject=modes(n) - 6)
    del out
    ps = lambda ms, cnt: 1e9 * ms / cnt                           # picoseconds per mode
    row["per_mode"] = dict(
        draw_ms=a_draw, inject_ms=a_inject, draw_modes=drawn["draw"], inject_modes=drawn["inject"],
        draw_ps=ps(float(np.median(a_draw)), drawn["draw"]), inject_ps=ps(float(np.median(a_inject)), drawn["inject"]),
        draw_spread=(max(a_draw) - min(a_draw)) / float(np.median(a_draw)),
        inject_spread=(max(a_inject) - min(a_inject)) / float(np.median(a_inject)))
    row["per_mode"]["ratio"] = row["per_mode"]["draw_ps"] / row["per_mode"]["inject_ps"]

    # the transforms alone
    stages.append(fft_row("irfftn", lambda: torch.fft.irfftn(spec, s=(n, n, n)), reps))
    stages.append(fft_row("irfftn x3 (batched)", lambda: torch.fft.irfftn(psi_k, s=(n, n, n), dim=(1, 2, 3)), reps))
    del psi_k
    white = T.white_noise(n, seed=SEED)
    stages.append(fft_row("rfftn", lambda: torch.fft.rfftn(white), reps))
    row["stages"] = stages
    del spec
    torch.cuda.empty_cache()

    # the whole calls
    calls = dict(gaussian_field=event_ms(lambda: T.gaussian_field(n, L, k, pk, seed=SEED), reps),
                 linear_ics=event_ms(lambda: T.linear_ics(n, L, k, pk, SEED), reps),
                 linear_ics_no_delta=event_ms(lambda: T.linear_ics(n, L, k, pk, SEED, return_delta=False), reps),
                 colour_noise=event_ms(lambda: T.colour_noise(white, L, k, pk), reps))
    row["calls"] = calls
    t = {st["stage"]: st["ms"] for st in stages}
    row["linear_ics_irfftn_ms"] = t["irfftn"] + t["irfftn x3 (batched)"]
    row["linear_ics_remainder_ms"] = calls["linear_ics"] - row["linear_ics_irfftn_ms"]
    return row


def show(row):
    n, c, pm = row["n"], row["calls"], row["per_mode"]
    print("%d^3: gaussian_field %9.3f ms; linear_ics %9.3f ms (without delta %9.3f ms); colour_noise %9.3f ms"
          % (n, c["gaussian_field"], c["linear_ics"], c["linear_ics_no_delta"], c["colour_noise"]))
    for s in row["stages"]:
        if s["kind"] == "kernel":
            print("    %-30s %9.3f ms; %6.2f GB at copy bandwidth %9.3f ms (%.2f x)"
                  % (s["stage"], s["ms"], s["traffic_bytes"] / 1e9, s["copy_ms"], s["ratio"]))
        else:
            print("    %-30s %9.3f ms (rocFFT)" % (s["stage"], s["ms"]))
    print("    (a) per drawn mode: nbe_gaussian_spectrum %.2f ps, nbe_spectrum_inject (n_in = 2) %.2f ps: ratio %.3f; "
          "spread over %d alternating rounds %.1f %% and %.1f %%"
          % (pm["draw_ps"], pm["inject_ps"], pm["ratio"], len(pm["draw_ms"]), 100 * pm["draw_spread"],
             100 * pm["inject_spread"]))
    print("    (b) linear_ics %.3f ms = its four irfftn alone %.3f ms + %.3f ms (%.1f %%)"
          % (c["linear_ics"], row["linear_ics_irfftn_ms"], row["linear_ics_remainder_ms"],
             100 * row["linear_ics_remainder_ms"] / c["linear_ics"]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sizes = [int(v) for v in a.sizes.split(",") if v]
    k = np.geomspace(np.pi / L, 0.7 * np.pi * max(sizes) / L, 256)
    table = T._validate_table(k, 2.0e4 * (k / 0.1) ** -1.7)
    big = 1 << 30
    rows_copy = copy_ms(big, a.reps, dev)
    print("device-to-device copy_ of 1 GiB: %.3f ms = %.2f TB/s of traffic (read + write)"
          % (rows_copy, 2 * big / rows_copy / 1e9))
    rows = []
    for n in sizes:
        rows.append(size_case(n, table, a.reps, a.rounds, dev))
        show(rows[-1])
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, rounds=a.rounds,
               copy_1gib_ms=rows_copy, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
