#!/usr/bin/env python
"""Time the cosmic-web classification and the mesh readout (web.py, density.read_mesh) on one MI355X.

Per size (256^3, 512^3, 1024^3 of a Gaussian field with a red spectrum in a 1000 Mpc/h box): the whole calls tidal_tensor,
tensor_eigenvalues, classify_web (1 and 64 thresholds) and cosmic_web on device tensors (HIP events, median of --reps after
a warm-up call) with rocFFT's share, the transforms of the call alone through torch.fft; and each new kernel through the
C ABI beside a device-to-device copy_ of half the kernel's traffic, which reads and writes as many bytes as the kernel does.

The readout is timed alternately, in the same run, with the painter that is its adjoint: the lattice form (CIC and PCS, 1
and 4 channels) against paint_field of the same displacement; a shuffled catalogue of n^3 rows, sorted and unsorted,
against paint_particles of the same rows; and a catalogue of 10^4 rows.  min .. max of the alternating runs stand beside
each median.

    python tools/time_web.py --out profiles/web_timing_512.json > profiles/web_timing_512.txt

--ab times paint_particles, paint_field and lpt2_displacement at --sizes alone and prints one line each with --label in
front; it also runs on a library from before these entry points (NBE_LIB), which is how profiles/web_paint_lpt2_ab.txt was
made.
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

from jax_nbody_emulator_with_dj_amd import _lib  # noqa: E402

NEW = ("nbe_shear_spectrum", "nbe_tensor_eigenvalues", "nbe_web_classify", "nbe_mesh_read")
if os.environ.get("NBE_LIB"):                               # a library from before these entry points has no such symbols
    for name in NEW:
        _lib.SIGNATURES.pop(name, None)

from jax_nbody_emulator_with_dj_amd import density as D, lpt as T  # noqa: E402
from jax_nbody_emulator_with_dj_amd.density import _ptr, _stream  # noqa: E402
from time_lpt import L, copy_ms, event_ms, fft_row, kernel_row, red_field, spec_bytes  # noqa: E402


def alternate(fns, reps):
    """{name: (median, min, max) ms} of the calls `fns` (name -> fn), taken in turn reps times after one warm-up round."""
    times = {k: [] for k in fns}
    for r in range(reps + 1):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in times.items()}


def displacement(n, dev, rms=5.0):
    psi = T.zeldovich_displacement(red_field(n, n, dev), L)
    return (psi * (rms / psi.std())).contiguous()


def web_case(n, reps, dev):
    from jax_nbody_emulator_with_dj_amd import web as W
    l, s = _lib.lib(), _stream(dev)
    x = red_field(n, n, dev)
    sm = 4.0 * L / n
    row = dict(n=n, smoothing=sm, calls={}, stages=[])
    row["calls"]["tidal_tensor"] = event_ms(lambda: W.tidal_tensor(x, L, smoothing=sm), reps)
    tensor = W.tidal_tensor(x, L, smoothing=sm)
    row["calls"]["tensor_eigenvalues"] = event_ms(lambda: W.tensor_eigenvalues(tensor), reps)
    eig = W.tensor_eigenvalues(tensor)
    th64 = np.linspace(-0.5, 1.0, 64)
    row["calls"]["classify_web T=1"] = event_ms(lambda: W.classify_web(eig, 0.0), reps)
    row["calls"]["classify_web T=64"] = event_ms(lambda: W.classify_web(eig, th64), reps)
    torch.cuda.empty_cache()
    row["calls"]["cosmic_web"] = event_ms(lambda: W.cosmic_web(x, L, sm, 0.0), reps)
    row["calls"]["cosmic_web with mass"] = event_ms(lambda: W.cosmic_web(x, L, sm, 0.0, mass=x), reps)
    torch.cuda.empty_cache()
    # the stages of cosmic_web, each alone
    spec = T._half_spectrum(x)
    hk = T._empty_spectrum(n, dev, (6,))
    vk = T._empty_spectrum(n, dev, (3,))
    vk[:] = spec
    cells = n ** 3
    counts = torch.zeros((64, 5), dtype=torch.int64, device=dev)
    types = torch.empty((n, n, n), dtype=torch.uint8, device=dev)
    import ctypes as C
    th1, th = (C.c_float * 1)(0.0), (C.c_float * 64)(*[float(v) for v in th64])
    row["stages"] = [
        fft_row("rfftn %d^3" % n, lambda: torch.fft.rfftn(x), reps),
        kernel_row("nbe_gaussian_filter", lambda: _lib.check(l.nbe_gaussian_filter(_ptr(spec), n, sm / L, s)),
                   spec_bytes(n, 2), reps, dev),
        kernel_row("nbe_lpt2_hessian_spectrum", lambda: _lib.check(l.nbe_lpt2_hessian_spectrum(_ptr(spec), n, 0, 6, _ptr(hk), 0, s)),
                   spec_bytes(n, 7), reps, dev),
        kernel_row("nbe_shear_spectrum", lambda: _lib.check(l.nbe_shear_spectrum(_ptr(vk), n, L, 1.0, 0, 6, _ptr(hk), 0, s)),
                   spec_bytes(n, 9), reps, dev),
        fft_row("irfftn %d^3 x6 (batched)" % n, lambda: torch.fft.irfftn(hk, s=(n, n, n), dim=(1, 2, 3)), reps),
        kernel_row("nbe_tensor_eigenvalues", lambda: _lib.check(l.nbe_tensor_eigenvalues(_ptr(tensor), n, _ptr(eig), 0, s)),
                   9 * 4 * cells, reps, dev),
        kernel_row("nbe_web_classify T=1 + types", lambda: _lib.check(l.nbe_web_classify(_ptr(eig), n, th1, 1, 0, _ptr(types),
                                                                                         _ptr(counts), 0, s)),
                   13 * cells, reps, dev),
        kernel_row("nbe_web_classify T=64 + types", lambda: _lib.check(l.nbe_web_classify(_ptr(eig), n, th, 64, 0, _ptr(types),
                                                                                          _ptr(counts), 0, s)),
                   13 * cells, reps, dev),
        kernel_row("nbe_web_classify T=64", lambda: _lib.check(l.nbe_web_classify(_ptr(eig), n, th, 64, 0, None,
                                                                                  _ptr(counts), 0, s)),
                   12 * cells, reps, dev),
    ]
    return row


def read_case(n, reps, dev):
    """The readout beside its adjoint, res = n."""
    psi = displacement(n, dev)
    res = (n, n, n)
    box = (L, L, L)
    g = torch.Generator(device=dev).manual_seed(3)
    out = dict(n=n, lattice=[], catalogue=[])
    for worder in (2, 4):
        for nchan in (1, 4):
            f = torch.randn((nchan,) + res, generator=g, device=dev)
            q = torch.randn((nchan,) + res, generator=g, device=dev)
            t = alternate({"read_mesh": lambda: D._read_mesh(f, res, box, worder, 0.0, x=psi, n=res),
                           "paint_field": lambda: D._paint_fields(psi, q, None, 2, 0.0, res, box, res, worder)}, reps)
            out["lattice"].append(dict(worder=worder, nchan=nchan, read_mesh=t["read_mesh"], paint_field=t["paint_field"],
                                       ratio=t["read_mesh"][0] / t["paint_field"][0]))
            del f, q
    idx = torch.stack(torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float32)] * 3, indexing="ij")).reshape(3, -1)
    pos = (idx * (L / n) + psi.reshape(3, -1)).t().contiguous()
    del idx
    pos = pos[torch.randperm(pos.shape[0], device=dev, generator=g)].contiguous()
    f = torch.randn((1,) + res, generator=g, device=dev)
    for sort in (True, False):
        t = alternate({"read_mesh": lambda: D._read_mesh(f, res, box, 2, 0.0, p=pos, sort=sort),
                       "paint_particles": lambda: D._paint_particles(pos, None, None, 2, 0.0, box, res, 2, sort=sort,
                                                                      want_delta=True)}, reps)
        out["catalogue"].append(dict(rows=int(pos.shape[0]), sort=sort, read_mesh=t["read_mesh"],
                                     paint_particles=t["paint_particles"], ratio=t["read_mesh"][0] / t["paint_particles"][0]))
    halos = pos[:10000].contiguous()
    f4 = torch.randn((4,) + res, generator=g, device=dev)
    t = alternate({"read_mesh": lambda: D._read_mesh(f4, res, box, 2, 0.0, p=halos, sort=False),
                   "paint_particles": lambda: D._paint_particles(halos, None, None, 2, 0.0, box, res, 2, sort=False,
                                                                  want_delta=True)}, reps)
    out["catalogue"].append(dict(rows=10000, sort=False, nchan=4, read_mesh=t["read_mesh"], paint_particles=t["paint_particles"],
                                 ratio=t["read_mesh"][0] / t["paint_particles"][0]))
    return out


def show_web(row):
    n = row["n"]
    fft = sum(s["ms"] for s in row["stages"] if s["kind"] == "rocFFT")
    for k, v in row["calls"].items():
        print("%-28s %4d^3: call %9.3f ms" % (k, n, v))
    print("    rocFFT of cosmic_web (rfftn + six inverse transforms), alone: %9.3f ms = %.0f %% of the call"
          % (fft, 100.0 * fft / row["calls"]["cosmic_web"]))
    for s in row["stages"]:
        if s["kind"] == "kernel":
            print("    %-34s %9.3f ms; %6.2f GB at copy bandwidth %9.3f ms (%.2f x)"
                  % (s["stage"], s["ms"], s["traffic_bytes"] / 1e9, s["copy_ms"], s["ratio"]))
        else:
            print("    %-34s %9.3f ms (rocFFT)" % (s["stage"], s["ms"]))
    sys.stdout.flush()


def show_read(row):
    n = row["n"]
    span = lambda t: "%9.3f ms (%.3f .. %.3f)" % t
    for c in row["lattice"]:
        print("read_mesh lattice %4d^3 -> %d^3 %s %d ch: %s; paint_field %s; ratio %.2f"
              % (n, n, D.WORDERS[c["worder"]], c["nchan"], span(c["read_mesh"]), span(c["paint_field"]), c["ratio"]))
    for c in row["catalogue"]:
        print("read_mesh catalogue %9d rows -> %d^3 CIC %d ch sort=%-5s: %s; paint_particles %s; ratio %.2f"
              % (c["rows"], n, c.get("nchan", 1), c["sort"], span(c["read_mesh"]), span(c["paint_particles"]), c["ratio"]))
    sys.stdout.flush()


def ab(sizes, reps, dev, label):
    """The calls these entry points must not move: one line a case."""
    for n in sizes:
        psi = displacement(n, dev)
        res, box = (n, n, n), (L, L, L)
        q = torch.randn((1,) + res, device=dev)
        idx = torch.stack(torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float32)] * 3, indexing="ij")).reshape(3, -1)
        pos = (idx * (L / n) + psi.reshape(3, -1)).t().contiguous()
        del idx
        for worder in (2, 4):
            pf = event_ms(lambda: D._paint_fields(psi, q, None, 2, 0.0, res, box, res, worder), reps)
            pp = event_ms(lambda: D._paint_particles(pos, None, None, 2, 0.0, box, res, worder, sort=False, want_delta=True), reps)
            print("%s: %4d^3 %s: paint_field %9.3f ms, paint_particles %9.3f ms" % (label, n, D.WORDERS[worder], pf, pp))
        del pos, q, psi
        torch.cuda.empty_cache()
        x = red_field(n, n, dev)
        print("%s: %4d^3: lpt2_displacement %9.3f ms" % (label, n, event_ms(lambda: T.lpt2_displacement(x, L), reps)))
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--read-sizes", default="256,512", dest="read_sizes")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--label", default="run")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sizes = [int(v) for v in a.sizes.split(",") if v]
    if a.ab:
        ab(sizes, a.reps, dev, a.label)
        return
    big = 1 << 30
    rows_copy = copy_ms(big, a.reps, dev)
    print("device-to-device copy_ of 1 GiB: %.3f ms = %.2f TB/s of traffic (read + write)"
          % (rows_copy, 2 * big / rows_copy / 1e9))
    web_rows, read_rows = [], []
    for n in sizes:
        web_rows.append(web_case(n, a.reps, dev))
        show_web(web_rows[-1])
        torch.cuda.empty_cache()
    for n in [int(v) for v in a.read_sizes.split(",") if v]:
        read_rows.append(read_case(n, a.reps, dev))
        show_read(read_rows[-1])
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, copy_1gib_ms=rows_copy,
               web=web_rows, read=read_rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
