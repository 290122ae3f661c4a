#!/usr/bin/env python
"""Time density.paint_particles on one MI355X: the positions of the two Zel'dovich fields of tools/time_density.py (3-D rms
6 and 18 Mpc/h in a 1000 Mpc/h box) at 256^3 and 512^3 particles, in lattice order and in a seeded random permutation,
painted onto 256^3 .. 1024^3 meshes with CIC and PCS.

Per case, HIP events, the median of --reps after a warm-up call, the variants alternating inside every repetition:
the whole call with sort=True and sort=False; the stages of the sorted call (keys, torch.sort, paint) and the share of
512-particle chunks on the direct path, sorted and unsorted; paint_density on the same displacement (what generality
costs); and a device-to-device copy_ of the bytes the paint kernel touches (the positions, the order and one read and one
write of the mesh).  Then the key variants (tile edge 4 / 8 / 16, row-major or Morton) on the shuffled positions, and
halo-scale catalogues of 10^4 .. 10^6 positions, on a 512^3 mesh and on a mesh of about one cell per position.

    python tools/time_particles.py --out profiles/particles_timing_512.json
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, density as D  # noqa: E402
from time_density import gaussian_displacement  # noqa: E402


def positions_of(psi, L):
    """(count, 3) float32 positions q + psi of a (3, n, n, n) device displacement, rows in lattice order."""
    n = psi.shape[1]
    q = torch.arange(n, device=psi.device, dtype=torch.float32) * (L / n)
    x = torch.stack([psi[0] + q[:, None, None], psi[1] + q[None, :, None], psi[2] + q[None, None, :]], dim=-1)
    return x.reshape(-1, 3).contiguous()


class Events:
    """HIP-event timer: ms between start() and stop()."""
    def start(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.e0.record()

    def stop(self):
        self.e1.record()
        torch.cuda.synchronize()
        return self.e0.elapsed_time(self.e1)


def timed(fn):
    ev = Events()
    ev.start()
    fn()
    return ev.stop()


def stages(x, L, res, worder, sort, edge=None, morton=None):
    """({stage: ms}, direct chunks) of one _paint_particles call; the stage marks are HIP events on the stream."""
    marks = []

    def timer(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))

    _, _, stats = D._paint_particles(x, None, None, 0, 0.0, (L,) * 3, (res,) * 3, worder, sort=sort, want_delta=True,
                                     tile_edge=edge, morton=morton, timer=timer)
    torch.cuda.synchronize()
    out = {}
    for (name, e0), (_, e1) in zip(marks[:-1], marks[1:]):
        out[name] = e0.elapsed_time(e1)
    return out, int(stats[0])


def copy_ms(nbytes, dev):
    a = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    b = torch.empty_like(a)
    t = timed(lambda: b.copy_(a))
    del a, b
    return t


def median(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


def time_case(x, psi, L, res, worder, reps, dev):
    """One row: every variant once per repetition, in turn."""
    count = int(x.shape[0])
    chunks = (count + 511) // 512
    touched = count * 12 + count * 8 + 2 * 8 * res ** 3
    runs = []
    direct = {}
    for r in range(reps + 1):
        row = {}
        row["call_sorted_ms"] = timed(lambda: D.paint_particles(x, L, res, worder, deconvolve=False, sort=True))
        row["call_unsorted_ms"] = timed(lambda: D.paint_particles(x, L, res, worder, deconvolve=False, sort=False))
        st, direct["sorted"] = stages(x, L, res, worder, True)
        row.update({"keys_ms": st["keys"], "sort_ms": st["sort"], "paint_sorted_ms": st["paint"],
                    "convert_ms": st["convert"]})
        st, direct["unsorted"] = stages(x, L, res, worder, False)
        row["paint_unsorted_ms"] = st["paint"]
        if psi is not None:
            row["paint_density_ms"] = timed(lambda: D.paint_density(psi, L, res, worder, deconvolve=False))
        row["copy_touched_bytes_ms"] = copy_ms(touched, dev)
        if r:
            runs.append(row)
    out = median(runs)
    out.update(count=count, res=res, worder=worder, mas=D.WORDERS[worder], chunks=chunks, touched_bytes=touched,
               direct_share_sorted=direct["sorted"] / chunks, direct_share_unsorted=direct["unsorted"] / chunks)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="256,512")
    ap.add_argument("--res", default="256,512,1024")
    ap.add_argument("--worders", default="2,4")
    ap.add_argument("--boxsize", type=float, default=1000.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--halo-counts", default="10000,100000,1000000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = a.boxsize
    ints = lambda s: [int(v) for v in s.split(",") if v]
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, rows=[], keys=[],
               halo_scale=[], auto=dict(min_count=D._AUTO_MIN_COUNT, max_cells_per_particle=D._AUTO_MAX_CELLS_PER_PARTICLE,
                                        tile_edges=list(D._KEY_EDGES), sparse_from_cells_per_particle=D._KEY_SPARSE,
                                        morton=bool(D._KEY_MORTON)))

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    for n in ints(a.n):
        base = gaussian_displacement(n, L, 6.0, 1, dev)
        perm = torch.randperm(n ** 3, generator=torch.Generator(device=dev).manual_seed(7), device=dev)
        for case, scale in (("realistic", 1.0), ("clustered", 3.0)):
            psi = (base * scale).contiguous()
            lattice = positions_of(psi, L)
            for order in ("lattice", "shuffled"):
                x = lattice if order == "lattice" else lattice[perm].contiguous()
                for res in ints(a.res):
                    for p in ints(a.worders):
                        row = time_case(x, psi, L, res, p, a.reps, dev)
                        row.update(case=case, rms3d_mpc_h=6.0 * scale, n=n, order=order)
                        out["rows"].append(row)
                        print("%-9s %4d^3 %-8s -> %4d^3 %s: sorted call %8.2f ms (keys %6.2f, sort %7.2f, paint %7.2f, "
                              "direct %5.1f %%), unsorted call %8.2f ms (paint %7.2f, direct %5.1f %%), paint_density "
                              "%7.2f ms, copy %6.2f ms"
                              % (case, n, order, res, row["mas"], row["call_sorted_ms"], row["keys_ms"], row["sort_ms"],
                                 row["paint_sorted_ms"], 100 * row["direct_share_sorted"], row["call_unsorted_ms"],
                                 row["paint_unsorted_ms"], 100 * row["direct_share_unsorted"], row["paint_density_ms"],
                                 row["copy_touched_bytes_ms"]), flush=True)
                        save()
                # the key of the sort, on the shuffled positions of the realistic field at res = n and 2 n
                if order == "shuffled" and case == "realistic":
                    for kres, p in [(n, p) for p in ints(a.worders)] + [(2 * n, p) for p in ints(a.worders)]:
                        for edge in (4, 8, 16):
                            for morton in (False, True):
                                runs = []
                                for r in range(a.reps + 1):
                                    st, direct = stages(x, L, kres, p, True, edge, morton)
                                    if r:
                                        runs.append(st)
                                m = median(runs)
                                row = dict(n=n, res=kres, worder=p, tile_edge=edge, morton=morton, keys_ms=m["keys"],
                                           sort_ms=m["sort"], paint_ms=m["paint"],
                                           direct_share=direct / ((n ** 3 + 511) // 512))
                                out["keys"].append(row)
                                print("key  %4d^3 -> %4d^3 %s edge %2d %-9s: keys %6.2f, sort %7.2f, paint %7.2f ms, direct "
                                      "%5.1f %%" % (n, kres, D.WORDERS[p], edge, "morton" if morton else "row-major",
                                                    row["keys_ms"], row["sort_ms"], row["paint_ms"],
                                                    100 * row["direct_share"]), flush=True)
                    save()
                if order == "shuffled" and case == "clustered" and n == max(ints(a.n)):
                    # halo-scale catalogues: the first rows of the shuffled positions, i.e. a random subsample
                    for count, hres in [(c, 512) for c in ints(a.halo_counts)] + \
                            [(c, int(round(c ** (1.0 / 3.0)))) for c in ints(a.halo_counts)]:
                        for p in ints(a.worders):
                            row = time_case(x[:count].contiguous(), None, L, hres, p, a.reps, dev)
                            row.update(n=n, case=case)
                            out["halo_scale"].append(row)
                            print("halo %8d -> %3d^3 %s: sorted call %7.2f ms (keys %5.2f, sort %6.2f, paint %6.2f, direct "
                                  "%5.1f %%), unsorted call %7.2f ms (paint %6.2f), convert %6.2f ms"
                                  % (count, hres, row["mas"], row["call_sorted_ms"], row["keys_ms"], row["sort_ms"],
                                     row["paint_sorted_ms"], 100 * row["direct_share_sorted"], row["call_unsorted_ms"],
                                     row["paint_unsorted_ms"], row["convert_ms"]), flush=True)
                    save()
                if order == "shuffled":
                    del x
            del psi, lattice
        del base, perm
    save()


if __name__ == "__main__":
    main()
