#!/usr/bin/env python
"""Time halos.fof_halos on one MI355X.

At 256^3, 512^3 and (where the memory estimate allows) 1024^3 particles in a 1000 Mpc/h box, for b = 0.2 and nmin = 20, on
the zeldovich_displacement of the red Gaussian field of tools/time_lpt.py scaled to a 3-D rms of 6 and of 18 Mpc/h (the two
fields of profiles/density_timing_512.json), in one run:

- the whole call on a device tensor (HIP events, median of --reps after a warm-up call);
- its stages, from events recorded between them inside the same calls: coordinates and keys (nbe_fof_cells), torch.sort,
  linking (nbe_fof_gather and nbe_fof_link, apart), labels (nbe_fof_labels), the choice of the halos (torch) and the
  catalogue sums (nbe_fof_catalog, with and without the reduction of runs inside a wave);
- beside every kernel a device-to-device copy_ of the bytes it reads and writes at least once;
- the halo count, the largest Length, the largest cell occupancy and the peak of torch's allocations per particle.

For scale only: `--scipy_n 128` also times scipy's periodic cKDTree.query_pairs plus connected_components on the host for
a 128^3 field of the same recipe.  That is another machine part, another algorithm and another size; it is no comparison.

    python tools/time_fof.py --out profiles/fof_timing_512.json > profiles/fof_timing_512.txt
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, halos as H, lpt as T  # noqa: E402
from jax_nbody_emulator_with_dj_amd.density import _ptr, _stream  # noqa: E402
from time_lpt import copy_ms, event_ms, red_field  # noqa: E402

L = 1000.0
B = 0.2
NMIN = 20
# bytes per particle each kernel reads and writes at least once (float32 displacement)
KERNEL_BYTES = {"cells": 12 + 12 + 8 + 4, "gather": 8 + 12 + 16, "link": 16 + 8 + 4, "labels": 4 + 4 + 4,
                "catalog": 12 + 4 + 4}
STAGES = ("cells", "sort", "gather", "link", "labels", "select", "catalog", "finish")


def displacement(n, rms, dev):
    psi = T.zeldovich_displacement(red_field(n, n, dev), L)
    psi *= rms / float(torch.sqrt((psi.double() ** 2).sum(dim=0).mean()))
    return psi.contiguous()


class StageTimer:
    def __init__(self):
        self.marks = []

    def __call__(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((name, e))

    def times(self):
        torch.cuda.synchronize()
        return {a[0]: a[1].elapsed_time(b[1]) for a, b in zip(self.marks[:-1], self.marks[1:])}


def stage_times(psi, n, R2, ncell, reps, wave_reduce):
    rows = []
    for r in range(reps + 1):
        t = StageTimer()
        out = H._stages(psi, None, n, L, NMIN, R2, ncell, 0, False, wave_reduce=wave_reduce, timer=t)
        if r:
            rows.append(t.times())
    return {k: float(np.median([row[k] for row in rows])) for k in rows[0]}, out


def occupancy(psi, n, ncell, dev):
    count = n ** 3
    try:
        X = torch.empty((3, count), dtype=torch.int32, device=dev)
        keys = torch.empty(count, dtype=torch.int64, device=dev)
        parent = torch.empty(count, dtype=torch.int32, device=dev)
        stats = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().nbe_fof_cells(_ptr(psi), 0, n, L, ncell, 0, _ptr(X), _ptr(keys), _ptr(parent), _ptr(stats),
                                            _stream(dev)))
        del X, parent
        _, counts = torch.unique_consecutive(torch.sort(keys)[0], return_counts=True)
        return int(counts.max()), int(counts.numel())
    except RuntimeError:                                         # out of memory at the largest size: no figure
        return None, None


def case(n, rms, reps, dev):
    psi = displacement(n, rms, dev)
    count = n ** 3
    ell, R2, ncell = H.linking_geometry(n, L, B, False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    H.fof_halos(psi, L, B, NMIN)
    peak = (torch.cuda.max_memory_allocated(dev) - held) / count          # torch's allocations: the sort's workspace included
    call = event_ms(lambda: H.fof_halos(psi, L, B, NMIN), reps)
    stages, out = stage_times(psi, n, R2, ncell, reps, True)
    plain, _ = stage_times(psi, n, R2, ncell, reps, False)
    label, length = out[0], out[1]
    occ, cells = occupancy(psi, n, ncell, dev)
    row = dict(n=n, rms3d_mpc_h=rms, linking_length=ell, ncell=ncell, call_ms=call, stage_ms=stages,
               catalog_without_wave_reduce_ms=plain["catalog"], halos=int(len(label)), ngroups=int(out[5]),
               largest_length=int(length[0]) if len(length) else 0, largest_cell_occupancy=occ, occupied_cells=cells,
               bytes_per_particle_estimate=H.BYTES_PER_PARTICLE, bytes_per_particle_peak=peak)
    row["kernels"] = [dict(stage=k, ms=stages[k], bytes=b * count, copy_ms=copy_ms(b * count // 2, reps, dev))
                      for k, b in KERNEL_BYTES.items()]
    for k in row["kernels"]:
        k["ratio"] = k["ms"] / k["copy_ms"]
    return row


def show(row):
    print("%d^3, rms %g Mpc/h: fof_halos %9.3f ms; %d halos of %d groups, largest %d, fullest of %s cells holds %s"
          % (row["n"], row["rms3d_mpc_h"], row["call_ms"], row["halos"], row["ngroups"], row["largest_length"],
             row["occupied_cells"], row["largest_cell_occupancy"]))
    print("    peak device memory of the call: %.1f bytes per particle (the call budgets %d)"
          % (row["bytes_per_particle_peak"], row["bytes_per_particle_estimate"]))
    print("    stages (ms): " + ", ".join("%s %.3f" % (k, row["stage_ms"][k]) for k in STAGES if k in row["stage_ms"]))
    print("    catalogue sums without the wave reduction: %.3f ms" % row["catalog_without_wave_reduce_ms"])
    for k in row["kernels"]:
        print("    %-8s %9.3f ms; copy_ of the %6.2f GB it touches %9.3f ms (%.2f x)"
              % (k["stage"], k["ms"], k["bytes"] / 1e9, k["copy_ms"], k["ratio"]))
    sys.stdout.flush()


def scipy_scale(n, rms, dev):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    psi = displacement(n, rms, dev).cpu().numpy().astype(np.float64)
    q = np.stack(np.meshgrid(*([np.arange(n) * (L / n)] * 3), indexing="ij"))
    pos = np.mod((q + psi).reshape(3, -1).T, L)
    pos[pos >= L] = 0.0
    t0 = time.perf_counter()
    pairs = cKDTree(pos, boxsize=L).query_pairs(B * L / n, output_type="ndarray")
    ncomp, _ = connected_components(coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n ** 3,) * 2),
                                    directed=False)
    return dict(n=n, rms3d_mpc_h=rms, host_seconds=time.perf_counter() - t0, ngroups=int(ncomp),
                note="for scale only: scipy cKDTree + connected_components on the host CPU, one thread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--rms", default="6,18")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scipy_n", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows, skipped = [], []
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, boxsize=L,
               linking_length_b=B, nmin=NMIN, rows=rows, skipped=skipped)

    def save():                                                 # after every row: a run cut short keeps what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    if a.scipy_n:
        out["scipy_for_scale"] = scipy_scale(a.scipy_n, 6.0, dev)
        print("for scale only: scipy cKDTree route at %d^3 on the host: %.1f s" % (a.scipy_n, out["scipy_for_scale"]["host_seconds"]))
    for n in [int(v) for v in a.sizes.split(",") if v]:
        free, _ = torch.cuda.mem_get_info(dev)
        if (H.BYTES_PER_PARTICLE + 24) * n ** 3 > free:        # the call's estimate plus the field and its making
            skipped.append(n)
            print("%d^3 skipped: %d bytes per particle do not fit the %.1f GB that are free"
                  % (n, H.BYTES_PER_PARTICLE + 24, free / 1e9))
            continue
        for rms in [float(v) for v in a.rms.split(",") if v]:
            rows.append(case(n, rms, a.reps, dev))
            show(rows[-1])
            save()
            torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
