#!/usr/bin/env python
"""Time correlation.pair_counts on one MI355X.

In a 1000 Mpc/h box, 20 linear bins from 0 to r_max, auto counts, in one process:

- 10^5 uniform points and the FoF halos (b = 0.2, nmin = 20) of the 18 Mpc/h Zel'dovich field of tools/time_fof.py at
  512^3, each at r_max = 50 and 150;
- a 2^21-row seeded subsample of the positions of the 6 Mpc/h field at 512^3 at r_max = 30, without and with nmu = 10;
- the 256^3 displaced lattice of the 6 Mpc/h recipe itself (a displacement input) at r_max = 5;
- 2^20 uniform points at r_max from 2.5 to 50, that is from 0.02 to 130 points in a cell: where the two decompositions
  cross.

Per case: the whole call on device tensors (HIP events, median of --reps after a warm-up call), its stages from events
recorded between them inside the same calls (coordinates, torch.sort, gather, count), and the count kernel alone in its four
forms, alternating -- one LDS atomic per lane or the equal bins of a wave added once, a workgroup per run of one cell or a
thread per particle -- on records sorted once.  With them the candidate pairs tested (from the cell occupancies), the pairs
counted, ns per candidate, and lane-cycles per candidate beside the vector instructions of the inner loop's disassembly.

For scale only: `--scipy` also times scipy's periodic cKDTree.count_neighbors on the host for the 10^5 uniform points.
That is another machine part and another algorithm; it is no comparison.

`--fof_only` times halos.fof_halos at 512^3 (18 Mpc/h) and prints one JSON line: run with NBE_LIB pointing at the parent's
library and at this one, alternately, three processes each, to see that the FoF path did not move.

    python tools/time_pairs.py --scipy --out profiles/pairs_timing.json > profiles/pairs_timing.txt
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

from jax_nbody_emulator_with_dj_amd import _lib, correlation as CF, halos as H  # noqa: E402
from time_fof import StageTimer, displacement  # noqa: E402
from time_lpt import event_ms  # noqa: E402

L = 1000.0
CLOCK_HZ = 2.4e9                # the MI355X's peak engine clock: lane-cycles are an upper bound where it runs below that
FORMS = {0: "cells, atomic per lane", 1: "cells, wave-combined", 2: "particles, atomic per lane", 3: "particles, wave-combined"}
# v_* instructions of one pass of the loop over a range in pair_particles_kernel<false>, from the disassembly of the built
# library: up to the rejection on |d_c| > s, and in all for a pair that is binned without mu (tools: llvm-objdump -d on the
# gfx950 code object; DESIGN.md section 12.7 says how they were counted)
INNER_LOOP_VALU = {"rejected": 17, "to_the_squared_distance": 22}


def candidates(keys, ncell, dev):
    """Candidate pairs an auto count tests: the pairs inside a cell, and each pair of adjacent cells once."""
    c = torch.bincount(keys, minlength=ncell ** 3).reshape(ncell, ncell, ncell).to(torch.float64)
    around = torch.zeros_like(c)
    for o0 in (-1, 0, 1):
        for o1 in (-1, 0, 1):
            for o2 in (-1, 0, 1):
                around += torch.roll(c, (o0, o1, o2), (0, 1, 2))
    return float(((c * around).sum() - c.sum()) / 2.0), int((c > 0).sum()), int(c.max())


def kernel_ms(A, Lbox, T, ncell, nmu, reps, dev):
    """ms of nbe_pair_count_form alone in each form, alternating, on records sorted once; the counts of every form."""
    l = _lib.lib()
    from jax_nbody_emulator_with_dj_amd.density import _ptr, _stream
    import ctypes as C
    with torch.cuda.device(dev):
        s = _stream(dev)
        P, sk = CF._sorted_records(l, A[0], A[1], A[2], Lbox, ncell, 0, dev, s, lambda name: None)
        cand = candidates(sk, ncell, dev)
        nb = len(T) - 1
        th = (C.c_int64 * (nb + 1))(*T)
        times = {f: [] for f in FORMS}
        results = {}
        for r in range(reps + 1):
            for f in FORMS:
                counts = torch.zeros((nb, nmu), dtype=torch.int64, device=dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(l.nbe_pair_count_form(_ptr(P), _ptr(sk), A[2], None, None, 0, ncell, th, nb, nmu, 2, 0, f,
                                                 _ptr(counts), s))
                e1.record()
                torch.cuda.synchronize()
                if r:
                    times[f].append(e0.elapsed_time(e1))
                results[f] = counts.cpu().numpy()
    for f in FORMS:
        assert np.array_equal(results[f], results[0]), "form %d counts differently" % f
    return {f: float(np.median(v)) for f, v in times.items()}, cand, results[0]


def case(name, a, r_max, nmu, reps, dev, nbins=20):
    edges = np.linspace(0.0, r_max, nbins + 1)
    A, _, Lbox, _, T, ncell, nm, los, blocks = CF._validate(a, L, edges, None, nmu, 2, None)
    call = event_ms(lambda: CF.pair_counts(a, L, edges, nmu=nmu), reps)
    rows = []
    for r in range(reps + 1):
        t = StageTimer()
        CF._count(A, None, Lbox, T, ncell, nm or 1, los, blocks, timer=t)
        if r:
            rows.append(t.times())
    stages = {k: float(np.median([row[k] for row in rows])) for k in rows[0]}
    forms, (cand, cells, fullest), counts = kernel_ms(A, Lbox, T, ncell, nm or 1, reps, dev)
    lanes_hz = torch.cuda.get_device_properties(dev).multi_processor_count * 64 * CLOCK_HZ   # 4 SIMDs of 16 lanes
    best = min(forms, key=forms.get)
    chosen = stages["count"]
    row = dict(case=name, rows=A[2], r_max=r_max, nmu=nmu, ncell=ncell, mean_occupancy=A[2] / ncell ** 3, occupied_cells=cells,
               fullest_cell=fullest, candidates=cand, pairs=int(counts.sum()), call_ms=call, stage_ms=stages,
               sort_share=stages["sort"] / sum(stages.values()), kernel_ms={FORMS[f]: v for f, v in forms.items()},
               fastest_form=FORMS[best], library_choice_ms=chosen,
               ns_per_candidate=chosen * 1e6 / max(cand, 1.0),
               lane_cycles_per_candidate=chosen * 1e-3 * lanes_hz / max(cand, 1.0),
               inner_loop_valu=INNER_LOOP_VALU)
    return row


def show(row):
    print("%s: %d rows, r_max %g%s, ncell %d (%.2f rows a cell, fullest %d)"
          % (row["case"], row["rows"], row["r_max"], ", nmu %d" % row["nmu"] if row["nmu"] else "", row["ncell"],
             row["mean_occupancy"], row["fullest_cell"]))
    print("    pair_counts %9.3f ms; stages (ms): %s; the sort's share %.0f %%"
          % (row["call_ms"], ", ".join("%s %.3f" % kv for kv in row["stage_ms"].items()), 100.0 * row["sort_share"]))
    print("    %.3e candidates, %.3e counted; the library's choice %9.3f ms = %.4f ns, %.1f lane-cycles a candidate"
          % (row["candidates"], row["pairs"], row["library_choice_ms"], row["ns_per_candidate"],
             row["lane_cycles_per_candidate"]))
    for k, v in row["kernel_ms"].items():
        print("    %-28s %9.3f ms" % (k, v))
    sys.stdout.flush()


def scipy_scale(pos):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(np.mod(pos, L), boxsize=L)
    cum = tree.count_neighbors(tree, np.linspace(0.0, 50.0, 21)[1:])
    return dict(rows=len(pos), r_max=50.0, host_seconds=time.perf_counter() - t0, pairs=int((cum[-1] - len(pos)) // 2),
                note="for scale only: scipy cKDTree.count_neighbors on the host CPU, one thread")


def fof_only(reps, dev):
    if os.environ.get("NBE_LIB"):                                     # the parent's library has no pair counts to bind
        for k in [k for k in _lib.SIGNATURES if k.startswith("nbe_pair_")]:
            del _lib.SIGNATURES[k]
    psi = displacement(512, 18.0, dev)
    ms = event_ms(lambda: H.fof_halos(psi, L, 0.2, 20), reps)
    print(json.dumps(dict(lib=_lib.LIB_PATH, fof_halos_512_ms=ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--fof_only", action="store_true")
    ap.add_argument("--only", default=None, help="comma-separated prefixes of the cases to run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.fof_only:
        return fof_only(a.reps, dev)
    rows = []
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, boxsize=L, nbins=20,
               cells_from=None, rows=rows)

    def save():                                                 # after every row: a run cut short keeps what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    def run(name, make, r_max, nmu=None):
        if a.only and not any(name.startswith(p) for p in a.only.split(",")):
            return
        rows.append(case(name, make(), r_max, nmu, a.reps, dev))
        show(rows[-1])
        save()
        torch.cuda.empty_cache()

    g = torch.Generator(device=dev).manual_seed(7)
    uniform = torch.rand((1 << 20, 3), generator=g, device=dev, dtype=torch.float64) * L
    small = uniform[:100000].contiguous()
    if a.scipy and not a.only:
        out["scipy_for_scale"] = scipy_scale(small.cpu().numpy())
        print("for scale only: scipy count_neighbors of 10^5 points to 50 on the host: %.1f s" % out["scipy_for_scale"]["host_seconds"])
    for r_max in (50.0, 150.0):
        run("uniform 1e5", lambda: small, r_max)
    cache = {}

    def halos():
        if "halos" not in cache:
            cat = H.fof_halos(displacement(512, 18.0, dev), L, 0.2, 20)
            cache["halos"] = cat["CMPosition"].contiguous()
        return cache["halos"]

    def subsample():
        if "sub" not in cache:
            n = 512
            psi = displacement(n, 6.0, dev).reshape(3, -1)
            pick = torch.randperm(n ** 3, generator=g, device=dev)[:1 << 21]
            i2, rest = pick % n, pick // n
            q = torch.stack([rest // n, rest % n, i2]).to(torch.float32) * (L / n)
            cache["sub"] = (q + psi[:, pick]).t().contiguous()
        return cache["sub"]

    for r_max in (50.0, 150.0):
        run("fof halos 512^3 18 Mpc/h", halos, r_max)
    run("subsample 2^21 of 512^3 6 Mpc/h", subsample, 30.0)
    run("subsample 2^21 of 512^3 6 Mpc/h", subsample, 30.0, nmu=10)
    cache.clear()
    run("lattice 256^3 6 Mpc/h", lambda: displacement(256, 6.0, dev), 5.0)
    for r_max in (2.5, 5.0, 7.5, 10.0, 12.5, 15.0, 20.0, 30.0, 50.0):
        run("crossover 2^20 uniform", lambda: uniform, r_max)
    save()


if __name__ == "__main__":
    main()
