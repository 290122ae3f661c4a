#!/usr/bin/env python
"""Time profiles.radial_counts on one MI355X.

In a 1000 Mpc/h box, edges profile_edges(0.05, r_max, 20) with r_max = 5 and 15, in one process:

- the FoF halos (b = 0.2, nmin = 20) of the 6 and of the 18 Mpc/h Zel'dovich fields of tools/time_fof.py at 512^3 as
  centres, that displaced lattice as matter;
- those halos, and 10^4 and 10^5 uniform centres, against the 2^21-row subsample of tools/time_pairs.py;
- where the two forms cross: 10^4 uniform centres against the subsample with r_max from 10 to 40 (57 to 4100 matter rows in
  the 27 cells of a centre), and 2500 and 5000 centres at r_max 5, 15 and 25.

Per case: the whole call on device tensors (HIP events, median of --reps after a warm-up call), its stages from events
recorded between them inside the same calls (coordinates, torch.sort and gather of each catalogue, count), and on records
sorted once, alternating in one loop: nbe_halo_profiles_form in both forms, nbe_halo_profiles (the library's choice of
them), and nbe_pair_count's cross count of the same records -- the only way to the stacked sum before this kernel, and it
returns one row, not H.  With them the candidate pairs (the matter in the 27 cells of every centre), the pairs counted,
and ns per candidate.  `--image64_lib LIB` adds both forms of a build with -DNBE_PROFILE_IMAGE64=1 (64-bit counters in the
LDS image) to the same loop.

`--ab_only` times correlation.pair_counts (10^5 uniform points, 20 bins to 50) and halos.fof_halos at 512^3 (18 Mpc/h) and
prints one JSON line: run with NBE_LIB pointing at the parent's library and at this one, alternately, three processes each,
to see that neither path moved.

    python tools/time_profiles.py --out profiles/halo_profiles_timing.json > profiles/halo_profiles_timing.txt
"""

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, correlation as CF, halos as H, profiles as P  # noqa: E402
from jax_nbody_emulator_with_dj_amd.density import _ptr, _stream  # noqa: E402
from time_fof import StageTimer, displacement  # noqa: E402
from time_lpt import event_ms  # noqa: E402

L = 1000.0
FORMS = {0: "workgroup per centre", 1: "wave per centre"}
CHOSEN, PAIR = "nbe_halo_profiles (the library's choice)", "nbe_pair_count cross (one row)"


WIDE = None                     # --image64_lib: a build with -DNBE_PROFILE_IMAGE64=1, timed beside the library in the same loop


def label(k):
    return "%s, 64-bit LDS image" % FORMS[k[0]] if isinstance(k, tuple) else FORMS.get(k, k)


def load_wide(path):
    lib = C.CDLL(path)
    res, argtypes = _lib.SIGNATURES["nbe_halo_profiles_form"]
    lib.nbe_halo_profiles_form.restype, lib.nbe_halo_profiles_form.argtypes = res, argtypes
    return lib


class CatalogueStages(StageTimer):
    """StageTimer whose coords, sort and gather marks say which catalogue they belong to."""

    def __call__(self, name):
        if name in ("coords", "sort", "gather"):
            name = "%s %s" % ("matter" if any(m[0] == "centres " + name for m in self.marks) else "centres", name)
        super().__call__(name)


def candidates(PA, skB, ncell):
    """The matter rows in the 27 cells around every centre, summed: what either kernel tests."""
    c = torch.bincount(skB, minlength=ncell ** 3).reshape(ncell, ncell, ncell).to(torch.float64)
    around = torch.zeros_like(c)
    for o0 in (-1, 0, 1):
        for o1 in (-1, 0, 1):
            for o2 in (-1, 0, 1):
                around += torch.roll(c, (o0, o1, o2), (0, 1, 2))
    cell = (PA[:, :3].to(torch.int64) * ncell) >> 30
    per = around[cell[:, 0], cell[:, 1], cell[:, 2]]
    return float(per.sum()), float(per.max())


def kernels_ms(rec, count_a, count_b, T, ncell, reps, dev):
    """ms of both forms and of the pair kernel's cross count, alternating, on the records of one call."""
    l = _lib.lib()
    nb = len(T) - 1
    th = (C.c_int64 * (nb + 1))(*T)
    names = list(FORMS) + [CHOSEN, PAIR] + ([(f, 64) for f in FORMS] if WIDE else [])
    times = {k: [] for k in names}
    tables = {}
    with torch.cuda.device(dev):
        s = _stream(dev)
        args = (_ptr(rec["PA"]), _ptr(rec["skA"]), count_a, _ptr(rec["PB"]), _ptr(rec["skB"]), count_b, ncell, th, nb)
        for r in range(reps + 1):
            for k in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if k == PAIR:
                    out = torch.zeros((nb, 1), dtype=torch.int64, device=dev)
                    e0.record()
                    _lib.check(l.nbe_pair_count(*args, 1, 2, 0, _ptr(out), s))
                else:
                    out = torch.empty((count_a, nb), dtype=torch.int64, device=dev)
                    e0.record()
                    if k == CHOSEN:
                        _lib.check(l.nbe_halo_profiles(*args, 0, _ptr(out), s))
                    elif isinstance(k, tuple):
                        assert WIDE.nbe_halo_profiles_form(*args, 0, k[0], _ptr(out), s) == 0
                    else:
                        _lib.check(l.nbe_halo_profiles_form(*args, 0, k, _ptr(out), s))
                e1.record()
                torch.cuda.synchronize()
                if r:
                    times[k].append(e0.elapsed_time(e1))
                tables[k] = out
    for k in names:
        assert k == PAIR or torch.equal(tables[0], tables[k]), "%r counts differently" % (k,)
    assert torch.equal(tables[0].sum(dim=0), tables[PAIR].reshape(-1)), "the rows do not add up to the cross count"
    return {k: float(np.median(v)) for k, v in times.items()}, int(tables[0].sum())


def case(name, centres, matter, r_max, reps, dev, bar):
    edges = P.profile_edges(0.05, r_max, 20)
    A, B, Lbox, _, T, ncell, blocks, _ = P._validate(centres, matter, L, edges, None, None)
    call = event_ms(lambda: P.radial_counts(centres, matter, L, edges), reps)
    rows, rec = [], {}
    for r in range(reps + 1):
        t = CatalogueStages()
        P._count(A, B, Lbox, T, ncell, blocks, timer=t, records=rec)
        if r:
            rows.append(t.times())
    stages = {k: float(np.median([row[k] for row in rows])) for k in rows[0]}
    cand, most = candidates(rec["PA"], rec["skB"], ncell)
    ms, counted = kernels_ms(rec, A[2], B[2], T, ncell, reps, dev)
    chosen = ms[CHOSEN]
    return dict(case=name, centres=A[2], matter=B[2], r_max=r_max, ncell=ncell, matter_per_27_cells=27.0 * B[2] / ncell ** 3,
                candidates=cand, most_candidates_of_a_centre=most, counted=counted, call_ms=call, stage_ms=stages,
                kernel_ms={label(k): v for k, v in ms.items()}, library_choice_ms=chosen,
                ns_per_candidate=chosen * 1e6 / max(cand, 1.0), pair_kernel_over_library_choice=ms[PAIR] / chosen, bar=bar,
                meets_bar=(chosen <= ms[PAIR]) if bar else None)


def show(row):
    print("%s: %d centres, %d matter rows, r_max %g, ncell %d (%.1f matter rows in 27 cells)"
          % (row["case"], row["centres"], row["matter"], row["r_max"], row["ncell"], row["matter_per_27_cells"]))
    print("    radial_counts %9.3f ms; stages (ms): %s"
          % (row["call_ms"], ", ".join("%s %.3f" % kv for kv in row["stage_ms"].items())))
    print("    %.3e candidates (at most %.0f a centre), %.3e counted; the library's choice %9.4f ms = %.4f ns a candidate"
          % (row["candidates"], row["most_candidates_of_a_centre"], row["counted"], row["library_choice_ms"],
             row["ns_per_candidate"]))
    for k, v in row["kernel_ms"].items():
        print("    %-40s %9.4f ms" % (k, v))
    print("    the cross count takes %.2f times the library's choice%s"
          % (row["pair_kernel_over_library_choice"],
             "" if row["meets_bar"] is None else ": the bar (not slower than the cross count) is %s"
             % ("met" if row["meets_bar"] else "MISSED")))
    sys.stdout.flush()


def ab_only(reps, dev):
    if os.environ.get("NBE_LIB"):                                     # the parent's library has no profiles to bind
        for k in [k for k in _lib.SIGNATURES if k.startswith("nbe_halo_profiles")]:
            del _lib.SIGNATURES[k]
    g = torch.Generator(device=dev).manual_seed(7)
    small = (torch.rand((1 << 20, 3), generator=g, device=dev, dtype=torch.float64) * L)[:100000].contiguous()
    edges = np.linspace(0.0, 50.0, 21)
    pairs = event_ms(lambda: CF.pair_counts(small, L, edges), reps)
    psi = displacement(512, 18.0, dev)
    fof = event_ms(lambda: H.fof_halos(psi, L, 0.2, 20), reps)
    print(json.dumps(dict(lib=_lib.LIB_PATH, pair_counts_1e5_ms=pairs, fof_halos_512_ms=fof)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ab_only", action="store_true")
    ap.add_argument("--only", default=None, help="comma-separated prefixes of the cases to run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--image64_lib", default=None,
                    help="a library built with -DNBE_PROFILE_IMAGE64=1: its two forms are timed in the same loop")
    a = ap.parse_args()
    global WIDE
    if a.image64_lib:
        WIDE = load_wide(a.image64_lib)
    dev = torch.device("cuda", 0)
    if a.ab_only:
        return ab_only(a.reps, dev)
    rows = []
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, boxsize=L, nbins=20,
               bar="at the FoF catalogues the library's choice must not be slower than nbe_pair_count's cross count of the "
                   "same records; the uniform centres are reported only", rows=rows)

    def save():                                                 # after every row: a run cut short keeps what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    def run(name, centres, matter, r_max, bar):
        if not wanted(name):
            return
        rows.append(case(name, centres, matter, r_max, a.reps, dev, bar))
        show(rows[-1])
        save()
        torch.cuda.empty_cache()

    def wanted(name):
        return not a.only or any(name.startswith(p) for p in a.only.split(","))

    g = torch.Generator(device=dev).manual_seed(7)
    uniform = torch.rand((1 << 20, 3), generator=g, device=dev, dtype=torch.float64) * L     # time_pairs.py's draws, in its order
    n = 512
    psi = displacement(n, 6.0, dev).reshape(3, -1)
    pick = torch.randperm(n ** 3, generator=g, device=dev)[:1 << 21]
    i2, rest = pick % n, pick // n
    q = torch.stack([rest // n, rest % n, i2]).to(torch.float32) * (L / n)
    sub = (q + psi[:, pick]).t().contiguous()                   # the 2^21-row subsample of the 6 Mpc/h field
    del psi, pick, q

    for rms in (6.0, 18.0):
        name = "fof halos 512^3 %g Mpc/h" % rms
        if not wanted(name):
            continue
        psi = displacement(n, rms, dev)
        centres = H.fof_halos(psi, L, 0.2, 20)["CMPosition"].contiguous()
        if centres.shape[0] == 0:
            print("%s: no halo (b = 0.2, nmin = 20), so no row" % name)
            out.setdefault("without_a_halo", []).append(name)
            continue
        for r_max in (5.0, 15.0):
            run(name, centres, psi, r_max, True)
        del psi
        torch.cuda.empty_cache()
        for r_max in (5.0, 15.0):                               # few centres and few rows a cell: the other corner
            run(name + ", against the 2^21 subsample", centres, sub, r_max, False)

    for count in (10000, 100000):
        for r_max in (5.0, 15.0):
            run("uniform 1e%d against the 2^21 subsample" % round(np.log10(count)), uniform[:count].contiguous(), sub, r_max, False)
    # where the forms cross: 10^4 uniform centres, the cells growing from 57 to 3600 matter rows in 27 of them
    for r_max in (10.0, 20.0, 22.0, 25.0, 30.0, 40.0):
        run("crossover 1e4 uniform against the 2^21 subsample", uniform[:10000].contiguous(), sub, r_max, False)
    # ... and how many centres the wave form needs: 2500 and 5000 uniform centres at 7, 197 and 955 rows in 27 cells
    for count in (2500, 5000):
        for r_max in (5.0, 15.0, 25.0):
            run("crossover %d uniform against the 2^21 subsample" % count, uniform[:count].contiguous(), sub, r_max, False)
    save()


if __name__ == "__main__":
    main()
