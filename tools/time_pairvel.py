#!/usr/bin/env python
"""Time correlation.pairwise_velocity and profiles.radial_velocity_moments on one MI355X, against the count kernels.

In a 1000 Mpc/h box, the catalogues of tools/time_pairs.py and tools/time_profiles.py, with the Zel'dovich displacement
times 100 as the velocity of a lattice (v is proportional to psi at first order) and seeded Gaussian velocities elsewhere:

- pairs (20 linear bins to r_max, auto): 10^5 uniform points to 50; the FoF halos (b = 0.2, nmin = 20) of the 512^3 field of
  18 Mpc/h with their CMVelocity to 50; the 2^21-row subsample of the 6 Mpc/h field to 30; the 256^3 lattice of that recipe to 5;
- profiles (profile_edges(0.05, r_max, 20)): those halos about their own displaced lattice at r_max 5 and 15 and about the
  subsample at 15; 10^4 uniform centres about the subsample at r_max 10, 20, 25, 30 and 40, where the two forms cross.

Per case: the whole call on device tensors (HIP events, median of --reps after a warm-up call), its stages from events recorded
inside the same calls (range, coordinates, torch.sort and gather of each catalogue, words, moments), and on records sorted
once, alternating in one loop: the moments kernel in its forms and the library's choice of them, and the count kernel of the
parent (nbe_pair_count, nbe_halo_profiles) on the same records -- the yardstick: the moments kernel reads 32 instead of 16
bytes for a pair that is binned and adds six words instead of one.  With them the candidate pairs, the pairs binned, ns per
candidate and the ratio of the two kernels.

`--host N` only times tests/pairvel_ref.py on N uniform points to 50 on the host, for scale, and needs no device.  `--ab_only` is
tools/time_profiles.py's: correlation.pair_counts, profiles.radial_counts and halos.fof_halos with NBE_LIB pointing at the
parent's library and at this one, alternately, to see that none moved.

    python tools/time_pairvel.py --out profiles/pairvel_timing.json > profiles/pairvel_timing.txt
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from jax_nbody_emulator_with_dj_amd import _lib, correlation as CF, halos as H, profiles as P  # noqa: E402
from jax_nbody_emulator_with_dj_amd.density import _ptr, _stream  # noqa: E402
from time_fof import StageTimer, displacement  # noqa: E402
from time_lpt import event_ms  # noqa: E402
from time_pairs import candidates as auto_candidates  # noqa: E402
from time_profiles import CatalogueStages, candidates as centre_candidates  # noqa: E402

L = 1000.0
VELOCITY_PER_LENGTH = 100.0     # v = 100 psi: the scale of km/s per Mpc/h at z = 0
PAIR_FORMS = {0: "moments, LDS image", 1: "moments, global atomics"}
PROFILE_FORMS = {0: "moments, workgroup per centre", 1: "moments, wave per centre"}
CHOSEN, COUNT = "moments, the library's choice", "count kernel of the same records"


def alternate(launch, names, reps):
    """Median ms of launch(name) -> output tensor for every name, alternating, after a warm-up round; the last outputs."""
    times, outs = {k: [] for k in names}, {}
    for r in range(reps + 1):
        for k in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            outs[k] = launch(k, e0)
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in times.items()}, outs


def stages_of(run, timer, reps):
    rows, rec = [], {}
    for r in range(reps + 1):
        t = timer()
        run(t, rec)
        if r:
            rows.append(t.times())
    return {k: float(np.median([row[k] for row in rows])) for k in rows[0]}, rec


def pair_case(name, a, va, r_max, reps, dev):
    edges = np.linspace(0.0, r_max, 21)
    A, _, Lbox, _, T, ncell, _, _, blocks = CF._validate(a, L, edges, None, None, 2, None)
    call = event_ms(lambda: CF.pairwise_velocity(a, va, L, edges), reps)
    count_call = event_ms(lambda: CF.pair_counts(a, L, edges), reps)
    stages, rec = stages_of(lambda t, rec: CF._moments(A, va, None, None, Lbox, T, ncell, blocks, timer=t, records=rec),
                            StageTimer, reps)
    l, nb = _lib.lib(), len(T) - 1
    th = (C.c_int64 * (nb + 1))(*T)
    with torch.cuda.device(dev):
        s = _stream(dev)

        def launch(k, e0):
            if k == COUNT:
                out = torch.zeros((nb, 1), dtype=torch.int64, device=dev)
                e0.record()
                _lib.check(l.nbe_pair_count(_ptr(rec["PA"]), _ptr(rec["skA"]), A[2], None, None, 0, ncell, th, nb, 1, 2, 0, _ptr(out), s))
                return out
            out = torch.zeros((nb, 6), dtype=torch.int64, device=dev)
            args = (_ptr(rec["PA"]), _ptr(rec["skA"]), _ptr(rec["WA"]), A[2], None, None, None, 0, ncell, th, nb, 0)
            e0.record()
            if k == CHOSEN:
                _lib.check(l.nbe_pair_velocity(*args, _ptr(out), s))
            else:
                _lib.check(l.nbe_pair_velocity_form(*args, k, _ptr(out), s))
            return out

        ms, outs = alternate(launch, list(PAIR_FORMS) + [CHOSEN, COUNT], reps)
    for k in PAIR_FORMS:
        assert torch.equal(outs[k], outs[CHOSEN]), "form %r sums differently" % (k,)
    assert torch.equal(outs[CHOSEN][:, 0], outs[COUNT].reshape(-1)), "N is not the count kernel's"
    cand = auto_candidates(rec["skA"], ncell, dev)[0]
    label = lambda k: PAIR_FORMS.get(k, k)
    return dict(kind="pairs", case=name, rows=A[2], r_max=r_max, ncell=ncell, candidates=cand, binned=int(outs[COUNT].sum()),
                call_ms=call, count_call_ms=count_call, stage_ms=stages, kernel_ms={label(k): v for k, v in ms.items()},
                ns_per_candidate=ms[CHOSEN] * 1e6 / max(cand, 1.0), count_ns_per_candidate=ms[COUNT] * 1e6 / max(cand, 1.0),
                moments_over_count=ms[CHOSEN] / ms[COUNT])


def profile_case(name, centres, vc, matter, vm, r_max, reps, dev):
    edges = P.profile_edges(0.05, r_max, 20)
    A, B, Lbox, _, T, ncell, blocks, _ = P._validate(centres, matter, L, edges, None, None)
    call = event_ms(lambda: P.radial_velocity_moments(centres, vc, matter, vm, L, edges), reps)
    count_call = event_ms(lambda: P.radial_counts(centres, matter, L, edges), reps)
    stages, rec = stages_of(lambda t, rec: P._velocity_count(A, vc, B, vm, Lbox, T, ncell, blocks, timer=t, records=rec),
                            CatalogueStages, reps)
    l, nb = _lib.lib(), len(T) - 1
    th = (C.c_int64 * (nb + 1))(*T)
    with torch.cuda.device(dev):
        s = _stream(dev)

        def launch(k, e0):
            if k == COUNT:
                out = torch.empty((A[2], nb), dtype=torch.int64, device=dev)
                e0.record()
                _lib.check(l.nbe_halo_profiles(_ptr(rec["PA"]), _ptr(rec["skA"]), A[2], _ptr(rec["PB"]), _ptr(rec["skB"]), B[2], ncell,
                                               th, nb, 0, _ptr(out), s))
                return out
            out = torch.empty((A[2], nb, 6), dtype=torch.int64, device=dev)
            args = (_ptr(rec["PA"]), _ptr(rec["skA"]), _ptr(rec["WA"]), A[2], _ptr(rec["PB"]), _ptr(rec["skB"]), _ptr(rec["WB"]), B[2],
                    ncell, th, nb, 0)
            e0.record()
            if k == CHOSEN:
                _lib.check(l.nbe_halo_velocity_profiles(*args, _ptr(out), s))
            else:
                _lib.check(l.nbe_halo_velocity_profiles_form(*args, k, _ptr(out), s))
            return out

        ms, outs = alternate(launch, list(PROFILE_FORMS) + [CHOSEN, COUNT], reps)
    for k in PROFILE_FORMS:
        assert torch.equal(outs[k], outs[CHOSEN]), "form %r sums differently" % (k,)
    assert torch.equal(outs[CHOSEN][:, :, 0], outs[COUNT]), "N is not the count kernel's"
    cand, most = centre_candidates(rec["PA"], rec["skB"], ncell)
    label = lambda k: PROFILE_FORMS.get(k, k)
    return dict(kind="profiles", case=name, centres=A[2], matter=B[2], r_max=r_max, ncell=ncell,
                matter_per_27_cells=27.0 * B[2] / ncell ** 3, candidates=cand, most_candidates_of_a_centre=most,
                binned=int(outs[COUNT].sum()), call_ms=call, count_call_ms=count_call, stage_ms=stages,
                kernel_ms={label(k): v for k, v in ms.items()}, faster_form=label(min(PROFILE_FORMS, key=lambda k: ms[k])),
                ns_per_candidate=ms[CHOSEN] * 1e6 / max(cand, 1.0), count_ns_per_candidate=ms[COUNT] * 1e6 / max(cand, 1.0),
                moments_over_count=ms[CHOSEN] / ms[COUNT])


def show(row):
    if row["kind"] == "pairs":
        print("pairs, %s: %d rows, r_max %g, ncell %d" % (row["case"], row["rows"], row["r_max"], row["ncell"]))
    else:
        print("profiles, %s: %d centres, %d matter rows, r_max %g, ncell %d (%.1f matter rows in 27 cells)"
              % (row["case"], row["centres"], row["matter"], row["r_max"], row["ncell"], row["matter_per_27_cells"]))
    print("    the call %9.3f ms (the count's call %9.3f ms); stages (ms): %s"
          % (row["call_ms"], row["count_call_ms"], ", ".join("%s %.3f" % kv for kv in row["stage_ms"].items())))
    print("    %.3e candidates, %.3e binned; %.4f ns a candidate, the count kernel %.4f" % (row["candidates"], row["binned"],
          row["ns_per_candidate"], row["count_ns_per_candidate"]))
    for k, v in row["kernel_ms"].items():
        print("    %-40s %9.4f ms" % (k, v))
    print("    the moments kernel takes %.2f times the count kernel" % row["moments_over_count"])
    sys.stdout.flush()


def host_scale(count):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pairvel_ref as V
    rng = np.random.default_rng(7)
    pos, vel = rng.uniform(0.0, L, size=(count, 3)), 300.0 * rng.standard_normal((count, 3))
    t0 = time.perf_counter()
    sums, _ = V.moments_of(pos, vel, L, np.linspace(0.0, 50.0, 21), verify=False)
    return dict(rows=count, host_seconds=time.perf_counter() - t0, binned=int(sums[:, 0].sum()))


def ab_only(reps, dev):
    if os.environ.get("NBE_LIB"):                                     # the parent's library has no velocity moments to bind
        for k in [k for k in _lib.SIGNATURES if "velocity" in k]:
            del _lib.SIGNATURES[k]
    g = torch.Generator(device=dev).manual_seed(7)
    uniform = torch.rand((1 << 20, 3), generator=g, device=dev, dtype=torch.float64) * L
    small = uniform[:100000].contiguous()
    pairs = event_ms(lambda: CF.pair_counts(small, L, np.linspace(0.0, 50.0, 21)), reps)
    psi = displacement(512, 18.0, dev)
    fof = event_ms(lambda: H.fof_halos(psi, L, 0.2, 20), reps)
    centres = uniform[:10000].contiguous()
    prof = event_ms(lambda: P.radial_counts(centres, psi, L, P.profile_edges(0.05, 15.0, 20)), reps)
    print(json.dumps(dict(lib=_lib.LIB_PATH, pair_counts_1e5_ms=pairs, radial_counts_1e4_ms=prof, fof_halos_512_ms=fof)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ab_only", action="store_true")
    ap.add_argument("--host", type=int, default=0, metavar="N")
    ap.add_argument("--only", default=None, help="comma-separated prefixes of the cases to run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.host:                                                  # needs no device
        print("for scale only: tests/pairvel_ref.py on %(rows)d uniform points to 50 on the host (float64 rint, unverified): "
              "%(host_seconds).1f s, %(binned)d pairs binned" % host_scale(a.host))
        return
    dev = torch.device("cuda", 0)
    if a.ab_only:
        return ab_only(a.reps, dev)
    rows = []
    out = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), reps=a.reps, boxsize=L, nbins=20, rows=rows)

    def save():                                                 # after every row: a run cut short keeps what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    def wanted(name):
        return not a.only or any(name.startswith(p) for p in a.only.split(","))

    def run(fn, name, *args):
        if not wanted(name):
            return
        rows.append(fn(name, *args, a.reps, dev))
        show(rows[-1])
        save()
        torch.cuda.empty_cache()

    g = torch.Generator(device=dev).manual_seed(7)
    uniform = torch.rand((1 << 20, 3), generator=g, device=dev, dtype=torch.float64) * L     # time_pairs.py's draws, in its order
    gauss = 300.0 * torch.randn((1 << 20, 3), generator=g, device=dev, dtype=torch.float64)
    run(pair_case, "uniform 1e5", uniform[:100000].contiguous(), gauss[:100000].contiguous(), 50.0)

    n = 512
    psi = displacement(n, 6.0, dev).reshape(3, -1)
    pick = torch.randperm(n ** 3, generator=g, device=dev)[:1 << 21]
    i2, rest = pick % n, pick // n
    q = torch.stack([rest // n, rest % n, i2]).to(torch.float32) * (L / n)
    sub = (q + psi[:, pick]).t().contiguous()                   # the 2^21-row subsample of the 6 Mpc/h field
    vsub = (VELOCITY_PER_LENGTH * psi[:, pick]).t().contiguous()
    del psi, pick, q
    run(pair_case, "subsample 2^21 of 512^3 6 Mpc/h", sub, vsub, 30.0)
    small = displacement(256, 6.0, dev)
    run(pair_case, "lattice 256^3 6 Mpc/h", small, (VELOCITY_PER_LENGTH * small).contiguous(), 5.0)
    del small

    psi = displacement(n, 18.0, dev)
    vel = (VELOCITY_PER_LENGTH * psi).contiguous()
    cat = H.fof_halos(psi, L, 0.2, 20, velocity=vel)
    centres, cv = cat["CMPosition"].contiguous(), cat["CMVelocity"].contiguous()
    run(pair_case, "fof halos 512^3 18 Mpc/h", centres, cv, 50.0)
    for r_max in (5.0, 15.0):
        run(profile_case, "fof halos 512^3 18 Mpc/h about their lattice", centres, cv, psi, vel, r_max)
    del psi, vel
    torch.cuda.empty_cache()
    run(profile_case, "fof halos 512^3 18 Mpc/h about the 2^21 subsample", centres, cv, sub, vsub, 15.0)
    for r_max in (10.0, 20.0, 25.0, 30.0, 40.0):                # where the forms of the count kernel cross
        run(profile_case, "crossover 1e4 uniform about the 2^21 subsample", uniform[:10000].contiguous(), gauss[:10000].contiguous(),
            sub, vsub, r_max)
    save()


if __name__ == "__main__":
    main()
