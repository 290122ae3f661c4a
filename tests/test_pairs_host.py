"""Pair counts on the CPU: the NumPy restatement of tests/pairs_ref.py against hand-computed
answers, its own identities and scipy's periodic cKDTree; the thresholds, cell rule, estimator and multipoles of
correlation.py against it; and every ValueError of pair_counts, which must come before anything touches a device."""

import math
import re

import numpy as np
import pytest

import fof_ref as F
import pairs_ref as R
from jax_nbody_emulator_with_dj_amd import _lib, correlation as CF, halos as H


def test_restatement_on_the_lattice():
    """Spacing a: 6 neighbours at a, 12 at sqrt(2) a, 8 at sqrt(3) a, each pair once: 3 N, 6 N, 4 N."""
    N = R.LATTICE_N ** 3
    T = R.thresholds(R.LATTICE_EDGES, R.LATTICE_L)
    want = [3 * N, 6 * N, 4 * N]
    assert R.pair_counts(R.coordinates(R.lattice_positions(), R.LATTICE_L), T).tolist() == want
    assert R.pair_counts(R.catalogue(np.zeros((3, 16, 16, 16), np.float32), R.LATTICE_L), T).tolist() == want


def test_restatement_identities():
    pos, X, T, auto = R.uniform_case()
    assert pos.min() < -2.0 * R.UNIFORM_L and pos.max() > 3.0 * R.UNIFORM_L
    assert R.ncell_of(T) == 3 and T[0] == -1
    X1, X2 = X[:, :600], X[:, 600:]
    cross = R.pair_counts(X1, T, X2)
    assert np.array_equal(auto, R.pair_counts(X1, T) + R.pair_counts(X2, T) + cross)
    assert np.array_equal(cross, R.pair_counts(X2, T, X1))
    Tpos = [T[1]] + T[2:]                                                 # r_0 > 0: no coincident rows
    assert np.array_equal(R.pair_counts(X, Tpos, X), 2 * R.pair_counts(X, Tpos))
    assert R.pair_counts(X, T, X)[0] == 2 * auto[0] + X.shape[1]          # r_0 = 0: every row meets itself
    for nmu in (1, 5, 32):
        for los in (0, 1, 2):
            binned = R.pair_counts(X[:, :700], T, nmu=nmu, los=los)
            assert binned.shape == (5, nmu) and np.array_equal(binned.sum(axis=1), R.pair_counts(X[:, :700], T))
    rng = np.random.default_rng(3)
    for _ in range(2000):
        d2 = int(rng.integers(1, 1 << 60))
        dl2 = int(rng.integers(0, d2 + 1))
        nmu = int(rng.integers(1, 33))
        assert R.mu_bin(dl2, d2, nmu) == R.mu_bin_counted(dl2, d2, nmu)
    for nmu in (2, 5, 32):                                               # along and across the line of sight, and mu on an edge
        assert R.mu_bin(49, 49, nmu) == R.mu_bin_counted(49, 49, nmu) == nmu - 1
        assert R.mu_bin(0, 49, nmu) == 0
    assert R.mu_bin(9, 25, 5) == R.mu_bin_counted(9, 25, 5) == 3         # mu = 3 / 5 exactly: the bin that starts there


def test_restatement_equals_scipy():
    """cKDTree(boxsize=L).count_neighbors is cumulative and counts (i, j), (j, i) and (i, i): remove the rows themselves
    and halve.  The comparison needs an input on which float64 and the rounded coordinates agree: no pair within 1e-9
    relative of a threshold."""
    pytest.importorskip("scipy")
    from scipy.spatial import cKDTree
    pos, X, T, auto = R.uniform_case()
    N = X.shape[1]
    d2 = np.concatenate([(F.min_image(X[:, lo:lo + 250, None] - X[:, None, :]) ** 2).sum(axis=0).ravel()
                         for lo in range(0, N, 250)]).astype(np.float64)
    for t in T[1:]:
        assert (np.abs(d2 - float(t)) > 1e-9 * float(t)).all()
    wrapped = np.mod(pos, R.UNIFORM_L)
    wrapped[wrapped >= R.UNIFORM_L] = 0.0
    tree = cKDTree(wrapped, boxsize=R.UNIFORM_L)
    cum = tree.count_neighbors(tree, np.array(R.UNIFORM_EDGES[1:]))
    assert np.array_equal(np.diff(np.concatenate([[0], (cum - N) // 2])), auto)
    A, B = cKDTree(wrapped[:600], boxsize=R.UNIFORM_L), cKDTree(wrapped[600:], boxsize=R.UNIFORM_L)
    cum = A.count_neighbors(B, np.array(R.UNIFORM_EDGES[1:]))
    assert np.array_equal(np.diff(np.concatenate([[0], cum])), R.pair_counts(X[:, :600], T, X[:, 600:]))


def test_edge_points_hit_the_thresholds():
    X = R.coordinates(R.edge_points(), R.EDGE_L)
    T = R.thresholds(R.EDGE_EDGES, R.EDGE_L)
    assert T == [-1, 9 << 48, 25 << 48, 81 << 48, 169 << 48]
    d2 = (F.min_image(X[:, :, None] - X[:, None, :]) ** 2).sum(axis=0)
    for t in T[1:]:
        assert (d2 == t).sum() >= 2 * 60
    # a pair on a threshold is in the lower bin: moving every threshold down by one moves exactly those pairs up
    low = R.pair_counts(X, T)
    moved = R.pair_counts(X, [T[0]] + [t - 1 for t in T[1:]])
    on = [int((d2 == t).sum()) // 2 for t in T[1:]]
    assert [int(v) for v in low - moved] == [on[0], on[1] - on[0], on[2] - on[1], on[3] - on[2]]


def test_thresholds_and_cells():
    for L, edges in ((100.0, (0.0, 2.0, 5.0, 11.0, 20.0, 31.0)), (1000.0, (1.0, 7.5, 50.0)), (128.0, R.LATTICE_EDGES),
                     (25.0, (0.3, 8.3))):
        e, T, ncell = CF.pair_geometry(L, edges)
        assert e.dtype == np.float64 and np.array_equal(e, np.array(edges, np.float64))
        assert T[1:] == [F.r2_of(r, L) for r in edges[1:]] and T == R.thresholds(edges, L)
        assert T[0] == (-1 if edges[0] == 0 else F.r2_of(edges[0], L))
        assert ncell == R.ncell_of(T) == min(4096, F.U // (math.isqrt(T[-1]) + 1))
        assert 3 <= ncell <= 4096 and ncell * (math.isqrt(T[-1]) + 1) <= F.U
    assert CF.pair_geometry(100.0, (0.0, 31.0))[2] == 3 and CF.pair_geometry(100.0, (0.0, 0.01))[2] == 4096
    assert CF.pair_geometry(100.0, [0.0, 6.25])[1][1] == H.linking_geometry(16, 100.0, 1.0, False)[1]
    assert CF.pair_geometry(100.0, np.array([1, 2, 3]))[1] == R.thresholds((1.0, 2.0, 3.0), 100.0)


def test_pair_counts_validates_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("validation must come before the device is touched")
    monkeypatch.setattr(CF, "_device_of", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    ok = np.zeros((4, 3), np.float64)
    bad = [
        (dict(a=[[0.0, 0.0, 0.0]]), "NumPy array or a CUDA"),
        (dict(a=np.zeros((4, 2))), r"pair_counts: a must be \(count, 3\) positions or a \(3, n, n, n\) displacement"),
        (dict(a=np.zeros((3,))), "pair_counts: a must be"),
        (dict(a=np.zeros((0, 3))), "pair_counts: a must have 1 .. 2\\^30 rows"),
        (dict(a=np.zeros((4, 3), np.float16)), "pair_counts: positions a must be float32 or float64"),
        (dict(a=np.zeros((4, 3), np.int64)), "pair_counts: positions a must be float32 or float64"),
        (dict(a=np.zeros((3, 4, 4, 5), np.float32)), "pair_counts: a must be"),
        (dict(a=np.zeros((3, 4, 4, 4), np.float64)), "pair_counts: displacement a must be float32 or float16"),
        (dict(a=np.zeros((3, 1, 1, 1), np.float32)), "pair_counts: lattice size 1 unsupported"),
        (dict(b=np.zeros((4, 3, 1))), "pair_counts: b must be"),
        (dict(b=np.zeros((4, 3), np.int32)), "pair_counts: positions b must be float32 or float64"),
        (dict(boxsize=-1.0), "boxsize must be positive"),
        (dict(boxsize=(100.0, 100.0, 50.0)), "pair_counts needs a cubic box"),
        (dict(r_edges=[1.0]), "r_edges must be 2 .. 129 real numbers"),
        (dict(r_edges=np.linspace(0.0, 30.0, 130)), "r_edges must be 2 .. 129 real numbers"),
        (dict(r_edges=[[0.0, 1.0]]), "r_edges must be 2 .. 129 real numbers"),
        (dict(r_edges=["a", "b"]), "r_edges must be 2 .. 129 real numbers"),
        (dict(r_edges=[0.0, 2.0, 2.0]), "strictly increasing"),
        (dict(r_edges=[0.0, 3.0, 2.0]), "strictly increasing"),
        (dict(r_edges=[-1.0, 2.0]), "strictly increasing from 0 or more"),
        (dict(r_edges=[0.0, float("nan")]), "r_edges must be finite"),
        (dict(r_edges=[0.0, float("inf")]), "r_edges must be finite"),
        (dict(r_edges=[0.0, 1.0, 1.0 + 2e-16]), "give the same threshold"),
        (dict(r_edges=[1e-12, 2e-12]), "give the same threshold"),
        (dict(r_edges=[0.0, 100.0 / 3.0]), "must stay below L / 3"),
        (dict(r_edges=[0.0, 50.0]), "must stay below L / 3"),
        (dict(nmu=0), "nmu must be None or an int in 1 .. 32"),
        (dict(nmu=33), "nmu must be None or an int in 1 .. 32"),
        (dict(nmu=2.0), "nmu must be None or an int in 1 .. 32"),
        (dict(nmu=True), "nmu must be None or an int in 1 .. 32"),
        (dict(r_edges=np.linspace(0.0, 30.0, 130), nmu=32), "r_edges must be 2 .. 129"),
        (dict(nmu=4, los=3), "los must be the array axis"),
        (dict(_max_blocks=0), "pair_counts: _max_blocks must be an int >= 1"),
    ]
    for kw, match in bad:
        args = dict(a=ok, boxsize=100.0, r_edges=[0.0, 1.0, 2.0])
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            CF.pair_counts(**args)
    assert CF.pair_geometry(100.0, [0.0, 1e-12])[1] == [-1, 0]          # valid: a bin for coincident rows alone
    # nb nmu > 4096 cannot be reached inside nb <= 128 and nmu <= 32: the largest image is exactly the limit, and is taken
    # (tests/test_gpu_pairs.py counts with it); the check stands for limits that may be widened one at a time
    assert CF.MAX_BINS * CF.MAX_MU == CF.MAX_IMAGE
    monkeypatch.setattr(CF, "MAX_IMAGE", 4095)
    with pytest.raises(ValueError, match="128 x 32 bins exceed 4095"):
        CF.pair_counts(ok, 100.0, np.linspace(0.0, 30.0, 129), nmu=32)
    import torch
    with pytest.raises(ValueError, match="must live on a CUDA"):
        CF.pair_counts(torch.zeros((4, 3)), 100.0, [0.0, 1.0])
    with pytest.raises(ValueError, match="b: a torch tensor must live on a CUDA"):
        CF.pair_counts(ok, 100.0, [0.0, 1.0], b=torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="paint_halos needs fof_halos's dict"):
        H.halo_correlation([1, 2], 100.0, [0.0, 1.0])
    cat = dict(CMPosition=np.zeros((2, 3)), Length=np.array([30, 20]))
    with pytest.raises(ValueError, match="no halo is left"):
        H.halo_correlation(cat, 100.0, [0.0, 1.0], min_length=50)
    with pytest.raises(ValueError, match="redshift_space needs a catalogue with CMVelocity"):
        H.halo_correlation(cat, 100.0, [0.0, 1.0], redshift_space=True, velocity_to_length=1.0)
    cat["CMVelocity"] = np.zeros((2, 3))
    with pytest.raises(ValueError, match="velocity_to_length is required"):
        H.halo_correlation(cat, 100.0, [0.0, 1.0], redshift_space=True)


def test_estimator_and_multipoles():
    """The same float64 formulas on identical integers: only a few roundings may differ."""
    rng = np.random.default_rng(12)
    edges = np.array(R.UNIFORM_EDGES)
    for nmu in (None, 1, 5, 32):
        shape = (5,) if nmu is None else (5, nmu)
        npairs = rng.integers(0, 1 << 40, size=shape)
        for na, nb in ((1500, None), (600, 900)):
            ref = R.estimator(npairs, edges, R.UNIFORM_L, na, nb, nmu)
            rr = CF.analytic_rr(edges, R.UNIFORM_L, na, nb, nmu)
            np.testing.assert_allclose(rr, ref["rr"], rtol=1e-13, atol=0)
            xi = npairs / rr - 1.0
            np.testing.assert_allclose(xi, ref["xi"], rtol=1e-13, atol=0)
            if nmu is not None:
                for got, ell in zip(CF.multipoles(xi), (0, 2, 4)):
                    np.testing.assert_allclose(got, ref["xi%d" % ell], rtol=1e-13, atol=1e-13 * np.abs(xi).max())
    for nmu in (1, 2, 5, 10, 32):
        w = CF.legendre_bin_integrals(nmu)
        np.testing.assert_allclose(w, R.legendre_integrals(nmu), rtol=1e-13, atol=1e-16)
        np.testing.assert_allclose(w.sum(axis=1), [1.0, 0.0, 0.0], atol=1e-15)
        flat = np.full((3, nmu), 0.37)                                       # no mu dependence: no quadrupole, no hexadecapole
        xi0, xi2, xi4 = CF.multipoles(flat)
        np.testing.assert_allclose(xi0, 0.37, rtol=1e-14)
        assert np.abs(xi2).max() < 1e-15 and np.abs(xi4).max() < 1e-15
    # xi(mu) = L_2(mu) sampled as bin averages has xi2 -> 1 as the bins narrow
    nmu = 32
    w = CF.legendre_bin_integrals(nmu)
    xi2 = CF.multipoles((w[1] * nmu)[None, :])[1]
    assert abs(xi2[0] - 1.0) < 5e-3
    # analytic RR, by hand: N = 4, L = 10, one bin (0, 1]: 6 pairs times 4 pi / 3 / 1000
    assert CF.analytic_rr([0.0, 1.0], 10.0, 4)[0] == pytest.approx(6.0 * 4.0 * math.pi / 3.0 / 1000.0, rel=1e-15)
    assert CF.analytic_rr([0.0, 1.0], 10.0, 4, 5, nmu=2)[0, 1] == pytest.approx(20.0 * 4.0 * math.pi / 3.0 / 1000.0 / 2.0,
                                                                            rel=1e-15)


def test_abi_and_modules_are_declared():
    assert "nbe_pairs.hip" in _lib.SOURCES
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "nbe.h")).read()
    section = header[header.index("---- Pairs"):header.index("---- Input fields")]
    names = re.findall(r"^int (nbe_\w+)\(", section, flags=re.M)
    assert names == ["nbe_pair_coords", "nbe_pair_count", "nbe_pair_count_form"]
    for name in names:
        assert name in _lib.SIGNATURES
    for word in ("Corrfunc", "DDsmu", "SimulationBox2PCF"):
        assert word in section
    assert (CF.MAX_BINS, CF.MAX_MU, CF.MAX_IMAGE) == tuple(
        int(re.search(r"#define %s (\d+)" % n, section).group(1))
        for n in ("NBE_PAIR_MAX_BINS", "NBE_PAIR_MAX_MU", "NBE_PAIR_MAX_IMAGE"))
    assert set(CF.__all__) >= {"pair_counts", "correlation_function"}
    assert "halo_correlation" in H.__all__
    import jax_nbody_emulator_with_dj_amd as pkg
    assert not hasattr(pkg, "pair_counts") and "pair_counts" not in getattr(pkg, "__all__", ())
