"""Friends-of-friends halos on the MI355X: halos.fof_halos against the NumPy restatement of
tests/fof_ref.py.  Labels, lengths, group counts and per-particle labels are integers and must be equal; the centres are the
same integers divided in float64."""

import numpy as np
import pytest

import fof_ref as F
from jax_nbody_emulator_with_dj_amd import halos as H

pytestmark = pytest.mark.gpu


def check(out, ref, velocity=True):
    assert np.array_equal(out["label"], ref["label"]) and out["label"].dtype == np.int64
    assert np.array_equal(out["Length"], ref["Length"]) and out["Length"].dtype == np.int64
    assert out["ngroups"] == ref["ngroups"]
    assert out["linking_length"] == ref["linking_length"]
    if "labels" in out:
        assert out["labels"].dtype == np.int32 and np.array_equal(out["labels"], ref["labels"])
    assert out["CMPosition"].dtype == np.float64 and out["CMPosition"].shape == (len(ref["label"]), 3)
    np.testing.assert_allclose(out["CMPosition"], ref["CMPosition"], rtol=1e-12, atol=0)
    if velocity:
        assert out["CMVelocity"].dtype == np.float64
        np.testing.assert_allclose(out["CMVelocity"], ref["CMVelocity"], rtol=1e-12, atol=0)
    else:
        assert "CMVelocity" not in out


@pytest.mark.parametrize("name", ["clustered16", "clustered16_half", "clustered24"])
def test_clustered_field_equals_the_reference(name):
    psi, L, v, kw, ref = F.case(name)
    assert (ref["Length"] >= 50).sum() >= 5
    out = H.fof_halos(psi, boxsize=L, velocity=v, return_labels=True, **kw)
    check(out, ref)
    check(H.fof_halos(psi, boxsize=L, **kw), ref, velocity=False)


def test_threshold_is_decided_in_integers():
    """d = (2^26, 0, 0) against R2 = 2^52 links, d = (2^26 + 1, 0, 0) does not, inside the box and across its face."""
    psi, L, ell, linked, unlinked = F.threshold_field()
    out = H.fof_halos(psi, boxsize=L, linking_length=ell, nmin=2, absolute=True, return_labels=True)
    check(out, F.fof(psi, L, linking_length=ell, nmin=2, absolute=True), velocity=False)
    lab = out["labels"].ravel()
    assert sorted(out["label"].tolist()) == sorted(min(p) for p in linked)
    assert out["Length"].tolist() == [2, 2] and out["ngroups"] == 62
    for p, q in linked:
        assert lab[p] == lab[q] >= 0
    for p, q in unlinked:
        assert lab[p] == lab[q] == -1


def test_undisplaced_lattice():
    psi = np.zeros((3, 16, 16, 16), np.float32)
    out = H.fof_halos(psi, boxsize=100.0, linking_length=0.2, nmin=2)
    assert out["ngroups"] == 16 ** 3 and len(out["Length"]) == 0 and out["CMPosition"].shape == (0, 3)
    out = H.fof_halos(psi, boxsize=100.0, linking_length=1.0, nmin=2)        # equality through every face
    assert out["ngroups"] == 1 and out["Length"].tolist() == [16 ** 3] and out["label"].tolist() == [0]
    big = np.zeros((3, 32, 32, 32), np.float32)                              # 32768 particles hooking onto one root
    out = H.fof_halos(big, boxsize=100.0, linking_length=1.0, nmin=2, return_labels=True)
    assert out["ngroups"] == 1 and out["Length"].tolist() == [32 ** 3] and out["label"].tolist() == [0]
    assert out["labels"].shape == (32, 32, 32) and not out["labels"].any()


def test_chain_is_one_group():
    psi, L, ell = F.chain_field()
    out = H.fof_halos(psi, boxsize=L, linking_length=ell, nmin=2, absolute=True, return_labels=True)
    assert out["ngroups"] == 1 and out["Length"].tolist() == [512] and out["label"].tolist() == [0]
    assert not out["labels"].any()


def test_bits_do_not_depend_on_geometry_call_or_kind():
    import torch
    psi, L, v, kw, ref = F.case("clustered16")
    first = H.fof_halos(psi, boxsize=L, velocity=v, return_labels=True, **kw)
    again = H.fof_halos(psi, boxsize=L, velocity=v, return_labels=True, **kw)
    one = H.fof_halos(psi, boxsize=L, velocity=v, return_labels=True, _max_blocks=1, **kw)
    dev = H.fof_halos(torch.from_numpy(psi).cuda(), boxsize=L, velocity=torch.from_numpy(v).cuda(), return_labels=True, **kw)
    for key in ("CMPosition", "CMVelocity", "Length", "label", "labels"):
        assert isinstance(dev[key], torch.Tensor) and dev[key].is_cuda
        for other in (again[key], one[key], dev[key].cpu().numpy()):
            assert other.dtype == first[key].dtype and np.array_equal(other.view(np.uint8), first[key].view(np.uint8)), key
    assert first["ngroups"] == again["ngroups"] == one["ngroups"] == dev["ngroups"]


def test_wave_reduction_gives_the_same_sums():
    """nbe_fof_catalog with and without the reduction of runs inside a wave: integer sums, so the same bits."""
    import torch
    psi, L, v, kw, ref = F.case("clustered16")
    _, R2, ncell = H.linking_geometry(16, L, kw["linking_length"], False)
    xd, vd = torch.from_numpy(psi).cuda(), torch.from_numpy(v).cuda()
    plain = H._stages(xd, vd, 16, L, kw["nmin"], R2, ncell, 0, True, wave_reduce=False)
    for blocks in (0, 1):
        waved = H._stages(xd, vd, 16, L, kw["nmin"], R2, ncell, blocks, True, wave_reduce=True)
        assert np.array_equal(waved[0], ref["label"]) and np.array_equal(waved[1], ref["Length"])
        assert waved[3].shape == (5, 6) and np.array_equal(waved[3], plain[3])
        assert np.array_equal(waved[6].cpu().numpy(), plain[6].cpu().numpy())


def test_nan_raises_and_the_next_call_works():
    psi, L, v, kw, ref = F.case("clustered16")
    bad = psi.copy()
    bad[1, 3, 4, 5] = np.nan
    with pytest.raises(ValueError, match="fof_halos: 1 particle"):
        H.fof_halos(bad, boxsize=L, **kw)
    bad[1, 3, 4, 5] = np.float32(L * 2.0 ** 21)
    with pytest.raises(ValueError, match="fof_halos: 1 particle"):
        H.fof_halos(bad, boxsize=L, **kw)
    vbad = v.copy()
    vbad[2, 0, 0, 0] = np.inf
    with pytest.raises(ValueError, match="velocity are not finite"):
        H.fof_halos(psi, boxsize=L, velocity=vbad, **kw)
    check(H.fof_halos(psi, boxsize=L, **kw), ref, velocity=False)


CATALOG_DTYPES = dict(CMPosition=np.float32, Npart=np.int32, Mass=np.float64, BoxSize=np.float64, NpartPerDim=np.int32,
                      LinkingLength=np.float64, AbsoluteLinking=np.bool_, Nmin=np.int32)


def check_catalog(path, cat, n, L, Om, b, nmin):
    z = np.load(path)
    assert sorted(z.files) == sorted(CATALOG_DTYPES)
    for key, dt in CATALOG_DTYPES.items():
        assert z[key].dtype == dt, key
    assert np.array_equal(z["Npart"], cat["Length"])
    assert np.array_equal(z["CMPosition"], cat["CMPosition"].astype(np.float32))
    assert np.array_equal(z["Mass"], cat["Length"] * H.particle_mass(Om, L, n))
    assert z["BoxSize"].tolist() == [L] * 3 and int(z["NpartPerDim"]) == n
    assert float(z["LinkingLength"]) == b and not bool(z["AbsoluteLinking"]) and int(z["Nmin"]) == nmin


def test_halos_module_writes_the_reference_catalogue(tmp_path):
    psi, L, _, kw, ref = F.case("clustered16")
    np.save(tmp_path / "dis.npy", np.moveaxis(psi, 0, -1))                   # the (N, N, N, 3) layout
    H.main(["--displacement_file", str(tmp_path / "dis.npy"), "--output_dir", str(tmp_path / "out"), "--boxsize", str(L),
            "--omega_m", "0.31", "--nmin", "8", "--catalog-file", "cat.npz"])
    cat = H.fof_halos(psi, boxsize=L, **kw)
    assert len(cat["Length"]) == 5
    check_catalog(tmp_path / "out" / "cat.npz", cat, 16, L, 0.31, 0.2, 8)


def test_run_emulator_fof_writes_the_catalogue(tmp_path):
    import torch
    import jax_nbody_emulator_with_dj_amd as J
    from jax_nbody_emulator_with_dj_amd import run_emulator as R
    from oracle import params as P
    p = P.synthetic_params(seed=71, mid_chan=8)
    np.savez(tmp_path / "weights.npz", params=p["params"])
    sim = tmp_path / "sim0"
    sim.mkdir()
    Om, z = 0.3, 0.5
    np.save(sim / "params.npy", np.array([Om, 0.05, 0.7, 0.96, 0.8, z]))
    box = np.random.default_rng(72).standard_normal((3, 16, 16, 16)).astype(np.float32) * 5
    np.save(sim / "dis.npy", box)
    R.main(["--cosmo_param_files", str(sim / "params.npy"), "--displacement_files", str(sim / "dis.npy"),
            "--output_dirs", str(sim), "--ndiv", "1", "--quiet", "--params", str(tmp_path / "weights.npz"),
            "--fof", "--fof_linking_length", "1.0", "--fof_nmin", "2", "--boxsize", "100"])
    assert sorted(f.name for f in sim.iterdir()) == ["dis.npy", "emu_dis.npy", "emu_vel.npy", "fof_catalog.npz", "params.npy"]
    cfg = J.SubboxConfig(size=(16, 16, 16), ndiv=(1, 1, 1), output_dtype=np.float32)
    emu = J.create_emulator(load_params=False, processor_config=cfg, mid_chan=8)
    emu.processor.params = p
    d32, _ = emu.process_box(torch.from_numpy(box).cuda(), z, Om, show_progress=False)
    cat = H.fof_halos(d32.cpu().numpy(), boxsize=100.0, linking_length=1.0, nmin=2)
    assert len(cat["Length"]) > 0
    check_catalog(sim / "fof_catalog.npz", cat, 16, 100.0, Om, 1.0, 2)
    assert np.load(sim / "emu_dis.npy").dtype == np.float16
