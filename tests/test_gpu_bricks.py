"""GPU: the z-slab brick protocol (nbe_brick_encode -> _interior -> _exchange -> _finish, include/nbe.h "Brick mode") at
PRODUCTION width, on one card and in one process (tests/brick_rig.py): one Engine per brick, faces moved by device copies.

The shapes are the smallest the protocol admits that still reach every edge: y x x = 48 x 56 (the minimum extent, unequal,
at level 2 one even and one odd in tiles); bricks of 48 (the minimum), 56 (b0 / 8 odd) and 64 planes in one box of
168 x 48 x 56, so that every brick has distinct z-minus and z-plus neighbours; origins 0, 48, 104 (all even: the Winograd-z
kernel pairs the planes as the single-device run does at levels 0 - 2).  The reference of every case is nbe_process_box of
the whole box on an engine of the same class; one cone of case a is held against the float64 oracle, which ties brick mode
-- not only process_box -- to it (the branch probe itself refuses brick mode).

What equals what.  Levels 0 - 2 launch even plane counts from even global planes for every brick depth and origin that brick
mode admits, so the Winograd-z kernel pairs the planes as the single-device run does.  conv_c at level 3 launches b0 / 8 + 6 and
b0 / 8 + 4 planes (27 and 25 in the 168-plane box, 12 / 10, 13 / 11 and 14 / 12 in the bricks): it runs on the direct kernels
everywhere (lower_levels), and every case is held to the bits of process_box."""

import numpy as np
import pytest

import brick_rig
import kink

pytestmark = pytest.mark.gpu

OM = 0.3
DZ, VF = 0.7731811501855036, 50.537651303131064              # growth_factor / vel_norm at z = 0.5, Om = 0.3
MID, S1, S2 = 64, 48, 56
DEPTHS = (48, 56, 64)
SEED_P, SEED_X = 91, 92
CONE_O, CONE_N = (48, 40, 0), 8                               # the first eight planes of the middle brick; the y cone wraps the box

_cache = {}


def _params():
    if "p" not in _cache:
        from oracle import params as P
        _cache["p"] = P.synthetic_params(seed=SEED_P, mid_chan=MID)
    return _cache["p"]


def _box(depths):
    import torch
    key = ("box", sum(depths))
    if key not in _cache:
        x = np.random.default_rng(SEED_X).standard_normal((3, sum(depths), S1, S2)).astype(np.float32)
        _cache[key] = (x, torch.from_numpy(x).cuda())
    return _cache[key]


def _engine(engine_factory, precision, vel, slab=None):
    e = engine_factory(mid_chan=MID, compute_vel=vel, precision=precision)
    if slab is not None:
        e.set_slab(slab)
    e.load_params(_params(), premodulated=False)
    e.set_cosmology(OM, DZ)
    return e


def _reference(engine_factory, key, precision, vel, depths, probe=False):
    """process_box of the whole box on one engine of the same class, computed once per arithmetic and left unchanged;
    probe: with the branch probe on the cone block (case a)."""
    if key in _cache:
        return _cache[key]
    size = (sum(depths), S1, S2)
    e = _engine(engine_factory, precision, vel)
    try:
        br = None
        if probe:
            e.probe_begin(CONE_O, CONE_N)
        try:
            out = e.process_box(_box(depths)[1], size, (1, 1, 1), ((48, 48),) * 3, DZ, VF)
            if probe:
                br = e.probe_read()
        finally:
            if probe:
                e.probe_end()
        d, v = out if vel else (out, None)
        _cache[key] = (d.cpu().numpy(), None if v is None else v.cpu().numpy(), br)
    finally:
        e.close()
    return _cache[key]


def _run(engine_factory, precision, vel, depths, slab=None, profile=False):
    engines = [_engine(engine_factory, precision, vel, slab) for _ in depths]
    try:
        if profile:
            engines[1].profile_enable(True)
            engines[1].profile_reset()
        d, v = brick_rig.run_bricks(engines, _box(depths)[1], depths, DZ, VF)
        names = [k["kernel"] for k in engines[1].profile_read()] if profile else None
        return d.cpu().numpy(), None if v is None else v.cpu().numpy(), names
    finally:
        for e in engines:
            e.close()


def _figures(tag, got, ref, depths):
    """Print, per field, how the bricks differ from process_box: voxels per brick and the largest difference in units of the
    field's RMS."""
    for name, a, b in (("disp", got[0], ref[0]), ("vel", got[1], ref[1])):
        if b is None:
            assert a is None
            continue
        assert a.shape == b.shape
        bad = a != b                                            # (a NaN differs from everything, itself included)
        per_brick = [int(np.count_nonzero(bad[:, o:o + n])) for o, n in zip(brick_rig.origins_of(depths), depths)]
        fin = np.isfinite(a) & np.isfinite(b)
        delta = np.abs(a.astype(np.float64) - b)[fin]
        rms = float(np.sqrt(np.mean(b[fin].astype(np.float64) ** 2)))
        print("%s %s: voxels that differ from process_box per brick %s of %s (%d non-finite); max |delta| %.3e = %.2e RMS (RMS %.3e)"
              % (tag, name, per_brick, [3 * n * S1 * S2 for n in depths], int(np.count_nonzero(~np.isfinite(a))),
                 float(delta.max()) if delta.size else 0.0, (float(delta.max()) / rms) if delta.size else 0.0, rms))


def _assert_bits(tag, got, ref, depths=DEPTHS):
    _figures(tag, got, ref, depths)
    for name, a, b in (("disp", got[0], ref[0]), ("vel", got[1], ref[1])):
        if b is not None:
            assert np.array_equal(a, b), "%s: %s of the bricks is not bit for bit that of process_box" % (tag, name)


def _oracle(engine_factory):
    """The float64 oracle on the cone of CONE_O with the branches of the probed f16x3 process_box: evaluated once."""
    if "oracle" not in _cache:
        ref = _reference(engine_factory, "ref f16x3 vel", "f16x3", True, DEPTHS, probe=True)
        _cache["oracle"] = kink.oracle_cone(_params(), kink.cone_input_periodic(_box(DEPTHS)[0], CONE_O, CONE_N), OM, DZ, VF, ref[2])
    return _cache["oracle"]


def _cone_block(a):
    o, n = CONE_O, CONE_N
    return a[:, o[0]:o[0] + n, o[1]:o[1] + n, o[2]:o[2] + n]


def test_a_f16x3_velocity_kernels_and_cone_oracle(engine_factory):
    """f16x3 with velocity on the default kernels: the Winograd-z kernel with the eight-chunk fused skip of conv_r00, the
    128-channel two-source concat and the 64 -> 3 head kernel, fed from exchanged faces.  The cone block of process_box AND
    of the bricks against the float64 oracle with the branches process_box took, at kink.assert_cone's default tolerances."""
    ref = _reference(engine_factory, "ref f16x3 vel", "f16x3", True, DEPTHS, probe=True)
    got = _run(engine_factory, "f16x3", True, DEPTHS, profile=True)
    names = got[2]
    assert any(n.startswith("conv_h3w") for n in names), names
    assert any(n.startswith("conv_h3n") for n in names), names          # conv_h3nz_kernel, the head
    d_o, v_o, st = _oracle(engine_factory)
    kink.assert_cone("width 64 f16x3 process_box, cone %s" % (CONE_O,), _cone_block(ref[0]), _cone_block(ref[1]), d_o, v_o, st)
    kink.assert_cone("width 64 f16x3 bricks 48+56+64, cone %s" % (CONE_O,), _cone_block(got[0]), _cone_block(got[1]), d_o, v_o, st)
    _assert_bits("case a", got, ref)


def test_b_f16x3_slabs_of_32_inside_the_bricks(engine_factory):
    """nbe_set_slab(32) before the first brick: slabs of 32 + 16, 32 + 24 and 32 + 32 planes inside the bricks, with carried
    planes at the slab seams.  include/nbe.h: "Results are identical" -- held against case a's reference."""
    ref = _reference(engine_factory, "ref f16x3 vel", "f16x3", True, DEPTHS, probe=True)
    _assert_bits("case b", _run(engine_factory, "f16x3", True, DEPTHS, slab=32), ref)


def test_c_f16x3_displacement_only(engine_factory):
    """compute_vel=False: half-sized faces and the kernel form with two accumulator sets per workgroup."""
    ref = _reference(engine_factory, "ref f16x3 novel", "f16x3", False, DEPTHS)
    got = _run(engine_factory, "f16x3", False, DEPTHS)
    assert got[1] is None
    _assert_bits("case c", got, ref)


def test_d_float16_model(engine_factory):
    """precision="f16" at mid 64: planes of eight channels, faces half the size of the float32-based ones."""
    ref = _reference(engine_factory, "ref f16 vel", "f16", True, DEPTHS)
    _assert_bits("case d", _run(engine_factory, "f16", True, DEPTHS), ref)


def test_e_strict_f32_two_bricks(engine_factory):
    """Two bricks: z-minus == z-plus, every brick gets both faces from the same neighbour."""
    depths = (48, 48)
    ref = _reference(engine_factory, "ref f32 vel 96", "f32", True, depths)
    _assert_bits("case e", _run(engine_factory, "f32", True, depths), ref, depths)


def test_f_f16x3_direct_kernels(engine_factory, direct_kernels):
    """NBE_WINO=0: include/nbe.h promises bits for any cut here -- a difference in this case is a wrong face, not a plane
    pairing."""
    ref = _reference(engine_factory, "ref f16x3 vel direct", "f16x3", True, DEPTHS)
    _assert_bits("case f", _run(engine_factory, "f16x3", True, DEPTHS), ref)


def test_brick_plan_follows_set_slab(engine_factory):
    """include/nbe.h, nbe_set_slab: "S: always" -- also after a brick of the same size has been planned.  The plan cache of
    nbe_brick_plan / nbe_brick_encode must not outlive the setting it was made under."""
    from oracle import params as P
    b = (64, 48, 48)
    p = P.synthetic_params(seed=61, mid_chan=8)

    def make():
        e = engine_factory(mid_chan=8, compute_vel=True, precision="f16x3")
        e.load_params(p, premodulated=False)
        e.set_cosmology(OM, DZ)
        return e

    fresh = make().brick_plan(b)
    assert fresh > 0 and fresh != 32                            # (the engine's own choice for a brick this small: one slab)
    e = make()
    e.set_slab(32)
    assert e.brick_plan(b) == 32
    e.set_slab(-1)
    assert e.brick_plan(b) == fresh
    e = make()
    assert e.brick_plan(b) == fresh
    e.set_slab(32)
    assert e.brick_plan(b) == 32
    e.set_slab(-1)
    assert e.brick_plan(b) == fresh
