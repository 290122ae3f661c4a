"""The case tables of tests/stream_cases.py held to their purpose: every tile edge of the stem, up-sampling and stride-2 /
1x1x1 kernels that the tables were chosen for is named here, so that a table cannot be thinned out unnoticed.  CPU only:
the tiling is the restatement in stream_cases.py, the oracle is evaluated on every case (both of its backends)."""

import numpy as np
import pytest

import stream_cases as S
from oracle import layers as L


def _q(c):
    return S.flat_q(c.kind, c.dims, c.crop)


def test_names_are_unique_and_every_case_says_why():
    names = [c.name for c in S.CASES]
    assert len(set(names)) == len(names)
    assert all(len(c.why) > 5 for c in S.CASES)


@pytest.mark.parametrize("kind,table", [("up", S.UP), ("down", S.DOWN), ("skip", S.SKIP)])
def test_flat_tables_reach_the_tile_edges(kind, table):
    """Q one short of a tile, a whole tile, one into the next -- for each flat kernel family, and among the cases that run on
    every (arithmetic, velocity) combination"""
    assert all(c.kind == kind for c in table)
    assert {0, 1, 255} <= {_q(c) % S.TILE for c in table}
    assert {0, 1, 255} <= {_q(c) % S.TILE for c in table if c.rep}
    assert {255, 256, 257} <= {_q(c) for c in table}
    assert any(S.ntiles(_q(c)) > S.XCDS for c in table if c.rep) or kind == "skip"     # an XCD with two tiles
    assert any(S.ntiles(_q(c)) > 1 and _q(c) % S.TILE > 1 for c in table)              # several tiles and a ragged last one


def test_tile_counts_cover_the_xcd_remainders():
    nts = {S.ntiles(_q(c)) for c in S.FLAT}
    assert {0, 1, 7} <= {nt % S.XCDS for nt in nts}
    assert {7, 15, 17} <= {S.ntiles(_q(c)) for c in S.UP}
    assert any(_q(c) % (S.XCDS * S.TILE) == 0 for c in S.DOWN)
    assert 10 in {S.ntiles(_q(c)) for c in S.DOWN}


def test_xcd_tile_is_a_permutation():
    for nt in sorted({S.ntiles(_q(c)) for c in S.FLAT} | set(range(1, 40))):
        tiles = [S.xcd_tile(b, nt) for b in range(nt)]
        assert sorted(tiles) == list(range(nt)), nt
        # each XCD's workgroups (b & 7) take a contiguous run, the first nt & 7 XCDs one tile more
        for xcd in range(S.XCDS):
            run = [S.xcd_tile(b, nt) for b in range(xcd, nt, S.XCDS)]
            assert run == list(range(run[0], run[0] + len(run))) if run else True
            assert len(run) == nt // S.XCDS + (1 if xcd < nt % S.XCDS else 0)


def test_up_table():
    rows = {c.dims[2] for c in S.UP if c.dims[:2] == (1, 1)}
    assert rows >= {1, 31, 32, 33, 127, 128, 129, 255, 256, 257}
    assert {c.dims for c in S.UP} >= {(3, 7, 13), (5, 9, 11), (4, 16, 16), (9, 15, 17)}
    assert [_q(c) for c in S.UP if c.dims in ((3, 7, 13), (5, 9, 11), (4, 16, 16), (9, 15, 17))] == [273, 495, 1024, 2295]
    assert {c.cin for c in S.UP} >= {8, 16, 24, 48, 64} and {c.cout for c in S.UP} >= {64, 24, 8}
    assert {S.nchunk(c.cin) for c in S.UP} == {1, 2, 3, 4}
    assert all(S.nchunk(c.cin) <= 4 for c in S.UP)                                      # up8_launch: cin_pad <= 64
    # every wave-quarter boundary: a case whose last tile ends on each of the eight, and one position either side of the first
    # quarter's and of the half's
    ends = {_q(c) % S.TILE for c in S.UP}
    assert ends >= {(S.QUARTER * k) % S.TILE for k in range(1, 9)}
    assert ends >= {31, 33, 127, 129}
    for c in S.UP:
        tile, half, quarter, lane = S.up_place(_q(c) - 1)
        assert tile == S.ntiles(_q(c)) - 1 and 0 <= half < 2 and 0 <= quarter < 4 and 0 <= lane < 32


def test_down_table():
    assert {_q(c) for c in S.DOWN} >= {1, 129, 255, 256, 257, 2322}
    assert {c.cin for c in S.DOWN} >= {64, 24, 8} and all(c.cin == c.cout for c in S.DOWN)
    odd = [c for c in S.DOWN if c.dims == (5, 7, 9)]
    assert odd and S.out_dims("down", odd[0].dims) == (2, 3, 4)


def test_skip_table():
    assert {(c.cin, c.cout) for c in S.SKIP} >= {(128, 64), (64, 3), (3, 64)}
    assert all(c.crop == 2 for c in S.SKIP)
    assert all(c.has_dx == (c.cin > 3) for c in S.SKIP)
    # the pitched count: a case whose valid outputs are fewer than its flat positions (rows and planes masked)
    assert any(_q(c) > np.prod(S.out_dims("skip", c.dims, c.crop)) for c in S.SKIP)


def test_stem_table():
    tl = {c.name: S.stem_tiling(c.dims) for c in S.STEM}
    assert all(1 <= t.Dv <= 4 and t.Hv >= 1 for t in tl.values())
    edge = {t.Wv for t in tl.values() if t.Dv <= 3 and t.Hv <= 3}
    assert edge >= {1, 31, 32, 33, 127, 128, 129, 257}
    assert {t.Wv % S.STEM_COLS for t in tl.values()} >= {S.STEM_WAVE * k % S.STEM_COLS for k in range(1, 5)}   # every wave boundary
    nts = [t.nt for t in tl.values()]
    assert any(nt < 512 for nt in nts) and 512 in nts and 513 in nts and any(nt >= 1537 for nt in nts)
    assert tl["stem-nt1548"].nt == 1548
    assert {t.tnx for t in tl.values()} >= {1, 2, 3}
    assert {t.walks for t in tl.values()} >= {1, 2} and max(t.walks for t in tl.values()) >= 3
    assert {c.cout for c in S.STEM} >= {64, 24, 8} and {c.cin for c in S.STEM} >= {3, 2, 1}
    assert all(c.cin <= 3 and c.cout <= 64 and not c.has_dx for c in S.STEM)           # packs_stem
    # the cases that run on every (arithmetic, velocity) combination: a ragged, a whole and a second tile per row; one, two and
    # three or more tiles per workgroup
    rep = [tl[c.name] for c in S.STEM if c.rep]
    assert {1, 2} <= {t.walks for t in rep} and max(t.walks for t in rep) >= 3
    assert {0, 1} <= {t.Wv % S.STEM_COLS for t in rep} and any(t.Wv % S.STEM_COLS > 1 for t in rep)
    # where voxels sit: the last voxel of the 513-tile case is workgroup 0's second tile, in the other patch buffer
    t = tl["stem-nt513"]
    assert S.stem_place(t, t.Dv - 1, t.Hv - 1, t.Wv - 1)[:3] == (512, 1, 1)
    t = tl["stem-nt1548"]
    assert S.stem_place(t, t.Dv - 1, t.Hv - 1, t.Wv - 1)[:3] == (1547, 3, 1) and S.stem_place(t, 2, 100, 0)[1:3] == (2, 0)


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_oracle_evaluates_the_case_and_its_backends_agree(case):
    x, dx, w, dw, b = (None if a is None else a.astype(np.float64) for a in S.operands(case))
    y, dy = L.conv_layer_vel(case.kind, x, dx, w, dw, b)
    with L.backend('torch'):
        yt, dyt = L.conv_layer_vel(case.kind, x, dx, w, dw, b)
    want = S.out_dims(case.kind, case.dims, case.crop)
    if case.kind == "up":
        want = tuple(2 * n for n in want)
    if case.crop:
        cr = slice(case.crop, -case.crop)
        y, dy, yt, dyt = (a[:, cr, cr, cr] for a in (y, dy, yt, dyt))
    assert y.shape == dy.shape == (case.cout,) + want
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(dy))
    assert np.abs(y - yt).max() <= 1e-12 and np.abs(dy - dyt).max() <= 1e-12
    assert np.array_equal(L.conv_layer(case.kind, x, w, b)[(slice(None),) + ((cr,) * 3 if case.crop else ())], y)
