"""One-process rig of the z-slab brick protocol (test infrastructure; include/nbe.h, "Brick mode").

ShardedBox._process_zbrick drives nbe_brick_encode -> _interior -> _exchange -> _finish on one rank per GPU and moves the
faces with torch.distributed.  Here the ranks are Engines of ONE process on one card, one per brick, and an exchange is a
device copy: recv_lo of brick i is send_hi of brick i - 1, recv_hi of brick i is send_lo of brick i + 1 (periodic), for the
down_l0 faces, the down_l1 faces and the skip-connection planes alike.  Everything runs on torch's current stream, which
orders the four calls of every context against the copies.  The bricks may differ in depth.

Every send buffer is filled with 0xFF bytes before its owner writes it -- a NaN in float32 and in float16 -- so a receiver
that consumes a byte no sender wrote (the padding of a plane stride, the words behind the range tag, a plane too many)
shows up as a NaN in the fields or as a range flag: a finding about the face layout, never a flake."""

import torch

RAW_HALO = 4            # planes of raw input a brick reads from either z neighbour (Engine.RAW_HALO)


def origins_of(depths):
    o, out = 0, []
    for b in depths:
        out.append(o)
        o += int(b)
    return out


def haloed_brick(box, origin, depth):
    """(C, depth + 8, S1, S2): the brick's own planes of the periodic box with 4 raw planes per side."""
    D = box.shape[1]
    idx = (torch.arange(origin - RAW_HALO, origin + depth + RAW_HALO, device=box.device) % D)
    return box.index_select(1, idx).contiguous()


class _Faces:
    """The twelve buffers of one brick: (send_lo, send_hi, recv_lo, recv_hi) of the three exchanges."""

    def __init__(self, eng, bshape, device):
        self.n = [eng.brick_halo_bytes(bshape, w) for w in (1, 2, 3)]
        mk = lambda k: [torch.empty(k, dtype=torch.uint8, device=device) for _ in range(4)]
        self.f1, self.f2, self.f3 = mk(self.n[0]), mk(self.n[1]), mk(self.n[2])

    def poison_sends(self):
        for f in (self.f1, self.f2, self.f3):
            f[0].fill_(0xFF)
            f[1].fill_(0xFF)


def _move(faces, which):
    """send_lo / send_hi of every brick -> recv_hi of its z-minus neighbour / recv_lo of its z-plus neighbour."""
    N = len(faces)
    for i in range(N):
        mine, minus, plus = getattr(faces[i], which), getattr(faces[(i - 1) % N], which), getattr(faces[(i + 1) % N], which)
        assert mine[2].numel() == minus[1].numel() and mine[3].numel() == plus[0].numel(), "the bricks size their faces differently"
        mine[2].copy_(minus[1])                                  # recv_lo <- the z-minus neighbour's send_hi
        mine[3].copy_(plus[0])                                   # recv_hi <- the z-plus neighbour's send_lo


def run_bricks(engines, box, depths, Dz, vel_fac):
    """box: periodic (3, sum(depths), S1, S2) float32 CUDA tensor; engines: one Engine per brick, same parameters and
    cosmology.  Returns the assembled (disp, vel); vel is None for displacement-only engines."""
    depths = [int(b) for b in depths]
    assert len(engines) == len(depths) and box.is_cuda and box.shape[1] == sum(depths)
    S1, S2 = int(box.shape[2]), int(box.shape[3])
    with_vel = engines[0].compute_vel
    shapes = [(b, S1, S2) for b in depths]
    amax = float(box.abs().max())
    try:
        for e in engines:
            e.set_input_range(amax)
        faces = [_Faces(e, s, box.device) for e, s in zip(engines, shapes)]
        # NaN-filled outputs: a voxel that brick_finish does not write cannot pass for a computed one
        disp = [torch.full((3,) + s, float("nan"), device=box.device) for s in shapes]
        vel = [torch.full((3,) + s, float("nan"), device=box.device) if with_vel else None for s in shapes]
        for e, f, s, o in zip(engines, faces, shapes, origins_of(depths)):
            f.poison_sends()
            e.brick_encode(haloed_brick(box, o, s[0]), s, Dz, vel_fac, f.f1[0], f.f1[1], f.f3[0], f.f3[1])
        _move(faces, "f1")
        _move(faces, "f3")
        for e in engines:
            e.brick_interior()
        for e, f in zip(engines, faces):
            e.brick_exchange(f.f1[2], f.f1[3], f.f2[0], f.f2[1])
        _move(faces, "f2")
        for e, f, d, v in zip(engines, faces, disp, vel):
            e.brick_finish(f.f2[2], f.f2[3], f.f3[2], f.f3[3], Dz, vel_fac, d, v)
        for e in engines:
            e.check_finite()
    finally:
        for e in engines:
            e.set_input_range(None)
    return torch.cat(disp, 1), (torch.cat(vel, 1) if with_vel else None)
