#!/usr/bin/env python
"""Batch driver: seeds and a tabulated linear P(k) to the displacement files `run_emulator --displacement_files` reads.

The reference draws its linear field inside its pipeline (`scripts/core.py:263-302`: white noise coloured with the CLASS
table) and hands it to first-order LPT.  Here the draw, the displacement and the field all come from the GPU (lpt.py,
`linear_ics`), so a seed and a P(k) table are the only inputs of a run:

    python -m jax_nbody_emulator_with_dj_amd.ic_input \\
        --seeds 1:9 --output_dirs '/path/to/sims/seed_{seed}' --npart 512 --pk_table class_linear_pk_z0_table.txt \\
        --boxsize 1000 --z 0.5 --omega_m 0.3175 --paired

    --seeds          '1,2,3', or 'A:B' for A, A+1, ..., B-1
    --output_dirs    a pattern with {seed} (directories are created), or a glob that matches as many directories as seeds
    --pk_table       the two columns k [h/Mpc] and P(k) [(Mpc/h)^3] the reference writes with np.savetxt
    output           <dir>/lpt_dis.npy (3, N, N, N) float32, <dir>/delta_linear.npy (N, N, N) float32 (not with
                     --no-save-delta) and <dir>/ic_metadata.json (seed, n, boxsize, scale, flags, table file)

`--scale S` multiplies the field; `--z Z --omega_m OM` set it to growth_factor(Z, OM) / growth_factor(0, OM) instead, for a
table given at z = 0.  `--fixed_amplitude` draws the Quijote "fixed" fields; `--paired` writes the phase-inverted partner
as a second set under <dir>_paired.  `--white_noise_file FILE` colours that (N, N, N) field (e.g. the reference's
white_noise_ngenic.npy) instead of drawing: one output directory, no --seeds, no --fixed_amplitude.
`--lpt_order 2` also writes <dir>/lpt2_dis.npy, the second-order displacement (lpt.lpt2_displacement): `--growth2 G` is
-D_2 / D_1^2, by default that of `--z Z --omega_m OM` (cosmology.growth_factor_2) and 3/7 without them; `--lpt2_dealias`
forms the quadratic source on the mesh of 3 N / 2.  lpt_dis.npy, the emulator's input, stays first order; the order and G
are recorded in ic_metadata.json.
"""

import argparse
import json
import sys
from glob import glob
from pathlib import Path

import numpy as np

from .lpt_input import lpt2_options, read_table


def seed_list(text):
    """'1,2,3' -> [1, 2, 3]; '4:7' -> [4, 5, 6]."""
    try:
        if ':' in text:
            a, b = (int(t) for t in text.split(':'))
            seeds = list(range(a, b))
        else:
            seeds = [int(t) for t in text.split(',')]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected 'A,B,C' or 'A:B', got '{text}'")
    if not seeds:
        raise argparse.ArgumentTypeError(f"no seeds in '{text}'")
    if len(set(seeds)) != len(seeds):
        raise argparse.ArgumentTypeError(f"repeated seeds in '{text}'")
    return seeds


def build_parser():
    ap = argparse.ArgumentParser(
        description="Draw linear density fields from seeds and write them with their Zel'dovich displacements.",
        formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--seeds', type=seed_list, default=None, help="Seeds: '1,2,3' or 'A:B' (A .. B-1)")
    ap.add_argument('--output_dirs', type=str, required=True,
                    help='Output directories: a pattern with {seed}, or a glob matching one directory per seed')
    ap.add_argument('--npart', type=int, required=True, help='Particle grid size N: the output is (3, N, N, N)')
    ap.add_argument('--pk_table', type=str, required=True, help='Two-column text file k, P(k) of the linear spectrum')
    ap.add_argument('--boxsize', type=float, default=1000.0, help='Box size in Mpc/h (default: 1000.0, Quijote)')
    ap.add_argument('--scale', type=float, default=None, help='Factor on the field, e.g. a growth factor (default: 1)')
    ap.add_argument('--z', type=float, default=None, help='With --omega_m: scale = D(z) / D(0)')
    ap.add_argument('--omega_m', type=float, default=None, help='With --z: the matter density of the growth factor')
    ap.add_argument('--fixed_amplitude', action='store_true', help='|delta_k| = sigma for every mode (Quijote "fixed")')
    ap.add_argument('--paired', action='store_true', help='Also write the phase-inverted partner under <dir>_paired')
    ap.add_argument('--white_noise_file', type=str, default=None,
                    help='Colour this (N, N, N) white-noise field instead of drawing one (no --seeds)')
    ap.add_argument('--lpt_order', type=int, default=1, help='2: also write lpt2_dis.npy, the second-order displacement')
    ap.add_argument('--growth2', type=float, default=None,
                    help='With --lpt_order 2: -D_2 / D_1^2 (default: from --z / --omega_m, else 3/7)')
    ap.add_argument('--lpt2_dealias', action='store_true', help='With --lpt_order 2: form the source on the mesh of 3 N / 2')
    ap.add_argument('--no-save-delta', dest='save_delta', action='store_false', help='Do not write delta_linear.npy')
    return ap


def output_dirs(pattern, seeds):
    """One directory per seed (None: one directory for a white-noise file): the pattern formatted with {seed}, or the
    sorted matches of a glob."""
    if '{seed}' in pattern:
        if seeds is None:
            raise ValueError('--output_dirs with {seed} needs --seeds')
        return [Path(pattern.format(seed=s)) for s in seeds]
    paths = sorted(Path(p) for p in glob(pattern))
    want = 1 if seeds is None else len(seeds)
    if len(paths) != want or not all(p.is_dir() for p in paths):
        raise ValueError('Number of directories must match:\n'
                         f'  seeds: {want}\n  output_dirs: {len(paths)} matching {pattern}')
    return paths


def growth_scale(z, omega_m):
    from .cosmology import growth_factor
    from . import lpt
    z = lpt._real(z, '--z')
    omega_m = lpt._real(omega_m, '--omega_m', positive=True)
    if z <= -1.0 or omega_m > 1.0:
        raise ValueError(f'--z {z} must be above -1 and --omega_m {omega_m} at most 1 (flat LambdaCDM)')
    return float(growth_factor(z, omega_m)) / float(growth_factor(0.0, omega_m))


def growth2_of(z, omega_m):
    """-D_2 / D_1^2 at z in flat LambdaCDM: cosmology.growth_factor_2 over the square of the float64 growth factor."""
    from .cosmology import growth_factor_2, _growth_factor64
    d1 = float(_growth_factor64(float(z), float(omega_m)))
    return -float(growth_factor_2(z, omega_m)) / (d1 * d1)


def validate(args):
    """Every argument error before any file is written or any device work: (seeds or None, dirs, k, pk, scale, growth2);
    growth2 is None for a first-order run."""
    from . import lpt
    lpt._size(args.npart, '--npart')
    lpt._real(args.boxsize, '--boxsize', positive=True)
    if args.scale is not None and (args.z is not None or args.omega_m is not None):
        raise ValueError('--scale and --z / --omega_m are mutually exclusive')
    if (args.z is None) != (args.omega_m is None):
        raise ValueError('--z and --omega_m go together')
    scale = growth_scale(args.z, args.omega_m) if args.z is not None else 1.0 if args.scale is None else args.scale
    scale = lpt._real(scale, '--scale', positive=True)
    if args.lpt_order not in (1, 2):
        raise ValueError(f'--lpt_order must be 1 or 2, got {args.lpt_order}')
    growth2 = lpt2_options(args, args.lpt_order == 2, '--lpt_order 2')
    if args.lpt_order == 2 and args.growth2 is None and args.z is not None:
        growth2 = growth2_of(args.z, args.omega_m)
    if args.white_noise_file is not None:
        if args.seeds is not None:
            raise ValueError('--white_noise_file colours a given field: --seeds is not allowed')
        if args.fixed_amplitude:
            raise ValueError('--white_noise_file colours a given field: --fixed_amplitude is not allowed')
    elif args.seeds is None:
        raise ValueError('one of --seeds and --white_noise_file is needed')
    else:
        for s in args.seeds:
            lpt._seed(s)
    dirs = output_dirs(args.output_dirs, args.seeds)
    k, pk = read_table(args.pk_table)
    lpt._validate_table(k, pk)
    return args.seeds, dirs, k, pk, scale, growth2


def read_white(path, n):
    try:
        w = np.load(path)
    except Exception as e:
        sys.exit(f'--white_noise_file {path} cannot be read: {e}')
    if w.ndim != 3 or w.shape != (n, n, n):
        sys.exit(f'in file {path}: the white-noise field must have shape ({n}, {n}, {n}), got {w.shape}')
    if not np.issubdtype(w.dtype, np.floating):
        sys.exit(f'in file {path}: the white-noise field must be real, got {w.dtype}')
    return np.ascontiguousarray(w, dtype=np.float32)


def write_set(out_dir, delta, psi, meta, save_delta, psi2lpt=None):
    out_dir.mkdir(parents=True, exist_ok=True)
    np.save(out_dir / 'lpt_dis.npy', psi.cpu().numpy())
    if psi2lpt is not None:
        np.save(out_dir / 'lpt2_dis.npy', psi2lpt.cpu().numpy())
    if save_delta:
        np.save(out_dir / 'delta_linear.npy', delta.cpu().numpy())
    with open(out_dir / 'ic_metadata.json', 'w') as f:
        json.dump(meta, f, indent=1)


def paired_dir(out_dir):
    return out_dir.parent / (out_dir.name + '_paired')


def run(args):
    from . import lpt
    try:
        seeds, dirs, k, pk, scale, growth2 = validate(args)
    except ValueError as e:
        sys.exit(str(e))
    n, L = args.npart, args.boxsize
    meta = dict(n=n, boxsize=L, scale=scale, fixed_amplitude=bool(args.fixed_amplitude), invert_phase=False,
                pk_table=str(args.pk_table), seed=None, white_noise_file=args.white_noise_file,
                lpt_order=args.lpt_order, growth2=growth2)
    second = dict(growth2=growth2, dealias=bool(args.lpt2_dealias))
    if args.white_noise_file is not None:
        import torch
        from .density import _device
        white = read_white(args.white_noise_file, n)
        signs = (1.0, -1.0) if args.paired else (1.0,)
        for sign in signs:
            w = torch.from_numpy(white if sign > 0 else -white).to(_device())
            delta = lpt.colour_noise(w, L, k, pk, scale=scale)
            psi = lpt.zeldovich_displacement(delta, boxsize=L)
            psi2lpt = lpt.lpt2_displacement(delta, boxsize=L, **second) if growth2 is not None else None
            out_dir = dirs[0] if sign > 0 else paired_dir(dirs[0])
            write_set(out_dir, delta, psi, dict(meta, invert_phase=sign < 0), args.save_delta, psi2lpt)
            print(f'{args.white_noise_file} -> {out_dir / "lpt_dis.npy"}')
        print('\nDone!')
        return
    print(f'Drawing {len(seeds)} field(s) of {n}^3 in a {L} Mpc/h box, scale {scale:.6g}')
    for i, (seed, out_dir) in enumerate(zip(seeds, dirs)):
        for invert in ((False, True) if args.paired else (False,)):
            draw = dict(scale=scale, fixed_amplitude=args.fixed_amplitude, invert_phase=invert,
                        return_delta=args.save_delta)
            if growth2 is None:
                (delta, psi), psi2lpt = lpt.linear_ics(n, L, k, pk, seed, **draw), None
            else:
                delta, psi, psi2lpt = lpt.linear_ics(n, L, k, pk, seed, order=2, **second, **draw)
            target = paired_dir(out_dir) if invert else out_dir
            write_set(target, delta, psi, dict(meta, seed=seed, invert_phase=invert), args.save_delta, psi2lpt)
            print(f'[{i + 1}/{len(seeds)}] seed {seed}{" (paired)" if invert else ""} -> {target / "lpt_dis.npy"}')
    print('\nDone!')


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == '__main__':
    main()
