#!/usr/bin/env python
"""Batch driver: many (cosmology, displacement) file pairs through one resident engine.

Same command line, file formats, range checks and output names as the reference's
`examples/run_jax_emulator.py` (:196-262 arguments, :117-139 cosmology files and ranges,
:265-355 loop):

    python -m jax_nbody_emulator_with_dj_amd.run_emulator \\
        --cosmo_param_files '/path/to/sims/*/params.npy' \\
        --displacement_files '/path/to/sims/*/dis.npy' \\
        --output_dirs '/path/to/sims/*/' \\
        --ndiv 4,2,2 --precision f16 --vel

    cosmology file   (6,)  [Omega_m, Omega_b, h, n_s, sigma_8, redshift]; Omega_m in [0.1, 0.5], z in [0, 3]
    displacement     (3, N0, N1, N2) z = 0 linear (ZA) displacement field
    outputs          <output_dir>/emu_dis.npy  and, with --vel, <output_dir>/emu_vel.npy

Density fields (the fork's DISCO-DJ step, scripts/core.py:447-458): with `--density_res N` every box also writes
<output_dir>/emu_delta.npy, the emulated displacement painted onto an N^3 mesh on the GPU (density.py; `--mas_worder`
1-4 = NGP/CIC/TSC/PCS, default 2; `--no-deconvolve` keeps the assignment window; `--boxsize` in Mpc/h, default 1000),
with `--pk` <output_dir>/emu_pk.npz (k, pk, nmodes), and with `--minkowski` <output_dir>/emu_minkowski.npz
(thresholds, v0, v1, v2, v3, counts, mean, std: the Minkowski functionals of the painted delta at the 41 default
thresholds of the standardized field, computed on the device by density.minkowski_functionals).  With `--bispectrum`
<output_dir>/emu_bispectrum.npz holds density.bispectrum's arrays for the reference's two configurations
(scripts/utils.py:1314-1399: k1 = k2 = 0.1 and k1 = 0.05, k2 = 0.1 h/Mpc, theta = linspace(0, pi, 25)), keys suffixed
_cfg1 and _cfg2; with `--onepoint` <output_dir>/emu_onepoint.npz holds mean, std, skewness, kurtosis_excess
(density.field_statistics) and a 120-bin PDF between the field's minimum and maximum (density.field_pdf: edges, centers,
counts, pdf, outside, nonfinite).  With `--vel`, `--paint_vel` writes <output_dir>/emu_vel_mesh.npy, the (3, N, N, N)
mass-weighted mean velocity on the same mesh (density.paint_field, normalize="density", not deconvolved), and `--rsd AXIS`
writes <output_dir>/emu_delta_rsd.npy, the density with every particle moved by v_AXIS (1 + z) / H(z) along array axis
AXIS (density.rsd_factor of the box's own redshift and Omega_m; `--mas_worder` and `--no-deconvolve` apply), and with
`--pk` its power spectrum <output_dir>/emu_pk_rsd.npz.  With `--rsd`, `--pk_multipoles` writes
<output_dir>/emu_pk_rsd_multipoles.npz (k, p0, p2, p4, nmodes: density.power_spectrum_multipoles of emu_delta_rsd about
AXIS) and `--pk_wedges NMU` writes <output_dir>/emu_pk_rsd_wedges.npz (k, mu, pk, nmodes, mu_edges:
density.power_spectrum_wedges in NMU bins of |mu|, 1 .. 64).  Painting reads the float32 displacement on the device; the saved emu_dis.npy is
rounded to --output-precision afterwards.

Halos (the fork's scripts/halos.py): `--fof` writes <output_dir>/fof_catalog.npz, the friends-of-friends catalogue of the
emulated displacement (halos.fof_halos on the device tensor, no host copy of the field; the reference's keys CMPosition,
Npart, Mass, BoxSize, NpartPerDim, LinkingLength, AbsoluteLinking, Nmin).  `--fof_linking_length B` (default 0.2, in units
of the mean particle spacing) and `--fof_nmin N` (default 20) set the finder; the box size is `--boxsize` and Omega_m the
cosmology file's.  It needs a cubic box and works with or without --density_res.  With `--fof`, `--halo_pk RES` paints the
halos (halos.paint_halos; `--halo_weight number|length`) and the matter (density.paint_density of the same displacement,
`--mas_worder`) onto one RES^3 mesh and writes <output_dir>/halo_delta.npy and <output_dir>/halo_pk.npz (k, p_hh, p_mm,
p_hm, r, bias, nmodes, shot_noise, count: density.cross_correlation of the two fields), and `--halo_xi` counts the halo
pairs (halos.halo_correlation; `--xi_rmin 1 --xi_rmax 50 --xi_nbins 20 [--xi_log] [--xi_nmu N]`) and writes
<output_dir>/halo_xi.npz (r_edges, r_mid, npairs, rr, xi, count, with --xi_nmu mu_edges, xi0, xi2,
xi4), and `--halo_profiles` counts the matter in shells about every halo (halos.halo_profiles; `--profile_rmin 0.05
--profile_rmax 5 --profile_nbins 20 [--so_overdensity 200 --so_reference mean|critical]`) and writes
<output_dir>/halo_profiles.npz (r_edges, r_mid, counts, rho, Length, R_delta, N_delta, M_delta, flag, overdensity,
reference, count; the spherical-overdensity radii and masses at the box's redshift), and with `--vel` `--halo_vprofiles`
writes <output_dir>/halo_vprofiles.npz (halos.halo_velocity_profiles in the shells of --profile_*: r_edges, r_mid, counts,
sums, exponent, v_r, sigma_r, sigma_t, Length, count) and `--halo_v12` <output_dir>/halo_v12.npz
(halos.halo_pairwise_velocity in the bins of --xi_*: r_edges, r_mid, npairs, sums, exponent, v12, sigma_r, sigma_t, count),
the catalogue's CMVelocity coming from the emulated velocity; a box without a halo writes none of these and says so.  With `--fof`, `--halo_environment RES` paints the matter onto a
RES^3 mesh (`--mas_worder`, deconvolved) and writes <output_dir>/halo_environment.npz (halos.halo_environment with the NGP
readout: eigenvalues, delta_s, web_type, Length, count, smoothing, threshold).  With `--density_res`, `--cosmic_web` writes
the T-web of emu_delta (web.cosmic_web with mass = emu_delta): <output_dir>/emu_web_type.npy (uint8, the first threshold)
and <output_dir>/emu_web.npz (thresholds, counts, volume_fraction, mass_fraction, smoothing); `--web_smoothing R` is the
Gaussian length in Mpc/h (default: two cells of the mesh) and `--web_threshold T [T ...]` the eigenvalue thresholds (default
0; --halo_environment reads the first).  `--xcorr FILE` (with --density_res) writes <output_dir>/emu_xcorr.npz, density.cross_correlation of
emu_delta against the saved (N, N, N) field FILE (k, p_aa, p_bb, p_ab, nmodes, r, transfer, bias): the reference's
emulator-against-target check (scripts/utils.py:1451-1470).

What differs from the reference: the engine, its weights and its ~100 GB workspace stay resident on the
GPU for the whole batch, and disk I/O overlaps compute -- the next displacement file is read and the
previous results are written by a background thread while the GPU works on the current box.
`--params FILE.npz` names the parameter tree ({'params': {...}} saved with np.savez, the reference's own
format); without it the default blob is looked up as in `load_default_parameters()`.
"""

import argparse
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from glob import glob
from pathlib import Path

import numpy as np

OM_RANGE = (0.1, 0.5)
Z_RANGE = (0.0, 3.0)


def _die(msg):
    sys.exit(msg)


def _check_file(path):
    if not path.is_file():
        _die(f'Input file path is not a readable file: {path}')
    try:
        with path.open('rb'):
            pass
    except Exception as e:
        _die(f'Input file cannot be read: {path} ({e})')


def _check_dir(path):
    if not path.is_dir():
        _die(f'Output directory path is not a directory: {path}')
    probe = path / '.write_test'
    try:
        with probe.open('w'):
            pass
        probe.unlink()
    except Exception as e:
        _die(f'Output directory is not writable: {path} ({e})')


def files_matching(pattern):
    paths = sorted(Path(p) for p in glob(pattern))
    if not paths:
        raise argparse.ArgumentTypeError(f'No files match pattern: {pattern}')
    for p in paths:
        _check_file(p)
    return paths


def dirs_matching(pattern):
    paths = sorted(Path(p) for p in glob(pattern))
    if not paths:
        raise argparse.ArgumentTypeError(f'No directories match pattern: {pattern}')
    for p in paths:
        _check_dir(p)
    return paths


def divisions(text):
    """'4' -> (4,4,4); '2,4,4' or '(2, 4, 4)' -> (2,4,4)."""
    vals = [int(t) for t in text.strip('()').split(',')]
    if len(vals) == 1:
        return (vals[0],) * 3
    if len(vals) == 3:
        return tuple(vals)
    raise argparse.ArgumentTypeError(f'Expected 1 or 3 values, got {len(vals)}')


def precision(text):
    table = {'f16': np.float16, 'f32': np.float32}
    if text not in table:
        raise argparse.ArgumentTypeError(f"precision must be 'f32' or 'f16', got '{text}'")
    return table[text]


def read_cosmology(path):
    """(Omega_m, z) from a (6,) array [Om, Ob, h, ns, s8, z], with the reference's validity ranges."""
    data = np.load(path)
    Om, z = float(data[0]), float(data[-1])
    if not OM_RANGE[0] <= Om <= OM_RANGE[1]:
        _die(f'in file {path}: Om={Om:.4f} out of valid range [0.1, 0.5]')
    if not Z_RANGE[0] <= z <= Z_RANGE[1]:
        _die(f'in file {path}: z={z:.4f} out of valid range [0.0, 3.0]')
    return Om, z


def displacement_shape(path, expected):
    shape = np.load(path, mmap_mode='r').shape
    if len(shape) != 4:
        _die(f'in file {path}: input array ndim {len(shape)} is not 4')
    if shape[0] != 3:
        _die(f'in file {path}: first dimension {shape[0]} is not 3 (expected 3 displacement components)')
    if expected is not None and shape != expected:
        _die(f'in file {path}: input array shape {shape} differs from first file shape {expected}')
    return shape


def build_parser():
    ap = argparse.ArgumentParser(
        description='Batch process displacement fields with the MI355X N-body emulator engine.',
        formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--cosmo_param_files', type=files_matching, required=True,
                    help='Glob pattern for cosmology parameter files (numpy arrays with [Om, Ob, h, ns, s8, z])')
    ap.add_argument('--displacement_files', type=files_matching, required=True,
                    help='Glob pattern for input displacement files (numpy arrays with shape [3, N, N, N])')
    ap.add_argument('--output_dirs', type=dirs_matching, required=True, help='Glob pattern for output directories')
    ap.add_argument('--ndiv', type=divisions, required=True,
                    help='Number of subbox divisions: single int (e.g., 4) or tuple (e.g., 2,4,4)')
    ap.add_argument('--vel', action=argparse.BooleanOptionalAction, default=True,
                    help='Compute velocity field in addition to displacement (default: True)')
    ap.add_argument('--style', action=argparse.BooleanOptionalAction, default=True,
                    help='Use style modulation for flexible cosmology; if False, premodulate parameters '
                         'for each cosmology (default: True)')
    ap.add_argument('--precision', type=precision, default=np.float32,
                    help='Model precision: f16 (half) or f32 (full) (default: f32)')
    ap.add_argument('--output-precision', type=precision, default=np.float16, dest='output_precision',
                    help='Output file precision: f16 (half) or f32 (full) (default: f16).')
    ap.add_argument('--quiet', '-q', action='store_true', help='Suppress progress bars (useful for batch jobs)')
    ap.add_argument('--params', type=Path, default=None,
                    help="Parameter tree: flat .npz (block/layer/leaf arrays, see params_io.py) or the reference's "
                         ".npz with a pickled {'params': ...} dict (read with a restricted unpickler); "
                         'default: the packaged pretrained blob')
    # density fields: absent from the Namespace unless given, so that runs without them are exactly today's
    ap.add_argument('--density_res', type=mesh_size, default=argparse.SUPPRESS,
                    help='Also paint the emulated displacement onto an N^3 mesh: <output_dir>/emu_delta.npy (float32)')
    ap.add_argument('--boxsize', type=float, default=argparse.SUPPRESS,
                    help='Box size in Mpc/h for --density_res (default: 1000.0, Quijote)')
    ap.add_argument('--mas_worder', type=int, choices=(1, 2, 3, 4), default=argparse.SUPPRESS,
                    help='Mass assignment for --density_res: 1 NGP, 2 CIC, 3 TSC, 4 PCS (default: 2)')
    ap.add_argument('--deconvolve', action=argparse.BooleanOptionalAction, default=argparse.SUPPRESS,
                    help='Deconvolve the mass assignment window (default: True)')
    ap.add_argument('--pk', action='store_true', default=argparse.SUPPRESS,
                    help='With --density_res: also write the power spectrum to <output_dir>/emu_pk.npz (k, pk, nmodes)')
    ap.add_argument('--minkowski', action='store_true', default=argparse.SUPPRESS,
                    help='With --density_res: also write the Minkowski functionals of the density field (standardized, '
                         '41 thresholds in [-3, 3]) to <output_dir>/emu_minkowski.npz')
    ap.add_argument('--bispectrum', action='store_true', default=argparse.SUPPRESS,
                    help='With --density_res: also write B and Q(theta) of the density field for k1 = k2 = 0.1 and '
                         'k1 = 0.05, k2 = 0.1 h/Mpc at 25 angles to <output_dir>/emu_bispectrum.npz')
    ap.add_argument('--onepoint', action='store_true', default=argparse.SUPPRESS,
                    help='With --density_res: also write mean, std, skewness, excess kurtosis and a 120-bin PDF of the '
                         'density field to <output_dir>/emu_onepoint.npz')
    ap.add_argument('--paint_vel', action='store_true', default=argparse.SUPPRESS,
                    help='With --vel and --density_res: also write the mass-weighted mean velocity on the density mesh to '
                         '<output_dir>/emu_vel_mesh.npy (3, N, N, N)')
    ap.add_argument('--rsd', type=int, choices=(0, 1, 2), metavar='AXIS', default=argparse.SUPPRESS,
                    help='With --vel and --density_res: also write the redshift-space density along array axis AXIS to '
                         '<output_dir>/emu_delta_rsd.npy (and with --pk <output_dir>/emu_pk_rsd.npz)')
    ap.add_argument('--pk_multipoles', action='store_true', default=argparse.SUPPRESS,
                    help='With --rsd: also write the monopole, quadrupole and hexadecapole of the redshift-space density '
                         'about AXIS to <output_dir>/emu_pk_rsd_multipoles.npz (k, p0, p2, p4, nmodes)')
    ap.add_argument('--pk_wedges', type=int, metavar='NMU', default=argparse.SUPPRESS,
                    help='With --rsd: also write the power spectrum of the redshift-space density in NMU wedges of |mu| '
                         'about AXIS to <output_dir>/emu_pk_rsd_wedges.npz (k, mu, pk, nmodes, mu_edges)')
    ap.add_argument('--fof', action='store_true', default=argparse.SUPPRESS,
                    help='Also write the friends-of-friends halo catalogue of the emulated displacement to '
                         '<output_dir>/fof_catalog.npz (box size from --boxsize, Omega_m from the cosmology file)')
    ap.add_argument('--fof_linking_length', type=float, default=argparse.SUPPRESS,
                    help='With --fof: linking length in units of the mean particle spacing (default: 0.2)')
    ap.add_argument('--fof_nmin', type=int, default=argparse.SUPPRESS,
                    help='With --fof: smallest particle count of a halo (default: 20)')
    ap.add_argument('--halo_pk', type=mesh_size, metavar='RES', default=argparse.SUPPRESS,
                    help='With --fof: also write the halo density on a RES^3 mesh to <output_dir>/halo_delta.npy and its '
                         'spectra against the matter field to <output_dir>/halo_pk.npz')
    ap.add_argument('--halo_weight', choices=('number', 'length'), default=argparse.SUPPRESS,
                    help='With --halo_pk: count halos, or weight each by its particle count (default: number)')
    from .halos import add_xi_arguments
    add_xi_arguments(ap, suppress=True)                      # --halo_xi, --xi_rmin, --xi_rmax, --xi_nbins, --xi_log, --xi_nmu
    from .halos import add_profile_arguments
    add_profile_arguments(ap, suppress=True)                 # --halo_profiles, --profile_rmin / _rmax / _nbins, --so_overdensity / _reference
    from .halos import add_velocity_arguments
    add_velocity_arguments(ap, suppress=True)                # --halo_vprofiles, --halo_v12
    from .halos import add_environment_arguments
    add_environment_arguments(ap, suppress=True, scan=True)  # --halo_environment, --web_smoothing, --web_threshold
    ap.add_argument('--cosmic_web', action='store_true', default=argparse.SUPPRESS,
                    help='With --density_res: also write the T-web of the density field (Gaussian smoothing --web_smoothing, '
                         'thresholds --web_threshold): <output_dir>/emu_web_type.npy (uint8: 0 void, 1 sheet, 2 filament, '
                         '3 knot under the first threshold) and <output_dir>/emu_web.npz (thresholds, counts, '
                         'volume_fraction, mass_fraction, smoothing)')
    ap.add_argument('--xcorr', type=Path, metavar='FILE', default=argparse.SUPPRESS,
                    help='With --density_res: also write r(k), transfer and bias of emu_delta against the saved (N, N, N) '
                         'float32 field FILE to <output_dir>/emu_xcorr.npz')
    return ap


def mesh_size(text):
    n = int(text)
    if n < 1:
        raise argparse.ArgumentTypeError(f'mesh size must be >= 1, got {n}')
    return n


def density_options(args):
    """The density-field settings of a parsed command line, or None without --density_res.  Accepts Namespaces that
    lack the density attributes (built before they existed)."""
    res = getattr(args, 'density_res', None)
    if res is None:
        if getattr(args, 'pk', False):
            _die('--pk needs --density_res')
        return None
    boxsize = float(getattr(args, 'boxsize', 1000.0))
    if not boxsize > 0:
        _die(f'--boxsize must be positive, got {boxsize}')
    return dict(res=int(res), boxsize=boxsize, worder=int(getattr(args, 'mas_worder', 2)),
                deconvolve=bool(getattr(args, 'deconvolve', True)), pk=bool(getattr(args, 'pk', False)))


def minkowski_option(args):
    """Whether --minkowski was given (read apart from density_options, whose dict it leaves as it was)."""
    on = bool(getattr(args, 'minkowski', False))
    if on and getattr(args, 'density_res', None) is None:
        _die('--minkowski needs --density_res')
    return on


BISPECTRUM_CONFIGS = ((0.1, 0.1), (0.05, 0.1))           # (k1, k2) in h/Mpc: reference scripts/utils.py:1314-1399
BISPECTRUM_KEYS = ('theta', 'k3', 'B', 'Q', 'ntriangles', 'pk', 'k', 'nmodes')
ONEPOINT_BINS = 120


def summary_options(args):
    """(bispectrum, onepoint): whether --bispectrum / --onepoint were given (read apart from density_options, whose dict
    they leave as it was)."""
    on = tuple(bool(getattr(args, name, False)) for name in ('bispectrum', 'onepoint'))
    for flag, name in zip(on, ('--bispectrum', '--onepoint')):
        if flag and getattr(args, 'density_res', None) is None:
            _die(f'{name} needs --density_res')
    return on


def velocity_options(args):
    """(paint_vel, rsd): whether --paint_vel was given, and the axis of --rsd or None (read apart from density_options,
    whose dict they leave as it was).  Both need --density_res and --vel."""
    paint_vel = bool(getattr(args, 'paint_vel', False))
    rsd = getattr(args, 'rsd', None)
    for flag, name in ((paint_vel, '--paint_vel'), (rsd is not None, '--rsd')):
        if flag and getattr(args, 'density_res', None) is None:
            _die(f'{name} needs --density_res')
        if flag and not getattr(args, 'vel', True):
            _die(f'{name} needs --vel')
    return paint_vel, (None if rsd is None else int(rsd))


MAX_WEDGES = 64                                          # density.power_spectrum_wedges: 1 <= nmu <= 64


def anisotropy_options(args):
    """(multipoles, wedges): whether --pk_multipoles was given, and the bin count of --pk_wedges or None (read apart from
    density_options, whose dict they leave as it was).  Both measure emu_delta_rsd, so both need --rsd and --density_res."""
    multipoles = bool(getattr(args, 'pk_multipoles', False))
    wedges = getattr(args, 'pk_wedges', None)
    for flag, name in ((multipoles, '--pk_multipoles'), (wedges is not None, '--pk_wedges')):
        if flag and getattr(args, 'density_res', None) is None:
            _die(f'{name} needs --density_res')
        if flag and getattr(args, 'rsd', None) is None:
            _die(f'{name} needs --rsd')
    if wedges is not None and not 1 <= int(wedges) <= MAX_WEDGES:
        _die(f'--pk_wedges must be in 1 .. {MAX_WEDGES}, got {wedges}')
    return multipoles, (None if wedges is None else int(wedges))


def velocity_fields(disp, vel, dens, paint_vel, rsd, z, Om, multipoles=False, wedges=None):
    """The arrays of emu_vel_mesh.npy, emu_delta_rsd.npy, emu_pk_rsd.npz, emu_pk_rsd_multipoles.npz and
    emu_pk_rsd_wedges.npz for the device fields of one box."""
    from .density import (paint_density, paint_field, power_spectrum, power_spectrum_multipoles, power_spectrum_wedges,
                          rsd_factor)
    out = {}
    if paint_vel:
        out['vel_mesh'] = paint_field(disp, vel, boxsize=dens['boxsize'], res=dens['res'], worder=dens['worder'],
                                      normalize='density').cpu().numpy()
    if rsd is not None:
        delta = paint_density(disp, boxsize=dens['boxsize'], res=dens['res'], worder=dens['worder'],
                              deconvolve=dens['deconvolve'], velocity=vel, los=rsd,
                              velocity_to_length=rsd_factor(z, Om))
        out['delta_rsd'] = delta.cpu().numpy()
        if dens['pk']:
            out['pk_rsd'] = power_spectrum(delta, boxsize=dens['boxsize'])
        if multipoles:
            out['pk_rsd_multipoles'] = power_spectrum_multipoles(delta, boxsize=dens['boxsize'], los=rsd)
        if wedges is not None:
            out['pk_rsd_wedges'] = power_spectrum_wedges(delta, boxsize=dens['boxsize'], los=rsd, nmu=wedges)
    return out


def fof_options(args):
    """The halo-finder settings of a parsed command line, or None without --fof (read apart from density_options, whose
    dict they leave as it was)."""
    if not getattr(args, 'fof', False):
        for name in ('fof_linking_length', 'fof_nmin'):
            if getattr(args, name, None) is not None:
                _die(f'--{name} needs --fof')
        return None
    boxsize = float(getattr(args, 'boxsize', 1000.0))
    if not boxsize > 0:
        _die(f'--boxsize must be positive, got {boxsize}')
    b, nmin = float(getattr(args, 'fof_linking_length', 0.2)), int(getattr(args, 'fof_nmin', 20))
    if not b > 0:
        _die(f'--fof_linking_length must be positive, got {b}')
    if nmin < 1:
        _die(f'--fof_nmin must be >= 1, got {nmin}')
    return dict(boxsize=boxsize, linking_length=b, nmin=nmin)


def halo_options(args):
    """The settings of --halo_pk, or None without it (read apart from fof_options, whose dict they leave as it was)."""
    res = getattr(args, 'halo_pk', None)
    if res is None:
        if getattr(args, 'halo_weight', None) is not None:
            _die('--halo_weight needs --halo_pk')
        return None
    if not getattr(args, 'fof', False):
        _die('--halo_pk needs --fof')
    from .halos import HALO_WEIGHT_NAMES
    return dict(res=int(res), worder=int(getattr(args, 'mas_worder', 2)),
                weight=HALO_WEIGHT_NAMES[getattr(args, 'halo_weight', 'number')])


def halo_xi_options(args):
    """The settings of --halo_xi (halos.xi_options: r_edges, nmu), or None without it.  It needs --fof."""
    from .halos import xi_options
    xi = xi_options(args, float(getattr(args, 'boxsize', 1000.0)), _die)
    if xi is not None and not getattr(args, 'fof', False):
        _die('--halo_xi needs --fof')
    return xi


def halo_profile_options(args):
    """The settings of --halo_profiles (halos.profile_options: r_edges, overdensity, reference), or None without it.  It
    needs --fof."""
    from .halos import profile_options
    prof = profile_options(args, float(getattr(args, 'boxsize', 1000.0)), _die)
    if prof is not None and not getattr(args, 'fof', False):
        _die('--halo_profiles needs --fof')
    return prof


def halo_velocity_options(args):
    """The settings of --halo_vprofiles and --halo_v12 (halos.velocity_moment_options: vprofiles, v12), or None without
    either.  They need --fof and --vel."""
    from .halos import velocity_moment_options
    vmom = velocity_moment_options(args, float(getattr(args, 'boxsize', 1000.0)), bool(getattr(args, 'vel', True)), _die,
                                   need='--vel')
    if vmom is not None and not getattr(args, 'fof', False):
        _die('--%s needs --fof' % ('halo_vprofiles' if vmom['vprofiles'] is not None else 'halo_v12'))
    return vmom


def halo_environment_options(args):
    """The settings of --halo_environment (halos.environment_options: res, worder, smoothing, threshold), or None without
    it.  It needs --fof."""
    from .halos import environment_options
    env = environment_options(args, float(getattr(args, 'boxsize', 1000.0)), _die, int(getattr(args, 'mas_worder', 2)))
    if env is not None and not getattr(args, 'fof', False):
        _die('--halo_environment needs --fof')
    return env


WEB_KEYS = ('thresholds', 'counts', 'volume_fraction', 'mass_fraction', 'smoothing')


def cosmic_web_options(args):
    """The settings of --cosmic_web (smoothing, thresholds), or None without it (read apart from density_options, whose
    dict they leave as it was).  It needs --density_res, and a mesh web.cosmic_web takes."""
    if not getattr(args, 'cosmic_web', False):
        return None
    res = getattr(args, 'density_res', None)
    if res is None:
        _die('--cosmic_web needs --density_res')
    if not 2 <= res <= 2048:
        _die(f'--cosmic_web needs a mesh of 2 .. 2048 cells a side, got {res}')
    from .halos import web_settings
    smoothing, thresholds = web_settings(args, float(getattr(args, 'boxsize', 1000.0)), int(res), _die)
    return dict(smoothing=smoothing, thresholds=thresholds)


def xcorr_option(args):
    """The (N, N, N) float32 field of --xcorr, or None without it.  It needs --density_res and that mesh size."""
    path = getattr(args, 'xcorr', None)
    if path is None:
        return None
    res = getattr(args, 'density_res', None)
    if res is None:
        _die('--xcorr needs --density_res')
    _check_file(path)
    field = np.load(path)
    if field.shape != (res,) * 3:
        _die(f'--xcorr: {path} has shape {field.shape}, expected {(res,) * 3}')
    return np.ascontiguousarray(field, dtype=np.float32)


def fof_catalog(disp, fof, Om, halo=None, xi=None, profiles=None, z=0.0, vel=None, vmom=None, env=None):
    """The arrays of fof_catalog.npz for the device displacement of one box, as {'fof': arrays}; with the settings of
    --halo_pk also 'halo': halos.halo_spectra's result (None for a box without a halo); with those of --halo_xi also
    'halo_xi': halos.halo_xi_arrays's; with those of --halo_profiles also 'halo_profiles': halos.halo_profile_arrays's at
    redshift z; with those of --halo_vprofiles / --halo_v12 (vmom, and the device velocity vel, which then gives the
    catalogue its CMVelocity) also 'halo_vprofiles': halos.halo_vprofile_arrays's and 'halo_v12': halos.halo_v12_arrays's;
    with those of --halo_environment (env) also 'halo_environment': halos.halo_environment_arrays's."""
    from .halos import (catalog_arrays, fof_halos, halo_environment_arrays, halo_profile_arrays, halo_spectra,
                        halo_v12_arrays, halo_vprofile_arrays, halo_xi_arrays)
    cat = fof_halos(disp, boxsize=fof['boxsize'], linking_length=fof['linking_length'], nmin=fof['nmin'],
                    velocity=vel if vmom is not None else None)
    out = {'fof': catalog_arrays(cat, int(disp.shape[1]), fof['boxsize'], Om, fof['linking_length'], False, fof['nmin'])}
    if halo is not None:
        out['halo'] = halo_spectra(cat, disp, fof['boxsize'], halo['res'], halo['worder'], halo['weight'])
    if xi is not None:
        out['halo_xi'] = halo_xi_arrays(cat, fof['boxsize'], xi['r_edges'], xi['nmu'])
    if profiles is not None:
        out['halo_profiles'] = halo_profile_arrays(cat, disp, fof['boxsize'], int(disp.shape[1]), Om, profiles['r_edges'],
                                                   profiles['overdensity'], profiles['reference'], z=z)
    if vmom is not None and vmom['vprofiles'] is not None:
        out['halo_vprofiles'] = halo_vprofile_arrays(cat, disp, vel, fof['boxsize'], vmom['vprofiles'])
    if vmom is not None and vmom['v12'] is not None:
        out['halo_v12'] = halo_v12_arrays(cat, fof['boxsize'], vmom['v12'])
    if env is not None:
        out['halo_environment'] = halo_environment_arrays(cat, disp, fof['boxsize'], env)
    return out


def density_summaries(delta, dens, bispec, onepoint):
    """The arrays of emu_bispectrum.npz and emu_onepoint.npz for the device field `delta` (None where not asked for)."""
    from .density import bispectrum, field_pdf, field_statistics
    bk = op = None
    if bispec:
        # the reference's mas_for_model (scripts/utils.py:1349): no window for a field that is already deconvolved
        mas = None if dens['deconvolve'] else dens['worder']
        bk = {}
        for i, (k1, k2) in enumerate(BISPECTRUM_CONFIGS, 1):
            r = bispectrum(delta, boxsize=dens['boxsize'], k1=k1, k2=k2, theta=np.linspace(0.0, np.pi, 25),
                           mas_worder=mas)
            bk.update({f'{key}_cfg{i}': r[key] for key in BISPECTRUM_KEYS})
    if onepoint:
        import torch
        lo, hi = (float(v) for v in torch.aminmax(delta))
        if lo == hi:                                         # a constant field: np.histogram's widening
            lo, hi = lo - 0.5, hi + 0.5
        op = dict(field_statistics(delta))
        op.update(field_pdf(delta, lo=lo, hi=hi, nbins=ONEPOINT_BINS))
    return bk, op


def load_params(path):
    from .nbody_emulator import load_default_parameters
    if path is None:
        return load_default_parameters()
    from .params_io import load_parameters
    return load_parameters(path)                       # flat .npz or the reference's format; nothing is executed


def run(args):
    from . import create_emulator, SubboxConfig
    from . import modulate_emulator_parameters, modulate_emulator_parameters_vel

    n = len(args.cosmo_param_files)
    if not (n == len(args.displacement_files) == len(args.output_dirs)):
        _die('Number of files must match:\n'
             f'  cosmo_param_files: {n}\n'
             f'  displacement_files: {len(args.displacement_files)}\n'
             f'  output_dirs: {len(args.output_dirs)}')
    print(f'Processing {n} simulation(s)')
    print(f'  Precision: {args.precision}')
    print(f'  Output precision: {args.output_precision}')
    print(f'  Compute velocity: {args.vel}')
    print(f'  Style modulation: {args.style}')
    print(f'  Subbox divisions: {args.ndiv}')
    dens = density_options(args)
    mink = minkowski_option(args)
    bispec, onepoint = summary_options(args)
    paint_vel, rsd = velocity_options(args)
    multipoles, wedges = anisotropy_options(args)
    fof = fof_options(args)
    halo = halo_options(args)
    halo_xi = halo_xi_options(args)
    halo_prof = halo_profile_options(args)
    halo_vmom = halo_velocity_options(args)
    halo_env = halo_environment_options(args)
    web = cosmic_web_options(args)
    target = xcorr_option(args)
    if bispec:
        for k1, k2 in BISPECTRUM_CONFIGS:                    # density.bispectrum's closure condition, before any work
            if 2.0 * (k1 + k2) * dens['boxsize'] / (2.0 * np.pi) + 1.5 >= dens['res']:
                _die(f"--bispectrum: k1 = {k1}, k2 = {k2} h/Mpc do not fit a {dens['res']}^3 mesh of a "
                     f"{dens['boxsize']} Mpc/h box")
    if dens is not None:
        print(f"  Density: {dens['res']}^3 mesh, worder {dens['worder']}, deconvolve {dens['deconvolve']}, "
              f"boxsize {dens['boxsize']}, P(k) {dens['pk']}" + (", Minkowski functionals" if mink else "")
              + (", bispectrum" if bispec else "") + (", one-point statistics" if onepoint else "")
              + (", velocity mesh" if paint_vel else "") + (f", redshift space along axis {rsd}" if rsd is not None else "")
              + (", multipoles" if multipoles else "") + (f", {wedges} wedges" if wedges is not None else "")
              + (f", T-web smoothed over {web['smoothing']:g}" if web is not None else ""))
    if fof is not None:
        print(f"  Halos: FoF b = {fof['linking_length']}, nmin {fof['nmin']}, boxsize {fof['boxsize']}"
              + (f", halo spectra on a {halo['res']}^3 mesh" if halo is not None else "")
              + (f", halo pairs in {len(halo_xi['r_edges']) - 1} bins" if halo_xi is not None else "")
              + (f", halo profiles in {len(halo_prof['r_edges']) - 1} bins" if halo_prof is not None else "")
              + (", halo velocity moments" if halo_vmom is not None else "")
              + (f", halo environment on a {halo_env['res']}^3 mesh" if halo_env is not None else ""))
    print()

    shape = None
    for f in args.displacement_files:
        shape = displacement_shape(f, shape)
    box = tuple(shape[1:])
    print(f'  Box size: {box}')
    if fof is not None:
        from .halos import linking_geometry
        if len(set(box)) != 1 or not 2 <= box[0] <= 1024:
            _die(f'--fof needs a cubic box of 2 .. 1024 particles per axis, got {box}')
        try:
            linking_geometry(box[0], fof['boxsize'], fof['linking_length'], False)
        except ValueError as e:
            _die(f'--fof: {e}')
    cosmologies = [read_cosmology(f) for f in args.cosmo_param_files]

    params = load_params(args.params)
    mid = int(params['params']['conv_l01']['conv_0']['weight'].shape[0])
    # density mode: float32 fields on the device (painted from), rounded to --output-precision for the files
    config = SubboxConfig(size=box, ndiv=args.ndiv, dtype=args.precision,
                          output_dtype=args.output_precision if dens is None and fof is None else np.float32)
    emu = create_emulator(premodulate=not args.style, compute_vel=args.vel, load_params=False,
                          processor_config=config, mid_chan=mid)
    if args.style:
        emu.params = emu.processor.params = params

    def save(out_dir, result, extra=None):
        if args.vel:
            np.save(out_dir / 'emu_dis.npy', result[0])
            np.save(out_dir / 'emu_vel.npy', result[1])
        else:
            np.save(out_dir / 'emu_dis.npy', result)
        if extra is not None and 'fof' in extra:
            np.savez_compressed(out_dir / 'fof_catalog.npz', **extra['fof'])
        if extra is not None and 'halo' in extra:
            from .halos import save_halo_spectra
            save_halo_spectra(out_dir, extra['halo'])
        if extra is not None and 'halo_xi' in extra:
            from .halos import save_halo_xi
            save_halo_xi(out_dir, extra['halo_xi'])
        if extra is not None and 'halo_profiles' in extra:
            from .halos import save_halo_profiles
            save_halo_profiles(out_dir, extra['halo_profiles'])
        for key in ('halo_vprofiles', 'halo_v12'):
            if extra is not None and key in extra:
                from .halos import save_halo_velocity
                save_halo_velocity(out_dir, key + '.npz', extra[key])
        if extra is not None and 'halo_environment' in extra:
            from .halos import save_halo_environment
            save_halo_environment(out_dir, extra['halo_environment'])
        if extra is not None and 'delta' in extra:
            np.save(out_dir / 'emu_delta.npy', extra['delta'])
            if 'pk' in extra:
                k, pk, nmodes = extra['pk']
                np.savez(out_dir / 'emu_pk.npz', k=k, pk=pk, nmodes=nmodes)
            if 'mf' in extra:
                mf = extra['mf']
                np.savez(out_dir / 'emu_minkowski.npz', **{key: mf[key] for key in
                         ('thresholds', 'v0', 'v1', 'v2', 'v3', 'counts', 'mean', 'std')})
            if extra.get('bk') is not None:
                np.savez(out_dir / 'emu_bispectrum.npz', **extra['bk'])
            if extra.get('onepoint') is not None:
                np.savez(out_dir / 'emu_onepoint.npz', **extra['onepoint'])
            if 'vel_mesh' in extra:
                np.save(out_dir / 'emu_vel_mesh.npy', extra['vel_mesh'])
            if 'delta_rsd' in extra:
                np.save(out_dir / 'emu_delta_rsd.npy', extra['delta_rsd'])
            if 'pk_rsd' in extra:
                k, pk, nmodes = extra['pk_rsd']
                np.savez(out_dir / 'emu_pk_rsd.npz', k=k, pk=pk, nmodes=nmodes)
            if 'pk_rsd_multipoles' in extra:
                np.savez(out_dir / 'emu_pk_rsd_multipoles.npz', **extra['pk_rsd_multipoles'])
            if 'pk_rsd_wedges' in extra:
                np.savez(out_dir / 'emu_pk_rsd_wedges.npz', **extra['pk_rsd_wedges'])
            if 'xcorr' in extra:
                np.savez(out_dir / 'emu_xcorr.npz', **extra['xcorr'])
            if 'web' in extra:
                np.save(out_dir / 'emu_web_type.npy', extra['web']['types'])
                np.savez(out_dir / 'emu_web.npz', **{key: extra['web'][key] for key in WEB_KEYS})

    def with_density(dis_in, z, Om):
        """process_box on the device, the density field of its float32 displacement, host copies of the fields."""
        import torch
        from .density import minkowski_functionals, paint_density, power_spectrum
        box_t = torch.from_numpy(np.ascontiguousarray(dis_in)).to('cuda')
        result = emu.process_box(box_t, z=z, Om=Om, show_progress=not args.quiet)
        disp = result[0] if args.vel else result
        extra = {} if fof is None else fof_catalog(disp, fof, Om, halo, halo_xi, halo_prof, float(z),
                                                   vel=result[1] if halo_vmom is not None else None, vmom=halo_vmom,
                                                   env=halo_env)
        out_dt = np.dtype(args.output_precision)
        if dens is None:
            host = tuple(t.cpu().numpy().astype(out_dt, copy=False) for t in (result if args.vel else (result,)))
            return (host if args.vel else host[0]), extra
        delta = paint_density(disp, boxsize=dens['boxsize'], res=dens['res'], worder=dens['worder'],
                              deconvolve=dens['deconvolve'])
        extra['delta'] = delta.cpu().numpy()
        if dens['pk']:
            extra['pk'] = power_spectrum(delta, boxsize=dens['boxsize'])
        if target is not None:
            from .density import cross_correlation
            extra['xcorr'] = cross_correlation(delta, torch.from_numpy(target).to(delta.device), boxsize=dens['boxsize'])
        if mink:
            extra['mf'] = minkowski_functionals(delta, boxsize=dens['boxsize'])
        if bispec or onepoint:
            extra['bk'], extra['onepoint'] = density_summaries(delta, dens, bispec, onepoint)
        if web is not None:
            from .web import cosmic_web
            w = cosmic_web(delta, dens['boxsize'], web['smoothing'], threshold=web['thresholds'], mass=delta)
            extra['web'] = dict({key: w[key] for key in WEB_KEYS}, types=w['types'].cpu().numpy())
        if paint_vel or rsd is not None:
            extra.update(velocity_fields(disp, result[1], dens, paint_vel, rsd, z, Om, multipoles, wedges))
        host = tuple(t.cpu().numpy().astype(out_dt, copy=False) for t in (result if args.vel else (result,)))
        return (host if args.vel else host[0]), extra

    # one reader and one writer thread: disk I/O of the neighbours overlaps the GPU work on the current box
    with ThreadPoolExecutor(max_workers=2) as pool:
        nxt = pool.submit(np.load, args.displacement_files[0])
        pending = None
        for i, (cosmo, out_dir) in enumerate(zip(cosmologies, args.output_dirs)):
            Om, z = cosmo
            dis_in = nxt.result()
            if i + 1 < n:
                nxt = pool.submit(np.load, args.displacement_files[i + 1])
            if not args.style:
                tree = (modulate_emulator_parameters_vel if args.vel else modulate_emulator_parameters)(params, z, Om)
                emu.params = emu.processor.params = tree
            t0 = time.time()
            extra = None
            if dens is None and fof is None:
                result = emu.process_box(dis_in, z=z, Om=Om, show_progress=not args.quiet)
            else:
                result, extra = with_density(dis_in, z, Om)
            dt = time.time() - t0
            if pending is not None:
                pending.result()
            pending = pool.submit(save, out_dir, result, extra)
            print(f'[{i + 1}/{n}] z={z:.4f}, Om={Om:.4f}: {dt:.2f}s -> {out_dir}')
        if pending is not None:
            pending.result()
    print('\nDone!')


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == '__main__':
    main()
