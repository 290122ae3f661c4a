"""Flat-LambdaCDM scalars with the reference's names and signatures
(reference src/jax_nbody_emulator/cosmology.py:34-155).

Host-side NumPy; no SciPy/JAX dependency: 2F1(1, 1/3; 11/6; x) is summed as a power
series after the same Pfaff transformation the reference uses for x < 0
(cosmology.py:24-31).  The reference differentiates with jax.jvp; here the
derivatives are analytic.  Inputs may be scalars or arrays; results are float32
arrays of the broadcast shape (JAX's default precision), computed in float64.
The same series is implemented in C inside libnbe.so (nbe_growth_factor, nbe_vel_norm).
"""

import functools
import math

import numpy as np

_A, _B, _C = 1.0, 1.0 / 3.0, 11.0 / 6.0


def _series(a, b, c, z):
    z = np.asarray(z, dtype=np.float64)
    term = np.ones_like(z)
    total = np.ones_like(z)
    for n in range(200000):
        term = term * ((a + n) * (b + n) / ((c + n) * (n + 1.0))) * z
        total = total + term
        if np.all(np.abs(term) <= 1e-17 * np.abs(total)):
            break
    return total


def _hyp2f1(a, b, c, x):
    x = np.asarray(x, dtype=np.float64)
    neg = x < 0
    xs = np.where(neg, x, 0.0)
    pf = np.power(1.0 - xs, -a) * _series(a, c - b, c, xs / (xs - 1.0))      # Pfaff, x < 0
    ps = _series(a, b, c, np.where(neg, 0.0, x))
    return np.where(neg, pf, ps)


def _f64(z, Om):
    z, Om = np.broadcast_arrays(np.asarray(z, dtype=np.float64), np.asarray(Om, dtype=np.float64))
    return z, Om


def _growth_factor64(z, Om):
    a = 1.0 / (1.0 + z)
    OL = 1.0 - Om
    return a * _hyp2f1(_A, _B, _C, -OL * a ** 3 / Om) / _hyp2f1(_A, _B, _C, -OL / Om)


def _hubble64(z, Om):
    return 100.0 * np.sqrt(Om * (1.0 + z) ** 3 + (1.0 - Om))


def _growth_rate64(z, Om):
    a = 1.0 / (1.0 + z)
    x = -(1.0 - Om) * a ** 3 / Om
    F = _hyp2f1(_A, _B, _C, x)
    dF = (_A * _B / _C) * _hyp2f1(_A + 1.0, _B + 1.0, _C + 1.0, x)
    return 1.0 + 3.0 * x * dF / F


def _dlogH_dloga64(z, Om):
    E2 = Om * (1.0 + z) ** 3 + (1.0 - Om)
    return -1.5 * Om * (1.0 + z) ** 3 / E2


def _out(v):
    return np.asarray(v, dtype=np.float32)


def growth_factor(z, Om):
    """Linear growth function for flat LambdaCDM, normalized to 1 at redshift zero."""
    return _out(_growth_factor64(*_f64(z, Om)))


def hubble_rate(z, Om):
    """Hubble parameter in [h km/s/Mpc] for flat LambdaCDM."""
    return _out(_hubble64(*_f64(z, Om)))


def growth_rate(z, Om):
    """Linear growth rate f = d log D / d log a."""
    return _out(_growth_rate64(*_f64(z, Om)))


def dlogH_dloga(z, Om):
    """Log-log derivative of Hubble w.r.t. scale factor."""
    return _out(_dlogH_dloga64(*_f64(z, Om)))


def vel_norm(z, Om):
    """Velocity normalization factor [km/s]: D f H / (1+z)."""
    z, Om = _f64(z, Om)
    return _out(_growth_factor64(z, Om) * _growth_rate64(z, Om) * _hubble64(z, Om) / (1.0 + z))


def acc_norm(z, Om):
    """Acceleration normalization factor [km/s^2]."""
    z, Om = _f64(z, Om)
    return _out(_growth_factor64(z, Om) * _growth_rate64(z, Om) * _hubble64(z, Om) ** 2
                * _dlogH_dloga64(z, Om) / (1.0 + z))


# ---- second-order growth ---------------------------------------------------------------------------------------------------

GROWTH2_START = 1.0e-4                  # the scale factor the integration starts at, deep in the matter era
GROWTH2_STEPS = 20000                   # fixed RK4 steps in ln a from GROWTH2_START to the end: part of the definition


def _matter_fraction(x, Om):
    """Om(a) = Om a^-3 / E^2 at x = ln a."""
    m = Om * math.exp(-3.0 * x)
    return m / (m + (1.0 - Om))


@functools.lru_cache(maxsize=256)
def _growth2_integrate(a_end, Om):
    """(D1, D1', D2, D2') at a_end (primes are d/dx, x = ln a), from the matter-era start D1 = a, D2 = -3/7 a^2 at
    a = GROWTH2_START: GROWTH2_STEPS equal RK4 steps, whatever a_end is, of
        D1'' = 1.5 Om(a) D1 - (2 + dlnH/dlna) D1',   D2'' = 1.5 Om(a) (D2 - D1^2) - (2 + dlnH/dlna) D2',
    with dlnH/dlna = -1.5 Om(a).  Python floats: a scalar recurrence, for which NumPy would only add overhead."""
    x = math.log(GROWTH2_START)
    h = (math.log(a_end) - x) / GROWTH2_STEPS
    a0 = GROWTH2_START
    d1, v1, d2, v2 = a0, a0, -3.0 / 7.0 * a0 * a0, -6.0 / 7.0 * a0 * a0
    o0 = _matter_fraction(x, Om)
    for _ in range(GROWTH2_STEPS):
        om, o1 = _matter_fraction(x + 0.5 * h, Om), _matter_fraction(x + h, Om)
        g0, gm, g1 = 1.5 * o0, 1.5 * om, 1.5 * o1                      # the source coefficient at the three points
        f0, fm, f1 = 2.0 - g0, 2.0 - gm, 2.0 - g1                      # the friction
        a1, b1 = g0 * d1 - f0 * v1, g0 * (d2 - d1 * d1) - f0 * v2
        p, q, r, s = d1 + 0.5 * h * v1, v1 + 0.5 * h * a1, d2 + 0.5 * h * v2, v2 + 0.5 * h * b1
        a2, b2 = gm * p - fm * q, gm * (r - p * p) - fm * s
        p2, q2, r2, s2 = d1 + 0.5 * h * q, v1 + 0.5 * h * a2, d2 + 0.5 * h * s, v2 + 0.5 * h * b2
        a3, b3 = gm * p2 - fm * q2, gm * (r2 - p2 * p2) - fm * s2
        p3, q3, r3, s3 = d1 + h * q2, v1 + h * a3, d2 + h * s2, v2 + h * b3
        a4, b4 = g1 * p3 - f1 * q3, g1 * (r3 - p3 * p3) - f1 * s3
        d1, v1, d2, v2 = (d1 + (h / 6.0) * (v1 + 2.0 * (q + q2) + q3), v1 + (h / 6.0) * (a1 + 2.0 * (a2 + a3) + a4),
                          d2 + (h / 6.0) * (v2 + 2.0 * (s + s2) + s3), v2 + (h / 6.0) * (b1 + 2.0 * (b2 + b3) + b4))
        x, o0 = x + h, o1
    return d1, v1, d2, v2


def _growth2(z, Om):
    """(D2 normalised, f2) as float64 arrays of the broadcast shape, element by element."""
    z, Om = _f64(z, Om)
    if np.any(z <= -1.0) or np.any(Om <= 0.0) or np.any(Om > 1.0):
        raise ValueError("second-order growth needs z > -1 and 0 < Om <= 1 (flat LambdaCDM)")
    D2, f2 = np.empty(z.shape), np.empty(z.shape)
    for i in np.ndindex(z.shape):
        om = float(Om[i])
        _, _, d2, v2 = _growth2_integrate(1.0 / (1.0 + float(z[i])), om)
        today = _growth2_integrate(1.0, om)[0]
        D2[i], f2[i] = d2 / (today * today), v2 / d2
    return D2, f2


def growth_factor_2(z, Om):
    """Second-order growth function D_2 for flat LambdaCDM, in the normalisation where growth_factor(0, Om) = 1.  It is
    negative: the second-order displacement is psi2_k = -D_2 i k / |k|^2 S_k (lpt.lpt2_displacement's growth2 is
    -D_2 / D_1^2).  float64, of the broadcast shape.

    Defined by the ODE in x = ln a,  D'' + (2 + dlnH/dlna) D' - 1.5 Om(a) D = -1.5 Om(a) D_1^2,  integrated together with
    D_1 from a = 1e-4 with the matter-era start D_1 = a, D_2 = -3/7 a^2, by GROWTH2_STEPS = 20000 equal RK4 steps in ln a
    to the epoch asked for, and once more to a = 1 for the normalisation: D_2(z) = D_2(a) / D_1(a = 1)^2.  The common fit
    -3/7 D_1^2 Om(z)^(-1/143) (Bouchet et al. 1995) is within 2e-4 of it for Om >= 0.1; it is not the definition."""
    return _growth2(z, Om)[0]


def growth_rate_2(z, Om):
    """Second-order growth rate f_2 = d log D_2 / d log a, from the integration of `growth_factor_2`.  float64.  The fit
    2 Om(z)^(6/11) is within half a percent of it from Om = 0.2 and 1.2 percent off at Om = 0.1, z = 0."""
    return _growth2(z, Om)[1]
