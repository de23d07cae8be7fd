"""Charge statistics (``ChargeChain.set_charge_statistics``, ``simulate_pixels.py --charge_statistics``): the numpy
restatement of ``quench_drift_stat_kernel``'s counting (csrc/kernels_seg.hip), operation for operation in float64, and the
analytic mean and variance of what it draws.

Per segment, from five keyed draws (stage tag ``rng.TAG_CHARGE``, stream ``segment_keys``): draw 0 = Fano normal,
1 / 2 = recombination normal / uniform, 3 / 4 = attachment normal / uniform.

    N_i = max(0, rint(dE / W_ion + sqrt(F dE / W_ion) z0))
    n_q ~ Binomial(N_i, R)                       R = Box / Birks factor clamped to [0, 1]
    n_photons = (dE / W_ph - n_q) scint_prescale
    n_electrons ~ Binomial(n_q, exp(-t_drift / lifetime)) inside a TPC, n_q outside
"""
import numpy as np

from . import rng

NORMAL_MIN = 30.0        # n * min(p, 1 - p) from which a binomial is drawn as a rounded normal
WALK_MAX = 256.0         # where the inversion walk stops
FANO_DEFAULT = 0.107
DRAW_FANO, DRAW_RECOMB_Z, DRAW_RECOMB_U, DRAW_ATTACH_Z, DRAW_ATTACH_U = range(5)


def segment_keys(batch_keys, batch_id):
    """stream key of every segment: key_mix(batch key, index of the segment within its batch); ``batch_id`` as uploaded
    (each batch one run); segments with id < 0 get key 0 (they draw nothing)"""
    b = np.asarray(batch_id, dtype=np.int64)
    idx = np.arange(len(b), dtype=np.int64)
    first = np.r_[True, b[1:] != b[:-1]] if len(b) else np.zeros(0, dtype=bool)
    within = idx - np.maximum.accumulate(np.where(first, idx, 0))
    ok = b >= 0
    keys = np.zeros(len(b), dtype=np.uint64)
    keys[ok] = rng.key_mix(np.asarray(batch_keys, dtype=np.uint64)[b[ok]], within[ok])
    return keys


def binomial_branch(n, p):
    """True where ``binomial`` draws the rounded normal, False where it inverts (degenerate inputs: False)"""
    n, p = np.broadcast_arrays(np.asarray(n, dtype=np.float64), np.asarray(p, dtype=np.float64))
    return (n > 0) & (p > 0) & (p < 1) & (n * np.minimum(p, 1 - p) >= NORMAL_MIN)


def binomial(n, p, z, u):
    """Binomial(n, p) from one normal draw ``z`` and one uniform draw ``u`` per element (float32 as the device draws them).
    p <= 0 -> 0, p >= 1 -> n, n = 0 -> 0.  With pm = min(p, 1 - p): n pm >= 30 gives clamp(rint(n p + sqrt(n p (1 - p)) z), 0, n);
    otherwise inversion on the minority outcome at u - 2^-25 (the centre of the uniform's 24-bit cell):
    P(0) = exp(n log1p(-pm)), P(j + 1) = P(j) (n - j) / (j + 1) * (pm / (1 - pm)), j the first index whose running sum reaches
    the centre, the walk stopping at min(n, 256); the result is j for p <= 1/2, n - j above."""
    n, p, z, u = (np.array(a, dtype=np.float64) for a in np.broadcast_arrays(n, p, z, u))
    out = np.zeros(n.shape)
    live = (n > 0) & (p > 0)
    full = live & (p >= 1)
    out[full] = n[full]
    live &= ~full
    pm = np.minimum(p, 1 - p)
    with np.errstate(all="ignore"):
        normal = live & (n * pm >= NORMAL_MIN)
        k = np.rint(n * p + np.sqrt(n * p * (1 - p)) * z)
        out[normal] = np.minimum(np.maximum(k, 0.0), n)[normal]
        inv = np.flatnonzero(live & ~normal)
        ni, pmi = n.flat[inv], pm.flat[inv]
        centre = u.flat[inv] - 2.0 ** -25
        ratio, jmax = pmi / (1 - pmi), np.minimum(ni, WALK_MAX)
        q = np.exp(ni * np.log1p(-pmi))
        total, j = q.copy(), np.zeros(len(inv))
        while True:
            go = (total < centre) & (j < jmax)
            if not go.any():
                break
            qn = q * (ni - j) / (j + 1) * ratio
            q = np.where(go, qn, q)
            j = np.where(go, j + 1, j)
            total = np.where(go, total + q, total)
    out.flat[inv] = np.where(p.flat[inv] <= 0.5, j, ni - j)
    return out


def recombination(dEdx, mode, c, e_field=None):
    """the Box (mode 1) / Birks (mode 2) factor with the kernel's expressions, from the packed constants ``c``
    (abi.pack_consts); ``e_field``: the local field per segment (default: the constants')"""
    dEdx = np.asarray(dEdx, dtype=np.float64)
    E = c.e_field if e_field is None else np.asarray(e_field, dtype=np.float64)
    with np.errstate(all="ignore"):
        if mode == 1:
            csi = c.box_beta * dEdx / (E * c.lar_density)
            r = np.log(c.box_alpha + csi) / csi
            return np.where(r > 0, r, 0.0)
        if mode == 2:
            return c.birks_ab / (1 + c.birks_kb * dEdx / (E * c.lar_density))
    raise ValueError("mode must be 1 (BOX) or 2 (BIRKS)")


def counts(dE, recomb, lifetime, draws_normal, draws_uniform, w_ion, w_ph, scint_prescale=1.0, fano=FANO_DEFAULT):
    """The kernel's counting before the stores narrow it.  ``recomb``: the recombination factor per segment
    (``recombination``); ``lifetime``: exp(-t_drift / electron_lifetime) per segment, NaN for a segment outside every TPC
    (it keeps n_q); ``draws_normal`` / ``draws_uniform``: [n][5] draws 0-4 of every segment's stream.
    Returns (n_ion, n_q, n_electrons, n_photons) in float64."""
    dE = np.asarray(dE, dtype=np.float64)
    zn, un = np.asarray(draws_normal, dtype=np.float64), np.asarray(draws_uniform, dtype=np.float64)
    n0 = dE / w_ion
    with np.errstate(invalid="ignore"):
        n_ion = np.fmax(0.0, np.rint(n0 + np.sqrt(fano * n0) * zn[:, DRAW_FANO]))
    r = np.minimum(np.maximum(np.asarray(recomb, dtype=np.float64), 0.0), 1.0)
    n_q = binomial(n_ion, r, zn[:, DRAW_RECOMB_Z], un[:, DRAW_RECOMB_U])
    n_ph = (dE / w_ph - n_q) * scint_prescale
    lifetime = np.asarray(lifetime, dtype=np.float64)
    inside = ~np.isnan(lifetime)
    n_e = n_q.copy()
    n_e[inside] = binomial(n_q[inside], lifetime[inside], zn[inside, DRAW_ATTACH_Z], un[inside, DRAW_ATTACH_U])
    return n_ion, n_q, n_e, n_ph


def mean_variance(dE, recomb, lifetime, w_ion, fano=FANO_DEFAULT):
    """analytic mean and variance of n_electrons: with N = dE / W_ion and p = R L, mean N p and variance
    N p (1 - p) + F N p^2 (binomial thinning of a count of mean N and variance F N; the rounding of N_i adds at most 1/12)"""
    N = np.asarray(dE, dtype=np.float64) / w_ion
    p = np.clip(recomb, 0.0, 1.0) * np.asarray(lifetime, dtype=np.float64)
    return N * p, N * p * (1 - p) + fano * N * p * p
