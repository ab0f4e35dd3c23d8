"""Proper orthogonal decomposition of a trajectory by the method of snapshots

    S (m x NV, the kept velocities),  G = S W S^T,  Gc = H G H,
    Gc = V diag(lambda) V^T,  modes = (H V Lambda^{-1/2})^T S,

`W` the (symmetric, positive definite) weight matrix -- the mass matrix --, `H =
I - 1 1^T / m` the centring (the device keeps RAW snapshots, the mean is taken
out of the small matrix).  What is large -- `G` and the products with `S` -- runs
on the device where the time loop does (`ImexStepper.ensemble_gram`,
`.ensemble_combine` over the snapshot ensemble the steps fill); what is `m x m`
runs here, `decompose`, shared by both paths.  `evaluate` is the fp64 host
statement of the whole thing.

The POD covers the inner (condensed) velocity dofs `v`: with controlled
Dirichlet values the boundary values are NOT part of the snapshots.
"""
import numpy as np
import scipy.sparse as sps

__all__ = ['SnapshotPOD']

_U = 2.0**-53
RANK_TOL = 1e-12        # modes with lambda_k <= lambda_1 * RANK_TOL are dropped


def _ldv(nv):
    return -(-int(nv)//64)*64


class SnapshotPOD(object):
    """the weight matrix, which times are kept, how the modes are truncated

    `W`: NV x NV, symmetric.  Kept are the times `times` (each must be one of
    the loop's step times, `ValueError` otherwise) or, with `times=None`,
    every `every`-th step of `trange[1:]` -- entry `k` of `trange` with `k %
    every == 0`.  The rows cover the AB2 / BDF2 steps of the loop, `trange[2:]`:
    the Heun start runs on the host and is not a snapshot (as it has no row of
    the functionals) -- `every=1` keeps `trange[2:]`, and `trange[1]` among
    `times` is refused by name.  `nmodes`: at most this many modes; `energy`:
    the fewest modes whose eigenvalues sum to this fraction of all kept ones;
    `center`: take the mean flow out (it is returned beside the modes).  `max_bytes`
    caps the ensemble on the device, `m * ldv * 8` bytes, `ldv` = NV rounded up
    to 64."""

    def __init__(self, W, times=None, every=1, nmodes=None, energy=None,
                 center=True, max_bytes=1 << 30):
        self.W = sps.csr_matrix(W)
        if self.W.shape[0] != self.W.shape[1]:
            raise ValueError('`W` must be square, it is {0}'.format(
                self.W.shape))
        self.NV = self.W.shape[0]
        self.times = None if times is None else [float(t) for t in times]
        self.every = int(every)
        if self.every < 1:
            raise ValueError('`every` must be positive')
        if energy is not None and not 0. < energy <= 1.:
            raise ValueError('`energy` is a fraction in (0, 1]')
        if nmodes is not None and int(nmodes) < 1:
            raise ValueError('`nmodes` must be positive')
        self.nmodes = None if nmodes is None else int(nmodes)
        self.energy, self.center = energy, bool(center)
        self.max_bytes = int(max_bytes)
        self._slot_of = {}

    # ---- which steps --------------------------------------------------------
    def plan(self, trange):
        """`(kept, slots)`: the entries of `trange` that are kept (indices,
        ascending, all >= 2) and their global slots `0 .. m - 1`.  Remembers
        the plan for `slots_for`."""
        tr = [float(t) for t in trange]
        if self.times is None:
            kept = [k for k in range(2, len(tr)) if k % self.every == 0]
        else:
            where = {t: k for k, t in enumerate(tr) if k >= 2}
            if len(tr) > 1 and tr[1] in self.times:
                raise ValueError(
                    'kept time {0!r} is `trange[1]`, the Heun start: it runs '
                    'on the host and cannot be kept, the snapshots are the '
                    'step times `trange[2:]`'.format(tr[1]))
            off = [t for t in self.times if t not in where]
            if off:
                raise ValueError(
                    'kept time {0!r} is none of the step times `trange[2:]` '
                    '({1} of {2} are not)'.format(off[0], len(off),
                                                  len(self.times)))
            kept = sorted(set(where[t] for t in self.times))
        m = len(kept)
        if m < 1:
            raise ValueError('no step of the loop is kept')
        need = m*_ldv(self.NV)*8
        if need > self.max_bytes:
            raise ValueError(
                'an ensemble of m = {0} snapshots takes {1} bytes on the '
                'device, the cap `max_bytes` is {2}'.format(m, need,
                                                            self.max_bytes))
        kept = np.array(kept, dtype=np.int64)
        slots = np.arange(m, dtype=np.int32)
        self._slot_of = {tr[k]: int(s) for k, s in zip(kept, slots)}
        self._times = np.array([tr[k] for k in kept])
        return kept, slots

    @property
    def m(self):
        return len(self._slot_of)

    def slots_for(self, times):
        """the slot table of a slice: global slot of each step time, -1 where
        the step is not kept (int32)"""
        return np.array([self._slot_of.get(float(t), -1) for t in times],
                        dtype=np.int32)

    # ---- the m x m algebra --------------------------------------------------
    def decompose(self, G):
        """from the Gram matrix of the RAW snapshots: a dict with `sigma`
        (r singular values of `W^{1/2}`-weighted, centred snapshots),
        `coeffs` (r x m: snapshot s - mean = sum_k coeffs[k, s] modes[k]),
        `coef` (r x m, or (r + 1) x m with `center`: modes = coef[:r] @ S and
        the mean flow = coef[r] @ S) and `nmodes` = r"""
        G = np.asarray(G, dtype=np.float64)
        m = G.shape[0]
        if G.shape != (m, m):
            raise ValueError('`G` must be square')
        H = np.eye(m) - (1./m if self.center else 0.)*np.ones((m, m))
        Gc = H @ G @ H
        lam, V = np.linalg.eigh(.5*(Gc + Gc.T))
        lam, V = lam[::-1], V[:, ::-1]
        if not lam[0] > 0.:
            raise ValueError('the snapshots span nothing (largest eigenvalue '
                             '{0})'.format(lam[0]))
        r = int(np.sum(lam > lam[0]*RANK_TOL))
        if self.energy is not None:
            frac = np.cumsum(lam[:r])/np.sum(lam[:r])
            r = min(r, int(np.searchsorted(frac, self.energy*(1. - 1e-15))
                           ) + 1)
        if self.nmodes is not None:
            r = min(r, self.nmodes)
        lam, V = lam[:r], V[:, :r]
        sigma = np.sqrt(lam)
        coef = (H @ V/sigma).T
        if self.center:
            coef = np.vstack([coef, np.full((1, m), 1./m)])
        return dict(sigma=sigma, coeffs=(V*sigma).T,
                    coef=np.ascontiguousarray(coef), nmodes=r)

    def split(self, dec, full):
        """`(modes, mean)` of `full = coef @ S`"""
        r = dec['nmodes']
        return full[:r], (full[r] if self.center else None)

    def evaluate(self, snapshots):
        """the host model: `gram`, `sigma`, `modes` (r x NV, `modes W modes^T
        = I`), `mean` (NV, None without `center`), `coeffs`, `coef`"""
        S = np.asarray(snapshots, dtype=np.float64)
        if S.ndim != 2 or S.shape[1] != self.NV:
            raise ValueError('`snapshots` must be m x NV = m x {0}, it is '
                             '{1}'.format(self.NV, S.shape))
        G = S @ (self.W @ S.T)
        dec = self.decompose(G)
        modes, mean = self.split(dec, dec['coef'] @ S)
        return dict(gram=G, sigma=dec['sigma'], modes=modes, mean=mean,
                    coeffs=dec['coeffs'], coef=dec['coef'])

    # ---- a-priori bounds of the two device operations -----------------------
    def bound_gram(self, S):
        """`|G_dev - S W S^T|_ij <= 1.01 (NV + maxrownnz(W) + 2) u sum_k
        |S_ik| (|W| |S_j|)_k`, `u = 2^-53`: any summation order, with or
        without fma (m x m)"""
        return gram_bound(S, self.W)

    def bound_combine(self, S, coef):
        """`|out_dev - coef S|_qk <= 1.01 (m + 1) u sum_s |coef_qs| |S_sk|`"""
        return combine_bound(S, coef)


def gram_bound(S, W=None):
    S = np.abs(np.asarray(S, dtype=np.float64))
    nv = S.shape[1]
    if W is None:
        Wa, rownnz = sps.identity(nv, format='csr'), 1
    else:
        Wa = abs(sps.csr_matrix(W))
        rownnz = int(np.diff(Wa.indptr).max()) if nv else 0
    return 1.01*(nv + rownnz + 2)*_U*(S @ (Wa @ S.T))


def combine_bound(S, coef):
    S = np.abs(np.asarray(S, dtype=np.float64))
    return 1.01*(S.shape[0] + 1)*_U*(np.abs(np.asarray(coef)) @ S)
