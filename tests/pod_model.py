"""Shared pieces of the POD tests: seeded data, extended-precision references of
the two device operations, and a host model of the stepper's snapshot
ensemble."""
import numpy as np
import scipy.sparse as sps

import imex_host_model

# `modes W modes^T = I` and the singular values against an SVD, for the host
# model `SnapshotPOD.evaluate` at NV = 60, m = 9 (seeded, with and without
# centring): measured 1.0e-14 (orthonormality, max entry) and 2.1e-15
# (singular values, relative to the largest) on the CPU -- see
# test_pod_cpu.py::test_evaluate_against_an_svd, which prints them -- times 10.
# The method of snapshots squares the condition: the departure from
# orthonormality grows like u lambda_1 / lambda_k, which the rank cut-off
# 1e-12 of `decompose` caps.
ORTHO_TOL = 1.0e-13
SIGMA_TOL = 2.1e-14

# Beyond well-conditioned data the tolerance above cannot hold, and what holds
# instead is derived: the modes are `Lambda^{-1/2} V^T H S` with `(Lambda, V)`
# the eigenpairs of the COMPUTED `Gc = H G H`, which differs from the exact
# one by `|dGc|_2 <= c m u |G|_2` (the Gram matrix's own rounding, two m-term
# products with the projection `H`, `eigh`'s backward error), so
#     |modes W modes^T - I|_kl = |V^T dGc V|_kl / sqrt(lambda_k lambda_l)
#                             <= c m u |G|_2 / sqrt(lambda_k lambda_l),
# `u = 2^-53`, for EVERY kept mode down to the rank cut-off.  `c` measured on
# the host model `evaluate` (test_pod_cpu.py::
# test_orthonormality_follows_the_derived_law prints it: toy wake, CNAB and
# SBDF2, 6 and 13 snapshots, with and without centring, all modes kept, and
# the seeded data above): at most 1.67 -- times 10.
ORTHO_C = 17.


def ortho_bound(gram, sigma):
    """the bound above, r x r, for the modes with singular values `sigma`
    from the Gram matrix `gram` of the raw snapshots"""
    lam = np.asarray(sigma, dtype=np.float64)**2
    m = gram.shape[0]
    return ORTHO_C*m*2.**-53*np.linalg.norm(gram, 2)/np.sqrt(
        np.outer(lam, lam))


def ortho_error(res, W):
    """`|modes W modes^T - I|` of a POD result (r x r)"""
    modes = res['modes']
    return np.abs(modes @ (W @ modes.T) - np.eye(modes.shape[0]))


def seeded_spd(nv, seed):
    """`(W sparse, L dense)` with `W = L^T L` from a dense Cholesky"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((nv, nv))
    Wd = B @ B.T/nv + np.eye(nv)
    Wd = .5*(Wd + Wd.T)
    L = np.linalg.cholesky(Wd).T            # W = L^T L
    return sps.csr_matrix(Wd), L


def gram_longdouble(S, W=None):
    """`S W S^T` in `np.longdouble` (m x m)"""
    ld = np.longdouble
    Sl = np.asarray(S, dtype=np.float64).astype(ld)
    if W is None:
        return Sl @ Sl.T
    W = sps.csr_matrix(W)
    Y = np.zeros_like(Sl)                   # Y[:, r] = sum_c W[r, c] S[:, c]
    for r in range(W.shape[0]):             # (W symmetric: Y = S W)
        a, b = W.indptr[r], W.indptr[r + 1]
        if b > a:
            Y[:, r] = Sl[:, W.indices[a:b]] @ W.data[a:b].astype(ld)
    return Sl @ Y.T


def combine_longdouble(S, coef):
    ld = np.longdouble
    return np.asarray(coef, dtype=np.float64).astype(ld) @ \
        np.asarray(S, dtype=np.float64).astype(ld)


class PodStepper(imex_host_model.HostStepper):
    """the host model with the snapshot ensemble: a slot table per call of
    `set_ensemble`, the ensemble kept unless `reset` or another size"""

    def set_ensemble(self, slots, nslots=None, reset=False):
        slots = np.asarray(slots, dtype=np.int32)
        nslots = int(slots.max()) + 1 if nslots is None else int(nslots)
        assert slots.min() >= -1 and slots.max() < nslots
        E = getattr(self, 'ens', None)
        if reset or E is None or E.shape[0] != nslots:
            self.ens = np.zeros((nslots, self.R1.shape[0]))
        self.ens_slots, self.ens_row = slots, 0
        self.ens_armed = getattr(self, 'ens_armed', 0) + 1
        self.ens_resets = getattr(self, 'ens_resets', 0) + int(bool(reset))

    def step(self, cf, nfc_new=None, opts=None):
        imex_host_model.HostStepper.step(self, cf, nfc_new=nfc_new, opts=opts)
        if getattr(self, 'ens_slots', None) is not None:
            assert self.ens_row < self.ens_slots.size, 'past the slot table'
            sl = self.ens_slots[self.ens_row]
            if sl >= 0:
                self.ens[sl] = np.asarray(self.v_c).reshape(-1)
            self.ens_row += 1

    def ensemble(self, first=0, count=None):
        count = self.ens.shape[0] - first if count is None else count
        return self.ens[first:first + count].copy()

    def ensemble_gram(self, W=None, m=None):
        S = self.ens if m is None else self.ens[:m]
        return S @ S.T if W is None else S @ (sps.csr_matrix(W) @ S.T)

    def ensemble_combine(self, coef, m=None):
        return np.asarray(coef) @ (self.ens if m is None else self.ens[:m])

    def clear_ensemble(self):
        self.ens_slots = None
        self.ens_cleared = True
