"""Sensors, actuators and a seeded linear observer for the closed-loop tests
(`tests/golden/make_golden_feedback.py`, `test_feedback_cpu.py`,
`test_gpu_feedback.py`): the same builder feeds the reference, the CPU oracle
and the HIP path, so all three see identical matrices.

 * `cv_mat` (Ny x NV): box means of the vertical velocity in the wake
 * `b_mat`  (NV x Nu): `M`-weighted Gaussian bumps of vertical force behind
                       the obstacle (the inner rows of `M g`)
 * observer: `ha = -5 I + randn`, `hb, hc = randn` (`hc` times `gain`),
             `inihx = 0.1 randn`, `drift(t) = sin(7 t) d`
"""
import numpy as np
import scipy.sparse as sps

BOXES = ((0.55, 0.10), (0.55, 0.20), (0.55, 0.30))     # centres of the sensors
BOX_HALF = (0.12, 0.055)
BUMPS = ((0.32, 0.14), (0.32, 0.26))                   # centres of the bumps
BUMP_SIGMA, BUMP_RADIUS = 0.03, 0.085


def sensors_actuators(th, invinds, M, boxes=BOXES, box_half=BOX_HALF,
                      bumps=BUMPS, sigma=BUMP_SIGMA, radius=BUMP_RADIUS):
    """`(cv_mat, b_mat)` as CSR on the inner velocity dofs; the full velocity
    vector holds the x / y components of node i at 2i / 2i + 1"""
    invinds = np.asarray(invinds)
    NV = invinds.size
    node, comp = invinds//2, invinds % 2
    xy = th.nodecoords[node]
    rows, cols, vals = [], [], []
    for k, (cx, cy) in enumerate(boxes):
        inbox = (comp == 1) & (np.abs(xy[:, 0] - cx) <= box_half[0]) \
            & (np.abs(xy[:, 1] - cy) <= box_half[1])
        idx = np.flatnonzero(inbox)
        assert idx.size > 0, 'empty sensor box'
        rows += [k]*idx.size
        cols += idx.tolist()
        vals += [1./idx.size]*idx.size
    cv_mat = sps.csr_matrix((vals, (rows, cols)), shape=(len(boxes), NV))
    gcols = []
    for (cx, cy) in bumps:
        d2 = (xy[:, 0] - cx)**2 + (xy[:, 1] - cy)**2
        g = np.where((comp == 1) & (d2 <= radius**2),
                     np.exp(-d2/(2*sigma**2)), 0.)
        assert np.count_nonzero(g) > 0, 'empty actuator bump'
        gcols.append(sps.csr_matrix(g.reshape((-1, 1))))
    b_mat = sps.csr_matrix(sps.csr_matrix(M) @ sps.hstack(gcols).tocsr())
    b_mat.eliminate_zeros()
    b_mat.sort_indices()
    cv_mat.sort_indices()
    return cv_mat, b_mat


def observer(seed, Ny, Nu, hN=12, gain=1.):
    """`dict(ha, hb, hc, inihx, dvec)` from `default_rng(100 + seed)`"""
    rng = np.random.default_rng(100 + seed)
    ha = -5.*np.eye(hN) + rng.standard_normal((hN, hN))
    hb = rng.standard_normal((hN, Ny))
    hc = gain*rng.standard_normal((Nu, hN))
    inihx = 0.1*rng.standard_normal((hN, 1))
    dvec = rng.standard_normal((hN, 1))
    return dict(ha=ha, hb=hb, hc=hc, inihx=inihx, dvec=dvec)


def drift_of(dvec):
    def drift(t):
        return np.sin(7*t)*dvec
    return drift


def csr_pack(prefix, mat):
    mat = sps.csr_matrix(mat)
    mat.sort_indices()
    return {prefix+'_data': mat.data, prefix+'_indices': mat.indices,
            prefix+'_indptr': mat.indptr, prefix+'_shape': np.array(mat.shape)}


def csr_unpack(dat, prefix):
    return sps.csr_matrix((dat[prefix+'_data'], dat[prefix+'_indices'],
                           dat[prefix+'_indptr']),
                          shape=tuple(dat[prefix+'_shape']))


def mnorm(M, x):
    x = np.asarray(x).reshape((-1, 1))
    return float(np.sqrt((x.T @ (M @ x)).item()))
