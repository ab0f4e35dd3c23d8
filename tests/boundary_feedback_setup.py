"""The controlled toy problem of the boundary-feedback tests
(`test_boundary_feedback_cpu.py`, `test_gpu_boundary_feedback.py`): the
`movingbc` scenario (the inflow dofs of the 22 x 8 channel are the controlled
boundary) with a `time_int_utils.BoundaryFeedback` in the place of its
`getbcs`.  Sensors and observer come from `feedback_setup`.

 * `s_mat` (nc x Nu): the inflow profile cut into `Nu` contiguous pieces, one
                      control per dof (`b = base + s_mat u`)
 * `base`:            the inflow profile itself, or zero
 * `applybcs`:        the scenario's (the values ARE written), or the literal
                      zero closure
"""
import numpy as np
import scipy.sparse as sps

import feedback_setup as fs
import scenarios


def split(prob):
    """`(statinds, statvals, cntinds, cntbase)`: inflow dofs are controlled"""
    dbcinds, dbcvals = prob['dbcinds'], prob['dbcvals']
    ctrl = np.abs(dbcvals) > 0
    return dbcinds[~ctrl], dbcvals[~ctrl], dbcinds[ctrl], dbcvals[ctrl]


def shape_matrix(cntbase, Nu, scale=1.):
    nc = cntbase.size
    owner = (np.arange(nc)*Nu)//nc
    return sps.csr_matrix((scale*cntbase, (np.arange(nc), owner)),
                          shape=(nc, Nu))


def full_sensors(prob):
    """the sensors of `feedback_setup` over the FULL velocity dofs"""
    inv = np.asarray(prob['invinds'])
    C, _ = fs.sensors_actuators(prob['th'], inv, prob['smc']['M'])
    C = C.tocoo()
    return sps.csr_matrix((C.data, (C.row, inv[C.col])),
                          shape=(C.shape[0], prob['th'].vdim))


def make_feedback(tiu, prob, seed=3, hN=12, Nu=1, gain=.5, base=True,
                  drift=True, zero_gain=False):
    _, _, _, cntbase = split(prob)
    obs = fs.observer(seed, 3, Nu, hN=hN, gain=gain)
    if zero_gain:
        obs['hc'] = np.zeros_like(obs['hc'])
    fb = tiu.BoundaryFeedback(
        full_sensors(prob), shape_matrix(cntbase, Nu), obs['ha'], obs['hb'],
        obs['hc'], obs['inihx'], invinds=prob['invinds'],
        base=cntbase if base else None,
        drift=fs.drift_of(obs['dvec']) if drift else None)
    return fb, obs


def literal_applybcs(NV, NP):
    zv, zp = np.zeros((NV, 1)), np.zeros((NP, 1))

    def applybcs(bcs_n):
        return -zv, -zp, zv.copy()
    return applybcs


def build(tiu, prob, seed=3, Nts=12, tE=0.06, literal=False, getbcs=None,
          **fbkw):
    """`(kw, rec, fb)`: the keywords of `cnab` / `sbdftwo` with the feedback
    as `getbcs` (or the `getbcs` given, `bcs_ini` from it) and `bcs_ini` from
    its `init` call"""
    kw, rec, _ = scenarios.build(variant='movingbc', seed=seed, Nts=Nts,
                                 tE=tE, prob=prob)
    fb = None
    if getbcs is None:
        fb, _ = make_feedback(tiu, prob, seed=seed, **fbkw)
        kw.update(getbcs=fb, bcs_ini=fb(kw['trange'][0], mode='init'))
    else:
        kw.update(getbcs=getbcs,
                  bcs_ini=getbcs(kw['trange'][0], None, None, mode='init'))
    if literal:
        NP, NV = kw['J'].shape
        kw.update(applybcs=literal_applybcs(NV, NP))
    return kw, rec, fb


def toy_cvop(prob):
    """the device convection with the static Dirichlet dofs first, the
    controlled ones behind them; `(cvop, statvals)`"""
    from dolfin_navier_scipy_amd import convection
    statinds, statvals, cntinds, cntbase = split(prob)
    cvop = convection.ConvectionP2.from_taylor_hood(
        prob['th'], prob['invinds'], np.concatenate([statinds, cntinds]),
        np.concatenate([statvals, cntbase]))
    return cvop, statvals.tolist()
