"""Record closed-loop golden vectors by executing the REFERENCE's own `cnab`
and `sbdftwo` with the reference's own observer.

Run where the reference tree exists only (nothing of it is copied):

    python tests/golden/make_golden_feedback.py

The reference's `time_int_utils` is loaded as `make_golden.py` does
(`load_reference_tiu`).  The `dynamic_rhs` handed to its integrators is
composed exactly as its `solve_nse` does (snu:1243-1247) from its
`get_heunab_lti` (tiu:148-196):

    def dynamic_rhs(t, vc=None, memory={}, mode=None):
        cy = cv_mat.dot(vc)
        curu, memory = dyn_obs_fbk(t, vc=cy, memory=memory, mode=mode)
        return b_mat.dot(curu), memory

Inputs: `scenarios.build('plain', seed=5, Nts=48, tE=0.24)` on the toy problem
(NV = 1286); sensors, actuators and observer of `tests/feedback_setup.py`
(Ny = 3 box means of the vertical velocity in the wake, Nu = 2 `M`-weighted
Gaussian bumps behind the obstacle, hN = 12, `drift(t) = sin(7t) d`, rng seed
105).

Written to `tests/golden/imex_{cnab,sbdf2}_feedback_s5.npz`, data only:
  C_*, B_*            CSR triplets of `cv_mat`, `b_mat`
  ha, hb, hc, inihx, dvec   the observer (`drift(t) = sin(7 t) dvec`)
  drift_rows          `drift` at the time grid
  trange, inivel, inip
  times, vels, prss   of every `savevp` (49 time points)
  vfinal, pfinal, ffflag
  cb_t, cb_mode, cb_y, cb_u   what the callback saw and returned, per call
                      (`cb_y` of the `init` call, which sees no output: NaN)
  mem_lastt, mem_lasthx, mem_lastrhs, mem_lastdt   the final observer memory
  open_relv, open_relp      distance of the final state to the open-loop run

Checked when recorded (printed by this script): `ffflag` 0 for both schemes,
and the feedback moves the final state by
  cnab : 5.64e-03 (velocity, M-norm, relative), 2.74e-02 (pressure)
  sbdf2: 5.64e-03, 2.79e-02
(nnz(C) = 65, nnz(B) = 64) -- five orders above the 1e-8 of the GPU tests, so a feedback term that is
missing, late by a step or wrongly scaled cannot pass.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

SEED, NTS, TE = 5, 48, 0.24
MODES = ('init', 'heunpred', 'heuncorr', 'abtwo')


def main():
    import scenarios
    import feedback_setup as fs
    from make_golden import load_reference_tiu
    reftiu = load_reference_tiu()
    prob = scenarios.toy_problem()
    M = prob['smc']['M']
    cv_mat, b_mat = fs.sensors_actuators(prob['th'], prob['invinds'], M)
    obs = fs.observer(SEED, cv_mat.shape[0], b_mat.shape[1])
    drift = fs.drift_of(obs['dvec'])
    print('NV', M.shape[0], 'nnz(C)', cv_mat.nnz, 'nnz(B)', b_mat.nnz)
    for scheme in ('cnab', 'sbdf2'):
        integ = reftiu.cnab if scheme == 'cnab' else reftiu.sbdftwo
        # open loop first (the size of the effect)
        kw, rec, aux = scenarios.build(variant='plain', seed=SEED, Nts=NTS,
                                       tE=TE, prob=prob)
        vo, po, ffo = integ(**kw)
        kw, rec, aux = scenarios.build(variant='plain', seed=SEED, Nts=NTS,
                                       tE=TE, prob=prob)
        dyn_obs_fbk = reftiu.get_heunab_lti(hb=obs['hb'], ha=obs['ha'],
                                            hc=obs['hc'], inihx=obs['inihx'],
                                            drift=drift)
        seen = []

        def dynamic_rhs(t, vc=None, memory={}, mode=None):     # snu:1243-1247
            cy = cv_mat.dot(vc)
            curu, memory = dyn_obs_fbk(t, vc=cy, memory=memory, mode=mode)
            seen.append((t, MODES.index(mode),
                         np.full(cv_mat.shape[0], np.nan) if mode == 'init'
                         else np.array(cy).reshape(-1),
                         np.array(curu).reshape(-1)))
            return b_mat.dot(curu), memory
        mem = {}
        kw.update(dynamic_rhs=dynamic_rhs, dynamic_rhs_memory=mem)
        v, p, ff = integ(**kw)
        times, vels, prss = rec.arrays()
        relv = fs.mnorm(M, v - vo)/fs.mnorm(M, vo)
        relp = np.linalg.norm(p - po)/np.linalg.norm(po)
        out = dict(times=times, vels=vels, prss=prss, vfinal=v, pfinal=p,
                   ffflag=np.array(ff), trange=kw['trange'],
                   inivel=kw['inivel'], inip=kw['inip'],
                   ha=obs['ha'], hb=obs['hb'], hc=obs['hc'],
                   inihx=obs['inihx'], dvec=obs['dvec'],
                   drift_rows=np.array([drift(t)[:, 0]
                                        for t in kw['trange']]),
                   cb_t=np.array([s[0] for s in seen]),
                   cb_mode=np.array([s[1] for s in seen]),
                   cb_y=np.array([s[2] for s in seen]),
                   cb_u=np.array([s[3] for s in seen]),
                   mem_lastt=np.array(mem['lastt']),
                   mem_lasthx=np.array(mem['lasthx']),
                   mem_lastrhs=np.array(mem['lastrhs']),
                   mem_lastdt=np.array(mem['lastdt']),
                   open_relv=np.array(relv), open_relp=np.array(relp))
        out.update(fs.csr_pack('C', cv_mat))
        out.update(fs.csr_pack('B', b_mat))
        fn = os.path.join(HERE, 'imex_{0}_feedback_s{1}.npz'.format(scheme,
                                                                    SEED))
        np.savez_compressed(fn, **out)
        print(fn, vels.shape, 'ffflag', ff, '(open loop', ffo, ')',
              'effect of the feedback: v %.2e p %.2e' % (relv, relp),
              'calls', len(seen))
        assert ff == 0 and ffo == 0 and relv >= 1e-5


if __name__ == '__main__':
    main()
