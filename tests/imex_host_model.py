"""A host model of what `time_int_utils.cnab` / `sbdftwo` drive, so that their
loop -- all of it host Python -- runs without a device: `install` puts

 * `HostSystem` in place of `_device_system`'s `SaddleSystem`: the sparse LU
   of `oracle.saddle_oracle.SaddleLU(F, J)`,
 * `HostStepper` in place of `ImexStepper`: the step as `include/dns_amd.h`
   states it,
       rhs_v = R1 (a_c v_c + a_p v_p) + cn_c nfc_c + cn_o nfc_o + g,
       one direct solve,  p = pscale p~,
   with `step` rotating the velocity and the convection history, and
 * `oracle.saddle_oracle.solve_sadpnt_smw` in place of the Heun start's
   `lau.solve_sadpnt_smw`.

`StubConvection` stands for a `convection.ConvectionP2`: its `eval(v, row)`
calls the scenario's `f_vdp(appndbcs(v, values of that row))`.  No attachment
of the device is modelled (recorder, functionals, statistics, resident
feedback): those stay GPU-tested.  `HostStepper.made` lists the steppers since
`install`; `glog` of each holds the `g` every step solved with."""
import types

import numpy as np
import scipy.sparse as sps

from oracle import saddle_oracle


class HostSystem(object):
    schur_hierarchy = None

    def __init__(self, F, J):
        self.lu = saddle_oracle.SaddleLU(F, J)
        self.NP, self.NV = J.shape

    def precond_info(self):
        return dict(kind='direct')

    def close(self):
        pass


class HostStepper(object):
    made = []

    def __init__(self, system, R1):
        self.sys, self.R1 = system, sps.csr_matrix(R1)
        self.total_steps = self.total_iters = self.run_calls = 0
        self.g = self.gp = self.table = self.conv = None
        self.glog = []
        HostStepper.made.append(self)

    @staticmethod
    def coeffs(extrapolate=True, carry_residual=True, **kw):
        return types.SimpleNamespace(**kw)

    def set_state(self, v_c, v_p=None, ptilde_c=None, nfc_c=None, nfc_o=None):
        zero = np.zeros((self.sys.NV, 1))
        self.v_c, self.v_p = v_c, (zero if v_p is None else v_p)
        self.nfc_c = zero if nfc_c is None else nfc_c
        self.nfc_o = zero if nfc_o is None else nfc_o

    def set_convection(self, conv, scale=-1.0):
        self.conv = conv

    def set_rhs(self, gvec=None, rhsp=None):
        self.g = self.g if gvec is None else gvec
        self.gp = self.gp if rhsp is None else rhsp
        self.table = None

    def set_rhs_table(self, gv=None, gp=None):
        self.table, self.pos = (np.array(gv), np.array(gp)), 0

    def step(self, cf, nfc_new=None, opts=None):
        NV = self.sys.NV
        if self.table is not None:
            self.g, self.gp = (t[self.pos].reshape((-1, 1))
                               for t in self.table)
        if nfc_new is None and self.conv is not None:
            nfc_new = self.conv.eval(
                self.v_c, None if self.table is None else self.pos)
        if nfc_new is not None:
            self.nfc_o, self.nfc_c = self.nfc_c, nfc_new
        self.glog.append(np.array(self.g, dtype=np.float64).reshape(-1))
        rhs = self.R1 @ (cf.a_c*self.v_c + cf.a_p*self.v_p) \
            + cf.cn_c*self.nfc_c + cf.cn_o*self.nfc_o + self.g
        x = self.sys.lu(np.vstack([rhs, self.gp]).flatten())
        self.v_p, self.v_c = self.v_c, x[:NV].reshape((NV, 1))
        self.p = cf.pscale*x[NV:].reshape((-1, 1))
        self.total_steps += 1
        if self.table is not None:
            self.pos += 1

    def run(self, nsteps, cf, opts=None):
        for _ in range(nsteps):
            self.step(cf)
        self.run_calls += 1

    def get_state(self):
        return self.v_c, self.p

    def vnorm(self):
        return np.linalg.norm(self.v_c)

    def close(self):
        pass


class StubConvection(object):
    """`nstatic`: leading (static) values of a row, which the scenario's
    `appndbcs` does not take"""

    def __init__(self, f_vdp, appndbcs, nstatic=0):
        self.f_vdp, self.appndbcs, self.nstatic = f_vdp, appndbcs, nstatic
        self.vals, self.table = [], None

    def host_callback(self, invinds):
        return self.f_vdp

    def set_dbcvals(self, vals):
        self.vals, self.table = list(vals), None

    def set_dbc_table(self, table):
        self.table = np.array(table)

    def eval(self, v, row):
        vals = self.vals if (self.table is None or row is None) \
            else self.table[row].tolist()
        return self.f_vdp(self.appndbcs(v, vals[self.nstatic:]))


def _direct_solve(krylov=None, krpslvprms=None, **kw):
    return saddle_oracle.solve_sadpnt_smw(**kw)


def install(monkeypatch):
    """the `time_int_utils` module with the host model behind it"""
    from dolfin_navier_scipy_amd import time_int_utils as tiu
    monkeypatch.setattr(tiu, '_device_system',
                        lambda F, J, prm: (HostSystem(F, J), None))
    monkeypatch.setattr(tiu, 'ImexStepper', HostStepper)
    monkeypatch.setattr(tiu.lau, 'solve_sadpnt_smw', _direct_solve)
    monkeypatch.setattr(HostStepper, 'made', [])
    return tiu
