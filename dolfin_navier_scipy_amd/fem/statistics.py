"""Flow statistics of a time loop as running sums: mean flow, mean pressure,
variances, covariances of listed index pairs (Reynolds shear stress), by bins
(phase averages, batch means).

With `x = [v; p]` of a step that goes into bin `b`

    N_b += 1,  S1_b += x,  S2_b += x**2,  SX_b[q] += x[pi[q]]*x[pj[q]]

-- the definition the device kernel follows (`csrc/stats.hpp`,
`ImexStepper.set_statistics`); `FlowStatistics.add` is its NumPy statement.
`cnab` / `sbdftwo` take a `FlowStatistics` as `resident=dict(statistics=fs)`
and fill it, on the device where the loop runs resident.
"""
import numpy as np

__all__ = ['FlowStatistics', 'component_pairs']


def component_pairs(th, invinds):
    """the inner-index pairs `(vx, vy)` of every node of the Taylor-Hood space
    `th` whose two components are both free (`invinds`: the inner dofs of the
    full velocity vector; full-space dof of a node: `2*node + component`),
    `(npairs, 2)` int32 -- what the Reynolds shear stress `<u'v'>` needs"""
    inv = np.asarray(invinds, dtype=np.int64).reshape(-1)
    pos = -np.ones(int(th.vdim), dtype=np.int64)
    pos[inv] = np.arange(inv.size)
    px, py = pos[0::2], pos[1::2]
    both = (px >= 0) & (py >= 0)
    return np.stack([px[both], py[both]], axis=1).astype(np.int32)


class FlowStatistics(object):
    """running sums of `[v; p]` over the steps of a time loop

    `pairs`: `(npairs, 2)` indices into `[0, NV + NP)` (velocity dofs first)
    whose products are summed, None: none.  `nbins` bins; `bin_of(t) -> int`
    says which one the state at time `t` goes into, `-1`: none (default: bin 0
    for `t >= t_start`, every time if `t_start` is None).  The sums (`counts`,
    `s1_v`, `s1_p`, `s2_v`, `s2_p`, `sx`) appear with the first state."""

    KEYS = ('counts', 's1_v', 's1_p', 's2_v', 's2_p', 'sx')

    def __init__(self, pairs=None, nbins=1, bin_of=None, t_start=None):
        self.nbins = int(nbins)
        if not 1 <= self.nbins <= 256:
            raise ValueError('`nbins` = {0} outside 1..256'.format(nbins))
        pr = np.zeros((0, 2), dtype=np.int32) if pairs is None else \
            np.asarray(pairs)
        if pr.size == 0:
            pr = np.zeros((0, 2), dtype=np.int32)
        if pr.ndim != 2 or pr.shape[1] != 2 or pr.min(initial=0) < 0:
            raise ValueError('`pairs` must be npairs x 2 indices')
        self.pairs = np.ascontiguousarray(pr, dtype=np.int32)
        self.t_start = t_start
        self._bin_of = bin_of
        self.counts = np.zeros(self.nbins, dtype=np.int64)
        self.s1_v = self.s1_p = self.s2_v = self.s2_p = self.sx = None

    def bin_of(self, t):
        if self._bin_of is not None:
            b = int(self._bin_of(t))
            if not -1 <= b < self.nbins:
                raise ValueError('bin_of({0}) = {1} outside -1..{2}'.format(
                    t, b, self.nbins - 1))
            return b
        return 0 if (self.t_start is None or t >= self.t_start) else -1

    def bins(self, times):
        """the bin table of the steps towards `times`, int32"""
        return np.array([self.bin_of(t) for t in times], dtype=np.int32)

    def _room(self, NV, NP):
        if self.s1_v is None:
            if self.pairs.size and self.pairs.max() >= NV + NP:
                raise ValueError('`pairs`: indices into [0, NV + NP) = '
                                 '[0, {0})'.format(NV + NP))
            self.s1_v, self.s2_v = (np.zeros((self.nbins, NV))
                                    for _ in range(2))
            self.s1_p, self.s2_p = (np.zeros((self.nbins, NP))
                                    for _ in range(2))
            self.sx = np.zeros((self.nbins, self.pairs.shape[0]))
        elif self.s1_v.shape[1] != NV or self.s1_p.shape[1] != NP:
            raise ValueError('a state of another size than the sums')

    def add(self, v, p, t):
        """the state `(v, p)` at time `t`, by the definition"""
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        self._room(v.size, p.size)
        b = self.bin_of(t)
        if b < 0:
            return
        x = np.concatenate([v, p])
        self.counts[b] += 1
        self.s1_v[b] += v
        self.s1_p[b] += p
        self.s2_v[b] += v*v
        self.s2_p[b] += p*p
        self.sx[b] += x[self.pairs[:, 0]]*x[self.pairs[:, 1]]

    def add_sums(self, sums):
        """sums formed elsewhere (`ImexStepper.statistics()`) on top"""
        self._room(sums['s1_v'].shape[1], sums['s1_p'].shape[1])
        self.counts += np.asarray(sums['counts'], dtype=np.int64)
        for key in self.KEYS[1:]:
            getattr(self, key)[...] += sums[key]

    def sums(self):
        return {key: getattr(self, key) for key in self.KEYS}

    def _over_n(self, arr):
        """`arr / N` per bin, NaN where the bin is empty"""
        if arr is None:
            raise ValueError('no state was added yet')
        cnt = np.where(self.counts > 0, self.counts, 1).astype(np.float64)
        out = arr/cnt[:, None]
        out[self.counts == 0] = np.nan
        return out

    def mean(self):
        """`(mean v (nbins, NV), mean p (nbins, NP))`"""
        return self._over_n(self.s1_v), self._over_n(self.s1_p)

    def variance(self):
        """`(var v, var p)` = `S2/N - (S1/N)**2` per entry"""
        mv, mp = self.mean()
        return (self._over_n(self.s2_v) - mv*mv,
                self._over_n(self.s2_p) - mp*mp)

    def covariance(self):
        """`SX/N - mean[pi]*mean[pj]` of the pairs, `(nbins, npairs)`"""
        m = np.hstack(self.mean())
        return self._over_n(self.sx) \
            - m[:, self.pairs[:, 0]]*m[:, self.pairs[:, 1]]
