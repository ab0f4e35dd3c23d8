"""A NumPy `longdouble` model of the linearised P2 convection about a base flow
`V`, on top of tests/conv_model.py and written from the mathematics: with the
local matrices `n12 = N1(V) + N2(V)` of `conv_model.cell_quantities`,

    forward   L(V) w      per cell:  n12   @ w_cell
    adjoint   L(V)^T w    per cell:  n12.T @ w_cell

(slot = 2 * node + component), gathered over the inner rows like N(u)u.  With
zero Dirichlet values of `w` the gathered adjoint is `(L_II)^T w_I`.

Every quantity has its MAGNITUDE TWIN (the twin of `n12` times `|w_cell|`: the
sum of the absolute values of all terms of the trilinear form), and the bound
of an entry is `gamma_K x twin`, `K` the largest number of roundings a term
passes through in the device kernels (`conv_lin_point`, `conv_adj_point`,
`conv_lin_values` and the tree over the points), counted as in conv_model.py
(a fused multiply-add is one rounding; T: the fp64 tables, `conv_model.T_TAB`
-- a term holds one weight, two shape functions and one gradient, as there):

  forward, cv_i = w_q |T| (grad V_i . w + grad w_i . V):
     gx/gy 3, the gradient sums 6, the values at the point 6, the chain of
     four products (one product, three fma) 4, times the weight 1, the weight
     itself 1, phi_a cv_i 1, tree over the points 3
                                                       K_LIN = 25 + T
  adjoint, slot (a,i) at a point = phi_a cs_i + da_a cw_i:
     first term:  grad V 3 + 6, w at the point 6, s_i = sum_k w_k d_i V_k 2,
        times the weight 1, the weight 1, phi_a cs_i 1, the fma that adds the
        second term 1, tree 3                                         (24)
     second term: V at the point 6, grad phi_a 3, da_a = V . grad phi_a 2,
        w_i at the point 6, times the weight 1, the weight 1, the fma (product
        and sum in one) 1, tree 3                                     (23)
                                                       K_ADJ = 24 + T
  gathers: + len - 1, `scale`: + 1 (as for N(u)u: K + row_len holds both)

`lin_cells_direct` is the second statement: the point formulas of the two
kernels (not the matrices), in any precision, with the sums over points,
nodes and terms in a shuffled order -- the fp64 evaluation
tests/test_conv_lin_model_cpu.py holds against the bounds.

Margins measured on the CPU (`pytest -s tests/test_conv_lin_model_cpu.py`),
largest error / bound: shuffled fp64 evaluation, cells forward 0.140, adjoint
0.148, rows forward 0.130, adjoint 0.134; `TaylorHood.linearised_convection_vec`
(its own count, K_MAT + 4 + cells + nnz of the row) forward 0.021, adjoint
0.023; the two long double statements differ by at most 2.9 long double u x
magnitude.
"""
import numpy as np

import conv_model as cm

LD = cm.LD
K_LIN = 25 + cm.T_TAB
K_ADJ = 24 + cm.T_TAB


def k_of(adjoint):
    return K_ADJ if adjoint else K_LIN


def lin_cells(glam, area, Vl, wl, adjoint, absval=False):
    """`(nc, 12)` cell values in long double from the local matrices of the
    base flow: `n12 @ w_cell` or `n12.T @ w_cell`.  `Vl`, `wl (nc,6,2)`"""
    _, _, n12 = cm.cell_quantities(glam, area, Vl, LD, absval)
    w = np.asarray(wl).reshape(-1, 12).astype(LD)
    if absval:
        w = np.abs(w)
    return np.einsum('cba,cb->ca' if adjoint else 'cab,cb->ca', n12, w)


def lin_cells_direct(glam, area, Vl, wl, adjoint, dtype=np.float64, rng=None):
    """the same cell values by the point formulas of the device kernels, in
    `dtype`; with `rng` every sum is taken in a random order"""
    qw, phi, dphi = cm.tables(dtype)
    glam, area, Vl, wl = (np.asarray(x).astype(dtype)
                          for x in (glam, area, Vl, wl))
    nc = area.size

    def order(n):
        return np.arange(n) if rng is None else rng.permutation(n)

    def ssum(terms, shuffle=True):
        idx = order(len(terms)) if shuffle else range(len(terms))
        s = None
        for i in idx:
            s = terms[i] if s is None else s + terms[i]
        return s
    pts = []
    for q in range(7):
        gphi = ssum([dphi[q][None, :, k, None]*glam[:, None, k, :]
                     for k in range(3)])                          # (nc,6,2)
        ao = order(6)
        wx = ssum([phi[q, a]*wl[:, a, :] for a in ao], False)      # (nc,2)
        Vx = ssum([phi[q, a]*Vl[:, a, :] for a in ao], False)
        gw = ssum([gphi[:, a, None, :]*wl[:, a, :, None] for a in ao], False)
        gV = ssum([gphi[:, a, None, :]*Vl[:, a, :, None] for a in ao], False)
        wt = qw[q]*area                                            # (nc,)
        if not adjoint:
            cv = wt[:, None]*ssum([gV[:, :, 0]*wx[:, None, 0],
                                   gV[:, :, 1]*wx[:, None, 1],
                                   gw[:, :, 0]*Vx[:, None, 0],
                                   gw[:, :, 1]*Vx[:, None, 1]])    # (nc,2)
            pts.append(phi[q][None, :, None]*cv[:, None, :])       # c,a,i
        else:
            # s_i = sum_k w_k d_i V_k,  gV[c, k, i] = d_i V_k
            s = ssum([wx[:, 0, None]*gV[:, 0, :], wx[:, 1, None]*gV[:, 1, :]])
            cs, cw = wt[:, None]*s, wt[:, None]*wx
            da = ssum([Vx[:, None, 0]*gphi[:, :, 0],
                       Vx[:, None, 1]*gphi[:, :, 1]])              # c,a
            pts.append(ssum([phi[q][None, :, None]*cs[:, None, :],
                             da[:, :, None]*cw[:, None, :]]))
    return ssum(pts).reshape(nc, 12)


def lin_model(sp, V_inner, V_dbc, w_inner, w_dbc, adjoint):
    """dict of `(value, bound)` pairs on the condensed space `sp`
    (`conv_model.Space`): `cells (nc,12)` in the caller's cell order and `vec`,
    the inner rows; `mag`: the twin of the cells"""
    Vl, wl = sp.local(V_inner, V_dbc), sp.local(w_inner, w_dbc)
    val = lin_cells(sp.glam, sp.area, Vl, wl, adjoint)
    mag = lin_cells(sp.glam, sp.area, Vl, wl, adjoint, absval=True)
    K = k_of(adjoint)
    return dict(cells=(val, cm.gamma(K)*mag),
                vec=(sp.gather_rows(val),
                     cm.gamma(K + sp.row_len)*sp.gather_rows(mag)),
                mag=mag)
