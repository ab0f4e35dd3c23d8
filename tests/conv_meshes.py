"""Synthetic P2 triangulations for the convection tests: a few lines of NumPy,
nothing stored.  Every mesh is a real conforming triangulation (a subset of
the cells of a conforming triangulation is one), handed out as the raw element
data the C API takes: `cell_vdofs (nc, 6, 2)`, `glam (nc, 3, 2)`, `area (nc,)`.

Local node k < 3 is vertex k of the cell, node 3 + k the midpoint of the edge
opposite vertex k; velocity dof = 2 * node + component.  With a `seed` the cell
order and the node numbering are random permutations."""
import numpy as np

# the block edges of the element kernels (32 cells per block with eight lanes
# per cell, 256 with one) and one size with several blocks of both
SIZES = (1, 2, 31, 32, 33, 255, 256, 257, 1000)


class RawMesh(object):
    def __init__(self, verts, cells, seed=None):
        verts = np.asarray(verts, dtype=np.float64)
        cells = np.array(cells, dtype=np.int64)
        p = verts[cells]
        det = ((p[:, 1, 0] - p[:, 0, 0])*(p[:, 2, 1] - p[:, 0, 1])
               - (p[:, 1, 1] - p[:, 0, 1])*(p[:, 2, 0] - p[:, 0, 0]))
        flip = det < 0
        cells[flip, 1], cells[flip, 2] = cells[flip, 2].copy(), \
            cells[flip, 1].copy()
        used = np.unique(cells)                       # drop unused vertices
        renum = np.full(verts.shape[0], -1, dtype=np.int64)
        renum[used] = np.arange(used.size)
        verts, cells = verts[used], renum[cells]
        rng = None if seed is None else np.random.default_rng(seed)
        if rng is not None:
            cells = cells[rng.permutation(cells.shape[0])]
        nv = verts.shape[0]
        loc = np.stack([cells[:, [1, 2]], cells[:, [0, 2]], cells[:, [0, 1]]],
                       axis=1)
        loc = np.sort(loc.reshape(-1, 2), axis=1)
        ukey, inv, cnt = np.unique(loc[:, 0]*nv + loc[:, 1],
                                   return_inverse=True, return_counts=True)
        edges = np.stack([ukey // nv, ukey % nv], axis=1)
        cellnodes = np.hstack([cells, nv + inv.reshape(-1, 3)])
        nnodes = nv + edges.shape[0]
        coords = np.vstack([verts, 0.5*(verts[edges[:, 0]] + verts[edges[:, 1]])])
        on_bnd = np.zeros(nnodes, dtype=bool)
        on_bnd[nv + np.flatnonzero(cnt == 1)] = True
        on_bnd[edges[cnt == 1].ravel()] = True
        if rng is not None:
            newid = rng.permutation(nnodes)
            cellnodes = newid[cellnodes]
            coords2, bnd2 = np.empty_like(coords), np.empty_like(on_bnd)
            coords2[newid], bnd2[newid] = coords, on_bnd
            coords, on_bnd = coords2, bnd2
        self.verts, self.cells = verts, cells
        self.ncells, self.nnodes, self.vdim = cells.shape[0], nnodes, 2*nnodes
        self.cellnodes, self.coords, self.on_boundary = cellnodes, coords, on_bnd
        self.cell_vdofs = 2*cellnodes[:, :, None] + np.arange(2)[None, None, :]
        p = verts[cells]
        self.area = 0.5*((p[:, 1, 0] - p[:, 0, 0])*(p[:, 2, 1] - p[:, 0, 1])
                         - (p[:, 1, 1] - p[:, 0, 1])*(p[:, 2, 0] - p[:, 0, 0]))
        assert self.area.min() > 0
        glam = np.empty((self.ncells, 3, 2))
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            glam[:, k, 0] = (p[:, i, 1] - p[:, j, 1])/(2*self.area)
            glam[:, k, 1] = (p[:, j, 0] - p[:, i, 0])/(2*self.area)
        self.glam = glam

    def cells_per_node(self):
        return np.bincount(self.cellnodes.ravel(), minlength=self.nnodes)

    def split(self, dirichlet='boundary', full_cells=0, seed=0):
        """`(invinds, dbcinds)`.  `dirichlet`: 'boundary' (the nodes of the
        boundary edges), 'none', or a fraction of the nodes drawn at random.
        `full_cells`: the nodes of that many cells are Dirichlet as well --
        cells without an inner dof, which the operator sorts to the end of
        its internal order.  The inner dofs are numbered at random."""
        rng = np.random.default_rng(seed)
        dn = np.zeros(self.nnodes, dtype=bool)
        if dirichlet == 'boundary':
            dn |= self.on_boundary
        elif dirichlet != 'none':
            dn[rng.permutation(self.nnodes)[:int(dirichlet*self.nnodes)]] = True
        for c in rng.permutation(self.ncells)[:full_cells]:
            dn[self.cellnodes[c]] = True
        dd = np.repeat(dn, 2)
        inv = rng.permutation(np.flatnonzero(~dd))
        dbc = rng.permutation(np.flatnonzero(dd))
        return inv.astype(np.int32), dbc.astype(np.int32)


def rectangle(ncells, seed=None, lx=1.3, ly=0.7, decades=0.0):
    """the first `ncells` triangles of a structured `nx x ny` rectangle (rows
    of squares, each split in two); `decades` > 0: the columns shrink
    geometrically, the cell areas span that many decades"""
    ny = max(1, int(round(np.sqrt(ncells/2.0)*0.8)))
    nx = -(-ncells // (2*ny))
    xs = np.linspace(0.0, 1.0, nx + 1)
    if decades:
        w = 10.0**(-decades*np.arange(nx)/max(1, nx - 1))
        xs = np.concatenate([[0.0], np.cumsum(w)/w.sum()])
    ys = np.linspace(0.0, 1.0, ny + 1)**1.3
    X, Y = np.meshgrid(lx*xs, ly*ys, indexing='ij')
    verts = np.stack([X.ravel(), Y.ravel()], axis=1)
    vid = lambda i, j: i*(ny + 1) + j
    cells = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            cells += ([[a, b, c], [a, c, d]] if (i + j) % 2 == 0
                      else [[a, b, d], [b, c, d]])
    return RawMesh(verts, np.array(cells[:ncells]), seed=seed)


def fan(K=40, seed=None):
    """K triangles round one hub vertex; the rim is the boundary"""
    th = 2*np.pi*(np.arange(K) + 0.3*np.sin(1.7*np.arange(K)))/K
    rad = 1.0 + 0.4*np.cos(3*th)
    verts = np.vstack([[0.0, 0.0], np.stack([rad*np.cos(th), rad*np.sin(th)], 1)])
    cells = [[0, 1 + k, 1 + (k + 1) % K] for k in range(K)]
    mesh = RawMesh(verts, np.array(cells), seed=seed)
    mesh.hub_node = int(np.argmax(mesh.cells_per_node()))
    return mesh
