// extern "C" entry points of the small resident helpers around the solver
// (included by dns_amd.hip): CSR operators kept in HBM and the Dirichlet
// scatter `append_bcs_vec`.

namespace dns {

// full = NaN; full[invinds] = v; full[bcinds] = bcvals  (dts:49-64).  `last`
// marks, for an index listed more than once, the occurrence NumPy's fancy
// assignment lets win (the last one) -- computed on the host at create time so
// that the parallel scatter is deterministic.
__global__ void __launch_bounds__(kBlock)
k_bc_scatter(int vdim, int ninv, const int *__restrict__ invinds,
             const double *__restrict__ v, int nbc,
             const int *__restrict__ bcinds, const unsigned char *__restrict__ last,
             const unsigned char *__restrict__ shadowed,
             const double *__restrict__ bcvals, double *__restrict__ full) {
    const int tid = blockIdx.x * kBlock + threadIdx.x;
    const int nth = gridDim.x * kBlock;
    // phase split by target: a full-space entry is written by exactly one
    // thread -- inner entries that a boundary index shadows are skipped
    for (int i = tid; i < ninv; i += nth)
        if (!shadowed[i]) full[invinds[i]] = v[i];
    for (int k = tid; k < nbc; k += nth)
        if (last[k]) full[bcinds[k]] = bcvals[k];
}

__global__ void __launch_bounds__(kBlock)
k_fill_nan_except(int vdim, const unsigned char *__restrict__ covered,
                  double *__restrict__ full) {
    const double nanv = __longlong_as_double(0x7ff8000000000000LL);
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < vdim;
         i += gridDim.x * kBlock)
        if (!covered[i]) full[i] = nanv;
}

}  // namespace dns

struct dns_op {
    int device = 0;
    hipStream_t stream = nullptr;
    dns::CsrDev A;
    dns::DevBuf<double> x, y;
    ~dns_op() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct dns_bcmap {
    int device = 0, vdim = 0, ninv = 0, nbc = 0;
    hipStream_t stream = nullptr;
    dns::DevBuf<int> invinds, bcinds;
    dns::DevBuf<unsigned char> last, shadowed, covered;
    dns::DevBuf<double> v, bcvals, full;
    ~dns_bcmap() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

extern "C" {

int dns_op_create(int device, const dns_csr *a, dns_op **out) try {
    if (!out) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null output handle");
    *out = nullptr;
    DNS_TRY(dns::check_csr(a, "A"));
    DNS_HIP(hipSetDevice(device));
    auto op = std::make_unique<dns_op>();
    op->device = device;
    if (hipStreamCreateWithFlags(&op->stream, hipStreamNonBlocking) != hipSuccess)
        return dns::fail(DNS_ERR_HIP, "hipStreamCreate failed");
    DNS_TRY(op->A.upload(a, op->stream));
    DNS_TRY(op->x.alloc((size_t)std::max(1, a->ncols)));
    DNS_TRY(op->y.alloc((size_t)std::max(1, a->nrows)));
    if (hipStreamSynchronize(op->stream) != hipSuccess)
        return dns::fail(DNS_ERR_HIP, "stream sync failed");
    *out = op.release();
    return DNS_OK;
} DNS_CAPI_CATCH

void dns_op_destroy(dns_op *op) {
    if (!op) return;
    (void)hipSetDevice(op->device);
    if (op->stream) (void)hipStreamSynchronize(op->stream);
    delete op;
}

int dns_op_apply(dns_op *op, const double *x, double *y, double alpha,
                 double beta) try {
    if (!op || !x || !y) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_HIP(hipSetDevice(op->device));
    const size_t nr = (size_t)op->A.nrows, nc = (size_t)op->A.ncols;
    DNS_TRY(op->x.upload(x, nc, op->stream));
    if (beta != 0.0) DNS_TRY(op->y.upload(y, nr, op->stream));
    // (in place: y = alpha A x + beta y; the kernel reads b[row] and writes
    // y[row] of its own rows only)
    const int variant = (op->A.nnz > 4000000 && op->A.c16.p)
                            ? DNS_SPMV_STREAM16 : DNS_SPMV_VECTOR;
    DNS_TRY(dns::launch_spmv(op->A, op->x.p, op->y.p, alpha, beta,
                             beta != 0.0 ? op->y.p : nullptr, variant,
                             op->stream));
    DNS_TRY(op->y.download(y, nr, op->stream));
    DNS_HIP(hipStreamSynchronize(op->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_bcmap_create(int device, int32_t vdim, int32_t ninv,
                     const int32_t *invinds, int32_t nbc, const int32_t *bcinds,
                     dns_bcmap **out) try {
    if (!out || vdim < 1 || ninv < 0 || nbc < 0 || (ninv > 0 && !invinds) ||
        (nbc > 0 && !bcinds))
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    *out = nullptr;
    std::vector<unsigned char> covered((size_t)vdim, 0), isbc((size_t)vdim, 0);
    std::vector<unsigned char> last((size_t)std::max(1, nbc), 0),
        shadowed((size_t)std::max(1, ninv), 0);
    std::vector<int> lastpos((size_t)vdim, -1);
    for (int k = 0; k < nbc; ++k) {
        if (bcinds[k] < 0 || bcinds[k] >= vdim)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "boundary index %d out of range", bcinds[k]);
        lastpos[bcinds[k]] = k;
        isbc[bcinds[k]] = 1;
        covered[bcinds[k]] = 1;
    }
    for (int k = 0; k < nbc; ++k) last[k] = lastpos[bcinds[k]] == k;
    std::vector<int> lastinv((size_t)vdim, -1);
    for (int i = 0; i < ninv; ++i) {
        if (invinds[i] < 0 || invinds[i] >= vdim)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "inner index %d out of range", invinds[i]);
        lastinv[invinds[i]] = i;
        covered[invinds[i]] = 1;
    }
    // the boundary values are written after the inner ones (dts:61-62): an
    // inner entry survives only where no boundary index names the same dof,
    // and of repeated inner indices the last
    for (int i = 0; i < ninv; ++i)
        shadowed[i] = isbc[invinds[i]] || lastinv[invinds[i]] != i;
    DNS_HIP(hipSetDevice(device));
    auto m = std::make_unique<dns_bcmap>();
    m->device = device;
    m->vdim = vdim;
    m->ninv = ninv;
    m->nbc = nbc;
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess)
        return dns::fail(DNS_ERR_HIP, "hipStreamCreate failed");
    DNS_TRY(m->invinds.alloc((size_t)std::max(1, ninv)));
    DNS_TRY(m->bcinds.alloc((size_t)std::max(1, nbc)));
    DNS_TRY(m->last.alloc(last.size()));
    DNS_TRY(m->shadowed.alloc(shadowed.size()));
    DNS_TRY(m->covered.alloc(covered.size()));
    DNS_TRY(m->v.alloc((size_t)std::max(1, ninv)));
    DNS_TRY(m->bcvals.alloc((size_t)std::max(1, nbc)));
    DNS_TRY(m->full.alloc((size_t)vdim));
    if (ninv > 0)
        DNS_TRY(m->invinds.upload(invinds, (size_t)ninv, m->stream));
    if (nbc > 0) DNS_TRY(m->bcinds.upload(bcinds, (size_t)nbc, m->stream));
    DNS_TRY(m->last.upload(last.data(), last.size(), m->stream));
    DNS_TRY(m->shadowed.upload(shadowed.data(), shadowed.size(), m->stream));
    DNS_TRY(m->covered.upload(covered.data(), covered.size(), m->stream));
    if (hipStreamSynchronize(m->stream) != hipSuccess)
        return dns::fail(DNS_ERR_HIP, "stream sync failed");
    *out = m.release();
    return DNS_OK;
} DNS_CAPI_CATCH

void dns_bcmap_destroy(dns_bcmap *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    delete m;
}

int dns_bc_scatter(dns_bcmap *m, const double *v_inner, const double *bcvals,
                   double *out_full) try {
    if (!m || !out_full || (m->ninv > 0 && !v_inner) || (m->nbc > 0 && !bcvals))
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_HIP(hipSetDevice(m->device));
    if (m->ninv > 0) DNS_TRY(m->v.upload(v_inner, (size_t)m->ninv, m->stream));
    if (m->nbc > 0) DNS_TRY(m->bcvals.upload(bcvals, (size_t)m->nbc, m->stream));
    hipLaunchKernelGGL(dns::k_fill_nan_except, dns::grid_for_elems(m->vdim),
                       dns::kBlock, 0, m->stream, m->vdim, m->covered.p,
                       m->full.p);
    hipLaunchKernelGGL(dns::k_bc_scatter,
                       dns::grid_for_elems(std::max(m->ninv, m->nbc)),
                       dns::kBlock, 0, m->stream, m->vdim, m->ninv,
                       m->invinds.p, m->v.p, m->nbc, m->bcinds.p, m->last.p,
                       m->shadowed.p, m->bcvals.p, m->full.p);
    DNS_HIP(hipGetLastError());
    DNS_TRY(m->full.download(out_full, (size_t)m->vdim, m->stream));
    DNS_HIP(hipStreamSynchronize(m->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

}  // extern "C"
