// Shared host-side plumbing for the gfx950 saddle-point library.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dns_amd.h"
#include "status.hpp"

namespace dns {

constexpr int kBlock = 256;      // 4 wavefronts of 64 lanes
constexpr int kWave = 64;
constexpr int kMaxRestart = 64;  // GMRES cycle length bound (DnsCtl arrays)

#define DNS_HIP(call)                                                        \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess)                                               \
            return dns::fail(DNS_ERR_HIP, "%s failed: %s (%s:%d)", #call,    \
                             hipGetErrorString(e__), __FILE__, __LINE__);    \
    } while (0)

// DNS_DEBUG_UPLOADS=1: every copy between HOST memory and the device says
// its host range [ptr, ptr + bytes) on stderr before it is enqueued, so that
// the address of a "Memory access fault by GPU ... on address" report can be
// tied to a buffer and an offset (round 4: a fault at a host heap address
// whose record held no ranges).  Copies of the library's own page-locked
// buffers carry the tags "pinned_h2d" / "pinned_d2h".
inline bool debug_uploads() {
    static const bool on = [] {
        const char *e = getenv("DNS_DEBUG_UPLOADS");
        return e && e[0] != '0' && e[0] != 0;
    }();
    return on;
}
inline void log_host_copy(const char *what, const void *host, const void *dev,
                          size_t bytes) {
    if (!debug_uploads()) return;
    fprintf(stderr, "[dns copy] %-10s host [%p, %p) dev %p bytes %zu\n", what,
            host, (const void *)((const char *)host + bytes), dev, bytes);
    fflush(stderr);
}

// page-locked host memory (hipHostMalloc) owned by the library
template <typename T>
struct PinnedBuf {
    T *p = nullptr;
    size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    int reserve(size_t count) {
        if (count <= n) return DNS_OK;
        release();
        DNS_HIP(hipHostMalloc(reinterpret_cast<void **>(&p),
                              count * sizeof(T), hipHostMallocDefault));
        n = count;
        return DNS_OK;
    }
};

// ---------------------------------------------------------------------------
// THE copy layer: no other code moves bytes between host memory and the
// device (tests/test_capi_cpu.py::test_every_host_copy_goes_through_common_hpp).
//
// Staged copies, for ANY host memory (a caller's array, a std::vector, a
// stack scalar): DevBuf::upload / download, upload_to, download_from and the
// raw staged_h2d / staged_d2h under them.  The DMA engine never sees pageable
// memory.  Twice now (rounds 4 and 5) a run of the GPU suite died with
// "Memory access fault by GPU ... on address <page-aligned HOST heap
// address>" inside a call whose only touch of host memory was a
// hipMemcpyAsync out of pageable memory -- intermittently, at different
// places, every kernel argument accounted for.  For pageable memory the
// runtime pins the pages in place and lets a blit kernel read them; what
// exactly goes wrong there is not established (DNS_DEBUG_UPLOADS prints the
// ranges for whoever looks).  So the CPU copies between the caller's memory
// and a page-locked bounce buffer of this thread, and the DMA engine only
// sees the bounce buffer: 4 MiB chunks, each synchronised, PCIe rate minus a
// few per cent.  A staged copy is COMPLETE when it returns, so the lifetime
// of the host memory after the call is nobody's concern.  It synchronises
// the stream, which an open stream capture cannot take: inside one it fails
// with its name instead of invalidating the capture.
//
// Pinned copies, for the library's PinnedBuf memory (and the trajectory
// export stages) only: h2d_pinned / d2h_pinned only ENQUEUE.  The caller
// synchronises before it reads or refills the host side.
// ---------------------------------------------------------------------------
inline thread_local PinnedBuf<char> g_bounce;
constexpr size_t kBounceChunk = (size_t)4 << 20;

inline int staged_prologue(const char *what, const void *host, const void *dev,
                           size_t bytes, hipStream_t s) {
    log_host_copy(what, host, dev, bytes);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess ||
        cs != hipStreamCaptureStatusNone)
        return fail(DNS_ERR_HIP,
                    "%s: a staged host copy of %zu bytes inside an open "
                    "stream capture", what, bytes);
    return g_bounce.reserve(std::min(bytes, kBounceChunk));
}

inline int staged_h2d(const char *what, void *dev, const void *host,
                      size_t bytes, hipStream_t s) {
    if (bytes == 0) return DNS_OK;
    DNS_TRY(staged_prologue(what, host, dev, bytes, s));
    const char *src = static_cast<const char *>(host);
    char *dst = static_cast<char *>(dev);
    for (size_t off = 0; off < bytes; off += kBounceChunk) {
        const size_t len = std::min(kBounceChunk, bytes - off);
        memcpy(g_bounce.p, src + off, len);
        DNS_HIP(hipMemcpyAsync(dst + off, g_bounce.p, len,
                               hipMemcpyHostToDevice, s));
        DNS_HIP(hipStreamSynchronize(s));
    }
    return DNS_OK;
}

inline int staged_d2h(const char *what, void *host, const void *dev,
                      size_t bytes, hipStream_t s) {
    if (bytes == 0) return DNS_OK;
    DNS_TRY(staged_prologue(what, host, dev, bytes, s));
    char *dst = static_cast<char *>(host);
    const char *src = static_cast<const char *>(dev);
    for (size_t off = 0; off < bytes; off += kBounceChunk) {
        const size_t len = std::min(kBounceChunk, bytes - off);
        DNS_HIP(hipMemcpyAsync(g_bounce.p, src + off, len,
                               hipMemcpyDeviceToHost, s));
        DNS_HIP(hipStreamSynchronize(s));
        memcpy(dst + off, g_bounce.p, len);
    }
    return DNS_OK;
}

// staged, into / out of the middle of a device buffer
template <typename T>
inline int upload_to(T *dev, const T *host, size_t count, hipStream_t s) {
    return staged_h2d("upload_to", dev, host, count * sizeof(T), s);
}
template <typename T>
inline int download_from(T *host, const T *dev, size_t count, hipStream_t s) {
    return staged_d2h("download_from", host, dev, count * sizeof(T), s);
}

// staged, `rows` pieces of `width` entries that lie `dstride` entries apart on
// the device (a column block of a row-major table) into consecutive rows of
// `host`: only the pieces cross the bus, one 2D copy and one synchronisation
// per bounce chunk
template <typename T>
inline int download_rows(T *host, const T *dev, size_t rows, size_t width,
                         size_t dstride, hipStream_t s) {
    if (rows == 0 || width == 0) return DNS_OK;
    if (dstride == width)
        return staged_d2h("download_rows", host, dev, rows * width * sizeof(T),
                          s);
    const size_t wb = width * sizeof(T);
    if (wb > kBounceChunk) {
        for (size_t r = 0; r < rows; ++r)
            DNS_TRY(staged_d2h("download_rows", host + r * width,
                               dev + r * dstride, wb, s));
        return DNS_OK;
    }
    DNS_TRY(staged_prologue("download_rows", host, dev, rows * wb, s));
    const size_t per = std::max<size_t>(1, kBounceChunk / wb);
    DNS_TRY(g_bounce.reserve(std::min(rows, per) * wb));
    for (size_t r = 0; r < rows; r += per) {
        const size_t nr = std::min(per, rows - r);
        DNS_HIP(hipMemcpy2DAsync(g_bounce.p, wb, dev + r * dstride,
                                 dstride * sizeof(T), wb, nr,
                                 hipMemcpyDeviceToHost, s));
        DNS_HIP(hipStreamSynchronize(s));
        memcpy(host + r * width, g_bounce.p, nr * wb);
    }
    return DNS_OK;
}

// pinned: only enqueued on `s`
template <typename T>
inline int h2d_pinned(T *dev, const T *pinned, size_t count, hipStream_t s) {
    log_host_copy("pinned_h2d", pinned, dev, count * sizeof(T));
    DNS_HIP(hipMemcpyAsync(dev, pinned, count * sizeof(T),
                           hipMemcpyHostToDevice, s));
    return DNS_OK;
}
template <typename T>
inline int d2h_pinned(T *pinned, const T *dev, size_t count, hipStream_t s) {
    log_host_copy("pinned_d2h", pinned, dev, count * sizeof(T));
    DNS_HIP(hipMemcpyAsync(pinned, dev, count * sizeof(T),
                           hipMemcpyDeviceToHost, s));
    return DNS_OK;
}

// device buffer with explicit lifetime (no exceptions across the C-ABI)
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    int alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        DNS_HIP(hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T)));
        n = count;
        return DNS_OK;
    }
    // staged: complete on return, ordered on `s` like any other work
    int upload(const T *host, size_t count, hipStream_t s) {
        if (count > n) return fail(DNS_ERR_BAD_ARGUMENT, "upload overflow");
        return staged_h2d("upload", p, host, count * sizeof(T), s);
    }
    int download(T *host, size_t count, hipStream_t s) const {
        if (count > n) return fail(DNS_ERR_BAD_ARGUMENT, "download overflow");
        return staged_d2h("download", host, p, count * sizeof(T), s);
    }
    int zero(hipStream_t s) {
        DNS_HIP(hipMemsetAsync(p, 0, n * sizeof(T), s));
        return DNS_OK;
    }
};

// CSR matrix resident in HBM
struct CsrDev {
    int nrows = 0, ncols = 0;
    int64_t nnz = 0;
    int lpr = 16;                 // lanes per row of the vector kernel
    DevBuf<int> rowptr, colidx;
    DevBuf<double> vals;
    // fp32 copy of the values (operators of the PRECONDITIONER in the
    // bandwidth regime: 6 instead of 10 bytes per non-zero cross the HBM)
    DevBuf<float> vals32;
    // row-block table of the LDS-streaming kernel (built on the host)
    DevBuf<int> rowblocks_t[3];   // tiles of 1024 / 2048 / 4096 non-zeros
    int nrowblocks_t[3] = {0, 0, 0};
    // 16-bit column indices for the 2048 tile: entry = 15-bit offset from one
    // of two bases of its row block (bit 15 selects); c16base[2b] < 0 marks a
    // block whose columns do not fit two 32768-wide windows (read raw)
    DevBuf<unsigned short> c16;
    DevBuf<int> c16base;
    // per row block of the 2048 tile: r0, nr, k0, nn, blo, bhi, 0, 0 -- what
    // the 16-bit streaming kernels read INSTEAD of rowblocks / rowptr / c16base
    // at the head of a tile (passed in the `rowblocks` argument)
    DevBuf<int> meta16;
    int c16_rawblocks = 0;

    int upload(const dns_csr *a, hipStream_t s);
    void release_all() {
        rowptr.release();
        colidx.release();
        vals.release();
        vals32.release();
        for (int t = 0; t < 3; ++t) {
            rowblocks_t[t].release();
            nrowblocks_t[t] = 0;
        }
        c16.release();
        c16base.release();
        meta16.release();
        nrows = ncols = 0;
        nnz = 0;
    }
};

inline int pick_lpr(double avg_nnz_per_row) {
    // smallest power of two that covers an average row in ONE pass of the
    // sub-wave: the reference-size systems are latency bound and every extra
    // pass is another dependent (col,val) -> x[col] round trip
    int lpr = 2;
    while (lpr < 64 && lpr < avg_nnz_per_row) lpr *= 2;
    return lpr;
}

inline int check_csr(const dns_csr *a, const char *name) {
    if (!a || !a->rowptr || (a->nnz > 0 && (!a->colidx || !a->vals)))
        return fail(DNS_ERR_BAD_ARGUMENT, "%s: null CSR arrays", name);
    if (a->nrows < 0 || a->ncols < 0 || a->nnz < 0)
        return fail(DNS_ERR_BAD_ARGUMENT, "%s: negative sizes", name);
    if (a->rowptr[0] != 0 || a->rowptr[a->nrows] != a->nnz)
        return fail(DNS_ERR_BAD_ARGUMENT, "%s: rowptr does not span nnz",
                    name);
    for (int i = 0; i < a->nrows; ++i)
        if (a->rowptr[i + 1] < a->rowptr[i])
            return fail(DNS_ERR_BAD_ARGUMENT, "%s: rowptr not monotone", name);
    for (int64_t k = 0; k < a->nnz; ++k)
        if (a->colidx[k] < 0 || a->colidx[k] >= a->ncols)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "%s: column index %d out of range at %lld", name,
                        a->colidx[k], (long long)k);
    return DNS_OK;
}

}  // namespace dns
