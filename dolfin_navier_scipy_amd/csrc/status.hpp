// The last-error string, the exception barrier of the C-ABI and what a body
// behind it returns through (DNS_TRY, ScopeExit).
// No HIP in here: tests/host_sanitize.cpp exercises it on the host alone.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <exception>
#include <new>
#include <string>
#include <utility>

#include "../../include/dns_amd.h"

namespace dns {

inline thread_local std::string g_last_error;

inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// the C-ABI is an exception barrier: called from a catch (...) handler, it
// turns the exception in flight into DNS_ERR_HOST with its message
inline int caught() noexcept {
    try {
        throw;
    } catch (const std::bad_alloc &) {
        return fail(DNS_ERR_HOST, "out of host memory");
    } catch (const std::exception &e) {
        return fail(DNS_ERR_HOST, "host-side exception: %s", e.what());
    } catch (...) {
        return fail(DNS_ERR_HOST, "host-side exception");
    }
}

// runs `f` when it goes out of scope: on every return and on an exception
template <typename F>
class ScopeExit {
  public:
    explicit ScopeExit(F f) : f_(std::move(f)) {}
    ScopeExit(const ScopeExit &) = delete;
    ScopeExit &operator=(const ScopeExit &) = delete;
    ~ScopeExit() { f_(); }

  private:
    F f_;
};

}  // namespace dns

// closes the function-try-block of an export that returns a status:
//     int dns_x(args) try { body } DNS_CAPI_CATCH
#define DNS_CAPI_CATCH                                                       \
    catch (...) {                                                            \
        return dns::caught();                                                \
    }

#define DNS_TRY(call)                                                        \
    do {                                                                     \
        int s__ = (call);                                                    \
        if (s__ != DNS_OK) return s__;                                       \
    } while (0)
