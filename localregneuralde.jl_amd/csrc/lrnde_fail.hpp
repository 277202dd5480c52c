// lrnde_fail.hpp — how every handle of the library reports a failure: the one formatter and the one HIP check.
// A handle type has a `std::string err`; failf(h, code, fmt, ...) writes the message there and returns the code, so a
// call site reads `return fail(c, LRNDE_BADARG, "...", ...)`.  The handles' own spellings (fail / cfail / lat_fail /
// chain_refuse, HIPCHK / CHK / LATCHK) are names for these two.  Host-only; includes nothing of HIP.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

namespace lrnde {

inline int vfailf(std::string* err, int code, const char* fmt, va_list ap) {
  char buf[512];
  vsnprintf(buf, sizeof(buf), fmt, ap);
  if (err) *err = buf;
  return code;
}

// into a string the caller names: Membership (lrnde_comm.hpp), and the create calls, which have no handle yet and
// write a thread-local string
inline int failf(std::string* err, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  const int rc = vfailf(err, code, fmt, ap);
  va_end(ap);
  return rc;
}

// into the handle's err; a null handle gets the code alone
template <class H> int failf(H* h, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  const int rc = vfailf(h ? &h->err : nullptr, code, fmt, ap);
  va_end(ap);
  return rc;
}

}  // namespace lrnde

// `to`: a handle or a std::string*, as for failf
#define LRNDE_HIPCHK(to, x)                                                                                   \
  do {                                                                                                        \
    hipError_t e_ = (x);                                                                                      \
    if (e_ != hipSuccess)                                                                                     \
      return lrnde::failf(to, LRNDE_HIP_ERROR, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, \
                          __LINE__);                                                                          \
  } while (0)
