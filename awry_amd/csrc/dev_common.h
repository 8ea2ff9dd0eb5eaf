// dev_common.h -- error types and the guarded C ABI wrapper, HIP_CHECK, device and pinned buffers, runtime flags -> template arguments
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

#include "../../include/awry_hip.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <set>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "accel_plan.h"
#include "alphabet.h"
#include "count_plan.h"
#include "host_index.h"
#include "host_pack.h"
#include "kernels.hip.h"
#include "mismatch_kernels.hip.h"
#include "sais.hpp"

using namespace awry;

namespace {

thread_local std::string g_last_error;

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };
struct QueryError : std::runtime_error { using std::runtime_error::runtime_error; };
struct NoDeviceError : std::runtime_error { using std::runtime_error::runtime_error; };

#define HIP_CHECK(expr)                                                                              \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                            \
      throw HipError(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" + __FILE__ + ":" + \
                     std::to_string(__LINE__) + ")");                                                \
  } while (0)

template <class F>
int guarded(F&& fn) {
  try {
    fn();
    return AWRY_OK;
  } catch (const HipError& e) { g_last_error = e.what(); return AWRY_ERR_HIP;
  } catch (const ArgError& e) { g_last_error = e.what(); return AWRY_ERR_ARG;
  } catch (const QueryError& e) { g_last_error = e.what(); return AWRY_ERR_INVALID_QUERY;
  } catch (const NoDeviceError& e) { g_last_error = e.what(); return AWRY_ERR_NO_DEVICE;
  } catch (const std::bad_alloc&) { g_last_error = "out of host memory"; return AWRY_ERR_OOM;
  } catch (const std::invalid_argument& e) { g_last_error = e.what(); return AWRY_ERR_FORMAT;
  } catch (const std::exception& e) { g_last_error = e.what(); return AWRY_ERR_IO;
  } catch (...) { g_last_error = "unknown error"; return AWRY_ERR_IO; }
}

template <class T>
struct DevBuf {  // RAII device allocation on the current device
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  explicit DevBuf(size_t count) { alloc(count); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; return *this; }
  ~DevBuf() { reset(); }
  void alloc(size_t count) {
    reset();
    n = count;
    if (count) {
      hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
      if (e != hipSuccess) { p = nullptr; n = 0; throw HipError(std::string("hipMalloc failed: ") + hipGetErrorString(e)); }
    }
  }
  void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

template <class T>
struct PinBuf {  // pinned host staging, grows on demand
  T* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  void ensure(size_t n) {
    if (n <= cap) return;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t c = n + n / 4 + 1024;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), c * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) { p = nullptr; throw HipError(std::string("hipHostMalloc failed: ") + hipGetErrorString(e)); }
    cap = c;
  }
};

void require(bool ok, const char* msg) { if (!ok) throw ArgError(msg); }

// Runtime flags -> template arguments: fn is a generic lambda that receives one std::true_type / std::false_type per flag
// (S() is then a constant expression) and is instantiated for every combination -- so a launch site passes only the flags
// that really vary there and spells the others out.  with_alphabet: the same for NUCLEOTIDE / AMINO.
template <class F>
void with_flags(bool a, F&& fn) { if (a) fn(std::true_type{}); else fn(std::false_type{}); }
template <class F>
void with_flags(bool a, bool b, F&& fn) { with_flags(a, [&](auto A) { with_flags(b, [&](auto B) { fn(A, B); }); }); }
template <class F>
void with_flags(bool a, bool b, bool c, F&& fn) { with_flags(a, b, [&](auto A, auto B) { with_flags(c, [&](auto C) { fn(A, B, C); }); }); }
template <class F>
void with_alphabet(int alphabet, F&& fn) {
  if (alphabet == NUCLEOTIDE) fn(std::integral_constant<int, NUCLEOTIDE>{}); else fn(std::integral_constant<int, AMINO>{});
}

}  // namespace
