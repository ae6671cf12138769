// Stream-position signal bindings (csrc/kernels/signal.hip, parallel/ddp.py).
#include <atomic>
#include <chrono>
#include <thread>

#include "common.h"

namespace {

// (host word, its device address, device counter) as integers
std::vector<int64_t> signal_create() {
  unsigned long long *h = nullptr, *d = nullptr, *c = nullptr;
  const int rc = tdg_signal_create(&h, &d, &c);
  TORCH_CHECK(rc == 0, "signal_create failed (rc=", rc, ")");
  return {reinterpret_cast<int64_t>(h), reinterpret_cast<int64_t>(d), reinterpret_cast<int64_t>(c)};
}

// launches the signal kernel on the current stream of `device` (captured
// into a graph when the stream is capturing)
void signal_emit(int64_t dhost, int64_t cnt, int64_t device) {
  hipStream_t st = c10::hip::getCurrentHIPStream(static_cast<c10::DeviceIndex>(device)).stream();
  const int rc = tdg_signal_emit(reinterpret_cast<unsigned long long*>(cnt),
                                 reinterpret_cast<unsigned long long*>(dhost), st);
  TORCH_CHECK(rc == 0, "signal_emit: launch failed");
}

// Spins (pause, then yield) until the host word reaches `expected`; false on
// timeout. Runs without the GIL: the comm thread waits here while the main
// thread keeps launching.
bool signal_wait(int64_t host, int64_t expected, double timeout_s) {
  py::gil_scoped_release nogil;
  const volatile unsigned long long* p = reinterpret_cast<const volatile unsigned long long*>(host);
  const unsigned long long want = static_cast<unsigned long long>(expected);
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  while (*p < want) {
    if (++spins < 4096) {
      __builtin_ia32_pause();
      continue;
    }
    spins = 0;
    std::this_thread::yield();
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
      return false;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return true;
}

int64_t signal_read(int64_t host) {
  return static_cast<int64_t>(*reinterpret_cast<const volatile unsigned long long*>(host));
}

}  // namespace

void def_signal(py::module_& m) {
  m.def("signal_create", &signal_create);
  m.def("signal_emit", &signal_emit);
  m.def("signal_wait", &signal_wait);
  m.def("signal_read", &signal_read);
}
