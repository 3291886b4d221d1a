// Host worker threads of the set-up phases (plain host C++: setup.hip, constraints.cpp, symbolic.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

namespace smcp {

// How many threads a phase takes: max(1, min(hardware threads (1 when unknown), max_threads, limits...)); the limits say
// how much work there is to split.
template <class... L>
int host_threads(int64_t max_threads, L... limits) {
  const unsigned hw = std::thread::hardware_concurrency();
  return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)(hw ? hw : 1), max_threads, (int64_t)limits...}));
}

// work(tix) for tix = 0 .. nth - 1.  Thread creation can fail (std::system_error); nothing may propagate across the
// extern "C" boundary, so whatever did not start runs inline.
template <class F>
void run_threads(int nth, F work) {
  if (nth <= 1) { work(0); return; }
  std::vector<std::thread> pool;
  int started = 0;
  try {
    for (; started < nth; ++started) pool.emplace_back(work, started);
  } catch (...) {
  }
  for (int tix = started; tix < nth; ++tix) work(tix);
  for (auto& th : pool) th.join();
}

}  // namespace smcp
