// host_threads.h — the one host-thread fan-out of the library (plain C++, no HIP).
#pragma once

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace mrag {

// fn(i) once for every i in [0, n), on at most min(threads, n) threads (at least one); the calling
// thread is one of them, and the indices are handed out through one counter. An exception from
// fn on any thread is caught there and stops the hand-out: the result is false (the callers sit
// behind a C ABI and turn it into MRAG_ERR_OOM). A thread that does not start is no error: the
// caller and the threads that did start finish the work. Every started thread is joined on
// every path, so no exception can meet a joinable std::thread.
template <class Fn>
bool for_each_index(int n, int threads, Fn fn) {
  const int nth = std::max(1, std::min(threads, n));
  std::atomic<int> next{0};
  std::atomic<bool> failed{false};
  auto work = [&]() {
    try {
      for (int i = next++; i < n && !failed; i = next++) fn(i);
    } catch (...) {
      failed = true;
    }
  };
  std::vector<std::thread> th;
  try {
    th.reserve((size_t)(nth - 1));
    for (int t = 1; t < nth; ++t) {
#ifdef MRAG_HOST_THREADS_FAIL_AFTER  // the check program only: every start after that many throws
      if (t > MRAG_HOST_THREADS_FAIL_AFTER) throw t;
#endif
      th.emplace_back(work);
    }
  } catch (...) {  // fewer helpers than asked
  }
  work();
  for (auto& x : th) x.join();
  return !failed;
}

}  // namespace mrag
