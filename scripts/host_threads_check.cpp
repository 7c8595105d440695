// The host-thread fan-out (csrc/host_threads.h) on its own, for tests/test_host_threads_cpu.py.
// Test infrastructure: nothing in the library calls it. Exit status 0 when every case holds.
//   c++ -std=c++17 -O1 -pthread -I<pkg>/csrc scripts/host_threads_check.cpp -o scripts/host_threads_check
//   host_threads_check                    every case below
//   host_threads_check visit <n> <threads>  every index of [0, n) exactly once, result true, and no
//                                         more than max(1, min(threads, n)) threads took part
//   host_threads_check throw              fn throws on one index of 1000, 8 threads: result false
// -DMRAG_HOST_THREADS_FAIL_AFTER=<k> makes every thread start after the k-th throw: the cases
// hold all the same, on at most k + 1 threads. Also the program to run under -fsanitize=thread
// and -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>

#include "host_threads.h"

namespace {

bool visit(int n, int threads) {
  std::vector<std::atomic<int>> seen((size_t)(n > 0 ? n : 0));
  std::mutex mu;
  std::set<std::thread::id> who;
  const bool ok = mrag::for_each_index(n, threads, [&](int i) {
    seen[(size_t)i]++;
    std::this_thread::yield();  // or the first thread to start is done before the second exists
    std::lock_guard<std::mutex> lk(mu);
    who.insert(std::this_thread::get_id());
  });
  int most = std::max(1, std::min(threads, n));
#ifdef MRAG_HOST_THREADS_FAIL_AFTER
  most = std::min(most, MRAG_HOST_THREADS_FAIL_AFTER + 1);
#endif
  bool good = ok && (int)who.size() <= most;
  for (auto& s : seen) good = good && s == 1;
  std::printf("visit n=%d threads=%d: result %d, %zu thread(s) of at most %d: %s\n", n, threads, (int)ok, who.size(), most,
              good ? "ok" : "FAILED");
  return good;
}

bool throws() {
  std::atomic<int> calls{0};
  const bool ok = mrag::for_each_index(1000, 8, [&](int i) {
    ++calls;
    if (i == 500) throw std::runtime_error("index 500");
  });
  const bool good = !ok && calls <= 1000;  // every thread joined: the program goes on and exits 0
  std::printf("throw on index 500 of 1000, 8 threads: result %d after %d calls: %s\n", (int)ok, (int)calls,
              good ? "ok" : "FAILED");
  return good;
}

}  // namespace

int main(int argc, char** argv) {
  bool good = true;
  if (argc == 4 && std::string(argv[1]) == "visit") {
    good = visit(std::atoi(argv[2]), std::atoi(argv[3]));
  } else if (argc == 2 && std::string(argv[1]) == "throw") {
    good = throws();
  } else {
    for (int n : {0, 1, 7, 1000})
      for (int t : {0, 1, 3, 8, 64}) good = visit(n, t) && good;
    good = throws() && good;
  }
  return good ? 0 : 1;
}
