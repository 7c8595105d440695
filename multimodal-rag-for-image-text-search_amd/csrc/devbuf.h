// devbuf.h — the library's growable buffers: one device type, one pinned-host type, two growth
// rules. A buffer belongs to its holder and is freed with it, which must happen with the
// buffer's device current and after the streams that use it are drained (mrag_knn_destroy,
// mrag_encoder_destroy). Holders that are process globals are never destroyed (jpeg.hip, png.hip,
// imgprep.hip): at process exit their hipFree could meet a HIP runtime that has already shut down.
#pragma once

#include <algorithm>
#include <utility>

#include "common.h"

namespace mrag {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr);
      bytes = std::exchange(o.bytes, 0);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// Pinned host memory (hipHostMallocDefault), owned the same way.
struct PinnedBuf {
  uint8_t* p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { reset(); }
  void reset() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// At least `bytes` (and at least 256): a buffer that is too small is replaced by one of exactly
// that size, its contents dropped; a failing free is reported.
inline int ensure(DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return MRAG_OK;
  if (b.p) {
    MRAG_HIP(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
  }
  const size_t want = std::max<size_t>(bytes, 256);
  MRAG_HIP(hipMalloc(&b.p, want));
  b.bytes = want;
  return MRAG_OK;
}

// At least `bytes`, growing to max(bytes, twice the old size) so that batches of slowly rising
// size do not reallocate every time; contents dropped. An empty buffer gets exactly `bytes`, and
// stays empty (p null) for a request of 0. The caller first waits for whatever still reads the
// old buffer: only it knows the stream.
inline int ensure_doubling(DevBuf& b, size_t bytes) {
  if (bytes <= b.bytes) return MRAG_OK;
  const size_t want = std::max(bytes, b.bytes * 2);
  b.reset();
  MRAG_HIP(hipMalloc(&b.p, want));
  b.bytes = want;
  return MRAG_OK;
}

inline int ensure_doubling(PinnedBuf& b, size_t bytes) {
  if (bytes <= b.bytes) return MRAG_OK;
  const size_t want = std::max(bytes, b.bytes * 2);
  b.reset();
  MRAG_HIP(hipHostMalloc((void**)&b.p, want, hipHostMallocDefault));
  b.bytes = want;
  return MRAG_OK;
}

}  // namespace mrag
