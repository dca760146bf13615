// Device and pinned host memory of an engine or a replay: zero-filled arenas freed as a whole, and the
// process-wide registry of live allocations that the RLE_AUDIT / RLE_HAZARD checks read.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "host.h"
#include "plan.h"

namespace rle {

// Live device allocations of the process, for the RLE_AUDIT=1 operand-range check and the RLE_HAZARD=1
// level check (plan.h AllocRegistry; it locks internally).  One registry per process: defined in memory.cpp.
AllocRegistry& live_allocs();
// Zero-filled device buffers.  Small ones (< 1 MB: step scratch, vectors, op tables, ...) are
// carved out of 32 MB slabs that are zeroed once, each rounded up to a whole page plus a guard
// page (as a hipMalloc of its own would be padded), so an engine's thousands of buffers cost a
// few hipMalloc / hipMemset calls instead of one synchronised pair each.
struct DevMem {
  static constexpr size_t kSlab = 32u << 20, kSmall = 1u << 20, kPage = 4096;
  std::vector<std::pair<void*, size_t>> ptrs;  // hipMalloc'd blocks (slabs and large buffers)
  char* slab = nullptr;
  size_t slab_used = 0;
  void* fresh(size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    HIPCHK(hipMemset(p, 0, bytes));
    // hipMemset runs on the null stream, which does not order against our
    // non-blocking streams: finish it before any stream touches the buffer.
    HIPCHK(hipDeviceSynchronize());
    ptrs.emplace_back(p, bytes);
    return p;
  }
  void* alloc(size_t bytes) {
    if (bytes == 0) bytes = 16;
    void* p;
    if (bytes >= kSmall) {
      p = fresh(bytes);
    } else {
      const size_t need = (bytes + kPage - 1) / kPage * kPage + kPage;
      if (!slab || slab_used + need > kSlab) {
        slab = static_cast<char*>(fresh(kSlab));
        slab_used = 0;
      }
      p = slab + slab_used;
      slab_used += need;
    }
    live_allocs().add(p, bytes);
    return p;
  }
  template <class T>
  T* make(size_t n) {
    return reinterpret_cast<T*>(alloc(n * sizeof(T)));
  }
  ~DevMem() {
    for (auto& [p, bytes] : ptrs) {
      live_allocs().drop_range(p, bytes);  // the block's buffers (a large buffer, or a slab's carved ones)
      (void)hipFree(p);
    }
  }
};

// Pinned host allocations (coherent, mapped into the device's address space): act-call
// staging and the zero-copy action output.
struct PinMem {
  std::vector<void*> ptrs;
  void* alloc(size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(p, 0, bytes);
    ptrs.push_back(p);
    live_allocs().add(p, bytes);
    return p;
  }
  ~PinMem() {
    for (void* p : ptrs) {
      live_allocs().drop(p);
      (void)hipHostFree(p);
    }
  }
};

// Named device buffers reused across calls (grown on demand, never shrunk): the replay's eager
// entry points (sample_indices, update_priority, ...) allocate once instead of per call.
struct Scratch {
  DevMem mem;
  std::map<std::string, std::pair<void*, size_t>> bufs;
  template <class T>
  T* get(const std::string& name, size_t n) {
    const size_t bytes = std::max<size_t>(n * sizeof(T), 16);
    auto& b = bufs[name];
    if (b.second < bytes) {
      b.first = mem.alloc(bytes);
      b.second = bytes;
    }
    return static_cast<T*>(b.first);
  }
};

}  // namespace rle
