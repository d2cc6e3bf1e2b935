// The host ranges pinned through lamd_host_register / lamd_host_unregister, so that the in-place queue forms can tell whether a column lies in memory the
// runtime holds pinned END TO END (one registration covers it) before they let it cross the bus by DMA from where it is.  Two probe points are not
// enough: a column may span two adjacent registrations, or have a pageable hole in the middle, and an asynchronous copy from such memory has hung the
// runtime.  Host code only (no HIP): tests/test_host_ranges.py compiles it into a host program.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <map>
#include <mutex>

namespace lamd {

class host_ranges {
 public:
  // a range the runtime has pinned ([p, p + bytes)); a second registration at the same base replaces the first
  void add(const void *p, size_t bytes) {
    if (!p || !bytes) return;
    std::lock_guard<std::mutex> lk(mu_);
    r_[(uintptr_t)p] = bytes;
  }
  // the range registered at base p is no longer pinned; false when there is none
  bool remove(const void *p) {
    std::lock_guard<std::mutex> lk(mu_);
    return r_.erase((uintptr_t)p) != 0;
  }
  // [p, p + bytes) lies inside ONE recorded range (ranges that merely touch or overlap one another do not add up)
  bool covers(const void *p, size_t bytes) const {
    const uintptr_t lo = (uintptr_t)p;
    if (!p || !bytes || lo + bytes < lo) return false;
    std::lock_guard<std::mutex> lk(mu_);
    for (auto it = r_.begin(); it != r_.end() && it->first <= lo; ++it)   // every range that begins at or below p (a handful: one per shared block)
      if (lo + bytes <= it->first + it->second) return true;
    return false;
  }
  size_t size() const {
    std::lock_guard<std::mutex> lk(mu_);
    return r_.size();
  }

 private:
  mutable std::mutex mu_;
  std::map<uintptr_t, size_t> r_;  // base -> bytes
};

}  // namespace lamd
