// alloc_ledger.hpp -- the book that devMalloc / devFree (abi.hip) keep of the library's device memory, and the switch that
// makes a chosen allocation fail (spmvHipAllocRefuse; for tests, include/spmvHip.h).  Nothing of HIP is included: the
// backend -- two functions that return 0 for success, an error code of their own otherwise -- is passed in, so the same
// text runs over malloc / free on the CPU (tests/harness/alloc_ledger_check.cpp).
//
//   live, liveBytes, peakBytes   the pointers held now, their bytes, the most bytes held at once
//   calls                        allocations asked for since the last arm()
//   refused                      how many of those were refused on purpose
//   badFrees                     releases of a pointer the ledger does not hold (a foreign one, or a second release)
//
// A refused allocation is a real refusal of the backend: it is asked for REFUSED_BYTES, more than any device holds, and
// what it answers is what the caller gets -- the runtime's own error code and its own sticky last error.  A backend that
// grants that size has its memory given back and the allocation fails with `fallbackError`.
// One mutex: allocation happens in builds, never on a launch path.
#pragma once
#include <cstddef>
#include <mutex>
#include <unordered_map>

namespace spmvhip {

struct AllocCounts {
    unsigned long live, liveBytes, peakBytes, calls, refused, badFrees;
};

class AllocLedger {
public:
    typedef int (*AllocFn)(void** p, size_t bytes);
    typedef int (*FreeFn)(void* p);
    static constexpr size_t REFUSED_BYTES = (size_t)1 << 62;

    AllocLedger(AllocFn a, FreeFn f, int fallbackError) : alloc_(a), free_(f), fallback_(fallbackError) {}

    // allocation number n from now (0-based) is refused -- that one alone, or with fromThenOn that one and every later
    // one; n < 0 disarms.  Either way calls and refused start again at 0.
    void arm(long n, bool fromThenOn) {
        std::lock_guard<std::mutex> g(m_);
        c_.calls = c_.refused = 0;
        at_ = n;
        onward_ = fromThenOn;
    }

    int allocate(void** p, size_t bytes) {
        std::lock_guard<std::mutex> g(m_);
        const long k = (long)c_.calls++;
        if (at_ >= 0 && (k == at_ || (onward_ && k > at_))) {
            ++c_.refused;
            void* q = nullptr;
            int e = alloc_(&q, REFUSED_BYTES);
            if (e == 0) { (void)free_(q); e = fallback_; }
            *p = nullptr;
            return e;
        }
        void* q = nullptr;
        const int e = alloc_(&q, bytes);
        if (e != 0) { *p = nullptr; return e; }
        *p = q;
        held_[q] = bytes;
        c_.live = held_.size();
        c_.liveBytes += bytes;
        if (c_.liveBytes > c_.peakBytes) c_.peakBytes = c_.liveBytes;
        return 0;
    }

    // a null pointer is released as free(NULL) is: nothing happens.  A pointer the ledger does not hold is counted and
    // still handed to the backend, whose answer is returned (memory that came from elsewhere is the backend's to judge).
    int release(void* p) {
        if (!p) return 0;
        std::lock_guard<std::mutex> g(m_);
        auto it = held_.find(p);
        if (it == held_.end()) {
            ++c_.badFrees;
            return free_(p);
        }
        c_.liveBytes -= it->second;
        held_.erase(it);
        c_.live = held_.size();
        return free_(p);
    }

    AllocCounts counts() {
        std::lock_guard<std::mutex> g(m_);
        return c_;
    }

private:
    AllocFn alloc_;
    FreeFn free_;
    int fallback_;
    std::mutex m_;
    std::unordered_map<void*, size_t> held_;
    AllocCounts c_{0, 0, 0, 0, 0, 0};
    long at_ = -1;
    bool onward_ = false;
};

}  // namespace spmvhip
