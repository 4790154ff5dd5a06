// alloc_ledger_check.cpp -- the allocation ledger of libspmvhip.so (csrc/hip/alloc_ledger.hpp) over malloc / free, built
// with AddressSanitizer + UBSan (`make ledger`; tests/test_alloc_abi.py runs it).  The backend here answers as the device
// runtime does: a size above BACKEND_LIMIT is refused with error 2 and remembered as the "sticky" last error, a release
// of a pointer it did not hand out is refused with error 1 and never reaches free().
#include <cstdio>
#include <cstdlib>
#include <set>

#include "alloc_ledger.hpp"

using spmvhip::AllocCounts;
using spmvhip::AllocLedger;

namespace {
const size_t BACKEND_LIMIT = (size_t)1 << 30;
std::set<void*> handedOut;
int lastError = 0, backendAllocs = 0, backendFrees = 0;
size_t lastAsked = 0;

int backendAlloc(void** p, size_t bytes) {
    ++backendAllocs;
    lastAsked = bytes;
    if (bytes > BACKEND_LIMIT) { lastError = 2; return 2; }
    *p = malloc(bytes ? bytes : 1);
    if (!*p) { lastError = 2; return 2; }
    handedOut.insert(*p);
    return 0;
}
int backendFree(void* p) {
    ++backendFrees;
    if (!handedOut.erase(p)) { lastError = 1; return 1; }
    free(p);
    return 0;
}

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "alloc_ledger_check: line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

bool same(const AllocCounts& c, unsigned long live, unsigned long bytes, unsigned long peak, unsigned long calls, unsigned long refused,
          unsigned long bad) {
    return c.live == live && c.liveBytes == bytes && c.peakBytes == peak && c.calls == calls && c.refused == refused && c.badFrees == bad;
}
}  // namespace

int main() {
    AllocLedger L(backendAlloc, backendFree, 7);
    void *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;

    // the counters, peakBytes
    CHECK(same(L.counts(), 0, 0, 0, 0, 0, 0));
    CHECK(L.allocate(&a, 100) == 0 && a);
    CHECK(L.allocate(&b, 50) == 0 && b);
    CHECK(same(L.counts(), 2, 150, 150, 2, 0, 0));
    CHECK(L.release(a) == 0);
    CHECK(same(L.counts(), 1, 50, 150, 2, 0, 0));
    CHECK(L.allocate(&a, 30) == 0);
    CHECK(same(L.counts(), 2, 80, 150, 3, 0, 0));          // the peak stays what it was
    CHECK(L.allocate(&c, 200) == 0);
    CHECK(same(L.counts(), 3, 280, 280, 4, 0, 0));
    CHECK(L.release(nullptr) == 0 && same(L.counts(), 3, 280, 280, 4, 0, 0));      // nothing, and no bad release

    // the n-th allocation alone: the backend is asked for the size it cannot give, and its answer is the caller's
    L.arm(1, false);
    CHECK(same(L.counts(), 3, 280, 280, 0, 0, 0));         // calls and refused start again, the rest stays
    lastError = 0;
    CHECK(L.allocate(&d, 10) == 0 && d);                    // number 0
    void* e = (void*)0x1;
    CHECK(L.allocate(&e, 10) == 2 && e == nullptr);         // number 1: refused, the pointer nulled
    CHECK(lastAsked == AllocLedger::REFUSED_BYTES && lastError == 2);
    CHECK(same(L.counts(), 4, 290, 290, 2, 1, 0));
    CHECK(L.allocate(&e, 10) == 0 && e);                    // number 2 passes again
    CHECK(same(L.counts(), 5, 300, 300, 3, 1, 0));
    CHECK(L.release(e) == 0 && L.release(d) == 0);

    // from the n-th on, until disarmed
    L.arm(0, true);
    for (int k = 0; k < 3; ++k) CHECK(L.allocate(&e, 8) == 2 && !e);
    CHECK(same(L.counts(), 3, 280, 300, 3, 3, 0));
    L.arm(2, true);                                         // re-arming: the count starts again
    CHECK(L.allocate(&d, 8) == 0 && L.allocate(&e, 8) == 0);
    void* f = nullptr;
    CHECK(L.allocate(&f, 8) == 2 && L.allocate(&f, 8) == 2 && !f);
    CHECK(same(L.counts(), 5, 296, 300, 4, 2, 0));
    L.arm(-1, false);                                       // disarmed: nothing is refused, the counters start again
    CHECK(L.allocate(&f, 8) == 0 && f);
    CHECK(same(L.counts(), 6, 304, 304, 1, 0, 0));
    CHECK(L.release(d) == 0 && L.release(e) == 0 && L.release(f) == 0);

    // a backend that grants the refused size: the memory goes back and the fallback error is returned
    {
        AllocLedger G([](void** p, size_t) { *p = malloc(1); return 0; }, [](void* p) { free(p); return 0; }, 7);
        G.arm(0, false);
        void* g = nullptr;
        CHECK(G.allocate(&g, 4) == 7 && !g);
        const AllocCounts gc = G.counts();
        CHECK(gc.live == 0 && gc.refused == 1);
    }

    // an allocation that the backend itself refuses is no refusal of the ledger's and is not held
    CHECK(L.allocate(&f, BACKEND_LIMIT + 1) == 2 && !f);
    CHECK(same(L.counts(), 3, 280, 304, 2, 0, 0));

    // a second release and a foreign one: counted, passed on, the backend's answer returned
    const int freesBefore = backendFrees;
    CHECK(L.release(a) == 0);
    CHECK(L.release(a) == 1);
    int local = 0;
    CHECK(L.release(&local) == 1);
    CHECK(backendFrees == freesBefore + 3);
    CHECK(same(L.counts(), 2, 250, 304, 2, 0, 2));
    CHECK(L.release(b) == 0 && L.release(c) == 0);
    CHECK(same(L.counts(), 0, 0, 304, 2, 0, 2));
    CHECK(handedOut.empty());

    if (failures) { fprintf(stderr, "alloc_ledger_check: %d check(s) failed\n", failures); return 1; }
    printf("alloc_ledger_check OK\n");
    return 0;
}
