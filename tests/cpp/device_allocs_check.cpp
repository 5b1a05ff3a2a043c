// device_allocs_check.cpp -- stand-alone check of csrc/device_allocs.hpp (tests/test_device_allocs_cpu.py builds it with
// AddressSanitizer + UBSan and runs it).  The five runtime calls the header makes are defined HERE, over malloc, with a live
// count per kind and a "fail the k-th allocation" switch; no HIP runtime is linked, so no device is ever opened.
#include "../../ellalgo-rs_amd/csrc/device_allocs.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>

namespace {
std::set<void*> g_device, g_pinned;   // what is live, by the kind of call that made it
int g_calls = 0, g_fail_at = 0;       // allocation calls so far; fail the g_fail_at-th (0: none)
int g_finegrained = 0, g_wrong_free = 0;
unsigned g_last_flags = 0;

hipError_t stand_in_alloc(std::set<void*>& live, void** p, size_t bytes) {
    if (++g_calls == g_fail_at) {
        *p = reinterpret_cast<void*>(0x1);  // (a failing call may leave anything behind: the owner must not keep it)
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    live.insert(*p);
    return hipSuccess;
}
hipError_t stand_in_free(std::set<void*>& live, void* p) {
    if (live.erase(p) != 1) {
        g_wrong_free += 1;  // not live, or made by the other kind of call
        return hipErrorInvalidValue;
    }
    free(p);
    return hipSuccess;
}
size_t live() { return g_device.size() + g_pinned.size(); }

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            g_failed += 1;                                                 \
        }                                                                  \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stand_in_alloc(g_device, p, bytes); }
hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned flags) {
    if (flags == hipDeviceMallocFinegrained) g_finegrained += 1;
    return stand_in_alloc(g_device, p, bytes);
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
    g_last_flags = flags;
    return stand_in_alloc(g_pinned, p, bytes);
}
hipError_t hipFree(void* p) { return stand_in_free(g_device, p); }
hipError_t hipHostFree(void* p) { return stand_in_free(g_pinned, p); }
}

namespace {
struct Handle {  // a handle as the library writes them: plain pointer fields and one owner
    ellhip::Allocs mem;
    double* d_a = nullptr;
    int* d_b = nullptr;
    double* d_fine = nullptr;
    double* h_c = nullptr;
    char* h_d = nullptr;
    bool all_null() const { return !d_a && !d_b && !d_fine && !h_c && !h_d; }
};

// a lazy set of 5 buffers, written as the library's *_setup functions are: mark, allocate, roll back on any failure
hipError_t lazy_set(Handle& h) {
    const size_t mark = h.mem.mark();
    hipError_t e = h.mem.device(h.d_a, 64);
    if (e == hipSuccess) e = h.mem.device(h.d_b, 16);
    if (e == hipSuccess) e = h.mem.device_finegrained(h.d_fine, 32);
    if (e == hipSuccess) e = h.mem.pinned(h.h_c, 128, hipHostMallocMapped);
    if (e == hipSuccess) e = h.mem.pinned(h.h_d, 8, hipHostMallocDefault);
    if (e != hipSuccess) h.mem.rollback(mark);
    return e;
}

void fail_at(int k) {
    g_calls = 0;
    g_fail_at = k;
}

void test_rollback_for_every_k() {
    for (int k = 1; k <= 5; ++k) {
        Handle h;
        double* d_before = nullptr;  // something allocated before the mark stays
        CHECK(h.mem.device(d_before, 8) == hipSuccess);
        fail_at(k);
        CHECK(lazy_set(h) == hipErrorOutOfMemory);
        CHECK(h.all_null());
        CHECK(live() == 1 && d_before != nullptr && h.mem.count() == 1);
        fail_at(0);
        CHECK(lazy_set(h) == hipSuccess);  // the retry
        CHECK(h.d_a && h.d_b && h.d_fine && h.h_c && h.h_d);
        CHECK(live() == 6 && g_device.size() == 4 && g_pinned.size() == 2);
        h.d_a[7] = 1.0;  // (the memory is really there: the sanitizer watches these)
        h.h_d[7] = 1;
    }
    CHECK(live() == 0);  // every Handle went out of scope with its buffers outstanding
}

void test_free_one_through_its_field() {
    Handle h;
    fail_at(0);
    CHECK(lazy_set(h) == hipSuccess);
    void* b = h.d_b;
    void* c = h.h_c;
    h.mem.free(h.d_b);
    CHECK(h.d_b == nullptr && g_device.count(b) == 0 && live() == 4 && h.mem.count() == 4);
    CHECK(h.d_a && h.d_fine && h.h_c && h.h_d);
    h.mem.free(h.h_c);  // a pinned one: it must reach hipHostFree
    CHECK(h.h_c == nullptr && g_pinned.count(c) == 0 && live() == 3);
    h.mem.free(h.d_b);  // a null field, and one the owner never held: nothing happens
    double* alias = h.d_a;
    h.mem.free(alias);
    CHECK(alias == h.d_a && live() == 3 && h.mem.count() == 3);
    CHECK(g_wrong_free == 0);
}

void test_kinds_and_flags() {
    Handle h;
    fail_at(0);
    g_finegrained = 0;
    CHECK(lazy_set(h) == hipSuccess);
    CHECK(g_finegrained == 1 && g_last_flags == hipHostMallocDefault);
    CHECK(g_device.count(h.d_a) && g_device.count(h.d_b) && g_device.count(h.d_fine));
    CHECK(g_pinned.count(h.h_c) && g_pinned.count(h.h_d));
    h.mem.release_all();
    CHECK(g_wrong_free == 0 && live() == 0);  // each kind reached its own free function
}

void test_release_all_twice_and_reuse() {
    Handle h;
    fail_at(0);
    CHECK(lazy_set(h) == hipSuccess);
    h.mem.release_all();
    CHECK(h.all_null() && live() == 0 && h.mem.count() == 0);
    h.mem.release_all();
    CHECK(live() == 0 && g_wrong_free == 0);
    fail_at(2);
    CHECK(lazy_set(h) == hipErrorOutOfMemory);
    CHECK(h.all_null() && live() == 0);
    fail_at(0);
    CHECK(h.mem.device(h.d_a, 24) == hipSuccess);  // the object goes on working after a rollback
    CHECK(h.d_a && live() == 1 && h.mem.count() == 1);
    CHECK(lazy_set(h) == hipSuccess);  // (d_a allocated over: both allocations are held and both are released)
    CHECK(live() == 6);
}

void test_local_owner_of_a_temporary() {
    double* d_tmp = nullptr;
    {
        ellhip::Allocs tmp;
        fail_at(0);
        CHECK(tmp.device(d_tmp, 4 * sizeof(double)) == hipSuccess);
        CHECK(live() == 1);
    }
    CHECK(live() == 0 && d_tmp == nullptr);
}
}  // namespace

int main() {
    test_rollback_for_every_k();
    test_free_one_through_its_field();
    CHECK(live() == 0);
    test_kinds_and_flags();
    test_release_all_twice_and_reuse();
    CHECK(live() == 0);
    test_local_owner_of_a_temporary();
    CHECK(g_wrong_free == 0);
    if (g_failed) return 1;
    printf("device_allocs_check: ok\n");
    return 0;
}
