// device_allocs.hpp -- the one owner of a handle's device and pinned memory.
//
// Every handle of the C ABI embeds one `Allocs`; the handle's pointer fields stay plain `T*` (the launch sites read them
// as before) and Allocs remembers, per allocation, the pointer, how to free it and the ADDRESS OF THE FIELD that holds it.
// These are the only calls of the five runtime allocation / free functions under csrc/ (tests/test_device_allocs_cpu.py
// checks that), so a buffer cannot be allocated without its release being recorded.
//   device / device_finegrained / pinned   allocate into a field; on failure the field is null and nothing is recorded
//   free(field)                            release one allocation and null its field (no-op for a field Allocs does not own:
//                                          a null one, or a non-owning alias such as d_gt[k] or a borrowed block)
//   mark / rollback(mark)                  release everything allocated since the mark, newest first, and null those fields
//   release_all                            release everything, newest first; idempotent; the destructor calls it
// Rules for the code that uses it:
//   * A lazy buffer set (symv_alloc, overlap_setup, multi_setup, resident_setup, side_setup, ellhip_queue_upload, the SVM
//     margins) is all-or-nothing: take a mark, allocate, and on ANY failure roll back to the mark and undo whatever else
//     the call created (events, streams, counts): the handle is exactly as before the call and a later call tries again.
//     The set's "already there" test is therefore only ever true with the whole set in place.
//   * Every *_destroy selects the handle's device (DeviceGuard), drains the handle's streams, calls release_all() while the
//     guard is alive, then destroys events and streams, then deletes the handle.  Memory goes before the streams do.
//   * A temporary that lives for one call is a local Allocs next to the local pointer: every return path frees it.
//   * The recorded field addresses must stay valid while the allocation is held: handles live on the heap and are never
//     copied or moved, and Allocs itself cannot be.
// No pool, no caching, no allocator interface: one runtime call per allocation and per release, as before.
// Needs <hip/hip_runtime_api.h> only (host code; a plain C++ compiler can build it).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <new>
#include <vector>

namespace ellhip {

class Allocs {
  public:
    Allocs() = default;
    Allocs(const Allocs&) = delete;
    Allocs& operator=(const Allocs&) = delete;
    ~Allocs() { release_all(); }

    template <typename T>
    hipError_t device(T*& field, size_t bytes) {
        return take(field, DEVICE, [&](void** p) { return hipMalloc(p, bytes); });
    }
    // fine-grained device memory (the host writes it through the PCIe BAR)
    template <typename T>
    hipError_t device_finegrained(T*& field, size_t bytes) {
        return take(field, DEVICE, [&](void** p) { return hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained); });
    }
    template <typename T>
    hipError_t pinned(T*& field, size_t bytes, unsigned flags) {
        return take(field, PINNED, [&](void** p) { return hipHostMalloc(p, bytes, flags); });
    }

    template <typename T>
    void free(T*& field) {
        for (size_t i = held_.size(); i-- > 0;)
            if (held_[i].field == (void*)&field) {
                drop(held_[i]);
                held_.erase(held_.begin() + (std::ptrdiff_t)i);
                return;
            }
    }

    size_t mark() const { return held_.size(); }
    void rollback(size_t mark) {
        while (held_.size() > mark) {
            drop(held_.back());
            held_.pop_back();
        }
    }
    void release_all() { rollback(0); }
    size_t count() const { return held_.size(); }

  private:
    enum Kind : unsigned char { DEVICE, PINNED };
    struct Held {
        void* ptr;
        void* field;             // address of the T* that holds ptr
        void (*clear)(void*);    // nulls that T* (typed: no store through a void**)
        Kind kind;
    };
    std::vector<Held> held_;

    template <typename T, typename F>
    hipError_t take(T*& field, Kind kind, F alloc) {
        field = nullptr;
        try {
            held_.reserve(held_.size() + 1);  // (the record cannot fail once the memory exists)
        } catch (const std::bad_alloc&) {
            return hipErrorOutOfMemory;
        }
        void* p = nullptr;
        const hipError_t e = alloc(&p);
        if (e != hipSuccess) return e;
        field = static_cast<T*>(p);
        held_.push_back({p, (void*)&field, [](void* f) { *static_cast<T**>(f) = nullptr; }, kind});
        return hipSuccess;
    }
    static void drop(const Held& h) {
        if (h.kind == PINNED) (void)hipHostFree(h.ptr);
        else (void)hipFree(h.ptr);
        h.clear(h.field);
    }
};

}  // namespace ellhip
