// rg_grow.h -- the one grower of the engine's staging buffers (d_records, pin_records, the packed pair, d_cells). No HIP in
// here: the caller brings the allocator, so tests/host_check/grow_check.cpp runs it over malloc under the sanitizers.
//   alloc(void **p, size_t bytes) -> E, where E() means success (hipError_t, int);  release(void *p);
//   before_free() -> E: runs only when an old buffer exists (the stream may still read it); its error leaves everything as it was
// A buffer holds `cap` elements of `elem` bytes plus `pad` bytes; capacities are `first` doubled until the need fits.
// When an allocation fails the pointer is nullptr, the capacity 0, the error returned and nothing leaked -- a later call
// whose need would have fitted the old capacity allocates again and never meets a null buffer.
#pragma once
#include <cstddef>

template <typename C> static inline C rg_grow_cap(C need, C first) {
    C cap = first;
    while (cap < need) cap *= 2;
    return cap;
}

// Two buffers of one capacity (a device buffer and its pinned twin) grow as one unit: both exist, or neither.
template <typename T, typename C, typename AllocA, typename FreeA, typename AllocB, typename FreeB, typename Before>
static inline auto rg_grow_pair(T **a, T **b, C *cap, C need, C first, size_t elem, size_t pad, AllocA alloc_a, FreeA free_a,
                                AllocB alloc_b, FreeB free_b, Before before_free) -> decltype(alloc_a((void **)nullptr, (size_t)0)) {
    using E = decltype(alloc_a((void **)nullptr, (size_t)0));
    if (need <= *cap) return E();
    if (*a || *b) {
        const E e = before_free();
        if (e != E()) return e;
        if (*a) free_a(*a);
        if (*b) free_b(*b);
    }
    *a = *b = nullptr;
    *cap = 0;
    const C c = rg_grow_cap(need, first);
    void *pa = nullptr, *pb = nullptr;
    E e = alloc_a(&pa, (size_t)c * elem + pad);
    if (e != E()) return e;
    e = alloc_b(&pb, (size_t)c * elem + pad);
    if (e != E()) {
        free_a(pa);
        return e;
    }
    *a = static_cast<T *>(pa);
    *b = static_cast<T *>(pb);
    *cap = c;
    return E();
}

// One buffer: a pair whose second half does not exist.
template <typename T, typename C, typename Alloc, typename Free, typename Before>
static inline auto rg_grow(T **ptr, C *cap, C need, C first, size_t elem, size_t pad, Alloc alloc, Free release,
                           Before before_free) -> decltype(alloc((void **)nullptr, (size_t)0)) {
    using E = decltype(alloc((void **)nullptr, (size_t)0));
    T *none = nullptr;
    return rg_grow_pair(ptr, &none, cap, need, first, elem, pad, alloc, release,
                        [](void **p, size_t) { return *p = nullptr, E(); }, [](void *) {}, before_free);
}
