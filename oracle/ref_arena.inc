// Shared by the oracle/_ref wrapper libraries: operator new on an arena that never reuses memory, so that heap
// addresses grow with creation order (ORBextractor::DistributeOctTree orders equal-sized nodes by address,
// ORBextractor.cc:675).  The version scripts keep these definitions local to each library.  Thread-safe (the Frame
// constructor runs its two extractors on two threads).
#include <sys/mman.h>

#include <atomic>
#include <cstdlib>
#include <new>

namespace {
char *arena_base = nullptr;
std::atomic<size_t> arena_used(0);
const size_t ARENA_BYTES = 16ull << 30;       // virtual, MAP_NORESERVE
std::atomic<bool> arena_on(false);
void arena_prepare() {
    if (!arena_base) {
        void *p = mmap(nullptr, ARENA_BYTES, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) std::abort();
        arena_base = static_cast<char *>(p);
    }
}
void *arena_alloc(size_t n) {
    n = (n + 15) & ~size_t(15);
    const size_t at = arena_used.fetch_add(n);
    if (at + n > ARENA_BYTES) std::abort();
    return arena_base + at;
}
bool in_arena(const void *p) { return arena_base && p >= arena_base && p < arena_base + ARENA_BYTES; }
void arena_begin(bool on) { arena_prepare(); arena_used = 0; arena_on = on; }
void arena_end() {
    if (arena_on && arena_used) madvise(arena_base, arena_used, MADV_DONTNEED);
    arena_on = false;
}
}  // namespace

void *operator new(size_t n) { return arena_on ? arena_alloc(n) : std::malloc(n ? n : 1); }
void *operator new[](size_t n) { return arena_on ? arena_alloc(n) : std::malloc(n ? n : 1); }
void *operator new(size_t n, const std::nothrow_t &) noexcept { return arena_on ? arena_alloc(n) : std::malloc(n ? n : 1); }
void *operator new[](size_t n, const std::nothrow_t &) noexcept { return arena_on ? arena_alloc(n) : std::malloc(n ? n : 1); }
void operator delete(void *p, const std::nothrow_t &) noexcept { if (p && !in_arena(p)) std::free(p); }
void operator delete[](void *p, const std::nothrow_t &) noexcept { if (p && !in_arena(p)) std::free(p); }
void operator delete(void *p) noexcept { if (p && !in_arena(p)) std::free(p); }
void operator delete[](void *p) noexcept { if (p && !in_arena(p)) std::free(p); }
void operator delete(void *p, size_t) noexcept { if (p && !in_arena(p)) std::free(p); }
void operator delete[](void *p, size_t) noexcept { if (p && !in_arena(p)) std::free(p); }
