// device_mem_check.cpp — the invariants of csrc/hip/device_mem.h on the CPU (tests/test_device_mem_host.py builds this with the host
// compiler under AddressSanitizer + UBSan and runs it): Buffer over a malloc / free space that counts live blocks and can be told to
// fail the n-th allocation, and PerStream over plain structs with the device switch a no-op,
// forget_stream over two such registries included. Needs no GPU and links no HIP.
#include "../gradient-based-path-tracing_amd/csrc/hip/device_mem.h"

#include <cstdio>
#include <cstdlib>

namespace {

int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

struct TestSpace {
    static int live, allocs, frees, syncs, switches;
    static int fail_at;          // the allocation (counted from 1) that throws; 0 = none
    static void *alloc(size_t bytes, const char *what) {
        if (++allocs == fail_at) throw std::runtime_error(std::string(what) + ": out of memory (injected)");
        live++;
        return std::malloc(bytes);
    }
    static void free(void *p) { live--; frees++; std::free(p); }
    static void sync(hipStream_t) { syncs++; }
    static int set_device(int dev) { switches++; return dev; }
    static void fail_next() { fail_at = allocs + 1; }
};
int TestSpace::live = 0, TestSpace::allocs = 0, TestSpace::frees = 0, TestSpace::syncs = 0, TestSpace::switches = 0, TestSpace::fail_at = 0;

using Buf = gdpt::Buffer<double, TestSpace>;

template <class F>
bool throws(F &&f) {
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}
bool empty(const Buf &b) { return b.data() == nullptr && b.size() == 0; }

const hipStream_t kStream = nullptr;

// (a) a failed alloc / grow leaves the buffer empty and gives back what it held; (b) the next grow, of a smaller size too, allocates
void failed_allocations() {
    {   // from empty
        Buf b;
        CHECK(empty(b));
        TestSpace::fail_next();
        CHECK(throws([&] { b.alloc(100, "alloc") ; }));
        CHECK(empty(b) && TestSpace::live == 0);
        TestSpace::fail_next();
        CHECK(throws([&] { b.grow(100, "grow"); }));
        CHECK(empty(b) && TestSpace::live == 0);
        TestSpace::fail_next();
        CHECK(throws([&] { b.grow(100, kStream, "grow"); }));
        CHECK(empty(b) && TestSpace::live == 0);
        const int before = TestSpace::allocs;
        b.grow(10, "grow");                                  // smaller than what failed: allocated, not skipped
        CHECK(TestSpace::allocs == before + 1 && b.data() && b.size() == 10 && TestSpace::live == 1);
        b.data()[9] = 1.0;
    }
    CHECK(TestSpace::live == 0);
    for (int with_stream = 0; with_stream < 2; with_stream++) {   // from populated
        Buf b;
        b.alloc(64, "alloc");
        CHECK(b.size() == 64 && TestSpace::live == 1);
        const int syncs = TestSpace::syncs, frees = TestSpace::frees;
        TestSpace::fail_next();
        CHECK(throws([&] { if (with_stream) b.grow(128, kStream, "grow"); else b.grow(128, "grow"); }));
        CHECK(empty(b));
        CHECK(TestSpace::live == 0 && TestSpace::frees == frees + 1);      // the old block went, nothing came
        CHECK(TestSpace::syncs == syncs + with_stream);                    // the stream was waited for before the free
        int before = TestSpace::allocs;
        if (with_stream) b.grow(32, kStream, "grow"); else b.grow(32, "grow");   // smaller than the size held before the failure
        CHECK(TestSpace::allocs == before + 1 && b.data() && b.size() == 32 && TestSpace::live == 1);
        CHECK(TestSpace::syncs == syncs + with_stream);                    // nothing held: nothing to wait for
        b.data()[31] = 2.0;
        before = TestSpace::allocs;
        b.grow(32, kStream, "grow"); b.grow(7, "grow");                    // enough held: no allocation, no wait
        CHECK(TestSpace::allocs == before && b.size() == 32 && TestSpace::syncs == syncs + with_stream);
        TestSpace::fail_next();
        CHECK(throws([&] { b.alloc(8, "alloc"); }));                       // alloc on a populated buffer
        CHECK(empty(b) && TestSpace::live == 0);
        b.alloc(0, "alloc");
        CHECK(empty(b) && TestSpace::live == 0);
    }
    TestSpace::fail_at = 0;
    CHECK(TestSpace::live == 0 && TestSpace::allocs - 7 == TestSpace::frees);   // (7 allocations were refused)
}

// (c) moves leave the source empty and free nothing twice (ASan would report the second free)
void moves() {
    const int frees = TestSpace::frees;
    {
        Buf a;
        a.alloc(16, "alloc");
        double *p = a.data();
        Buf b(std::move(a));
        CHECK(empty(a) && b.data() == p && b.size() == 16 && TestSpace::live == 1);
        Buf c;
        c.alloc(4, "alloc");
        CHECK(TestSpace::live == 2);
        c = std::move(b);                                    // c's own block goes, b's moves in
        CHECK(empty(b) && c.data() == p && c.size() == 16 && TestSpace::live == 1 && TestSpace::frees == frees + 1);
        Buf &self = c;
        c = std::move(self);
        CHECK(c.data() == p && c.size() == 16 && TestSpace::live == 1);
        a.reset(); b.reset();                                // empty: nothing to free
        CHECK(TestSpace::frees == frees + 1);
        Buf arr[3];
        arr[1].alloc(2, "alloc");
        Buf moved[3] = {std::move(arr[0]), std::move(arr[1]), std::move(arr[2])};
        CHECK(empty(arr[1]) && moved[1].size() == 2 && empty(moved[0]) && TestSpace::live == 2);
    }
    CHECK(TestSpace::live == 0 && TestSpace::frees == frees + 3);
}

// (d) the registry: forget of an absent key is a no-op, get after forget makes a fresh T
struct Plain {
    static int made, gone;
    int value = 0;
    Buf scratch;
    Plain() { made++; }
    ~Plain() { gone++; }
};
int Plain::made = 0, Plain::gone = 0;

void registry() {
    gdpt::PerStream<Plain, TestSpace> reg;
    const hipStream_t s1 = reinterpret_cast<hipStream_t>(0x10), s2 = reinterpret_cast<hipStream_t>(0x20);
    reg.forget(0, s1);
    CHECK(Plain::made == 0 && Plain::gone == 0 && TestSpace::switches == 0);
    Plain &a = reg.get(0, s1);
    a.value = 7; a.scratch.alloc(5, "alloc");
    CHECK(&reg.get(0, s1) == &a && Plain::made == 1);
    CHECK(&reg.get(1, s1) != &a && &reg.get(0, s2) != &a && Plain::made == 3);      // the device and the stream both key
    reg.forget(0, nullptr); reg.forget(2, s1);
    CHECK(Plain::gone == 0 && reg.get(0, s1).value == 7);
    reg.forget(0, s1);
    CHECK(Plain::gone == 1 && TestSpace::live == 0 && TestSpace::switches == 2);    // destroyed with its device current, then back
    reg.forget(0, s1);
    CHECK(Plain::gone == 1);
    Plain &fresh = reg.get(0, s1);
    CHECK(Plain::made == 4 && fresh.value == 0 && fresh.scratch.size() == 0);
    fresh.scratch.alloc(3, "alloc");
    reg.clear();
    CHECK(Plain::gone == 4 && TestSpace::live == 0);
    CHECK(reg.get(0, s1).value == 0 && Plain::made == 5);
}

// (e) forget_stream reaches every registry alive, whatever it keeps: the pair goes from both, other pairs and devices stay
struct Other {
    static int made, gone;
    Buf a, b;
    Other() { made++; }
    ~Other() { gone++; }
};
int Other::made = 0, Other::gone = 0;

void forget_stream_reaches_every_registry() {
    const hipStream_t s1 = reinterpret_cast<hipStream_t>(0x10), s2 = reinterpret_cast<hipStream_t>(0x20);
    const int plain_made = Plain::made, plain_gone = Plain::gone;
    gdpt::forget_stream(0, s1);                              // the registry of registry() has left the list: nothing to visit
    CHECK(Plain::gone == plain_gone && Other::gone == 0);
    {
        gdpt::PerStream<Plain, TestSpace> plains;
        gdpt::PerStream<Other, TestSpace> others;
        for (int dev = 0; dev < 2; dev++)
            for (hipStream_t s : {s1, s2}) {
                plains.get(dev, s).value = 10 * dev + (s == s1 ? 1 : 2);
                plains.get(dev, s).scratch.alloc(4, "alloc");
                others.get(dev, s).a.alloc(2, "alloc");
            }
        CHECK(Plain::made == plain_made + 4 && Other::made == 4 && TestSpace::live == 8);
        const int switches = TestSpace::switches;
        gdpt::forget_stream(0, s1);
        CHECK(Plain::gone == plain_gone + 1 && Other::gone == 1 && TestSpace::live == 6);
        CHECK(TestSpace::switches == switches + 4);          // each entry destroyed with its device current, then back
        CHECK(plains.get(0, s2).value == 2 && plains.get(1, s1).value == 11 && plains.get(1, s2).value == 12);   // the others: untouched
        CHECK(others.get(0, s2).a.size() == 2 && others.get(1, s1).a.size() == 2 && others.get(1, s2).a.size() == 2);
        CHECK(Plain::made == plain_made + 4 && Other::made == 4);
        gdpt::forget_stream(0, s1);                          // again: a no-op
        gdpt::forget_stream(2, s1); gdpt::forget_stream(0, nullptr);      // pairs nobody keeps
        CHECK(Plain::gone == plain_gone + 1 && Other::gone == 1 && TestSpace::live == 6 && TestSpace::switches == switches + 4);
        CHECK(plains.get(0, s1).value == 0 && others.get(0, s1).a.size() == 0);      // a later stream of the same value starts fresh
        CHECK(Plain::made == plain_made + 5 && Other::made == 5);
    }
    CHECK(Plain::gone == plain_gone + 5 && Other::gone == 5 && TestSpace::live == 0);
    gdpt::forget_stream(1, s2);                              // both registries have left the list
    CHECK(Plain::gone == plain_gone + 5 && Other::gone == 5);
}

} // namespace

int main() {
    failed_allocations();
    moves();
    registry();
    forget_stream_reaches_every_registry();
    CHECK(TestSpace::live == 0);       // (the registry of registry() has gone with its entry)
    if (g_failures) { std::printf("%d check(s) failed\n", g_failures); return 1; }
    std::printf("device_mem_check ok\n");
    return 0;
}
