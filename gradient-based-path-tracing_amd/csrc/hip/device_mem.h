// device_mem.h — who owns device memory on the host side: a move-only Buffer for device and pinned memory, an Event, and the
// registries of what the solvers keep per (device, stream), which enrol themselves so that forget_stream reaches all of them. Every
// handle (GdptScene, GdptProgressive, the solvers' workspaces, the ranks of GdptMulti) holds these as members, so a handle's
// destructor names no field, and a buffer's size cannot disagree with its pointer: after a failed allocation the buffer is empty
// and the next call allocates again.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace gdpt {

inline void ck(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// what an entry point that launches kernels refuses on a machine without a device; `who` names the caller
inline void need_a_device(const std::string &who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); ndev = 0; }      // (without a device the count itself is an error)
    if (ndev <= 0) throw std::runtime_error(who + ": no HIP device visible (this library has no CPU fallback)");
}

struct DeviceSpace {
    static void *alloc(size_t bytes, const char *what) { void *p = nullptr; ck(hipMalloc(&p, bytes), what); return p; }
    static void free(void *p) { (void)hipFree(p); }
    static void sync(hipStream_t stream) { ck(hipStreamSynchronize(stream), "hipStreamSynchronize"); }
    static int set_device(int dev) { int cur = 0; (void)hipGetDevice(&cur); (void)hipSetDevice(dev); return cur; }   // returns the device that was current
};
struct PinnedSpace {
    static void *alloc(size_t bytes, const char *what) { void *p = nullptr; ck(hipHostMalloc(&p, bytes), what); return p; }
    static void free(void *p) { (void)hipHostFree(p); }
};

// `size()` elements of T in Space. data() == nullptr exactly when size() == 0, after every member function, one that throws included.
// `what` is the text an allocation failure is reported with. Frees on the device that is current: a handle's destructor sets it first.
template <class T, class Space>
class Buffer {
    T *p_ = nullptr;
    size_t n_ = 0;
public:
    Buffer() = default;
    Buffer(Buffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    ~Buffer() { reset(); }

    T *data() const { return p_; }
    size_t size() const { return n_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }

    void reset() {
        if (p_) Space::free(p_);
        p_ = nullptr; n_ = 0;
    }
    // for an empty buffer (one that holds something is freed first)
    void alloc(size_t n, const char *what) {
        reset();
        if (n == 0) return;
        p_ = static_cast<T *>(Space::alloc(n * sizeof(T), what));
        n_ = n;
    }
    // at least n elements; the contents do not survive a growth
    void grow(size_t n, const char *what) { if (n > n_) alloc(n, what); }
    // ... where work enqueued on `stream` may still use the buffer held: waits for the stream before freeing it
    void grow(size_t n, hipStream_t stream, const char *what) {
        if (n <= n_) return;
        if (p_) Space::sync(stream);
        alloc(n, what);
    }
};
template <class T> using DeviceBuffer = Buffer<T, DeviceSpace>;
template <class T> using PinnedBuffer = Buffer<T, PinnedSpace>;

class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event &operator=(Event &&o) noexcept {
        if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
        return *this;
    }
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { reset(); }
    operator hipEvent_t() const { return e_; }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    void create(unsigned flags = 0) { reset(); ck(hipEventCreateWithFlags(&e_, flags), "hipEventCreate"); }
};

// A stream a handle owns for work of its own beside the caller's stream. Non-blocking: it takes no implicit order from the null
// stream, every dependency is an event. Destroyed after a join, on the device that is current.
class Stream {
    hipStream_t s_ = nullptr;
public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { reset(); }
    operator hipStream_t() const { return s_; }
    void reset() { if (s_) { (void)hipStreamSynchronize(s_); (void)hipStreamDestroy(s_); } s_ = nullptr; }
    void create() { reset(); ck(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking), "hipStreamCreate"); }
};

// Every registry of per-(device, stream) state in the process, so that a stream's owner can drop all of it in one call without
// knowing who keeps any: a registry enrols itself when it is made and leaves when it goes. The list and its mutex are leaked like the
// registries of the solvers themselves, so no static destructor touches them.
inline void forget_stream(int dev, hipStream_t stream);
class PerStreamBase {
public:
    // Drops what the registry keeps for the pair, if anything. The caller guarantees that nothing of the pair is in flight.
    virtual void forget(int dev, hipStream_t stream) = 0;
    PerStreamBase(const PerStreamBase &) = delete;
    PerStreamBase &operator=(const PerStreamBase &) = delete;
protected:
    PerStreamBase() { std::lock_guard<std::mutex> lk(all().mu); all().list.push_back(this); }
    ~PerStreamBase() { std::lock_guard<std::mutex> lk(all().mu); auto &l = all().list; l.erase(std::find(l.begin(), l.end(), this)); }
private:
    struct All { std::mutex mu; std::vector<PerStreamBase *> list; };
    static All &all() { static All &a = *new All(); return a; }
    friend void forget_stream(int dev, hipStream_t stream);
};

// Drops everything any registry keeps for the pair. A stream's owner calls it before it destroys the stream: the key is the handle's
// value, and a later stream with the same value must not inherit another one's state.
inline void forget_stream(int dev, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(PerStreamBase::all().mu);
    for (PerStreamBase *r : PerStreamBase::all().list) r->forget(dev, stream);
}

// What a solver keeps per (device, stream): one T per pair, made on first use, dropped by forget_stream (above).
// An entry is destroyed with its device current. (Space: only the device switch is taken from it.)
template <class T, class Space = DeviceSpace>
class PerStream : public PerStreamBase {
    std::mutex mu_;
    std::map<std::pair<int, hipStream_t>, std::unique_ptr<T>> map_;
public:
    T &get(int dev, hipStream_t stream) {
        std::lock_guard<std::mutex> lk(mu_);
        auto &slot = map_[{dev, stream}];
        if (!slot) slot.reset(new T());
        return *slot;
    }
    void forget(int dev, hipStream_t stream) override {
        std::unique_ptr<T> gone;
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = map_.find({dev, stream});
            if (it == map_.end()) return;
            gone = std::move(it->second);
            map_.erase(it);
        }
        const int cur = Space::set_device(dev);
        gone.reset();
        Space::set_device(cur);
    }
    void clear() {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto &kv : map_) {
            const int cur = Space::set_device(kv.first.first);
            kv.second.reset();
            Space::set_device(cur);
        }
        map_.clear();
    }
};

} // namespace gdpt
