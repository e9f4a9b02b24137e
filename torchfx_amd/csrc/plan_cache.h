// plan_cache.h -- the one cache behind every per-filter table of libtorchfx_hip.so (SOS plans, tap vectors, spectra, warm-up
// lengths, overlap-save plans) and the device buffer those tables live in.  Host code only.
#pragma once
#include "common.h"

#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace tfx {

// One device allocation, filled from host memory with a blocking copy (host == nullptr: left unfilled), freed by the
// destructor.  hipFree waits for the device, so a buffer freed after a launch was enqueued outlives that launch.
struct DeviceBuffer {
    void *p = nullptr;
    DeviceBuffer(const void *host, size_t bytes) : DeviceBuffer()     // delegating: the destructor runs if the copy throws
    {
        if (!bytes) return;
        TFX_HIP(hipMalloc(&p, bytes));
        if (host) TFX_HIP(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    }
    template <typename T> explicit DeviceBuffer(const std::vector<T> &h) : DeviceBuffer(h.data(), h.size() * sizeof(T)) {}
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;

private:
    DeviceBuffer() = default;
};

// Values built once per filter, keyed by the exact bytes of the filter's host coefficients plus a tail of NT integers and
// the ordinal of the current device (a table lives on one device).  Byte keys: a NaN coefficient is a filter of its own, and
// -0.0 and +0.0 are two filters.
//  * get() hands out shared ownership: an entry evicted (or cleared) while a caller still holds it lives on until that caller
//    lets go, i.e. until its launches are enqueued.
//  * At most `cap` entries; the least recently used one goes first.
//  * Steady state (the same filter call after call, e.g. streaming chunks): the entry used last on this device is recognised
//    with no key construction and no allocation.
//  * A cache constructed with a name refuses a miss while `stream` is capturing: building a value allocates and copies with
//    blocking calls, which a capture cannot hold.
// One mutex guards the cache; build() runs under it.
template <typename V, size_t NT> class PlanCache {
public:
    explicit PlanCache(size_t cap, const char *refuse_capture = nullptr) : cap_(cap), refuse_capture_(refuse_capture) {}

    template <typename Build>
    std::shared_ptr<V> get(const void *bytes, size_t nb, const int64_t (&tail_in)[NT], hipStream_t stream, Build &&build)
    {
        int64_t tail[NT + 1];
        for (size_t i = 0; i < NT; ++i) tail[i] = tail_in[i];
        const int dev = current_device();
        tail[NT] = dev;
        std::lock_guard<std::mutex> lk(mu_);
        if (Node *n = last_[dev]) {
            const std::vector<char> &k = n->first;
            if (k.size() == nb + sizeof(tail) && memcmp(k.data(), bytes, nb) == 0 && memcmp(k.data() + nb, tail, sizeof(tail)) == 0) {
                n->second.used = ++tick_;
                return n->second.value;
            }
        }
        std::vector<char> key((const char *)bytes, (const char *)bytes + nb);
        key.insert(key.end(), (const char *)tail, (const char *)tail + sizeof(tail));
        auto it = map_.find(key);
        if (it == map_.end()) {
            if (refuse_capture_) {
                hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
                TFX_CHECK(!(hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone),
                          "%s: first use of this filter inside a stream capture -- run it once before capturing "
                          "(its tables are uploaded with blocking copies)", refuse_capture_);
            }
            std::shared_ptr<V> v = build();
            while (!map_.empty() && map_.size() >= cap_) evict_lru();
            it = map_.emplace(std::move(key), Entry{std::move(v), 0}).first;
        }
        it->second.used = ++tick_;
        last_[dev] = &*it;                              // std::map nodes are stable
        return it->second.value;
    }

    void clear()
    {
        std::lock_guard<std::mutex> lk(mu_);
        map_.clear();
        for (Node *&n : last_) n = nullptr;
    }

private:
    struct Entry {
        std::shared_ptr<V> value;
        uint64_t used;                                  // tick of the last use
    };
    typedef std::pair<const std::vector<char>, Entry> Node;

    void evict_lru()
    {
        auto victim = map_.begin();
        for (auto u = map_.begin(); u != map_.end(); ++u)
            if (u->second.used < victim->second.used) victim = u;
        for (Node *&n : last_)
            if (n == &*victim) n = nullptr;
        map_.erase(victim);
    }

    const size_t cap_;
    const char *const refuse_capture_;
    std::mutex mu_;
    std::map<std::vector<char>, Entry> map_;
    uint64_t tick_ = 0;
    Node *last_[TFX_MAX_DEVICES] = {};
};

// fir.hip: device copy of a host tap vector zero padded to `padded` bytes, cached by content, padded size and device
std::shared_ptr<DeviceBuffer> cached_taps(const void *host, size_t bytes, size_t padded);

}  // namespace tfx
