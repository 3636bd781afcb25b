// m3d_mask_pool.hpp -- the writers of a mask expansion (m3d_mask_expand.hpp): one pool per process, created on first use, never
// torn down.  Header-only and free of HIP: the library (m3d_refine.cpp) and the microbenchmark (tools/ubench/expand_mask.cpp) run
// the same pool.
//
// Helpers = min(writer cap, CPUs of the process' affinity mask) - 1; the caller's thread is always a writer as well.
// arm() -- when a fit queues a mask compaction -- wakes the parked helpers: they spin on the job word for at most spin_us (so
// their wake-up hides under the device work still ahead), then park again.  expand() publishes the job as spans of the list of
// equal length, each beginning on a 64-byte line of the destination, claimed through ONE word: (spans << 32 | next span).  A claim
// is only made on the current job (the word carries its span count), the caller works on spans too and returns once every
// claimed span is written.  A second caller while the pool is busy (another lane) expands alone: the result never depends on the
// helpers.
//
// Placement: arm() binds each helper to one CPU of the process' own affinity mask that shares a last-level cache with the CPU
// the caller runs on (sysfs: cache/index3/shared_cpu_list, topology/thread_siblings_list; read only), a core of its own first,
// so that a list's lines move inside one cache and not between two -- or between two sockets (profiles/r10_expand_ladder.txt).
// Thread affinity of the pool's own threads only.  Helpers for which that cache has no free CPU inside the mask, and all helpers
// where the topology is not told, run anywhere in the mask, as before.  The sysfs files are read under the pool's mutex, inside
// arm(), the first time a caller is seen on a cache (about twenty small files, once); later calls compare two integers.
#pragma once

#include "m3d_mask_expand.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <mutex>
#include <sched.h>
#include <thread>
#include <vector>

namespace m3d {

namespace mask_detail {
// "0-7,128-135" -> the CPUs; empty where the file is missing or malformed
inline std::vector<int> read_cpu_list(const char* path) {
    std::vector<int> out;
    FILE* f = std::fopen(path, "r");
    if (!f) return out;
    char buf[4096];
    const size_t got = std::fread(buf, 1, sizeof(buf) - 1, f);
    std::fclose(f);
    buf[got] = 0;
    const char* p = buf;
    while (*p >= '0' && *p <= '9') {
        char* e;
        const long a = std::strtol(p, &e, 10);
        long b = a;
        if (*e == '-') b = std::strtol(e + 1, &e, 10);
        if (a < 0 || b < a || b - a > 4096) return std::vector<int>();
        for (long c = a; c <= b; ++c) out.push_back((int)c);
        p = *e == ',' ? e + 1 : e;
    }
    return out;
}
}  // namespace mask_detail

class MaskPool {
public:
    std::string sysfs_cpu = "/sys/devices/system/cpu";   // (the tests point it elsewhere: a host that tells no topology)

    static MaskPool& get() {
        static MaskPool* p = new MaskPool();   // (leaked on purpose: helpers may still be parked at exit)
        return *p;
    }
    // list_mask: m3d_config.list_mask (>= 2: that many writers; 1: the default of 8), never more than the affinity mask holds
    static uint32_t writer_cap(int list_mask) {
        uint32_t cap = list_mask >= 2 ? (uint32_t)list_mask : 8u;
        cpu_set_t set;
        CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof(set), &set) == 0) cap = std::min<uint32_t>(cap, (uint32_t)std::max(CPU_COUNT(&set), 1));
        return std::max<uint32_t>(cap, 1u);
    }
    void arm(uint32_t writers, int spin_us) {
        const uint32_t helpers = writers ? writers - 1 : 0;
        spin_us_.store(std::max(spin_us, 0), std::memory_order_relaxed);
        if (helpers == 0) return;
        std::lock_guard<std::mutex> lk(mu_);
        place(helpers);
        try {
            while (threads_ < helpers) {
                std::thread(&MaskPool::helper, this, threads_).detach();
                ++threads_;
            }
        } catch (...) {   // (no thread to be had: fewer helpers -- the caller writes what they do not)
        }
        want_ = std::min(helpers, threads_);
        arm_seq_.fetch_add(1, std::memory_order_release);
        if (parked_) cv_.notify_all();
    }
    // false: the mask disagrees with its counts (dst[0, total) may then hold anything, nothing beyond it was written)
    bool expand(const uint64_t* mask, uint64_t n, const uint32_t* counts, uint64_t* dst, uint32_t writers) {
        const uint32_t nb = (uint32_t)((n + 64ull * kMaskTileWords - 1) / (64ull * kMaskTileWords));
        if (nb == 0) return true;
        bool expected = false;
        if (!busy_.compare_exchange_strong(expected, true, std::memory_order_acquire)) {
            std::vector<uint64_t> prefix(nb + 1);
            const uint64_t total = mask_tile_prefix(counts, nb, prefix.data());
            return mask_expand_span(mask, n, prefix.data(), nb, 0, total, dst);
        }
        prefix_.resize(nb + 1);
        const uint64_t total = mask_tile_prefix(counts, nb, prefix_.data());
        const uint32_t spans = std::min<uint32_t>(nb, 4u * std::max<uint32_t>(writers, 1u));
        cuts_.resize(spans + 1);
        mask_split_lines(total, spans, dst, cuts_.data());
        mask_ = mask;
        n_ = n;
        nb_ = nb;
        dst_ = dst;
        failed_.store(false, std::memory_order_relaxed);
        done_.store(0, std::memory_order_relaxed);
        job_.store((uint64_t)spans << 32, std::memory_order_release);   // (publishes the fields above)
        work();
        while (done_.load(std::memory_order_acquire) != spans) {
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
        }
        const bool ok = !failed_.load(std::memory_order_relaxed);
        busy_.store(false, std::memory_order_release);
        return ok;
    }

private:
    // claim and write spans of the current job until none is left; true if any was claimed
    bool work() {
        bool any = false;
        for (;;) {
            const uint64_t v = job_.load(std::memory_order_relaxed);
            if ((v & 0xFFFFFFFFull) >= (v >> 32)) return any;
            const uint64_t c = job_.fetch_add(1, std::memory_order_acq_rel);
            const uint32_t k = (uint32_t)c, spans = (uint32_t)(c >> 32);
            if (k >= spans) return any;
            if (!mask_expand_span(mask_, n_, prefix_.data(), nb_, cuts_[k], cuts_[k + 1], dst_))
                failed_.store(true, std::memory_order_relaxed);
            done_.fetch_add(1, std::memory_order_release);
            any = true;
        }
    }
    // (mu_) the helpers' CPUs for a caller on the CPU it runs on now; a new placement only when the caller changed caches
    void place(uint32_t helpers) {
        const int cpu = sched_getcpu();
        if (cpu < 0) return;
        if ((size_t)cpu < llc_of_.size() && llc_of_[cpu] == placed_llc_ && placed_for_ >= helpers &&
            std::find(given_.begin(), given_.end(), cpu) == given_.end())
            return;
        if ((size_t)cpu >= llc_of_.size()) llc_of_.resize((size_t)cpu + 1, -2);
        if (llc_of_[cpu] == -2) {   // first time on this CPU: which CPUs share its last-level cache
            char path[512];
            std::snprintf(path, sizeof(path), "%s/cpu%d/cache/index3/shared_cpu_list", sysfs_cpu.c_str(), cpu);
            std::vector<int> group = mask_detail::read_cpu_list(path);
            const int id = group.empty() ? -1 : group[0];
            for (int c : group) {
                if ((size_t)c >= llc_of_.size()) llc_of_.resize((size_t)c + 1, -2);
                llc_of_[c] = id;
            }
            llc_of_[cpu] = id;
            if (id >= 0 && !groups_.count(id)) {
                cpu_set_t mine;
                CPU_ZERO(&mine);
                if (sched_getaffinity(0, sizeof(mine), &mine) != 0) group.clear();
                // one CPU of every core first, the cores' other threads after them
                std::vector<std::pair<int, int>> keyed;   // (rank among its core's threads, cpu)
                for (int c : group) {
                    if (c >= CPU_SETSIZE || !CPU_ISSET(c, &mine)) continue;
                    std::snprintf(path, sizeof(path), "%s/cpu%d/topology/thread_siblings_list", sysfs_cpu.c_str(), c);
                    const std::vector<int> sib = mask_detail::read_cpu_list(path);
                    const int rank = (int)(std::find(sib.begin(), sib.end(), c) - sib.begin());
                    keyed.emplace_back(sib.empty() ? 0 : rank, c);
                }
                std::sort(keyed.begin(), keyed.end());
                std::vector<int>& g = groups_[id];
                for (const auto& kc : keyed) g.push_back(kc.second);
            }
        }
        const int id = llc_of_[cpu];
        placed_llc_ = id;
        placed_for_ = helpers;
        if (id < 0) return;   // (not told: the helpers stay where they are)
        const std::vector<int>& g = groups_[id];
        // the caller's own CPU and its core's other thread get no helper
        std::vector<int> order;
        char path[512];
        std::snprintf(path, sizeof(path), "%s/cpu%d/topology/thread_siblings_list", sysfs_cpu.c_str(), cpu);
        const std::vector<int> own = mask_detail::read_cpu_list(path);
        for (int c : g)
            if (c != cpu && std::find(own.begin(), own.end(), c) == own.end()) order.push_back(c);
        if (bind_.size() < helpers) bind_.resize(helpers);
        given_.clear();
        cpu_set_t anywhere;   // the caller's own mask: for the helpers this cache has no free CPU for
        CPU_ZERO(&anywhere);
        if (sched_getaffinity(0, sizeof(anywhere), &anywhere) != 0) return;
        for (uint32_t h = 0; h < helpers; ++h) {
            cpu_set_t& s = bind_[h];
            CPU_ZERO(&s);
            if (h >= order.size()) {
                s = anywhere;
            } else {
                CPU_SET(order[h], &s);
                given_.push_back(order[h]);
            }
        }
        bind_seq_.fetch_add(1, std::memory_order_release);
    }
    void helper(uint32_t id) {
        uint64_t seen = 0, bound = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                ++parked_;
                cv_.wait(lk, [&] { return arm_seq_.load(std::memory_order_relaxed) != seen && id < want_; });
                --parked_;
                seen = arm_seq_.load(std::memory_order_relaxed);
                rebind(id, &bound);
            }
            auto t0 = std::chrono::steady_clock::now();
            for (uint32_t spins = 1;; ++spins) {
                if (work()) t0 = std::chrono::steady_clock::now();
                const uint64_t a = arm_seq_.load(std::memory_order_relaxed);
                if (a != seen) {   // armed again while awake: the spin starts over
                    seen = a;
                    t0 = std::chrono::steady_clock::now();
                    if (bind_seq_.load(std::memory_order_acquire) != bound) {
                        std::lock_guard<std::mutex> lk(mu_);
                        rebind(id, &bound);
                    }
                }
                if ((spins & 0xFFu) == 0 &&
                    std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() >=
                        spin_us_.load(std::memory_order_relaxed))
                    break;
#if defined(__x86_64__) || defined(__i386__)
                __builtin_ia32_pause();
#endif
            }
        }
    }
    // (mu_) this helper onto the CPUs the latest placement gives it
    void rebind(uint32_t id, uint64_t* bound) {
        const uint64_t b = bind_seq_.load(std::memory_order_acquire);
        if (b == *bound) return;
        *bound = b;
        if (id < bind_.size() && CPU_COUNT(&bind_[id]) > 0) (void)sched_setaffinity(0, sizeof(cpu_set_t), &bind_[id]);
    }
    std::mutex mu_;
    std::condition_variable cv_;
    uint32_t threads_ = 0, want_ = 0, parked_ = 0;   // (mu_)
    // placement (mu_)
    std::vector<int> llc_of_;                 // per CPU: the first CPU of its last-level cache's list; -1 not told; -2 not read yet
    std::map<int, std::vector<int>> groups_;  // per cache: its CPUs inside the affinity mask, one per core first
    std::vector<cpu_set_t> bind_;             // per helper
    std::vector<int> given_;                  // the CPUs that have one helper each: the caller landing on one asks for a new placement
    int placed_llc_ = -3;
    uint32_t placed_for_ = 0;
    std::atomic<uint64_t> bind_seq_{0};
    std::atomic<uint64_t> arm_seq_{0};
    std::atomic<int> spin_us_{0};
    std::atomic<bool> busy_{false};
    // the job (written by the pool's owner while no span of it can be claimed)
    std::atomic<uint64_t> job_{0};   // spans << 32 | next span
    std::atomic<uint32_t> done_{0};
    std::atomic<bool> failed_{false};
    const uint64_t* mask_ = nullptr;
    uint64_t n_ = 0;
    uint32_t nb_ = 0;
    uint64_t* dst_ = nullptr;
    std::vector<uint64_t> prefix_;
    std::vector<uint64_t> cuts_;
};

}  // namespace m3d
