// copy_pool.h -- the host-side copy workers of the staging ring (staging.hip).  Plain C++, no device runtime: tests/host_layer_check.cc
// runs it under the thread and address sanitizers.
#pragma once

#include <stdint.h>
#include <string.h>
#include <sys/mman.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif

// Host-side copy workers for the host-buffer entry points: a chunk is cut into page-aligned parts and every worker (and the
// caller) memcpy's one.  One thread moves ~10 GB/s into or out of pinned staging -- and pays every first-touch page fault
// of a fresh output buffer alone -- which is below what the PCIe link carries.
struct CopyPool {
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    uint64_t generation = 0;
    int pending = 0;
    bool stop = false;
    char *dst = nullptr;
    const char *src = nullptr;
    size_t len = 0;
    int parts = 1;
    bool touching = false;  // the current job pre-faults the pages of dst (madvise, contents untouched) instead of copying
    std::atomic<bool> touch_failed{false};

    void part(int i)
    {
        if (touching) {                   // workers 1 .. parts-1 share the buffer; the caller takes no part
            // MADV_POPULATE_WRITE maps the pages writable WITHOUT changing what they hold (a store of zeros, the first form, clobbered
            // the caller's buffer although the call could still fail, and -- in a batch -- an input that the output aliases).  Where the
            // kernel refuses it (before Linux 5.14, or a mapping it cannot populate) nothing is pre-faulted: the copy out pays the faults.
            const int nw = parts - 1;
            const uintptr_t b = ((uintptr_t)dst + 4095) & ~(uintptr_t)4095, e = ((uintptr_t)dst + len) & ~(uintptr_t)4095;
            if (e <= b) return;
            const size_t pages = (e - b) >> 12, per = (pages + (size_t)nw - 1) / (size_t)nw;
            const size_t lo = per * (size_t)(i - 1) < pages ? per * (size_t)(i - 1) : pages;
            const size_t hi = lo + per < pages ? lo + per : pages;
            // (in pieces of 32 MiB: a worker that is told to stop gives up soon)
            for (size_t o = lo; o < hi && !touch_failed.load(std::memory_order_relaxed); o += 8192) {
                const size_t cnt = hi - o < 8192 ? hi - o : 8192;
                if (madvise((void *)(b + (o << 12)), cnt << 12, MADV_POPULATE_WRITE) != 0) touch_failed.store(true, std::memory_order_relaxed);
            }
            return;
        }
        // page-aligned cuts: two workers never fault on the same page of a fresh destination
        const size_t per = ((len / (size_t)parts) + 4095) & ~(size_t)4095;
        const size_t lo = per * (size_t)i < len ? per * (size_t)i : len;
        const size_t hi = i + 1 == parts ? len : (lo + per < len ? lo + per : len);
        if (hi > lo) memcpy(dst + lo, src + lo, hi - lo);
    }

    void start(int threads)
    {
        parts = threads < 1 ? 1 : threads;
        for (int t = 1; t < parts; t++) {
            workers.emplace_back([this, t] {
                uint64_t seen = 0;
                for (;;) {
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv_work.wait(lk, [&] { return stop || generation != seen; });
                        if (stop) return;
                        seen = generation;
                    }
                    part(t);
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        if (--pending == 0) cv_done.notify_one();
                    }
                }
            });
        }
    }

    void copy(void *d, const void *s_, size_t n)         // returns when all parts are done
    {
        if (parts == 1 || n < ((size_t)1 << 20)) { memcpy(d, s_, n); return; }
        {
            std::lock_guard<std::mutex> lk(mu);
            dst = (char *)d; src = (const char *)s_; len = n;
            pending = parts - 1;
            generation++;
        }
        cv_work.notify_all();
        part(0);
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
    }

    // The workers alone fault in the pages of a fresh buffer (MADV_POPULATE_WRITE: mapped writable, contents as they were) while
    // the caller goes on: the first-touch faults of a caller's output buffer are paid while the GPU transforms.  wait() before the
    // next job.
    void touch_async(void *d, size_t n)
    {
        if (parts == 1 || n < ((size_t)4 << 20)) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            dst = (char *)d; src = nullptr; len = n;
            touching = true;
            touch_failed.store(false, std::memory_order_relaxed);
            pending = parts - 1;
            generation++;
        }
        cv_work.notify_all();
    }

    void wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
        touching = false;
    }

    void shutdown()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_work.notify_all();
        for (std::thread &t : workers) t.join();
        workers.clear();
    }
};
