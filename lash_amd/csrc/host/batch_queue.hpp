// batch_queue.hpp — the hand-off between the planner, the GPU workers and the in-order writer of `lash sketch` (sketch_files.cpp).
// A batch is planned (take_slot, push), sketched by a worker (next, add_part, finish) or on the planner's own thread (publish), and
// written in index order (writer_next, writer_next_part, writer_done).  Standard library only: tests/host_queue_check.cpp drives it
// with fake buffers under ThreadSanitizer.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace lashhost {

// page-locked host memory (H2D at PCIe speed); recycled between batches.  The allocator is the caller's (the library's pinned one).
struct PinnedBuf {
    typedef void *(*AllocFn)(size_t);
    typedef void (*FreeFn)(void *);
    uint8_t *p = nullptr;
    size_t cap = 0;
    PinnedBuf(AllocFn a, FreeFn f) : alloc_(a), free_(f) {}
    bool reserve(size_t n)
    {
        if (n <= cap) return true;
        free_(p);
        cap = n + n / 8 + (1u << 20);
        p = static_cast<uint8_t *>(alloc_(cap));
        if (!p) cap = 0;
        return p != nullptr;
    }
    ~PinnedBuf() { free_(p); }
private:
    AllocFn alloc_;
    FreeFn free_;
};

struct Batch {
    uint64_t index = 0;
    size_t f0 = 0, f1 = 0;                // files [f0, f1)
    std::unique_ptr<PinnedBuf> buf;
    std::vector<uint64_t> file_off{0};
    std::vector<uint8_t> fmt;
    std::atomic<size_t> remaining{0};
    std::vector<uint8_t> images;
    std::string err;
    std::mutex emu;
    // --per-record: the images leave in parts (one per sub-call) that the writer takes while the batch is still being sketched, so
    // that a batch of many small records never holds all its images at once (parts / parts_bytes: guarded by the queue mutex)
    std::deque<std::vector<uint8_t>> parts;
    size_t parts_bytes = 0;
    std::vector<std::string> names;       // record ids, in order
};

class BatchQueue {
public:
    typedef std::shared_ptr<Batch> Ptr;
    // ---- planner ----
    // Waits until fewer than `cap` batches are planned / queued / running / unwritten, counts one more, and hands back a recycled
    // pinned buffer if there is one (else null: the caller makes a new one).
    std::unique_ptr<PinnedBuf> take_slot(size_t cap)
    {
        std::unique_lock<std::mutex> lk(qmu_);
        cv_done_.wait(lk, [&] { return in_flight_ < cap; });
        ++in_flight_;
        std::unique_ptr<PinnedBuf> buf;
        if (!pool_bufs_.empty()) { buf = std::move(pool_bufs_.back()); pool_bufs_.pop_back(); }
        return buf;
    }
    // a planned batch whose bytes are in memory: ready for a worker
    void push(Ptr b) { std::lock_guard<std::mutex> lk(qmu_); todo_.push_back(std::move(b)); cv_todo_.notify_one(); }
    // a batch that was sketched outside the workers (a streamed big file): it takes its slot without waiting and is finished at once
    void publish(Ptr b)
    {
        std::lock_guard<std::mutex> lk(qmu_);
        ++in_flight_;
        finished_[b->index] = std::move(b);
        cv_done_.notify_all();
    }
    // no batch follows; `n_batches` were planned in all
    void close(uint64_t n_batches)
    {
        std::lock_guard<std::mutex> lk(qmu_);
        no_more_ = batches_known_ = true;
        n_batches_total_ = n_batches;
        cv_todo_.notify_all();
        cv_done_.notify_all();
    }
    // ---- GPU workers ----
    // The next batch to sketch, or null once the queue is closed and empty.  `live`: the batch hands parts to the writer while it
    // is being sketched (the by-record routes).
    Ptr next(bool live)
    {
        std::unique_lock<std::mutex> lk(qmu_);
        cv_todo_.wait(lk, [&] { return !todo_.empty() || no_more_; });
        if (todo_.empty()) return nullptr;
        Ptr b = todo_.front();
        todo_.pop_front();
        if (live) { live_[b->index] = b; cv_done_.notify_all(); }
        return b;
    }
    // One more part of a live batch.  A worker whose batch holds `cap_bytes` of unwritten parts waits for the writer — unless the writer
    // is waiting for a batch nobody has started yet (which may be the next one in this worker's own queue).  Returns the batch's
    // unwritten bytes after the push.
    size_t add_part(Batch &b, std::vector<uint8_t> part, size_t cap_bytes)
    {
        std::unique_lock<std::mutex> lk(qmu_);
        cv_done_.wait(lk, [&] {
            return b.parts_bytes < cap_bytes || (writer_want_ != b.index && !live_.count(writer_want_) && !finished_.count(writer_want_));
        });
        b.parts_bytes += part.size();
        b.parts.push_back(std::move(part));
        cv_done_.notify_all();
        return b.parts_bytes;
    }
    // sketched (or failed: b->err): its pinned buffer goes back to the pool, the writer may finish it
    void finish(const Ptr &b)
    {
        std::lock_guard<std::mutex> lk(qmu_);
        if (b->buf) pool_bufs_.push_back(std::move(b->buf));
        live_.erase(b->index);
        finished_[b->index] = b;
        cv_done_.notify_all();
    }
    // ---- writer (one thread) ----
    // the batch whose turn it is, as soon as it is live or finished; null once every planned batch has been written
    Ptr writer_next()
    {
        std::unique_lock<std::mutex> lk(qmu_);
        const uint64_t want = writer_want_;
        cv_done_.wait(lk, [&] { return finished_.count(want) || live_.count(want) || (batches_known_ && want >= n_batches_total_); });
        if (finished_.count(want)) return finished_[want];
        if (live_.count(want)) return live_[want];
        return nullptr;
    }
    // the next part of that batch, as it comes; false once the batch is finished and has no part left
    bool writer_next_part(Batch &b, std::vector<uint8_t> &part)
    {
        std::unique_lock<std::mutex> lk(qmu_);
        cv_done_.wait(lk, [&] { return !b.parts.empty() || finished_.count(writer_want_); });
        if (b.parts.empty()) return false;
        part = std::move(b.parts.front());
        b.parts.pop_front();
        b.parts_bytes -= part.size();
        cv_done_.notify_all();
        return true;
    }
    // that batch has no part left: its slot is free, the next batch's turn
    void writer_done()
    {
        std::lock_guard<std::mutex> lk(qmu_);
        finished_.erase(writer_want_);
        --in_flight_;
        ++writer_want_;
        cv_done_.notify_all();
    }
    // (for checks) batches planned but not yet written; pinned buffers at rest in the pool
    size_t in_flight() { std::lock_guard<std::mutex> lk(qmu_); return in_flight_; }
    size_t pooled_buffers() { std::lock_guard<std::mutex> lk(qmu_); return pool_bufs_.size(); }

private:
    std::mutex qmu_;                                        // guards everything below, and every Batch's parts / parts_bytes
    std::condition_variable cv_todo_, cv_done_;
    std::deque<Ptr> todo_;                                  // read into memory, waiting for a worker
    std::map<uint64_t, Ptr> live_;                          // being sketched, parts leaving
    std::map<uint64_t, Ptr> finished_;                      // sketched, not yet written
    std::vector<std::unique_ptr<PinnedBuf>> pool_bufs_;     // recycled pinned buffers
    size_t in_flight_ = 0;                                  // batches planned but not yet written
    uint64_t writer_want_ = 0;                              // the batch the writer is at
    bool no_more_ = false, batches_known_ = false;
    uint64_t n_batches_total_ = 0;
};

}  // namespace lashhost
