// host_queue_check.cpp — lash_amd/csrc/host/batch_queue.hpp without the library and without a GPU: a planner thread, 1 and 3 fake
// workers that sleep where the GPU would work, and a writer, over fake "pinned" buffers.  One worker or three under an in-flight cap of 3
// (the smallest the driver computes) are the shapes at which the wait rules could deadlock; tests/test_host.py builds this file with
// ThreadSanitizer, and again with AddressSanitizer + UBSan, and runs it.  Exit status 0 and "all scenarios passed" = every check held.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "../lash_amd/csrc/host/batch_queue.hpp"

using namespace lashhost;

namespace {

std::atomic<int> g_live_allocs{0}, g_failures{0};
void *fake_alloc(size_t n) { ++g_live_allocs; return malloc(n); }
void fake_free(void *p) { if (p) { --g_live_allocs; free(p); } }

#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

enum Scenario { WHOLE_IMAGES, BY_RECORD, MIXED_WITH_PUBLISHED };
const char *const kNames[] = {"whole-image batches", "by-record batches", "every fifth batch published by the planner"};

constexpr uint64_t kBatches = 40, kErrorBatch = 7;
constexpr size_t kInFlightCap = 3, kParts = 5, kPartBytes = 100, kPartCap = 2 * kPartBytes;

void nap(int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }

bool published(Scenario sc, uint64_t i) { return sc == MIXED_WITH_PUBLISHED && i % 5 == 4; }

void run(Scenario sc, int n_workers)
{
    BatchQueue q;
    std::atomic<int> buffers_made{0};
    const bool live = sc == BY_RECORD;

    std::thread planner([&] {
        for (uint64_t i = 0; i < kBatches; ++i) {
            auto b = std::make_shared<Batch>();
            b->index = i;
            b->f0 = (size_t)i;
            b->f1 = (size_t)i + 1;
            if (i == kErrorBatch) b->err = "batch 7 could not be read";
            if (published(sc, i)) {                         // a streamed big file: sketched right here, no slot awaited, no buffer
                nap(300);
                b->images.assign(8, (uint8_t)i);
                q.publish(b);
                continue;
            }
            b->buf = q.take_slot(kInFlightCap);
            CHECK(q.in_flight() <= kInFlightCap + (sc == MIXED_WITH_PUBLISHED ? kBatches / 5 : 0), "batch %llu", (unsigned long long)i);
            if (!b->buf) { b->buf.reset(new PinnedBuf(fake_alloc, fake_free)); ++buffers_made; }
            CHECK(b->buf->reserve(64 + (size_t)i), "reserve");
            b->buf->p[0] = (uint8_t)i;
            q.push(b);
        }
        q.close(kBatches);
    });

    std::vector<std::thread> workers;
    for (int w = 0; w < n_workers; ++w)
        workers.emplace_back([&] {
            while (BatchQueue::Ptr b = q.next(live)) {
                CHECK(b->buf && b->buf->p[0] == (uint8_t)b->index, "batch %llu came without its buffer", (unsigned long long)b->index);
                if (b->err.empty() && live) {
                    for (size_t part = 0; part < kParts; ++part) {
                        nap(200);
                        std::vector<uint8_t> bytes(kPartBytes, (uint8_t)part);
                        bytes[0] = (uint8_t)b->index;
                        const size_t unwritten = q.add_part(*b, std::move(bytes), kPartCap);
                        CHECK(unwritten <= kPartCap + kPartBytes, "batch %llu holds %zu unwritten bytes", (unsigned long long)b->index, unwritten);
                    }
                } else if (b->err.empty()) {
                    nap(300);
                    b->images.assign(8, (uint8_t)b->index);
                }
                q.finish(b);
            }
        });

    std::thread writer([&] {
        uint64_t want = 0;
        while (BatchQueue::Ptr b = q.writer_next()) {
            CHECK(b->index == want, "the writer got batch %llu, expected %llu", (unsigned long long)b->index, (unsigned long long)want);
            size_t parts = 0;
            for (;;) {
                std::vector<uint8_t> part;
                if (!q.writer_next_part(*b, part)) break;
                CHECK(part.size() == kPartBytes && part[0] == (uint8_t)want && part[1] == (uint8_t)parts, "batch %llu part %zu out of order",
                      (unsigned long long)want, parts);
                ++parts;
                nap(400);                                   // a writer slower than the workers: they run into the part cap
            }
            q.writer_done();
            if (want == kErrorBatch) CHECK(!b->err.empty() && b->images.empty() && parts == 0, "the error batch was not delivered as one");
            else if (live) CHECK(parts == kParts && b->err.empty(), "batch %llu delivered %zu parts", (unsigned long long)want, parts);
            else CHECK(parts == 0 && b->images.size() == 8 && b->images[0] == (uint8_t)want, "batch %llu delivered other images", (unsigned long long)want);
            ++want;
        }
        CHECK(want == kBatches, "the writer saw %llu batches", (unsigned long long)want);
    });

    planner.join();
    for (auto &t : workers) t.join();
    writer.join();
    CHECK(q.in_flight() == 0, "in_flight ends at %zu", q.in_flight());
    CHECK(q.pooled_buffers() == (size_t)buffers_made && buffers_made >= 1 && buffers_made <= (int)kInFlightCap,
          "%zu buffers in the pool, %d made", q.pooled_buffers(), (int)buffers_made);
    printf("%s, %d worker%s: %d buffers made, all back in the pool\n", kNames[sc], n_workers, n_workers == 1 ? "" : "s", (int)buffers_made);
}

}  // namespace

int main()
{
    for (int sc = 0; sc < 3; ++sc)
        for (int n_workers : {1, 3}) run((Scenario)sc, n_workers);
    CHECK(g_live_allocs == 0, "%d fake pinned allocations were never freed", (int)g_live_allocs);
    if (g_failures) { fprintf(stderr, "%d checks failed\n", (int)g_failures); return 1; }
    printf("all scenarios passed\n");
    return 0;
}
