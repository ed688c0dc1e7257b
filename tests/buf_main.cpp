// buf_main.cpp — the owning types of tinysql_amd/csrc/tsq_internal.h (DevBuf, PinnedBuf, DevEvent, StreamDrain) on the host, without
// a GPU and without the HIP runtime: the few HIP entry points the header calls are defined here over malloc, with counters of the
// live blocks and events.  Built with -fsanitize=address,undefined by tests/test_buf_cpu.py; prints one "ok <case>" line per case
// and exits 1 at the first expectation that does not hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../tinysql_amd/csrc/tsq_internal.h"

static long live_dev = 0, live_host = 0, live_events = 0, dev_frees = 0, host_frees = 0, syncs = 0, syncs_at_first_free = -1;

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    *p = malloc(n ? n : 1);
    live_dev++;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) {
    if (p) {
        live_dev--;
        dev_frees++;
        if (syncs_at_first_free < 0) syncs_at_first_free = syncs;
    }
    free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) {
    *p = malloc(n ? n : 1);
    live_host++;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) {
    if (p) {
        live_host--;
        host_frees++;
    }
    free(p);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) {
    memcpy(dst, src, n);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    syncs++;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    *e = (hipEvent_t)malloc(1);
    live_events++;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    live_events--;
    free((void*)e);
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stub error"; }
}
void tsq_set_global_error(const std::string&) {}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static const size_t SMALL = 1000;         // below the pool's 64 KiB floor: hipFree at release
static const size_t LARGE = 128 << 10;    // kept by the context's pool at release

static tsq_ctx* new_ctx() {
    tsq_ctx* c = new tsq_ctx();
    c->hdr.magic = TSQ_MAGIC_CTX;
    return c;
}
static void drain_pool(tsq_ctx* c) {  // what tsq_ctx_destroy does with the pool
    for (auto& b : c->pool) (void)hipFree(b.first);
    c->pool.clear();
    c->pool_bytes = 0;
}
static void fill(void* p, size_t n, unsigned seed) {
    for (size_t i = 0; i < n; i++) ((unsigned char*)p)[i] = (unsigned char)(seed + i * 7);
}
static bool filled(const void* p, size_t n, unsigned seed) {
    for (size_t i = 0; i < n; i++)
        if (((const unsigned char*)p)[i] != (unsigned char)(seed + i * 7)) return false;
    return true;
}

static void case_scope_exit(tsq_ctx* c) {
    const long frees0 = dev_frees;
    {
        DevBuf b;
        CHECK(b.reserve(c, &c->hdr, SMALL) == TSQ_OK);
        CHECK(b.p && b.cap >= SMALL && b.owner == c && live_dev == 1);
    }
    CHECK(live_dev == 0 && dev_frees == frees0 + 1 && c->pool.empty());
    {
        DevBuf b;
        CHECK(b.reserve(c, &c->hdr, LARGE) == TSQ_OK);
    }
    CHECK(live_dev == 1 && c->pool.size() == 1 && c->pool_bytes == LARGE);  // the pool keeps it
    drain_pool(c);
    CHECK(live_dev == 0);
    puts("ok scope_exit");
}

static void case_moves(tsq_ctx* c) {
    const long frees0 = dev_frees;
    {
        DevBuf a;
        CHECK(a.reserve(c, &c->hdr, SMALL) == TSQ_OK);
        void* p = a.p;
        const size_t cap = a.cap;
        DevBuf b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && !a.foreign);
        CHECK(b.p == p && b.cap == cap && b.owner == c && live_dev == 1);
        DevBuf d;
        CHECK(d.reserve(c, &c->hdr, SMALL) == TSQ_OK && live_dev == 2);
        d = std::move(b);  // d's own block goes, b's arrives
        CHECK(b.p == nullptr && b.cap == 0 && d.p == p && live_dev == 1 && dev_frees == frees0 + 1);
        DevBuf& self = d;
        d = std::move(self);
        CHECK(d.p == p && d.cap == cap && live_dev == 1 && dev_frees == frees0 + 1);
    }
    CHECK(live_dev == 0 && dev_frees == frees0 + 2);  // two blocks were made, each freed exactly once
    puts("ok moves");
}

static void case_foreign(tsq_ctx* c) {
    const long frees0 = dev_frees;
    unsigned char* callers = (unsigned char*)malloc(256);
    fill(callers, 256, 3);
    {
        DevBuf b;
        b.adopt(callers, 256);
        CHECK(b.foreign && b.p == callers);
        DevBuf m(std::move(b));  // the flag travels
        CHECK(m.foreign && !b.foreign && b.p == nullptr);
    }
    CHECK(dev_frees == frees0 && live_dev == 0 && filled(callers, 256, 3));  // never freed here
    {
        DevBuf b;
        b.adopt(callers, 256);
        CHECK(b.reserve(c, &c->hdr, 4096, true, 256) == TSQ_OK);
        CHECK(!b.foreign && b.p != callers && b.cap >= 4096 && filled(b.p, 256, 3) && live_dev == 1);
        CHECK(dev_frees == frees0 && filled(callers, 256, 3));
    }
    CHECK(live_dev == 0 && dev_frees == frees0 + 1);
    free(callers);
    puts("ok foreign");
}

static void case_keep_growth(tsq_ctx* c) {
    {
        DevBuf b;
        CHECK(b.reserve(c, &c->hdr, 512) == TSQ_OK);
        fill(b.p, 512, 9);
        void* old = b.p;
        CHECK(b.reserve(c, &c->hdr, 300) == TSQ_OK && b.p == old);  // never shrinks, never moves for less
        CHECK(b.reserve(c, &c->hdr, 5000, true, 512) == TSQ_OK);
        CHECK(b.cap >= 5000 && filled(b.p, 512, 9) && live_dev == 1);
    }
    CHECK(live_dev == 0);
    puts("ok keep_growth");
}

static void case_vector(tsq_ctx* c) {
    const long frees0 = dev_frees;
    {
        std::vector<DevBuf> v(2);
        CHECK(v[0].reserve(c, &c->hdr, SMALL) == TSQ_OK && v[1].reserve(c, &c->hdr, 2 * SMALL) == TSQ_OK);
        fill(v[1].p, 2 * SMALL, 5);
        void *p0 = v[0].p, *p1 = v[1].p;
        const DevBuf* where = v.data();
        v.resize(4 * v.capacity() + 100);  // a reallocation: the elements move, the blocks stay
        CHECK(v.data() != where && v[0].p == p0 && v[1].p == p1 && filled(v[1].p, 2 * SMALL, 5));
        CHECK(live_dev == 2 && dev_frees == frees0);
        std::vector<PinnedBuf> hv(1);
        CHECK(hv[0].reserve(&c->hdr, SMALL) == TSQ_OK);
        void* hp = hv[0].p;
        hv.resize(200);
        CHECK(hv[0].p == hp && live_host == 1 && host_frees == 0);
    }
    CHECK(live_dev == 0 && dev_frees == frees0 + 2);
    puts("ok vector");
}

static void case_pool_reuse(tsq_ctx* c) {
    void* first = nullptr;
    {
        DevBuf b;
        CHECK(b.reserve(c, &c->hdr, LARGE) == TSQ_OK);
        first = b.p;
    }
    CHECK(c->pool.size() == 1 && c->pool_bytes == LARGE && live_dev == 1);
    {
        DevBuf b;
        CHECK(b.reserve(c, &c->hdr, LARGE - 100) == TSQ_OK);  // within the pool's fit window
        CHECK(b.p == first && b.cap == LARGE && c->pool.empty() && c->pool_bytes == 0 && live_dev == 1);
    }
    CHECK(c->pool.size() == 1 && c->pool_bytes == LARGE);
    drain_pool(c);
    CHECK(live_dev == 0);
    puts("ok pool_reuse");
}

static void case_arena(tsq_ctx* c) {
    const size_t slab = 1 << 20;
    c->arena_base = (char*)malloc(slab);
    c->arena.reset(slab);
    const long live0 = live_dev;
    {
        DevBuf a, b;
        CHECK(a.reserve(c, &c->hdr, 10000) == TSQ_OK && b.reserve(c, &c->hdr, LARGE) == TSQ_OK);
        CHECK(a.p >= (void*)c->arena_base && (char*)a.p < c->arena_base + slab && live_dev == live0);
        CHECK(c->arena.used == ((10000 + 255) & ~(size_t)255) + LARGE && c->arena.peak == c->arena.used);
        DevBuf m(std::move(a));
        CHECK(c->arena.used == ((10000 + 255) & ~(size_t)255) + LARGE);
    }
    CHECK(c->arena.used == 0 && c->arena.peak > 0 && c->arena.free_.size() == 1 && c->pool.empty() && live_dev == live0);
    free(c->arena_base);
    c->arena_base = nullptr;
    c->arena.reset(0);
    puts("ok arena");
}

static void case_pinned(tsq_ctx* c) {
    tsq_pinned_pool& pool = tsq_pinned();
    for (auto& b : pool.free_list) (void)hipHostFree(b.first);  // (what earlier cases left)
    pool.free_list.clear();
    pool.bytes = 0;
    CHECK(live_host == 0);
    const long hfrees0 = host_frees;
    void* first = nullptr;
    size_t cap = 0;
    {
        PinnedBuf b;
        CHECK(b.reserve(&c->hdr, 100000) == TSQ_OK);
        first = b.p;
        cap = b.cap;
        CHECK(cap == (size_t)128 << 10 && live_host == 1);  // 64 KiB granules below 1 MiB
        PinnedBuf m(std::move(b));
        CHECK(b.p == nullptr && b.cap == 0 && m.p == first && m.cap == cap);
        PinnedBuf& self = m;
        m = std::move(self);
        CHECK(m.p == first && m.cap == cap);
    }
    CHECK(pool.free_list.size() == 1 && pool.bytes == cap && live_host == 1 && host_frees == hfrees0);  // to the pool, once
    {
        PinnedBuf b;
        CHECK(b.reserve(&c->hdr, 90000) == TSQ_OK);
        CHECK(b.p == first && pool.free_list.empty() && pool.bytes == 0);  // ... and back
        void* q = b.detach();
        CHECK(q == first && b.p == nullptr);
        (void)hipHostFree(q);  // (a detached block is the caller's)
    }
    CHECK(pool.free_list.empty() && live_host == 0);
    puts("ok pinned");
}

static tsq_status failing_step(tsq_ctx* c) { return tsq_fail(&c->hdr, TSQ_ERR_INVALID, "no"); }
static tsq_status three_temporaries(tsq_ctx* c, bool drain_first) {
    DevBuf a, b, d;
    if (drain_first) {
        StreamDrain drain(c->stream);  // (declared after the buffers: runs before they go)
        TSQ_TRY(a.reserve(c, &c->hdr, SMALL));
        TSQ_TRY(b.reserve(c, &c->hdr, SMALL));
        TSQ_TRY(d.reserve(c, &c->hdr, SMALL));
        CHECK(live_dev == 3);
        TSQ_TRY(failing_step(c));
        return TSQ_OK;
    }
    TSQ_TRY(a.reserve(c, &c->hdr, SMALL));
    TSQ_TRY(b.reserve(c, &c->hdr, SMALL));
    TSQ_TRY(d.reserve(c, &c->hdr, SMALL));
    CHECK(live_dev == 3);
    TSQ_TRY(failing_step(c));
    return TSQ_OK;
}
static void case_early_return(tsq_ctx* c) {
    long frees0 = dev_frees;
    const long syncs0 = syncs;
    CHECK(three_temporaries(c, false) == TSQ_ERR_INVALID);
    CHECK(live_dev == 0 && dev_frees == frees0 + 3 && syncs == syncs0 && c->hdr.err == "no");  // no wait that the function does not ask for
    frees0 = dev_frees;
    syncs_at_first_free = -1;
    CHECK(three_temporaries(c, true) == TSQ_ERR_INVALID);
    CHECK(live_dev == 0 && dev_frees == frees0 + 3 && syncs == syncs0 + 1 && syncs_at_first_free == syncs0 + 1);  // the guard ran first
    puts("ok early_return");
}

static void case_events() {
    {
        DevEvent e;
        CHECK(!e && live_events == 0);
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && e && live_events == 1);
        hipEvent_t raw = e;
        CHECK(e.create() == hipSuccess && (hipEvent_t)e == raw && live_events == 1);  // on demand: once
        DevEvent m(std::move(e));
        CHECK(!e && (hipEvent_t)m == raw && live_events == 1);
        DevEvent ring[3];
        CHECK(ring[1].create() == hipSuccess && live_events == 2);
        ring[1] = std::move(m);
        CHECK(live_events == 1 && (hipEvent_t)ring[1] == raw && !m);
    }
    CHECK(live_events == 0);
    puts("ok events");
}

int main() {
    tsq_ctx* c = new_ctx();
    case_scope_exit(c);
    case_moves(c);
    case_foreign(c);
    case_keep_growth(c);
    case_vector(c);
    case_pool_reuse(c);
    case_arena(c);
    case_pinned(c);
    case_early_return(c);
    case_events();
    CHECK(live_dev == 0 && live_host == 0 && live_events == 0 && c->pool.empty());
    delete c;
    puts("ok all");
    return 0;
}
