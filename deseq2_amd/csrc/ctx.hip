// ctx.hip -- the host-side state of the C ABI (see capi.hip for the three files): the per-(device, stream) context,
// the error text, the tuning knobs, the profile list, and the entry points that manage them.
#include "../../include/deseq2_mi355x.h"
#include "dsq_internal.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace dsq {

thread_local char g_err[512] = "";
std::mutex g_mu;

int capi_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

const Tuning &tuning() {
    static Tuning t = {env_int("DSQ_BETA_WAVES", 4), env_int("DSQ_BETA_STAGE", -1), env_int("DSQ_BETA_BPC", 0),
                       env_int("DSQ_BETA_LDS_KB", 160),
                       env_int("DSQ_DISP_WAVES", 4), env_int("DSQ_DISP_STAGE", -1), env_int("DSQ_DISP_BPC", 0),
                       env_int("DSQ_DISP_LDS_KB", 160), env_int("DSQ_ABLATE", 0), env_int("DSQ_FORCE_ITERS", 0),
                       env_int("DSQ_DISP_XLDS", 1), env_int("DSQ_BETA_XLDS", 1), env_int("DSQ_DYNAMIC", 1),
                       env_int("DSQ_BETA_CELLS", 1), env_int("DSQ_DISP_CELL_MINP", DSQ_DISP_CELL_MINP),
                       env_int("DSQ_OVERLAP", 1), env_int("DSQ_LPT", 1),
                       env_int("DSQ_LPT_MAXN", 16384), env_int("DSQ_LPT_KEY1", 1), env_int("DSQ_LPT_KEYD", 1), env_int("DSQ_LPT_KEYM", 2),
                       env_int("DSQ_LPT_KEY2", 1), env_int("DSQ_OUTLIER_FIRST", 1), env_int("DSQ_DISP_PREDICT", -1)};
    return t;
}

int device_cu_count() {
    static int cached[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
    if (cached[dev] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cached[dev] = v;
    }
    return cached[dev];
}

int capi_check_device() {
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        return capi_fail(DSQ_ERR_DEVICE, "no HIP device available (%s); libdeseq2_mi355x has no CPU path",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    return DSQ_OK;
}

// ---- optional kernel timing (HIP events on the launch stream) ----------------------
// dsq_profile_enable(1) starts a list of (name, genes, event pair) -- one entry per bracketed launch (a fit call has
// one, the fused pipeline one per kernel); dsq_profile_count / dsq_profile_get read the durations back.  One list per
// process: dsq_profile_get indexes it.
struct ProfEntry { char name[32]; int n; hipEvent_t e0, e1; };
static bool g_prof = false;
static std::vector<ProfEntry> g_prof_list;
static std::vector<hipEvent_t> g_prof_free;
static hipEvent_t prof_event() {
    if (!g_prof_free.empty()) { hipEvent_t e = g_prof_free.back(); g_prof_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
static void prof_clear() {
    for (auto &p : g_prof_list) { g_prof_free.push_back(p.e0); g_prof_free.push_back(p.e1); }
    g_prof_list.clear();
}
static std::mutex g_prof_mu;
void capi_prof_begin(const char *name, int n, hipStream_t st) {
    if (!g_prof) return;
    std::lock_guard<std::mutex> plk(g_prof_mu);
    ProfEntry p;
    snprintf(p.name, sizeof p.name, "%s", name);
    p.n = n; p.e0 = prof_event(); p.e1 = prof_event();
    (void)hipEventRecord(p.e0, st);
    g_prof_list.push_back(p);
}
void capi_prof_end(hipStream_t st) {
    if (!g_prof) return;
    std::lock_guard<std::mutex> plk(g_prof_mu);
    if (g_prof_list.empty()) return;
    (void)hipEventRecord(g_prof_list.back().e1, st);
}
bool capi_prof_on() { return g_prof; }

// ---- the context of a (device, stream) ------------------------------------------------------------------------------
// Calls issued on different streams (e.g. the chunks of a pipelined DESeq(), deseq2_amd/parallel.py; the worker threads
// of a host call) must not share scratch, counters, staging buffers or events while both are in flight: each
// (device, stream) has its own.  Everything in a context is created, recorded and waited for on that one device and
// that one stream, by the one thread that has latched it.
struct Slot {       // a grow-only device buffer
    void *p = nullptr; size_t bytes = 0;
    std::vector<unsigned char> table;      // capi_upload_table: the bytes the slot holds (uploaded to `table_p`)
    void *table_p = nullptr;
};
struct PinBuf { void *h = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool used = false; };
constexpr int kPinRing = 8;
struct SideStream { hipStream_t s = nullptr; hipEvent_t f = nullptr, j = nullptr; };
struct StreamCtx {
    int dev = 0;
    hipStream_t main = nullptr;
    Slot slot[DSQ_WS_COUNT];
    PinBuf pin[kPinRing];                  // allocated on first use: only small host tables go through the ring
    int pin_next = 0;
    SideStream side;                       // created on first use
};
static std::map<std::pair<int, hipStream_t>, std::unique_ptr<StreamCtx>> g_ctx;   // heap-allocated: a latched pointer stays valid
static std::mutex g_ctx_mu;                // the registry alone (the workers of a host call resolve their contexts concurrently)
static thread_local StreamCtx *t_ctx = nullptr;    // resolved afresh at every entry and every job, never kept across calls

void capi_latch_stream(hipStream_t s) {
    t_ctx = nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;      // (no device: the entry point's capi_check_device() says so)
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    std::unique_ptr<StreamCtx> &c = g_ctx[{dev, s}];
    if (!c) { c.reset(new StreamCtx); c->dev = dev; c->main = s; }
    t_ctx = c.get();
}

int capi_ws_get(int slot, size_t bytes, void **out) {
    if (!t_ctx) return capi_fail(DSQ_ERR_DEVICE, "no stream context latched (hipGetDevice failed)");
    Slot &s = t_ctx->slot[slot];
    if (s.bytes < bytes) {
        if (s.p) { DSQ_HIP(hipDeviceSynchronize()); DSQ_HIP(hipFree(s.p)); s.p = nullptr; s.bytes = 0; }
        s.table_p = nullptr;               // (a new allocation may land on the old address: its bytes are not the table's)
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&s.p, want);
        if (e != hipSuccess) { s.p = nullptr; return capi_fail(DSQ_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); }
        s.bytes = want;
    }
    *out = s.p;
    return DSQ_OK;
}

// Small host tables of an ASYNCHRONOUS call (design cells, outlier metadata, replaceable flags, a spline table: the chain's
// and the per-call entries' alike; tests/test_gpu_stream_order.py calls back to back behind a busy stream).  Two things the plain
// hipMemcpyAsync from a thread_local pageable buffer did not give: (1) the source may be rewritten as soon as this
// returns -- the bytes travel through a ring of PINNED buffers, each fenced by an event recorded behind its copy (a
// buffer is reused only when its copy has run), so nothing depends on how the runtime stages pageable copies; (2) the
// tables of a design are the same analysis after analysis: a slot that already holds these bytes is not uploaded again
// (one memcmp of a few KiB instead of a copy command in front of every chain).
int capi_upload_table(int slot, const void *src, size_t bytes, hipStream_t st, void **dev_out) {
    void *v;
    int rc = capi_ws_get(slot, bytes, &v);
    if (rc) return rc;
    *dev_out = v;
    StreamCtx &c = *t_ctx;
    Slot *sl = &c.slot[slot];
    if (sl->table_p == v && sl->table.size() == bytes && memcmp(sl->table.data(), src, bytes) == 0) return DSQ_OK;
    PinBuf &b = c.pin[c.pin_next];
    c.pin_next = (c.pin_next + 1) % kPinRing;
    if (b.used) DSQ_HIP(hipEventSynchronize(b.done));              // (eight uploads ago: long done)
    if (b.cap < bytes) {
        if (b.h) DSQ_HIP(hipHostFree(b.h));
        b.h = nullptr; b.cap = 0;
        DSQ_HIP(hipHostMalloc(&b.h, bytes + bytes / 2 + 256, hipHostMallocDefault));
        b.cap = bytes + bytes / 2 + 256;
    }
    if (!b.done) DSQ_HIP(hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
    memcpy(b.h, src, bytes);
    DSQ_HIP(hipMemcpyAsync(v, b.h, bytes, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipEventRecord(b.done, st));
    b.used = true;
    sl->table.assign((const unsigned char *)src, (const unsigned char *)src + bytes);
    sl->table_p = v;
    return DSQ_OK;
}

int capi_side_stream(hipStream_t *side, hipEvent_t *fork_ev, hipEvent_t *join_ev) {
    if (!t_ctx) return capi_fail(DSQ_ERR_DEVICE, "no stream context latched (hipGetDevice failed)");
    SideStream &e = t_ctx->side;
    if (!e.s) {
        // (default priority: the refit beside the bulk Cook's pass was not measurably quicker with this stream at the lowest,
        //  profiles/outlier_first.md)
        DSQ_HIP(hipStreamCreateWithFlags(&e.s, hipStreamNonBlocking));
        DSQ_HIP(hipEventCreateWithFlags(&e.f, hipEventDisableTiming));
        DSQ_HIP(hipEventCreateWithFlags(&e.j, hipEventDisableTiming));
    }
    *side = e.s; *fork_ev = e.f; *join_ev = e.j;
    return DSQ_OK;
}

}  // namespace dsq

using namespace dsq;

extern "C" {

int dsq_version(void) { return DSQ_VERSION; }
const char *dsq_last_error(void) { return g_err; }

int dsq_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

int dsq_set_device(int device) {
    if (hipSetDevice(device) != hipSuccess) return capi_fail(DSQ_ERR_DEVICE, "hipSetDevice(%d) failed", device);
    return DSQ_OK;
}

int dsq_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_prof = on != 0;
    prof_clear();
    return DSQ_OK;
}

static double prof_ms(const ProfEntry &p) {
    float ms = 0.f;
    if (hipEventSynchronize(p.e1) != hipSuccess || hipEventElapsedTime(&ms, p.e0, p.e1) != hipSuccess) return -1.0;
    return (double)ms;
}

double dsq_profile_last_ms(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_prof_list.empty()) return -1.0;
    return prof_ms(g_prof_list.back());
}

int dsq_profile_count(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return (int)g_prof_list.size();
}

int dsq_profile_get(int i, char *name, int cap, int32_t *genes, double *ms) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (i < 0 || i >= (int)g_prof_list.size()) return capi_fail(DSQ_ERR_ARG, "profile entry %d out of range", i);
    const ProfEntry &p = g_prof_list[i];
    if (name && cap > 0) snprintf(name, (size_t)cap, "%s", p.name);
    if (genes) *genes = p.n;
    if (ms) *ms = prof_ms(p);
    return DSQ_OK;
}

// destroys every context: per device, synchronise, then free the slots, the pinned buffers, the events and the side
// stream.  (The worker threads of the host calls keep their streams; their next job makes a fresh context.)
int dsq_release_workspace(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    std::lock_guard<std::mutex> clk(g_ctx_mu);
    int cur = 0, synced = -1;
    (void)hipGetDevice(&cur);
    for (auto &kv : g_ctx) {               // (ordered by device)
        StreamCtx &c = *kv.second;
        if (c.dev != synced) { (void)hipSetDevice(c.dev); (void)hipDeviceSynchronize(); synced = c.dev; }
        for (Slot &s : c.slot) if (s.p) (void)hipFree(s.p);
        for (PinBuf &b : c.pin) {
            if (b.h) (void)hipHostFree(b.h);
            if (b.done) (void)hipEventDestroy(b.done);
        }
        if (c.side.s) { (void)hipStreamDestroy(c.side.s); (void)hipEventDestroy(c.side.f); (void)hipEventDestroy(c.side.j); }
    }
    g_ctx.clear();
    t_ctx = nullptr;
    (void)hipSetDevice(cur);
    return DSQ_OK;
}

}  // extern "C"
