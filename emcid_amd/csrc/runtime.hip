// The library's process-wide state, and nothing that computes: the last error message, the per-kernel-class event profiler, the
// ABI version, environment switches, and the cache of captured hipGraphs with its capture streams and mutex.
#include <mutex>

#include "common.h"

namespace emcid {

thread_local char g_last_error[512] = "";

int env_flag(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// ---- profiling state ------------------------------------------------------------------------------------
namespace {
constexpr int PROF_MAX = 16384;
unsigned g_prof_mask = 0;
int g_prof_n = 0;
hipEvent_t g_prof_ev[PROF_MAX][2];
int g_prof_cls[PROF_MAX];
bool g_prof_init = false;
}  // namespace

void prof_begin(int cls, hipStream_t st) {
    if (!(g_prof_mask & (1u << cls)) || g_prof_n >= PROF_MAX) return;
    g_prof_cls[g_prof_n] = cls;
    (void)hipEventRecord(g_prof_ev[g_prof_n][0], st);
}
void prof_end(int cls, hipStream_t st) {
    if (!(g_prof_mask & (1u << cls)) || g_prof_n >= PROF_MAX) return;
    (void)hipEventRecord(g_prof_ev[g_prof_n][1], st);
    ++g_prof_n;
}

// ---- chains of launches as cached hipGraphs -------------------------------------------------------------------
// The ~100 launches of one layer's Cholesky + block-inverse build + triangular solves take only workspace
// pointers and sizes, so the whole chain is captured once
// per (workspace, shape) and replayed: dependent-kernel boundaries inside a graph cost ~1.2 us instead of a host
// launch each.  Not used while per-kernel event timing is on (the events would be recorded at capture time).
// Graphs are captured on an internal stream: the caller's stream may be the legacy default stream, which cannot capture.
namespace {
constexpr int MAX_DEVICES = 64;
hipStream_t g_capture_stream[MAX_DEVICES] = {};      // one per device: a stream belongs to the device current at its creation
std::mutex g_state_mutex;                           // graph cache + capture streams (entry points may be called from threads)
int current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev;
}
int capture_stream_init(int dev, hipStream_t* out) {
    if (dev < 0 || dev >= MAX_DEVICES) return fail(EMCID_ERR_BAD_ARG, "emcid graph", "device ordinal out of range");
    if (!g_capture_stream[dev] && hipStreamCreateWithFlags(&g_capture_stream[dev], hipStreamNonBlocking) != hipSuccess)
        return fail(EMCID_ERR_HIP, "emcid graph", "hipStreamCreateWithFlags");
    *out = g_capture_stream[dev];
    return EMCID_OK;
}

struct GraphSlot { GraphKey key; hipGraphExec_t exec; hipGraph_t graph; uint64_t used; };
constexpr int GRAPH_SLOTS = 64;     // (32 was one bench process short: its SDXL record re-captured graphs in every call once the other records had filled the cache)
GraphSlot g_graphs[GRAPH_SLOTS];
int g_graph_n = 0;
uint64_t g_graph_clock = 0;
}  // namespace

GraphKey make_key(GraphTag tag, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> nums) {
    GraphKey k;
    memset(&k, 0, sizeof(k));
    int i = 0;
    for (const void* p : ptrs) k.ptr[i++] = p;
    i = 0;
    k.num[5] = tag;
    for (int64_t n : nums) k.num[i++] = n;
    return k;
}

int with_graph(const GraphKey& key_in, hipStream_t st, const std::function<int(hipStream_t)>& body) {
    static const int use_graph = env_flag("EMCID_GRAPH", 1);
    if (!use_graph || g_prof_mask != 0) return body(st);
    std::lock_guard<std::mutex> lock(g_state_mutex);
    GraphKey key = key_in;
    key.dev = current_device();     // the caller made the buffers' device current (emcid_amd/hip.py does; see emcid_hip.h)
    GraphSlot* slot = nullptr;
    for (int i = 0; i < g_graph_n; ++i)
        if (g_graphs[i].key == key) { slot = &g_graphs[i]; break; }
    if (!slot) {
        hipStream_t cap = nullptr;
        EMCID_TRY(capture_stream_init((int)key.dev, &cap));
        if (hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal) != hipSuccess)
            return fail(EMCID_ERR_HIP, "emcid graph", "hipStreamBeginCapture");
        const int rc = body(cap);
        hipGraph_t graph = nullptr;
        const hipError_t ec = hipStreamEndCapture(cap, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (ec != hipSuccess || !graph) return fail(EMCID_ERR_HIP, "emcid graph", "hipStreamEndCapture");
        hipGraphExec_t exec = nullptr;
        if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGraphDestroy(graph);
            return fail(EMCID_ERR_HIP, "emcid graph", "hipGraphInstantiate");
        }
        if (g_graph_n < GRAPH_SLOTS) {
            slot = &g_graphs[g_graph_n++];
        } else {   // evict the least recently used graph
            slot = &g_graphs[0];
            for (int i = 1; i < GRAPH_SLOTS; ++i)
                if (g_graphs[i].used < slot->used) slot = &g_graphs[i];
            (void)hipDeviceSynchronize();   // the evicted graph may still be executing
            (void)hipGraphExecDestroy(slot->exec);
            (void)hipGraphDestroy(slot->graph);
        }
        slot->key = key; slot->exec = exec; slot->graph = graph;
    }
    slot->used = ++g_graph_clock;
    if (hipGraphLaunch(slot->exec, st) != hipSuccess) return fail(EMCID_ERR_HIP, "emcid graph", "hipGraphLaunch");
    return EMCID_OK;
}

}  // namespace emcid

using namespace emcid;

extern "C" {

int emcid_abi_version(void) { return EMCID_ABI_VERSION; }

int emcid_profile_enable(unsigned class_mask) {
    if (class_mask && !g_prof_init) {
        for (int i = 0; i < PROF_MAX; ++i)
            for (int j = 0; j < 2; ++j)
                if (hipEventCreate(&g_prof_ev[i][j]) != hipSuccess) return fail(EMCID_ERR_HIP, __func__, "hipEventCreate");
        g_prof_init = true;
    }
    g_prof_mask = class_mask;
    g_prof_n = 0;
    return EMCID_OK;
}

int emcid_profile_collect(double* ms_per_class, int64_t* launches_per_class, int n_classes) {
    EMCID_CHECK_ARG(ms_per_class && launches_per_class && n_classes >= KC_COUNT);
    for (int c = 0; c < n_classes; ++c) { ms_per_class[c] = 0.0; launches_per_class[c] = 0; }
    for (int i = 0; i < g_prof_n; ++i) {
        if (hipEventSynchronize(g_prof_ev[i][1]) != hipSuccess) return fail(EMCID_ERR_HIP, __func__, "hipEventSynchronize");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof_ev[i][0], g_prof_ev[i][1]) != hipSuccess)
            return fail(EMCID_ERR_HIP, __func__, "hipEventElapsedTime");
        ms_per_class[g_prof_cls[i]] += ms;
        launches_per_class[g_prof_cls[i]] += 1;
    }
    const int dropped = (g_prof_n >= PROF_MAX) ? 1 : 0;
    g_prof_n = 0;
    return dropped ? fail(EMCID_ERR_WORKSPACE, __func__, "event pool exhausted; enable fewer classes") : EMCID_OK;
}

const char* emcid_last_error(void) { return g_last_error; }

}  // extern "C"
