/* launch_workspace.cpp — the library's one launch-workspace cache. */

#include "launch_workspace.hpp"

#include <map>
#include <vector>

namespace skelly {

/* The launch workspace (the source records of every launch and the partials
 * of the split ones). SKELLY_PERSISTENT_WS / skelly_set_persistent_ws():
 *   1 (default)  a grow-only hipMalloc block cached per (device, stream).
 *      Reuse across launches is safe because launches on one stream are
 *      ordered; an outgrown block is RETIRED, not freed or reused, for as
 *      long as its stream lives (queued work and captured graphs may still
 *      reference it; geometric growth bounds what is held at ~2x the final
 *      size). Nothing is allocated by a launch that fits, so such launches
 *      can be captured into a graph.
 *   0  a hipMallocAsync/hipFreeAsync pair per launch on the stream-ordered
 *      mempool. This was the default until it was found to give wrong
 *      results; see WORKSPACE_DEFECT below. Kept as a switch for comparison
 *      only. A launch also falls back to it if hipMalloc fails.
 *
 * WORKSPACE_DEFECT (open; DESIGN.md, "Launch workspace"): with the mempool
 * workspace, a fresh process that made ten synchronised calls of different
 * kernels back to back, host forms or device forms, got a wrong result in
 * 15 of 48 runs on MI355X (every target off by about one far source's worth:
 * some of the records the pair kernel read were not the ones pack_sources
 * had just written). It takes the pool handing its memory back at
 * hipStreamSynchronize (release threshold 0) and the next launch mapping
 * memory anew: with the threshold at its maximum, or with the persistent
 * block, none in 24 and none in 48. */
static Knob g_persistent_ws{"SKELLY_PERSISTENT_WS", 1, [](int v) { return v != 0 ? 1 : 0; }};

namespace {
struct WsEntry {
    void *ptr = nullptr;
    size_t cap = 0;
    std::vector<void *> retired;
};
struct WsCache {
    std::mutex mu;
    std::map<std::pair<int, hipStream_t>, WsEntry> blocks; /* (device, stream) */
};
WsCache &ws_cache() {
    static WsCache c;
    return c;
}
int current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev;
}
} // namespace

static double *persistent_ws(hipStream_t stream, size_t bytes) {
    WsCache &c = ws_cache();
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(c.mu);
    WsEntry &e = c.blocks[{dev, stream}];
    if (e.cap < bytes) {
        size_t want = bytes * 2;
        void *p = nullptr;
        if (hipMalloc(&p, want) != hipSuccess)
            return nullptr; /* caller falls back to the async path */
        if (e.ptr)
            e.retired.push_back(e.ptr);
        e.ptr = p;
        e.cap = want;
    }
    return static_cast<double *>(e.ptr);
}

long long persistent_ws_bytes(hipStream_t stream) {
    WsCache &c = ws_cache();
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.blocks.find({dev, stream});
    return it == c.blocks.end() ? 0 : (long long)it->second.cap;
}

void release_persistent_ws(hipStream_t stream) {
    WsCache &c = ws_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    for (auto it = c.blocks.begin(); it != c.blocks.end();) {
        if (it->first.second != stream) {
            ++it;
            continue;
        }
        (void)hipFree(it->second.ptr);
        for (void *p : it->second.retired)
            (void)hipFree(p);
        it = c.blocks.erase(it);
    }
}

hipError_t LaunchWorkspace::acquire(hipStream_t stream, size_t bytes) {
    stream_ = stream;
    if (g_persistent_ws.get() != 0) {
        ptr_ = persistent_ws(stream, bytes);
        pooled_ = ptr_ != nullptr;
    }
    if (pooled_)
        return hipSuccess;
    const hipError_t err = hipMallocAsync((void **)&ptr_, bytes, stream);
    if (err != hipSuccess)
        ptr_ = nullptr;
    return err;
}

hipError_t LaunchWorkspace::finish(hipError_t launch_err) {
    if (pooled_ || !ptr_)
        return launch_err;
    const hipError_t freed = hipFreeAsync(ptr_, stream_);
    ptr_ = nullptr;
    return launch_err != hipSuccess ? launch_err : freed;
}

LaunchWorkspace::~LaunchWorkspace() { (void)finish(hipSuccess); }

} // namespace skelly

/* Runtime override of the persistent launch workspace (see
 * g_persistent_ws above): hipGraph capture of the GMRES iteration
 * (gmres.py use_graph) requires it — hipMallocAsync nodes cannot be
 * recorded reliably, and the grow-only hipMalloc happens during the
 * UNCAPTURED warmup pass, so capture itself allocates nothing. */
extern "C" void skelly_set_persistent_ws(int on) {
    skelly::g_persistent_ws.forced = on;
}

extern "C" int skelly_persistent_ws_bytes(void *stream, long long *out_bytes) {
    *out_bytes = skelly::persistent_ws_bytes((hipStream_t)stream);
    return 0;
}

