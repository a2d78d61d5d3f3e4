/* launch_workspace.hpp — the device memory a launch works in (the packed
 * source records, the partials of a split launch), and the launch knobs'
 * type. Host code. launch_workspace.cpp holds the one cache of the library;
 * the launchers of pair_kernels.hip and trace_kernels.hip take their block
 * through LaunchWorkspace. */

#ifndef SKELLY_LAUNCH_WORKSPACE_HPP
#define SKELLY_LAUNCH_WORKSPACE_HPP

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>

namespace skelly {

/* A launch knob: the value a skelly_set_*() call forced (>= 0), else the
 * environment variable, read once and passed through `clamp` (`dflt` without
 * the variable). */
struct Knob {
    const char *env;
    int dflt;
    int (*clamp)(int);
    int forced = -1; /* -1 = follow env var */
    std::once_flag once;
    int from_env = 0;

    int get() {
        if (forced >= 0)
            return forced;
        std::call_once(once, [this] {
            const char *e = getenv(env);
            from_env = clamp(e ? atoi(e) : dflt);
        });
        return from_env;
    }
};

/* The persistent launch workspace of `stream` on the current device: its
 * capacity in bytes (0 without one), and its release with every block it
 * retired, for a stream that is idle and about to be destroyed. */
long long persistent_ws_bytes(hipStream_t stream);
void release_persistent_ws(hipStream_t stream);

/* One launch's workspace on `stream`: the stream's persistent block when
 * SKELLY_PERSISTENT_WS / skelly_set_persistent_ws() says so and it can be had,
 * else a hipMallocAsync block that finish() hands back with hipFreeAsync (see
 * launch_workspace.cpp for the two modes). A launch that fits the persistent
 * block allocates nothing. */
class LaunchWorkspace {
  public:
    LaunchWorkspace() = default;
    LaunchWorkspace(const LaunchWorkspace &) = delete;
    LaunchWorkspace &operator=(const LaunchWorkspace &) = delete;
    /* a mempool block that finish() never saw still goes back to its pool */
    ~LaunchWorkspace();

    /* `bytes` of workspace; on an error (hipMallocAsync's) there is none. */
    hipError_t acquire(hipStream_t stream, size_t bytes);
    double *get() const { return ptr_; }
    /* What the launcher returns: launch_err, or for a mempool block that
     * launched without error the result of its hipFreeAsync. */
    hipError_t finish(hipError_t launch_err);

  private:
    double *ptr_ = nullptr;
    hipStream_t stream_ = nullptr;
    bool pooled_ = false; /* the persistent block: nothing to free */
};

} // namespace skelly

#endif /* SKELLY_LAUNCH_WORKSPACE_HPP */
