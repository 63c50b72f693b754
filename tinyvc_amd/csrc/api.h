// What the entry files (api.hip, api_convert.hip) share: the readiness and blob checks, and the two workspace walks every entry makes
// (run_walks; measure for the tvc_workspace_bytes* queries).  The blob registry's storage stays in api.hip.
#pragma once
#include "tvc_common.h"

namespace tvc {

enum { NEED_NONE = 0, NEED_ENC = 1, NEED_DEC = 2 };
// null context -> TVC_ERR_ARG; the weights a call needs are loaded (api.hip)
int need_ready(tvc_ctx* ctx, int need);
// the prepared-blob registry (api.hip): `p` was prepared for N vectors, or carries a header that says so
int blob_check(tvc_ctx* ctx, hipStream_t s, const void* p, int64_t N, const char* what);
// noise_angle = NULL inside a stream capture is refused (api.hip)
int draw_under_capture(tvc_ctx* ctx, hipStream_t s, const float* noise_angle, const char* what);

// stands for a caller's buffer in a walk that only sizes the workspace (ws.dry: no pointer is dereferenced)
static float* const kDryPtr = (float*)(uintptr_t)256;

// behind the launching walk of an entry: it took no more workspace than its measuring walk (ws.dry) found
static inline int walks_agree(tvc_ctx* ctx, const char* entry, size_t real_peak, size_t measured) {
    return real_peak <= measured ? TVC_OK : fail(ctx, TVC_ERR_WORKSPACE, "%s: the launching walk took %zu workspace bytes, the measuring walk %zu", entry, real_peak, measured);
}

// Workspace is validated *before* launching: every entry walks its drivers twice, first with a Ws that only measures (ws.dry), then with the
// caller's workspace.  Both walks take the same allocations (tvc_common.h Ws); the host check behind the second one states it.
//   walk(Ws&) -> int        the entry's driver calls; called twice, so it must not change what it captures
//   granule                 the measured peak counts in whole granules: 1, or 4 KiB pages for the ragged entries (kRagGranule)
//   before_launch() -> int  (optional) runs once the workspace is known to suffice, in front of the launching walk
// A refused call has launched nothing: the measuring walk launches nothing, and before_launch runs behind the size check.
// (Function templates over the callables, no std::function: this is the host time of a B = 1 call.)
static inline size_t whole_granules(size_t bytes, size_t granule) { return (bytes + granule - 1) / granule * granule; }
template <class Walk, class Step>
static int run_walks(tvc_ctx* ctx, const char* entry, void* wsp, size_t ws_bytes, size_t granule, Walk&& walk, Step&& before_launch) {
    Ws need(nullptr, 0, true);
    TVC_CHECK(walk(need));
    const size_t bytes = whole_granules(need.peak, granule);
    if (bytes > ws_bytes) return fail(ctx, TVC_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", bytes, ws_bytes);
    TVC_CHECK(before_launch());
    Ws ws(wsp, bytes, false);
    TVC_CHECK(walk(ws));
    return walks_agree(ctx, entry, ws.peak, need.peak);
}
template <class Walk>
static int run_walks(tvc_ctx* ctx, const char* entry, void* wsp, size_t ws_bytes, size_t granule, Walk&& walk) {
    return run_walks(ctx, entry, wsp, ws_bytes, granule, walk, [] { return 0; });
}
// the measuring walk alone, for the tvc_workspace_bytes* queries: the same granules, and 4096 bytes on top of the peak
template <class Walk>
static int measure(size_t granule, size_t* out_bytes, Walk&& walk) {
    Ws ws(nullptr, 0, true);
    TVC_CHECK(walk(ws));
    *out_bytes = whole_granules(ws.peak, granule) + 4096;
    return TVC_OK;
}
constexpr size_t kRagGranule = 4096;

}  // namespace tvc
