// wm_fpfh_ws.hpp -- the workspace of the feature descriptors (wm_fpfh.hip) and their matching (wm_feature_match.hip):
// the context's own (ctx->fpfh), grown on demand, freed by wm_ctx_destroy; shared with no other entry point.
#pragma once
#include "wm_internal.hpp"

namespace wm {

struct FpfhWs {
    // wm_fpfh_estimate
    DevBuf pos_of;   // unsigned per input point: where it stands in the query order (what a list entry addresses)
    DevBuf words;    // 3 x u64 per query: the SPFH counts, eleven 5-bit fields per word
    DevBuf lists;    // uint2 (position, d2 bits) x feature_k per query, entry j of query i at [j * nq + i]
    DevBuf nrm_in;   // a host caller's normals
    DevBuf out, counts, n_valid;
    // wm_feature_match
    DevBuf a, b, keys_a, keys_b, flags_a, flags_b, idx, d2, n_matched;
    PinnedBuf h;     // the small results (n_valid, n_matched)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

// the workspace, created with its events on first use; nullptr (ctx->last_error set) if an event cannot be made
inline FpfhWs *fpfh_ws(wm_ctx *ctx) {
    if (ctx->fpfh) return static_cast<FpfhWs *>(ctx->fpfh);
    FpfhWs *w = new FpfhWs();
    for (hipEvent_t &e : w->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            for (hipEvent_t &d : w->ev)
                if (d) (void) hipEventDestroy(d);
            delete w;
            ctx->last_error = "hipEventCreate (feature descriptors)";
            return nullptr;
        }
    ctx->fpfh = w;
    return w;
}

}  // namespace wm
