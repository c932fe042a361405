// debug.cpp -- profiling hooks that only download engine state (include/mxp.h); nothing here
// launches a kernel or changes what an evaluation does.
#include <algorithm>

#include "engine_impl.h"

extern "C" {

int mxp_debug_dtp_lists(mxp_engine* eng, const mxp_dbatch* db, uint32_t* out, uint64_t cap, uint64_t* n_out) {
    if (!eng || !db || !out || !n_out) return MXP_ERR_ARG;
    *n_out = 0;
    // the batch's plan (a plain predicate evaluation: the plan of its value classes)
    const auto it = eng->plans.find(db->vt_mask);
    const mxp_engine::Plan* P = it == eng->plans.end() ? nullptr : it->second.get();
    if (!P || !eng->last_dtp || !eng->d_dtp_n.p) return eng->fail(MXP_ERR_STATE, "the last evaluation deferred no pairs");
    // the index kernel's grid: one list per wave of 64 requests, the array padded to whole
    // workgroups of four (engine.cpp, "deferred-pair scratch")
    const uint64_t waves = ((uint64_t)db->n + 63) / 64;
    if (!waves || eng->d_dtp_n.n < (waves + 3) / 4 * 16) return eng->fail(MXP_ERR_ARG, "not the batch of the last evaluation");
    hipError_t e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return eng->hipfail(e, "sync");
    const uint32_t head[4] = {(uint32_t)waves, P->n_fills, P->n_vtfills, eng->dtp_cap};
    uint64_t k = 0;
    for (; k < cap && k < 4; k++) out[k] = head[k];
    const uint64_t w = cap > 4 ? std::min<uint64_t>(cap - 4, waves) : 0;
    if (w && (e = hipMemcpy(out + 4, eng->d_dtp_n.p, w * 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return eng->hipfail(e, "download wave list lengths");
    *n_out = k + w;
    return MXP_OK;
}

}  // extern "C"
