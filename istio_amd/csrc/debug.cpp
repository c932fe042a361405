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
    if (w < waves || cap < 4 + waves + 6) return MXP_OK;
    // the retained-bitmap fill: the host's decision, the device's dense fallbacks, live quad rows
    // (nonzero count bytes) of this evaluation's generation and of the previous one's, this
    // evaluation's quads with all 8 slots taken and the pairs it sent to the overflow list
    uint32_t tail[6] = {eng->last_sparse ? 1u : 0u, 0u, 0u, 0u, 0u, 0u};
    if (eng->d_ret_w.p && (e = hipMemcpy(&tail[1], eng->d_ret_w.as<uint32_t>() + 1, 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return eng->hipfail(e, "download fallback count");
    const uint64_t row = MXP_DTP_ROW(eng->last_tiles), live = (uint64_t)eng->last_tiles * 256u;
    std::vector<uint8_t> qn((size_t)eng->last_nch * row);
    for (uint32_t g = 0; g < (eng->last_sparse ? 2u : 1u); g++) {
        const DevBuf& B = eng->d_dtp_qn[g ? eng->last_prev_gen : eng->last_gen];
        if (!B.p || B.n < qn.size()) return eng->fail(MXP_ERR_STATE, "deferred-pair counts gone");
        if (!qn.empty() && (e = hipMemcpy(qn.data(), B.p, qn.size(), hipMemcpyDeviceToHost)) != hipSuccess)
            return eng->hipfail(e, "download pair counts");
        for (uint32_t c = 0; c < eng->last_nch; c++)
            for (uint64_t q = 0; q < live; q++) {
                tail[2 + g] += qn[c * row + q] != 0;
                if (!g) tail[4] += qn[c * row + q] >= 8;
            }
    }
    if (eng->d_dtp_ovf_n.p &&
        (e = hipMemcpy(&tail[5], eng->d_dtp_ovf_n.as<uint32_t>() + 4u * eng->last_cset, 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return eng->hipfail(e, "download overflow count");
    for (uint32_t i = 0; i < 6; i++) out[k + w + i] = tail[i];
    *n_out = k + w + 6;
    return MXP_OK;
}

}  // extern "C"
