// quota_keys.cpp -- batched Quota (include/mxp.h mxp_quota_*plan*, mxp_quota_batch), host side; the
// kernels are quota_keys.hip.  The semantics are stated in include/mxp.h; this file is the plan's
// tables and the pipeline, which follows check.cpp:
//   1. the instance engine evaluates the batch once (Eval mode, result registers, strings kept) on
//      its stream; an event marks its completion;
//   2. the rules engine resolves the batch with the ids left on the device (mxp_resolve_kept);
//   3. the rules engine's stream waits for the event, then: pick, measure, the Resolve's scan kernels
//      over the key words, ONE host synchronisation for their total (it sizes the call's blob and
//      the pool), write, probe, rank, scan, assign, follow;
//   4. the unchanged replay (mxp_quota_alloc_dedup_device, or mxp_quota_alloc_device without ids) on
//      the key ids, with amount 0 for every request that did not reach HandleQuota;
//   5. the answers, one download.
// The hash table is sized from sum(key_cap) at plan creation and never grows (it holds at most that
// many keys, so it stays at most half full); only the byte pool grows.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>

#include "quota_impl.h"
#include "quota_keys_args.h"
#include "resolve_args.h"

extern "C" hipError_t mxp_launch_resolve(const mxp_resolve_args* a, int write, hipStream_t s);
extern "C" hipError_t mxp_launch_qk_pick(const mxp_qk_args* a, int ids16, hipStream_t s);
extern "C" hipError_t mxp_launch_qk(const mxp_qk_args* a, int step, hipStream_t s);

static_assert(sizeof(mxp_quota_answer) == sizeof(mxp_qk_answer), "the answer as include/mxp.h describes it");

namespace {

constexpr int kResolveScan = 2;  // mxp_launch_resolve's scan of the counts (resolve.hip)

uint64_t pow2_at_least(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

struct mxp_quota_plan {
    mxp_engine* rules = nullptr;
    mxp_engine* inst = nullptr;
    uint64_t rules_gen = 0, res_gen = 0, inst_gen = 0;  // the configurations the plan was made for
    mxp_quota* Q = nullptr;
    int64_t def_valid = 0;
    uint32_t n_units = 0, n_cls = 0, n_keys = 0;
    uint32_t tslots = 0;
    uint64_t hash_mask = MXP_QK_OCC - 1;  // MXP_QKEY_HASH_BITS
    uint64_t ub_pool = 0;                 // upper bound of the pool bytes in use
    hipEvent_t inst_done = nullptr;
    DevBuf d_rule_unit, d_units, d_dims, d_ovrs, d_conds, d_text, d_cls_base, d_cls_cap, d_cls_next, d_cls_valid;
    DevBuf d_ent, d_pool, d_pool_new, d_count, d_key_loc;
    DevBuf d_gb_off, d_gb;  // the instance rule set's []byte pool (host-only in the engine)
    DevBuf d_ob_off, d_ob;  // a host-packed batch's overlay []byte pool, per evaluation
    uint64_t n_ob = 0;
    DevBuf dm, de, dv;  // the instance evaluation
    DevBuf d_unit, d_len, d_words, d_cls, d_code, d_failed, d_key, d_bsum, d_woff, d_blob, d_btab, d_ref, d_role, d_blk;
    DevBuf d_amount, d_be, d_skip, d_ids, d_idoff, d_eff, d_granted, d_valid, d_dup, d_out;
    size_t req_cap = 0;
    const mxp_dbatch* eval_db = nullptr;  // mxp_quota_plan_eval's batch (the instance engine's last)
    uint32_t eval_n = 0;
};

namespace {

// the argument block's plan and evaluation fields; db: the evaluated batch (its string pool)
void fill_plan(mxp_qk_args* A, mxp_quota_plan* P, const mxp_dbatch* db, uint32_t n) {
    memset(A, 0, sizeof *A);
    A->n = n;
    mxp_engine* inst = P->inst;
    if (inst && db) {
        A->vstride = (uint32_t)inst->rules.size();
        A->vals = P->dv.as<uint64_t>();
        A->err = P->de.as<uint32_t>();
        A->n_gstr = inst->gstrs.size();
        A->gstr_off = inst->d_gstr_off.as<uint64_t>();
        A->gstr = inst->d_gstr.as<uint8_t>();
        A->bstr_off = db->bstr_off.as<uint64_t>();
        A->bstr = db->bstr.as<uint8_t>();
        A->n_gb = inst->gbytes.size();
        A->gb_off = P->d_gb_off.as<uint64_t>();
        A->gb = P->d_gb.as<uint8_t>();
        A->dev_packed = db->dev_packed ? 1u : 0u;
        A->ns = db->ns;
        A->pip = db->dev_packed ? db->pip.as<uint8_t>() : nullptr;
        A->ob_off = P->d_ob_off.as<uint64_t>();
        A->ob = P->d_ob.as<uint8_t>();
        A->n_ob = db->dev_packed ? 0 : P->n_ob;
    }
    A->units = P->d_units.as<mxp_qk_unit>();
    A->dims = P->d_dims.as<mxp_qk_dim>();
    A->ovrs = P->d_ovrs.as<mxp_qk_ovr>();
    A->conds = P->d_conds.as<mxp_qk_cond>();
    A->text = P->d_text.as<uint8_t>();
    A->n_units = P->n_units;
    A->n_cls = P->n_cls;
    A->cls_base = P->d_cls_base.as<uint32_t>();
    A->cls_cap = P->d_cls_cap.as<uint32_t>();
    A->cls_next = P->d_cls_next.as<uint32_t>();
    A->cls_valid = P->d_cls_valid.as<int64_t>();
    A->rule_unit = P->d_rule_unit.as<uint32_t>();
    A->ent = P->d_ent.as<mxp_qk_ent>();
    A->tmask = P->tslots - 1;
    A->count = P->d_count.as<unsigned long long>();
    A->key_loc = P->d_key_loc.as<uint64_t>();
    A->hash_mask = P->hash_mask;
    A->default_valid_ns = P->def_valid;
}

// per-request scratch for n requests
int reserve_requests(mxp_quota_plan* P, uint32_t n) {
    mxp_engine* eng = P->rules;
    hipError_t e;
    const size_t grid = ((size_t)n + 255u) / 256u, nb = ((size_t)n + MXP_QK_BLOCK - 1) / MXP_QK_BLOCK;
    if ((e = P->d_unit.reserve((size_t)n * 4)) != hipSuccess || (e = P->d_len.reserve((size_t)n * 4)) != hipSuccess ||
        (e = P->d_words.reserve((size_t)n * 4)) != hipSuccess || (e = P->d_cls.reserve((size_t)n * 4)) != hipSuccess ||
        (e = P->d_code.reserve((size_t)n * 4)) != hipSuccess || (e = P->d_failed.reserve((size_t)n * 4)) != hipSuccess ||
        (e = P->d_key.reserve((size_t)n * 4)) != hipSuccess || (e = P->d_bsum.reserve(grid * 8 + 8)) != hipSuccess ||
        (e = P->d_woff.reserve(((size_t)n + 1) * 8)) != hipSuccess ||
        (e = P->d_btab.reserve((size_t)pow2_at_least(2ull * n) * sizeof(mxp_qk_bslot))) != hipSuccess ||
        (e = P->d_ref.reserve((size_t)n * 4)) != hipSuccess || (e = P->d_role.reserve(n)) != hipSuccess ||
        (e = P->d_blk.reserve((size_t)P->n_cls * nb * 4)) != hipSuccess)
        return eng->hipfail(e, "quota key scratch");
    return MXP_OK;
}

// a host-packed batch's overlay []byte pool to the device (the device packer's lives there already);
// s: enqueued there (db outlives the call's last synchronisation), nullptr: copied synchronously
int upload_overlay_bytes(mxp_quota_plan* P, const mxp_dbatch* db, hipStream_t s) {
    P->n_ob = 0;
    if (!db || db->dev_packed || !db->overlay_bytes.size()) return MXP_OK;
    const StrPool& ob = db->overlay_bytes;
    hipError_t e;
    if ((e = P->d_ob_off.reserve(ob.desc.size() * 8)) != hipSuccess || (e = P->d_ob.reserve(ob.blob.size() + 16)) != hipSuccess)
        return P->rules->hipfail(e, "quota overlay bytes");
    if (s) {
        if ((e = hipMemcpyAsync(P->d_ob_off.p, ob.desc.data(), ob.desc.size() * 8, hipMemcpyHostToDevice, s)) != hipSuccess ||
            (ob.blob.size() &&
             (e = hipMemcpyAsync(P->d_ob.p, ob.blob.data(), ob.blob.size(), hipMemcpyHostToDevice, s)) != hipSuccess))
            return P->rules->hipfail(e, "quota overlay bytes");
    } else if ((e = hipMemcpy(P->d_ob_off.p, ob.desc.data(), ob.desc.size() * 8, hipMemcpyHostToDevice)) != hipSuccess ||
               (ob.blob.size() && (e = hipMemcpy(P->d_ob.p, ob.blob.data(), ob.blob.size(), hipMemcpyHostToDevice)) != hipSuccess)) {
        return P->rules->hipfail(e, "quota overlay bytes");
    }
    P->n_ob = ob.desc.size();
    return MXP_OK;
}

// The stage from the measure pass on.  A: plan, evaluation, unit_in / unit, amount and (batch) the
// pick's fields set; d_key / d_code / d_failed: where the stage's outputs go.  Synchronises s once.
int run_stage(mxp_quota_plan* P, mxp_qk_args& A, hipStream_t s, uint32_t* d_key, int32_t* d_code, uint32_t* d_failed) {
    mxp_engine* eng = P->rules;
    const uint32_t n = A.n;
    hipError_t e;
    A.len = P->d_len.as<uint32_t>();
    A.words = P->d_words.as<uint32_t>();
    A.cls = P->d_cls.as<uint32_t>();
    A.code = d_code;
    A.failed = d_failed;
    A.key = d_key;
    A.block_sum = P->d_bsum.as<uint64_t>();
    A.woff = P->d_woff.as<uint64_t>();
    A.btab = P->d_btab.as<mxp_qk_bslot>();
    A.bmask = (uint32_t)(pow2_at_least(2ull * n) - 1);
    A.ref = P->d_ref.as<uint32_t>();
    A.role = P->d_role.as<uint8_t>();
    A.blk_cnt = P->d_blk.as<uint32_t>();
    A.nb = (n + MXP_QK_BLOCK - 1) / MXP_QK_BLOCK;
    mxp_resolve_args S;  // the Resolve's scan kernels over the key words
    memset(&S, 0, sizeof S);
    S.n = n;
    S.count = A.words;
    S.block_sum = A.block_sum;
    S.sel_off_out = P->d_woff.as<uint64_t>();
    uint64_t total_words = 0;
    if ((e = mxp_launch_qk(&A, 0, s)) != hipSuccess || (e = mxp_launch_resolve(&S, kResolveScan, s)) != hipSuccess ||
        (e = hipMemsetAsync((uint8_t*)P->d_count.p + 16, 0, 8, s)) != hipSuccess ||
        (e = hipMemcpyAsync(&total_words, P->d_woff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return eng->hipfail(e, "quota key lengths");
    const uint64_t bytes = total_words * 8u;
    if (bytes >= (1ull << 35)) return eng->fail(MXP_ERR_NOMEM, "quota keys: more than 32 GiB of key text in a call");
    if ((e = P->d_blob.reserve(bytes + 16)) != hipSuccess) return eng->hipfail(e, "quota key blob");
    if ((e = hipMemsetAsync(P->d_blob.as<uint8_t>() + bytes, 0, 16, s)) != hipSuccess)  // (the slack the word compares read)
        return eng->hipfail(e, "quota key blob");
    // the pool able to take every key of the call (an upper bound: hits add nothing); when the bound
    // says otherwise the true count is read back once
    if (P->ub_pool + bytes + 16 > P->d_pool.cap) {
        unsigned long long cnt[2];
        if ((e = hipMemcpyAsync(cnt, P->d_count.p, 16, hipMemcpyDeviceToHost, s)) != hipSuccess ||
            (e = hipStreamSynchronize(s)) != hipSuccess)
            return eng->hipfail(e, "quota key counts");
        P->ub_pool = cnt[1];
        if (P->ub_pool + bytes + 16 > P->d_pool.cap) {
            if ((e = P->d_pool_new.alloc(pow2_at_least(P->ub_pool + bytes + 16))) != hipSuccess)
                return eng->hipfail(e, "quota key pool growth");
            if ((e = hipMemsetAsync(P->d_pool_new.p, 0, P->d_pool_new.cap, s)) != hipSuccess ||
                (P->ub_pool &&
                 (e = hipMemcpyAsync(P->d_pool_new.p, P->d_pool.p, P->ub_pool, hipMemcpyDeviceToDevice, s)) != hipSuccess) ||
                (e = hipStreamSynchronize(s)) != hipSuccess)  // (the old block is freed below)
                return eng->hipfail(e, "quota key pool growth");
            P->d_pool.swap(P->d_pool_new);
            P->d_pool_new.reset();
        }
    }
    A.blob = P->d_blob.as<uint8_t>();
    A.pool = P->d_pool.as<uint8_t>();
    if ((e = mxp_launch_qk(&A, 1, s)) != hipSuccess || (e = mxp_launch_qk(&A, 2, s)) != hipSuccess)
        return eng->hipfail(e, "launch quota key stage");
    P->ub_pool += bytes;
    return MXP_OK;
}

}  // namespace

extern "C" {

int mxp_quota_plan_create(mxp_engine* rules, mxp_engine* inst, const mxp_quota_limit* limits, uint32_t n_limits,
                          const mxp_quota_unit* units, uint32_t n_units, const uint32_t* rule_unit, int64_t def_valid,
                          mxp_quota_plan** out) {
    if (!rules || !out || (n_limits && !limits) || (n_units && !units)) return MXP_ERR_ARG;
    if (!rules->have_rules || !rules->resolver.set)
        return rules->fail(MXP_ERR_STATE, "quota plan: the rules engine has no resolver configured");
    if (rules->device < 0) return rules->fail(MXP_ERR_STATE, "host-only engine");
    if (inst == rules) return rules->fail(MXP_ERR_ARG, "quota plan: dimension expressions belong in an engine of their own");
    if (inst && inst->device != rules->device)
        return rules->fail(MXP_ERR_ARG, "quota plan: the two engines are on different devices");
    const uint32_t NR = (uint32_t)rules->rules.size();
    if (NR && !rule_unit) return MXP_ERR_ARG;
    for (uint32_t r = 0; r < NR; r++)
        if (rule_unit[r] >= n_units && rule_unit[r] != MXP_QUOTA_NO_UNIT && rule_unit[r] != MXP_QUOTA_OTHER_UNIT)
            return rules->fail(MXP_ERR_ARG, "quota plan: rule_unit[" + std::to_string(r) + "] = " +
                                                std::to_string(rule_unit[r]) + " is not a unit (" + std::to_string(n_units) + ")");
    std::string text;
    auto put_text = [&](const std::string& s) {
        const uint32_t o = (uint32_t)text.size();
        text += s;
        return o;
    };
    // classes: per limit the default, then its overrides
    std::map<std::string, uint32_t> limit_of;
    std::vector<uint32_t> cls_first(n_limits), cls_base, cls_cap;
    std::vector<int64_t> cls_max, cls_valid;
    uint64_t n_keys = 0;
    for (uint32_t l = 0; l < n_limits; l++) {
        const mxp_quota_limit& L = limits[l];
        const std::string at = "quota plan: limit " + std::to_string(l) + ": ";
        if (!L.name) return rules->fail(MXP_ERR_ARG, at + "no name");
        if (!limit_of.emplace(L.name, l).second) return rules->fail(MXP_ERR_ARG, at + "the name '" + L.name + "' twice");
        if (L.n_overrides && !L.overrides) return MXP_ERR_ARG;
        cls_first[l] = (uint32_t)cls_base.size();
        for (uint32_t o = 0; o <= L.n_overrides; o++) {
            const bool d = o == 0;
            const int64_t mx = d ? L.max_amount : L.overrides[o - 1].max_amount;
            const int64_t vd = d ? L.valid_duration_ns : L.overrides[o - 1].valid_duration_ns;
            const uint32_t cap = d ? L.key_cap : L.overrides[o - 1].key_cap;
            if (vd < 0) return rules->fail(MXP_ERR_ARG, at + "a negative valid duration");
            cls_base.push_back((uint32_t)n_keys);
            cls_cap.push_back(cap);
            cls_max.push_back(mx);
            cls_valid.push_back(vd);
            n_keys += cap;
        }
    }
    if (cls_base.size() > MXP_QK_MAX_CLASSES)
        return rules->fail(MXP_ERR_ARG, "quota plan: " + std::to_string(cls_base.size()) + " classes (limits + overrides), at most " +
                                            std::to_string(MXP_QK_MAX_CLASSES));
    if (!n_keys || n_keys > (1u << 30)) return rules->fail(MXP_ERR_ARG, "quota plan: the key capacities sum to 0 or to more than 2^30");
    // units
    std::vector<mxp_qk_unit> U(n_units);
    std::vector<mxp_qk_dim> D;
    std::vector<mxp_qk_ovr> O;
    std::vector<mxp_qk_cond> C;
    for (uint32_t u = 0; u < n_units; u++) {
        const mxp_quota_unit& in = units[u];
        const std::string at = "quota plan: unit " + std::to_string(u) + ": ";
        if (!in.instance_name) return rules->fail(MXP_ERR_ARG, at + "no instance name");
        auto li = limit_of.find(in.instance_name);
        if (li == limit_of.end()) return rules->fail(MXP_ERR_ARG, at + "no limit named '" + in.instance_name + "'");
        if (in.n_dims > 32) return rules->fail(MXP_ERR_ARG, at + "more than 32 dimensions");
        if (in.n_dims && (!in.labels || !in.value_rules)) return MXP_ERR_ARG;
        if (in.n_dims && (!inst || !inst->have_rules)) return rules->fail(MXP_ERR_ARG, at + "dimensions without an instance engine");
        std::vector<std::pair<std::string, uint32_t>> labs;  // (label, configured index), sort.Strings order
        for (uint32_t d = 0; d < in.n_dims; d++) {
            if (!in.labels[d]) return MXP_ERR_ARG;
            labs.emplace_back(in.labels[d], d);
        }
        std::sort(labs.begin(), labs.end());
        mxp_qk_unit& W = U[u];
        memset(&W, 0, sizeof W);
        W.dim_off = (uint32_t)D.size();
        W.n_dims = in.n_dims;
        W.name_len = (uint32_t)strlen(in.instance_name);
        W.name_off = put_text(in.instance_name);
        W.fixed_len = W.name_len;
        std::map<std::string, uint32_t> dim_of;
        for (const auto& ld : labs) {
            const std::string lab = "label '" + ld.first + "': ";
            if (!dim_of.emplace(ld.first, (uint32_t)D.size()).second) return rules->fail(MXP_ERR_ARG, at + lab + "twice");
            const uint32_t vr = in.value_rules[ld.second];
            if (vr >= inst->rules.size()) return rules->fail(MXP_ERR_ARG, at + lab + "no such value rule");
            const auto& R = inst->rules[vr];
            mxp_qk_dim dd;
            memset(&dd, 0, sizeof dd);
            dd.value_rule = vr;
            dd.bit = ld.second;
            dd.label_len = (uint32_t)ld.first.size();
            dd.label_off = put_text(ld.first);
            switch (R.il_ret) {
            case mxp::IL_STRING: dd.kind = MXP_STRING; break;
            case mxp::IL_BOOL: dd.kind = MXP_BOOL; break;
            case mxp::IL_INTEGER: dd.kind = MXP_INT64; break;
            case mxp::IL_DOUBLE: dd.kind = MXP_DOUBLE; break;
            case mxp::IL_INTERFACE: dd.kind = 0; break;
            default:
                // (a rule that failed to compile errs on every evaluation, whatever its type: EVAL_ERROR)
                if (R.status == MXP_RULE_OK)
                    return rules->fail(MXP_ERR_ARG, at + lab + "a dimension of type " +
                                                        (R.il_ret == mxp::IL_DURATION ? "DURATION" : "IL " + std::to_string((int)R.il_ret)) +
                                                        " is not supported (STRING, INT64, DOUBLE, BOOL and interface-typed "
                                                        "expressions are)");
                dd.kind = 0;
            }
            W.fixed_len += 2u + dd.label_len;
            D.push_back(dd);
        }
        const mxp_quota_limit& L = limits[li->second];
        W.cls_default = cls_first[li->second];
        W.ovr_off = (uint32_t)O.size();
        W.n_ovr = L.n_overrides;
        for (uint32_t o = 0; o < L.n_overrides; o++) {
            const mxp_quota_override& ov = L.overrides[o];
            if (ov.n && (!ov.labels || !ov.values)) return MXP_ERR_ARG;
            mxp_qk_ovr oo;
            memset(&oo, 0, sizeof oo);
            oo.cond_off = (uint32_t)C.size();
            oo.cls = cls_first[li->second] + 1 + o;
            std::map<std::string, std::string> cfg;  // (a Go map: a label given twice keeps its last value)
            for (uint32_t k = 0; k < ov.n; k++) {
                if (!ov.labels[k] || !ov.values[k]) return MXP_ERR_ARG;
                cfg[ov.labels[k]] = ov.values[k];
            }
            for (const auto& kv : cfg) {
                auto di = dim_of.find(kv.first);
                if (di == dim_of.end()) {  // inst[k] == nil: matches nothing
                    oo.never = 1;
                    continue;
                }
                mxp_qk_cond cc;
                memset(&cc, 0, sizeof cc);
                cc.dim = di->second;
                cc.val_len = (uint32_t)kv.second.size();
                cc.val_off = put_text(kv.second);
                C.push_back(cc);
                oo.n_cond++;
            }
            O.push_back(oo);
        }
    }
    std::unique_ptr<mxp_quota_plan> P(new mxp_quota_plan());
    P->rules = rules;
    P->inst = inst;
    P->def_valid = def_valid;
    P->n_units = n_units;
    P->n_cls = (uint32_t)cls_base.size();
    P->n_keys = (uint32_t)n_keys;
    if (const char* v = getenv("MXP_QKEY_HASH_BITS")) {
        const int b = atoi(v);
        if (b >= 1 && b < 63) P->hash_mask = (1ull << b) - 1;
    }
    hipError_t e;
    if ((e = hipSetDevice(rules->device)) != hipSuccess) return rules->hipfail(e, "hipSetDevice");
    auto put = [&](DevBuf& d, const void* src, size_t bytes) -> bool {
        if ((e = d.alloc(bytes + 16)) != hipSuccess || (e = hipMemset(d.p, 0, bytes + 16)) != hipSuccess) return false;
        return !bytes || !src || (e = hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice)) == hipSuccess;  // (no src: zeros)
    };
    std::vector<uint32_t> zero(P->n_cls, 0);
    StrPool gb;  // (the rule set's []byte constants: fixed until the next compile, which retires the plan)
    if (inst)
        for (const std::string& b : inst->gbytes) gb.push(b);
    P->tslots = (uint32_t)pow2_at_least(std::max<uint64_t>(2 * n_keys, 16));
    if (!put(P->d_rule_unit, rule_unit, (size_t)NR * 4) || !put(P->d_units, U.data(), U.size() * sizeof(mxp_qk_unit)) ||
        !put(P->d_dims, D.data(), D.size() * sizeof(mxp_qk_dim)) || !put(P->d_ovrs, O.data(), O.size() * sizeof(mxp_qk_ovr)) ||
        !put(P->d_conds, C.data(), C.size() * sizeof(mxp_qk_cond)) || !put(P->d_text, text.data(), text.size()) ||
        !put(P->d_cls_base, cls_base.data(), cls_base.size() * 4) || !put(P->d_cls_cap, cls_cap.data(), cls_cap.size() * 4) ||
        !put(P->d_cls_next, zero.data(), zero.size() * 4) || !put(P->d_cls_valid, cls_valid.data(), cls_valid.size() * 8) ||
        !put(P->d_ent, nullptr, (size_t)P->tslots * sizeof(mxp_qk_ent)) || !put(P->d_pool, nullptr, 1u << 16) ||
        !put(P->d_count, nullptr, 32) || !put(P->d_gb_off, gb.desc.data(), gb.desc.size() * 8) ||
        !put(P->d_gb, gb.blob.data(), gb.blob.size()) || (e = P->d_key_loc.alloc((size_t)n_keys * 8)) != hipSuccess ||
        (e = hipMemset(P->d_key_loc.p, 0xFF, (size_t)n_keys * 8)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&P->inst_done, hipEventDisableTiming)) != hipSuccess)
        return rules->hipfail(e, "quota plan tables");
    // the unchanged memquota state, the limits expanded per id
    std::vector<int64_t> mx(n_keys), vd(n_keys);
    for (uint32_t c = 0; c < P->n_cls; c++)
        for (uint32_t k = 0; k < cls_cap[c]; k++) {
            mx[cls_base[c] + k] = cls_max[c];
            vd[cls_base[c] + k] = cls_valid[c];
        }
    if (int rc = mxp_quota_create(rules, (uint32_t)n_keys, mx.data(), vd.data(), &P->Q)) {
        if (P->inst_done) (void)hipEventDestroy(P->inst_done);
        return rc;
    }
    P->rules_gen = rules->rules_gen;
    P->res_gen = rules->res_gen;
    P->inst_gen = inst ? inst->rules_gen : 0;
    *out = P.release();
    return MXP_OK;
}

void mxp_quota_plan_destroy(mxp_quota_plan* plan) {
    if (!plan) return;
    if (plan->rules && plan->rules->device >= 0) (void)hipSetDevice(plan->rules->device);
    if (plan->inst_done) (void)hipEventDestroy(plan->inst_done);
    if (plan->Q) mxp_quota_destroy(plan->rules, plan->Q);
    delete plan;
}

mxp_quota* mxp_quota_plan_quota(mxp_quota_plan* plan) { return plan ? plan->Q : nullptr; }

static int plan_fresh(mxp_quota_plan* P) {
    mxp_engine *rules = P->rules, *inst = P->inst;
    if (rules->rules_gen != P->rules_gen || rules->res_gen != P->res_gen || (inst && inst->rules_gen != P->inst_gen))
        return rules->fail(MXP_ERR_ARG, "quota: a rule set was compiled (or a resolver set) after the plan was created");
    return MXP_OK;
}

int mxp_quota_batch(mxp_quota_plan* P, const mxp_bag_batch* batch, uint32_t variety, const int64_t* amount,
                    const uint8_t* best_effort, const uint8_t* id_bytes, const uint32_t* id_off, const uint8_t* skip,
                    int64_t now_ns, uint8_t* status, uint32_t* err_rule, mxp_quota_answer* out) {
    if (!P || !batch || variety >= 32 || (batch->n_requests && (!amount || !best_effort || !status || !err_rule || !out)) ||
        (id_bytes && !id_off) || (id_off && id_off[batch->n_requests] && !id_bytes))
        return MXP_ERR_ARG;
    mxp_engine *rules = P->rules, *inst = P->inst;
    int rc;
    if ((rc = plan_fresh(P))) return rc;
    const uint32_t n = batch->n_requests;
    if (n > (1u << 30)) return rules->fail(MXP_ERR_ARG, "quota: more than 2^30 requests in a call");
    if (id_off) {
        char msg[96];
        if (id_off[0] != 0) return rules->fail(MXP_ERR_ARG, "quota: id_off[0] is not 0 (request 0)");
        for (uint32_t i = 0; i < n; i++)
            if (id_off[i + 1] < id_off[i]) {
                snprintf(msg, sizeof msg, "quota: id_off decreases at request %u", i);
                return rules->fail(MXP_ERR_ARG, msg);
            }
    }
    const uint32_t NR = (uint32_t)rules->rules.size();
    uint8_t no_status = 0;  // (an empty batch: the Resolve still takes its two pointers)
    uint32_t no_rule = 0;
    if (!n && !status) status = &no_status;
    if (!n && !err_rule) err_rule = &no_rule;
    const char* e32 = getenv("MXP_CHECK_IDS32");
    const bool ids16 = NR <= 65536u && !(e32 && atoi(e32) != 0);
    hipError_t e;
    if ((e = hipSetDevice(rules->device)) != hipSuccess) return rules->hipfail(e, "hipSetDevice");
    P->eval_db = nullptr;  // (the evaluation below replaces mxp_quota_plan_eval's)
    // 1. the dimension values, on the instance engine's stream
    std::unique_ptr<mxp_dbatch> idb;
    // (the instance evaluation awaited, its error texts fetched, the batch kept as that engine's last:
    // every return after the evaluation goes through here)
    auto inst_done = [&](int ret) -> int {
        if (!idb) return ret;
        const int r2 = inst->collect_errors(batch, idb);
        if (r2 && !ret) rules->last_error = inst->last_error;
        return ret ? ret : r2;
    };
    if (inst && inst->have_rules) {
        const bool saved = inst->need_strings;
        inst->need_strings = true;  // (string dimensions are read from the batch's string pool)
        rc = inst->evaluate(batch, P->dm, P->de, &P->dv, idb);
        inst->need_strings = saved;
        if (rc) {
            rules->last_error = inst->last_error;
            idb.reset();
            return rc;
        }
        if (n && (e = hipEventRecord(P->inst_done, inst->stream)) != hipSuccess)
            return inst_done(rules->hipfail(e, "record instance event"));
    }
    // 2. the Resolve, ids kept on the device
    uint64_t n_ids = 0;
    if ((rc = mxp_resolve_kept(rules, batch, variety, ids16, status, err_rule, &n_ids))) return inst_done(rc);
    if (!n) return inst_done(MXP_OK);
    // 3. the stage
    hipStream_t s = rules->stream;
    const uint32_t id_total = id_off ? id_off[n] : 0u;
    if ((rc = reserve_requests(P, n))) return inst_done(rc);
    if ((e = P->d_amount.reserve((size_t)n * 8)) != hipSuccess || (e = P->d_be.reserve(n)) != hipSuccess ||
        (e = P->d_skip.reserve(n)) != hipSuccess || (e = P->d_eff.reserve((size_t)n * 8)) != hipSuccess ||
        (e = P->d_granted.reserve((size_t)n * 8)) != hipSuccess || (e = P->d_valid.reserve((size_t)n * 8)) != hipSuccess ||
        (e = P->d_dup.reserve(n)) != hipSuccess || (e = P->d_out.reserve((size_t)n * sizeof(mxp_qk_answer))) != hipSuccess ||
        (id_off && ((e = P->d_ids.reserve((size_t)id_total + 16)) != hipSuccess ||
                    (e = P->d_idoff.reserve(((size_t)n + 1) * 4)) != hipSuccess)))
        return inst_done(rules->hipfail(e, "alloc quota buffers"));
    if ((e = hipMemcpyAsync(P->d_amount.p, amount, (size_t)n * 8, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = hipMemcpyAsync(P->d_be.p, best_effort, n, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (skip && (e = hipMemcpyAsync(P->d_skip.p, skip, n, hipMemcpyHostToDevice, s)) != hipSuccess) ||
        (id_off && ((e = hipMemcpyAsync(P->d_idoff.p, id_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s)) != hipSuccess ||
                    (id_total && (e = hipMemcpyAsync(P->d_ids.p, id_bytes, id_total, hipMemcpyHostToDevice, s)) != hipSuccess) ||
                    (e = hipMemsetAsync(P->d_ids.as<uint8_t>() + id_total, 0, 16, s)) != hipSuccess)))
        return inst_done(rules->hipfail(e, "quota upload"));
    if (idb && (e = hipStreamWaitEvent(s, P->inst_done, 0)) != hipSuccess)
        return inst_done(rules->hipfail(e, "wait for the dimension values"));
    if ((rc = upload_overlay_bytes(P, idb.get(), s))) return inst_done(rc);
    mxp_qk_args A;
    fill_plan(&A, P, idb.get(), n);
    A.ids = rules->res_sel.p;
    A.id_off = rules->res_off.as<uint64_t>();
    A.status = rules->res_status.as<uint8_t>();
    A.skip = skip ? P->d_skip.as<uint8_t>() : nullptr;
    A.unit = P->d_unit.as<uint32_t>();
    A.unit_in = A.unit;
    A.amount = P->d_amount.as<int64_t>();
    A.code = P->d_code.as<int32_t>();
    A.eff_amount = P->d_eff.as<int64_t>();
    if ((e = mxp_launch_qk_pick(&A, ids16, s)) != hipSuccess) return inst_done(rules->hipfail(e, "launch quota pick"));
    if ((rc = run_stage(P, A, s, P->d_key.as<uint32_t>(), P->d_code.as<int32_t>(), P->d_failed.as<uint32_t>())))
        return inst_done(rc);
    // 4. the replay: requests that did not reach HandleQuota go in with amount 0
    if (id_off)
        rc = mxp_quota_alloc_dedup_device(rules, P->Q, n, A.key, A.eff_amount, P->d_be.as<uint8_t>(), P->d_ids.as<uint8_t>(),
                                          P->d_idoff.as<uint32_t>(), id_total, now_ns, s, P->d_granted.as<int64_t>(),
                                          P->d_valid.as<int64_t>(), P->d_dup.as<uint8_t>(), nullptr);
    else
        rc = mxp_quota_alloc_device(rules, P->Q, n, A.key, A.eff_amount, P->d_be.as<uint8_t>(), now_ns, s,
                                    P->d_granted.as<int64_t>(), nullptr);
    if (rc) {
        (void)hipStreamSynchronize(s);
        return inst_done(rc);
    }
    // 5. the answers
    A.best_effort = P->d_be.as<uint8_t>();
    A.granted = P->d_granted.as<int64_t>();
    A.valid_ns = id_off ? P->d_valid.as<int64_t>() : nullptr;
    A.dup = id_off ? P->d_dup.as<uint8_t>() : nullptr;
    A.out = P->d_out.as<mxp_qk_answer>();
    if ((e = mxp_launch_qk(&A, 3, s)) != hipSuccess) return inst_done(rules->hipfail(e, "launch quota answers"));
    unsigned long long full = 0;
    if ((rc = rules->download_all({{out, P->d_out.p, (size_t)n * sizeof(mxp_qk_answer)},
                                   {&full, (uint8_t*)P->d_count.p + 16, 8}},
                                  "download quota answers")))
        return inst_done(rc);
    if (full) (void)rules->fail(MXP_ERR_NOMEM, "quota: a class ran out of key ids (MXP_QUOTA_KEYS_FULL answers; every answer is complete)");
    return inst_done(full ? MXP_ERR_NOMEM : MXP_OK);
}

int mxp_quota_plan_eval(mxp_quota_plan* P, const mxp_bag_batch* batch) {
    if (!P || !batch) return MXP_ERR_ARG;
    mxp_engine *rules = P->rules, *inst = P->inst;
    int rc;
    if ((rc = plan_fresh(P))) return rc;
    P->eval_db = nullptr;
    if (!inst || !inst->have_rules) return rules->fail(MXP_ERR_STATE, "quota plan: no instance engine");
    hipError_t e;
    if ((e = hipSetDevice(rules->device)) != hipSuccess) return rules->hipfail(e, "hipSetDevice");
    std::unique_ptr<mxp_dbatch> idb;
    const bool saved = inst->need_strings;
    inst->need_strings = true;
    rc = inst->evaluate(batch, P->dm, P->de, &P->dv, idb);
    inst->need_strings = saved;
    if (!rc) rc = inst->collect_errors(batch, idb);  // (synchronises; the batch becomes that engine's last)
    if (rc) {
        rules->last_error = inst->last_error;
        return rc;
    }
    if ((rc = upload_overlay_bytes(P, inst->last_db.get(), nullptr))) return rc;
    P->eval_db = inst->last_db.get();
    P->eval_n = batch->n_requests;
    return MXP_OK;
}

int mxp_quota_keys_device(mxp_quota_plan* P, uint32_t n, const uint32_t* d_unit, const int64_t* d_amount, void* stream,
                          uint32_t* d_key, int32_t* d_code, uint32_t* d_failed) {
    if (!P || (n && (!d_unit || !d_amount || !d_key || !d_code || !d_failed))) return MXP_ERR_ARG;
    mxp_engine *rules = P->rules, *inst = P->inst;
    int rc;
    if ((rc = plan_fresh(P))) return rc;
    if (!n) return MXP_OK;
    if (!P->eval_db || !inst || inst->last_db.get() != P->eval_db || n != P->eval_n)
        return rules->fail(MXP_ERR_STATE, "quota keys: no evaluation of a batch of this many requests (mxp_quota_plan_eval)");
    hipError_t e;
    if ((e = hipSetDevice(rules->device)) != hipSuccess) return rules->hipfail(e, "hipSetDevice");
    if ((rc = reserve_requests(P, n))) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : rules->stream;
    mxp_qk_args A;
    fill_plan(&A, P, P->eval_db, n);
    A.unit_in = d_unit;
    A.amount = d_amount;
    return run_stage(P, A, s, d_key, d_code, d_failed);
}

int mxp_quota_key_text(mxp_quota_plan* P, uint32_t key_id, uint8_t* buf, uint32_t cap, uint32_t* len) {
    if (!P || !len || (cap && !buf)) return MXP_ERR_ARG;
    mxp_engine* rules = P->rules;
    if (key_id >= P->n_keys) return rules->fail(MXP_ERR_ARG, "quota key text: no key with id " + std::to_string(key_id));
    hipError_t e;
    if ((e = hipSetDevice(rules->device)) != hipSuccess) return rules->hipfail(e, "hipSetDevice");
    // the id's entry of key_loc (written by the assign pass), then its bytes: two small copies behind
    // the work queued on the rules engine's stream
    uint64_t loc = ~0ull;
    if ((e = hipMemcpyAsync(&loc, P->d_key_loc.as<uint64_t>() + key_id, 8, hipMemcpyDeviceToHost, rules->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(rules->stream)) != hipSuccess)
        return rules->hipfail(e, "quota key text");
    if (loc == ~0ull) return rules->fail(MXP_ERR_ARG, "quota key text: no key with id " + std::to_string(key_id));
    const uint32_t n = (uint32_t)loc;
    *len = n;
    if (n > cap) return MXP_ERR_NOMEM;
    if (n && ((e = hipMemcpyAsync(buf, P->d_pool.as<uint8_t>() + (loc >> 32) * 8u, n, hipMemcpyDeviceToHost, rules->stream)) != hipSuccess ||
              (e = hipStreamSynchronize(rules->stream)) != hipSuccess))
        return rules->hipfail(e, "quota key text");
    return MXP_OK;
}

int mxp_quota_plan_stats(mxp_quota_plan* P, uint64_t* out, uint32_t cap) {
    if (!P || !out || cap < 4) return MXP_ERR_ARG;
    mxp_engine* rules = P->rules;
    hipError_t e;
    if ((e = hipSetDevice(rules->device)) != hipSuccess) return rules->hipfail(e, "hipSetDevice");
    if ((e = hipDeviceSynchronize()) != hipSuccess) return rules->hipfail(e, "quota plan stats");
    unsigned long long cnt[2];
    std::vector<uint32_t> next(P->n_cls);
    if ((e = hipMemcpy(cnt, P->d_count.p, 16, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(next.data(), P->d_cls_next.p, next.size() * 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return rules->hipfail(e, "quota plan stats");
    out[0] = cnt[0];
    out[1] = P->tslots;
    out[2] = cnt[1];
    out[3] = P->n_cls;
    for (uint32_t c = 0; c < P->n_cls && 4 + c < cap; c++) out[4 + c] = next[c];
    return MXP_OK;
}

}  // extern "C"
