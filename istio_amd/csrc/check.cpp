// check.cpp -- batched Check (include/mxp.h mxp_check_*): dispatcher.Check and combineResults
// (mixer/pkg/runtime/dispatcher.go:216-236, :322-361) down to the numbers grpcServer.Check answers
// with (mixer/pkg/api/grpcServer.go:160-179).  The semantics are stated in include/mxp.h and
// check.hip; this file is the pipeline:
//   1. the instance engine evaluates the batch once (Eval mode, result registers) on its stream, and
//      the list kernel runs once per distinct (value_rule, list, blacklist) into one plane of an
//      int32 [planes][n] array; an event marks the planes' completion;
//   2. the rules engine resolves the batch with the ids left on the device (mxp_resolve_kept:
//      resolver.cpp's stages, nothing delivered); status and err_rule come back as always;
//   3. the rules engine's stream waits for the event (no host synchronisation between the engines),
//      then the fold's count pass, the Resolve's scan kernels over the record counts, one download of
//      results and rec_off, and -- where records exist and fit -- the write pass and their download.
#include <cstring>
#include <map>
#include <tuple>

#include "check_args.h"
#include "engine_impl.h"
#include "lists.h"
#include "resolve_args.h"

extern "C" hipError_t mxp_launch_resolve(const mxp_resolve_args* a, int write, hipStream_t s);
extern "C" hipError_t mxp_launch_check(const mxp_check_args* a, int write, uint32_t group, int ids16, int wide,
                                       hipStream_t s);
extern "C" uint32_t mxp_check_group(uint64_t mean);

namespace {

constexpr int kResolveScan = 2;  // mxp_launch_resolve's scan of the counts (resolve.hip)

struct Unit {
    uint32_t kind = 0, value_rule = 0, plane = MXP_CHECK_NO_PLANE;
    int32_t code = 0;
    std::string message, handler;
};

struct Plane {
    uint32_t value_rule;
    const mxp_list* list;
    uint32_t blacklist;
    bool iface;
};

}  // namespace

struct mxp_check_plan {
    mxp_engine* rules = nullptr;
    mxp_engine* inst = nullptr;
    uint64_t rules_gen = 0, res_gen = 0, inst_gen = 0;  // the configurations the plan was made for
    std::vector<Unit> units;
    std::vector<Plane> planes;
    bool wide = false;  // a rule with more than 255 units (or 2^24 rules): the fold's 64-bit key
    int64_t def_dur = 0;
    int32_t def_use = 0;
    hipEvent_t planes_done = nullptr;
    DevBuf d_unit_off, d_entries;                               // the plan's tables
    DevBuf dm, de, dv, d_planes;                                // the instance evaluation, the code planes
    DevBuf d_rcount, d_bsum, d_recoff, d_results, d_recs;       // the fold's outputs
};

extern "C" {

int mxp_check_plan_create(mxp_engine* rules, mxp_engine* inst, const mxp_check_unit* units, uint32_t n_units,
                          const uint32_t* rule_unit_off, const uint32_t* rule_units, int64_t def_dur, int32_t def_use,
                          mxp_check_plan** out) {
    if (!rules || !out || (n_units && !units) || !rule_unit_off) return MXP_ERR_ARG;
    if (!rules->have_rules || !rules->resolver.set)
        return rules->fail(MXP_ERR_STATE, "check plan: the rules engine has no resolver configured");
    if (rules->device < 0) return rules->fail(MXP_ERR_STATE, "host-only engine");
    if (inst == rules) return rules->fail(MXP_ERR_ARG, "check plan: instance expressions belong in an engine of their own");
    if (inst && inst->device != rules->device)
        return rules->fail(MXP_ERR_ARG, "check plan: the two engines are on different devices");
    const uint32_t NR = (uint32_t)rules->rules.size();
    for (uint32_t r = 0; r < NR; r++)
        if (rule_unit_off[r + 1] < rule_unit_off[r])
            return rules->fail(MXP_ERR_ARG, "check plan: rule_unit_off[" + std::to_string(r + 1) + "] < rule_unit_off[" +
                                                std::to_string(r) + "]");
    const uint32_t n_ent = rule_unit_off[NR];
    if (n_ent && !rule_units) return MXP_ERR_ARG;
    for (uint32_t i = rule_unit_off[0]; i < n_ent; i++)
        if (rule_units[i] >= n_units)
            return rules->fail(MXP_ERR_ARG, "check plan: rule_units[" + std::to_string(i) + "] = " +
                                                std::to_string(rule_units[i]) + " is not a unit (" + std::to_string(n_units) + ")");
    std::unique_ptr<mxp_check_plan> P(new mxp_check_plan());
    P->rules = rules;
    P->inst = inst;
    P->def_dur = def_dur;
    P->def_use = def_use;
    std::map<std::tuple<uint32_t, const mxp_list*, uint32_t>, uint32_t> plane_of;
    for (uint32_t i = 0; i < n_units; i++) {
        const mxp_check_unit& u = units[i];
        const std::string at = "check plan: unit " + std::to_string(i) + ": ";
        Unit U;
        U.kind = u.kind;
        U.handler = u.handler_name ? u.handler_name : "";
        if (u.kind == MXP_CHECK_UNIT_CONST) {
            if (u.const_code < 0) return rules->fail(MXP_ERR_ARG, at + "a negative code");
            U.code = u.const_code;
            U.message = u.const_message ? u.const_message : "";
        } else if (u.kind == MXP_CHECK_UNIT_LIST) {
            if (!inst || !inst->have_rules) return rules->fail(MXP_ERR_ARG, at + "a list unit without an instance engine");
            if (!u.list) return rules->fail(MXP_ERR_ARG, at + "no list");
            if (u.value_rule >= inst->rules.size()) return rules->fail(MXP_ERR_ARG, at + "no such value rule");
            const auto& R = inst->rules[u.value_rule];
            const bool iface = R.il_ret == mxp::IL_INTERFACE;
            if (R.status == MXP_RULE_OK && R.il_ret != mxp::IL_STRING && !iface)
                return rules->fail(MXP_ERR_ARG, at + "the value expression is not of type STRING");
            U.value_rule = u.value_rule;
            const auto key = std::make_tuple(u.value_rule, u.list, u.blacklist ? 1u : 0u);
            auto it = plane_of.find(key);
            if (it == plane_of.end()) {
                it = plane_of.emplace(key, (uint32_t)P->planes.size()).first;
                P->planes.push_back(Plane{u.value_rule, u.list, u.blacklist ? 1u : 0u, iface});
            }
            U.plane = it->second;
        } else {
            return rules->fail(MXP_ERR_ARG, at + "unknown kind");
        }
        P->units.push_back(std::move(U));
    }
    std::vector<mxp_check_entry> ent(n_ent);
    memset(ent.data(), 0, ent.size() * sizeof(mxp_check_entry));
    for (uint32_t i = rule_unit_off[0]; i < n_ent; i++) {
        const mxp_check_unit& u = units[rule_units[i]];
        const Unit& U = P->units[rule_units[i]];
        ent[i].dur = u.valid_duration_ns;
        ent[i].use = u.valid_use_count;
        ent[i].code = U.code;
        ent[i].plane = U.plane;
        ent[i].value_rule = U.value_rule;
        ent[i].unit = rule_units[i];
    }
    P->wide = NR > (1u << 24);  // (the 32-bit key: 24 bits of position, 8 of unit index)
    for (uint32_t r = 0; r < NR; r++) P->wide |= rule_unit_off[r + 1] - rule_unit_off[r] > 255u;
    hipError_t e;
    if ((e = hipSetDevice(rules->device)) != hipSuccess) return rules->hipfail(e, "hipSetDevice");
    if ((e = P->d_unit_off.alloc(((size_t)NR + 1) * 4)) != hipSuccess ||
        (e = hipMemcpy(P->d_unit_off.p, rule_unit_off, ((size_t)NR + 1) * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = P->d_entries.alloc(ent.size() * sizeof(mxp_check_entry))) != hipSuccess ||
        (n_ent && (e = hipMemcpy(P->d_entries.p, ent.data(), ent.size() * sizeof(mxp_check_entry),
                                 hipMemcpyHostToDevice)) != hipSuccess) ||
        (e = hipEventCreateWithFlags(&P->planes_done, hipEventDisableTiming)) != hipSuccess)
        return rules->hipfail(e, "check plan tables");
    P->rules_gen = rules->rules_gen;
    P->res_gen = rules->res_gen;
    P->inst_gen = inst ? inst->rules_gen : 0;
    *out = P.release();
    return MXP_OK;
}

void mxp_check_plan_destroy(mxp_check_plan* plan) {
    if (!plan) return;
    if (plan->rules && plan->rules->device >= 0) (void)hipSetDevice(plan->rules->device);
    if (plan->planes_done) (void)hipEventDestroy(plan->planes_done);
    delete plan;
}

int mxp_check_batch(mxp_check_plan* P, const mxp_bag_batch* batch, uint32_t variety, uint8_t* status, uint32_t* err_rule,
                    mxp_check_result* results, uint64_t* rec_off, mxp_check_record* recs, uint64_t rec_cap) {
    if (!P || !batch || !rec_off || (batch->n_requests && (!status || !err_rule || !results)) || (rec_cap && !recs) ||
        variety >= 32)
        return MXP_ERR_ARG;
    mxp_engine *rules = P->rules, *inst = P->inst;
    if (rules->rules_gen != P->rules_gen || rules->res_gen != P->res_gen || (inst && inst->rules_gen != P->inst_gen))
        return rules->fail(MXP_ERR_ARG, "check: a rule set was compiled (or a resolver set) after the plan was created");
    const uint32_t n = batch->n_requests;
    const uint32_t NR = (uint32_t)rules->rules.size();
    uint8_t no_status = 0;  // (an empty batch: the Resolve still takes its two pointers)
    uint32_t no_rule = 0;
    if (!n && !status) status = &no_status;
    if (!n && !err_rule) err_rule = &no_rule;
    const char* e32 = getenv("MXP_CHECK_IDS32");
    const bool ids16 = NR <= 65536u && !(e32 && atoi(e32) != 0);
    hipError_t e;
    int rc;
    if ((e = hipSetDevice(rules->device)) != hipSuccess) return rules->hipfail(e, "hipSetDevice");
    // 1. the code planes, on the instance engine's stream
    std::unique_ptr<mxp_dbatch> idb;
    // (the instance evaluation awaited, its error texts fetched, the batch kept as that engine's last:
    // every return after the evaluation goes through here)
    auto inst_done = [&](int ret) -> int {
        if (!idb) return ret;
        const int r2 = inst->collect_errors(batch, idb);
        if (r2 && !ret) rules->last_error = inst->last_error;
        return ret ? ret : r2;
    };
    if (!P->planes.empty()) {
        const bool saved = inst->need_strings;
        inst->need_strings = true;  // (the symbols are read from the batch's string pool)
        rc = inst->evaluate(batch, P->dm, P->de, &P->dv, idb);
        inst->need_strings = saved;
        if (rc) {
            rules->last_error = inst->last_error;
            idb.reset();
            return rc;
        }
        if (n) {
            if ((e = P->d_planes.reserve(P->planes.size() * (size_t)n * 4)) != hipSuccess)
                return inst_done(rules->hipfail(e, "alloc code planes"));
            for (size_t p = 0; p < P->planes.size(); p++) {
                const Plane& pl = P->planes[p];
                mxp_list_args A;
                mxp_list_fill_args(&A, pl.list, (int)pl.blacklist, n, P->d_planes.as<int32_t>() + p * (size_t)n);
                mxp_list_fill_value(&A, inst, idb.get(), P->dv.as<uint64_t>(), P->de.as<uint32_t>(), pl.value_rule, pl.iface);
                if ((rc = mxp_list_launch(inst, &A, inst->stream, "launch check plane"))) {
                    rules->last_error = inst->last_error;
                    return inst_done(rc);
                }
            }
            if ((e = hipEventRecord(P->planes_done, inst->stream)) != hipSuccess)
                return inst_done(rules->hipfail(e, "record planes event"));
        }
    }
    // 2. the Resolve, ids kept on the device
    uint64_t n_ids = 0;
    if ((rc = mxp_resolve_kept(rules, batch, variety, ids16, status, err_rule, &n_ids))) return inst_done(rc);
    if (!n) {
        rec_off[0] = 0;
        return inst_done(MXP_OK);
    }
    // 3. the fold
    const size_t grid = ((size_t)n + 255u) / 256u;
    if ((e = P->d_rcount.reserve((size_t)n * 4)) != hipSuccess || (e = P->d_bsum.reserve(grid * 8 + 8)) != hipSuccess ||
        (e = P->d_recoff.reserve(((size_t)n + 1) * 8)) != hipSuccess ||
        (e = P->d_results.reserve((size_t)n * sizeof(mxp_check_result))) != hipSuccess)
        return inst_done(rules->hipfail(e, "alloc check outputs"));
    if (!P->planes.empty() && (e = hipStreamWaitEvent(rules->stream, P->planes_done, 0)) != hipSuccess)
        return inst_done(rules->hipfail(e, "wait for the code planes"));
    mxp_check_args C;
    memset(&C, 0, sizeof C);
    C.n = n;
    C.vstride = inst ? (uint32_t)inst->rules.size() : 0u;
    C.ids = rules->res_sel.p;
    C.id_off = rules->res_off.as<uint64_t>();
    C.status = rules->res_status.as<uint8_t>();
    C.rule_unit_off = P->d_unit_off.as<uint32_t>();
    C.entries = P->d_entries.as<mxp_check_entry>();
    C.planes = P->d_planes.as<int32_t>();
    C.vals = P->dv.as<uint64_t>();
    C.rcount = P->d_rcount.as<uint32_t>();
    C.block_sum = P->d_bsum.as<uint64_t>();
    C.rec_off = P->d_recoff.as<uint64_t>();
    C.results = P->d_results.p;
    C.def_dur = P->def_dur;
    C.def_use = P->def_use;
    const uint32_t group = mxp_check_group((n_ids + n - 1) / n);
    mxp_resolve_args S;  // the Resolve's scan kernels over the record counts
    memset(&S, 0, sizeof S);
    S.n = n;
    S.count = C.rcount;
    S.block_sum = C.block_sum;
    S.sel_off_out = P->d_recoff.as<uint64_t>();
    if ((e = mxp_launch_check(&C, 0, group, ids16, P->wide, rules->stream)) != hipSuccess ||
        (e = mxp_launch_resolve(&S, kResolveScan, rules->stream)) != hipSuccess)
        return inst_done(rules->hipfail(e, "launch check fold"));
    if ((rc = rules->download_all({{results, P->d_results.p, (size_t)n * sizeof(mxp_check_result)},
                                   {rec_off, P->d_recoff.p, ((size_t)n + 1) * 8}},
                                  "download check results")))
        return inst_done(rc);
    const uint64_t total = rec_off[n];
    if (total > rec_cap) return inst_done(MXP_ERR_NOMEM);
    if (total) {
        if ((e = P->d_recs.reserve(total * sizeof(mxp_check_record))) != hipSuccess)
            return inst_done(rules->hipfail(e, "alloc check records"));
        C.recs = P->d_recs.p;
        if ((e = mxp_launch_check(&C, 1, group, ids16, P->wide, rules->stream)) != hipSuccess)
            return inst_done(rules->hipfail(e, "launch check records"));
        if ((rc = rules->download(recs, P->d_recs.p, total * sizeof(mxp_check_record), "download check records")))
            return inst_done(rc);
    }
    return inst_done(MXP_OK);
}

int mxp_check_message(mxp_check_plan* P, const mxp_check_record* recs, uint32_t n, char* buf, uint32_t cap) {
    if (!P || (n && !recs) || !buf || !cap) return MXP_ERR_ARG;
    std::string out;
    bool first = true;
    std::vector<char> tmp(1u << 16);
    for (uint32_t i = 0; i < n; i++) {
        const mxp_check_record& r = recs[i];
        if (r.code <= 0) continue;
        if (r.unit >= P->units.size()) return P->rules->fail(MXP_ERR_ARG, "check message: no such unit");
        const Unit& U = P->units[r.unit];
        std::string msg;
        if (U.kind == MXP_CHECK_UNIT_CONST) {
            msg = U.message;
        } else {
            if (int rc = mxp_value_text(P->inst, U.value_rule, r.value, tmp.data(), (uint32_t)tmp.size())) return rc;
            const std::string sym = tmp.data();
            msg = sym + (r.code == MXP_RPC_NOT_FOUND           ? " is not whitelisted"
                         : r.code == MXP_RPC_PERMISSION_DENIED ? " is blacklisted"
                                                               : " is not a valid IP address");
        }
        if (!first) out += ", ";
        first = false;
        out += U.handler + ":" + msg;
    }
    const size_t k = std::min<size_t>(out.size(), cap - 1);
    memcpy(buf, out.data(), k);
    buf[k] = 0;
    return out.size() >= cap ? MXP_ERR_NOMEM : MXP_OK;
}

}  // extern "C"
