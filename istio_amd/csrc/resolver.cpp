// resolver.cpp -- batched runtime.resolver on top of the predicate bitmaps (include/mxp.h,
// resolve.hip).
//
// Reference: resolver.Resolve (mixer/pkg/runtime/resolver.go:110-168), destAndNamespace
// (:180-199), filterActions (:202-238).  The host derives each request's namespace and TCP flag
// from its bag exactly as destAndNamespace / filterActions do; the GPU walks the namespace rule
// ranges over the bitmaps mxp_eval_kernel / mxp_index_kernel produced.
#include <cstddef>
#include <cstring>
#include <numeric>
#include <string_view>

#include "delta8_args.h"
#include "engine_impl.h"
#include "pack_args.h"
#include "resolve_args.h"

extern "C" hipError_t mxp_launch_resolve(const mxp_resolve_args* a, int write, hipStream_t s);
extern "C" hipError_t mxp_launch_d8(const mxp_d8_args* a, int write, uint32_t group, hipStream_t s);
extern "C" uint32_t mxp_d8_group(uint64_t mean);
extern "C" hipError_t mxp_launch_ns(const mxp_ns_args* a, hipStream_t s);
extern "C" hipError_t mxp_launch_resolve_scatter(const uint32_t* pairs, uint32_t m, uint32_t* err_in, hipStream_t s);
extern "C" hipError_t mxp_launch_resolve_first_err(const mxp_resolve_args* a, const void* recs, uint32_t m, hipStream_t s);

namespace {

const char* const kProtocolAttr = "context.protocol";  // ContextProtocolAttributeName (resolver.go:95)

// namespace info of every request: destAndNamespace + the tcp flag of filterActions (parallel over
// requests; namespace names looked up as string views)
int request_info(mxp_engine* eng, const mxp_bag_batch* b, std::vector<uint32_t>* info) {
    const auto& R = eng->resolver;
    const uint32_t n = b->n_requests;
    int idc = -1, pc = -1;
    for (uint32_t c = 0; c < b->n_columns; c++) {
        if (R.identity == b->column_names[c]) idc = (int)c;
        if (strcmp(kProtocolAttr, b->column_names[c]) == 0) pc = (int)c;
    }
    std::unordered_map<std::string_view, uint32_t> ns_ids;
    for (const auto& kv : R.ns_ids) ns_ids.emplace(std::string_view(kv.first), kv.second);
    auto str = [&](uint64_t sid) {
        return std::string_view((const char*)b->str_bytes + b->str_offsets[sid],
                                (size_t)(b->str_offsets[sid + 1] - b->str_offsets[sid]));
    };
    info->resize(n);
    uint32_t* out = info->data();
    mxp::par_for(n, 16384, [&](uint64_t q0, uint64_t q1, unsigned) {
        for (uint64_t q = q0; q < q1; q++) {
            // attrs.Get(idAttr): nil -> "identity not found"; not a string -> "identity must be string"
            if (idc < 0 || b->kinds[idc][q] == MXP_ABSENT) {
                out[q] = MXP_NS_MISSING;
                continue;
            }
            if (b->kinds[idc][q] != MXP_STRING) {
                out[q] = MXP_NS_NOTSTRING;
                continue;
            }
            const std::string_view d = str(b->values[idc][q]);
            // strings.SplitN(dest, ".", 3): ns = splits[1] when there is at least one '.'
            std::string_view ns;
            const size_t dot1 = d.find('.');
            if (dot1 != std::string_view::npos) {
                const std::string_view rest = d.substr(dot1 + 1);
                ns = rest.substr(0, rest.find('.'));
            }
            auto it = ns_ids.find(ns);
            const uint32_t v = it == ns_ids.end() ? MXP_NS_NONE : it->second;
            // tcp := attrs.Get("context.protocol") == "tcp": an interface compare, so only a string
            const bool tcp = pc >= 0 && b->kinds[pc][q] == MXP_STRING && str(b->values[pc][q]) == "tcp";
            out[q] = v | (tcp ? 0x80000000u : 0u);
        }
    });
    return MXP_OK;
}

}  // namespace

extern "C" {

int mxp_resolver_set(mxp_engine* eng, const char* identity_attr, const char* default_ns, const char* const* rule_ns,
                     const uint32_t* variety_mask, const uint8_t* is_tcp, const uint8_t* empty_match, uint32_t n) {
    if (!eng || !identity_attr || !default_ns || (n && (!rule_ns || !variety_mask || !is_tcp || !empty_match)))
        return MXP_ERR_ARG;
    if (!eng->have_rules) return eng->fail(MXP_ERR_STATE, "no rule set compiled");
    if (n != eng->rules.size()) return eng->fail(MXP_ERR_ARG, "resolver: rule count differs from the rule set");
    mxp_engine::ResolverConf R;
    R.identity = identity_attr;
    R.default_ns = default_ns;
    // the attributes every Resolve reads get their vocabulary positions now (the finder is asked
    // here, at snapshot time, never on the evaluation path: refs.cpp uses vocab_find)
    (void)eng->vocab_pos(R.identity);
    (void)eng->vocab_pos("context.protocol");
    R.vmask.assign(variety_mask, variety_mask + n);
    R.tcp.assign(is_tcp, is_tcp + n);
    R.empty.assign(empty_match, empty_match + n);
    for (uint32_t i = 0; i < n; i++) {
        const std::string ns = rule_ns[i] ? rule_ns[i] : "";
        auto it = R.ns_ids.find(ns);
        if (it == R.ns_ids.end()) {
            const uint32_t id = (uint32_t)R.ns_names.size();
            if (id >= MXP_NS_NONE) return eng->fail(MXP_ERR_ARG, "resolver: too many namespaces");
            R.ns_ids.emplace(ns, id);
            R.ns_names.push_back(ns);
            R.ns_lo.push_back(i);
            R.ns_hi.push_back(i + 1);
        } else if (R.ns_hi[it->second] != i) {
            return eng->fail(MXP_ERR_ARG, "resolver: rules of namespace '" + ns + "' are not contiguous");
        } else {
            R.ns_hi[it->second] = i + 1;
        }
    }
    auto d = R.ns_ids.find(R.default_ns);
    R.default_id = d == R.ns_ids.end() ? MXP_NS_NONE : d->second;
    R.set = true;
    eng->res_gen++;  // (the device tables of the previous configuration are stale)
    // the namespace names on the device (mxp_ns_kernel): content-hash table, descriptors, bytes
    if (eng->device >= 0) {
        hipError_t e;
        if ((e = hipSetDevice(eng->device)) != hipSuccess) return eng->hipfail(e, "hipSetDevice");
        uint32_t cap = 64;
        while (cap < 2 * R.ns_names.size()) cap <<= 1;
        std::vector<unsigned long long> tab(cap, 0ull);
        std::vector<uint64_t> desc;
        std::string blob;
        for (uint32_t id = 0; id < R.ns_names.size(); id++) {
            const std::string& nm = R.ns_names[id];
            desc.push_back(((uint64_t)blob.size() << 24) | nm.size());
            blob += nm;
            const uint64_t h = mxp_item_hash((const uint8_t*)nm.data(), (uint32_t)nm.size());
            uint32_t slot = (uint32_t)h & (cap - 1);
            while (tab[slot]) slot = (slot + 1) & (cap - 1);
            tab[slot] = ((h >> 32) << 32) | (id + 1ull);
        }
        blob.append(16, '\0');
        desc.push_back(0);
        auto put = [&](DevBuf& b, const void* src, size_t bytes) -> int {
            if ((e = b.alloc(bytes)) != hipSuccess || (e = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice)) != hipSuccess)
                return eng->hipfail(e, "resolver namespaces");
            return MXP_OK;
        };
        int rc;
        if ((rc = put(eng->res_ns_tab, tab.data(), tab.size() * 8)) || (rc = put(eng->res_ns_desc, desc.data(), desc.size() * 8)) ||
            (rc = put(eng->res_ns_blob, blob.data(), blob.size())))
            return rc;
        eng->res_ns_mask = cap - 1;
    }
    eng->resolver = std::move(R);
    return MXP_OK;
}

}  // extern "C"

namespace {

// (MXP_DBG_RESOLVE_BITMAP: resolve through the error bitmap, the pre-round-5 path, for A/B and tests)
// ids enqueued with the other outputs only for capacities up to this many bytes (the device buffer
// is sized by the capacity, not the count)
constexpr uint64_t kEarlyIdsMax = 256ull << 20;

// Each request's first applicable erroring rule in resolution order (filterActions returns at the
// first EvalPredicate error, resolver.go:226-228) from the error records of a compact evaluation:
// (request, rule) pairs for the requests that fail.  hinfo: the requests' namespace info.
void first_errors(mxp_engine* eng, uint32_t n, uint32_t variety, const uint32_t* hinfo, std::vector<uint32_t>* pairs) {
    const auto& R = eng->resolver;
    std::vector<uint32_t>& best = eng->res_best;  // (kept all ~0 between calls)
    if (best.size() < n) best.assign(n, 0xFFFFFFFFu);
    const bool has_def = R.default_id != MXP_NS_NONE;
    const uint32_t dlo = has_def ? R.ns_lo[R.default_id] : 0u, dhi = has_def ? R.ns_hi[R.default_id] : 0u;
    const uint32_t dlen = dhi - dlo;
    std::vector<uint32_t> touched;
    (void)eng->ensure_recs();  // (class records make collect_errors download them at once; kept for safety)
    for (const mxp_err_rec& rec : eng->last_recs) {
        const uint32_t q = rec.req, r = rec.rule;
        if (q >= n || r >= R.vmask.size()) continue;
        const uint32_t info = hinfo[q];
        if (info == MXP_NS_MISSING || info == MXP_NS_NOTSTRING) continue;
        const uint32_t tcp = info >> 31, ns = info & 0x7FFFFFFFu;
        if (R.empty[r] || !((R.vmask[r] >> variety) & 1u) || R.tcp[r] != tcp) continue;
        uint32_t rank;
        if (has_def && r >= dlo && r < dhi) {
            rank = r - dlo;
        } else if (ns != MXP_NS_NONE && ns != R.default_id && r >= R.ns_lo[ns] && r < R.ns_hi[ns]) {
            rank = dlen + (r - R.ns_lo[ns]);
        } else {
            continue;
        }
        if (best[q] == 0xFFFFFFFFu) touched.push_back(q);
        if (rank < best[q]) best[q] = rank;
    }
    pairs->clear();
    pairs->reserve(2 * touched.size());
    for (uint32_t q : touched) {
        const uint32_t rank = best[q];
        const uint32_t ns = hinfo[q] & 0x7FFFFFFFu;
        pairs->push_back(q);
        pairs->push_back(rank < dlen ? dlo + rank : R.ns_lo[ns] + (rank - dlen));
        best[q] = 0xFFFFFFFFu;
    }
}

}  // namespace

// A Resolve in two phases (resolve_impl runs both; mxp_resolve_submit / _finish let a caller work
// between them): begin enqueues the evaluation and the request namespaces and returns without
// waiting for the device; end waits, finds the first errors, counts, places and downloads.
struct mxp_resolve_job {
    mxp_engine* eng = nullptr;
    const mxp_bag_batch* batch = nullptr;
    uint32_t variety = 0;
    ResIds ids = ResIds::U32;  // the action lists' format
    bool compact = false;
    uint32_t n = 0, W = 0;
    uint64_t* ref_off = nullptr;
    mxp_attr_ref* refs = nullptr;
    uint64_t ref_cap = 0;
    std::unique_ptr<mxp_dbatch> db;
    std::vector<mxp_ref_rec> recs;
    std::vector<uint32_t> info;  // host copy of the namespaces (host pass; referenced attributes)
    const uint32_t* hinfo = nullptr;
    mxp_engine::PairView pairs;  // the evaluation's filed pairs (pair Resolve; on = false: the bitmap)
    bool pairs_filed = false;    // (the evaluation filed them; pairs_ovf: how many overflowed)
    uint32_t pairs_ovf = 0;
    uint32_t recs_n = 0, class_recs_n = 0;  // (the evaluation's error records: diagnostics)
    // a group member whose ids go first in the batch's list (member 0): the group's capacity, so its
    // ids are enqueued with the other outputs, before the placement (0: after it)
    uint64_t first_cap = 0;
};

namespace {

// mxp_launch_resolve's passes (the table above it in resolve.hip)
enum ResPass : int { kCount = 0, kWrite = 1, kScan = 2, kTileCount = 3, kTileWrite = 4, kPairsCount = 5, kPairsWrite = 6 };

// eng->res_small by field: the pinned 64-byte block a Resolve's small counts are downloaded into
struct ResSmall {
    uint32_t err_cnt[4];    // a compact Resolve's d_errcount: [0] records, [2] class records
    uint32_t pairs_ovf[2];  // ... and the pairs past their lists / slots
    uint32_t unused[2];
    uint64_t ids_total;     // a delta8 Resolve's id count (its sel_off counts bytes)
};
static_assert(offsetof(ResSmall, ids_total) == 32 && sizeof(ResSmall) <= 64, "res_small as engine_impl.h describes it");

int res_small(mxp_engine* eng, ResSmall** out) {
    hipError_t e;
    if (!eng->res_small && (e = hipHostMalloc((void**)&eng->res_small, 64, hipHostMallocDefault)) != hipSuccess) {
        eng->res_small = nullptr;
        return eng->hipfail(e, "pinned counters");
    }
    *out = reinterpret_cast<ResSmall*>(eng->res_small);
    return MXP_OK;
}

// src into d (grown to hold it) on the engine's stream
int upload(mxp_engine* eng, DevBuf& d, const void* src, size_t bytes, const char* what) {
    hipError_t e;
    if ((e = d.reserve(bytes)) != hipSuccess) return eng->hipfail(e, what);
    if (bytes && (e = hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, eng->stream)) != hipSuccess)
        return eng->hipfail(e, what);
    return MXP_OK;
}

int resolve_begin(mxp_resolve_job& J) {
    mxp_engine* eng = J.eng;
    const mxp_bag_batch* batch = J.batch;
    mxp_dbatch* pre = J.db.get();
    if (pre && (J.ref_off || pre->n != batch->n_requests))
        return eng->fail(MXP_ERR_ARG, "resolve: the uploaded batch is not this batch");
    if (pre && eng->device >= 0 && hipSetDevice(eng->device) != hipSuccess) return eng->fail(MXP_ERR_DEVICE, "hipSetDevice");
    if (!eng->resolver.set) return eng->fail(MXP_ERR_STATE, "resolver not configured (mxp_resolver_set)");
    const auto& R = eng->resolver;
    const uint32_t n = J.n = batch->n_requests;
    const uint32_t NR = (uint32_t)eng->rules.size();
    const uint32_t W = J.W = (NR + 31) / 32;
    if (J.ids != ResIds::U32 && NR > 65536u)
        return eng->fail(MXP_ERR_ARG, J.ids == ResIds::U16 ? "u16 rule ids: more than 65536 rules"
                                                            : "delta8 rule ids: more than 65536 rules");
    DevBuf& dm = eng->res_dm;  // (engine-owned scratch: no allocation per call once large enough)
    DevBuf& de = eng->res_de;
    hipError_t e;
    int rc;
    // the resolver's tables first, before the evaluation is queued: a copy from pageable memory
    // returns only once the stream has reached it, so behind the evaluation it would hold the
    // caller until the kernels end (r6_s25: 0.79 ms)
    // (kept on the device while the configuration and variety stay: four pageable copies a call,
    // ~0.1 ms of the caller's time, before)
    DevBuf& d_info = eng->res_info;
    const uint64_t tab_key = eng->res_gen << 6 | J.variety;
    if (eng->res_tab_key != tab_key) {
        std::vector<uint32_t> amask(2 * (size_t)W, 0), empty(W, 0);  // per-word masks: variety / tcp, empty matches
        bool any_empty = false;
        for (uint32_t r = 0; r < NR; r++) {
            const uint32_t bit = 1u << (r & 31);
            if ((R.vmask[r] >> J.variety) & 1u) amask[(size_t)R.tcp[r] * W + r / 32] |= bit;
            if (R.empty[r]) {
                empty[r / 32] |= bit;
                any_empty = true;
            }
        }
        eng->res_tab_key = ~0ull;  // (until every table is up)
        if ((rc = upload(eng, eng->res_lo, R.ns_lo.data(), R.ns_lo.size() * 4, "upload ns_lo"))) return rc;
        if ((rc = upload(eng, eng->res_hi, R.ns_hi.data(), R.ns_hi.size() * 4, "upload ns_hi"))) return rc;
        if ((rc = upload(eng, eng->res_amask, amask.data(), amask.size() * 4, "upload amask"))) return rc;
        if ((rc = upload(eng, eng->res_empty, empty.data(), empty.size() * 4, "upload empty"))) return rc;
        eng->res_tab_key = tab_key;
        eng->res_any_empty = any_empty;
    }
    J.compact = !J.ref_off && !(eng->debug_flags & MXP_DBG_RESOLVE_BITMAP);
    if (J.compact) {
        if (eng->device >= 0 && (e = eng->res_flags.reserve(n ? n : 1)) != hipSuccess) return eng->hipfail(e, "alloc flags");
        // pair Resolve: the selected rules from the evaluation's deferred pairs, the bitmap left
        // unwritten, where the plan allows it (the launch decides); rules with an empty match are
        // selected without a pair, so their sets keep the bitmap
        eng->pair_req = eng->resolve_pairs != 0 && !eng->res_any_empty;
        if (pre) {
            rc = eng->evaluate_uploaded(J.db.get(), dm, de, nullptr, eng->res_flags.as<uint8_t>());
        } else {
            rc = eng->evaluate(batch, dm, de, nullptr, J.db, eng->res_flags.as<uint8_t>());
        }
        J.pairs = eng->pair_req && !rc ? eng->last_pairs : mxp_engine::PairView{};
        J.pairs_filed = J.pairs.on;
        eng->pair_req = false;
    } else {
        rc = J.ref_off ? eng->refs_evaluate(batch, dm, de, J.db, J.recs)
             : pre     ? eng->evaluate_uploaded(J.db.get(), dm, de, nullptr, nullptr)
                       : eng->evaluate(batch, dm, de, nullptr, J.db);
    }
    if (rc) return rc;
    // request namespaces: on the device from the batch as uploaded (pack_device), else on the host
    mxp_dbatch* db = J.db.get();
    if (db->res_raw && !J.ref_off) {
        if ((e = d_info.reserve((size_t)n * 4 + 4)) != hipSuccess) return eng->hipfail(e, "alloc nsinfo");
        mxp_ns_args N;
        memset(&N, 0, sizeof N);
        N.n = n;
        N.ns_mask = eng->res_ns_mask;
        N.id_kind = db->res_id_kind;
        N.id_val = db->res_id_val;
        N.pr_kind = db->res_pr_kind;
        N.pr_val = db->res_pr_val;
        N.soff = db->pk.pk_soff.as<uint64_t>();
        N.sbytes = db->pk.pk_sbytes.as<uint8_t>();
        N.ns_tab = eng->res_ns_tab.as<unsigned long long>();
        N.ns_desc = eng->res_ns_desc.as<uint64_t>();
        N.ns_blob = eng->res_ns_blob.as<uint8_t>();
        N.nsinfo = d_info.as<uint32_t>();
        if (n && (e = mxp_launch_ns(&N, eng->stream)) != hipSuccess) return eng->hipfail(e, "launch namespaces");
        eng->trace_mark("request namespaces (device)");
    } else {
        if (db->wide && batch == &db->wide->view) db->wide->materialize();  // (a narrow upload)
        request_info(eng, batch, &J.info);
        J.hinfo = J.info.data();
        eng->trace_mark("request namespaces (host)");
        if ((rc = upload(eng, d_info, J.info.data(), J.info.size() * 4, "upload nsinfo"))) return rc;
    }
    return MXP_OK;
}

// ---- resolve_end's stages, in the order its driver (below them) runs them

// The resolve kernels' argument block over the engine's scratch, grown to this batch.
int resolve_args(mxp_resolve_job& J, mxp_resolve_args* out) {
    mxp_engine* eng = J.eng;
    const size_t n = J.n, grid = (J.n + 255u) / 256u;
    hipError_t e;
    if ((e = eng->res_status.reserve(n)) != hipSuccess) return eng->hipfail(e, "alloc status");
    if ((e = eng->res_err_rule.reserve(n * 4)) != hipSuccess) return eng->hipfail(e, "alloc err_rule");
    if ((e = eng->res_count.reserve(n * 4)) != hipSuccess) return eng->hipfail(e, "alloc count");
    if ((e = eng->res_bsum.reserve(grid * 8 + 8)) != hipSuccess) return eng->hipfail(e, "alloc block sums");
    if ((e = eng->res_off.reserve((n + 1) * 8)) != hipSuccess) return eng->hipfail(e, "alloc sel_off");
    if ((e = eng->res_stash.reserve(n * 16 + 16)) != hipSuccess) return eng->hipfail(e, "alloc stash");
    mxp_resolve_args& A = *out;
    memset(&A, 0, sizeof A);
    A.n = J.n;
    A.n_words = J.W;
    A.nsinfo = eng->res_info.as<uint32_t>();
    A.ns_lo = eng->res_lo.as<uint32_t>();
    A.ns_hi = eng->res_hi.as<uint32_t>();
    A.default_id = eng->resolver.default_id;
    A.amask = eng->res_amask.as<uint32_t>();
    A.empty = eng->res_empty.as<uint32_t>();
    A.match = eng->res_dm.as<uint32_t>();
    A.err = J.compact ? nullptr : eng->res_de.as<uint32_t>();
    A.status = eng->res_status.as<uint8_t>();
    A.err_rule = eng->res_err_rule.as<uint32_t>();
    A.count = eng->res_count.as<uint32_t>();
    A.block_sum = eng->res_bsum.as<uint64_t>();
    A.sel_off_out = eng->res_off.as<uint64_t>();
    A.sel_off = eng->res_off.as<uint64_t>();
    A.ids16 = J.ids != ResIds::U32 ? 1u : 0u;
    A.stash = (uint4*)eng->res_stash.p;
    return MXP_OK;
}

// Error triage of a compact evaluation: where the resolve kernels find each request's first error.
// Waits for the evaluation (the log's counts come back), then one of three: records past the log's
// capacity -- the error bitmap after all (A.err); records only -- first errors on the device
// (A.err_in, A.err_rank); class records -- expanded and ranked on the host (A.err_in; *collected).
// J.pairs.on is cleared wherever the evaluation ended up writing the bitmaps.
int triage_errors(mxp_resolve_job& J, mxp_resolve_args& A, bool* collected) {
    mxp_engine* eng = J.eng;
    const uint32_t n = J.n;
    DevBuf &dm = eng->res_dm, &de = eng->res_de;
    hipError_t e;
    int rc;
    ResSmall* hs;
    if ((rc = res_small(eng, &hs))) return rc;
    // (into pinned memory: both copies queued, one synchronisation)
    hs->pairs_ovf[0] = hs->pairs_ovf[1] = 0;
    if ((e = hipMemcpyAsync(hs->err_cnt, eng->d_errcount.p, 16, hipMemcpyDeviceToHost, eng->stream)) != hipSuccess ||
        (J.pairs.on &&
         (e = hipMemcpyAsync(hs->pairs_ovf, J.pairs.ovf_n, 8, hipMemcpyDeviceToHost, eng->stream)) != hipSuccess) ||
        (e = hipStreamSynchronize(eng->stream)) != hipSuccess)
        return eng->hipfail(e, "download errcount");
    const uint32_t n_recs = hs->err_cnt[0], n_class = hs->err_cnt[2];
    // (pairs past their lists or slots: the fills stored the bitmap after all -- read it)
    J.pairs_ovf = hs->pairs_ovf[0];
    J.recs_n = n_recs;
    J.class_recs_n = n_class;
    if (J.pairs_ovf) J.pairs.on = false;
    if ((e = eng->res_err_in.reserve((size_t)n * 4 + 4)) != hipSuccess) return eng->hipfail(e, "alloc err_in");
    if (n && (e = hipMemsetAsync(eng->res_err_in.p, 0xFF, (size_t)n * 4, eng->stream)) != hipSuccess)
        return eng->hipfail(e, "reset err_in");
    // (an evaluation without a log: it writes both bitmaps)
    auto error_bitmap = [&](mxp_dbatch* db) -> int {
        if ((e = de.reserve((size_t)J.W * n * 4)) != hipSuccess) return eng->hipfail(e, "alloc err");
        if (int r = eng->launch(db, eng->stream, dm.as<uint32_t>(), de.as<uint32_t>(), nullptr, false)) return r;
        A.err = de.as<uint32_t>();
        J.pairs.on = false;
        return MXP_OK;
    };
    if (n_recs > eng->errcap) {
        // records past the log's capacity: the error bitmap after all
        if ((rc = error_bitmap(J.db.get()))) return rc;
        eng->trace_mark("error bitmap (log overflow)");
    } else if (!n_class) {
        // each request's first error from the records, on the device
        A.err_in = eng->res_err_in.as<uint32_t>();
        A.err_rank = 1u;
        if ((e = mxp_launch_resolve_first_err(&A, eng->d_errlog.p, n_recs, eng->stream)) != hipSuccess)
            return eng->hipfail(e, "launch first errors");
        eng->trace_mark("first errors (device)");
    } else {
        // value-class records stand for whole classes: expanded per request on the host
        // (collect_errors), then the first error of each failing request found there
        if ((rc = eng->collect_errors(J.batch, J.db))) return rc;
        *collected = true;
        if (!eng->errors_complete) {
            if ((rc = error_bitmap(eng->last_db.get()))) return rc;
        } else {
            if (n && J.hinfo == nullptr) {  // (the device namespaces, brought back for this pass)
                J.info.resize(n);
                if ((rc = eng->download(J.info.data(), eng->res_info.p, (size_t)n * 4, "download nsinfo"))) return rc;
                J.hinfo = J.info.data();
            }
            std::vector<uint32_t> pairs;
            first_errors(eng, n, J.variety, J.hinfo, &pairs);
            if ((rc = upload(eng, eng->res_pairs, pairs.data(), pairs.size() * 4, "upload first errors"))) return rc;
            if ((e = mxp_launch_resolve_scatter(eng->res_pairs.as<uint32_t>(), (uint32_t)(pairs.size() / 2),
                                                eng->res_err_in.as<uint32_t>(), eng->stream)) != hipSuccess)
                return eng->hipfail(e, "launch first errors");
            A.err_in = eng->res_err_in.as<uint32_t>();
        }
        eng->trace_mark("first errors (class records, host)");
    }
    return MXP_OK;
}

// Count and scan: the pass pair picked (the filed pairs where the evaluation left them and no error
// bitmap is read; the default namespace's range tiled through LDS, resolve_tile, MXP_RESOLVE_TILE=0
// the per-lane walk), its count pass and the scan launched.  *write_pass: the pair's write pass.
int count_and_scan(mxp_resolve_job& J, mxp_resolve_args& A, ResPass* write_pass) {
    mxp_engine* eng = J.eng;
    const bool tiled = eng->resolve_tile && eng->resolver.default_id != MXP_NS_NONE;
    const bool pairs = J.pairs.on && !A.err;
    if (eng->resolve_pairs == 2 && J.n && !pairs) {
        char why[160];
        snprintf(why, sizeof why,
                 "pair Resolve not taken (MXP_RESOLVE_PAIRS=2): pairs filed %d, overflowed %u, error bitmap %d "
                 "(records %u of %u, class records %u)",
                 J.pairs_filed ? 1 : 0, J.pairs_ovf, A.err ? 1 : 0, J.recs_n, eng->errcap, J.class_recs_n);
        return eng->fail(MXP_ERR_STATE, why);
    }
    if (pairs) {
        A.pr_slots = J.pairs.slots;
        A.pr_qn = J.pairs.qn;
        A.pr_fills = J.pairs.fills;
        A.pr_row = J.pairs.row;
        A.pr_nch = J.pairs.nch;
    }
    const ResPass count_pass = pairs ? kPairsCount : tiled ? kTileCount : kCount;
    *write_pass = pairs ? kPairsWrite : tiled ? kTileWrite : kWrite;
    hipError_t e;
    if (J.n && (e = mxp_launch_resolve(&A, count_pass, eng->stream)) != hipSuccess) return eng->hipfail(e, "launch resolve");
    if (J.n && (e = mxp_launch_resolve(&A, kScan, eng->stream)) != hipSuccess) return eng->hipfail(e, "launch resolve scan");
    eng->trace_mark("  resolve: count + scan kernels");
    return MXP_OK;
}

// The action lists' format, as the ids stage sees it.
struct IdsFormat {
    size_t unit;   // bytes of one unit of sel_off / sel_cap: an id, or for delta8 a byte of the stream
    size_t id;     // bytes of an id as the write pass stores it
    bool encoded;  // delta8: the u16 list stays on the device (res_sel, id offsets res_off) and the
                   // encoder follows the write pass; the caller's sel_off receives byte offsets
};
IdsFormat ids_format(ResIds f) {
    return f == ResIds::DELTA8 ? IdsFormat{1, 2, true} : f == ResIds::U16 ? IdsFormat{2, 2, false} : IdsFormat{4, 4, false};
}

// The ids stage: the action lists produced on the device (list, and for delta8 stream) and brought to
// the caller (deliver_early / deliver_late).  A guard of 0 is no guard; under a guard a pass writes
// nothing when its count exceeds it (the write pass: sel_off[n]; the encoder's passes: the ids, the
// stream's also the bytes), so a guarded pass never writes past the room sized by that guard.
struct IdsStage {
    mxp_resolve_job& J;
    mxp_resolve_args& A;
    const ResPass write_pass;
    const IdsFormat f;
    ResSmall* small = nullptr;  // (encoded: ids_total, the ids' count, comes with the first downloads)
    mxp_d8_args D{};            // encoded: bytes per request (mxp_d8_count_kernel), then the stream (mxp_d8_write_kernel)
    mxp_resolve_args S{};       // ... and between them the Resolve's scan kernels over the byte counts

    int init() {
        if (!f.encoded) return MXP_OK;
        mxp_engine* eng = J.eng;
        const size_t n = J.n, grid = (J.n + 255u) / 256u;
        hipError_t e;
        if ((e = eng->res_bcount.reserve(n * 4 + 4)) != hipSuccess) return eng->hipfail(e, "alloc byte counts");
        if ((e = eng->res_bsum8.reserve(grid * 8 + 8)) != hipSuccess) return eng->hipfail(e, "alloc byte sums");
        if ((e = eng->res_boff.reserve((n + 1) * 8)) != hipSuccess) return eng->hipfail(e, "alloc byte offsets");
        if (int rc = res_small(eng, &small)) return rc;
        small->ids_total = 0;
        D.n = J.n;
        D.id_off = eng->res_off.as<uint64_t>();
        D.bcount = eng->res_bcount.as<uint32_t>();
        D.block_sum = eng->res_bsum8.as<uint64_t>();
        D.boff = eng->res_boff.as<uint64_t>();
        S.n = J.n;
        S.count = D.bcount;
        S.block_sum = D.block_sum;
        S.sel_off_out = eng->res_boff.as<uint64_t>();
        return MXP_OK;
    }
    // the device's copy of what the caller's sel_off receives
    const uint64_t* offsets() const { return (f.encoded ? J.eng->res_boff : J.eng->res_off).as<uint64_t>(); }

    // The ids into res_sel (room for `entries`), by the write pass; encoded: then their byte offsets
    // (bytes per request and the scan).  group: the encoder's lanes per request.
    int list(uint64_t entries, uint64_t guard, uint32_t group) {
        mxp_engine* eng = J.eng;
        DevBuf& d_sel = eng->res_sel;
        // (the encoder reads the list in 8-byte words: 16 bytes of slack)
        hipError_t e = d_sel.reserve(entries * f.id + (f.encoded ? 16 : 0));
        if (e != hipSuccess) return eng->hipfail(e, "alloc sel");
        A.sel_rules = d_sel.as<uint32_t>();
        A.sel_cap_dev = guard;
        if (entries) e = mxp_launch_resolve(&A, write_pass, eng->stream);
        A.sel_cap_dev = 0;
        if (e != hipSuccess) return eng->hipfail(e, "launch resolve write");
        if (!f.encoded) return MXP_OK;
        D.ids = d_sel.as<uint16_t>();
        D.cap = guard;
        if ((e = mxp_launch_d8(&D, 0, group, eng->stream)) != hipSuccess ||
            (e = mxp_launch_resolve(&S, kScan, eng->stream)) != hipSuccess)
            return eng->hipfail(e, "launch delta8 count");
        return MXP_OK;
    }
    // encoded: the list in res_sel coded into res_d8 (room for `room` bytes)
    int stream(uint64_t room, uint64_t guard, uint32_t group) {
        mxp_engine* eng = J.eng;
        hipError_t e;
        if ((e = eng->res_d8.reserve(room)) != hipSuccess) return eng->hipfail(e, "alloc delta8 stream");
        D.ids = eng->res_sel.as<uint16_t>();
        D.out = eng->res_d8.as<uint8_t>();
        D.cap = guard;
        if ((e = mxp_launch_d8(&D, 1, group, eng->stream)) != hipSuccess) return eng->hipfail(e, "launch delta8 write");
        return MXP_OK;
    }
    const void* produced() const { return f.encoded ? J.eng->res_d8.p : J.eng->res_sel.p; }

    // early: a copy kernel sized on the device by offsets()[n] into mapped pinned memory, nothing
    // when that exceeds cap -- enqueued before the host knows the count
    int deliver_early(void* sel_hd, uint64_t cap) {
        const hipError_t e = mxp_launch_d2h_copy_ids(sel_hd, produced(), offsets() + J.n, (uint32_t)f.unit, cap, J.eng->stream);
        return e == hipSuccess ? MXP_OK : J.eng->hipfail(e, "download sel");
    }
    // late: `total` units to unit `at` of the caller's list
    int deliver_late(void* sel_rules, uint64_t at, uint64_t total) {
        return J.eng->download((uint8_t*)sel_rules + (size_t)at * f.unit, produced(), total * f.unit, "download sel");
    }
};

// The caller's sel_off from the device's offsets.  A group member (place != nullptr) never writes
// sel_off[0]: that entry is the previous member's last one, and the group sets it.
mxp_engine::Piece offsets_piece(uint64_t* sel_off, const uint64_t* offs, size_t n, bool member) {
    return member ? mxp_engine::Piece{sel_off + 1, offs + 1, n * 8} : mxp_engine::Piece{sel_off, offs, (n + 1) * 8};
}

// The second phase, stage by stage.  On MXP_ERR_NOMEM status, err_rule and sel_off are complete:
// every return of it comes after their downloads.
// kept != nullptr (a batched Check, check.cpp): nothing of the ids is delivered -- the u16 / u32 list
// stays in res_sel with its offsets in res_off, *kept receives its length, and sel_off / sel_rules
// are not written.
int resolve_end(mxp_resolve_job& J, uint8_t* status, uint32_t* err_rule, uint64_t* sel_off, void* sel_rules,
                uint64_t sel_cap, const mxp_resolve_place* place, uint64_t* kept = nullptr) {
    mxp_engine* eng = J.eng;
    const uint32_t n = J.n;
    int rc;
    mxp_resolve_args A;
    if ((rc = resolve_args(J, &A))) return rc;
    bool collected = false;  // (records collected after the resolve kernels unless the triage needed them first)
    if (J.compact && (rc = triage_errors(J, A, &collected))) return rc;
    ResPass write_pass;
    if ((rc = count_and_scan(J, A, &write_pass))) return rc;
    IdsStage ids{J, A, write_pass, ids_format(J.ids)};
    if ((rc = ids.init())) return rc;
    const IdsFormat& f = ids.f;
    // The ids enqueued now, with the other outputs, when they go to the start of pinned caller memory:
    // the passes guarded by the capacity and a copy sized on the device -- one synchronisation for
    // every output instead of two (the ids' count is known on the host only after the first).
    // Taken only when all of these hold: requests, a capacity, no referenced attributes, sel_rules a
    // mapped pinned pointer, and the device buffers the capacity sizes (not the count; encoded: a u16
    // list entry beside every stream byte, 3 bytes a unit) within kEarlyIdsMax.  A group member that
    // is not the first has first_cap == 0, so it never goes early.
    const uint64_t early_cap = place ? J.first_cap : sel_cap;
    void* const sel_hd = n && early_cap && !J.ref_off && early_cap * (f.encoded ? f.id + f.unit : f.unit) <= kEarlyIdsMax
                             ? eng->host_dev_ptr(sel_rules)
                             : nullptr;
    if (sel_hd) {
        // encoded: the list's room is early_cap entries -- ids <= bytes, so it suffices whenever the
        // stream fits; the lanes per request from early_cap / n (the host does not know the ids' count
        // yet, and a caller sizes the capacity by the lists it expects)
        const uint32_t group = f.encoded ? mxp_d8_group(early_cap / n) : 1u;
        if ((rc = ids.list(early_cap, early_cap, group)) ||
            (f.encoded && (rc = ids.stream(early_cap, early_cap, group))) || (rc = ids.deliver_early(sel_hd, early_cap)))
            return rc;
    }
    if (kept) *kept = 0;
    if (!n) {
        if (!place && !kept) sel_off[0] = 0;
    } else {
        std::vector<mxp_engine::Piece> outs = {{status, eng->res_status.p, n}, {err_rule, eng->res_err_rule.p, (size_t)n * 4}};
        // (encoded: the byte offsets only where the guarded passes above enqueued them)
        if (kept) outs.push_back({kept, eng->res_off.as<uint64_t>() + n, 8});
        else if (!f.encoded || sel_hd) outs.push_back(offsets_piece(sel_off, ids.offsets(), n, place != nullptr));
        if (f.encoded) outs.push_back({&ids.small->ids_total, eng->res_off.as<uint64_t>() + n, 8});
        if ((rc = eng->download_all(outs, "download resolve outputs"))) return rc;
    }
    eng->trace_mark("resolve kernels + downloads");
    if (!collected) {
        if ((rc = eng->collect_errors(J.batch, J.db))) return rc;  // synchronises the stream
        eng->trace_mark("error records");
    }
    int ref_rc = MXP_OK;
    if (J.ref_off) {
        const mxp_engine::RefScope scope{&J.info, status, err_rule, J.variety};
        ref_rc = eng->refs_assemble(J.batch, J.recs, &scope, J.ref_off, J.refs, J.ref_cap);
        if (ref_rc && ref_rc != MXP_ERR_NOMEM) return ref_rc;
    }
    if (kept) return n ? ids.list(*kept, 0, 1u) : MXP_OK;  // (the list written, nothing delivered)
    // encoded, after the first synchronisation: the ids' count is known, and the lanes per request
    // come from the true mean.  The list is written again, and its byte offsets computed and brought
    // back, only if the early list did not fit (or there was none): otherwise both stand.
    const uint64_t ids_n = f.encoded && n ? ids.small->ids_total : 0;
    const uint32_t group = f.encoded && n ? mxp_d8_group((ids_n + n - 1) / n) : 1u;
    if (f.encoded && n && !(sel_hd && ids_n <= early_cap)) {
        if ((rc = ids.list(ids_n, 0, group))) return rc;
        if ((rc = eng->download_all({offsets_piece(sel_off, ids.offsets(), n, place != nullptr)}, "download byte offsets")))
            return rc;
        eng->trace_mark("delta8: u16 list + byte offsets");
    }
    const uint64_t total = n ? sel_off[n] : 0;
    // (a group member learns where its ids go in the whole batch's list once every member knows its
    // own count: place blocks until then, -1 = the whole list does not fit)
    int64_t at = 0;
    if (place) {
        at = (*place)(total);
        if (at < 0) return MXP_ERR_NOMEM;
    } else if (total > sel_cap) {
        return MXP_ERR_NOMEM;
    }
    // the early result stands only if it fitted its guard and belongs at the start of the list
    if (total && sel_hd && total <= early_cap && at == 0) {
        eng->trace_mark("action lists (with the outputs)");
        return ref_rc;
    }
    if (total) {  // (encoded: the list is in res_sel by now -- the stream alone; else the write pass)
        if ((rc = f.encoded ? ids.stream(total, 0, group) : ids.list(total, 0, group))) return rc;
        if ((rc = ids.deliver_late(sel_rules, (uint64_t)at, total))) return rc;
    }
    eng->trace_mark("action lists (gather + download)");
    return ref_rc;
}

// mxp_resolve_batch(_ex), and with ref_off its referenced attributes (mxp_resolve_refs).
//
// Compact path (round 5; not for referenced attributes): the evaluation writes the match bitmap and
// per-request error flags with error records instead of the error bitmap; namespaces come from the
// device (mxp_ns_kernel on the batch as uploaded); each failing request's first applicable error is
// found from the records on the host and scattered to the device; the counts are scanned on the
// device.  Records past the log's capacity fall back to the error bitmap.
int resolve_impl(mxp_engine* eng, const mxp_bag_batch* batch, uint32_t variety, ResIds ids, uint8_t* status,
                 uint32_t* err_rule, uint64_t* sel_off, void* sel_rules, uint64_t sel_cap, uint64_t* ref_off,
                 mxp_attr_ref* refs, uint64_t ref_cap, const mxp_resolve_place* place = nullptr,
                 mxp_dbatch* pre = nullptr, uint64_t first_cap = 0) {
    mxp_resolve_job J;
    J.first_cap = first_cap;
    J.db.reset(pre);  // (a batch uploaded before: taken over, whatever happens)
    if (!eng || !batch || !status || !err_rule || !sel_off || (sel_cap && !sel_rules) || variety >= 32)
        return MXP_ERR_ARG;
    J.eng = eng;
    J.batch = batch;
    J.variety = variety;
    J.ids = ids;
    J.ref_off = ref_off;
    J.refs = refs;
    J.ref_cap = ref_cap;
    if (int rc = resolve_begin(J)) return rc;
    return resolve_end(J, status, err_rule, sel_off, sel_rules, sel_cap, place);
}

}  // namespace

// (check.cpp) a Resolve whose ids stay on the device: rule ids as u16 (ids16) or u32 in res_sel, their
// offsets in res_off, *n_ids of them; status and err_rule as mxp_resolve_batch
int mxp_resolve_kept(mxp_engine* eng, const mxp_bag_batch* batch, uint32_t variety, bool ids16, uint8_t* status,
                     uint32_t* err_rule, uint64_t* n_ids) {
    if (!eng || !batch || !status || !err_rule || !n_ids || variety >= 32) return MXP_ERR_ARG;
    mxp_resolve_job J;
    J.eng = eng;
    J.batch = batch;
    J.variety = variety;
    J.ids = ids16 ? ResIds::U16 : ResIds::U32;
    if (int rc = resolve_begin(J)) return rc;
    return resolve_end(J, status, err_rule, nullptr, nullptr, 0, nullptr, n_ids);
}

int mxp_resolve_placed(mxp_engine* eng, mxp_dbatch* db, const mxp_bag_batch* batch, uint32_t variety, uint32_t flags,
                       uint8_t* status, uint32_t* err_rule, uint64_t* sel_off, void* sel_rules,
                       const mxp_resolve_place& place, uint64_t first_cap) {
    if (!batch && db && db->wide) batch = &db->wide->view;  // (a narrow upload: its host view)
    ResIds ids;
    if (!resolve_ids_format(flags, &ids)) {
        if (eng && db) eng->recycle(db);
        return MXP_ERR_ARG;
    }
    return resolve_impl(eng, batch, variety, ids, status, err_rule, sel_off, sel_rules,
                        0, nullptr, nullptr, 0, &place, db, first_cap);
}

// (group.cpp) a member's finish with its ids placed by the group, and dropping a submitted job
int mxp_resolve_finish_placed(mxp_resolve_job* job, uint8_t* status, uint32_t* err_rule, uint64_t* sel_off,
                              void* sel_rules, const mxp_resolve_place& place, uint64_t first_cap) {
    std::unique_ptr<mxp_resolve_job> J(job);
    if (!J) return MXP_ERR_ARG;
    J->first_cap = first_cap;
    return resolve_end(*J, status, err_rule, sel_off, sel_rules, 0, &place);
}
void mxp_resolve_job_free(mxp_resolve_job* job) { delete job; }

extern "C" {

int mxp_resolve_batch(mxp_engine* eng, const mxp_bag_batch* batch, uint32_t variety, uint8_t* status,
                      uint32_t* err_rule, uint64_t* sel_off, uint32_t* sel_rules, uint64_t sel_cap) {
    return resolve_impl(eng, batch, variety, ResIds::U32, status, err_rule, sel_off, sel_rules, sel_cap, nullptr,
                        nullptr, 0);
}

int mxp_resolve_batch_ex(mxp_engine* eng, const mxp_bag_batch* batch, uint32_t variety, uint32_t flags,
                         uint8_t* status, uint32_t* err_rule, uint64_t* sel_off, void* sel_rules, uint64_t sel_cap) {
    ResIds ids;
    if (!resolve_ids_format(flags, &ids)) return MXP_ERR_ARG;
    return resolve_impl(eng, batch, variety, ids, status, err_rule, sel_off, sel_rules,
                        sel_cap, nullptr, nullptr, 0);
}

int mxp_resolve_uploaded(mxp_engine* eng, mxp_dbatch* db, const mxp_bag_batch* batch, uint32_t variety, uint32_t flags,
                         uint8_t* status, uint32_t* err_rule, uint64_t* sel_off, void* sel_rules, uint64_t sel_cap) {
    if (!db) return MXP_ERR_ARG;
    if (!batch && db->wide) batch = &db->wide->view;  // (a narrow upload: its host view)
    ResIds ids;
    if (!eng || !resolve_ids_format(flags, &ids)) {
        if (eng) eng->recycle(db);
        return MXP_ERR_ARG;
    }
    return resolve_impl(eng, batch, variety, ids, status, err_rule, sel_off, sel_rules,
                        sel_cap, nullptr, nullptr, 0, nullptr, db);
}

int mxp_resolve_submit(mxp_engine* eng, mxp_dbatch* db, const mxp_bag_batch* batch, uint32_t variety, uint32_t flags,
                       mxp_resolve_job** out) {
    std::unique_ptr<mxp_resolve_job> J(new mxp_resolve_job());
    J->db.reset(db);  // (taken over, whatever happens)
    ResIds ids;
    if (!eng || !db || !out || !resolve_ids_format(flags, &ids) || variety >= 32) return MXP_ERR_ARG;
    if (!batch && db->wide) batch = &db->wide->view;  // (a narrow upload: its host view)
    if (!batch) return MXP_ERR_ARG;
    J->eng = eng;
    J->batch = batch;
    J->variety = variety;
    J->ids = ids;
    if (int rc = resolve_begin(*J)) return rc;
    *out = J.release();
    return MXP_OK;
}

int mxp_resolve_finish(mxp_resolve_job* job, uint8_t* status, uint32_t* err_rule, uint64_t* sel_off, void* sel_rules,
                       uint64_t sel_cap) {
    std::unique_ptr<mxp_resolve_job> J(job);
    if (!J || !status || !err_rule || !sel_off || (sel_cap && !sel_rules)) return MXP_ERR_ARG;
    return resolve_end(*J, status, err_rule, sel_off, sel_rules, sel_cap, nullptr);
}

int mxp_resolve_refs(mxp_engine* eng, const mxp_bag_batch* batch, uint32_t variety, uint8_t* status,
                     uint32_t* err_rule, uint64_t* sel_off, uint32_t* sel_rules, uint64_t sel_cap, uint64_t* ref_off,
                     mxp_attr_ref* refs, uint64_t ref_cap) {
    if (!ref_off) return MXP_ERR_ARG;
    return resolve_impl(eng, batch, variety, ResIds::U32, status, err_rule, sel_off, sel_rules, sel_cap, ref_off,
                        refs, ref_cap);
}

}  // extern "C"
