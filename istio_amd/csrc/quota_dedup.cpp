// quota_dedup.cpp -- memquota DeduplicationID handling, host side (include/mxp.h; kernels in
// quota_dedup.hip).
//
// Reference: mixer/adapter/memquota/dedup.go:61-116 (handleDedup, reapDedup) and memquota.go:118-211
// (what alloc and free hand to it, QuotaResult.ValidDuration).  One dedup state per mxp_quota, as
// handler.common: two generations of id -> (amount, exp), shared by allocs and frees and by every
// key.  A call probes the generations, elects the lowest arrival index of each missing id, runs the
// unchanged replay (mxp_quota_alloc_device) on amounts zeroed for everyone else, and finishes:
// answers by role, the replayed results stored in `recent`.
//
// The host keeps upper bounds of what `recent` holds (ids and pool bytes added since the last reap:
// every request of a call could be a new id) and keeps the table at most half full and the pool
// large enough before each call; when the bounds say otherwise it reads the true counts back once
// and grows only if those say so too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "quota_dedup_args.h"
#include "quota_impl.h"

extern "C" hipError_t mxp_launch_qdd_probe(const mxp_qdd_args* a, hipStream_t s);
extern "C" hipError_t mxp_launch_qdd_finish(const mxp_qdd_args* a, hipStream_t s);
extern "C" hipError_t mxp_launch_qdd_rehash(const mxp_qdd_gen* from, const mxp_qdd_gen* to, hipStream_t s);

namespace {

struct Gen {
    DevBuf tab, pool, count;  // tab: `slots` entries (mxp_qdd_ent)
    uint32_t slots = 0;
    void view(mxp_qdd_gen* g) const {
        memset(g, 0, sizeof *g);
        if (!slots) return;
        g->ent = tab.as<mxp_qdd_ent>();
        g->pool = pool.as<uint8_t>();
        g->count = count.as<unsigned long long>();
        g->mask = slots - 1;
    }
};

uint64_t pow2_at_least(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

struct mxp_quota_dedup {
    Gen gen[2];
    int recent = 0;
    DevBuf tab_new, pool_new;  // growth: the larger table / pool before it trades places
    DevBuf key_valid, btab, ref, role, eff, sgrant;
    size_t req_cap = 0;
    uint64_t ub_ids = 0, ub_bytes = 0;  // upper bounds of recent's count[0], count[1]
    uint32_t init_slots = 1u << 16;     // MXP_QDD_SLOTS
    uint64_t hash_mask = MXP_QDD_OCC - 1;  // MXP_QDD_HASH_BITS
};

void mxp_quota_dedup_delete::operator()(mxp_quota_dedup* d) const { delete d; }

namespace {

// device blocks of the dedup state come from the engine's bin (DevBuf::alloc draws from it for
// buffers inside [g_bin_db, g_bin_db + size)) ...
struct BinTake {
    BlockBin* take0 = g_bin_take;
    const void* db0 = g_bin_db;
    size_t sz0 = g_bin_db_size;
    BinTake(mxp_engine* eng, const mxp_quota_dedup* D) {
        g_bin_take = &eng->bin;
        g_bin_db = D;
        g_bin_db_size = sizeof *D;
    }
    ~BinTake() {
        g_bin_take = take0;
        g_bin_db = db0;
        g_bin_db_size = sz0;
    }
};
// ... and return to it behind an event on the stream whose work still reads them
void give_back(mxp_engine* eng, hipStream_t s, std::initializer_list<DevBuf*> bufs) {
    BlockBin::Group g;
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, kOrderEvent) != hipSuccess || hipEventRecord(ev, s) != hipSuccess) {
        if (ev) (void)hipEventDestroy(ev);
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s);
        for (DevBuf* d : bufs) d->reset();
        return;
    }
    g.evs.push_back(ev);
    g_bin_give = &g.blks;
    for (DevBuf* d : bufs) d->reset();
    g_bin_give = nullptr;
    if (g.blks.empty()) (void)hipEventDestroy(ev);
    else eng->bin.put(std::move(g));
}

int dedup_state(mxp_engine* eng, mxp_quota* Q) {
    if (Q->dedup) return MXP_OK;
    std::unique_ptr<mxp_quota_dedup, mxp_quota_dedup_delete> D(new mxp_quota_dedup());
    if (const char* v = getenv("MXP_QDD_SLOTS")) {
        const long long s = atoll(v);
        if (s >= 2 && s <= (1ll << 30)) D->init_slots = (uint32_t)pow2_at_least((uint64_t)s);
    }
    if (const char* v = getenv("MXP_QDD_HASH_BITS")) {
        const int b = atoi(v);
        if (b >= 1 && b < 63) D->hash_mask = (1ull << b) - 1;
    }
    hipError_t e;
    BinTake bt(eng, D.get());
    if ((e = D->key_valid.alloc((size_t)Q->n_keys * 8)) != hipSuccess) return eng->hipfail(e, "quota dedup durations");
    if (Q->n_keys && (e = hipMemcpy(D->key_valid.p, Q->valid_ns.data(), (size_t)Q->n_keys * 8, hipMemcpyHostToDevice)) !=
                         hipSuccess)
        return eng->hipfail(e, "quota dedup durations");
    Q->dedup = std::move(D);
    return MXP_OK;
}

// `recent` able to take n more ids of add_bytes pool bytes (padding included)
int ensure_recent(mxp_engine* eng, mxp_quota_dedup* D, uint32_t n, uint64_t add_bytes, hipStream_t s) {
    Gen& G = D->gen[D->recent];
    hipError_t e;
    if (!G.slots) {  // the first call, or the first after the reap that made this generation recent
        const uint64_t slots = std::max<uint64_t>(D->init_slots, pow2_at_least(2ull * n));
        if (slots > (1ull << 31)) return eng->fail(MXP_ERR_NOMEM, "quota dedup table too large");
        if ((e = G.tab.alloc(slots * 32)) != hipSuccess || (e = G.pool.alloc(pow2_at_least(add_bytes + 16))) != hipSuccess ||
            (e = G.count.alloc(16)) != hipSuccess)
            return eng->hipfail(e, "quota dedup table");
        if ((e = hipMemsetAsync(G.tab.p, 0, slots * 32, s)) != hipSuccess ||
            (e = hipMemsetAsync(G.count.p, 0, 16, s)) != hipSuccess)
            return eng->hipfail(e, "quota dedup table");
        G.slots = (uint32_t)slots;
        D->ub_ids = D->ub_bytes = 0;
        return MXP_OK;
    }
    if (2 * (D->ub_ids + n) <= G.slots && D->ub_bytes + add_bytes + 16 <= G.pool.cap) return MXP_OK;
    unsigned long long cnt[2];
    if ((e = hipMemcpyAsync(cnt, G.count.p, 16, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return eng->hipfail(e, "quota dedup counts");
    D->ub_ids = cnt[0];
    D->ub_bytes = cnt[1];
    if (2 * (D->ub_ids + n) > G.slots) {
        const uint64_t slots = pow2_at_least(2 * (D->ub_ids + n));
        if (slots > (1ull << 31)) return eng->fail(MXP_ERR_NOMEM, "quota dedup table too large");
        if ((e = D->tab_new.alloc(slots * 32)) != hipSuccess) return eng->hipfail(e, "quota dedup growth");
        if ((e = hipMemsetAsync(D->tab_new.p, 0, slots * 32, s)) != hipSuccess) return eng->hipfail(e, "quota dedup growth");
        mxp_qdd_gen from, to;
        G.view(&from);
        G.tab.swap(D->tab_new);
        G.slots = (uint32_t)slots;
        G.view(&to);
        if ((e = mxp_launch_qdd_rehash(&from, &to, s)) != hipSuccess) return eng->hipfail(e, "quota dedup rehash");
        give_back(eng, s, {&D->tab_new});
    }
    if (D->ub_bytes + add_bytes + 16 > G.pool.cap) {
        if ((e = D->pool_new.alloc(pow2_at_least(D->ub_bytes + add_bytes + 16))) != hipSuccess)
            return eng->hipfail(e, "quota dedup growth");
        if (D->ub_bytes && (e = hipMemcpyAsync(D->pool_new.p, G.pool.p, D->ub_bytes, hipMemcpyDeviceToDevice, s)) != hipSuccess)
            return eng->hipfail(e, "quota dedup growth");
        G.pool.swap(D->pool_new);
        give_back(eng, s, {&D->pool_new});
    }
    return MXP_OK;
}

}  // namespace

extern "C" {

int mxp_quota_alloc_dedup_device(mxp_engine* eng, mxp_quota* Q, uint32_t n, const uint32_t* d_key,
                                 const int64_t* d_amount, const uint8_t* d_best_effort, const uint8_t* d_id_bytes,
                                 const uint32_t* d_id_off, uint32_t id_bytes_total, int64_t now_ns, void* stream,
                                 int64_t* d_granted, int64_t* d_valid_ns, uint8_t* d_dup, int64_t* d_delta) {
    if (!eng || !Q || (n && (!d_key || !d_amount || !d_best_effort || !d_id_bytes || !d_id_off || !d_granted)))
        return MXP_ERR_ARG;
    if (!n) return MXP_OK;
    if (n > (1u << 30)) return eng->fail(MXP_ERR_ARG, "quota dedup: more than 2^30 requests in a call");
    if (eng->device < 0) return eng->fail(MXP_ERR_STATE, "host-only engine");
    hipStream_t s = stream ? (hipStream_t)stream : eng->stream;
    hipError_t e;
    if ((e = hipSetDevice(eng->device)) != hipSuccess) return eng->hipfail(e, "hipSetDevice");
    int rc;
    if ((rc = dedup_state(eng, Q))) return rc;
    mxp_quota_dedup* D = Q->dedup.get();
    BinTake bt(eng, D);
    if (n > D->req_cap) {
        const size_t bslots = (size_t)pow2_at_least(2ull * n);
        if ((e = D->btab.alloc(bslots * sizeof(mxp_qdd_bslot))) != hipSuccess ||
            (e = D->ref.alloc((size_t)n * 4)) != hipSuccess || (e = D->role.alloc(n)) != hipSuccess ||
            (e = D->eff.alloc((size_t)n * 8)) != hipSuccess || (e = D->sgrant.alloc((size_t)n * 8)) != hipSuccess) {
            D->req_cap = 0;
            return eng->hipfail(e, "quota dedup scratch");
        }
        D->req_cap = n;
    }
    // every id padded to 8 bytes in the pool
    const uint64_t add_bytes = (uint64_t)id_bytes_total + 8ull * n;
    if ((rc = ensure_recent(eng, D, n, add_bytes, s))) return rc;

    mxp_qdd_args A;
    memset(&A, 0, sizeof A);
    A.n = n;
    A.n_keys = Q->n_keys;
    A.now_ns = now_ns;
    A.hash_mask = D->hash_mask;
    A.key = d_key;
    A.amount = d_amount;
    A.best_effort = d_best_effort;
    A.id_bytes = d_id_bytes;
    A.id_off = d_id_off;
    D->gen[D->recent].view(&A.recent);
    D->gen[D->recent ^ 1].view(&A.old);
    A.btab = D->btab.as<mxp_qdd_bslot>();
    A.bmask = (uint32_t)(pow2_at_least(2ull * n) - 1);  // (at least 2n slots, whatever the scratch holds)
    A.ref = D->ref.as<uint32_t>();
    A.role = D->role.as<uint8_t>();
    A.eff_amount = D->eff.as<int64_t>();
    A.sgrant = D->sgrant.as<int64_t>();
    A.key_valid_ns = D->key_valid.as<int64_t>();
    A.granted = d_granted;
    A.valid_ns = d_valid_ns;
    A.dup = d_dup;
    if ((e = mxp_launch_qdd_probe(&A, s)) != hipSuccess) return eng->hipfail(e, "launch quota dedup probe");
    // the replay as it is: leaders with their own key, amount and flag, amount 0 for everyone else
    if (!Q->n_keys && (e = hipMemsetAsync(D->sgrant.p, 0, (size_t)n * 8, s)) != hipSuccess)
        return eng->hipfail(e, "quota dedup grants");
    if ((rc = mxp_quota_alloc_device(eng, Q, n, d_key, D->eff.as<int64_t>(), d_best_effort, now_ns, s,
                                     D->sgrant.as<int64_t>(), d_delta)))
        return rc;
    if ((e = mxp_launch_qdd_finish(&A, s)) != hipSuccess) return eng->hipfail(e, "launch quota dedup finish");
    D->ub_ids += n;
    D->ub_bytes += add_bytes;
    return MXP_OK;
}

int mxp_quota_alloc_dedup(mxp_engine* eng, mxp_quota* Q, uint32_t n, const uint32_t* key, const int64_t* amount,
                          const uint8_t* best_effort, const uint8_t* id_bytes, const uint32_t* id_off, int64_t now_ns,
                          int64_t* granted, int64_t* valid_ns, uint8_t* dup) {
    if (!eng || !Q || (n && (!key || !amount || !best_effort || !id_off || !granted))) return MXP_ERR_ARG;
    if (!n) return MXP_OK;
    char msg[96];
    if (id_off[0] != 0) return eng->fail(MXP_ERR_ARG, "quota dedup: id_off[0] is not 0 (request 0)");
    for (uint32_t i = 0; i < n; i++) {
        if (key[i] >= Q->n_keys) {
            snprintf(msg, sizeof msg, "quota key id out of range (request %u)", i);
            return eng->fail(MXP_ERR_ARG, msg);
        }
        if (id_off[i + 1] < id_off[i]) {
            snprintf(msg, sizeof msg, "quota dedup: id_off decreases at request %u", i);
            return eng->fail(MXP_ERR_ARG, msg);
        }
    }
    const uint32_t total = id_off[n];
    if (total && !id_bytes) return MXP_ERR_ARG;
    hipError_t e;
    if ((e = hipSetDevice(eng->device)) != hipSuccess) return eng->hipfail(e, "hipSetDevice");
    DevBuf dk, da, db, di, dof, dg, dv, dd;
    if ((e = dk.alloc((size_t)n * 4)) != hipSuccess || (e = da.alloc((size_t)n * 8)) != hipSuccess ||
        (e = db.alloc(n)) != hipSuccess || (e = di.alloc((size_t)total + 16)) != hipSuccess ||
        (e = dof.alloc(((size_t)n + 1) * 4)) != hipSuccess || (e = dg.alloc((size_t)n * 8)) != hipSuccess ||
        (e = dv.alloc((size_t)n * 8)) != hipSuccess || (e = dd.alloc(n)) != hipSuccess)
        return eng->hipfail(e, "quota dedup buffers");
    hipStream_t s = eng->stream;
    if ((e = hipMemcpyAsync(dk.p, key, (size_t)n * 4, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = hipMemcpyAsync(da.p, amount, (size_t)n * 8, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = hipMemcpyAsync(db.p, best_effort, n, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = hipMemcpyAsync(dof.p, id_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (total && (e = hipMemcpyAsync(di.p, id_bytes, total, hipMemcpyHostToDevice, s)) != hipSuccess) ||
        (e = hipMemsetAsync(di.as<uint8_t>() + total, 0, 16, s)) != hipSuccess)  // (the slack the word compares read)
        return eng->hipfail(e, "quota dedup upload");
    int rc = mxp_quota_alloc_dedup_device(eng, Q, n, dk.as<uint32_t>(), da.as<int64_t>(), db.as<uint8_t>(),
                                          di.as<uint8_t>(), dof.as<uint32_t>(), total, now_ns, s, dg.as<int64_t>(),
                                          dv.as<int64_t>(), dd.as<uint8_t>(), nullptr);
    // (each download synchronises; a failed call's queued work is waited for before the buffers go)
    if (rc) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    if ((rc = eng->download(granted, dg.p, (size_t)n * 8, "quota dedup download"))) return rc;
    if (valid_ns && (rc = eng->download(valid_ns, dv.p, (size_t)n * 8, "quota dedup download"))) return rc;
    if (dup && (rc = eng->download(dup, dd.p, n, "quota dedup download"))) return rc;
    return MXP_OK;
}

int mxp_quota_dedup_reap(mxp_engine* eng, mxp_quota* Q, void* stream) {
    if (!eng || !Q) return MXP_ERR_ARG;
    if (!Q->dedup) return MXP_OK;  // (nothing seen yet: both generations empty)
    mxp_quota_dedup* D = Q->dedup.get();
    hipStream_t s = stream ? (hipStream_t)stream : eng->stream;
    hipError_t e;
    if ((e = hipSetDevice(eng->device)) != hipSuccess) return eng->hipfail(e, "hipSetDevice");
    // dedup.go:103-116: old <- recent, recent <- the old map, cleared
    D->recent ^= 1;
    Gen& G = D->gen[D->recent];
    D->ub_ids = D->ub_bytes = 0;
    if (G.slots && ((e = hipMemsetAsync(G.tab.p, 0, (size_t)G.slots * 32, s)) != hipSuccess ||
                    (e = hipMemsetAsync(G.count.p, 0, 16, s)) != hipSuccess))
        return eng->hipfail(e, "quota dedup reap");
    return MXP_OK;
}

int mxp_quota_dedup_stats(mxp_engine* eng, mxp_quota* Q, uint64_t out[4]) {
    if (!eng || !Q || !out) return MXP_ERR_ARG;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!Q->dedup) return MXP_OK;
    mxp_quota_dedup* D = Q->dedup.get();
    hipError_t e;
    if ((e = hipSetDevice(eng->device)) != hipSuccess) return eng->hipfail(e, "hipSetDevice");
    if ((e = hipDeviceSynchronize()) != hipSuccess) return eng->hipfail(e, "quota dedup stats");
    for (int g = 0; g < 2; g++) {
        const Gen& G = D->gen[g ? D->recent ^ 1 : D->recent];
        if (!G.slots) continue;
        unsigned long long cnt[2];
        if ((e = hipMemcpy(cnt, G.count.p, 16, hipMemcpyDeviceToHost)) != hipSuccess)
            return eng->hipfail(e, "quota dedup stats");
        out[g] = cnt[0];
        if (!g) {
            out[2] = G.slots;
            out[3] = cnt[1];
        }
    }
    return MXP_OK;
}

}  // extern "C"
