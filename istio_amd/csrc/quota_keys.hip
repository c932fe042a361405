// quota_keys.hip -- the stage between a Resolve and memquota's replay (include/mxp.h
// mxp_quota_batch): which quota instance a request dispatches to, the instance's key text, its limit
// and a stable key id.
//
//   dispatch  mixer/pkg/runtime/dispatcher.go:242-281, :160-187: the first selected rule with a quota
//             action dispatches that action's first instance, nothing else
//   limit     mixer/adapter/memquota/memquota.go:65-105: the first override whose every configured
//             dimension equals the instance's STRING value, else the quota's own numbers
//   makeKey   mixer/adapter/memquota/keys.go:35-95 (quota_key_fmt.h for the formatted values)
//
// Lane = request in every pass:
//   mxp_qk_pick     the walk over the request's kept ids to its unit, the early codes
//   mxp_qk_measure  the unit's dimensions read from the instance engine's result registers: Eval
//                   errors, kinds, the key's length and its class; words per 256 requests for the scan
//   (the Resolve's scan kernels over the words)
//   mxp_qk_write    the key's bytes into the call's blob, 8-byte aligned, a word per store
//   mxp_qk_probe    the persistent table, else election in the call's batch table (tag, lowest index)
//   mxp_qk_rank     leader or follower; per class the leaders of a 1,024-lane block counted in
//                   arrival order
//   mxp_qk_scan     per class the counts scanned over the blocks, from the class's ids taken so far
//   mxp_qk_assign   leaders take their class's next ids in arrival order, insert into the table and
//                   copy their bytes into the pool (pool offsets drawn per block); beyond the
//                   class's capacity: KEYS_FULL
//   mxp_qk_follow   followers take their leader's id and code; the amounts the replay sees
//   mxp_qk_answers  the 24-byte answers
// Kernel boundaries order everything between waves, as in quota_dedup.hip: no kernel reads what
// another wave of the same launch stored plainly; words a launch CASes are read with relaxed
// agent-scope atomic loads; every store is a plain vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mxp.h"
#include "quota_bytes.h"
#include "quota_key_fmt.h"
#include "quota_keys_args.h"
#include "vm.h"

static_assert(sizeof(mxp_qk_answer) == 24 && sizeof(mxp_quota_answer) == 24, "the answer as include/mxp.h describes it");
static_assert(sizeof(mxp_qk_ent) == 24 && sizeof(mxp_qk_bslot) == 16, "table entries");

namespace {

using namespace mxp_qbytes;

struct Str {
    const uint8_t* p;
    uint32_t n;
};
__device__ __forceinline__ Str str_of(const mxp_qk_args& A, uint64_t id) {
    const bool g = id < A.n_gstr;
    const uint64_t d = g ? A.gstr_off[id] : A.bstr_off[id - A.n_gstr];
    return Str{(g ? A.gstr : A.bstr) + (d >> 24), (uint32_t)(d & 0xFFFFFFu)};
}

// the bytes of a []byte value by its raw id (quota_keys_args.h); false: not on the device
__device__ __forceinline__ bool bytes_of(const mxp_qk_args& A, uint64_t id, Str* out) {
    const uint64_t r = MXP_BYTES_RAW(id);
    uint64_t d;
    const uint8_t* pool;
    if (r < A.n_gb) {
        d = A.gb_off[r];
        pool = A.gb;
    } else {
        const uint64_t j = r - A.n_gb;
        if (!A.dev_packed) {
            if (j >= A.n_ob) return false;
            d = A.ob_off[j];
            pool = A.ob;
        } else if (j < A.ns) {  // a batch string used as bytes
            d = A.bstr_off[j];
            pool = A.bstr;
        } else {  // a parsed ip() value: net.ParseIP's 16-byte form
            if (!A.pip || j - A.ns >= A.n_gstr + A.ns) return false;
            *out = Str{A.pip + 16u * (j - A.ns), 16u};
            return true;
        }
    }
    *out = Str{pool + (d >> 24), (uint32_t)(d & 0xFFFFFFu)};
    return true;
}

// The kind of dimension D's value v for the key (0: outside v1), v reduced to its payload.  An
// interface register holds a kind and 56 bits: a string id, a bool and a []byte id are whole in
// it, a number is not, so an interface-typed INT64 or DOUBLE is refused like the kinds v1 leaves out.
__device__ __forceinline__ uint32_t value_kind(const mxp_qk_args& A, const mxp_qk_dim& D, uint64_t* v) {
    if (D.kind) return D.kind;
    const uint32_t k = MXP_FH_KIND(*v);
    *v = MXP_FH_ID(*v);
    if (k == MXP_BYTES) {
        Str s;
        return bytes_of(A, *v, &s) ? k : 0u;
    }
    return (k == MXP_STRING || k == MXP_BOOL) ? k : 0u;
}

__device__ __forceinline__ bool eval_failed(const mxp_qk_args& A, uint32_t q, uint32_t rule) {
    return (A.err[(uint64_t)(rule >> 5) * A.n + q] >> (rule & 31u)) & 1u;
}

// limit(): the class of the first matching override, else the default's
__device__ __forceinline__ uint32_t classify(const mxp_qk_args& A, const mxp_qk_unit& U, uint32_t q) {
    for (uint32_t o = 0; o < U.n_ovr; o++) {
        const mxp_qk_ovr O = A.ovrs[U.ovr_off + o];
        if (O.never) continue;
        bool m = true;
        for (uint32_t c = 0; c < O.n_cond && m; c++) {
            const mxp_qk_cond C = A.conds[O.cond_off + c];
            const mxp_qk_dim D = A.dims[C.dim];
            uint64_t v = A.vals[(uint64_t)q * A.vstride + D.value_rule];
            if (value_kind(A, D, &v) != MXP_STRING) {  // (neither a string nor a Stringer)
                m = false;
                break;
            }
            const Str s = str_of(A, v);
            m = s.n == C.val_len && same_bytes(s.p, A.text + C.val_off, s.n);
        }
        if (m) return O.cls;
    }
    return U.cls_default;
}

// bytes gathered into 8-byte words, each stored once; nothing stored at or past `end`
struct WordSink {
    uint64_t* dst;
    uint64_t* end;
    uint64_t w;
    uint32_t nb;
    __device__ __forceinline__ void operator()(uint8_t b) {
        w |= (uint64_t)b << (8u * nb);
        if (++nb == 8u) {
            if (dst < end) *dst = w;
            dst++;
            w = 0;
            nb = 0;
        }
    }
    __device__ __forceinline__ void bytes(const uint8_t* p, uint32_t n) {
        for (uint32_t i = 0; i < n; i++) (*this)(p[i]);
    }
    // n bytes of a string pool (8-aligned entries, 16 bytes of slack: ld8_any's reads stay inside),
    // a u64 word per load
    __device__ __forceinline__ void words(const uint8_t* p, uint32_t n) {
        uint32_t i = 0;
        for (; i + 8u <= n; i += 8u) {
            const uint64_t x = ld8_any(p + i);
            const uint64_t lo = nb ? w | (x << (8u * nb)) : x;
            if (dst < end) *dst = lo;
            dst++;
            w = nb ? x >> (64u - 8u * nb) : 0ull;
        }
        if (i < n) {
            uint64_t x = ld8_any(p + i);
            for (; i < n; i++, x >>= 8) (*this)((uint8_t)x);
        }
    }
    __device__ __forceinline__ void flush() {
        if (nb && dst < end) *dst = w;  // (the tail's padding bytes are zero)
    }
};

template <bool IDS16>
__device__ __forceinline__ uint32_t rule_at(const mxp_qk_args& A, uint64_t j) {
    if constexpr (IDS16) return ((const uint16_t*)A.ids)[j];
    else return ((const uint32_t*)A.ids)[j];
}

}  // namespace

template <bool IDS16>
__global__ __launch_bounds__(256) void mxp_qk_pick_kernel(mxp_qk_args A) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= A.n) return;
    int32_t code;
    uint32_t unit = MXP_QUOTA_NO_UNIT;
    if (A.skip && A.skip[q]) {
        code = MXP_QUOTA_SKIPPED;
    } else if (A.status[q] != MXP_RESOLVE_OK) {
        code = MXP_QUOTA_RESOLVE_ERROR;
    } else {
        code = MXP_QUOTA_NOT_APPLIED;
        const uint64_t end = A.id_off[q + 1u];
        for (uint64_t j = A.id_off[q]; j < end; j++) {
            const uint32_t u = A.rule_unit[rule_at<IDS16>(A, j)];
            if (u == MXP_QUOTA_NO_UNIT) continue;
            if (u == MXP_QUOTA_OTHER_UNIT) {
                code = MXP_QUOTA_OTHER;
            } else {
                unit = u;
                code = MXP_QUOTA_OK;
            }
            break;
        }
    }
    A.unit[q] = unit;
    A.code[q] = code;
}

extern "C" __global__ __launch_bounds__(256) void mxp_qk_measure(mxp_qk_args A) {
    __shared__ uint64_t wsum[4];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    uint32_t words = 0;
    if (q < A.n) {
        const uint32_t u = A.unit_in[q];
        // (the stage alone has no pick pass: a request without a unit is not applied)
        int32_t code = A.ids ? A.code[q] : (int32_t)MXP_QUOTA_NOT_APPLIED;
        uint32_t len = 0, cls = MXP_QK_NO_CLASS, failed = 0;
        if (u < A.n_units) {
            const mxp_qk_unit U = A.units[u];
            bool unsupported = false;
            uint32_t L = U.fixed_len;
            for (uint32_t d = 0; d < U.n_dims; d++) {
                const mxp_qk_dim D = A.dims[U.dim_off + d];
                if (eval_failed(A, q, D.value_rule)) {
                    failed |= 1u << D.bit;
                    continue;
                }
                uint64_t v = A.vals[(uint64_t)q * A.vstride + D.value_rule];
                const uint32_t k = value_kind(A, D, &v);
                Str s{nullptr, 0u};
                if (!k) unsupported = true;
                else if (k == MXP_STRING) L += str_of(A, v).n;
                else if (k == MXP_BYTES) L += bytes_of(A, v, &s) ? s.n : 0u;
                else L += mxp_qk_len(k, v);
            }
            if (failed) {
                code = MXP_QUOTA_EVAL_ERROR;
            } else if (unsupported) {
                code = MXP_QUOTA_KEY_UNSUPPORTED;
            } else {
                code = MXP_QUOTA_OK;
                if (A.amount[q] != 0) {  // (amount 0: QuotaResult{}, no key is made)
                    len = L;
                    cls = classify(A, U, q);
                }
            }
        }
        words = (len + 7u) / 8u;
        A.code[q] = code;
        A.len[q] = len;
        A.words[q] = words;
        A.cls[q] = cls;
        A.failed[q] = failed;
        A.key[q] = MXP_QK_NO_KEY;
        A.role[q] = MXP_QK_NONE;
    }
    uint64_t mine = words;
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0u) A.block_sum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

extern "C" __global__ __launch_bounds__(256) void mxp_qk_write(mxp_qk_args A) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= A.n || A.cls[q] == MXP_QK_NO_CLASS) return;
    const mxp_qk_unit U = A.units[A.unit_in[q]];
    uint64_t* const blob = (uint64_t*)A.blob;
    WordSink out{blob + A.woff[q], blob + A.woff[q + 1u], 0ull, 0u};
    out.bytes(A.text + U.name_off, U.name_len);
    for (uint32_t d = 0; d < U.n_dims; d++) {
        const mxp_qk_dim D = A.dims[U.dim_off + d];
        out((uint8_t)';');
        out.bytes(A.text + D.label_off, D.label_len);
        out((uint8_t)'=');
        uint64_t v = A.vals[(uint64_t)q * A.vstride + D.value_rule];
        const uint32_t k = value_kind(A, D, &v);
        if (k == MXP_STRING) {
            const Str s = str_of(A, v);
            out.words(s.p, s.n);
        } else if (k == MXP_BYTES) {  // buf.Write(v)
            Str s{nullptr, 0u};
            if (bytes_of(A, v, &s)) out.bytes(s.p, s.n);
        } else {
            mxp_qk_fmt(k, v, out);
        }
    }
    out.flush();
}

extern "C" __global__ __launch_bounds__(256) void mxp_qk_probe(mxp_qk_args A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t cls = A.cls[i];
    if (cls == MXP_QK_NO_CLASS) return;
    const uint32_t len = A.len[i];
    const uint8_t* p = A.blob + A.woff[i] * 8u;
    const uint64_t h = id_hash(p, len) & A.hash_mask;
    const unsigned long long hk = h | MXP_QK_OCC;
    // the persistent table (at most half full: an empty slot ends the probe; no insert in this launch)
    for (uint32_t s = (uint32_t)h & A.tmask;; s = (s + 1u) & A.tmask) {
        const unsigned long long e = A.ent[s].hkey;
        if (!e) break;
        if (e != hk) continue;
        const uint64_t loc = A.ent[s].loc;
        if ((uint32_t)loc != len || !same_bytes(p, A.pool + (loc >> 32) * 8u, len)) continue;
        if (A.ent[s].cls == cls) {
            A.key[i] = A.ent[s].id;
            A.role[i] = MXP_QK_HIT;
        } else {  // the text is held under another limit: reported, not approximated
            A.code[i] = MXP_QUOTA_KEY_CONFLICT;
            A.cls[i] = MXP_QK_NO_CLASS;
        }
        return;
    }
    // a miss: every request of the call with this text ends on one slot of the batch table
    const uint64_t tag = h >> 32;
    const unsigned long long mine = (tag << 32) | (i + 1u);
    uint32_t s = (uint32_t)h & A.bmask;
    for (;; s = (s + 1u) & A.bmask) {
        unsigned long long e = vload(&A.btab[s].occ);
        if (e == MXP_QK_BEMPTY) {
            e = atomicCAS(&A.btab[s].occ, MXP_QK_BEMPTY, mine);
            if (e == MXP_QK_BEMPTY) break;
        }
        if ((e >> 32) != tag) continue;
        const uint32_t other = (uint32_t)e - 1u;
        if (A.len[other] == len && same_bytes(p, A.blob + A.woff[other] * 8u, len)) break;
    }
    atomicMin(&A.btab[s].lead, i);
    A.role[i] = MXP_QK_LEADER;  // (a candidate until the rank pass)
    A.ref[i] = s;
}

extern "C" __global__ __launch_bounds__(MXP_QK_BLOCK) void mxp_qk_rank(mxp_qk_args A) {
    __shared__ uint32_t s_cnt[MXP_QK_BLOCK / 64u][MXP_QK_MAX_CLASSES];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t k = t; k < (MXP_QK_BLOCK / 64u) * MXP_QK_MAX_CLASSES; k += MXP_QK_BLOCK) (&s_cnt[0][0])[k] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * MXP_QK_BLOCK + t;
    bool leader = false;
    uint32_t c = MXP_QK_NO_CLASS;
    if (i < A.n && A.role[i] == MXP_QK_LEADER) {
        c = A.cls[i];
        const uint32_t l = A.btab[A.ref[i]].lead;
        if (l == i) {
            leader = true;
        } else if (A.cls[l] != c) {  // the first arrival holds the text under another limit
            A.code[i] = MXP_QUOTA_KEY_CONFLICT;
            A.role[i] = MXP_QK_NONE;
        } else {
            A.role[i] = MXP_QK_FOLLOWER;
            A.ref[i] = l;
        }
    }
    // the wave's leaders ranked per class in lane order (every lane of the wave takes every round)
    uint32_t rank = 0;
    for (unsigned long long pend = __ballot(leader); pend;) {
        const int src = __builtin_ctzll(pend);
        const uint32_t cc = __shfl(c, src);
        const unsigned long long m = __ballot(leader && c == cc);
        if (leader && c == cc) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if ((int)lane == src) s_cnt[wave][cc] = (uint32_t)__popcll(m);
        pend &= ~m;
    }
    __syncthreads();
    if (t < A.n_cls) {  // the waves' counts to their exclusive prefix; the block's count out
        uint32_t run = 0;
        for (uint32_t w = 0; w < MXP_QK_BLOCK / 64u; w++) {
            const uint32_t x = s_cnt[w][t];
            s_cnt[w][t] = run;
            run += x;
        }
        A.blk_cnt[(uint64_t)t * A.nb + blockIdx.x] = run;
    }
    __syncthreads();
    if (leader) A.ref[i] = s_cnt[wave][c] + rank;  // rank among the block's leaders of the class
}

// one block per class: the blocks' leader counts to exclusive offsets from the class's ids taken so far
extern "C" __global__ __launch_bounds__(256) void mxp_qk_scan(mxp_qk_args A) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t s_next;
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    uint32_t* const row = A.blk_cnt + (uint64_t)c * A.nb;
    const uint32_t chunk = (A.nb + 255u) / 256u;
    const uint32_t b0 = t * chunk < A.nb ? t * chunk : A.nb;
    const uint32_t b1 = b0 + chunk < A.nb ? b0 + chunk : A.nb;
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += row[b];
    part[t] = sum;
    if (t == 0u) s_next = A.cls_next[c];
    __syncthreads();
    if (t == 0u) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < 256u; k++) {
            const uint32_t x = part[k];
            part[k] = run;
            run += x;
        }
        const uint32_t cap = A.cls_cap[c];
        const uint64_t taken = (uint64_t)s_next + run;
        A.cls_next[c] = taken < cap ? (uint32_t)taken : cap;
    }
    __syncthreads();
    uint32_t base = s_next + part[t];
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t x = row[b];
        row[b] = base;
        base += x;
    }
}

extern "C" __global__ __launch_bounds__(MXP_QK_BLOCK) void mxp_qk_assign(mxp_qk_args A) {
    __shared__ unsigned long long s_words[MXP_QK_BLOCK / 64u];
    __shared__ uint32_t s_leaders[MXP_QK_BLOCK / 64u];
    __shared__ unsigned long long s_base;
    const uint32_t i = blockIdx.x * MXP_QK_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool ins = false;
    uint32_t cls = 0, id = 0;
    if (i < A.n && A.role[i] == MXP_QK_LEADER) {
        cls = A.cls[i];
        const uint32_t slot = A.blk_cnt[(uint64_t)cls * A.nb + blockIdx.x] + A.ref[i];
        if (slot < A.cls_cap[cls]) {
            ins = true;
            id = A.cls_base[cls] + slot;
            A.key[i] = id;
        } else {
            A.code[i] = MXP_QUOTA_KEYS_FULL;
            A.count[2] = 1ull;  // (every such lane stores the same word)
        }
    }
    // the pool offsets of a block's new keys from one atomic add of their sum, the key count likewise
    const unsigned long long words = ins ? (unsigned long long)A.words[i] : 0ull;
    unsigned long long incl = words;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long x = __shfl_up(incl, d);
        if (lane >= d) incl += x;
    }
    if (lane == 63u) s_words[wave] = incl;
    const uint32_t wave_leaders = (uint32_t)__popcll(__ballot(ins));
    if (lane == 0u) s_leaders[wave] = wave_leaders;
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long words_all = 0, leaders = 0;
        for (uint32_t w = 0; w < MXP_QK_BLOCK / 64u; w++) {
            words_all += s_words[w];
            leaders += s_leaders[w];
        }
        s_base = leaders ? atomicAdd(A.count + 1, words_all * 8u) : 0ull;
        if (leaders) atomicAdd(A.count, leaders);
    }
    __syncthreads();
    if (!ins) return;
    unsigned long long base = s_base;
    for (uint32_t w = 0; w < wave; w++) base += s_words[w] * 8u;
    const uint64_t at = base + (incl - words) * 8u;  // (8-aligned: the pool starts empty, every key padded)
    const uint64_t* src = (const uint64_t*)A.blob + A.woff[i];
    uint64_t* dst = (uint64_t*)(A.pool + at);
    for (uint32_t k = 0; k < (uint32_t)words; k++) dst[k] = src[k];
    // leaders of one call carry distinct texts the table does not hold: the first empty slot, no compare
    const uint32_t len = A.len[i];
    const uint64_t h = id_hash((const uint8_t*)src, len) & A.hash_mask;
    uint32_t s = (uint32_t)h & A.tmask;
    for (;; s = (s + 1u) & A.tmask) {
        if (vload(&A.ent[s].hkey)) continue;
        if (!atomicCAS(&A.ent[s].hkey, 0ull, h | MXP_QK_OCC)) break;
    }
    A.ent[s].loc = ((at / 8u) << 32) | len;
    A.key_loc[id] = ((at / 8u) << 32) | len;
    A.ent[s].cls = cls;
    A.ent[s].id = id;
}

extern "C" __global__ __launch_bounds__(256) void mxp_qk_follow(mxp_qk_args A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    int32_t code = A.code[i];
    uint32_t key = A.key[i];
    if (A.role[i] == MXP_QK_FOLLOWER) {  // (a leader's words were stored by the launch before)
        const uint32_t l = A.ref[i];
        code = A.code[l];
        key = A.key[l];
        A.code[i] = code;
        A.key[i] = key;
    }
    if (A.eff_amount) A.eff_amount[i] = (code == MXP_QUOTA_OK && key != MXP_QK_NO_KEY) ? A.amount[i] : 0;
}

extern "C" __global__ __launch_bounds__(256) void mxp_qk_answers(mxp_qk_args A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const int32_t code = A.code[i];
    const uint32_t key = A.key[i];
    const int64_t amt = A.amount[i];
    int64_t g = 0, valid = 0;
    uint8_t dup = 0;
    if (code == MXP_QUOTA_NOT_APPLIED) {  // qr == nil: the amount asked, the default duration
        g = amt;
        valid = A.default_valid_ns;
    } else if (code == MXP_QUOTA_OK && key != MXP_QK_NO_KEY) {
        g = A.granted[i];
        if (A.valid_ns) {
            valid = A.valid_ns[i];
            dup = A.dup[i];
        } else {  // memquota.go:146-156: a window alloc that did not fail returns its ValidDuration
            const int64_t vd = A.cls_valid[A.cls[i]];
            valid = (amt > 0 && vd != 0 && (A.best_effort[i] || g > 0)) ? vd : 0;
        }
    }
    A.out[i] = mxp_qk_answer{g, valid, code == MXP_QUOTA_OK ? key : MXP_QK_NO_KEY, (int16_t)code, dup,
                             (uint8_t)(A.failed[i] & 0xFFu)};
}

extern "C" hipError_t mxp_launch_qk_pick(const mxp_qk_args* a, int ids16, hipStream_t s) {
    const dim3 grid((a->n + 255u) / 256u), block(256);
    if (ids16) hipLaunchKernelGGL(mxp_qk_pick_kernel<true>, grid, block, 0, s, *a);
    else hipLaunchKernelGGL(mxp_qk_pick_kernel<false>, grid, block, 0, s, *a);
    return hipGetLastError();
}

// step 0 measure; 1 write + probe; 2 rank, scan, assign, follow; 3 answers
extern "C" hipError_t mxp_launch_qk(const mxp_qk_args* a, int step, hipStream_t s) {
    const dim3 grid((a->n + 255u) / 256u), block(256);
    if (step == 0) {
        hipLaunchKernelGGL(mxp_qk_measure, grid, block, 0, s, *a);
    } else if (step == 1) {
        hipError_t e = hipMemsetAsync(a->btab, 0xFF, ((size_t)a->bmask + 1) * sizeof(mxp_qk_bslot), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(mxp_qk_write, grid, block, 0, s, *a);
        hipLaunchKernelGGL(mxp_qk_probe, grid, block, 0, s, *a);
    } else if (step == 2) {
        hipLaunchKernelGGL(mxp_qk_rank, dim3(a->nb), dim3(MXP_QK_BLOCK), 0, s, *a);
        hipLaunchKernelGGL(mxp_qk_scan, dim3(a->n_cls), dim3(256), 0, s, *a);
        hipLaunchKernelGGL(mxp_qk_assign, dim3(a->nb), dim3(MXP_QK_BLOCK), 0, s, *a);
        hipLaunchKernelGGL(mxp_qk_follow, grid, block, 0, s, *a);
    } else {
        hipLaunchKernelGGL(mxp_qk_answers, grid, block, 0, s, *a);
    }
    return hipGetLastError();
}
