// quota_dedup.hip -- memquota's DeduplicationID handling (mixer/adapter/memquota/dedup.go:61-116)
// around the batched replay of quota.hip.
//
// handleDedup looks the request's id up in two generations of a handler-wide map and runs the quota
// function only on a miss, storing its result.  For a batch taken in arrival order that is: requests
// whose id a generation holds are answered from it (HIT); of the others, the lowest arrival index of
// each id is replayed (LEADER) and every later one gets the leader's result (FOLLOWER).  The replay
// treats amount 0 as nothing (memquota.go:107-116), so the passes here run before and after it:
//   mxp_qdd_probe   lane = request: hash the id, probe recent then old, else elect in the batch table
//   mxp_qdd_roles   lane = request: leader or follower, the amounts the replay sees
//   (mxp_quota_alloc_device on those amounts, into scratch grants)
//   mxp_qdd_finish  lane = request: the answers by role; leaders insert into `recent`
// Kernel boundaries order everything between waves: no kernel reads what another wave of the same
// launch stored plainly.  Words a launch CASes are read with relaxed agent-scope atomic loads, which
// stay on the vector memory path (a plain load of a wave-uniform address may be served by the scalar
// cache, which does not see the vector path's writes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quota_bytes.h"
#include "quota_dedup_args.h"

namespace {

using namespace mxp_qbytes;  // ld8_any, tail_mask, id_hash, same_bytes, vload

// the slot of `G` that holds the id, or ~0 (stored hash first, then length, then bytes)
__device__ __forceinline__ uint32_t gen_find(const mxp_qdd_gen& G, unsigned long long hk, uint32_t start,
                                             const uint8_t* p, uint32_t len) {
    if (!G.ent) return ~0u;
    for (uint32_t s = start & G.mask;; s = (s + 1u) & G.mask) {  // (at most half full: an empty slot ends it)
        const unsigned long long e = G.ent[s].hkey;
        if (!e) return ~0u;
        if (e != hk) continue;
        const uint64_t loc = G.ent[s].loc;
        if ((uint32_t)loc != len) continue;
        if (same_bytes(p, G.pool + (loc >> 32) * 8u, len)) return s;
    }
}

// ValidDuration and exp of a replayed request (memquota.go:146-156: a window alloc that did not
// fail returns currentTime.Add(ValidDuration); cells, frees and a failed plain alloc a zero time)
__device__ __forceinline__ int64_t replayed_valid(const mxp_qdd_args& A, uint32_t i, int64_t g) {
    const uint32_t k = A.key[i];
    if (k >= A.n_keys || A.amount[i] <= 0) return 0;
    const int64_t vd = A.key_valid_ns[k];
    return (vd != 0 && (A.best_effort[i] || g > 0)) ? vd : 0;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void mxp_qdd_probe(mxp_qdd_args A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    if (A.amount[i] == 0) {  // HandleQuota returns before handleDedup (memquota.go:107-116)
        A.role[i] = MXP_QDD_ZERO;
        return;
    }
    const uint32_t o = A.id_off[i], len = A.id_off[i + 1] - o;
    const uint8_t* p = A.id_bytes + o;
    const uint64_t h = id_hash(p, len) & A.hash_mask;
    const unsigned long long hk = h | MXP_QDD_OCC;
    uint32_t s = gen_find(A.recent, hk, (uint32_t)h, p, len);  // dedup.go:73-76
    uint32_t old = 0;
    if (s == ~0u) {
        s = gen_find(A.old, hk, (uint32_t)h, p, len);
        old = 1u << 31;
    }
    if (s != ~0u) {
        A.role[i] = MXP_QDD_HIT;
        A.ref[i] = old | s;
        return;
    }
    // a miss: every request of the batch with this id ends on one slot of the batch table (the
    // occupant is whoever won the CAS; the lowest arrival index is kept beside it, in the same line)
    const uint64_t tag = h >> 32;
    const unsigned long long mine = (tag << 32) | (i + 1u);
    for (s = (uint32_t)h & A.bmask;; s = (s + 1u) & A.bmask) {
        unsigned long long e = vload(&A.btab[s].occ);
        if (e == MXP_QDD_BEMPTY) {
            e = atomicCAS(&A.btab[s].occ, MXP_QDD_BEMPTY, mine);
            if (e == MXP_QDD_BEMPTY) break;
        }
        if ((e >> 32) != tag) continue;
        const uint32_t other = (uint32_t)e - 1u;
        const uint32_t oo = A.id_off[other];
        if (A.id_off[other + 1] - oo == len && same_bytes(p, A.id_bytes + oo, len)) break;
    }
    atomicMin(&A.btab[s].lead, i);
    A.role[i] = MXP_QDD_LEADER;
    A.ref[i] = s;
}

extern "C" __global__ __launch_bounds__(256) void mxp_qdd_roles(mxp_qdd_args A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    int64_t eff = 0;
    if (A.role[i] == MXP_QDD_LEADER) {
        const uint32_t l = A.btab[A.ref[i]].lead;
        A.ref[i] = l;
        if (l == i) eff = A.amount[i];
        else A.role[i] = MXP_QDD_FOLLOWER;
    }
    A.eff_amount[i] = eff;
}

// (1,024 lanes a block: the pool offsets and the id count are two atomic adds on two words that every
// block of the launch shares.  Drawn per wave -- 16k waves for 1M requests, ~11 ns per same-address
// atomic as in pack.hip's intern pass -- they made this kernel 0.436 ms on the C5 batch; drawn per
// block of 16 waves, 0.148 ms: profiles/quota_dedup_ab.log.)
constexpr uint32_t kFinishBlock = 1024;
extern "C" __global__ __launch_bounds__(kFinishBlock) void mxp_qdd_finish(mxp_qdd_args A) {
    __shared__ unsigned long long s_words[kFinishBlock / 64];
    __shared__ uint32_t s_leaders[kFinishBlock / 64];
    __shared__ unsigned long long s_base;
    const uint32_t i = blockIdx.x * kFinishBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool in = i < A.n;
    const uint32_t role = in ? A.role[i] : (uint32_t)MXP_QDD_ZERO;
    const int64_t amt = in ? A.amount[i] : 0;
    int64_t g = 0, valid = 0, exp = MXP_QDD_NO_EXP;
    if (role == MXP_QDD_HIT) {
        const uint32_t r = A.ref[i];
        const mxp_qdd_gen& G = (r >> 31) ? A.old : A.recent;
        g = G.ent[r & 0x7FFFFFFFu].amount;
        exp = G.ent[r & 0x7FFFFFFFu].exp;
    } else if (role == MXP_QDD_LEADER || role == MXP_QDD_FOLLOWER) {
        const uint32_t l = A.ref[i];  // (a leader's own index)
        g = A.sgrant[l];
        const int64_t vd = replayed_valid(A, l, g);
        if (vd) exp = A.now_ns + vd;
    }
    // an alloc's ValidDuration: the replayed one, or max(0, exp - now) of the stored result
    // (dedup.go:78-83); a free returns none (memquota.go:171, 207-210)
    if (amt > 0 && exp != MXP_QDD_NO_EXP && exp > A.now_ns) valid = exp - A.now_ns;
    if (in) {
        A.granted[i] = g;
        if (A.valid_ns) A.valid_ns[i] = valid;
        if (A.dup) A.dup[i] = role == MXP_QDD_HIT || role == MXP_QDD_FOLLOWER;
    }
    // leaders store their result in `recent` (dedup.go:86).  The pool offsets of a block's ids come
    // from one atomic add of their sum (the waves' sums through LDS, a lane prefix inside each wave),
    // the id count likewise.
    const bool ins = role == MXP_QDD_LEADER;
    uint32_t o = 0, len = 0;
    if (ins) {
        o = A.id_off[i];
        len = A.id_off[i + 1] - o;
    }
    const unsigned long long words = ins ? ((unsigned long long)len + 7u) / 8u : 0ull;
    unsigned long long incl = words;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63u) s_words[wave] = incl;
    const uint32_t wave_leaders = (uint32_t)__popcll(__ballot(ins));
    if (lane == 0) s_leaders[wave] = wave_leaders;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long words_all = 0, leaders = 0;
        for (uint32_t w = 0; w < kFinishBlock / 64; w++) {
            words_all += s_words[w];
            leaders += s_leaders[w];
        }
        s_base = leaders ? atomicAdd(A.recent.count + 1, words_all * 8u) : 0ull;
        if (leaders) atomicAdd(A.recent.count, leaders);
    }
    __syncthreads();
    if (!ins) return;
    unsigned long long base = s_base;
    for (uint32_t w = 0; w < wave; w++) base += s_words[w] * 8u;
    const uint64_t at = base + (incl - words) * 8u;  // (8-aligned: the pool starts empty, every id padded)
    const uint8_t* p = A.id_bytes + o;
    uint64_t* dst = (uint64_t*)(A.recent.pool + at);
    for (uint32_t b = 0; b < len; b += 8) dst[b / 8u] = ld8_any(p + b) & tail_mask(len - b);
    // leaders of one batch carry distinct ids that `recent` does not hold: the first empty slot, no compare
    const uint64_t h = id_hash(p, len) & A.hash_mask;
    const unsigned long long hk = h | MXP_QDD_OCC;
    uint32_t s = (uint32_t)h & A.recent.mask;
    for (;; s = (s + 1u) & A.recent.mask) {
        if (vload(&A.recent.ent[s].hkey)) continue;
        if (!atomicCAS(&A.recent.ent[s].hkey, 0ull, hk)) break;
    }
    A.recent.ent[s].loc = ((at / 8u) << 32) | len;
    A.recent.ent[s].amount = g;
    A.recent.ent[s].exp = exp;
}

// growth: the entries of `from` reinserted into the (empty, larger) table `to` by their stored hash;
// the pool is copied as it is, so the locations stay
extern "C" __global__ __launch_bounds__(256) void mxp_qdd_rehash(mxp_qdd_gen from, mxp_qdd_gen to) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > from.mask) return;
    const mxp_qdd_ent e = from.ent[i];
    if (!e.hkey) return;
    uint32_t s = (uint32_t)e.hkey & to.mask;
    for (;; s = (s + 1u) & to.mask) {
        if (vload(&to.ent[s].hkey)) continue;
        if (!atomicCAS(&to.ent[s].hkey, 0ull, e.hkey)) break;
    }
    to.ent[s].loc = e.loc;
    to.ent[s].amount = e.amount;
    to.ent[s].exp = e.exp;
}

extern "C" hipError_t mxp_launch_qdd_probe(const mxp_qdd_args* a, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a->btab, 0xFF, ((size_t)a->bmask + 1) * sizeof(mxp_qdd_bslot), s);
    if (e != hipSuccess) return e;
    const uint32_t grid = (a->n + 255u) / 256u;
    hipLaunchKernelGGL(mxp_qdd_probe, dim3(grid), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(mxp_qdd_roles, dim3(grid), dim3(256), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t mxp_launch_qdd_finish(const mxp_qdd_args* a, hipStream_t s) {
    hipLaunchKernelGGL(mxp_qdd_finish, dim3((a->n + kFinishBlock - 1) / kFinishBlock), dim3(kFinishBlock), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t mxp_launch_qdd_rehash(const mxp_qdd_gen* from, const mxp_qdd_gen* to, hipStream_t s) {
    hipLaunchKernelGGL(mxp_qdd_rehash, dim3(from->mask / 256u + 1u), dim3(256), 0, s, *from, *to);
    return hipGetLastError();
}
