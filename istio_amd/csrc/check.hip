// check.hip -- the fold of a batched Check (include/mxp.h mxp_check_batch): dispatcher.Check's unit
// results combined per request as combineResults does (mixer/pkg/runtime/dispatcher.go:216-236,
// :322-361), over the id list the Resolve's write pass left on the device -- the list's second
// consumer after delta8.hip, and like it a post-pass with lane groups.
//
// What one unit contributes (list.go:68-101, template.gen.go:2153-2202), as the header states it:
//   a code >= 0 (the list kernel's plane word, or a const unit's code): the code with the unit's
//     valid duration and use count;
//   MXP_LISTENTRY_EVAL_ERROR: ProcessCheck returned CheckResult{} and an error, and the result pointer
//     is non-nil (dispatcher.go:227) -- a ZERO result takes part: OK, 0, 0 (flag MXP_CHECK_EVAL_ERROR);
//   MXP_LISTENTRY_NOT_STRING: the type assertion panicked, safeDispatch left res == nil and
//     combineResults skips it (dispatcher.go:332-334) -- nothing (flag MXP_CHECK_UNIT_PANIC).
// Combined (combineResults, adapter/check.go:45-57): the signed minima of the int64 duration and the
// int32 use count over the contributed results; the code of the first non-OK one in dispatch order
// (rules in resolution order, a rule's units in configuration order: the order dispatch issues the
// calls in, dispatcher.go:175-183; the reference collects in completion order, :392-394, so this is
// one of the orders it can produce).  The response (grpcServer.go:160-179): a Resolve error is
// INTERNAL with the defaults; no contribution is the defaults with OK, or INTERNAL after a panic;
// otherwise the combined result, whose code an Eval error beside it does not change.
//
// G lanes fold one request (G = 1, 4, 16 or 64, chosen by the host from ids / requests): the run
// [id_off[q], id_off[q + 1]) is read G consecutive ids a round, coalesced along it, one id per lane;
// a lane walks its rule's unit range, reading for each unit the plane word planes[p][q] or the const
// entry.  A lane keeps the running minima, whether anything contributed, the flag bits and its
// earliest failure as a key (position in the run << 8 | unit index within the rule) with that
// failure's code; the group reduces them with shuffles at the end and its first lane stores the
// 24-byte result -- adjacent groups' results are adjacent.
// A rule with more than 255 units does not fit the key's 8 bits: the plan records that one exists and
// the WIDE instantiations run, whose key is 64 bits (position << 32 | unit index).  Each lane still
// walks its own rule; the fast instantiations carry neither the wider key nor a branch for it.
// The count pass (WRITE = false) stores the results, the records per request and per 256 requests
// (the Resolve's scan kernels turn them into record offsets); the write pass stores the records in
// dispatch order, each round's positions from a group prefix sum over the lanes' counts, carried
// across rounds.  No LDS beyond the block sums, plain vector stores.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "../../include/mxp.h"
#include "check_args.h"

static_assert(sizeof(mxp_check_result) == 24 && sizeof(mxp_check_record) == 24 && sizeof(mxp_check_entry) == 32,
              "the structs as include/mxp.h and check_args.h describe them");

namespace {

__device__ __forceinline__ int32_t unit_code(const mxp_check_args& A, const mxp_check_entry& e, uint32_t q) {
    return e.plane == MXP_CHECK_NO_PLANE ? e.code : A.planes[(uint64_t)e.plane * A.n + q];
}

template <bool IDS16>
__device__ __forceinline__ uint32_t rule_at(const mxp_check_args& A, uint64_t j) {
    if constexpr (IDS16) return ((const uint16_t*)A.ids)[j];
    else return ((const uint32_t*)A.ids)[j];
}

// min of a signed 64-bit value over the group: the two 32-bit halves travel apart and are compared
// as ONE signed 64-bit value (10 s is 1e10 ns, above 2^32: a min per half would mix two durations)
template <uint32_t G>
__device__ __forceinline__ int64_t group_min_i64(int64_t v) {
#pragma unroll
    for (uint32_t off = G / 2u; off; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)(uint64_t)v, (int)off, (int)G);
        const uint32_t hi = __shfl_xor((uint32_t)((uint64_t)v >> 32), (int)off, (int)G);
        const int64_t o = (int64_t)(((uint64_t)hi << 32) | lo);
        if (o < v) v = o;
    }
    return v;
}

// one request folded by the G lanes of a group: its first lane stores the result; returns the
// request's records (every lane of the group)
template <uint32_t G, bool IDS16, bool WIDE>
__device__ __forceinline__ uint32_t check_fold(const mxp_check_args& A, uint32_t q, uint32_t lane) {
    using Key = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
    constexpr uint32_t kShift = WIDE ? 32u : 8u;
    constexpr Key kNone = ~(Key)0;
    const uint32_t lig = lane & (G - 1u);  // lane in group
    mxp_check_result* const out = (mxp_check_result*)A.results + q;
    if (A.status[q] != MXP_RESOLVE_OK) {  // (group-uniform) cr == nil: INTERNAL, the defaults
        if (lig == 0u) *out = mxp_check_result{A.def_dur, A.def_use, MXP_RPC_INTERNAL, 0u, MXP_CHECK_RESOLVE_ERROR};
        return 0u;
    }
    const uint64_t beg = A.id_off[q], end = A.id_off[q + 1u];
    int64_t dur = INT64_MAX;
    int32_t use = INT32_MAX, fcode = 0;
    uint32_t flags = 0, any = 0, nrec = 0;
    Key key = kNone;
    for (uint64_t jb = beg; jb < end; jb += G) {  // (group-uniform trip count)
        const uint64_t j = jb + lig;
        if (j >= end) continue;
        const uint32_t r = rule_at<IDS16>(A, j);
        const uint32_t u0 = A.rule_unit_off[r], u1 = A.rule_unit_off[r + 1u];
        for (uint32_t u = u0; u < u1; u++) {
            const mxp_check_entry e = A.entries[u];
            const int32_t c = unit_code(A, e, q);
            nrec += c != 0 ? 1u : 0u;
            if (c == MXP_LISTENTRY_NOT_STRING) {  // res == nil: skipped
                flags |= MXP_CHECK_UNIT_PANIC;
                continue;
            }
            any = 1u;
            const bool everr = c == MXP_LISTENTRY_EVAL_ERROR;  // CheckResult{}: OK, 0, 0
            if (everr) flags |= MXP_CHECK_EVAL_ERROR;
            const int64_t d = everr ? 0 : e.dur;
            const int32_t w = everr ? 0 : e.use;
            dur = d < dur ? d : dur;
            use = w < use ? w : use;
            if (c > 0 && key == kNone) {  // (a lane's positions only grow: its first failure is its earliest)
                key = ((Key)(j - beg) << kShift) | (Key)(u - u0);
                fcode = c;
            }
        }
    }
    if constexpr (G > 1u) {
        dur = group_min_i64<G>(dur);
#pragma unroll
        for (uint32_t off = G / 2u; off; off >>= 1) {
            const int32_t w = __shfl_xor(use, (int)off, (int)G);
            use = w < use ? w : use;
            const Key k2 = __shfl_xor(key, (int)off, (int)G);
            const int32_t c2 = __shfl_xor(fcode, (int)off, (int)G);
            if (k2 < key) {  // (keys of different lanes differ: the owner of the least supplies the code)
                key = k2;
                fcode = c2;
            }
            flags |= __shfl_xor(flags, (int)off, (int)G);
            any |= __shfl_xor(any, (int)off, (int)G);
            nrec += __shfl_xor(nrec, (int)off, (int)G);
        }
    }
    if (lig == 0u) {
        if (!any)  // cr == nil: the defaults; err != nil after a panic
            *out = mxp_check_result{A.def_dur, A.def_use, (flags & MXP_CHECK_UNIT_PANIC) ? MXP_RPC_INTERNAL : MXP_RPC_OK,
                                    nrec, flags | MXP_CHECK_NO_CHECKS};
        else
            *out = mxp_check_result{dur, use, key != kNone ? fcode : MXP_RPC_OK, nrec, flags};
    }
    return nrec;
}

// the records of one request, in dispatch order, at rec_off[q]
template <uint32_t G, bool IDS16>
__device__ __forceinline__ void check_records(const mxp_check_args& A, uint32_t q, uint32_t lane) {
    const uint32_t lig = lane & (G - 1u);
    if (A.status[q] != MXP_RESOLVE_OK) return;  // (group-uniform)
    uint64_t base = A.rec_off[q];               // the round's first record (group-uniform)
    if (base == A.rec_off[q + 1u]) return;
    mxp_check_record* const recs = (mxp_check_record*)A.recs;
    const uint64_t beg = A.id_off[q], end = A.id_off[q + 1u];
    for (uint64_t jb = beg; jb < end; jb += G) {
        const uint64_t j = jb + lig;
        uint32_t r = 0, u0 = 0, u1 = 0, cnt = 0;
        if (j < end) {
            r = rule_at<IDS16>(A, j);
            u0 = A.rule_unit_off[r];
            u1 = A.rule_unit_off[r + 1u];
        }
        for (uint32_t u = u0; u < u1; u++) cnt += unit_code(A, A.entries[u], q) != 0 ? 1u : 0u;
        uint32_t incl = cnt;  // inclusive prefix over the group's lanes
        if constexpr (G > 1u) {
#pragma unroll
            for (uint32_t off = 1; off < G; off <<= 1) {
                const uint32_t y = __shfl_up(incl, off, (int)G);
                if (lig >= off) incl += y;
            }
        }
        if (cnt) {
            uint64_t at = base + incl - cnt;
            for (uint32_t u = u0; u < u1; u++) {
                const mxp_check_entry e = A.entries[u];
                const int32_t c = unit_code(A, e, q);
                if (c == 0) continue;
                const bool sym = c > 0 && e.plane != MXP_CHECK_NO_PLANE;  // (the messages' %s)
                recs[at++] = mxp_check_record{r, e.unit, c, 0u, sym ? A.vals[(uint64_t)q * A.vstride + e.value_rule] : 0ull};
            }
        }
        if constexpr (G > 1u) base += __shfl(incl, (int)(G - 1u), (int)G);
        else base += incl;
    }
}

// a block takes 256 requests (the scan's tile): group g of its 256 / G takes requests g, g + 256 / G, ...
template <uint32_t G, bool IDS16, bool WRITE, bool WIDE>
__global__ __launch_bounds__(256) void mxp_check_combine_kernel(mxp_check_args A) {
    constexpr uint32_t NG = 256u / G;
    const uint32_t lane = threadIdx.x & 63u, grp = threadIdx.x / G;
    if constexpr (WRITE) {
        for (uint32_t k = 0; k < G; k++) {
            const uint32_t q = blockIdx.x * 256u + k * NG + grp;
            if (q >= A.n) break;  // (group-uniform; later k only larger)
            check_records<G, IDS16>(A, q, lane);
        }
    } else {
        __shared__ uint64_t wsum[4];
        uint64_t mine = 0;
        for (uint32_t k = 0; k < G; k++) {
            const uint32_t q = blockIdx.x * 256u + k * NG + grp;
            if (q >= A.n) break;
            const uint32_t c = check_fold<G, IDS16, WIDE>(A, q, lane);
            if ((lane & (G - 1u)) == 0u) {
                A.rcount[q] = c;
                mine += c;
            }
        }
        for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off);
        if (lane == 0u) wsum[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0u) A.block_sum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

template <uint32_t G, bool IDS16>
void check_launch(const mxp_check_args& a, int write, bool wide, hipStream_t s) {
    const dim3 grid((a.n + 255u) / 256u), block(256);
    if (write) hipLaunchKernelGGL((mxp_check_combine_kernel<G, IDS16, true, false>), grid, block, 0, s, a);
    else if (wide) hipLaunchKernelGGL((mxp_check_combine_kernel<G, IDS16, false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((mxp_check_combine_kernel<G, IDS16, false, false>), grid, block, 0, s, a);
}

template <uint32_t G>
void check_launch(const mxp_check_args& a, int write, bool ids16, bool wide, hipStream_t s) {
    if (ids16) check_launch<G, true>(a, write, wide, s);
    else check_launch<G, false>(a, write, wide, s);
}

}  // namespace

// The lanes per request for lists of `mean` ids, one id per lane and round: the widest of 1, 4, 16,
// 64 that such a list fills four times over -- delta8's thresholds (mxp_d8_group), UNMEASURED for this
// kernel (MXP_CHECK_GROUP: a fixed width, for A/B and tests).
extern "C" uint32_t mxp_check_group(uint64_t mean) {
    if (const char* v = getenv("MXP_CHECK_GROUP")) {
        const int g = atoi(v);
        if (g == 1 || g == 4 || g == 16 || g == 64) return (uint32_t)g;
    }
    uint32_t g = 1;
    while (g < 64u && 4u * (4u * g) <= mean) g <<= 2;
    return g;
}

// write 0: results, records per request + block sums; 1: the records.  group: mxp_check_group's;
// wide: a rule has more than 255 units (the count pass's 64-bit key).
extern "C" hipError_t mxp_launch_check(const mxp_check_args* a, int write, uint32_t group, int ids16, int wide,
                                       hipStream_t s) {
    if (!a->n) return hipSuccess;
    switch (group) {
        case 1: check_launch<1>(*a, write, ids16 != 0, wide != 0, s); break;
        case 4: check_launch<4>(*a, write, ids16 != 0, wide != 0, s); break;
        case 16: check_launch<16>(*a, write, ids16 != 0, wide != 0, s); break;
        case 64: check_launch<64>(*a, write, ids16 != 0, wide != 0, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
