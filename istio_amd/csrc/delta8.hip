// delta8.hip -- MXP_RESOLVE_IDS_DELTA8 (include/mxp.h): the Resolve's u16 id list, left on the
// device by the write pass, coded as a gap byte stream with an escape.
//
// Each request is coded alone, prev = -1: d = r - prev - 1 as one byte when 0 <= d <= 254, else
// 0xFF and the absolute id, little-endian (a gap above 254, or the backward step from the default
// namespace's range to the request's own).  An id's byte position inside its request is its index
// in the list plus two for every escape before it.
//
// G lanes code one request (G a power of two, 1..64, chosen by the host from ids / requests): the
// list is read 4 * G ids at a time, coalesced along it, four consecutive ids per lane; a lane's
// first id takes its predecessor from the neighbouring lane (the first lane's from the previous
// iteration's last id); the escapes before an id are ballots masked to the group and popcounts, plus
// the group's running count.  No lane walks a list.
// The count pass leaves bytes per request and per 256 requests (the Resolve's scan kernels turn
// them into byte offsets), the write pass stores the stream -- plain byte stores.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "delta8_args.h"

namespace {

constexpr uint32_t kD8Ids = 4;  // ids per lane and iteration: one 8-byte load

// one request by the G lanes of a group; returns the bytes of its code (every lane of the group).
// An iteration takes 4 * G ids, lane l the four at 4 * l: the list is read in 8-byte words aligned in
// the whole id list (so the first word may start before the request and the last end after it:
// those ids are masked, and the list has 8 bytes of slack behind it).  One id per lane and
// iteration spent ~50 instructions on every 64 ids -- the shuffles, the ballot, the addressing --
// and the kernels were bound by instruction issue at 1.4 TB/s.
template <uint32_t G, bool WRITE>
__device__ __forceinline__ uint32_t d8_request(const mxp_d8_args& A, uint32_t q, uint32_t lane) {
    const uint32_t lig = lane & (G - 1u);  // lane in group
    const uint64_t beg = A.id_off[q], end = A.id_off[q + 1u];
    if (beg == end) return 0u;  // (group-uniform)
    uint8_t* __restrict__ out = WRITE ? A.out + A.boff[q] : nullptr;
    const uint64_t low = (1ull << lig) - 1ull;  // the lanes of the group before this one
    auto group_bits = [&](uint64_t ballot) -> uint64_t {  // bit = lane in group
        if constexpr (G == 64u) return ballot;
        else return (ballot >> (lane & ~(G - 1u))) & ((1ull << G) - 1ull);
    };
    uint32_t esc = 0;   // escapes before this iteration (group-uniform)
    int32_t last = -1;  // the previous iteration's last id (group-uniform)
    for (uint64_t jb = beg & ~(uint64_t)(kD8Ids - 1u); jb < end; jb += kD8Ids * G) {  // (group-uniform trip count)
        const uint64_t j0 = jb + lig * kD8Ids;
        uint2 w = make_uint2(0u, 0u);
        if (j0 < end) w = *(const uint2*)(A.ids + j0);
        const int32_t r[kD8Ids] = {(int32_t)(w.x & 0xFFFFu), (int32_t)(w.x >> 16), (int32_t)(w.y & 0xFFFFu),
                                   (int32_t)(w.y >> 16)};
        int32_t prev = last;  // the id before r[0]: the lane before's last one
        if constexpr (G > 1u) {
            const int32_t up = __shfl_up(r[kD8Ids - 1u], 1, (int)G);
            if (lig) prev = up;
        }
        bool v[kD8Ids], e[kD8Ids];
        uint32_t d[kD8Ids], cnt = 0;
#pragma unroll
        for (uint32_t s = 0; s < kD8Ids; s++) {
            const uint64_t j = j0 + s;
            v[s] = j >= beg && j < end;
            const int32_t p = j == beg ? -1 : s ? r[s - 1u] : prev;  // (each request alone: prev = -1)
            d[s] = (uint32_t)(r[s] - p - 1);  // (a backward step wraps far above 254)
            e[s] = v[s] && d[s] > 254u;
            cnt += e[s] ? 1u : 0u;
        }
        // escapes of this iteration before this lane's ids, and in the whole group (most iterations
        // have none: one ballot then)
        uint32_t below = 0, tot = 0;
        bool any;
        if constexpr (G > 1u) any = group_bits(__ballot(cnt != 0u)) != 0ull;
        else any = cnt != 0u;
        if (any) {  // (group-uniform)
            if constexpr (G > 1u) {
#pragma unroll
                for (uint32_t s = 0; s < kD8Ids; s++) {
                    const uint64_t gm = group_bits(__ballot(e[s]));
                    below += (uint32_t)__popcll(gm & low);
                    tot += (uint32_t)__popcll(gm);
                }
            } else {
                tot = cnt;
            }
        }
        if constexpr (WRITE) {
            uint32_t run = esc + below;
#pragma unroll
            for (uint32_t s = 0; s < kD8Ids; s++) {
                if (!v[s]) continue;
                uint8_t* p = out + (j0 + s - beg) + 2u * run;
                if (e[s]) {
                    p[0] = 0xFFu;
                    p[1] = (uint8_t)(r[s] & 0xFF);
                    p[2] = (uint8_t)(r[s] >> 8);
                    run++;
                } else {
                    p[0] = (uint8_t)d[s];
                }
            }
        }
        esc += tot;
        if constexpr (G > 1u) last = __shfl(r[kD8Ids - 1u], (int)(G - 1u), (int)G);
        else last = r[kD8Ids - 1u];
    }
    return (uint32_t)(end - beg) + 2u * esc;
}

// a block takes 256 requests (the scan's tile): group g of its 256 / G takes requests g, g + 256 / G, ...
template <uint32_t G>
__global__ __launch_bounds__(256) void mxp_d8_count_kernel(mxp_d8_args A) {
    __shared__ uint64_t wsum[4];
    if (A.cap && A.id_off[A.n] > A.cap) return;  // (uniform per launch)
    constexpr uint32_t NG = 256u / G;
    const uint32_t lane = threadIdx.x & 63u, grp = threadIdx.x / G;
    uint64_t mine = 0;
    for (uint32_t k = 0; k < G; k++) {
        const uint32_t q = blockIdx.x * 256u + k * NG + grp;
        if (q >= A.n) break;  // (group-uniform; later k only larger)
        const uint32_t b = d8_request<G, false>(A, q, lane);
        if ((lane & (G - 1u)) == 0u) {
            A.bcount[q] = b;
            mine += b;
        }
    }
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0u) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0u) A.block_sum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

template <uint32_t G>
__global__ __launch_bounds__(256) void mxp_d8_write_kernel(mxp_d8_args A) {
    if (A.cap && (A.id_off[A.n] > A.cap || A.boff[A.n] > A.cap)) return;  // (uniform per launch)
    constexpr uint32_t NG = 256u / G;
    const uint32_t lane = threadIdx.x & 63u, grp = threadIdx.x / G;
    for (uint32_t k = 0; k < G; k++) {
        const uint32_t q = blockIdx.x * 256u + k * NG + grp;
        if (q >= A.n) break;
        (void)d8_request<G, true>(A, q, lane);
    }
}

template <uint32_t G>
void d8_launch(const mxp_d8_args& a, int write, hipStream_t s) {
    const uint32_t grid = (a.n + 255u) / 256u;
    if (write) hipLaunchKernelGGL(mxp_d8_write_kernel<G>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(mxp_d8_count_kernel<G>, dim3(grid), dim3(256), 0, s, a);
}

}  // namespace

// The lanes per request for lists of `mean` ids, four ids per lane and iteration: the largest power
// of two whose iteration such a list fills, 64 at most (MXP_D8_GROUP: a fixed width, for A/B and tests).
extern "C" uint32_t mxp_d8_group(uint64_t mean) {
    if (const char* v = getenv("MXP_D8_GROUP")) {
        const int g = atoi(v);
        if (g >= 1 && g <= 64 && (g & (g - 1)) == 0) return (uint32_t)g;
    }
    uint32_t g = 1;
    while (g < 64u && 2u * g * 4u <= mean) g <<= 1;
    return g;
}

// write 0: bytes per request + block sums; 1: the stream.  group: mxp_d8_group's.
extern "C" hipError_t mxp_launch_d8(const mxp_d8_args* a, int write, uint32_t group, hipStream_t s) {
    if (!a->n) return hipSuccess;
    switch (group) {
        case 1: d8_launch<1>(*a, write, s); break;
        case 2: d8_launch<2>(*a, write, s); break;
        case 4: d8_launch<4>(*a, write, s); break;
        case 8: d8_launch<8>(*a, write, s); break;
        case 16: d8_launch<16>(*a, write, s); break;
        case 32: d8_launch<32>(*a, write, s); break;
        case 64: d8_launch<64>(*a, write, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
