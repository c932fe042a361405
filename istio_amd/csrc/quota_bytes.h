// quota_bytes.h -- byte strings hashed and compared a u64 word at a time, shared by the memquota
// DeduplicationID kernels (quota_dedup.hip) and the quota key stage (quota_keys.hip).  Device code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mxp_qbytes {

// ids are hashed and compared 8 bytes at a time: two aligned loads and a funnel shift for an
// unaligned operand, so up to 15 bytes past the last byte are read (the blob's and the pools' slack)
__device__ __forceinline__ uint64_t ld8_any(const uint8_t* p) {
    const uintptr_t a = (uintptr_t)p;
    const uint64_t* q = (const uint64_t*)(a & ~(uintptr_t)7);
    const uint32_t sh = (uint32_t)(a & 7) * 8u;
    const uint64_t lo = q[0];
    return sh == 0 ? lo : (lo >> sh) | (q[1] << (64u - sh));
}
__device__ __forceinline__ uint64_t tail_mask(uint32_t r) { return r >= 8u ? ~0ull : (1ull << (8u * r)) - 1ull; }
__device__ __forceinline__ uint64_t id_hash(const uint8_t* p, uint32_t n) {
    uint64_t h = 0;
    for (uint32_t i = 0; i < n; i += 8) {
        h ^= ld8_any(p + i) & tail_mask(n - i);
        h *= 0x9E3779B97F4A7C15ull;
        h ^= h >> 31;
    }
    h ^= (uint64_t)n * 0xC2B2AE3D27D4EB4Full;
    h *= 0xFF51AFD7ED558CCDull;
    return h ^ (h >> 33);
}
__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t n) {
    for (uint32_t i = 0; i < n; i += 8)
        if ((ld8_any(a + i) ^ ld8_any(b + i)) & tail_mask(n - i)) return false;
    return true;
}

__device__ __forceinline__ unsigned long long vload(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace mxp_qbytes
