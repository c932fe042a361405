// quota_key_fmt.h -- the bytes memquota's makeKey writes for a non-string dimension value
// (mixer/adapter/memquota/keys.go:52-64), for the device's key stage (quota_keys.hip) and, compiled
// for the host, for tests/quota_key_host.cpp.
//
// keys.go appends to bytes[:] of a zeroed [32]byte -- a slice of LENGTH 32 -- so every formatted
// int64, float64 and bool is preceded by 32 NUL bytes:
//   int64    strconv.AppendInt(v, 16): lowercase hex of the magnitude, '-' first for negatives
//   float64  strconv.AppendFloat(v, 'b', -1, 64): [-]mantissa 'p' (+|-)exponent, both decimal
//            (ftoa.go: Inf and NaN are settled before the format is looked at: +Inf, -Inf, NaN;
//            fmtB: the 53-bit mantissa with its hidden bit, the exponent less the bias and the 52
//            mantissa bits; a subnormal has exponent field 1 and no hidden bit)
//   bool     strconv.AppendBool: true / false
// The functions emit the bytes in order through a sink (`void operator()(uint8_t)`); mxp_qk_len is
// the count alone.  No per-lane byte arrays (they would live in scratch): hex digits come from
// shifts, decimal digits most significant first by repeated subtraction of a power of ten.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MXP_QK_HD __host__ __device__ inline
#else
#define MXP_QK_HD inline
#endif

#define MXP_QK_PAD 32u  // len(bytes[:]) of keys.go's [32]byte

// kinds of a formatted value (the engine's mxp_kind numbers)
#define MXP_QK_INT64 2u
#define MXP_QK_DOUBLE 3u
#define MXP_QK_BOOL 4u

MXP_QK_HD uint64_t mxp_qk_pow10(uint32_t k) {  // k <= 19
    static constexpr uint64_t kPow10[20] = {1ull,
                                            10ull,
                                            100ull,
                                            1000ull,
                                            10000ull,
                                            100000ull,
                                            1000000ull,
                                            10000000ull,
                                            100000000ull,
                                            1000000000ull,
                                            10000000000ull,
                                            100000000000ull,
                                            1000000000000ull,
                                            10000000000000ull,
                                            100000000000000ull,
                                            1000000000000000ull,
                                            10000000000000000ull,
                                            100000000000000000ull,
                                            1000000000000000000ull,
                                            10000000000000000000ull};
    return kPow10[k];
}

// decimal digits of u
MXP_QK_HD uint32_t mxp_qk_dec_digits(uint64_t u) {
    uint32_t k = 1;
    while (k < 20u && u >= mxp_qk_pow10(k)) k++;
    return k;
}

template <class Sink>
MXP_QK_HD void mxp_qk_dec(uint64_t u, Sink& put) {
    for (uint32_t k = mxp_qk_dec_digits(u); k-- > 0u;) {
        const uint64_t p = mxp_qk_pow10(k);
        uint32_t d = 0;
        while (u >= p) {  // (at most 9 rounds)
            u -= p;
            d++;
        }
        put((uint8_t)('0' + d));
    }
}

MXP_QK_HD uint32_t mxp_qk_hex_digits(uint64_t u) {
    uint32_t k = 1;
    while (k < 16u && (u >> (4u * k)) != 0ull) k++;
    return k;
}

// the float's 'b' form in pieces: special 1 +Inf, 2 -Inf, 3 NaN, else 0 with mant / exp / neg
struct mxp_qk_float {
    uint64_t mant;
    int32_t exp;
    uint32_t neg, special;
};
MXP_QK_HD mxp_qk_float mxp_qk_split(uint64_t bits) {
    mxp_qk_float f;
    f.neg = (uint32_t)(bits >> 63);
    f.mant = bits & ((1ull << 52) - 1ull);
    int32_t e = (int32_t)((bits >> 52) & 0x7FFu);
    f.special = 0;
    if (e == 0x7FF) f.special = f.mant ? 3u : (f.neg ? 2u : 1u);
    if (e == 0) e = 1;  // subnormal
    else f.mant |= 1ull << 52;
    f.exp = e - 1023 - 52;
    return f;
}

// bytes mxp_qk_fmt emits for a value of `kind` held as `bits` (an int64, a double's bits, a bool)
MXP_QK_HD uint32_t mxp_qk_len(uint32_t kind, uint64_t bits) {
    if (kind == MXP_QK_BOOL) return MXP_QK_PAD + ((uint32_t)bits != 0u ? 4u : 5u);
    if (kind == MXP_QK_INT64) {
        const bool neg = (int64_t)bits < 0;
        const uint64_t u = neg ? 0ull - bits : bits;
        return MXP_QK_PAD + (neg ? 1u : 0u) + mxp_qk_hex_digits(u);
    }
    const mxp_qk_float f = mxp_qk_split(bits);
    if (f.special) return MXP_QK_PAD + (f.special == 3u ? 3u : 4u);
    const uint32_t ae = (uint32_t)(f.exp < 0 ? -f.exp : f.exp);
    return MXP_QK_PAD + f.neg + mxp_qk_dec_digits(f.mant) + 2u + mxp_qk_dec_digits(ae);
}

template <class Sink>
MXP_QK_HD void mxp_qk_text(const char* s, Sink& put) {
    for (; *s; s++) put((uint8_t)*s);
}

template <class Sink>
MXP_QK_HD void mxp_qk_fmt(uint32_t kind, uint64_t bits, Sink& put) {
    for (uint32_t i = 0; i < MXP_QK_PAD; i++) put((uint8_t)0);
    if (kind == MXP_QK_BOOL) {
        mxp_qk_text((uint32_t)bits != 0u ? "true" : "false", put);
        return;
    }
    if (kind == MXP_QK_INT64) {
        const bool neg = (int64_t)bits < 0;
        const uint64_t u = neg ? 0ull - bits : bits;
        if (neg) put((uint8_t)'-');
        for (uint32_t k = mxp_qk_hex_digits(u); k-- > 0u;) {
            const uint32_t d = (uint32_t)(u >> (4u * k)) & 15u;
            put((uint8_t)(d < 10u ? '0' + d : 'a' + (d - 10u)));
        }
        return;
    }
    const mxp_qk_float f = mxp_qk_split(bits);
    if (f.special) {
        mxp_qk_text(f.special == 3u ? "NaN" : f.special == 2u ? "-Inf" : "+Inf", put);
        return;
    }
    if (f.neg) put((uint8_t)'-');
    mxp_qk_dec(f.mant, put);
    put((uint8_t)'p');
    put((uint8_t)(f.exp < 0 ? '-' : '+'));
    mxp_qk_dec((uint64_t)(f.exp < 0 ? -f.exp : f.exp), put);
}
