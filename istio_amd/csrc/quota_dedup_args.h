// quota_dedup_args.h -- argument block of the memquota DeduplicationID kernels (quota_dedup.hip /
// quota_dedup.cpp).
#pragma once

#include <stdint.h>

// exp of a stored result that carries no time (Go's time.Time{}: exp.Sub(now) saturates below 0)
#define MXP_QDD_NO_EXP INT64_MIN
// an occupied slot's hash word: this bit | the id's (masked) hash; 0 = empty
#define MXP_QDD_OCC (1ull << 63)

// request roles (mxp_qdd_probe writes ZERO / HIT / LEADER, mxp_qdd_roles turns the LEADERs that are
// not their slot's lowest arrival index into FOLLOWERs)
enum { MXP_QDD_ZERO = 0, MXP_QDD_HIT = 1, MXP_QDD_LEADER = 2, MXP_QDD_FOLLOWER = 3 };

// One generation of the dedup map (dedupUtil.recentDedup / oldDedup, dedup.go:30-32): an open
// addressing table and the byte pool its ids live in (each id 8-byte aligned, 16 bytes of slack
// behind the pool).  An entry is one 32-byte record, so a probe, a hit's read and an insert each
// touch one cache line of the table (as four arrays an insert dirtied four random lines).
typedef struct mxp_qdd_ent {
    unsigned long long hkey;    // MXP_QDD_OCC | hash, 0 empty
    uint64_t loc;               // pool offset / 8 << 32 | id length
    int64_t amount;             // dedupState.amount
    int64_t exp;                // dedupState.exp in ns, MXP_QDD_NO_EXP
} mxp_qdd_ent;
// a slot of the call's batch table (every byte 0xFF = empty, so one memset clears it): who won the
// slot, and beside it the lowest arrival index among the slot's requests
#define MXP_QDD_BEMPTY (~0ull)
typedef struct mxp_qdd_bslot {
    unsigned long long occ;     // hash tag << 32 | (occupant request + 1); MXP_QDD_BEMPTY
    uint32_t lead;              // atomicMin of the slot's requests' indices
    uint32_t pad;
} mxp_qdd_bslot;

typedef struct mxp_qdd_gen {
    mxp_qdd_ent* ent;           // [mask + 1] (NULL: the generation holds nothing)
    uint8_t* pool;
    unsigned long long* count;  // [0] ids held, [1] pool bytes used
    uint32_t mask;
} mxp_qdd_gen;

typedef struct mxp_qdd_args {
    uint32_t n;                  // requests
    uint32_t n_keys;
    int64_t now_ns;
    uint64_t hash_mask;          // MXP_QDD_HASH_BITS (tests): the id hash is masked before use and storage
    // requests
    const uint32_t* key;
    const int64_t* amount;
    const uint8_t* best_effort;
    const uint8_t* id_bytes;     // 16 readable bytes of slack behind the last id
    const uint32_t* id_off;      // [n + 1]
    mxp_qdd_gen recent, old;
    // the call's batch table (cleared per call): ids of this batch found in neither generation
    mxp_qdd_bslot* btab;         // [bmask + 1]
    uint32_t bmask;
    // per request
    uint32_t* ref;               // HIT: old << 31 | slot; LEADER / FOLLOWER: batch slot, then the leader's index
    uint8_t* role;
    int64_t* eff_amount;         // what the replay sees: the leader's amount, 0 for everyone else
    const int64_t* sgrant;       // the replay's grants of eff_amount
    const int64_t* key_valid_ns; // [n_keys] Params_Quota.ValidDuration
    int64_t* granted;            // QuotaResult.Amount
    int64_t* valid_ns;           // QuotaResult.ValidDuration (nullable)
    uint8_t* dup;                // satisfied through deduplication (nullable)
} mxp_qdd_args;
