// quota_keys_args.h -- device tables and argument block of the quota key stage (quota_keys.hip /
// quota_keys.cpp): from a Resolve's id lists and an instance engine's result registers to memquota's
// key ids (include/mxp.h mxp_quota_batch).
#pragma once

#include <stdint.h>

#define MXP_QK_NO_KEY 0xFFFFFFFFu
#define MXP_QK_NO_CLASS 0xFFFFFFFFu
#define MXP_QK_MAX_CLASSES 256u  // the per-class leader counts of a 1,024-lane block live in LDS
#define MXP_QK_BLOCK 1024u       // lanes per block of the rank / assign passes
// an occupied slot's hash word: this bit | the key's (masked) hash; 0 = empty
#define MXP_QK_OCC (1ull << 63)
#define MXP_QK_BEMPTY (~0ull)

// request roles after the probe (HIT: the persistent table holds the key) and the rank pass (a
// CANDIDATE becomes the LEADER of its key -- the lowest arrival index -- or its FOLLOWER)
enum { MXP_QK_NONE = 0, MXP_QK_HIT = 1, MXP_QK_LEADER = 2, MXP_QK_FOLLOWER = 3 };

// A unit: one quota instance.  Its dimensions are dims[dim_off .. dim_off + n_dims) in sort.Strings
// order of their labels; its limit's overrides are ovrs[ovr_off .. ovr_off + n_ovr) in configuration order.
typedef struct mxp_qk_unit {
    uint32_t dim_off, n_dims;
    uint32_t name_off, name_len;  // instance name in `text`
    uint32_t cls_default;         // class of (limit, default)
    uint32_t ovr_off, n_ovr;
    uint32_t fixed_len;           // name + per dimension ';' label '='
} mxp_qk_unit;
typedef struct mxp_qk_dim {
    uint32_t value_rule;          // rule of the instance engine
    uint32_t kind;                // static kind (mxp_kind), 0: interface-typed, decided per request
    uint32_t label_off, label_len;
    uint32_t bit;                 // the label's index in the unit as configured (bit of the failed mask)
    uint32_t pad;
} mxp_qk_dim;
// An override as one unit sees it: every configured dimension names one of the unit's (never = 1
// when the unit lacks a configured label: rval == nil matches nothing)
typedef struct mxp_qk_ovr {
    uint32_t cond_off, n_cond;
    uint32_t cls;
    uint32_t never;
} mxp_qk_ovr;
typedef struct mxp_qk_cond {
    uint32_t dim;                 // index into dims
    uint32_t val_off, val_len;    // configured string in `text`
    uint32_t pad;
} mxp_qk_cond;

// persistent table entry (key bytes -> class, id), keys in a byte pool, each 8-byte aligned
typedef struct mxp_qk_ent {
    unsigned long long hkey;      // MXP_QK_OCC | hash, 0 empty
    uint64_t loc;                 // pool offset / 8 << 32 | key length
    uint32_t cls, id;
} mxp_qk_ent;
typedef struct mxp_qk_bslot {
    unsigned long long occ;       // hash tag << 32 | (occupant request + 1); MXP_QK_BEMPTY
    uint32_t lead;                // atomicMin of the slot's requests' indices
    uint32_t pad;
} mxp_qk_bslot;

// the 24-byte answer (include/mxp.h mxp_quota_answer)
typedef struct mxp_qk_answer {
    int64_t granted, valid_ns;
    uint32_t key;
    int16_t code;
    uint8_t dup, failed;
} mxp_qk_answer;

typedef struct mxp_qk_args {
    uint32_t n;                   // requests
    uint32_t vstride;             // rules of the instance engine: stride of vals
    // pick: the Resolve's outputs on the device
    const void* ids;              // selected rules, u16 or u32, in resolution order
    const uint64_t* id_off;       // [n + 1]
    const uint8_t* status;        // [n]
    const uint8_t* skip;          // [n] nullable
    const uint32_t* rule_unit;    // [rules]
    // the instance evaluation
    const uint64_t* vals;         // [n][vstride] result registers
    const uint32_t* err;          // [ceil(vstride / 32)][n] error bitmap
    uint64_t n_gstr;
    const uint64_t* gstr_off;     // offset << 24 | length (8-aligned pools, 16 bytes of slack)
    const uint8_t* gstr;
    const uint64_t* bstr_off;
    const uint8_t* bstr;
    // []byte values (vm.h MXP_BYTES_RAW): raw ids < n_gb in the instance rule set's pool (the plan's
    // device copy), the others batch-local -- the host packer's overlay pool (ob), or for a
    // device-packed batch (dev_packed) batch string j < ns, else the parsed ip() value 16 (j - ns) in pip
    uint64_t n_gb;
    const uint64_t* gb_off;       // offset << 24 | length
    const uint8_t* gb;
    const uint64_t* ob_off;
    const uint8_t* ob;
    uint64_t n_ob;
    const uint8_t* pip;           // nullable
    uint32_t dev_packed;
    uint32_t ns;
    // the plan
    const mxp_qk_unit* units;
    const mxp_qk_dim* dims;
    const mxp_qk_ovr* ovrs;
    const mxp_qk_cond* conds;
    const uint8_t* text;          // 16 bytes of slack
    uint32_t n_units, n_cls;
    const uint32_t* cls_base;     // [n_cls] first id
    const uint32_t* cls_cap;      // [n_cls] ids
    uint32_t* cls_next;           // [n_cls] ids taken (persistent)
    const int64_t* cls_valid;     // [n_cls] ValidDuration
    // per request
    const uint32_t* unit_in;      // [n] the unit (MXP_QUOTA_NO_UNIT: none)
    uint32_t* unit;               // pick's output (= unit_in for the stage alone)
    const int64_t* amount;
    uint32_t* len;                // key bytes (0 with no key)
    uint32_t* words;              // ceil(len / 8): what the scan sums
    uint32_t* cls;                // MXP_QK_NO_CLASS: no key
    int32_t* code;
    uint32_t* failed;
    uint32_t* key;
    uint64_t* block_sum;          // [ceil(n / 256)] words per 256 requests
    const uint64_t* woff;         // [n + 1] the scan of words
    uint8_t* blob;                // the call's key bytes (woff * 8), 16 bytes of slack
    // the persistent table
    mxp_qk_ent* ent;              // [tmask + 1], at most half full
    uint32_t tmask;
    uint32_t bmask;
    uint8_t* pool;
    unsigned long long* count;    // [0] keys held, [1] pool bytes used
    uint64_t* key_loc;            // [sum of key_cap] an id's pool offset / 8 << 32 | length (~0: not interned)
    uint64_t hash_mask;           // MXP_QKEY_HASH_BITS
    mxp_qk_bslot* btab;           // [bmask + 1] the call's batch table
    uint32_t* ref;                // HIT: slot; CANDIDATE: batch slot; LEADER: rank in block; FOLLOWER: leader
    uint8_t* role;
    uint32_t* blk_cnt;            // [n_cls][nb] leaders per class and block, then their exclusive scan
    uint32_t nb;                  // blocks of MXP_QK_BLOCK requests
    uint32_t pad;
    // answers
    const uint8_t* best_effort;
    int64_t* eff_amount;          // what the replay sees
    const int64_t* granted;
    const int64_t* valid_ns;      // the dedup replay's (nullable: from cls_valid)
    const uint8_t* dup;           // nullable
    int64_t default_valid_ns;
    mxp_qk_answer* out;
} mxp_qk_args;
