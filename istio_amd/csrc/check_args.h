// check_args.h -- argument block and device tables of the batched Check fold (check.hip).
#pragma once

#include <stdint.h>

#define MXP_CHECK_NO_PLANE 0xFFFFFFFFu

// One entry of a rule's unit range as the fold reads it: rule r's are
// entries[rule_unit_off[r] .. rule_unit_off[r + 1]), in configuration order.  32 bytes, two 16-byte loads.
typedef struct __attribute__((aligned(16))) mxp_check_entry {
    int64_t dur;          // the handler's valid duration (ns)
    int32_t use;          // ... and valid use count
    int32_t code;         // a const unit's code
    uint32_t plane;       // a list unit's code plane; MXP_CHECK_NO_PLANE: a const unit
    uint32_t value_rule;  // a list unit's Value expression (rule of the instance engine)
    uint32_t unit;        // index into the plan's units (mxp_check_record.unit)
    uint32_t pad;
} mxp_check_entry;

// A second consumer of the id list the Resolve's write pass left on the device (the first:
// delta8_args.h).  Kept to a handful of pointers and scalars, as there: it rides in SGPRs beside the
// loop state.
typedef struct mxp_check_args {
    uint32_t n;                      // requests
    uint32_t vstride;                // rules of the instance engine: stride of vals
    const void* ids;                 // the selected rules, u16 or u32, request by request, in resolution order
    const uint64_t* id_off;          // [n + 1] offsets into ids
    const uint8_t* status;           // [n] the Resolve's status
    const uint32_t* rule_unit_off;   // [rules + 1]
    const mxp_check_entry* entries;  // [rule_unit_off[rules]]
    const int32_t* planes;           // [planes][n] codes of the list kernel, one plane per distinct
                                     // (value_rule, list, blacklist)
    const uint64_t* vals;            // write pass: [n][vstride] result registers of the instance engine
    uint32_t* rcount;                // count pass: [n] records per request
    uint64_t* block_sum;             // count pass: [ceil(n / 256)] records per 256 requests
    const uint64_t* rec_off;         // write pass: [n + 1] the scan of rcount
    void* results;                   // count pass: [n] mxp_check_result
    void* recs;                      // write pass: mxp_check_record
    int64_t def_dur;                 // the response's defaults when no result is contributed
    int32_t def_use;
    uint32_t pad;
} mxp_check_args;
