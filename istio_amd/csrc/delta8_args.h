// delta8_args.h -- argument block of the delta-coded action list encoder (delta8.hip).
#pragma once

#include <stdint.h>

// MXP_RESOLVE_IDS_DELTA8 (include/mxp.h): a post-pass over the u16 id list the Resolve's write pass
// left on the device.  Kept to a handful of pointers: it rides in SGPRs beside the loop state.
typedef struct mxp_d8_args {
    uint32_t n;              // requests
    uint32_t pad;
    const uint16_t* ids;     // the u16 id list, request by request, in resolution order (8-byte
                             // aligned, 8 bytes of slack behind it: read in 8-byte words)
    const uint64_t* id_off;  // [n + 1] offsets into ids (the Resolve's scan of the counts)
    uint32_t* bcount;        // [n] count pass: bytes of each request's code
    uint64_t* block_sum;     // [ceil(n / 256)] count pass: bytes of each 256 requests
    const uint64_t* boff;    // [n + 1] write pass: byte offsets (the scan of bcount)
    uint8_t* out;            // write pass: the stream
    // a guarded pass (0: unchecked), enqueued before the host knows the totals: the count pass does
    // nothing when the ids exceed this many (the guarded id write pass wrote none), the write pass
    // nothing when the ids or the bytes do
    uint64_t cap;
} mxp_d8_args;
