// quota_impl.h -- the batched memquota state shared by quota.cpp (keys, replay) and quota_dedup.cpp
// (DeduplicationID handling).  Not part of the C-ABI.
#pragma once

#include <memory>
#include <vector>

#include "engine_impl.h"

struct mxp_quota_dedup;  // quota_dedup.cpp: created by the first dedup call
struct mxp_quota_dedup_delete {
    void operator()(mxp_quota_dedup* d) const;
};

struct mxp_quota {
    uint32_t n_keys = 0;
    DevBuf max_amount, ticks, cells, avail, win_cur, win_tick, slot_off, slots;
    DevBuf keys_clamped, keys_sorted, idx_in, order, seg_start, tmp, samt, sbe, big, prec, done;
    size_t cap = 0, tmp_bytes = 0, radix_cap = 0, bucket_cap = 0;  // (tmp: the radix sort's or the bucketing's)
    std::vector<int64_t> valid_ns;  // Params_Quota.ValidDuration per key (the dedup calls' ValidDuration)
    std::unique_ptr<mxp_quota_dedup, mxp_quota_dedup_delete> dedup;
};
