// out_ranges.hpp -- where each LD block's results lie in the caller's arrays (host only, no HIP).
//
// beta_s and beta_l are CSR by block (s_ptr / l_ptr), so the results of one block are one
// contiguous range of each and one status entry.  A streamed run (dbslmm_options.stream_out)
// copies finished blocks out of the plan's host-visible mirror one by one with this table; the
// non-empty blocks appear in block order, which is the order of the plan's route blocks.
#pragma once
#include <stdint.h>

#include <vector>

struct OutRange {
    int64_t s0, s1;   // beta_s[s0 .. s1): the block's small SNPs
    int64_t l0, l1;   // beta_l[l0 .. l1): its large SNPs (empty without l_ptr)
    int32_t blk;      // its original block id (the status entry)
};

// One entry per non-empty block; false when the offsets are not monotone.
inline bool build_out_ranges(int32_t num_block, const int64_t* s_ptr, const int64_t* l_ptr, std::vector<OutRange>& out) {
    out.clear();
    if (num_block < 0 || !s_ptr) return false;
    for (int32_t b = 0; b < num_block; ++b) {
        const int64_t s0 = s_ptr[b], s1 = s_ptr[b + 1];
        const int64_t l0 = l_ptr ? l_ptr[b] : 0, l1 = l_ptr ? l_ptr[b + 1] : 0;
        if (s1 < s0 || l1 < l0) return false;
        if (s1 == s0 && l1 == l0) continue;
        out.push_back(OutRange{s0, s1, l0, l1, b});
    }
    return true;
}
