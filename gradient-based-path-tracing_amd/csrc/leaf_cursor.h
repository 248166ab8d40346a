// leaf_cursor.h — the leaf reference of the traversal state read as a cursor (no HIP dependency: the kernels include it through
// render_device.h, tests/leaf_cursor_check.cpp includes it on the host).
//
// A leaf is cur < 0 with ~cur = first << 2 | (count - 1), count = 1..4 records starting at `first`. Testing the first K records of a
// leaf with count > K leaves the records first + K .. first + count - 1, which is again a leaf, (first + K) << 2 | (count - K - 1):
// the traversal state (cur, sp, best) holds a partly consumed leaf without a field of its own.
#pragma once

#if defined(__HIPCC__)
#define GDPT_LEAF_HD __host__ __device__ inline
#else
#define GDPT_LEAF_HD inline
#endif

namespace gd {

// Records a step of K tests on leaf `cur`: min(count, K).
GDPT_LEAF_HD unsigned leaf_step_records(int cur, int K) {
    const unsigned count = (~(unsigned)cur & 3u) + 1u;
    return count < (unsigned)K ? count : (unsigned)K;
}

// After the first K records of leaf `cur` have been tested: true and `cur` = the leaf of the records that remain (count > K), or
// false ("pop": the leaf is used up, `cur` is left as it was). count - 1 >= K, so subtracting K from the low two bits borrows nothing
// from `first`: the packed word grows by 4K - K and ~packed, a negative number, falls by 3K — the count falls by K with every step, a
// leaf is used up after ceil(count / K) of them whatever K in 1..3 is.
GDPT_LEAF_HD bool leaf_advance(int &cur, int K) {
    const unsigned packed = ~(unsigned)cur;
    if ((packed & 3u) < (unsigned)K) return false;
    cur = (int)~(packed + 3u * (unsigned)K);
    return true;
}

} // namespace gd
