// The wave-cooperative search of the query-per-wave kernels (tdt_region.hip, tdt_links.hip).
#pragma once
#include "tdt_common.h"

// Wave-cooperative 64-ary lower bounds (first i with a[i] >= v) for TWO keys in lock step: every round the 64 lanes probe 64
// evenly spaced elements of each key's bracket, a ballot counts the probes below the key and the bracket shrinks 64x —
// 5 dependent loads for 25 M reads instead of the 25 of a scalar binary search, with both chains in flight together.
// S: stride in int32 words between consecutive keys (1: a plain array; 2: posA of the 8-byte link records; 4: the start field of
// 16-byte evidence records).
template <int S>
__device__ __forceinline__ void rg_lower_bound2(const int32_t *__restrict__ a, int n, long long v0, long long v1, int lane, int &r0,
                                                int &r1) {
    int lo0 = 0, hi0 = n, lo1 = 0, hi1 = n;
    while (hi0 - lo0 > 64 || hi1 - lo1 > 64) {
        const int c0 = (hi0 - lo0) >> 6, c1 = (hi1 - lo1) >> 6;               // chunk; 0 = this bracket is already narrow
        const int x0 = c0 ? a[(size_t)(lo0 + (lane + 1) * c0 - 1) * S] : 0, x1 = c1 ? a[(size_t)(lo1 + (lane + 1) * c1 - 1) * S] : 0;
        if (c0) {
            const int k = __popcll(__ballot((long long)x0 < v0));
            hi0 = k < 64 ? lo0 + (k + 1) * c0 - 1 : hi0;
            lo0 += k * c0;
        }
        if (c1) {
            const int k = __popcll(__ballot((long long)x1 < v1));
            hi1 = k < 64 ? lo1 + (k + 1) * c1 - 1 : hi1;
            lo1 += k * c1;
        }
    }
    const bool b0 = lo0 + lane < hi0 && (long long)a[(size_t)(lo0 + lane) * S] < v0;
    const bool b1 = lo1 + lane < hi1 && (long long)a[(size_t)(lo1 + lane) * S] < v1;
    r0 = lo0 + __popcll(__ballot(b0));
    r1 = lo1 + __popcll(__ballot(b1));
}
