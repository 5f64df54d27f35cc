// The scan over a workgroup and the carry of per-tile counts into offsets of the key store's run-length launches (tdt_keystore.h), in a
// header of their own for the launches that walk rows in tiles of KS_TILE without a store (tdt_clip_ins.hip).
// Everything here has internal linkage: each translation unit instantiates its own copy.
#pragma once
#include "tdt_bam_record.h"

namespace {

typedef unsigned long long ks_ull;

#ifndef KS_BLOCK                              // (tdt_keystore.h defines its geometry in front of this header; a user without a store takes this one)
#define KS_BLOCK 256
#define KS_TILE 4096
#endif
static_assert(KS_BLOCK % 64 == 0 && KS_TILE % KS_BLOCK == 0, "whole waves, whole rounds");

// inclusive scan over the workgroup's 256 threads, in thread order (Op: tdt_max or tdt_sum; `none` its neutral element);
// *total = the reduction of all (s: KS_BLOCK / 64 words)
template <class Op> __device__ __forceinline__ int ks_block_scan(int v, int none, int *s, int t, int *total) {
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v = Op::of(v, u);
    }
    if (lane == 63) s[wave] = v;
    __syncthreads();
    int all = none;
#pragma unroll
    for (int w = 0; w < KS_BLOCK / 64; w++) {
        const int c = s[w];
        if (w < wave) v = Op::of(v, c);
        all = Op::of(all, c);
    }
    __syncthreads();
    *total = all;
    return v;
}

// ONE workgroup: tile_kept[k] = the kept runs of the tiles in front of tile k (an exclusive sum; the total is below 2^30)
__global__ __launch_bounds__(KS_BLOCK) void ks_carry_sum(int *__restrict__ tile_kept, int ntiles) {
    __shared__ int s[KS_BLOCK / 64];
    const int t = threadIdx.x;
    int running = 0;
    for (int c = 0; c < ntiles; c += KS_BLOCK) {                   // (uniform)
        const int k = c + t;
        const int mine = k < ntiles ? tile_kept[k] : 0;
        int all;
        const int v = ks_block_scan<tdt_sum>(mine, 0, s, t, &all);
        if (k < ntiles) tile_kept[k] = running + v - mine;
        running += all;
    }
}

}  // namespace
