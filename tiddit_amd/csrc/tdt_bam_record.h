// Device side of a consumer of the --sv scan that reads raw BAM record bytes (tdt_alleles / tdt_qc / tdt_dup / tdt_indel / tdt_snv /
// tdt_clip): the record bound, the unaligned load, the CIGAR op classes and span, the 4-bit base read, the wave reduction and the
// in-workgroup compaction, each written once.  Host side: tdt_batch.h.
#pragma once
#include "tdt_common.h"

__device__ __forceinline__ unsigned tdt_ld_u32(const uint8_t *p) {      // (records are not aligned)
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// One record of raw[0, raw_len) at offset ro (its block_size field), opened in two steps:
//     if (TDT_REC_HEADER_INSIDE(raw_len, ro)) {            1: the 36 header bytes (block_size, the fixed fields) are inside raw
//         tdt_rec R = TDT_REC_READ(raw, ro);                  ... and are read; l_seq is as stored, the caller judges it
//         if (R.l_seq >= 0 && TDT_REC_FITS(R, raw_len)) {  2: the body fits the block and the block fits raw
// This bound is the ONLY thing between adversarial record bytes and a read outside raw: behind step 2 everything of the record lies in
// [ro, ro + 4 + block_size), itself inside raw_len.  What a kernel calls malformed, skipped or counted around the two steps is its own.
// The two tests and the read are MACROS on purpose: as __forceinline__ functions they give the same answers but not the same code (a
// bool function's `&&` reaches the caller as a select, loads that arrive by inlining are scheduled differently: qc_bases took one
// more VGPR).  As macros qc_bases is instruction for instruction what it was with the bound typed in place (profiles/batch_view_240mb.md).
struct tdt_rec {
    unsigned long long ro;
    unsigned block_size, l_name, n_cig;
    int l_seq;
    // (offsets into raw, behind step 2) the CIGAR: 4 * n_cig bytes; the sequence: (l_seq + 1) / 2; the qualities: l_seq; the aux fields: the rest
    __device__ __forceinline__ unsigned long long body() const { return 32ull + l_name + 4ull * n_cig + ((unsigned long long)l_seq + 1) / 2 + (unsigned long long)l_seq; }
    __device__ __forceinline__ unsigned long long cig() const { return ro + 36 + l_name; }
    __device__ __forceinline__ unsigned long long seq() const { return cig() + 4ull * n_cig; }
    __device__ __forceinline__ unsigned long long qual() const { return seq() + ((unsigned long long)l_seq + 1) / 2; }
    __device__ __forceinline__ unsigned long long aux() const { return ro + 4 + body(); }
    __device__ __forceinline__ unsigned long long end() const { return ro + 4 + block_size; }
};
#define TDT_REC_HEADER_INSIDE(raw_len, ro) ((raw_len) >= 36 && (ro) <= (raw_len) - 36)
#define TDT_REC_FITS(R, raw_len) ((R).body() <= (unsigned long long)(R).block_size && (unsigned long long)(R).block_size <= (raw_len) - 4 - (R).ro)
#define TDT_REC_READ(raw, ro)                                                                                                             \
    tdt_rec{(ro), tdt_ld_u32((raw) + (ro)), ((raw) + (ro) + 4)[8], (unsigned)((raw) + (ro) + 4)[12] | ((unsigned)((raw) + (ro) + 4)[13] << 8), \
            (int)tdt_ld_u32((raw) + (ro) + 4 + 16)}

// ---- the CIGAR and the sequence of an opened record
// the ops whose length lies on the reference (M D N = X) / on the query (M I S = X)
__device__ __forceinline__ bool tdt_cig_on_ref(unsigned op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
__device__ __forceinline__ bool tdt_cig_on_query(unsigned op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }

// the 4-bit code of query base `at` of the sequence at raw[seq ...] (the even base in the high nibble)
__device__ __forceinline__ unsigned tdt_rec_base(const uint8_t *__restrict__ raw, unsigned long long seq, unsigned long long at) {
    return (raw[seq + (at >> 1)] >> ((at & 1ull) ? 0 : 4)) & 0xfu;
}

// ONE pass over the n_cig words at cig: the CIGAR's reference and query lengths and whether an op code above 8 was seen; with EDGES
// also the first two words and the last two (w0 w1 ... wy wz; zero where there is none, one word twice for n_cig == 1: w0 == wz).
// EDGES is a template argument because the tests on j peel the loop even where the words are never used: snv_keys, which does not
// want them, was slower with them (profiles/keyed_emit_240mb.md).  malformed(): the verdicts every consumer of the span shares — an
// op code above 8, pos + the reference length beyond 2^31 - 1, a query length that differs from l_seq (where both a sequence and a
// CIGAR are there).
struct tdt_cig_span {
    unsigned long long ref_len, query_len;
    unsigned w0, w1, wy, wz;
    bool bad_op;
    __device__ __forceinline__ bool malformed(int pos, int l_seq, unsigned n_cig) const {
        bool worse = bad_op;
        worse |= (unsigned long long)pos + ref_len > 0x7fffffffull;
        worse |= l_seq >= 1 && n_cig >= 1 && query_len != (unsigned long long)l_seq;
        return worse;
    }
};
template <bool EDGES = false> __device__ __forceinline__ tdt_cig_span tdt_cig_span_of(const uint8_t *cig, unsigned n_cig) {
    tdt_cig_span s{0, 0, 0, 0, 0, 0, false};
    for (unsigned j = 0; j < n_cig; j++) {
        const unsigned w = tdt_ld_u32(cig + 4ull * j), op = w & 0xfu, len = w >> 4;
        s.bad_op |= op > 8;
        s.ref_len += tdt_cig_on_ref(op) ? (unsigned long long)len : 0ull;
        s.query_len += tdt_cig_on_query(op) ? (unsigned long long)len : 0ull;
        if constexpr (EDGES) {
            if (j == 0) s.w0 = w;
            if (j == 1) s.w1 = w;
            s.wy = s.wz;
            s.wz = w;
        }
    }
    return s;
}

// ---- a value of every lane reduced over the wave by a butterfly: all 64 lanes call it and all receive the result
struct tdt_sum { template <class T> __device__ static T of(T a, T b) { return a + b; } };
struct tdt_or { template <class T> __device__ static T of(T a, T b) { return a | b; } };
struct tdt_max { template <class T> __device__ static T of(T a, T b) { return b > a ? b : a; } };
template <class Op, class T> __device__ __forceinline__ T tdt_wave_reduce(T v) {
    for (int d = 32; d > 0; d >>= 1) v = Op::of(v, __shfl_xor(v, d));
    return v;
}

// ---- compaction inside a workgroup of NW waves, in thread order.  m = the wave's ballot of the lanes that take a slot.  Called by every
// thread of the workgroup: ONE __syncthreads() inside, between the waves' counts going to s_wsum[NW] and being read.  A lane whose bit
// of m is set owns slot base + tdt_lane_rank(m, lane); the caller writes its slots and synchronises before it reads them.
struct tdt_slots {
    int base, total;                             // the wave's first slot; the slots taken in the workgroup
};
template <int NW> __device__ __forceinline__ tdt_slots tdt_block_slots(unsigned long long m, int (&s_wsum)[NW], int lane, int wave) {
    if (lane == 0) s_wsum[wave] = __popcll(m);
    __syncthreads();
    tdt_slots s{0, 0};
    for (int w = 0; w < NW; w++) {
        s.base += w < wave ? s_wsum[w] : 0;
        s.total += s_wsum[w];
    }
    return s;
}
__device__ __forceinline__ int tdt_lane_rank(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }
