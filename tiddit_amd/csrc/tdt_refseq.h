// The resident reference (tdt_refseq.hip), as the kernels that read it see it.  ONE HBM buffer of 4-bit base codes (BAM's own,
// "=ACMGRSVTWYHKDBN"), two bases per byte, the even base in the high nibble — the layout of a record's sequence.  Contig c starts at byte
// off[c], a multiple of 8, and has at least TDT_REF_GUARD zero bytes in front of it and behind it: code 0 is no base, so a comparison
// that runs off either end stops there, and whole 64-bit words can be loaded at either end without a bounds branch.  len[c] < 0: the
// contig is not loaded (its bytes are zero).
#pragma once
#include "tdt_common.h"

#define TDT_REF_GUARD 16

struct tdt_refseq {
    tdt_ctx *ctx;
    int n_contigs;
    uint8_t *d_store;                             // `bytes` bytes, zero wherever nothing is loaded
    size_t bytes;
    unsigned long long *d_off;                    // [n_contigs] byte offsets into d_store
    int *d_len;                                   // [n_contigs] bases, -1 until the contig is loaded
    std::vector<unsigned long long> off;          // the host's copy of both
    std::vector<long long> len;
    std::vector<char> loaded;
};

// what a kernel takes (by value); n == 0: no contig is loaded
struct tdt_refview {
    const uint8_t *store;
    const unsigned long long *off;
    const int *len;
    int n;
};

#ifdef __HIPCC__
// the code of base i of the contig at byte offset off
__device__ __forceinline__ unsigned tdt_ref_code(const uint8_t *__restrict__ store, unsigned long long off, long long i) {
    return (store[off + (unsigned long long)(i >> 1)] >> ((i & 1) ? 0 : 4)) & 0xfu;
}

// the 16 bases that END at nibble g of the store (g >= 15): nibble t of the result, counted from the low end, is base g - t.  Two aligned
// 64-bit loads; the byte swap makes the base order monotone over the word.
__device__ __forceinline__ unsigned long long tdt_ref_left16(const uint8_t *__restrict__ store, unsigned long long g) {
    const unsigned long long first = g - 15ull;
    const unsigned long long *w = reinterpret_cast<const unsigned long long *>(store) + (first >> 4);
    const unsigned r = (unsigned)(first & 15ull) * 4u;
    const unsigned long long hi = __builtin_bswap64(w[0]), lo = __builtin_bswap64(w[1]);
    return r ? (hi << r) | (lo >> (64u - r)) : hi;
}

// a word with a non-zero nibble wherever x's nibble is not one of A C G T (1, 2, 4, 8: exactly one bit set)
__device__ __forceinline__ unsigned long long tdt_ref_not_acgt(unsigned long long x) {
    const unsigned long long m = 0x1111111111111111ull;
    return ((x & m) + ((x >> 1) & m) + ((x >> 2) & m) + ((x >> 3) & m)) ^ m;
}
#endif
