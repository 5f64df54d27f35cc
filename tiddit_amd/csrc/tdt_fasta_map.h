// Where base b of a contig sits in the contig's FASTA bytes (line ends still in place): byte (b / linebases) * linewidth + b % linebases,
// `linebases` bases and `linewidth` bytes per full line (the .fai columns).  floor(b / linebases) = mulhi(b, magic) >> shift for
// 0 <= b < 2^31 (round-up method, as for the coverage bins).  Shared by gc_fasta_bins (tdt_gc.hip) and ref_pack (tdt_refseq.hip).
#pragma once
#include "tdt_common.h"

struct tdt_fasta_map {
    unsigned linebases, linewidth, magic;
    int shift;                                    // < 0: one base per line, the line IS the base
#ifdef __HIPCC__
    __device__ __forceinline__ unsigned line_of(unsigned b) const { return shift < 0 ? b : (unsigned)(__umulhi(b, magic) >> shift); }
    __device__ __forceinline__ long long byte_of(unsigned b) const {          // byte offset of base b (b < 2^31)
        const unsigned line = line_of(b);
        return (long long)line * linewidth + (b - line * linebases);
    }
#endif
};

// the layouts both kernels take: whole lines of linebases bases closed by at most two bytes, fewer than 2^31 bases
static inline bool tdt_fasta_layout_ok(int64_t len, int linebases, int linewidth) {
    return linebases > 0 && linewidth >= linebases && linewidth <= linebases + 2 && len < (1ll << 31);
}

// the bytes `len` bases occupy (no line end behind the last base)
static inline long long tdt_fasta_bytes(int64_t len, int linebases, int linewidth) {
    const long long nfull = len / linebases, tail = len - nfull * linebases;
    return nfull * linewidth + tail - (tail == 0 ? (linewidth - linebases) : 0);
}

// the reciprocal of a layout tdt_fasta_layout_ok accepts; false: the line length has no 32-bit one
static inline bool tdt_fasta_map_make(int linebases, int linewidth, tdt_fasta_map *m) {
    m->linebases = (unsigned)linebases, m->linewidth = (unsigned)linewidth, m->magic = 0, m->shift = -1;
    if (linebases > 1) {
        int l = 0;
        while ((1ll << l) < linebases) l++;
        const unsigned long long v = ((1ull << (31 + l)) + (unsigned long long)linebases - 1) / (unsigned long long)linebases;
        if (v > 0xffffffffull) return false;
        m->magic = (unsigned)v;
        m->shift = l - 1;   // mulhi already drops 32 bits: (b * m) >> (31 + l) == mulhi(b, m) >> (l - 1)
    }
    return true;
}
