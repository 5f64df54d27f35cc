// The launches of csrc/tdt_clip_ins.hip, for the entries that hold site rows on the device (tdt_clip.hip).
#pragma once
#include "tdt_common.h"

#define INS_SEQ_WORDS TDT_CLIP_INS_SEQ_WORDS
#define INS_MAX_SITES (1 << 30)               // rows of one call (the tile offsets are ints)

// the SN rows, in the order of the file; the first four are the push's (tdt_clip.hip fills them from the extension store's state line)
enum { IN_EXT_LEFT = 0, IN_EXT_RIGHT, IN_EXT_KEYS, IN_CUT, IN_EXTENDED, IN_LEFT, IN_RIGHT, IN_PAIRS, IN_CLOSED, IN_OPEN, IN_MULTI, IN_N };
static_assert(IN_N == TDT_CLIP_INS_SN_N, "SN rows");

// the site columns of n rows (device), ascending by (K1, side): K1 = tid << 32 | P, side, ECLEN, five words of 56 bits per row
struct ins_sites {
    const unsigned long long *k1;
    const unsigned *side, *eclen;
    const unsigned long long *cons5;
};

// the (chunk, site) rows of the extension store's finish (device), ascending by (K1, side) with the chunk in K1's top byte
struct ins_chunks {
    const unsigned long long *k1;
    const unsigned *side, *clen;
    const unsigned long long *cons;
};

// what the pair launches write (device, one entry per pair; seq10: INS_SEQ_WORDS words per pair)
struct ins_out {
    unsigned *r_row, *l_row, *tsd, *status, *len, *mm, *closures;
    unsigned long long *seq10;
    size_t lay(void *base, size_t n) {
        tdt_carver cv(base);
        r_row = cv.take<unsigned>(n), l_row = cv.take<unsigned>(n), tsd = cv.take<unsigned>(n), status = cv.take<unsigned>(n), len = cv.take<unsigned>(n);
        mm = cv.take<unsigned>(n), closures = cv.take<unsigned>(n), seq10 = cv.take<unsigned long long>(n * INS_SEQ_WORDS);
        return cv.size;
    }
};

// the workspace of the pair launches over n rows (device): the tiles' pair counts, then their offsets
struct ins_work {
    int *tile_pairs;
    size_t lay(void *base, size_t n) {
        tdt_carver cv(base);
        tile_pairs = cv.take<int>((n + 4095) / 4096);
        return cv.size;
    }
};

// the range checks of K, O, M (TDT_E_RANGE with the error text set)
int ins_check_range(const char *fn, int K, int O, int M);
// base rows (K1, side, CLEN, consensus) + the chunk rows -> ECLEN and the five words per base row; one launch, nothing is waited for
int ins_gather_launch(tdt_ctx *ctx, size_t n, const unsigned long long *k1, const unsigned *side, const unsigned *clen, const unsigned long long *cons, size_t nx,
                      ins_chunks X, unsigned *eclen, unsigned long long *cons5);
// clip_ins_count<false> and ks_carry_sum over the n rows: sn[TDT_CLIP_INS_SN_N] (device, zeroed by the caller) gets the site counters
// and the pairs; nothing is waited for
int ins_count_launch(tdt_ctx *ctx, size_t n, ins_sites S, int K, ins_work W, unsigned long long *sn);
// clip_ins_count<true> (the pairs' rows and TSD) and clip_ins_pairs (the closure) over the offsets ins_count_launch left; O has room for
// the pairs it counted; nothing is waited for
int ins_pairs_launch(tdt_ctx *ctx, size_t n, ins_sites S, int K, int O, int M, ins_work W, size_t n_pairs, ins_out Out, unsigned long long *sn);
