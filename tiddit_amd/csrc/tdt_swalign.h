// The launches of csrc/tdt_swalign.hip, for the entries that hold pair rows on the device (tdt_clip.hip).
#pragma once
#include "tdt_clip_ins.h"
#include "tdt_refseq.h"

// the SN rows, in the order of the file
enum { SW_QUERIES = 0, SW_CLOSED_Q, SW_LEFT_Q, SW_RIGHT_Q, SW_NAMED, SW_UNNAMED, SW_REVERSE, SW_AMBIGUOUS, SW_PAIRS_NAMED, SW_PAIRS_CONFLICT, SW_N };
static_assert(SW_N == TDT_SW_SN_N, "SN rows");
enum { SW_PART_SEQ = 0, SW_PART_LEFT, SW_PART_RIGHT };

// the query table of n queries (device): TDT_SW_SEQ_WORDS words of 56 bits per query (column 28 w + j in bits 2j + 1 : 2j of word w, in
// reference direction), the length, and where the table was built from pair rows the pair row and the part (both NULL otherwise: every
// query is then a pair of its own); a LEFT query is followed by its pair's RIGHT query
struct sw_queries {
    const unsigned long long *seq10;
    const unsigned *qlen, *pair, *part;
};

// the table as the build launch writes it (device), for n queries
struct sw_table {
    unsigned long long *seq10;
    unsigned *qlen, *pair, *part;
    size_t lay(void *base, size_t n) {
        tdt_carver cv(base);
        seq10 = cv.take<unsigned long long>(n * TDT_SW_SEQ_WORDS), qlen = cv.take<unsigned>(n), pair = cv.take<unsigned>(n), part = cv.take<unsigned>(n);
        return cv.size;
    }
};

// the result columns (device, one entry per query)
struct sw_out {
    unsigned *family, *strand, *score, *qstart, *qend, *fstart, *fend, *second, *second_family;
    size_t lay(void *base, size_t n) {
        tdt_carver cv(base);
        family = cv.take<unsigned>(n), strand = cv.take<unsigned>(n), score = cv.take<unsigned>(n), qstart = cv.take<unsigned>(n), qend = cv.take<unsigned>(n);
        fstart = cv.take<unsigned>(n), fend = cv.take<unsigned>(n), second = cv.take<unsigned>(n), second_family = cv.take<unsigned>(n);
        return cv.size;
    }
};

// the workspace of one run (device): every problem's best key and end cell, problem (q * 2 + strand) * families + family
struct sw_work {
    unsigned long long *pkey;
    unsigned *pend;
    size_t lay(void *base, size_t problems) {
        tdt_carver cv(base);
        pkey = cv.take<unsigned long long>(problems), pend = cv.take<unsigned>(problems);
        return cv.size;
    }
};

// A in TDT_SW_MIN_SCORE_LO ... TDT_SW_QMAX, the library inside its limits and loaded, queries x 2 x families below 2^31 (TDT_E_RANGE /
// TDT_E_ARG with the error text set)
int sw_check(const char *fn, tdt_ctx *ctx, const tdt_refseq *lib, size_t n, int A);
// the queries of the pair rows: off[n_pairs + 1] (device, ints) gets every pair's first query and the count; two launches, nothing is waited for
int sw_offsets_launch(tdt_ctx *ctx, size_t n_pairs, const unsigned *status, int *off);
// ... and the table behind them, from the rows' extended consensus and the pairs' closed sequences; one launch, nothing is waited for
int sw_build_launch(tdt_ctx *ctx, ins_sites S, size_t n_pairs, ins_out P, const int *off, sw_table T);
// sw_align_wave over queries x 2 strands x families; one launch, nothing is waited for
int sw_align_launch(tdt_ctx *ctx, const tdt_refseq *lib, size_t n, sw_queries Q, sw_work W);
// sw_reduce: the result columns (Out.family NULL: none are written) and sn[TDT_SW_SN_N] (device, zeroed by the caller); one launch
int sw_reduce_launch(tdt_ctx *ctx, const tdt_refseq *lib, size_t n, sw_queries Q, sw_work W, int A, sw_out Out, unsigned long long *sn);
