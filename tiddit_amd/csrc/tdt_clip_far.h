// The launches of csrc/tdt_clip_far.hip, for the entries that hold site rows on the device (tdt_clip.hip).
#pragma once
#include "tdt_clip_align.h"

// The 64-bit key of a candidate gives t 24 bits: a reference of more contigs is refused with TDT_E_RANGE.  (tdt_refseq_create refuses
// it too.)  A site takes two entries of the sort, which handles fewer than 2^30: 2^29 sites or more are refused the same way.
#define FAR_MAX_CONTIGS (1 << 24)
#define FAR_MAX_SITES (1 << 29)
#define FAR_FILTER_WORDS_MAX (1 << 16)
#define FAR_NO_MM 0xffffffffu

// what the launches write (device, n entries each); sn: TDT_CLIP_FAR_SN_N counters far_rows adds to, or NULL
struct far_out {
    unsigned *status, *ptid, *partner, *strand, *mm, *hits;
    unsigned long long *sn;
};

// the workspace of one search over n sites (device): two table entries per site
struct far_work {
    unsigned long long *keys, *keys_tmp, *tails, *slot_key, *slot_hits, *state;
    unsigned *vals, *vals_tmp, *filter;
    size_t lay(void *base, size_t n) {
        tdt_carver cv(base);
        keys = cv.take<unsigned long long>(2 * n), keys_tmp = cv.take<unsigned long long>(2 * n), tails = cv.take<unsigned long long>(2 * n);
        slot_key = cv.take<unsigned long long>(n), slot_hits = cv.take<unsigned long long>(n), state = cv.take<unsigned long long>(2);
        vals = cv.take<unsigned>(2 * n), vals_tmp = cv.take<unsigned>(2 * n), filter = cv.take<unsigned>(FAR_FILTER_WORDS_MAX);
        return cv.size;
    }
};

// the range checks of the reference, n, K, M (TDT_E_RANGE with the error text set)
int far_check_range(const char *fn, const tdt_refseq *ref, size_t n, int K, int M);
// the four launches (seeds + filter, sort, scan, rows) on the context's stream over a workspace laid for n sites; nothing is waited for.
// ev: NULL, or five events recorded in front of, between and behind them
int far_launch(tdt_ctx *ctx, const tdt_refseq *ref, size_t n, ca_sites S, int K, int M, far_out O, far_work &Wk, hipEvent_t *ev);
