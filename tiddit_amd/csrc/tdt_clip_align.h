// The launch of csrc/tdt_clip_align.hip, for the entries that hold site rows on the device (tdt_clip.hip).
#pragma once
#include "tdt_refseq.h"

// the site columns of n rows (device): K1 = tid << 32 | P, side, CLEN, the packed consensus
struct ca_sites {
    const unsigned long long *k1;
    const unsigned *side, *clen;
    const unsigned long long *cons;
};

// what the kernel writes (device, n entries each); sn: TDT_CLIP_ALIGN_SN_N counters the kernel adds to, or NULL
struct ca_out {
    unsigned *status, *partner, *strand, *mm, *hits;
    unsigned long long *sn;
};

// the range checks of W, K, M (TDT_E_RANGE with the error text set) and the launch on the context's stream; nothing is waited for
int ca_check_range(const char *fn, int W, int K, int M);
int ca_launch(tdt_ctx *ctx, const tdt_refseq *ref, size_t n, ca_sites S, int W, int K, int M, ca_out O);
