// Host side of a consumer of the --sv scan (tdt_alleles / tdt_qc / tdt_dup; tdt_signal_scan for the view alone): one batch of reads as
// typed, named columns — from the ingest's pointer table (TDT_COL_* of include/tiddit_hip.h), or uploaded from host columns into the
// handle's own block.  A consumer says which columns it reads (a mask of TDT_NEED) and fills its kernel arguments from the view by
// name; no entry point holds a column index or a carve of its own.  Device side: tdt_bam_record.h.
#pragma once
#include "tdt_common.h"

// X(TDT_COL_ suffix, member, element type): the thirteen field columns; the raw record bytes come behind them, raw_len bytes not n elements
#define TDT_BATCH_COLUMNS(X)                                                                                                              \
    X(TID, tid, int32_t) X(POS, pos, int32_t) X(END, end, int32_t) X(MAPQ, mapq, uint8_t) X(FLAG, flag, uint16_t) X(MATE_TID, mate_tid, int32_t) \
    X(MATE_POS, mate_pos, int32_t) X(TLEN, tlen, int32_t) X(L_SEQ, l_seq, int32_t) X(CIGAR_FIRST, cigar_first, uint32_t)                  \
    X(CIGAR_LAST, cigar_last, uint32_t) X(REC_OFF, rec_off, uint64_t) X(SA_OFF, sa_off, int64_t)
#define TDT_NEED(c) (1u << TDT_COL_##c)
static_assert(TDT_COL_RAW == TDT_NCOL - 1 && TDT_NCOL <= 32, "the raw bytes close the table; a mask is an unsigned");

struct tdt_batch {                               // device pointers, or the caller's host pointers on their way into tdt_batch_upload
#define X(C, m, T) const T *m;
    TDT_BATCH_COLUMNS(X)
#undef X
    const uint8_t *raw;
};

struct tdt_batch_io { void *d; size_t cap; };    // a handle's own block for the columns + raw bytes of its host entry (grows)

static inline tdt_batch tdt_batch_of(const void *const *table) {
    tdt_batch B;
#define X(C, m, T) B.m = (const T *)table[TDT_COL_##C];
    TDT_BATCH_COLUMNS(X)
#undef X
    B.raw = (const uint8_t *)table[TDT_COL_RAW];
    return B;
}

static inline bool tdt_batch_lacks(const tdt_batch &B, unsigned need, size_t raw_len) {
#define X(C, m, T) if ((need & TDT_NEED(C)) && !B.m) return true;
    TDT_BATCH_COLUMNS(X)
#undef X
    return (need & TDT_NEED(RAW)) && raw_len && !B.raw;
}

// The pointer table of a *_push_device entry `fn` as a view, behind the checks of every such entry: no handle, n >= 2^31 or no table
// -> "bad argument"; then (n > 0) a needed column that is NULL, or raw_len with NULL raw -> "a column of the batch is NULL".  Both
// TDT_E_ARG.  n == 0: TDT_OK and nothing is looked at.
static inline int tdt_batch_refuse(const char *fn, const char *why) {
    tdt_set_error("%s: %s", fn, why);
    return TDT_E_ARG;
}
static inline int tdt_batch_view(const char *fn, const void *h, const void *const *table, size_t n, size_t raw_len, unsigned need, tdt_batch *B) {
    if (!h || n >= 0x7fffffffull || (n && !table)) return tdt_batch_refuse(fn, "bad argument");
    *B = n ? tdt_batch_of(table) : tdt_batch{};
    return n && tdt_batch_lacks(*B, need, raw_len) ? tdt_batch_refuse(fn, "a column of the batch is NULL") : TDT_OK;
}

// ... and the host columns H of a *_push entry: all of it is one "bad argument"
static inline int tdt_batch_host(const char *fn, const void *h, const tdt_batch &H, size_t n, size_t raw_len, unsigned need) {
    const bool bad = !h || n >= 0x7fffffffull || (n && tdt_batch_lacks(H, need & ~TDT_NEED(RAW), 0)) || (raw_len && !H.raw);
    return bad ? tdt_batch_refuse(fn, "bad argument") : TDT_OK;
}

static inline int tdt_batch_offsets_ascend(const char *fn, const uint64_t *rec_off, size_t n) {
    size_t i = 1;
    while (i < n && rec_off[i] >= rec_off[i - 1]) i++;
    if (i >= n) return TDT_OK;
    tdt_set_error("%s: record offsets must not decrease (record %zu)", fn, i);
    return TDT_E_ARG;
}

// The needed host columns of H (n elements each) and raw_len record bytes go to the handle's block, which grows when it is too small
// (the stream is drained first: a kernel of the push before may still read the old one), and *D is their device view.  One lay()
// measures the block and hands its pieces out; raw has one byte of slack, so it is a pointer of its own for raw_len == 0 too.  The
// copies are enqueued on the context's stream; the caller synchronises before its host arrays are free again.
static inline int tdt_batch_upload(const char *fn, tdt_ctx *ctx, tdt_batch_io *io, const tdt_batch &H, unsigned need, size_t n, size_t raw_len,
                                   tdt_batch *D) {
    hipStream_t st = ctx->stream;
    auto lay = [&](void *base) {
        tdt_carver cv(base);
        *D = tdt_batch{};
#define X(C, m, T) if (need & TDT_NEED(C)) D->m = cv.take<T>(n);
        TDT_BATCH_COLUMNS(X)
#undef X
        D->raw = cv.take<uint8_t>(raw_len + 1);
        return cv.size;
    };
    const size_t bytes = lay(nullptr);
    if (bytes > io->cap) {
        TDT_HIP(hipStreamSynchronize(st));
        if (io->d) TDT_HIP(hipFree(io->d));
        io->d = nullptr;
        io->cap = 0;
        if (tdt_dev_malloc(&io->d, bytes) != hipSuccess) {
            tdt_set_error("%s: out of device memory (%zu reads, %zu bytes)", fn, n, raw_len);
            return TDT_E_NOMEM;
        }
        io->cap = bytes;
    }
    lay(io->d);
#define X(C, m, T) if (need & TDT_NEED(C)) TDT_HIP(hipMemcpyAsync((void *)D->m, H.m, n * sizeof(T), hipMemcpyHostToDevice, st));
    TDT_BATCH_COLUMNS(X)
#undef X
    if (raw_len) TDT_HIP(hipMemcpyAsync((void *)D->raw, H.raw, raw_len, hipMemcpyHostToDevice, st));
    return TDT_OK;
}
