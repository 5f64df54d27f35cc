// Reference support at clip-site junctions from the evidence store (TIDDIT_CLIPS_VCF, tiddit_clip_vcf.py rule 4), gfx950: for every
// boundary b of a contig of LN bases (0-based: b bases lie left of the cut) and the flank F, over the contig's records with
// e = min(end, LN) and end > start,
//   left      = the kept records with start <= b - F < e          (0 when b - F < 0)
//   right     = the kept records with start <= b + F - 1 < e      (0 when b + F > LN)
//   span      = the kept records with both: the reads that cross the cut with F aligned bases on either side
//   span_lowq = the records with both whose only excluding bit is TDT_EV_LOW_Q
// kept: none of TDT_EV_UNMAPPED | TDT_EV_DUPLICATE | TDT_EV_LOW_Q, the read filter of tdt_depth_dist.hip.  All positions are 64-bit:
// b + F passes 2^31 on a contig of 2^31 - 1 bases.
//
// ONE launch covers all boundaries, ONE WAVEFRONT answers one boundary (the shape of region_counts_packed, tdt_region.hip):
//   1. a record that can hold b - F or b + F - 1 has start in (b - F - max span, b + F - 1]: both ends of that bracket come from ONE
//      call of the 64-ary search (tdt_search.h) on the start field of the 16-byte records;
//   2. the lanes stride over the bracket, one 16-byte load per record, four counters per lane in registers;
//   3. a shuffle reduction over the wavefront, lane 0 writes the row of four.
// No atomics (the device entry's kernel marks the first boundary that names no contig row with one atomicMin, on that error path
// only), no LDS, no workgroup waits for another, no scratch.
#include "tdt_common.h"
#include "tdt_search.h"

#define JS_THREADS 256
#define JS_WAVES (JS_THREADS / 64)           // boundaries per workgroup
#define JS_MAX_FLANK 1000

// CHECK (the device entry, whose boundaries the host never sees): a boundary naming no row of the table writes zeros and leaves the
// lowest such index in *bad; the branch is uniform (one boundary per wavefront).
template <bool CHECK>
__global__ __launch_bounds__(JS_THREADS) void junction_support(const int4 *__restrict__ rec, const long long *__restrict__ ctab, int n_contigs,
                                                               const int2 *__restrict__ bnd, int nb, int F, long long *__restrict__ out,
                                                               int *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * JS_WAVES + (threadIdx.x >> 6);
    if (q >= nb) return;
    const int2 B = bnd[q];                                                        // (contig row, b)
    if (CHECK && (B.x < 0 || B.x >= n_contigs)) {
        if (lane < 4) out[(size_t)q * 4 + lane] = 0;
        if (lane == 0) atomicMin(bad, q);
        return;
    }
    const long long *C = ctab + 5 * (size_t)B.x;                                  // (offset, n, max span, tid, length)
    const int4 *__restrict__ R = rec + C[0];
    const int n = (int)C[1];
    const long long LN = C[4];
    const long long pl = (long long)B.y - F, pr = (long long)B.y + F - 1;         // the base F left of the cut, the base F - 1 right of it
    const bool have_l = pl >= 0, have_r = pr < LN;                                // (pr < LN  <=>  b + F <= LN)
    int i0, i1;   // start > pl - max span  <=>  i >= i0;   start <= pr  <=>  i < i1
    rg_lower_bound2<4>(reinterpret_cast<const int32_t *>(R), n, pl - C[2] + 1, pr + 1, lane, i0, i1);
    unsigned left = 0, right = 0, span = 0, lowq = 0;
    for (int i = i0 + lane; i < i1; i += 64) {
        const int4 r = R[i];
        const long long rs = r.x, e = (long long)r.y < LN ? (long long)r.y : LN;
        const unsigned x = (unsigned)r.w & (TDT_EV_UNMAPPED | TDT_EV_DUPLICATE | TDT_EV_LOW_Q);
        const bool real = r.y > r.x;                                              // end <= start counts nowhere
        const bool l = real && have_l && rs <= pl && pl < e, rr = real && have_r && rs <= pr && pr < e;
        left += (x == 0 && l) ? 1u : 0u;
        right += (x == 0 && rr) ? 1u : 0u;
        span += (x == 0 && l && rr) ? 1u : 0u;
        lowq += (x == TDT_EV_LOW_Q && l && rr) ? 1u : 0u;
    }
    for (int d = 32; d > 0; d >>= 1) {
        left += __shfl_xor(left, d);
        right += __shfl_xor(right, d);
        span += __shfl_xor(span, d);
        lowq += __shfl_xor(lowq, d);
    }
    if (lane == 0) {
        long long *o = out + (size_t)q * 4;
        o[0] = left; o[1] = right; o[2] = span; o[3] = lowq;
    }
}

// the checks both entries make before anything is launched
static int junction_check(const char *fn, tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, const void *boundaries, size_t nb,
                          int F, const void *out) {
    if (!ctx || !s || n_contigs < 0 || nb >= 0x7fffffffull || (n_contigs && !contigs) || (nb && (!boundaries || !out)) ||
        ((uintptr_t)contigs & 7) || ((uintptr_t)boundaries & 7) || ((uintptr_t)out & 7)) {
        tdt_set_error("%s: bad argument (a null or misaligned pointer)", fn);
        return TDT_E_ARG;
    }
    if (F < 1 || F > JS_MAX_FLANK) {
        tdt_set_error("%s: flank %d, 1 ... %d", fn, F, JS_MAX_FLANK);
        return TDT_E_ARG;
    }
    return tdt_evstore_check_rows(fn, s, contigs, n_contigs);
}

// the launch between two timed events; the caller's stream is synchronised before the events are read
template <bool CHECK>
static int junction_launch(tdt_ctx *ctx, tdt_evstore *s, const long long *dct, int n_contigs, const int2 *dq, size_t nb, int F, long long *dout,
                           int *dbad, hipEvent_t e0, hipEvent_t e1) {
    hipStream_t st = ctx->stream;
    TDT_HIP(hipEventRecord(e0, st));
    hipLaunchKernelGGL(junction_support<CHECK>, dim3((unsigned)((nb + JS_WAVES - 1) / JS_WAVES)), dim3(JS_THREADS), 0, st, s->rec, dct, n_contigs, dq,
                       (int)nb, F, dout, dbad);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipEventRecord(e1, st));
    return TDT_OK;
}

struct js_events {                             // two timing events for the length of one call
    hipEvent_t e[2] = {nullptr, nullptr};
    int make() {
        TDT_HIP(hipEventCreate(&e[0]));
        TDT_HIP(hipEventCreate(&e[1]));
        return TDT_OK;
    }
    int read(tdt_evstore *s) {
        float ms = 0;
        TDT_HIP(hipEventElapsedTime(&ms, e[0], e[1]));
        s->junction_ms = ms;
        return TDT_OK;
    }
    ~js_events() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

extern "C" int tdt_junction_support(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, const int32_t *boundaries, size_t nb,
                                    int F, int64_t *out) {
    int rc = junction_check("tdt_junction_support", ctx, s, contigs, n_contigs, boundaries, nb, F, out);
    if (rc) return rc;
    for (size_t q = 0; q < nb; q++) {
        if (boundaries[2 * q] < 0 || boundaries[2 * q] >= n_contigs) {
            tdt_set_error("tdt_junction_support: boundary %zu names contig %d of %d", q, boundaries[2 * q], n_contigs);
            return TDT_E_RANGE;
        }
    }
    if (nb == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(ctx->device));
    if (ctx != s->ctx) TDT_HIP(hipStreamSynchronize(s->ctx->stream));       // (the packs of another context's stream are complete)
    const size_t ct = ((size_t)n_contigs * 40 + 255) & ~(size_t)255, qb = (nb * 8 + 255) & ~(size_t)255;
    void *d = nullptr;
    rc = tdt_scratch(ctx, 28, ct + qb + nb * 32, &d);         // (the slot of tdt_depth_dist: both calls end with the stream idle)
    if (rc) return rc;
    long long *dct = (long long *)d;
    int2 *dq = (int2 *)((char *)d + ct);
    long long *dout = (long long *)((char *)d + ct + qb);
    js_events ev;
    rc = ev.make();
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    TDT_HIP(hipMemcpyAsync(dct, contigs, (size_t)n_contigs * 40, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dq, boundaries, nb * 8, hipMemcpyHostToDevice, st));
    rc = junction_launch<false>(ctx, s, dct, n_contigs, dq, nb, F, dout, nullptr, ev.e[0], ev.e[1]);
    if (rc) return rc;
    TDT_HIP(hipMemcpyAsync(out, dout, nb * 32, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    return ev.read(s);
}

// The same counts with the boundaries and the output in HBM.  The contig table is the host's; the kernel checks the boundaries' rows.
// The stream is synchronised before the return.
extern "C" int tdt_junction_support_device(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, const int32_t *d_boundaries,
                                           size_t nb, int F, int64_t *d_out) {
    int rc = junction_check("tdt_junction_support_device", ctx, s, contigs, n_contigs, d_boundaries, nb, F, d_out);
    if (rc) return rc;
    if (nb == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(ctx->device));
    if (ctx != s->ctx) TDT_HIP(hipStreamSynchronize(s->ctx->stream));
    const size_t ct = ((size_t)n_contigs * 40 + 255) & ~(size_t)255;
    void *d = nullptr;
    rc = tdt_scratch(ctx, 28, ct + 256, &d);
    if (rc) return rc;
    long long *dct = (long long *)d;
    int *dbad = (int *)((char *)d + ct);
    js_events ev;
    rc = ev.make();
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    int bad = 0x7fffffff;                          // (host words: the stream is synchronised before they go out of scope)
    if (n_contigs) TDT_HIP(hipMemcpyAsync(dct, contigs, (size_t)n_contigs * 40, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dbad, &bad, sizeof(int), hipMemcpyHostToDevice, st));
    rc = junction_launch<true>(ctx, s, dct, n_contigs, (const int2 *)d_boundaries, nb, F, (long long *)d_out, dbad, ev.e[0], ev.e[1]);
    if (rc) return rc;
    TDT_HIP(hipMemcpyAsync(&bad, dbad, sizeof(int), hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    rc = ev.read(s);
    if (rc) return rc;
    if (bad != 0x7fffffff) {
        int row = 0;
        TDT_HIP(hipMemcpy(&row, d_boundaries + 2 * (size_t)bad, sizeof(int), hipMemcpyDeviceToHost));
        tdt_set_error("tdt_junction_support_device: boundary %d names contig %d of %d", bad, row, n_contigs);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

extern "C" int tdt_junction_timing(tdt_evstore *s, double *ms) {
    if (!s || !ms) {
        tdt_set_error("tdt_junction_timing: bad argument");
        return TDT_E_ARG;
    }
    *ms = s->junction_ms;
    return TDT_OK;
}
