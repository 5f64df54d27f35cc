// Regional evidence counts per SV candidate for gfx950 — the inner loop of tiddit_variant.get_region
// (tiddit_variant.pyx:54-151), which the reference runs as one random-access BAM re-scan per candidate.
// Here the contig's packed, coordinate-sorted alignment arrays stay in HBM and ONE WAVE answers one query:
//   * the reads a region fetch would return (pos < q_end and end > q_start) lie in [lo, hi) of the sorted
//     starts: hi by binary search on q_end, lo by binary search on q_start - max_span (then `end > q_start` is
//     tested per read);
//   * lane = read, 64 reads per step, the reference's predicate chain is evaluated branch-free into seven
//     per-lane counters, reduced over the wave at the end.
// All seven outputs are order-independent sums, so the result is bit-identical to the sequential loop.
#include "tdt_common.h"
#include "tdt_search.h"      // rg_lower_bound2: the 64-ary search both the region counts and the link counts (tdt_links.hip) use

struct RegionArrays {
    const int32_t *start, *end, *mate_tid, *mate_pos, *tlen;
    const uint8_t *mapq, *has_sa;
    const uint16_t *flag;
    int n;
    int tid;
    int max_span;
    long long contig_length;
};

__global__ __launch_bounds__(256) void region_counts(RegionArrays R, const int32_t *__restrict__ qs, const int32_t *__restrict__ qe,
                                                     const int32_t *__restrict__ qbp, int nq, int min_q, long long max_ins,
                                                     long long *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const long long start = qs[q], end = qe[q], bp = qbp[q];
    long long q_start = start, q_end = end + max_ins;          // :68-75
    if (q_end > R.contig_length) q_end = R.contig_length;
    if (q_start >= q_end) q_start = q_end - 10;
    int lo, hi;   // pos < q_end  <=>  i < hi;   reads before lo end at or before q_start (start + max_span <= q_start)
    rg_lower_bound2<1>(R.start, R.n, q_start - (long long)R.max_span, q_end, lane, lo, hi);
    long long bases = 0;
    unsigned n_reads = 0, low_q = 0, n_discs = 0, n_splits = 0, cross_f = 0, cross_r = 0;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const bool in = i0 + lane < hi;
        const int i = in ? i0 + lane : lo;                                       // all eight loads issue together, predicates after
        const long long rs = R.start[i], re = R.end[i], mpos = R.mate_pos[i];
        long long isz = R.tlen[i];
        const int mtid = R.mate_tid[i];
        const unsigned f = R.flag[i];
        const bool lowq = (int)R.mapq[i] < min_q, sa = R.has_sa[i] != 0;
        bool live = in && re > q_start;                                          // returned by the region fetch
        live = live && !(f & 0x4u);                                              // :84
        live = live && !((f & 0x8u) ? rs > end : (mpos > end && rs > end));      // :89-94
        live = live && !(f & 0x400u);                                            // :96
        const bool counted = live && !(rs > end);                                // :99-102
        n_reads += counted ? 1u : 0u;
        low_q += (counted && lowq) ? 1u : 0u;
        live = live && !lowq;                                                    // :104
        cross_r += (live && rs < bp - 20 && re > bp + 20) ? 1u : 0u;             // :114
        const bool mate_bp_read = mpos < bp - 50 && re > bp + 50;                // :117
        isz = isz < 0 ? -isz : isz;
        const bool discordant = isz > max_ins || mtid != R.tid;                  // :118
        cross_f += (live && mate_bp_read && !discordant) ? 1u : 0u;              // :120
        live = live && !(re < start || rs > end);                                // :123-126
        const long long r_start = rs < start ? start : rs, r_end = re > end ? end : re;
        bases += live ? r_end - r_start + 1 : 0;                                 // :134
        n_splits += (live && sa) ? 1u : 0u;                                      // :136
        n_discs += (live && discordant) ? 1u : 0u;                               // :139
    }
    for (int d = 32; d > 0; d >>= 1) {
        bases += __shfl_xor(bases, d);
        n_reads += __shfl_xor(n_reads, d);
        low_q += __shfl_xor(low_q, d);
        n_discs += __shfl_xor(n_discs, d);
        n_splits += __shfl_xor(n_splits, d);
        cross_f += __shfl_xor(cross_f, d);
        cross_r += __shfl_xor(cross_r, d);
    }
    if (lane == 0) {
        long long *o = out + (size_t)q * 7;
        o[0] = bases; o[1] = n_reads; o[2] = low_q; o[3] = n_discs; o[4] = n_splits; o[5] = cross_f; o[6] = cross_r;
    }
}

extern "C" int tdt_region_counts_device(tdt_ctx *ctx, const int32_t *d_start, const int32_t *d_end, const uint8_t *d_mapq,
                                        const uint16_t *d_flag, const int32_t *d_mate_tid, const int32_t *d_mate_pos,
                                        const int32_t *d_tlen, const uint8_t *d_has_sa, size_t n, int tid, int max_span,
                                        int64_t contig_length, const int32_t *d_q_start, const int32_t *d_q_end,
                                        const int32_t *d_q_bp, size_t nq, int min_q, int64_t max_ins, int64_t *d_out) {
    if (!ctx || n >= 0x7fffffffull || nq >= 0x7fffffffull || (nq && (!d_q_start || !d_q_end || !d_q_bp || !d_out)) ||
        (n && (!d_start || !d_end || !d_mapq || !d_flag || !d_mate_tid || !d_mate_pos || !d_tlen || !d_has_sa))) {
        tdt_set_error("tdt_region_counts_device: bad argument");
        return TDT_E_ARG;
    }
    if (nq == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(ctx->device));
    RegionArrays R{d_start, d_end, d_mate_tid, d_mate_pos, d_tlen, d_mapq, d_has_sa, d_flag, (int)n, tid, max_span, (long long)contig_length};
    const unsigned blocks = (unsigned)((nq + 3) / 4);
    hipLaunchKernelGGL(region_counts, dim3(blocks), dim3(256), 0, ctx->stream, R, d_q_start, d_q_end, d_q_bp, (int)nq, min_q,
                       (long long)max_ins, (long long *)d_out);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

extern "C" int tdt_region_counts(tdt_ctx *ctx, const int32_t *start, const int32_t *end, const uint8_t *mapq, const uint16_t *flag,
                                 const int32_t *mate_tid, const int32_t *mate_pos, const int32_t *tlen, const uint8_t *has_sa,
                                 size_t n, int tid, int64_t contig_length, const int32_t *q_start, const int32_t *q_end,
                                 const int32_t *q_bp, size_t nq, int min_q, int64_t max_ins, int64_t *out) {
    if (!ctx || (nq && (!q_start || !q_end || !q_bp || !out)) ||
        (n && (!start || !end || !mapq || !flag || !mate_tid || !mate_pos || !tlen || !has_sa))) {
        tdt_set_error("tdt_region_counts: bad argument");
        return TDT_E_ARG;
    }
    if (nq == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(ctx->device));
    int max_span = 1;
    for (size_t i = 0; i < n; i++) {
        if (i && start[i] < start[i - 1]) {
            tdt_set_error("tdt_region_counts: reads must be coordinate sorted");
            return TDT_E_ARG;
        }
        const long long sp = (long long)end[i] - start[i];
        if (sp > max_span) max_span = (int)sp;
    }
    const size_t N = n ? n : 1;
    const size_t a4 = (N * 4 + 255) & ~(size_t)255, a2 = (N * 2 + 255) & ~(size_t)255, a1 = (N + 255) & ~(size_t)255;
    const size_t q4 = (nq * 4 + 255) & ~(size_t)255;
    void *d = nullptr;
    int rc = tdt_scratch(ctx, 14, 5 * a4 + a2 + 2 * a1 + 3 * q4 + nq * 56 + 256, &d);
    if (rc) return rc;
    char *p = (char *)d;
    int32_t *ds = (int32_t *)p; p += a4;
    int32_t *de = (int32_t *)p; p += a4;
    int32_t *dmt = (int32_t *)p; p += a4;
    int32_t *dmp = (int32_t *)p; p += a4;
    int32_t *dtl = (int32_t *)p; p += a4;
    uint16_t *df = (uint16_t *)p; p += a2;
    uint8_t *dq = (uint8_t *)p; p += a1;
    uint8_t *dsa = (uint8_t *)p; p += a1;
    int32_t *dqs = (int32_t *)p; p += q4;
    int32_t *dqe = (int32_t *)p; p += q4;
    int32_t *dqb = (int32_t *)p; p += q4;
    int64_t *dout = (int64_t *)p;
    hipStream_t st = ctx->stream;
    if (n) {
        TDT_HIP(hipMemcpyAsync(ds, start, n * 4, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(de, end, n * 4, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(dmt, mate_tid, n * 4, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(dmp, mate_pos, n * 4, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(dtl, tlen, n * 4, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(df, flag, n * 2, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(dq, mapq, n, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(dsa, has_sa, n, hipMemcpyHostToDevice, st));
    }
    TDT_HIP(hipMemcpyAsync(dqs, q_start, nq * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dqe, q_end, nq * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dqb, q_bp, nq * 4, hipMemcpyHostToDevice, st));
    rc = tdt_region_counts_device(ctx, ds, de, dq, df, dmt, dmp, dtl, dsa, n, tid, max_span, contig_length, dqs, dqe, dqb, nq, min_q,
                                  max_ins, dout);
    if (rc) return rc;
    TDT_HIP(hipMemcpyAsync(out, dout, nq * 56, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}

// ---- the evidence store: every placed record of the scan packed into 16 bytes, in file order --------------------------------------
// One record = int4 {start, end, mate_pos, bits}; bits (low byte; the three upper bytes are zero padding) carry every predicate of
// get_region that does not depend on the query: the flag bits it tests, the SA tag, and the two comparisons against the scan's own
// min_q / max_ins.  A coordinate-sorted file appends each contig as one contiguous, sorted range.
// (struct tdt_evstore: tdt_common.h — the depth distribution, tdt_depth_dist.hip, reads the same records)

__global__ __launch_bounds__(256) void evidence_pack(const int32_t *__restrict__ tid, const int32_t *__restrict__ pos,
                                                     const int32_t *__restrict__ end, const uint8_t *__restrict__ mapq,
                                                     const uint16_t *__restrict__ flag, const int32_t *__restrict__ mate_tid,
                                                     const int32_t *__restrict__ mate_pos, const int32_t *__restrict__ tlen,
                                                     const int64_t *__restrict__ sa_off, int n, int min_q, long long max_ins,
                                                     int4 *__restrict__ out, int *__restrict__ span, int n_contigs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n;
    int t = -1, sp = 0;
    if (in) {
        t = tid[i];
        const int s = pos[i], e = end[i];
        const unsigned f = flag[i];
        long long isz = tlen[i];
        isz = isz < 0 ? -isz : isz;
        unsigned bits = f & (TDT_EV_UNMAPPED | TDT_EV_MATE_UNMAPPED);                          // 0x4, 0x8
        bits |= (f & 0x400u) ? TDT_EV_DUPLICATE : 0u;
        bits |= sa_off[i] >= 0 ? TDT_EV_HAS_SA : 0u;
        bits |= (int)mapq[i] < min_q ? TDT_EV_LOW_Q : 0u;
        bits |= (isz > max_ins || mate_tid[i] != t) ? TDT_EV_DISCORDANT : 0u;
        out[i] = make_int4(s, e, mate_pos[i], (int)bits);
        sp = e - s;
    }
    // the max span per contig: one atomic per wave when the wave's records are all on one contig (nearly always)
    const int t0 = __shfl(t, 0);
    if (__all(!in || t == t0)) {
        for (int d = 32; d > 0; d >>= 1) sp = max(sp, __shfl_xor(sp, d));
        if ((threadIdx.x & 63) == 0 && t0 >= 0 && t0 < n_contigs) atomicMax(span + t0, sp);
    } else if (in && t >= 0 && t < n_contigs) {
        atomicMax(span + t, sp);
    }
}

extern "C" int tdt_evstore_create(tdt_ctx *ctx, int n_contigs, int min_q, int64_t max_ins, size_t capacity, tdt_evstore **out) {
    if (!ctx || !out || n_contigs < 0 || max_ins < 0) {
        tdt_set_error("tdt_evstore_create: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_evstore *s = new tdt_evstore{ctx, n_contigs, min_q, (long long)max_ins, nullptr, 0, 0, nullptr};
    const size_t nc = n_contigs ? (size_t)n_contigs : 1;
    if (tdt_dev_malloc((void **)&s->d_span, nc * 4) != hipSuccess ||
        (capacity && tdt_dev_malloc((void **)&s->rec, capacity * sizeof(int4)) != hipSuccess)) {
        if (s->d_span) (void)hipFree(s->d_span);
        delete s;
        tdt_set_error("tdt_evstore_create: out of device memory (%zu records)", capacity);
        return TDT_E_NOMEM;
    }
    s->cap = capacity;
    hipError_t e = hipMemsetAsync(s->d_span, 0, nc * 4, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(s->d_span);
        if (s->rec) (void)hipFree(s->rec);
        delete s;
        tdt_set_error("tdt_evstore_create: hipMemsetAsync: %s", hipGetErrorString(e));
        return TDT_E_HIP;
    }
    *out = s;
    return TDT_OK;
}

extern "C" int tdt_evstore_destroy(tdt_evstore *s) {
    if (!s) return TDT_OK;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);          // (no kernel of the stream still reads or writes the buffers)
    if (s->rec) (void)hipFree(s->rec);
    if (s->d_span) (void)hipFree(s->d_span);
    delete s;
    return TDT_OK;
}

// room for `more` records: a bigger buffer, the records so far copied over on the device (the stream orders the copy behind the packs
// that wrote them), the old buffer freed once the copy is done
static int ev_reserve(tdt_evstore *s, size_t more) {
    if (s->n + more <= s->cap) return TDT_OK;
    size_t want = s->cap + s->cap / 2;
    if (want < s->n + more) want = s->n + more;
    if (want < (1u << 20)) want = 1u << 20;
    int4 *p = nullptr;
    if (tdt_dev_malloc((void **)&p, want * sizeof(int4)) != hipSuccess) {
        tdt_set_error("tdt_evstore: out of device memory growing to %zu records", want);
        return TDT_E_NOMEM;
    }
    if (s->n) TDT_HIP(hipMemcpyAsync(p, s->rec, s->n * sizeof(int4), hipMemcpyDeviceToDevice, s->ctx->stream));
    TDT_HIP(hipStreamSynchronize(s->ctx->stream));
    if (s->rec) TDT_HIP(hipFree(s->rec));
    s->rec = p;
    s->cap = want;
    return TDT_OK;
}

extern "C" int tdt_evstore_append_device(tdt_evstore *s, const int32_t *d_tid, const int32_t *d_pos, const int32_t *d_end,
                                         const uint8_t *d_mapq, const uint16_t *d_flag, const int32_t *d_mate_tid,
                                         const int32_t *d_mate_pos, const int32_t *d_tlen, const int64_t *d_sa_off, size_t n) {
    if (!s || n >= 0x7fffffffull ||
        (n && (!d_tid || !d_pos || !d_end || !d_mapq || !d_flag || !d_mate_tid || !d_mate_pos || !d_tlen || !d_sa_off))) {
        tdt_set_error("tdt_evstore_append_device: bad argument");
        return TDT_E_ARG;
    }
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(s->ctx->device));
    int rc = ev_reserve(s, n);
    if (rc) return rc;
    hipLaunchKernelGGL(evidence_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->ctx->stream, d_tid, d_pos, d_end, d_mapq,
                       d_flag, d_mate_tid, d_mate_pos, d_tlen, d_sa_off, (int)n, s->min_q, s->max_ins, s->rec + s->n, s->d_span,
                       s->n_contigs);
    TDT_CHECK_LAUNCH();
    s->n += n;
    return TDT_OK;
}

extern "C" int tdt_evstore_append(tdt_evstore *s, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint8_t *mapq,
                                  const uint16_t *flag, const int32_t *mate_tid, const int32_t *mate_pos, const int32_t *tlen,
                                  const int64_t *sa_off, size_t n) {
    if (!s || n >= 0x7fffffffull || (n && (!tid || !pos || !end || !mapq || !flag || !mate_tid || !mate_pos || !tlen || !sa_off))) {
        tdt_set_error("tdt_evstore_append: bad argument");
        return TDT_E_ARG;
    }
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(s->ctx->device));
    const size_t a4 = (n * 4 + 255) & ~(size_t)255, a2 = (n * 2 + 255) & ~(size_t)255, a1 = (n + 255) & ~(size_t)255;
    const size_t a8 = (n * 8 + 255) & ~(size_t)255;
    void *d = nullptr;
    int rc = tdt_scratch(s->ctx, 27, 6 * a4 + a2 + a1 + a8, &d);
    if (rc) return rc;
    char *p = (char *)d;
    int32_t *dt = (int32_t *)p; p += a4;
    int32_t *dp = (int32_t *)p; p += a4;
    int32_t *de = (int32_t *)p; p += a4;
    int32_t *dmt = (int32_t *)p; p += a4;
    int32_t *dmp = (int32_t *)p; p += a4;
    int32_t *dtl = (int32_t *)p; p += a4;
    uint16_t *df = (uint16_t *)p; p += a2;
    uint8_t *dq = (uint8_t *)p; p += a1;
    int64_t *dsa = (int64_t *)p;
    hipStream_t st = s->ctx->stream;
    TDT_HIP(hipMemcpyAsync(dt, tid, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dp, pos, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(de, end, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dmt, mate_tid, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dmp, mate_pos, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dtl, tlen, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(df, flag, n * 2, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dq, mapq, n, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dsa, sa_off, n * 8, hipMemcpyHostToDevice, st));
    return tdt_evstore_append_device(s, dt, dp, de, dq, df, dmt, dmp, dtl, dsa, n);
}

extern "C" int tdt_evstore_info(tdt_evstore *s, size_t *n, size_t *capacity, void **d_records) {
    if (!s) {
        tdt_set_error("tdt_evstore_info: bad argument");
        return TDT_E_ARG;
    }
    if (n) *n = s->n;
    if (capacity) *capacity = s->cap;
    if (d_records) *d_records = s->rec;
    return TDT_OK;
}

extern "C" int tdt_evstore_spans(tdt_evstore *s, int32_t *spans) {
    if (!s || (s->n_contigs && !spans)) {
        tdt_set_error("tdt_evstore_spans: bad argument");
        return TDT_E_ARG;
    }
    if (!s->n_contigs) return TDT_OK;
    TDT_HIP(hipSetDevice(s->ctx->device));
    TDT_HIP(hipMemcpyAsync(spans, s->d_span, (size_t)s->n_contigs * 4, hipMemcpyDeviceToHost, s->ctx->stream));
    TDT_HIP(hipStreamSynchronize(s->ctx->stream));
    return TDT_OK;
}

// One wave per query over the store: the query's contig row of the table gives the record range, and everything else is
// region_counts above with the eight column loads replaced by one 16-byte load and the predicates read from the bits.
// CHECK (the device-query entry, whose queries the host never sees): a query naming no row of the table writes zeros and leaves
// the lowest such query index in *bad; the wave's branch is uniform (one query per wave).
template <bool CHECK>
__global__ __launch_bounds__(256) void region_counts_packed(const int4 *__restrict__ rec, const long long *__restrict__ ctab,
                                                            int n_contigs, const int32_t *__restrict__ qry, int nq, long long max_ins,
                                                            long long *__restrict__ out, int *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int4 Q = reinterpret_cast<const int4 *>(qry)[q];                        // (contig index, start, end, bp)
    if (CHECK && (Q.x < 0 || Q.x >= n_contigs)) {
        if (lane < 7) out[(size_t)q * 7 + lane] = 0;
        if (lane == 0) atomicMin(bad, q);
        return;
    }
    const long long *C = ctab + 5 * (size_t)Q.x;                                  // (offset, n, max span, tid, length)
    const int4 *__restrict__ R = rec + C[0];
    const int n = (int)C[1];
    const long long start = Q.y, end = Q.z, bp = Q.w;
    long long q_start = start, q_end = end + max_ins;                             // :68-75
    if (q_end > C[4]) q_end = C[4];
    if (q_start >= q_end) q_start = q_end - 10;
    int lo, hi;
    rg_lower_bound2<4>(reinterpret_cast<const int32_t *>(R), n, q_start - C[2], q_end, lane, lo, hi);
    long long bases = 0;
    unsigned n_reads = 0, low_q = 0, n_discs = 0, n_splits = 0, cross_f = 0, cross_r = 0;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const bool in = i0 + lane < hi;
        const int4 r = R[in ? i0 + lane : lo];
        const long long rs = r.x, re = r.y, mpos = r.z;
        const unsigned b = (unsigned)r.w;
        const bool lowq = b & TDT_EV_LOW_Q, sa = b & TDT_EV_HAS_SA, discordant = b & TDT_EV_DISCORDANT;
        bool live = in && re > q_start;                                          // returned by the region fetch
        live = live && !(b & TDT_EV_UNMAPPED);                                   // :84
        live = live && !((b & TDT_EV_MATE_UNMAPPED) ? rs > end : (mpos > end && rs > end));   // :89-94
        live = live && !(b & TDT_EV_DUPLICATE);                                  // :96
        const bool counted = live && !(rs > end);                                // :99-102
        n_reads += counted ? 1u : 0u;
        low_q += (counted && lowq) ? 1u : 0u;
        live = live && !lowq;                                                    // :104
        cross_r += (live && rs < bp - 20 && re > bp + 20) ? 1u : 0u;             // :114
        const bool mate_bp_read = mpos < bp - 50 && re > bp + 50;                // :117
        cross_f += (live && mate_bp_read && !discordant) ? 1u : 0u;              // :118-120
        live = live && !(re < start || rs > end);                                // :123-126
        const long long r_start = rs < start ? start : rs, r_end = re > end ? end : re;
        bases += live ? r_end - r_start + 1 : 0;                                 // :134
        n_splits += (live && sa) ? 1u : 0u;                                      // :136
        n_discs += (live && discordant) ? 1u : 0u;                               // :139
    }
    for (int d = 32; d > 0; d >>= 1) {
        bases += __shfl_xor(bases, d);
        n_reads += __shfl_xor(n_reads, d);
        low_q += __shfl_xor(low_q, d);
        n_discs += __shfl_xor(n_discs, d);
        n_splits += __shfl_xor(n_splits, d);
        cross_f += __shfl_xor(cross_f, d);
        cross_r += __shfl_xor(cross_r, d);
    }
    if (lane == 0) {
        long long *o = out + (size_t)q * 7;
        o[0] = bases; o[1] = n_reads; o[2] = low_q; o[3] = n_discs; o[4] = n_splits; o[5] = cross_f; o[6] = cross_r;
    }
}

// every contig row of a table inside the store (what every kernel over the store is allowed to touch)
int tdt_evstore_check_rows(const char *fn, const tdt_evstore *s, const int64_t *contigs, int n_contigs) {
    for (int c = 0; c < n_contigs; c++) {          // every range the kernel may touch lies inside the store
        const int64_t *C = contigs + 5 * (size_t)c;
        if (C[0] < 0 || C[1] < 0 || C[1] >= 0x7fffffffll || (size_t)(C[0] + C[1]) > s->n || C[2] < 0 || C[4] < 0) {
            tdt_set_error("%s: contig row %d (offset %lld, n %lld, span %lld, length %lld) outside the store of %zu", fn, c,
                          (long long)C[0], (long long)C[1], (long long)C[2], (long long)C[4], s->n);
            return TDT_E_RANGE;
        }
    }
    return TDT_OK;
}

// the checks both entries make on the host: the store's parameters, and every contig row inside the store
static int packed_check(const char *fn, tdt_evstore *s, const int64_t *contigs, int n_contigs, int min_q, int64_t max_ins) {
    if (min_q != s->min_q || (long long)max_ins != s->max_ins) {
        tdt_set_error("%s: the store was packed with min_q %d / max_ins %lld, the queries ask for %d / %lld", fn, s->min_q, s->max_ins,
                      min_q, (long long)max_ins);
        return TDT_E_ARG;
    }
    return tdt_evstore_check_rows(fn, s, contigs, n_contigs);
}

extern "C" int tdt_region_counts_packed(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, const int32_t *queries,
                                        size_t nq, int min_q, int64_t max_ins, int64_t *out) {
    if (!ctx || !s || n_contigs < 0 || nq >= 0x7fffffffull || (n_contigs && !contigs) || (nq && (!queries || !out))) {
        tdt_set_error("tdt_region_counts_packed: bad argument");
        return TDT_E_ARG;
    }
    int rc = packed_check("tdt_region_counts_packed", s, contigs, n_contigs, min_q, max_ins);
    if (rc) return rc;
    for (size_t q = 0; q < nq; q++) {
        if (queries[4 * q] < 0 || queries[4 * q] >= n_contigs) {
            tdt_set_error("tdt_region_counts_packed: query %zu names contig %d of %d", q, queries[4 * q], n_contigs);
            return TDT_E_RANGE;
        }
    }
    if (nq == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(ctx->device));
    if (ctx != s->ctx) TDT_HIP(hipStreamSynchronize(s->ctx->stream));       // (the packs of another context's stream are complete)
    const size_t ct = ((size_t)n_contigs * 40 + 255) & ~(size_t)255, qb = (nq * 16 + 255) & ~(size_t)255;
    void *d = nullptr;
    rc = tdt_scratch(ctx, 26, ct + qb + nq * 56, &d);
    if (rc) return rc;
    long long *dct = (long long *)d;
    int32_t *dq = (int32_t *)((char *)d + ct);
    long long *dout = (long long *)((char *)d + ct + qb);
    hipStream_t st = ctx->stream;
    TDT_HIP(hipMemcpyAsync(dct, contigs, (size_t)n_contigs * 40, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dq, queries, nq * 16, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(region_counts_packed<false>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, s->rec, dct, n_contigs, dq, (int)nq,
                       (long long)max_ins, dout, nullptr);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipMemcpyAsync(out, dout, nq * 56, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}

// The same counts with the queries and the output on the device (the N-rank variant stage: the queries arrive by a broadcast into a
// device tensor, the partial counts leave by a reduce from one).  The contig table is the host's; the kernel checks the queries' rows.
// The stream is synchronised before the return, so the caller's next collective reads finished counts.
extern "C" int tdt_region_counts_packed_device(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, const int32_t *d_queries,
                                               size_t nq, int min_q, int64_t max_ins, int64_t *d_out) {
    if (!ctx || !s || n_contigs < 0 || nq >= 0x7fffffffull || (n_contigs && !contigs) || (nq && (!d_queries || !d_out)) ||
        ((uintptr_t)d_queries & 15) || ((uintptr_t)d_out & 7)) {
        tdt_set_error("tdt_region_counts_packed_device: bad argument");
        return TDT_E_ARG;
    }
    int rc = packed_check("tdt_region_counts_packed_device", s, contigs, n_contigs, min_q, max_ins);
    if (rc) return rc;
    if (nq == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(ctx->device));
    if (ctx != s->ctx) TDT_HIP(hipStreamSynchronize(s->ctx->stream));
    const size_t ct = ((size_t)n_contigs * 40 + 255) & ~(size_t)255;
    void *d = nullptr;
    rc = tdt_scratch(ctx, 26, ct + 256, &d);
    if (rc) return rc;
    long long *dct = (long long *)d;
    int *dbad = (int *)((char *)d + ct);
    hipStream_t st = ctx->stream;
    int bad = 0x7fffffff;                          // (host words: the stream is synchronised before they go out of scope)
    TDT_HIP(hipMemcpyAsync(dct, contigs, (size_t)n_contigs * 40, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dbad, &bad, sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(region_counts_packed<true>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, s->rec, dct, n_contigs, d_queries,
                       (int)nq, (long long)max_ins, (long long *)d_out, dbad);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipMemcpyAsync(&bad, dbad, sizeof(int), hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    if (bad != 0x7fffffff) {
        int row = 0;
        TDT_HIP(hipMemcpy(&row, d_queries + 4 * (size_t)bad, sizeof(int), hipMemcpyDeviceToHost));
        tdt_set_error("tdt_region_counts_packed_device: query %d names contig %d of %d", bad, row, n_contigs);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}
