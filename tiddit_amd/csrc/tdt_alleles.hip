// Allele counts at known SNV sites for gfx950 — the bases the reads of the --sv scan carry at the positions of a sites file
// (TIDDIT_ALLELES): per site eight uint32 counters A C G T N DEL SKIP LOWBQ.  The definition is tiddit_alleles.py's.
// A handle keeps the sites (per contig sorted and unique, contig-major) and the zeroed counters in HBM; every batch of the scan costs
// ONE launch over its field columns and its raw record bytes, which are already resident:
//   * lane = read.  The filters (tid, flag, mapq) are tested on the columns; a read that passes finds the sites in [pos, end) of its
//     contig's range by two lower bounds.  The file is coordinate sorted, so the lanes of a wave walk the same few cache lines.
//     Most reads hold no site: their record bytes are never touched.
//   * the reads that hold a site are compacted within the workgroup (ballot + LDS), so the waves behind the compacted list leave and
//     the lanes of the first ones all have a CIGAR to walk.
//   * lane = compacted read.  The record is bounded first (block_size against the record's own fields and against raw_len, every op
//     code <= 8): nothing outside [rec_off, rec_off + 4 + block_size) is read afterwards.  The CIGAR is walked ONCE for all the read's
//     sites (they ascend, so the walk only moves forward).  A read whose CIGAR asks for more query bases than l_seq holds is walked
//     once more in front of that, without counting: a site whose query index is >= l_seq makes the whole read malformed.
//   * step k of a wave handles the k-th site of every lane: equal (site, column) keys are merged over the wave and ONE lane issues the
//     atomic with the number of lanes that share the key (30 neighbouring reads on one site: two or three atomics, not 30).
// Every counter is an order-independent integer sum: the result equals the per-read definition exactly.
#include "tdt_batch.h"
#include "tdt_bam_record.h"
#include "tdt_phase.h"

typedef unsigned long long ull;

#define AL_BLOCK 256
#define AL_MAX_SITES (1ll << 28)             // (site * 8 + column is a 32-bit key)
enum { AL_A = 0, AL_C, AL_G, AL_T, AL_N, AL_DEL, AL_SKIP, AL_LOWBQ, AL_COLS };
#define AL_FLAG_MASK 0xF04u                   // unmapped, secondary, QC fail, duplicate, supplementary

struct tdt_alleles {
    tdt_ctx *ctx;
    int n_contigs, min_q, min_bq;
    size_t ns;
    int32_t *d_pos;                           // ns site positions, 0-based, contig-major
    long long *d_off;                         // n_contigs + 1
    unsigned *d_cnt;                          // ns * 8
    ull *d_stat;                              // {reads used, malformed}
    tdt_batch_io io;                          // columns + raw bytes of the host entry
    tdt_phase *phase;                         // TIDDIT_PHASE: made by tdt_alleles_phase_enable (csrc/tdt_phase.hip), else NULL
    bool pushed;                              // a batch has been pushed since the create or the last reset
};

struct AlIn {
    const int32_t *tid, *pos, *end;
    const uint8_t *mapq;
    const uint16_t *flag;
    const uint64_t *rec_off;
    const uint8_t *raw;
};

// first index in [lo, hi) whose site is >= v
__device__ __forceinline__ long long al_lower_bound(const int32_t *__restrict__ s, long long lo, long long hi, int v) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (s[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct AlWalk {
    unsigned j;            // CIGAR operation
    long long r, q;        // reference position / query index of its first base
};

// The column site s (>= every site asked before, >= pos) adds to: AL_*; -1: no operation of the CIGAR touches it; -2: its query
// index is >= l_seq.  Reads cig[0, 4 * n_cig), seq[0, (l_seq + 1) / 2) and qual[0, l_seq) only.
__device__ __forceinline__ int al_site(const uint8_t *__restrict__ cig, unsigned n_cig, const uint8_t *__restrict__ seq,
                                       const uint8_t *__restrict__ qual, int l_seq, int min_bq, AlWalk &w, int s) {
    while (w.j < n_cig) {
        const unsigned cw = tdt_ld_u32(cig + 4 * (size_t)w.j), op = cw & 0xf;
        const long long len = cw >> 4;
        const bool ref = op == 0 || op == 2 || op == 3 || op == 7 || op == 8;       // M D N = X
        const bool qry = op == 0 || op == 1 || op == 4 || op == 7 || op == 8;       // M I S = X
        if (ref && s < w.r + len) {
            if (op == 2) return AL_DEL;
            if (op == 3) return AL_SKIP;
            const long long qi = w.q + (s - w.r);
            if (qi >= l_seq) return -2;
            const unsigned b = seq[qi >> 1], nib = (qi & 1) ? (b & 0xf) : (b >> 4);
            const unsigned ql = qual[qi];
            if (ql != 0xff && (int)ql < min_bq) return AL_LOWBQ;
            return nib == 1 ? AL_A : nib == 2 ? AL_C : nib == 4 ? AL_G : nib == 8 ? AL_T : AL_N;
        }
        if (ref) w.r += len;
        if (qry) w.q += len;
        w.j++;
    }
    return -1;
}

__global__ __launch_bounds__(AL_BLOCK) void al_count(AlIn I, int n, ull raw_len, const int32_t *__restrict__ site_pos,
                                                     const long long *__restrict__ site_off, int n_contigs, int min_q, int min_bq,
                                                     unsigned *__restrict__ cnt, ull *__restrict__ stat) {
    __shared__ int s_read[AL_BLOCK], s_lo[AL_BLOCK], s_hi[AL_BLOCK];
    __shared__ int s_wsum[AL_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long i = (long long)blockIdx.x * AL_BLOCK + t;
    // ---- lane = read: filters on the columns, the sites in [pos, end)
    int lo = 0, hi = 0;
    if (i < n) {
        const int c = I.tid[i];
        if (c >= 0 && c < n_contigs && (I.flag[i] & AL_FLAG_MASK) == 0 && (int)I.mapq[i] >= min_q) {
            const int p = I.pos[i], e = I.end[i];
            const long long o0 = site_off[c], o1 = site_off[c + 1];
            if (o1 > o0 && e > p) {
                const long long a = al_lower_bound(site_pos, o0, o1, p);
                if (a < o1 && site_pos[a] < e) {
                    lo = (int)a;
                    hi = (int)al_lower_bound(site_pos, a + 1, o1, e);
                }
            }
        }
    }
    // ---- the reads that hold a site, compacted in read order
    const bool has = hi > lo;
    const ull m = __ballot(has);
    const tdt_slots S = tdt_block_slots<AL_BLOCK / 64>(m, s_wsum, lane, wave);
    const int total = S.total;
    if (has) {
        const int k = S.base + tdt_lane_rank(m, lane);
        s_read[k] = (int)i;
        s_lo[k] = lo;
        s_hi[k] = hi;
    }
    __syncthreads();
    if (wave * 64 >= total) return;                    // (a whole wave: the branch is uniform)
    // ---- lane = compacted read: bound the record, then walk it
    bool live = t < total, bad = false, suspect = false;
    int ri = 0, l_seq = 0, pos = 0, ns_mine = 0;
    unsigned n_cig = 0;
    const uint8_t *cig = nullptr, *seq = nullptr, *qual = nullptr;
    lo = 0;
    if (live) {
        ri = s_read[t];
        lo = s_lo[t];
        ns_mine = s_hi[t] - lo;
        pos = I.pos[ri];
        const ull ro = I.rec_off[ri];
        bad = true;
        if (TDT_REC_HEADER_INSIDE(raw_len, ro)) {
            const tdt_rec R = TDT_REC_READ(I.raw, ro);
            n_cig = R.n_cig;
            l_seq = R.l_seq;
            if (n_cig == 0 || l_seq < 1) {             // not a read that counts (and not a malformed one)
                live = false;
                bad = false;
            } else if (TDT_REC_FITS(R, raw_len)) {
                cig = I.raw + R.cig();
                seq = I.raw + R.seq();
                qual = I.raw + R.qual();
                bad = false;
                ull qlen = 0;
                for (unsigned j = 0; j < n_cig; j++) {
                    const unsigned cw = tdt_ld_u32(cig + 4 * (size_t)j), op = cw & 0xf;
                    if (op > 8) bad = true;
                    if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qlen += cw >> 4;
                }
                suspect = !bad && qlen > (ull)l_seq;   // only such a read can ask for a base it does not have
            }
        }
        if (bad) live = false;
    }
    if (__any(suspect)) {                              // the walk without counting
        const int kmax = tdt_wave_reduce<tdt_max>(suspect ? ns_mine : 0);
        AlWalk w{0u, (long long)pos, 0ll};
        for (int k = 0; k < kmax; k++)
            if (suspect && !bad && k < ns_mine && al_site(cig, n_cig, seq, qual, l_seq, min_bq, w, site_pos[lo + k]) == -2) bad = true;
        if (bad) live = false;
    }
    const ull m_used = __ballot(live), m_bad = __ballot(bad);
    if (lane == 0) {
        if (m_used) atomicAdd(&stat[0], (ull)__popcll(m_used));
        if (m_bad) atomicAdd(&stat[1], (ull)__popcll(m_bad));
    }
    const int kmax = tdt_wave_reduce<tdt_max>(live ? ns_mine : 0);
    AlWalk w{0u, (long long)pos, 0ll};
    for (int k = 0; k < kmax; k++) {
        int col = -1;
        if (live && k < ns_mine) col = al_site(cig, n_cig, seq, qual, l_seq, min_bq, w, site_pos[lo + k]);
        const unsigned key = col >= 0 ? (unsigned)(lo + k) * AL_COLS + (unsigned)col : 0xffffffffu;
        ull todo = __ballot(col >= 0);
        while (todo) {                                 // (uniform: every lane of the wave holds the same mask)
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned lk = __shfl(key, leader);
            const ull same = __ballot(key == lk) & todo;
            if (lane == leader) atomicAdd(&cnt[lk], (unsigned)__popcll(same));
            todo &= ~same;
        }
    }
}

static void al_free(tdt_alleles *h) {
    if (h->phase) tdt_phase_free(h->phase);
    if (h->d_pos) (void)hipFree(h->d_pos);
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_cnt) (void)hipFree(h->d_cnt);
    if (h->d_stat) (void)hipFree(h->d_stat);
    if (h->io.d) (void)hipFree(h->io.d);
    delete h;
}

extern "C" int tdt_alleles_create(tdt_ctx *ctx, const int32_t *site_pos, const int64_t *site_off, int n_contigs, int min_q, int min_bq,
                                  tdt_alleles **out) {
    if (!ctx || !out || n_contigs < 0 || !site_off || site_off[0] != 0) {
        tdt_set_error("tdt_alleles_create: bad argument");
        return TDT_E_ARG;
    }
    if (min_bq < 0 || min_bq > 93) {
        tdt_set_error("tdt_alleles_create: min_bq %d is outside 0 ... 93", min_bq);
        return TDT_E_RANGE;
    }
    for (int c = 0; c < n_contigs; c++) {
        if (site_off[c + 1] < site_off[c]) {
            tdt_set_error("tdt_alleles_create: site offsets must not decrease (contig %d)", c);
            return TDT_E_ARG;
        }
    }
    const int64_t ns64 = site_off[n_contigs];
    if (ns64 >= AL_MAX_SITES) {
        tdt_set_error("tdt_alleles_create: %lld sites; the handle keeps fewer than 2^28", (long long)ns64);
        return TDT_E_RANGE;
    }
    const size_t ns = (size_t)ns64;
    if (ns && !site_pos) {
        tdt_set_error("tdt_alleles_create: bad argument");
        return TDT_E_ARG;
    }
    for (int c = 0; c < n_contigs; c++) {
        for (int64_t k = site_off[c]; k < site_off[c + 1]; k++) {
            if (site_pos[k] < 0 || (k > site_off[c] && site_pos[k] <= site_pos[k - 1])) {
                tdt_set_error("tdt_alleles_create: the sites of contig %d are not sorted, unique and >= 0 (site %lld)", c, (long long)k);
                return TDT_E_ARG;
            }
        }
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_alleles *h = new tdt_alleles{ctx, n_contigs, min_q, min_bq, ns, nullptr, nullptr, nullptr, nullptr, {nullptr, 0}, nullptr, false};
    const size_t N = ns ? ns : 1;
    if (tdt_dev_malloc((void **)&h->d_pos, N * 4) != hipSuccess || tdt_dev_malloc((void **)&h->d_off, (size_t)(n_contigs + 1) * 8) != hipSuccess ||
        tdt_dev_malloc((void **)&h->d_cnt, N * AL_COLS * 4) != hipSuccess || tdt_dev_malloc((void **)&h->d_stat, 256) != hipSuccess) {
        al_free(h);
        tdt_set_error("tdt_alleles_create: out of device memory (%zu sites)", ns);
        return TDT_E_NOMEM;
    }
    hipStream_t st = ctx->stream;
    auto body = [&]() -> int {
        if (ns) TDT_HIP(hipMemcpyAsync(h->d_pos, site_pos, ns * 4, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(h->d_off, site_off, (size_t)(n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemsetAsync(h->d_cnt, 0, N * AL_COLS * 4, st));
        TDT_HIP(hipMemsetAsync(h->d_stat, 0, 256, st));
        TDT_HIP(hipStreamSynchronize(st));             // (the host arrays are free again)
        return TDT_OK;
    };
    const int rc = body();
    if (rc) {
        al_free(h);
        return rc;
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_alleles_destroy(tdt_alleles *h) {
    if (!h) return TDT_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);        // (no kernel of the stream still adds to the counters)
    al_free(h);
    return TDT_OK;
}

extern "C" int tdt_alleles_reset(tdt_alleles *h) {
    if (!h) {
        tdt_set_error("tdt_alleles_reset: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    TDT_HIP(hipMemsetAsync(h->d_cnt, 0, (h->ns ? h->ns : 1) * AL_COLS * 4, h->ctx->stream));
    TDT_HIP(hipMemsetAsync(h->d_stat, 0, 256, h->ctx->stream));
    h->pushed = false;
    return h->phase ? tdt_phase_reset(h->phase) : TDT_OK;
}

static int al_launch(tdt_alleles *h, const AlIn &I, size_t n, size_t raw_len) {
    hipLaunchKernelGGL(al_count, dim3((unsigned)((n + AL_BLOCK - 1) / AL_BLOCK)), dim3(AL_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len,
                       (const int32_t *)h->d_pos, (const long long *)h->d_off, h->n_contigs, h->min_q, h->min_bq, h->d_cnt, h->d_stat);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

#define AL_NEED (TDT_NEED(TID) | TDT_NEED(POS) | TDT_NEED(END) | TDT_NEED(MAPQ) | TDT_NEED(FLAG) | TDT_NEED(REC_OFF) | TDT_NEED(RAW))

// One batch of the device ingest: d_arrays14 = the pointer table tdt_ingest_arrays filled (TDT_COL_*: a host array of TDT_NCOL device
// pointers).  The launch is enqueued on the context's stream; nothing is waited for.
extern "C" int tdt_alleles_push_device(tdt_alleles *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    tdt_batch B;                                       // (a handle without sites reads no column: none is asked for)
    const int rc = tdt_batch_view("tdt_alleles_push_device", h, d_arrays14, n, raw_len, h && h->ns ? AL_NEED : 0u, &B);
    if (rc) return rc;
    if (n == 0 || h->ns == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    h->pushed = true;
    const int rc2 = al_launch(h, AlIn{B.tid, B.pos, B.end, B.mapq, B.flag, B.rec_off, B.raw}, n, raw_len);
    return rc2 == TDT_OK && h->phase ? tdt_phase_push(h->phase, B, n, raw_len) : rc2;
}

// The same kernel on host columns and host record bytes (uploaded into the handle's own block).  The stream is synchronised before the
// return: the caller's arrays are free again.
extern "C" int tdt_alleles_push(tdt_alleles *h, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint8_t *mapq,
                                const uint16_t *flag, const uint64_t *rec_off, size_t n, const uint8_t *raw, size_t raw_len) {
    tdt_batch H{}, B;
    H.tid = tid, H.pos = pos, H.end = end, H.mapq = mapq, H.flag = flag, H.rec_off = rec_off, H.raw = raw;
    int rc = tdt_batch_host("tdt_alleles_push", h, H, n, raw_len, AL_NEED);
    if (rc) return rc;
    // (no tdt_batch_offsets_ascend here, unlike tdt_qc_push / tdt_dup_push: this entry has never refused offsets that decrease, and
    // al_count bounds every record by itself)
    if (n == 0 || h->ns == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    h->pushed = true;
    rc = tdt_batch_upload("tdt_alleles_push", h->ctx, &h->io, H, AL_NEED, n, raw_len, &B);
    if (rc == TDT_OK) rc = al_launch(h, AlIn{B.tid, B.pos, B.end, B.mapq, B.flag, B.rec_off, B.raw}, n, raw_len);
    if (rc == TDT_OK && h->phase) rc = tdt_phase_push(h->phase, B, n, raw_len);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

// uint32[ns][8] and the two read counters to the host, behind everything pushed so far
extern "C" int tdt_alleles_counts(tdt_alleles *h, uint32_t *out, uint64_t *reads_used, uint64_t *malformed) {
    if (!h || (h->ns && !out)) {
        tdt_set_error("tdt_alleles_counts: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    ull stat[2] = {0, 0};
    if (h->ns) TDT_HIP(hipMemcpyAsync(out, h->d_cnt, h->ns * AL_COLS * 4, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipMemcpyAsync(stat, h->d_stat, sizeof(stat), hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    if (reads_used) *reads_used = stat[0];
    if (malformed) *malformed = stat[1];
    return TDT_OK;
}

// ... to device memory: d_out uint32[ns][8], d_stat2 uint64[2] {reads used, malformed} (either may be NULL).  The stream is synchronised
// before the return.
extern "C" int tdt_alleles_counts_device(tdt_alleles *h, uint32_t *d_out, uint64_t *d_stat2) {
    if (!h || ((uintptr_t)d_out & 3) || ((uintptr_t)d_stat2 & 7)) {
        tdt_set_error("tdt_alleles_counts_device: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    if (h->ns && d_out) TDT_HIP(hipMemcpyAsync(d_out, h->d_cnt, h->ns * AL_COLS * 4, hipMemcpyDeviceToDevice, st));
    if (d_stat2) TDT_HIP(hipMemcpyAsync(d_stat2, h->d_stat, 16, hipMemcpyDeviceToDevice, st));
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}

// ---- TIDDIT_PHASE: the observation store beside the counters (csrc/tdt_phase.hip).  site_codes = one byte per device site, ref2 | alt2 << 2
// or 0xff for a site that is not phaseable.  Before the first push only (the store and the counters hold the same reads); a second
// call, a call behind a push, or n_sites that is not the handle's: TDT_E_ARG.
tdt_phase *tdt_alleles_phase_of(tdt_alleles *h) { return h ? h->phase : nullptr; }

extern "C" int tdt_alleles_phase_enable(tdt_alleles *h, const uint8_t *site_codes, size_t n_sites, size_t capacity, int hash_bits) {
    if (!h || h->phase || h->pushed || n_sites != h->ns || (n_sites && !site_codes)) {
        tdt_set_error("tdt_alleles_phase_enable: bad argument, enabled already, pushed to already, or not the handle's %zu sites", h ? h->ns : (size_t)0);
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    return tdt_phase_create(h->ctx, h->d_pos, h->d_off, h->ns, h->n_contigs, h->min_q, h->min_bq, site_codes, capacity, hash_bits, &h->phase);
}
