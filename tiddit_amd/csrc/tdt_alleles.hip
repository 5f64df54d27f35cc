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
#include "tdt_common.h"

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
    void *d_io;                               // columns + raw bytes of the host entry (grows)
    size_t io_cap;
};

struct AlIn {
    const int32_t *tid, *pos, *end;
    const uint8_t *mapq;
    const uint16_t *flag;
    const uint64_t *rec_off;
    const uint8_t *raw;
};

__device__ __forceinline__ unsigned al_u32(const uint8_t *p) {
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

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
        const unsigned cw = al_u32(cig + 4 * (size_t)w.j), op = cw & 0xf;
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

__device__ __forceinline__ int al_wave_max(int v) {
    for (int d = 32; d > 0; d >>= 1) {
        const int o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
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
    if (lane == 0) s_wsum[wave] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < AL_BLOCK / 64; w++) {
        base += w < wave ? s_wsum[w] : 0;
        total += s_wsum[w];
    }
    if (has) {
        const int k = base + __popcll(m & ((1ull << lane) - 1ull));
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
        if (raw_len >= 36 && ro <= raw_len - 36) {
            const uint8_t *r = I.raw + ro + 4;
            const unsigned bs = al_u32(I.raw + ro), l_name = r[8];
            n_cig = (unsigned)r[12] | ((unsigned)r[13] << 8);
            l_seq = (int)al_u32(r + 16);
            if (n_cig == 0 || l_seq < 1) {             // not a read that counts (and not a malformed one)
                live = false;
                bad = false;
            } else if (32ull + l_name + 4ull * n_cig + ((ull)l_seq + 1) / 2 + (ull)l_seq <= (ull)bs && (ull)bs <= raw_len - 4 - ro) {
                cig = r + 32 + l_name;
                seq = cig + 4 * (size_t)n_cig;
                qual = seq + ((size_t)l_seq + 1) / 2;
                bad = false;
                ull qlen = 0;
                for (unsigned j = 0; j < n_cig; j++) {
                    const unsigned cw = al_u32(cig + 4 * (size_t)j), op = cw & 0xf;
                    if (op > 8) bad = true;
                    if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qlen += cw >> 4;
                }
                suspect = !bad && qlen > (ull)l_seq;   // only such a read can ask for a base it does not have
            }
        }
        if (bad) live = false;
    }
    if (__any(suspect)) {                              // the walk without counting
        const int kmax = al_wave_max(suspect ? ns_mine : 0);
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
    const int kmax = al_wave_max(live ? ns_mine : 0);
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
    if (h->d_pos) (void)hipFree(h->d_pos);
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_cnt) (void)hipFree(h->d_cnt);
    if (h->d_stat) (void)hipFree(h->d_stat);
    if (h->d_io) (void)hipFree(h->d_io);
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
    tdt_alleles *h = new tdt_alleles{ctx, n_contigs, min_q, min_bq, ns, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
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
    return TDT_OK;
}

static int al_launch(tdt_alleles *h, const AlIn &I, size_t n, size_t raw_len) {
    hipLaunchKernelGGL(al_count, dim3((unsigned)((n + AL_BLOCK - 1) / AL_BLOCK)), dim3(AL_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len,
                       (const int32_t *)h->d_pos, (const long long *)h->d_off, h->n_contigs, h->min_q, h->min_bq, h->d_cnt, h->d_stat);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

// One batch of the device ingest: d_arrays14 = the pointer table tdt_ingest_arrays filled (a host array of 14 device pointers).  The
// launch is enqueued on the context's stream; nothing is waited for.
extern "C" int tdt_alleles_push_device(tdt_alleles *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    if (!h || n >= 0x7fffffffull || (n && !d_arrays14)) {
        tdt_set_error("tdt_alleles_push_device: bad argument");
        return TDT_E_ARG;
    }
    if (n == 0 || h->ns == 0) return TDT_OK;
    const void *const *p = d_arrays14;
    if (!p[0] || !p[1] || !p[2] || !p[3] || !p[4] || !p[11] || (raw_len && !p[13])) {
        tdt_set_error("tdt_alleles_push_device: a column of the batch is NULL");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    const AlIn I{(const int32_t *)p[0], (const int32_t *)p[1], (const int32_t *)p[2], (const uint8_t *)p[3], (const uint16_t *)p[4],
                 (const uint64_t *)p[11], (const uint8_t *)p[13]};
    return al_launch(h, I, n, raw_len);
}

// The same kernel on host columns and host record bytes (uploaded into the handle's own block).  The stream is synchronised before the
// return: the caller's arrays are free again.
extern "C" int tdt_alleles_push(tdt_alleles *h, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint8_t *mapq,
                                const uint16_t *flag, const uint64_t *rec_off, size_t n, const uint8_t *raw, size_t raw_len) {
    if (!h || n >= 0x7fffffffull || (n && (!tid || !pos || !end || !mapq || !flag || !rec_off)) || (raw_len && !raw)) {
        tdt_set_error("tdt_alleles_push: bad argument");
        return TDT_E_ARG;
    }
    if (n == 0 || h->ns == 0) return TDT_OK;
    tdt_ctx *ctx = h->ctx;
    TDT_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    tdt_carver sz(nullptr);
    sz.take<int32_t>(3 * n), sz.take<uint64_t>(n), sz.take<uint16_t>(n), sz.take<uint8_t>(n), sz.take<uint8_t>(raw_len + 1);
    if (sz.size > h->io_cap) {
        TDT_HIP(hipStreamSynchronize(st));
        if (h->d_io) TDT_HIP(hipFree(h->d_io));
        h->d_io = nullptr;
        h->io_cap = 0;
        if (tdt_dev_malloc(&h->d_io, sz.size) != hipSuccess) {
            tdt_set_error("tdt_alleles_push: out of device memory (%zu reads, %zu bytes)", n, raw_len);
            return TDT_E_NOMEM;
        }
        h->io_cap = sz.size;
    }
    tdt_carver cv(h->d_io);
    int32_t *d3 = cv.take<int32_t>(3 * n);
    uint64_t *doff = cv.take<uint64_t>(n);
    uint16_t *dflag = cv.take<uint16_t>(n);
    uint8_t *dmapq = cv.take<uint8_t>(n);
    uint8_t *draw = cv.take<uint8_t>(raw_len + 1);
    TDT_HIP(hipMemcpyAsync(d3, tid, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(d3 + n, pos, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(d3 + 2 * n, end, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(doff, rec_off, n * 8, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dflag, flag, n * 2, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dmapq, mapq, n, hipMemcpyHostToDevice, st));
    if (raw_len) TDT_HIP(hipMemcpyAsync(draw, raw, raw_len, hipMemcpyHostToDevice, st));
    const AlIn I{d3, d3 + n, d3 + 2 * n, dmapq, dflag, doff, draw};
    const int rc = al_launch(h, I, n, raw_len);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(st));
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
