// Copy-number segments from the 50-bp depth bins of the --sv scan (TIDDIT_CNV, tiddit_cnv.py), gfx950: the CNV bins of every processed
// contig (cnv_bins_kernel) and an exact Viterbi segmentation over them (five kernels), all contigs in one call each.
//
// The model (tiddit_cnv.py has the definition): 8 states = copy numbers 0 .. 7, emission e_t(k) = min(cap, (x_t - unit * k)^2), 0 for a
// masked bin (x_t < 0), one jump cost lambda between any two states.  With a uniform jump cost a step is
//     V_t(k) = e_t(k) + min(V_{t-1}(k), m + lambda),   m = min_i V_{t-1}(i)
// — the (min,+) product of the row vector V_{t-1} with M_t[i][k] = e_t(k) + (i == k ? 0 : lambda).  Everything is int64, (min,+) over the
// integers is associative, so the chain is cut into chunks of CNV_CHUNK bins and stitched, and the result IS the sequential
// definition's: no tolerance anywhere.  The start of a contig is a step like any other from the vector (k == P ? 0 : CNV_BIG): CNV_BIG
// never wins a minimum and never overflows (the entries bound unit, cap, lambda and the number of bins so that every real cost is
// below 2^60).
//   cnv_chunk_matrices  one wavefront per chunk: lane (i, j) of the 64 holds the best cost from entering the chunk in state i to being
//                       in state j; a step is a row minimum over 8 lanes (three __shfl_xor) and an add.  -> the chunk's 8x8 matrix.
//   cnv_carry           one wavefront per contig: the 8-vector through the chunk matrices in order (the next matrix is loaded while
//                       this one is applied); every chunk's incoming vector is kept, and the contig's end state.
//   cnv_backpointers    one wavefront per 8 chunks, 8 lanes per chunk: the same walk from the chunk's true incoming vector.  B_t(k) is
//                       k or the lowest argmin a, so a bin's back-pointers are 11 bits: the mask of states that jump, and a.  The walk
//                       also composes the chunk's end-state -> entry-state map (3 bits per state).
//   cnv_chunk_ends      one wavefront per contig: the maps backwards, 64 at a load, to every chunk's end state.
//   cnv_backtrace       one lane per chunk: from its end state back through its bins into state[].
#include "tdt_common.h"

#define CNV_CHUNK 256              // bins per chunk of the Viterbi chain
#define CNV_STATES 8               // copy numbers 0 .. 7: a row of the wavefront's 8 x 8 lanes
#define CNV_CLASSES 101            // GC classes 0 .. 100 (per cent)
#define CNV_BIG (1ll << 61)        // "no path": above every real cost (< 2^60), and CNV_BIG + a real cost fits int64
#define CNV_MAX_PARAM (1ll << 28)  // cap and lambda at most; with fewer than 2^31 bins a path costs less than 2^60
#define CNV_MAX_UNIT (1 << 20)

typedef long long ll;
typedef unsigned long long ull;

struct CnvBinRow {
    ll off, nb, K, P, toff;
};
struct CnvSeqRow {
    ll toff, T, P, choff;          // choff: the contig's first chunk
};

// the last s with start[s] <= g (start is non-decreasing, start[0] == 0 <= g): the row that owns item g — rows without items share
// their start with the row behind them and are never the last
__device__ static inline int cnv_find(const ll *__restrict__ start, int n, ll g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ static inline ll cnv_min(ll a, ll b) { return b < a ? b : a; }

// ---- CNV bins -----------------------------------------------------------------------------------------------------------------
// one lane per CNV bin: both sums in the stated order (left to right over at most 64 bins), one division, one multiplication, rint
__global__ __launch_bounds__(256) void cnv_bins_kernel(const double *__restrict__ cov, const signed char *__restrict__ gc,
                                                        const CnvBinRow *__restrict__ rows, const ll *__restrict__ tstart, int nseg,
                                                        const double *__restrict__ E, int unit, ll total, int *__restrict__ x) {
    const ll g = (ll)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int s = cnv_find(tstart, nseg, g);
    const CnvBinRow r = rows[s];
    const ll b0 = (g - r.toff) * r.K, b1 = b0 + r.K < r.nb ? b0 + r.K : r.nb;
    int n = 0;
    double obs = 0.0, ex = 0.0;
    for (ll b = b0; b < b1; b++) {
        const unsigned c = (unsigned)(int)gc[r.off + b];
        if (c < (unsigned)CNV_CLASSES) {              // (-1 is not usable; nothing else outside 0 .. 100 is a GC bin)
            n++;
            obs += cov[r.off + b];
            ex += E[(size_t)s * CNV_CLASSES + c];
        }
    }
    int v = -1;
    if (2 * n >= r.K) {
        const double q = rint((obs / ex) * (double)(r.P * unit)), top = (double)(8 * unit);
        v = q < top ? (int)q : 8 * unit;              // (also where the ratio is not a number)
    }
    x[g] = v;
}

// ---- the walk shared by the chunk matrices and the back-pointers ------------------------------------------------------------
// Lanes are 8 rows of 8: lane (row, j) holds V(j) of its row's chain, which runs over x[t0 .. t0 + len) — t0 / len are the row's,
// maxlen is the wavefront's largest len.  Every lane runs every step (the cross-lane operations need them); a row past its len keeps
// its values.  RECORD: bp[t] = (mask of the states that jump) | a << 8, and map = the entry state the chain reaches from end state j.
template <bool RECORD>
__device__ static inline void cnv_walk(const int *__restrict__ x, ll t0, int len, int maxlen, int lane, ll unit, ll cap, ll lambda, ll &V,
                                       unsigned short *__restrict__ bp, int &map) {
    const int j = lane & 7, row = lane & ~7;
    const ll centre = unit * j;
    for (int b = 0; b < maxlen; b += 8) {
        const int xv = b + j < len ? x[t0 + b + j] : -1;          // the row's next 8 bins, one per lane
        const int steps = maxlen - b < 8 ? maxlen - b : 8;
        for (int s = 0; s < steps; s++) {
            const int xt = __shfl(xv, row | s);
            const bool act = b + s < len;
            ll m = V;
            m = cnv_min(m, __shfl_xor(m, 1));
            m = cnv_min(m, __shfl_xor(m, 2));
            m = cnv_min(m, __shfl_xor(m, 4));
            const ll d = (ll)xt - centre;
            const ll e = xt < 0 ? 0 : cnv_min(cap, d * d);
            const ll jump = m + lambda;
            const bool stay = V <= jump;
            if (RECORD) {
                const ull bj = __ballot(!stay), bm = __ballot(V == m);
                const unsigned jm = (unsigned)(bj >> row) & 255u;
                const int a = __ffs((unsigned)(bm >> row) & 255u) - 1;       // the lowest state attaining m (some lane of the row does)
                const int from = __shfl(map, row | a);                       // (every lane: the lane of state a itself stays)
                if (act) {
                    map = stay ? map : from;
                    if (j == 0) bp[t0 + b + s] = (unsigned short)(jm | ((unsigned)a << 8));
                }
            }
            const ll nv = e + (stay ? V : jump);
            if (act) V = nv;
        }
    }
}

__device__ static inline void cnv_chunk_of(const CnvSeqRow *__restrict__ rows, const ll *__restrict__ choff, int nseg, ll c, ll &t0, int &len) {
    const CnvSeqRow r = rows[cnv_find(choff, nseg, c)];
    const ll first = (c - r.choff) * CNV_CHUNK;
    t0 = r.toff + first;
    len = (int)(r.T - first < CNV_CHUNK ? r.T - first : CNV_CHUNK);
}

// pass 1: A[c][i * 8 + j]
__global__ __launch_bounds__(256) void cnv_chunk_matrices(const int *__restrict__ x, const CnvSeqRow *__restrict__ rows,
                                                           const ll *__restrict__ choff, int nseg, ll nchunks, ll unit, ll cap, ll lambda,
                                                           ll *__restrict__ A) {
    const int lane = threadIdx.x & 63;
    const ll c = (ll)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nchunks) return;                         // (the whole wavefront)
    ll t0;
    int len, map = 0;
    cnv_chunk_of(rows, choff, nseg, c, t0, len);
    ll V = (lane >> 3) == (lane & 7) ? 0 : CNV_BIG;   // the identity of (min,+)
    cnv_walk<false>(x, t0, len, len, lane, unit, cap, lambda, V, nullptr, map);
    A[c * 64 + lane] = V;
}

// pass 2: vin[c][8] = the vector entering chunk c; contig_end[s] = the lowest state attaining the minimal end cost
__global__ __launch_bounds__(64) void cnv_carry(const CnvSeqRow *__restrict__ rows, const ll *__restrict__ A, ll lambda, ll *__restrict__ vin,
                                                 int *__restrict__ contig_end) {
    const CnvSeqRow r = rows[blockIdx.x];
    if (r.T == 0) return;
    const int lane = threadIdx.x, i = lane >> 3, j = lane & 7;
    const ll nch = (r.T + CNV_CHUNK - 1) / CNV_CHUNK;
    const ll *a = A + r.choff * 64;
    ll v = i == r.P ? 0 : CNV_BIG;                    // lane (i, j) holds v(i)
    ll next = a[lane];
    for (ll c = 0; c < nch; c++) {
        const ll cur = next;
        if (c + 1 < nch) next = a[(c + 1) * 64 + lane];
        if (j == 0) vin[(r.choff + c) * 8 + i] = v;
        ll w = v + cur;                               // column minimum over i: every lane (., j) then holds the new v(j)
        w = cnv_min(w, __shfl_xor(w, 8));
        w = cnv_min(w, __shfl_xor(w, 16));
        w = cnv_min(w, __shfl_xor(w, 32));
        v = __shfl(w, i);
    }
    const ll cost = v + (i == r.P ? 0 : lambda);
    ll m = cost;
    m = cnv_min(m, __shfl_xor(m, 8));
    m = cnv_min(m, __shfl_xor(m, 16));
    m = cnv_min(m, __shfl_xor(m, 32));
    const ull hit = __ballot(cost == m && j == 0);    // bit 8 i for state i
    if (lane == 0) contig_end[blockIdx.x] = (__ffsll((ll)hit) - 1) >> 3;
}

// pass 3: bp[t] of every bin, emap[c] = 3 bits per end state j: the state of the bin before the chunk
__global__ __launch_bounds__(256) void cnv_backpointers(const int *__restrict__ x, const CnvSeqRow *__restrict__ rows, const ll *__restrict__ choff,
                                                         int nseg, ll nchunks, ll unit, ll cap, ll lambda, const ll *__restrict__ vin,
                                                         unsigned short *__restrict__ bp, unsigned *__restrict__ emap) {
    const int lane = threadIdx.x & 63, k = lane & 7;
    const ll first = ((ll)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8;
    if (first >= nchunks) return;                     // (the whole wavefront)
    const ll c = first + (lane >> 3);
    ll t0 = 0, V = 0;
    int len = 0, map = k;
    if (c < nchunks) {
        cnv_chunk_of(rows, choff, nseg, c, t0, len);
        V = vin[c * 8 + k];
    }
    int maxlen = len;
    for (int d = 8; d < 64; d <<= 1) {
        const int o = __shfl_xor(maxlen, d);
        maxlen = o > maxlen ? o : maxlen;
    }
    cnv_walk<true>(x, t0, len, maxlen, lane, unit, cap, lambda, V, bp, map);
    unsigned pm = (unsigned)map << (3 * k);
    pm |= __shfl_xor(pm, 1);
    pm |= __shfl_xor(pm, 2);
    pm |= __shfl_xor(pm, 4);
    if (c < nchunks && k == 0) emap[c] = pm;
}

// pass 4: cend[c] = the state of chunk c's last bin
__global__ __launch_bounds__(64) void cnv_chunk_ends(const CnvSeqRow *__restrict__ rows, const unsigned *__restrict__ emap,
                                                      const int *__restrict__ contig_end, signed char *__restrict__ cend) {
    const CnvSeqRow r = rows[blockIdx.x];
    if (r.T == 0) return;
    const int lane = threadIdx.x;
    const ll nch = (r.T + CNV_CHUNK - 1) / CNV_CHUNK;
    int e = contig_end[blockIdx.x];                   // (the same in every lane, here and below)
    for (ll hi = nch - 1; hi >= 0; hi -= 64) {
        const ll idx = hi - lane;
        const unsigned pm = idx >= 0 ? emap[r.choff + idx] : 0u;
        const int cnt = hi + 1 < 64 ? (int)(hi + 1) : 64;
        int mine = 0;
        for (int l = 0; l < cnt; l++) {
            if (lane == l) mine = e;
            e = (int)(__shfl(pm, l) >> (3 * e)) & 7;
        }
        if (lane < cnt) cend[r.choff + idx] = (signed char)mine;
    }
}

// pass 5: s_{t-1} = B_t(s_t)
__global__ __launch_bounds__(256) void cnv_backtrace(const CnvSeqRow *__restrict__ rows, const ll *__restrict__ choff, int nseg, ll nchunks,
                                                      const unsigned short *__restrict__ bp, const signed char *__restrict__ cend,
                                                      signed char *__restrict__ state) {
    const ll c = (ll)blockIdx.x * 256 + threadIdx.x;
    if (c >= nchunks) return;
    ll t0;
    int len;
    cnv_chunk_of(rows, choff, nseg, c, t0, len);
    int s = cend[c];
    for (ll t = t0 + len - 1;; t--) {
        state[t] = (signed char)s;
        if (t == t0) break;
        const unsigned w = bp[t];
        if ((w >> s) & 1u) s = (int)(w >> 8);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
static bool cnv_misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

static int cnv_grid(const char *who, ll items, ll per_block, unsigned *out) {
    const ll g = (items + per_block - 1) / per_block;
    if (g > 0x7fffffffll) {
        tdt_set_error("%s: too many blocks", who);
        return TDT_E_RANGE;
    }
    *out = (unsigned)g;
    return TDT_OK;
}

struct CnvBinsWork {
    double *cov, *E;
    int8_t *gc;
    int *x;
    CnvBinRow *rows;
    ll *tstart;
    size_t lay(void *base, size_t n, size_t nseg, size_t total, bool host) {
        tdt_carver c(base);
        rows = c.take<CnvBinRow>(nseg);
        tstart = c.take<ll>(nseg);
        cov = c.take<double>(host ? n : 0);
        gc = c.take<int8_t>(host ? n : 0);
        E = c.take<double>(host ? nseg * CNV_CLASSES : 0);
        x = c.take<int>(host ? total : 0);
        return c.size;
    }
};

// the rows of a bins table against the n bins; -> the number of CNV bins
static int cnv_check_bin_rows(const char *who, int64_t n, const int64_t *table, int nseg, std::vector<ll> &tstart, ll *total) {
    ll at = 0;
    tstart.resize((size_t)nseg);
    for (int s = 0; s < nseg; s++) {
        const int64_t *r = table + 5 * s;
        if (r[0] < 0 || r[1] < 0 || r[0] > n || r[1] > n - r[0]) {
            tdt_set_error("%s: row %d (offset %lld, %lld bins) lies outside the %lld bins", who, s, (ll)r[0], (ll)r[1], (ll)n);
            return TDT_E_RANGE;
        }
        if (r[2] < 1 || r[2] > 64 || r[3] < 1 || r[3] > 6) {
            tdt_set_error("%s: row %d has K = %lld (1 .. 64) and P = %lld (1 .. 6)", who, s, (ll)r[2], (ll)r[3]);
            return TDT_E_RANGE;
        }
        if (r[4] != at) {
            tdt_set_error("%s: row %d writes from CNV bin %lld, the rows before it end at %lld", who, s, (ll)r[4], at);
            return TDT_E_RANGE;
        }
        tstart[(size_t)s] = at;
        at += (r[1] + r[2] - 1) / r[2];
    }
    *total = at;
    return TDT_OK;
}

static int cnv_bins_run(const char *who, tdt_ctx *ctx, const double *cov, const int8_t *gc, int64_t n, const int64_t *table, int nseg,
                        const double *E, int unit, int32_t *x, bool host) {
    if (!ctx || n < 0 || nseg < 0 || unit < 1 || unit > CNV_MAX_UNIT) {
        tdt_set_error("%s: bad argument", who);
        return TDT_E_ARG;
    }
    if (n == 0 || nseg == 0) return TDT_OK;
    if (!cov || !gc || !table || !E || !x || cnv_misaligned(cov, 8) || cnv_misaligned(table, 8) || cnv_misaligned(E, 8) || cnv_misaligned(x, 4)) {
        tdt_set_error("%s: a null or misaligned pointer", who);
        return TDT_E_ARG;
    }
    if (n >= 0x7fffffffll) {
        tdt_set_error("%s: %lld bins (2^31 - 1 or more)", who, (ll)n);
        return TDT_E_RANGE;
    }
    std::vector<ll> tstart;
    ll total = 0;
    int rc = cnv_check_bin_rows(who, n, table, nseg, tstart, &total);
    if (rc) return rc;
    if (total == 0) return TDT_OK;
    unsigned grid;
    if ((rc = cnv_grid(who, total, 256, &grid))) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    CnvBinsWork w;
    rc = tdt_scratch_layout(ctx, 29, w, (size_t)n, (size_t)nseg, (size_t)total, host);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    TDT_HIP(hipMemcpyAsync(w.rows, table, (size_t)nseg * sizeof(CnvBinRow), hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(w.tstart, tstart.data(), (size_t)nseg * sizeof(ll), hipMemcpyHostToDevice, st));
    if (host) {
        TDT_HIP(hipMemcpyAsync(w.cov, cov, (size_t)n * 8, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(w.gc, gc, (size_t)n, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(w.E, E, (size_t)nseg * CNV_CLASSES * 8, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(cnv_bins_kernel, dim3(grid), dim3(256), 0, st, host ? w.cov : cov, (const signed char *)(host ? w.gc : gc), w.rows, w.tstart,
                       nseg, host ? w.E : E, unit, total, host ? w.x : x);
    TDT_CHECK_LAUNCH();
    if (host) TDT_HIP(hipMemcpyAsync(x, w.x, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));                 // (tstart is read by the copy until here)
    return TDT_OK;
}

extern "C" int tdt_cnv_bins(tdt_ctx *ctx, const double *cov, const int8_t *gc, int64_t n, const int64_t *table, int nseg, const double *E,
                            int unit, int32_t *x) {
    return cnv_bins_run("tdt_cnv_bins", ctx, cov, gc, n, table, nseg, E, unit, x, true);
}

extern "C" int tdt_cnv_bins_device(tdt_ctx *ctx, const double *d_cov, const int8_t *d_gc, int64_t n, const int64_t *table, int nseg,
                                   const double *d_E, int unit, int32_t *d_x) {
    return cnv_bins_run("tdt_cnv_bins_device", ctx, d_cov, d_gc, n, table, nseg, d_E, unit, d_x, false);
}

struct CnvSeqWork {
    CnvSeqRow *rows;
    ll *choff, *A, *vin;
    unsigned short *bp;
    unsigned *emap;
    signed char *cend, *state;
    int *contig_end, *x;
    size_t lay(void *base, size_t n, size_t nseg, size_t nch, bool host) {
        tdt_carver c(base);
        rows = c.take<CnvSeqRow>(nseg);
        choff = c.take<ll>(nseg);
        contig_end = c.take<int>(nseg);
        A = c.take<ll>(nch * 64);
        vin = c.take<ll>(nch * 8);
        emap = c.take<unsigned>(nch);
        cend = c.take<signed char>(nch);
        bp = c.take<unsigned short>(n);
        x = c.take<int>(host ? n : 0);
        state = c.take<signed char>(host ? n : 0);
        return c.size;
    }
};

static int cnv_viterbi_run(const char *who, tdt_ctx *ctx, const int32_t *x, int64_t n, const int64_t *table, int nseg, int unit, int64_t cap,
                           int64_t lambda, int8_t *state, bool host) {
    if (!ctx || n < 0 || nseg < 0 || unit < 1 || unit > CNV_MAX_UNIT || cap < 0 || cap > CNV_MAX_PARAM || lambda < 0 || lambda > CNV_MAX_PARAM) {
        tdt_set_error("%s: bad argument", who);
        return TDT_E_ARG;
    }
    if (n == 0 || nseg == 0) return TDT_OK;
    if (!x || !table || !state || cnv_misaligned(x, 4) || cnv_misaligned(table, 8)) {
        tdt_set_error("%s: a null or misaligned pointer", who);
        return TDT_E_ARG;
    }
    if (n >= 0x7fffffffll) {
        tdt_set_error("%s: %lld bins (2^31 - 1 or more)", who, (ll)n);
        return TDT_E_RANGE;
    }
    std::vector<CnvSeqRow> rows((size_t)nseg);
    std::vector<ll> choff((size_t)nseg);
    ll at = 0, nch = 0;
    for (int s = 0; s < nseg; s++) {
        const int64_t *r = table + 3 * s;
        if (r[1] < 0 || r[1] > n - at || r[0] != at) {
            tdt_set_error("%s: row %d (from bin %lld, %lld bins) does not follow the rows before it (which end at %lld) inside the %lld bins", who,
                          s, (ll)r[0], (ll)r[1], at, (ll)n);
            return TDT_E_RANGE;
        }
        if (r[2] < 0 || r[2] >= CNV_STATES) {
            tdt_set_error("%s: row %d has P = %lld (0 .. 7)", who, s, (ll)r[2]);
            return TDT_E_RANGE;
        }
        rows[(size_t)s] = {at, r[1], r[2], nch};
        choff[(size_t)s] = nch;
        at += r[1];
        nch += (r[1] + CNV_CHUNK - 1) / CNV_CHUNK;
    }
    if (at != n) {
        tdt_set_error("%s: the rows hold %lld bins, the arrays %lld", who, at, (ll)n);
        return TDT_E_RANGE;
    }
    unsigned g1, g3, g5;
    int rc;
    if ((rc = cnv_grid(who, nch, 4, &g1)) || (rc = cnv_grid(who, nch, 32, &g3)) || (rc = cnv_grid(who, nch, 256, &g5))) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    CnvSeqWork w;
    rc = tdt_scratch_layout(ctx, 29, w, (size_t)n, (size_t)nseg, (size_t)nch, host);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    TDT_HIP(hipMemcpyAsync(w.rows, rows.data(), (size_t)nseg * sizeof(CnvSeqRow), hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(w.choff, choff.data(), (size_t)nseg * sizeof(ll), hipMemcpyHostToDevice, st));
    if (host) TDT_HIP(hipMemcpyAsync(w.x, x, (size_t)n * 4, hipMemcpyHostToDevice, st));
    const int *d_x = host ? w.x : x;
    signed char *d_state = (signed char *)(host ? (int8_t *)w.state : state);
    const ll U = unit, C = cap, L = lambda;
    hipLaunchKernelGGL(cnv_chunk_matrices, dim3(g1), dim3(256), 0, st, d_x, w.rows, w.choff, nseg, nch, U, C, L, w.A);
    hipLaunchKernelGGL(cnv_carry, dim3((unsigned)nseg), dim3(64), 0, st, w.rows, w.A, L, w.vin, w.contig_end);
    hipLaunchKernelGGL(cnv_backpointers, dim3(g3), dim3(256), 0, st, d_x, w.rows, w.choff, nseg, nch, U, C, L, w.vin, w.bp, w.emap);
    hipLaunchKernelGGL(cnv_chunk_ends, dim3((unsigned)nseg), dim3(64), 0, st, w.rows, w.emap, w.contig_end, w.cend);
    hipLaunchKernelGGL(cnv_backtrace, dim3(g5), dim3(256), 0, st, w.rows, w.choff, nseg, nch, w.bp, w.cend, d_state);
    TDT_CHECK_LAUNCH();
    if (host) TDT_HIP(hipMemcpyAsync(state, w.state, (size_t)n, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));                 // (rows / choff are read by the copies until here)
    return TDT_OK;
}

extern "C" int tdt_cnv_viterbi(tdt_ctx *ctx, const int32_t *x, int64_t n, const int64_t *table, int nseg, int unit, int64_t cap, int64_t lambda,
                               int8_t *state) {
    return cnv_viterbi_run("tdt_cnv_viterbi", ctx, x, n, table, nseg, unit, cap, lambda, state, true);
}

extern "C" int tdt_cnv_viterbi_device(tdt_ctx *ctx, const int32_t *d_x, int64_t n, const int64_t *table, int nseg, int unit, int64_t cap,
                                      int64_t lambda, int8_t *d_state) {
    return cnv_viterbi_run("tdt_cnv_viterbi_device", ctx, d_x, n, table, nseg, unit, cap, lambda, d_state, false);
}
