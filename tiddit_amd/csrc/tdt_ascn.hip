// Allele-specific copy number from the CNV bins and the allele counters of the --sv scan (TIDDIT_ASCN, tiddit_ascn.py), gfx950: the
// per-bin emissions of 16 states (ascn_emissions_kernel) and an exact Viterbi segmentation over any [n][16] emissions (five kernels,
// tdt_hmm16_viterbi), all contigs in one call each.
//
// The model (tiddit_ascn.py has the definition): 16 states (c, m) = total copies 0 .. 6 with 0 <= m <= c / 2 minor copies, c
// ascending, then m.  A bin's emission is the depth score of tdt_cnv.hip at c copies plus, for every informative site of the bin, the
// squared distance of the site's minor-allele fraction beta (in units of 1 / BU) from m / c — or, at a price HOM, from 0.
//
// The chain is tdt_cnv.hip's with 16 states: V_t(k) = e_t(k) + min(V_{t-1}(k), m + lambda), int64, cut into chunks of H16_CHUNK bins
// whose (min,+) matrices are stitched, which IS the sequential result.  The 8 x 8 lanes of one wavefront do not hold a 16 x 16 matrix,
// so here a ROW of a matrix — one chain — is a group of 16 lanes, four groups to a wavefront:
//   h16_chunk_matrices  one block of 256 per chunk: group i of the 16 walks the chunk from the unit vector of state i -> A[c][i][.]
//   h16_carry           one wavefront per contig: lane (r, j) holds A[r + 4q][j], q = 0 .. 3, of the chunk matrix; the 16-vector goes
//                       through the matrices in order (the next one is loaded while this one is applied); every chunk's incoming
//                       vector is kept, and the contig's end state.
//   h16_backpointers    one wavefront per 4 chunks, 16 lanes per chunk: the same walk from the chunk's true incoming vector.  A bin's
//                       back-pointers are 20 bits: the mask of the states that jump, and the lowest argmin a.  The walk also composes
//                       the chunk's end-state -> entry-state map (4 bits per state: 64 bits).
//   h16_chunk_ends      one wavefront per contig: the maps backwards, 64 at a load, to every chunk's end state.
//   h16_backtrace       one lane per chunk: from its end state back through its bins into state[].
#include "tdt_common.h"

#define H16_CHUNK 256              // bins per chunk of the Viterbi chain
#define H16_STATES 16
#define H16_BIG (1ll << 61)        // "no path": above every real cost (< 2^60), and H16_BIG + a real cost fits int64
#define H16_MAX_PARAM (1ll << 28)  // an emission and lambda at most; with fewer than 2^31 bins a path costs less than 2^60
#define ASCN_MAX_W 3200            // a bin's sites are unique positions: at most W of them
#define ASCN_MAX_UNIT (1 << 20)

typedef long long ll;
typedef unsigned long long ull;

struct AscnRow {
    ll site_lo, site_hi, toff, T, W;
};
struct H16Row {
    ll toff, T, home, choff;       // choff: the contig's first chunk
};

// the last s with start[s] <= g (start is non-decreasing, start[0] == 0 <= g): the row that owns item g — rows without items share
// their start with the row behind them and are never the last
__device__ static inline int h16_find(const ll *__restrict__ start, int n, ll g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ static inline ll h16_min(ll a, ll b) { return b < a ? b : a; }

// ---- emissions ----------------------------------------------------------------------------------------------------------------
// the first index in [lo, hi) whose position is >= v
__device__ static inline ll ascn_lower(const int *__restrict__ pos, ll lo, ll hi, ll v) {
    while (lo < hi) {
        const ll mid = (lo + hi) >> 1;
        if ((ll)pos[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// lane = (bin, state): 16 lanes per bin, 16 bins per block.  Every lane of a bin walks the bin's sites and derives beta from the
// table row itself (the 16 lanes read the same 32 bytes: one fetch, no exchange between lanes).
__global__ __launch_bounds__(256) void ascn_emissions_kernel(const unsigned *__restrict__ counts, const int *__restrict__ site_pos,
                                                              const unsigned char *__restrict__ cols, const int *__restrict__ x,
                                                              const AscnRow *__restrict__ rows, const ll *__restrict__ tstart, int nseg, ll total,
                                                              ll unit, ll cap, int bu, int acap, int hom, unsigned min_n, int *__restrict__ E,
                                                              int *__restrict__ nsite, int *__restrict__ sum_beta) {
    const ll g = (ll)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (g >= total) return;
    const int k = threadIdx.x & 15;
    // state k = (c, m): c ascending, then m
    const int c = k < 1 ? 0 : k < 2 ? 1 : k < 4 ? 2 : k < 6 ? 3 : k < 9 ? 4 : k < 12 ? 5 : 6;
    const int first = c == 0 ? 0 : c == 1 ? 1 : c == 2 ? 2 : c == 3 ? 4 : c == 4 ? 6 : c == 5 ? 9 : 12;
    const int m = k - first;
    const int mu = c ? (bu * m) / c : 0;
    const AscnRow r = rows[h16_find(tstart, nseg, g)];
    const ll t = g - r.toff;
    const ll s0 = ascn_lower(site_pos, r.site_lo, r.site_hi, t * r.W), s1 = ascn_lower(site_pos, s0, r.site_hi, (t + 1) * r.W);
    const int xt = x[g];
    const ll d = (ll)xt - unit * c;
    ll e = xt < 0 ? 0 : h16_min(cap, d * d);
    int n_inf = 0, sb = 0;
    for (ll s = s0; s < s1; s++) {
        const unsigned rn = counts[s * 8 + (cols[2 * s] & 7u)], an = counts[s * 8 + (cols[2 * s + 1] & 7u)];
        const ull n = (ull)rn + an;
        if (n < min_n) continue;
        const ull lo = rn < an ? rn : an;
        const int beta = (int)((lo * (ull)bu) / n);          // <= bu / 2
        const int h = beta * beta < acap ? beta * beta : acap;
        int gk = h;
        if (m) {
            const int dm = beta - mu;
            const int het = dm * dm < acap ? dm * dm : acap;
            const ll homo = (ll)h + hom;
            gk = het < homo ? het : (int)homo;
        }
        e += gk;
        n_inf++;
        sb += beta;
    }
    E[g * 16 + k] = (int)e;
    if (k == 0) {
        nsite[g] = n_inf;
        sum_beta[g] = sb;
    }
}

// ---- the walk shared by the chunk matrices and the back-pointers ------------------------------------------------------------
// Lanes are 4 groups of 16: lane (grp, j) holds V(j) of its group's chain, which runs over e[t0 .. t0 + len)[16] — t0 / len are the
// group's, maxlen is the wavefront's largest len.  Every lane runs every step (the cross-lane operations need them); a group past its
// len keeps its values.  RECORD: bp[t] = (mask of the states that jump) | a << 16, and map = the entry state the chain reaches from
// end state j.
template <bool RECORD>
__device__ static inline void h16_walk(const int *__restrict__ e, ll t0, int len, int maxlen, int lane, ll lambda, ll &V, unsigned *__restrict__ bp,
                                       int &map) {
    const int j = lane & 15, grp = lane & ~15;
    for (int b = 0; b < maxlen; b += 8) {
        int ev[8];
#pragma unroll
        for (int s = 0; s < 8; s++) ev[s] = b + s < len ? e[(t0 + b + s) * 16 + j] : 0;       // the group's next 8 bins, this lane's state
#pragma unroll
        for (int s = 0; s < 8; s++) {
            if (b + s >= maxlen) break;                                                        // (the whole wavefront)
            const bool act = b + s < len;
            ll m = V;
            m = h16_min(m, __shfl_xor(m, 1));
            m = h16_min(m, __shfl_xor(m, 2));
            m = h16_min(m, __shfl_xor(m, 4));
            m = h16_min(m, __shfl_xor(m, 8));
            const ll jump = m + lambda;
            const bool stay = V <= jump;
            if (RECORD) {
                const ull bj = __ballot(!stay), bm = __ballot(V == m);
                const unsigned jm = (unsigned)(bj >> grp) & 0xffffu;
                const int a = __ffs((unsigned)(bm >> grp) & 0xffffu) - 1;      // the lowest state attaining m (some lane of the group does)
                const int from = __shfl(map, grp | (a & 15));                  // (every lane: the lane of state a itself stays)
                if (act) {
                    map = stay ? map : from;
                    if (j == 0) bp[t0 + b + s] = jm | ((unsigned)a << 16);
                }
            }
            const ll nv = (ll)ev[s] + (stay ? V : jump);
            if (act) V = nv;
        }
    }
}

__device__ static inline void h16_chunk_of(const H16Row *__restrict__ rows, const ll *__restrict__ choff, int nseg, ll c, ll &t0, int &len) {
    const H16Row r = rows[h16_find(choff, nseg, c)];
    const ll first = (c - r.choff) * H16_CHUNK;
    t0 = r.toff + first;
    len = (int)(r.T - first < H16_CHUNK ? r.T - first : H16_CHUNK);
}

// pass 1: A[c][i * 16 + j]; block = chunk, thread = (i, j)
__global__ __launch_bounds__(256) void h16_chunk_matrices(const int *__restrict__ e, const H16Row *__restrict__ rows, const ll *__restrict__ choff,
                                                           int nseg, ll lambda, ll *__restrict__ A) {
    const ll c = blockIdx.x;
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 4, j = threadIdx.x & 15;
    ll t0;
    int len, map = 0;
    h16_chunk_of(rows, choff, nseg, c, t0, len);
    ll V = i == j ? 0 : H16_BIG;                      // the identity of (min,+)
    h16_walk<false>(e, t0, len, len, lane, lambda, V, nullptr, map);
    A[c * 256 + threadIdx.x] = V;
}

// pass 2: vin[c][16] = the vector entering chunk c; contig_end[s] = the lowest state attaining the minimal end cost
__global__ __launch_bounds__(64) void h16_carry(const H16Row *__restrict__ rows, const ll *__restrict__ A, ll lambda, ll *__restrict__ vin,
                                                 int *__restrict__ contig_end) {
    const H16Row r = rows[blockIdx.x];
    if (r.T == 0) return;
    const int lane = threadIdx.x, q0 = lane >> 4, j = lane & 15;
    const ll nch = (r.T + H16_CHUNK - 1) / H16_CHUNK;
    const ll *a = A + r.choff * 256;
    ll vj = j == r.home ? 0 : H16_BIG;                // every lane (., j) holds v(j)
    ll next[4];
#pragma unroll
    for (int q = 0; q < 4; q++) next[q] = a[(q0 + 4 * q) * 16 + j];
    for (ll c = 0; c < nch; c++) {
        ll cur[4];
#pragma unroll
        for (int q = 0; q < 4; q++) cur[q] = next[q];
        if (c + 1 < nch) {
#pragma unroll
            for (int q = 0; q < 4; q++) next[q] = a[(c + 1) * 256 + (q0 + 4 * q) * 16 + j];
        }
        if (lane < 16) vin[(r.choff + c) * 16 + lane] = vj;
        ll w = H16_BIG + H16_BIG;
#pragma unroll
        for (int q = 0; q < 4; q++) w = h16_min(w, __shfl(vj, q0 + 4 * q) + cur[q]);      // v(i) + A[i][j], i = q0 + 4q
        w = h16_min(w, __shfl_xor(w, 16));            // column minimum over i: every lane (., j) then holds the new v(j)
        w = h16_min(w, __shfl_xor(w, 32));
        vj = w;
    }
    const ll cost = vj + (j == r.home ? 0 : lambda);
    ll m = cost;
    m = h16_min(m, __shfl_xor(m, 1));
    m = h16_min(m, __shfl_xor(m, 2));
    m = h16_min(m, __shfl_xor(m, 4));
    m = h16_min(m, __shfl_xor(m, 8));
    const ull hit = __ballot(cost == m);
    if (lane == 0) contig_end[blockIdx.x] = __ffs((unsigned)hit & 0xffffu) - 1;
}

// pass 3: bp[t] of every bin, emap[c] = 4 bits per end state j: the state of the bin before the chunk
__global__ __launch_bounds__(256) void h16_backpointers(const int *__restrict__ e, const H16Row *__restrict__ rows, const ll *__restrict__ choff,
                                                         int nseg, ll nchunks, ll lambda, const ll *__restrict__ vin, unsigned *__restrict__ bp,
                                                         ull *__restrict__ emap) {
    const int lane = threadIdx.x & 63, k = lane & 15;
    const ll first = ((ll)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    if (first >= nchunks) return;                     // (the whole wavefront)
    const ll c = first + (lane >> 4);
    ll t0 = 0, V = 0;
    int len = 0, map = k;
    if (c < nchunks) {
        h16_chunk_of(rows, choff, nseg, c, t0, len);
        V = vin[c * 16 + k];
    }
    int maxlen = len;
    for (int d = 16; d < 64; d <<= 1) {
        const int o = __shfl_xor(maxlen, d);
        maxlen = o > maxlen ? o : maxlen;
    }
    h16_walk<true>(e, t0, len, maxlen, lane, lambda, V, bp, map);
    ull pm = (ull)map << (4 * k);
    pm |= __shfl_xor(pm, 1);
    pm |= __shfl_xor(pm, 2);
    pm |= __shfl_xor(pm, 4);
    pm |= __shfl_xor(pm, 8);
    if (c < nchunks && k == 0) emap[c] = pm;
}

// pass 4: cend[c] = the state of chunk c's last bin
__global__ __launch_bounds__(64) void h16_chunk_ends(const H16Row *__restrict__ rows, const ull *__restrict__ emap, const int *__restrict__ contig_end,
                                                      signed char *__restrict__ cend) {
    const H16Row r = rows[blockIdx.x];
    if (r.T == 0) return;
    const int lane = threadIdx.x;
    const ll nch = (r.T + H16_CHUNK - 1) / H16_CHUNK;
    int e = contig_end[blockIdx.x];                   // (the same in every lane, here and below)
    for (ll hi = nch - 1; hi >= 0; hi -= 64) {
        const ll idx = hi - lane;
        const ull pm = idx >= 0 ? emap[r.choff + idx] : 0ull;
        const int cnt = hi + 1 < 64 ? (int)(hi + 1) : 64;
        int mine = 0;
        for (int l = 0; l < cnt; l++) {
            if (lane == l) mine = e;
            e = (int)(__shfl(pm, l) >> (4 * e)) & 15;
        }
        if (lane < cnt) cend[r.choff + idx] = (signed char)mine;
    }
}

// pass 5: s_{t-1} = B_t(s_t)
__global__ __launch_bounds__(256) void h16_backtrace(const H16Row *__restrict__ rows, const ll *__restrict__ choff, int nseg, ll nchunks,
                                                      const unsigned *__restrict__ bp, const signed char *__restrict__ cend,
                                                      signed char *__restrict__ state) {
    const ll c = (ll)blockIdx.x * 256 + threadIdx.x;
    if (c >= nchunks) return;
    ll t0;
    int len;
    h16_chunk_of(rows, choff, nseg, c, t0, len);
    int s = cend[c];
    for (ll t = t0 + len - 1;; t--) {
        state[t] = (signed char)s;
        if (t == t0) break;
        const unsigned w = bp[t];
        if ((w >> s) & 1u) s = (int)(w >> 16) & 15;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
static bool ascn_misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

static int ascn_grid(const char *who, ll items, ll per_block, unsigned *out) {
    const ll g = (items + per_block - 1) / per_block;
    if (g > 0x7fffffffll) {
        tdt_set_error("%s: too many blocks", who);
        return TDT_E_RANGE;
    }
    *out = (unsigned)g;
    return TDT_OK;
}

// (the scratch slot is tdt_cnv.hip's: neither file keeps anything in it between calls)
#define ASCN_SLOT 29

struct AscnWork {
    AscnRow *rows;
    ll *tstart;
    unsigned *counts;
    int *site_pos, *x, *E, *nsite, *sum_beta;
    unsigned char *cols;
    size_t lay(void *base, size_t nsites, size_t total, size_t nseg, bool host) {
        tdt_carver c(base);
        rows = c.take<AscnRow>(nseg);
        tstart = c.take<ll>(nseg);
        counts = c.take<unsigned>(host ? nsites * 8 : 0);
        site_pos = c.take<int>(host ? nsites : 0);
        cols = c.take<unsigned char>(host ? nsites * 2 : 0);
        x = c.take<int>(host ? total : 0);
        E = c.take<int>(host ? total * 16 : 0);
        nsite = c.take<int>(host ? total : 0);
        sum_beta = c.take<int>(host ? total : 0);
        return c.size;
    }
};

static int ascn_emissions_run(const char *who, tdt_ctx *ctx, const uint32_t *counts, const int32_t *site_pos, const uint8_t *cols, int64_t nsites,
                              const int32_t *x, int64_t total, const int64_t *table, int nseg, int unit, int64_t cap, int bu, int acap, int hom,
                              int min_n, int32_t *E, int32_t *nsite, int32_t *sum_beta, bool host) {
    if (!ctx || nsites < 0 || total < 0 || nseg < 0 || unit < 1 || unit > ASCN_MAX_UNIT || cap < 0 || cap > H16_MAX_PARAM || bu < 1 || bu > (1 << 15) ||
        acap < 0 || acap > (1 << 16) || hom < 0 || hom > (int)H16_MAX_PARAM || min_n < 1) {
        tdt_set_error("%s: bad argument", who);
        return TDT_E_ARG;
    }
    if (total == 0 || nseg == 0) return TDT_OK;
    if (!x || !table || !E || !nsite || !sum_beta || (nsites && (!counts || !site_pos || !cols)) || ascn_misaligned(counts, 4) ||
        ascn_misaligned(site_pos, 4) || ascn_misaligned(x, 4) || ascn_misaligned(table, 8) || ascn_misaligned(E, 4) || ascn_misaligned(nsite, 4) ||
        ascn_misaligned(sum_beta, 4)) {
        tdt_set_error("%s: a null or misaligned pointer", who);
        return TDT_E_ARG;
    }
    if (total >= 0x7fffffffll || nsites >= 0x7fffffffll) {
        tdt_set_error("%s: %lld bins or %lld sites (2^31 - 1 or more)", who, (ll)total, (ll)nsites);
        return TDT_E_RANGE;
    }
    std::vector<ll> tstart((size_t)nseg);
    ll at = 0;
    for (int s = 0; s < nseg; s++) {
        const int64_t *r = table + 5 * s;
        if (r[0] < 0 || r[1] < r[0] || r[1] > nsites) {
            tdt_set_error("%s: row %d (sites %lld .. %lld) lies outside the %lld sites", who, s, (ll)r[0], (ll)r[1], (ll)nsites);
            return TDT_E_RANGE;
        }
        if (r[3] < 0 || r[3] > total - at || r[2] != at) {
            tdt_set_error("%s: row %d (from bin %lld, %lld bins) does not follow the rows before it (which end at %lld) inside the %lld bins", who, s,
                          (ll)r[2], (ll)r[3], at, (ll)total);
            return TDT_E_RANGE;
        }
        if (r[4] < 1 || r[4] > ASCN_MAX_W) {
            tdt_set_error("%s: row %d has W = %lld (1 .. %d)", who, s, (ll)r[4], ASCN_MAX_W);
            return TDT_E_RANGE;
        }
        tstart[(size_t)s] = at;
        at += r[3];
    }
    if (at != total) {
        tdt_set_error("%s: the rows hold %lld bins, the arrays %lld", who, at, (ll)total);
        return TDT_E_RANGE;
    }
    if (host) {
        for (int64_t s = 0; s < 2 * nsites; s++) {
            if (cols[s] > 7) {
                tdt_set_error("%s: site %lld names counter column %d (0 .. 7)", who, (ll)(s / 2), (int)cols[s]);
                return TDT_E_RANGE;
            }
        }
    }
    unsigned grid;
    int rc;
    if ((rc = ascn_grid(who, total, 16, &grid))) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    AscnWork w;
    rc = tdt_scratch_layout(ctx, ASCN_SLOT, w, (size_t)nsites, (size_t)total, (size_t)nseg, host);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    TDT_HIP(hipMemcpyAsync(w.rows, table, (size_t)nseg * sizeof(AscnRow), hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(w.tstart, tstart.data(), (size_t)nseg * sizeof(ll), hipMemcpyHostToDevice, st));
    if (host) {
        if (nsites) {
            TDT_HIP(hipMemcpyAsync(w.counts, counts, (size_t)nsites * 32, hipMemcpyHostToDevice, st));
            TDT_HIP(hipMemcpyAsync(w.site_pos, site_pos, (size_t)nsites * 4, hipMemcpyHostToDevice, st));
            TDT_HIP(hipMemcpyAsync(w.cols, cols, (size_t)nsites * 2, hipMemcpyHostToDevice, st));
        }
        TDT_HIP(hipMemcpyAsync(w.x, x, (size_t)total * 4, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(ascn_emissions_kernel, dim3(grid), dim3(256), 0, st, host ? w.counts : counts, host ? w.site_pos : site_pos,
                       host ? w.cols : cols, host ? w.x : x, w.rows, w.tstart, nseg, (ll)total, (ll)unit, (ll)cap, bu, acap, hom, (unsigned)min_n,
                       host ? w.E : E, host ? w.nsite : nsite, host ? w.sum_beta : sum_beta);
    TDT_CHECK_LAUNCH();
    if (host) {
        TDT_HIP(hipMemcpyAsync(E, w.E, (size_t)total * 64, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipMemcpyAsync(nsite, w.nsite, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipMemcpyAsync(sum_beta, w.sum_beta, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    }
    TDT_HIP(hipStreamSynchronize(st));                 // (tstart is read by the copy until here)
    return TDT_OK;
}

extern "C" int tdt_ascn_emissions(tdt_ctx *ctx, const uint32_t *counts, const int32_t *site_pos, const uint8_t *cols, int64_t nsites,
                                  const int32_t *x, int64_t total, const int64_t *table, int nseg, int unit, int64_t cap, int bu, int acap, int hom,
                                  int min_n, int32_t *E, int32_t *nsite, int32_t *sum_beta) {
    return ascn_emissions_run("tdt_ascn_emissions", ctx, counts, site_pos, cols, nsites, x, total, table, nseg, unit, cap, bu, acap, hom, min_n, E, nsite,
                              sum_beta, true);
}

extern "C" int tdt_ascn_emissions_device(tdt_ctx *ctx, const uint32_t *d_counts, const int32_t *d_site_pos, const uint8_t *d_cols, int64_t nsites,
                                         const int32_t *d_x, int64_t total, const int64_t *table, int nseg, int unit, int64_t cap, int bu, int acap,
                                         int hom, int min_n, int32_t *d_E, int32_t *d_nsite, int32_t *d_sum_beta) {
    return ascn_emissions_run("tdt_ascn_emissions_device", ctx, d_counts, d_site_pos, d_cols, nsites, d_x, total, table, nseg, unit, cap, bu, acap, hom,
                              min_n, d_E, d_nsite, d_sum_beta, false);
}

struct H16Work {
    H16Row *rows;
    ll *choff, *A, *vin;
    ull *emap;
    unsigned *bp;
    signed char *cend, *state;
    int *contig_end, *e;
    size_t lay(void *base, size_t n, size_t nseg, size_t nch, bool host) {
        tdt_carver c(base);
        rows = c.take<H16Row>(nseg);
        choff = c.take<ll>(nseg);
        contig_end = c.take<int>(nseg);
        A = c.take<ll>(nch * 256);
        vin = c.take<ll>(nch * 16);
        emap = c.take<ull>(nch);
        cend = c.take<signed char>(nch);
        bp = c.take<unsigned>(n);
        e = c.take<int>(host ? n * 16 : 0);
        state = c.take<signed char>(host ? n : 0);
        return c.size;
    }
};

static int h16_viterbi_run(const char *who, tdt_ctx *ctx, const int32_t *e, int64_t n, const int64_t *table, int nseg, int64_t lambda, int8_t *state,
                           bool host) {
    if (!ctx || n < 0 || nseg < 0 || lambda < 0 || lambda > H16_MAX_PARAM) {
        tdt_set_error("%s: bad argument", who);
        return TDT_E_ARG;
    }
    if (n == 0 || nseg == 0) return TDT_OK;
    if (!e || !table || !state || ascn_misaligned(e, 4) || ascn_misaligned(table, 8)) {
        tdt_set_error("%s: a null or misaligned pointer", who);
        return TDT_E_ARG;
    }
    if (n >= 0x7fffffffll) {
        tdt_set_error("%s: %lld bins (2^31 - 1 or more)", who, (ll)n);
        return TDT_E_RANGE;
    }
    std::vector<H16Row> rows((size_t)nseg);
    std::vector<ll> choff((size_t)nseg);
    ll at = 0, nch = 0;
    for (int s = 0; s < nseg; s++) {
        const int64_t *r = table + 3 * s;
        if (r[1] < 0 || r[1] > n - at || r[0] != at) {
            tdt_set_error("%s: row %d (from bin %lld, %lld bins) does not follow the rows before it (which end at %lld) inside the %lld bins", who,
                          s, (ll)r[0], (ll)r[1], at, (ll)n);
            return TDT_E_RANGE;
        }
        if (r[2] < 0 || r[2] >= H16_STATES) {
            tdt_set_error("%s: row %d has home state %lld (0 .. 15)", who, s, (ll)r[2]);
            return TDT_E_RANGE;
        }
        rows[(size_t)s] = {at, r[1], r[2], nch};
        choff[(size_t)s] = nch;
        at += r[1];
        nch += (r[1] + H16_CHUNK - 1) / H16_CHUNK;
    }
    if (at != n) {
        tdt_set_error("%s: the rows hold %lld bins, the arrays %lld", who, at, (ll)n);
        return TDT_E_RANGE;
    }
    if (host) {
        for (int64_t k = 0; k < n * 16; k++) {
            if (e[k] < 0 || e[k] > H16_MAX_PARAM) {
                tdt_set_error("%s: emission %d of bin %lld, state %d lies outside 0 .. 2^28", who, (int)e[k], (ll)(k / 16), (int)(k % 16));
                return TDT_E_RANGE;
            }
        }
    }
    unsigned g3, g5;
    int rc;
    if ((rc = ascn_grid(who, nch, 16, &g3)) || (rc = ascn_grid(who, nch, 256, &g5))) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    H16Work w;
    rc = tdt_scratch_layout(ctx, ASCN_SLOT, w, (size_t)n, (size_t)nseg, (size_t)nch, host);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    TDT_HIP(hipMemcpyAsync(w.rows, rows.data(), (size_t)nseg * sizeof(H16Row), hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(w.choff, choff.data(), (size_t)nseg * sizeof(ll), hipMemcpyHostToDevice, st));
    if (host) TDT_HIP(hipMemcpyAsync(w.e, e, (size_t)n * 64, hipMemcpyHostToDevice, st));
    const int *d_e = host ? w.e : e;
    signed char *d_state = (signed char *)(host ? (int8_t *)w.state : state);
    const ll L = lambda;
    hipLaunchKernelGGL(h16_chunk_matrices, dim3((unsigned)nch), dim3(256), 0, st, d_e, w.rows, w.choff, nseg, L, w.A);
    hipLaunchKernelGGL(h16_carry, dim3((unsigned)nseg), dim3(64), 0, st, w.rows, w.A, L, w.vin, w.contig_end);
    hipLaunchKernelGGL(h16_backpointers, dim3(g3), dim3(256), 0, st, d_e, w.rows, w.choff, nseg, nch, L, w.vin, w.bp, w.emap);
    hipLaunchKernelGGL(h16_chunk_ends, dim3((unsigned)nseg), dim3(64), 0, st, w.rows, w.emap, w.contig_end, w.cend);
    hipLaunchKernelGGL(h16_backtrace, dim3(g5), dim3(256), 0, st, w.rows, w.choff, nseg, nch, w.bp, w.cend, d_state);
    TDT_CHECK_LAUNCH();
    if (host) TDT_HIP(hipMemcpyAsync(state, w.state, (size_t)n, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));                 // (rows / choff are read by the copies until here)
    return TDT_OK;
}

extern "C" int tdt_hmm16_viterbi(tdt_ctx *ctx, const int32_t *e, int64_t n, const int64_t *table, int nseg, int64_t lambda, int8_t *state) {
    return h16_viterbi_run("tdt_hmm16_viterbi", ctx, e, n, table, nseg, lambda, state, true);
}

extern "C" int tdt_hmm16_viterbi_device(tdt_ctx *ctx, const int32_t *d_e, int64_t n, const int64_t *table, int nseg, int64_t lambda, int8_t *d_state) {
    return h16_viterbi_run("tdt_hmm16_viterbi_device", ctx, d_e, n, table, nseg, lambda, d_state, false);
}
