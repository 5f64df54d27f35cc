// Gapped local alignment of short queries to a family library for gfx950 (TIDDIT_CLIPS_MEI) — the first dynamic-programming kernel
// of the tree.  The definition is tiddit_clip_mei.py's (rules 2 to 4).  Integers throughout: device equals definition exactly.
//   * sw_align_wave — one wavefront per (query, strand, family) problem, SW_BLOCK / 64 independent problems per workgroup, no LDS and
//     no barrier.  The anti-diagonal systolic wave: lane l owns the C query columns C l ... C l + C - 1, C = ceil(qlen / 64) (1 ... 5,
//     a template parameter, so a 60-base query fills 60 lanes and a 272-base one 55), and holds their H and E keys of the row above in
//     registers.  At step t lane l works on family base t - l.  The H and the F key of the column in front of the lane's first (F runs
//     along the query) come from lane l - 1 by one cross-lane shift each per step; the H key received a step earlier is the diagonal.
//     Family codes are taken SW_FAM_BLOCK = 64 at a time from the packed store, one per lane, the block in front kept beside them (both
//     nibbles in one register), and every lane picks its base t - l out of them by one cross-lane read.  A lane reads the family's own
//     bytes only: rows at or beyond the family's length are never loaded, so the guard nibbles and the neighbours never take part.
//     A key is score << 32 | (2^32 - 1 - (fstart << 9 | qstart)), 0 = EMPTY; a penalty that would leave a score <= 0 gives EMPTY.  The
//     lane-local best (key, end cell) is taken with a strict >, which keeps the smallest (fend, qend) because a lane visits its cells in
//     that order, and is reduced once at the end: the wave maximum of the key, then the wave minimum of the end cell among its holders.
//   * sw_count + ks_carry_sum / sw_build — the query table of the handle path: a CLOSED pair gives its SEQ, an OPEN pair its R site's consensus and
//     its L site's reversed, all in reference direction, from the rows where tdt_clip_ins left them.
//   * sw_reduce — lane = query: the best problem by (score, family, strand), the best score among the other families, the spans
//     1-based (a strand - span converted back to the query as written), and the counters, the pair rule's among them.
#include "tdt_swalign.h"
#include "tdt_keyscan.h"

typedef unsigned long long ull;

#define SW_MATCH TDT_SW_MATCH                 // the four scores are bwa-mem's
#define SW_MISMATCH TDT_SW_MISMATCH
#define SW_GAP_OPEN TDT_SW_GAP_OPEN
#define SW_GAP_EXTEND TDT_SW_GAP_EXTEND
#define SW_OTHER TDT_SW_OTHER                 // a library base that is not A C G T, against anything
#define SW_BLOCK 256                          // sw_align_wave: four wavefronts, one problem each
#define SW_FAM_BLOCK 64                       // family codes taken at a time: one per lane
#define SW_MAX_COLS 5                         // query columns of a lane at most
#define SW_POS_BITS 9                         // a query position inside a key's low word

static_assert(SW_MATCH == 1, "a match adds one score unit");
static_assert(64 * SW_MAX_COLS >= TDT_SW_QMAX && TDT_SW_QMAX < (1 << SW_POS_BITS), "every column has a lane and a query position fits its bits");
static_assert(TDT_SW_LIB_MAX_BASES <= (1 << 20), "fstart << 9 | qstart fits 29 bits");
static_assert(TDT_SW_SEQ_WORDS * TDT_CLIP_COLS >= TDT_SW_QMAX && TDT_SW_SEQ_WORDS == INS_SEQ_WORDS, "a query fits its words");
static_assert(SW_FAM_BLOCK == 64, "one family code per lane");

struct sw_min { template <class T> __device__ static T of(T a, T b) { return b < a ? b : a; } };

// a key less `pen` score units; EMPTY where the score would be <= 0
__device__ __forceinline__ ull sw_less(ull k, unsigned pen) { return k >= ((ull)(pen + 1u) << 32) ? k - ((ull)pen << 32) : 0ull; }
__device__ __forceinline__ ull sw_max(ull a, ull b) { return b > a ? b : a; }
// base j of a query in words of 56 bits
__device__ __forceinline__ unsigned sw_code56(const ull *__restrict__ w, unsigned j) { return (unsigned)(w[j / TDT_CLIP_COLS] >> (2u * (j % TDT_CLIP_COLS))) & 3u; }

// one problem by one wavefront: the n bases of the query w10 (minus: its reverse complement) against the m bases of the family whose
// packed codes start at fam.  Every lane returns the problem's best key and end cell (fend << 9 | qend, 0-based; key 0: no positive cell).
template <int C>
__device__ __forceinline__ void sw_wave(const ull *__restrict__ w10, int n, bool minus, const uint8_t *__restrict__ fam, int m, int lane, ull *key_out,
                                        unsigned *end_out) {
    unsigned q[C];                                                 // the columns' bases as BAM's one-hot codes; 0: no column
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int j = C * lane + c;
        q[c] = 0u;
        if (j < n) {
            const unsigned code = sw_code56(w10, (unsigned)(minus ? n - 1 - j : j));
            q[c] = 1u << (minus ? 3u - code : code);
        }
    }
    ull H[C], E[C];                                                // the row above: H[i - 1][j] and E[i - 1][j]
#pragma unroll
    for (int c = 0; c < C; c++) H[c] = E[c] = 0ull;
    ull hout = 0ull, fout = 0ull, hdiag = 0ull;                    // H and F of the lane's last column in its row; the H received a step ago
    ull bestk = 0ull;
    unsigned bestpos = 0xffffffffu;
    unsigned codes = 0u;                                           // bits 3:0 the lane's code of this block, bits 7:4 of the block in front
    const int steps = m + (n + C - 1) / C - 1;                     // (the lanes behind the last column have nothing to add)
    for (int t = 0; t < steps; t++) {                              // (uniform over the wave)
        if ((t & (SW_FAM_BLOCK - 1)) == 0) {
            const int r = t + lane;
            codes = (codes << 4) & 0xf0u;
            if (r < m) codes |= (fam[r >> 1] >> ((r & 1) ? 0 : 4)) & 0xfu;
        }
        ull hin = __shfl_up(hout, 1), fin = __shfl_up(fout, 1);
        if (lane == 0) hin = fin = 0ull;
        const int i = t - lane;                                    // the lane's family base
        const unsigned both = (unsigned)__shfl((int)codes, i & (SW_FAM_BLOCK - 1));
        if (i >= 0 && i < m) {
            const unsigned fc = (i >= (t & ~(SW_FAM_BLOCK - 1)) ? both : both >> 4) & 0xfu;
            const unsigned pen = (fc & (fc - 1u)) == 0u ? (unsigned)SW_MISMATCH : (unsigned)SW_OTHER;      // (fc is 1 ... 15)
            ull diag = hdiag, hl = hin, fl = fin;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const int j = C * lane + c;
                const ull e = sw_max(sw_less(H[c], SW_GAP_OPEN + SW_GAP_EXTEND), sw_less(E[c], SW_GAP_EXTEND));
                const ull f = sw_max(sw_less(hl, SW_GAP_OPEN + SW_GAP_EXTEND), sw_less(fl, SW_GAP_EXTEND));
                const ull d0 = diag ? diag : (ull)(0xffffffffu - (((unsigned)i << SW_POS_BITS) | (unsigned)j));
                const ull d = fc == q[c] ? d0 + (1ull << 32) : sw_less(d0, pen);
                const ull h = sw_max(d, sw_max(e, f));
                diag = H[c], H[c] = h, E[c] = e, hl = h, fl = f;
                if (j < n && h > bestk) bestk = h, bestpos = ((unsigned)i << SW_POS_BITS) | (unsigned)j;
            }
            hout = hl, fout = fl, hdiag = hin;
        }
    }
    const ull k = tdt_wave_reduce<tdt_max>(bestk);
    *key_out = k;
    *end_out = tdt_wave_reduce<sw_min>(bestk == k ? bestpos : 0xffffffffu);
}

__global__ __launch_bounds__(SW_BLOCK) void sw_align_wave(sw_queries Q, int nq, tdt_refview L, ull *__restrict__ pkey, unsigned *__restrict__ pend) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * (SW_BLOCK / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (p >= 2ll * nq * L.n) return;                               // (uniform over the wave; no barrier below)
    const int f = (int)(p % L.n), qs = (int)(p / L.n), qi = qs >> 1;
    int n = __builtin_amdgcn_readfirstlane((int)Q.qlen[qi]), m = __builtin_amdgcn_readfirstlane(L.len[f]);
    n = n < 0 ? 0 : n > TDT_SW_QMAX ? TDT_SW_QMAX : n;
    m = m < 0 ? 0 : m;
    const ull *w10 = Q.seq10 + (size_t)qi * TDT_SW_SEQ_WORDS;
    const uint8_t *fam = L.store + L.off[f];
    const bool minus = qs & 1;
    ull key = 0ull;
    unsigned end = 0xffffffffu;
    switch ((n + 63) / 64) {                                       // (uniform)
    case 0: break;
    case 1: sw_wave<1>(w10, n, minus, fam, m, lane, &key, &end); break;
    case 2: sw_wave<2>(w10, n, minus, fam, m, lane, &key, &end); break;
    case 3: sw_wave<3>(w10, n, minus, fam, m, lane, &key, &end); break;
    case 4: sw_wave<4>(w10, n, minus, fam, m, lane, &key, &end); break;
    default: sw_wave<SW_MAX_COLS>(w10, n, minus, fam, m, lane, &key, &end); break;
    }
    if (lane == 0) pkey[p] = key, pend[p] = end;
}

// ---- the query table of the pair rows
// off[p] = the queries of pair p (a CLOSED pair has one, an OPEN pair two) and off[n_pairs] = 0: ks_carry_sum over the n_pairs + 1 entries
// turns them into every pair's first query and, in the last entry, the count
__global__ __launch_bounds__(KS_BLOCK) void sw_count(int n_pairs, const unsigned *__restrict__ status, int *__restrict__ off) {
    const int p = blockIdx.x * KS_BLOCK + threadIdx.x;
    if (p <= n_pairs) off[p] = p == n_pairs ? 0 : status[p] ? 1 : 2;
}

__device__ __forceinline__ unsigned sw_cols(unsigned eclen) { return eclen < (unsigned)TDT_CLIP_EXT_COLS ? eclen : (unsigned)TDT_CLIP_EXT_COLS; }

// lane = pair
__global__ __launch_bounds__(KS_BLOCK) void sw_build(ins_sites S, int n_pairs, ins_out P, const int *__restrict__ off, sw_table T) {
    const int p = blockIdx.x * KS_BLOCK + threadIdx.x;
    if (p >= n_pairs) return;
    const size_t at = (size_t)off[p];
    if (P.status[p]) {
        const unsigned len = P.len[p] < (unsigned)TDT_SW_QMAX ? P.len[p] : (unsigned)TDT_SW_QMAX;
        for (int w = 0; w < TDT_SW_SEQ_WORDS; w++) T.seq10[at * TDT_SW_SEQ_WORDS + w] = P.seq10[(size_t)p * INS_SEQ_WORDS + w];
        T.qlen[at] = len, T.pair[at] = (unsigned)p, T.part[at] = SW_PART_SEQ;
        return;
    }
    const unsigned r = P.r_row[p], l = P.l_row[p], a = sw_cols(S.eclen[r]), b = sw_cols(S.eclen[l]);
    const ull *x = S.cons5 + (size_t)r * TDT_CLIP_EXT_WORDS, *y = S.cons5 + (size_t)l * TDT_CLIP_EXT_WORDS;
    const ull mask56 = (1ull << 56) - 1ull;
    for (int w = 0; w < TDT_SW_SEQ_WORDS; w++) {
        ull vx = 0ull, vy = 0ull;
        if (w < TDT_CLIP_EXT_WORDS) {
            const int left = (int)a - TDT_CLIP_COLS * w;           // (the words hold nothing behind ECLEN, but an entry's caller may)
            vx = left >= TDT_CLIP_COLS ? x[w] & mask56 : left > 0 ? x[w] & ((1ull << (2 * left)) - 1ull) : 0ull;
            for (int j = 0; j < TDT_CLIP_COLS; j++) {
                const unsigned i = (unsigned)(TDT_CLIP_COLS * w + j);
                if (i < b) vy |= (ull)sw_code56(y, b - 1u - i) << (2 * j);
            }
        }
        T.seq10[at * TDT_SW_SEQ_WORDS + w] = vx, T.seq10[(at + 1) * TDT_SW_SEQ_WORDS + w] = vy;
    }
    T.qlen[at] = a, T.pair[at] = (unsigned)p, T.part[at] = SW_PART_LEFT;
    T.qlen[at + 1] = b, T.pair[at + 1] = (unsigned)p, T.part[at + 1] = SW_PART_RIGHT;
}

// ---- a query's result
struct sw_res {
    unsigned family, strand, score, qstart, qend, fstart, fend, second, second_family;
};

__device__ sw_res sw_best_of_query(const ull *__restrict__ pkey, const unsigned *__restrict__ pend, int qi, int nf, int n) {
    sw_res R{0xffffffffu, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0xffffffffu};
    ull key = 0ull;
    unsigned end = 0u;
    for (int f = 0; f < nf; f++)                                   // (score, then the smaller family, then strand + : a strict >)
        for (int s = 0; s < 2; s++) {
            const size_t p = ((size_t)qi * 2 + (size_t)s) * (size_t)nf + (size_t)f;
            const ull k = pkey[p];
            if ((unsigned)(k >> 32) > R.score) R.score = (unsigned)(k >> 32), R.family = (unsigned)f, R.strand = (unsigned)s, key = k, end = pend[p];
        }
    if (!R.score) return R;
    const unsigned start = 0xffffffffu - (unsigned)(key & 0xffffffffull);
    const unsigned qs = start & ((1u << SW_POS_BITS) - 1u), qe = end & ((1u << SW_POS_BITS) - 1u);
    R.fstart = (start >> SW_POS_BITS) + 1u, R.fend = (end >> SW_POS_BITS) + 1u;
    R.qstart = R.strand ? (unsigned)n - qe : qs + 1u, R.qend = R.strand ? (unsigned)n - qs : qe + 1u;
    for (int f = 0; f < nf; f++) {
        if ((unsigned)f == R.family) continue;
        for (int s = 0; s < 2; s++) {
            const unsigned sc = (unsigned)(pkey[((size_t)qi * 2 + (size_t)s) * (size_t)nf + (size_t)f] >> 32);
            if (sc > R.second) R.second = sc, R.second_family = (unsigned)f;
        }
    }
    return R;
}

__device__ __forceinline__ int sw_len(const sw_queries &Q, int qi) {
    const unsigned n = Q.qlen[qi];
    return n > (unsigned)TDT_SW_QMAX ? TDT_SW_QMAX : (int)n;
}

// lane = query
__global__ __launch_bounds__(KS_BLOCK) void sw_reduce(sw_queries Q, int nq, int nf, const ull *__restrict__ pkey, const unsigned *__restrict__ pend, unsigned A,
                                                      sw_out Out, ull *__restrict__ sn) {
    const int qi = blockIdx.x * KS_BLOCK + threadIdx.x;
    if (qi >= nq) return;
    const sw_res R = sw_best_of_query(pkey, pend, qi, nf, sw_len(Q, qi));
    if (Out.family) {
        Out.family[qi] = R.family, Out.strand[qi] = R.strand, Out.score[qi] = R.score, Out.qstart[qi] = R.qstart, Out.qend[qi] = R.qend;
        Out.fstart[qi] = R.fstart, Out.fend[qi] = R.fend, Out.second[qi] = R.second, Out.second_family[qi] = R.second_family;
    }
    const unsigned part = Q.part ? Q.part[qi] : (unsigned)SW_PART_SEQ;
    const bool named = R.score >= A;
    atomicAdd(&sn[SW_QUERIES], 1ull);
    atomicAdd(&sn[part == SW_PART_SEQ ? SW_CLOSED_Q : part == SW_PART_LEFT ? SW_LEFT_Q : SW_RIGHT_Q], 1ull);
    atomicAdd(&sn[named ? SW_NAMED : SW_UNNAMED], 1ull);
    if (named && R.strand) atomicAdd(&sn[SW_REVERSE], 1ull);
    if (named && R.second == R.score) atomicAdd(&sn[SW_AMBIGUOUS], 1ull);
    if (part == SW_PART_SEQ) {
        if (named) atomicAdd(&sn[SW_PAIRS_NAMED], 1ull);
    } else if (part == SW_PART_LEFT) {                             // (the pair's RIGHT query is the next one: the pair rule is the LEFT lane's)
        bool other = false, agree = true;
        if (qi + 1 < nq && Q.part[qi + 1] == SW_PART_RIGHT) {
            const sw_res R2 = sw_best_of_query(pkey, pend, qi + 1, nf, sw_len(Q, qi + 1));
            other = R2.score >= A, agree = R2.family == R.family && R2.strand == R.strand;
        }
        if (named && other && !agree) atomicAdd(&sn[SW_PAIRS_CONFLICT], 1ull);
        else if (named || other) atomicAdd(&sn[SW_PAIRS_NAMED], 1ull);
    }
}

// ---- the launches
int sw_check(const char *fn, tdt_ctx *ctx, const tdt_refseq *lib, size_t n, int A) {
    if (!ctx || !lib || lib->ctx->device != ctx->device) {
        tdt_set_error("%s: bad argument", fn);
        return TDT_E_ARG;
    }
    if (A < TDT_SW_MIN_SCORE_LO || A > TDT_SW_QMAX) {
        tdt_set_error("%s: minimum score %d (%d ... %d)", fn, A, TDT_SW_MIN_SCORE_LO, TDT_SW_QMAX);
        return TDT_E_RANGE;
    }
    if (lib->n_contigs < 1 || lib->n_contigs > TDT_SW_LIB_MAX_SEQS) {
        tdt_set_error("%s: the library has %d sequences (1 ... %d)", fn, lib->n_contigs, TDT_SW_LIB_MAX_SEQS);
        return TDT_E_RANGE;
    }
    long long total = 0;
    for (int c = 0; c < lib->n_contigs; c++)
        if (lib->len[c] < 1 || lib->len[c] > TDT_SW_LIB_MAX_BASES || (total += lib->len[c]) > TDT_SW_LIB_MAX_BASES) {
            tdt_set_error("%s: library sequence %d has %lld bases (1 ... %d each, %d in all)", fn, c, lib->len[c], TDT_SW_LIB_MAX_BASES, TDT_SW_LIB_MAX_BASES);
            return TDT_E_RANGE;
        }
    for (int c = 0; c < lib->n_contigs; c++) {
        if (!lib->loaded[c]) {
            tdt_set_error("%s: library sequence %d is not loaded", fn, c);
            return TDT_E_ARG;
        }
    }
    if (n >= (1ull << 31) / (2ull * (ull)lib->n_contigs)) {
        tdt_set_error("%s: %zu queries x 2 strands x %d sequences (below 2^31 problems)", fn, n, lib->n_contigs);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

int sw_offsets_launch(tdt_ctx *ctx, size_t n_pairs, const unsigned *status, int *off) {
    hipLaunchKernelGGL(sw_count, dim3((unsigned)(n_pairs / KS_BLOCK + 1)), dim3(KS_BLOCK), 0, ctx->stream, (int)n_pairs, status, off);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ks_carry_sum, dim3(1), dim3(KS_BLOCK), 0, ctx->stream, off, (int)n_pairs + 1);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

int sw_build_launch(tdt_ctx *ctx, ins_sites S, size_t n_pairs, ins_out P, const int *off, sw_table T) {
    if (!n_pairs) return TDT_OK;
    hipLaunchKernelGGL(sw_build, dim3((unsigned)((n_pairs + KS_BLOCK - 1) / KS_BLOCK)), dim3(KS_BLOCK), 0, ctx->stream, S, (int)n_pairs, P, off, T);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

int sw_align_launch(tdt_ctx *ctx, const tdt_refseq *lib, size_t n, sw_queries Q, sw_work W) {
    if (!n) return TDT_OK;
    const size_t problems = n * 2 * (size_t)lib->n_contigs, per = SW_BLOCK / 64;
    const tdt_refview L{lib->d_store, lib->d_off, lib->d_len, lib->n_contigs};
    hipLaunchKernelGGL(sw_align_wave, dim3((unsigned)((problems + per - 1) / per)), dim3(SW_BLOCK), 0, ctx->stream, Q, (int)n, L, W.pkey, W.pend);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

int sw_reduce_launch(tdt_ctx *ctx, const tdt_refseq *lib, size_t n, sw_queries Q, sw_work W, int A, sw_out Out, ull *sn) {
    if (!n) return TDT_OK;
    hipLaunchKernelGGL(sw_reduce, dim3((unsigned)((n + KS_BLOCK - 1) / KS_BLOCK)), dim3(KS_BLOCK), 0, ctx->stream, Q, (int)n, lib->n_contigs, W.pkey, W.pend, (unsigned)A,
                       Out, sn);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

// ---- the entries on caller-owned query tables
static thread_local double sw_last_ms[2];     // tdt_sw_align_timing's

// One run over a DEVICE table: d_sn (TDT_SW_SN_N device words) is zeroed here.  Returns when the launches are done.
static int sw_run(const char *fn, tdt_ctx *ctx, const tdt_refseq *lib, size_t n, sw_queries Q, int A, sw_out Out, ull *d_sn) {
    hipStream_t st = ctx->stream;
    sw_work W{};
    void *d_work = nullptr;
    const size_t problems = n * 2 * (size_t)lib->n_contigs;
    if (n && tdt_dev_malloc(&d_work, W.lay(nullptr, problems)) != hipSuccess) {
        tdt_set_error("%s: out of device memory (%zu problems)", fn, problems);
        return TDT_E_NOMEM;
    }
    W.lay(d_work, problems);
    hipEvent_t ev[3] = {};
    hipError_t e = hipMemsetAsync(d_sn, 0, TDT_SW_SN_N * 8, st);
    for (int k = 0; k < 3 && e == hipSuccess; k++) e = hipEventCreate(&ev[k]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    int rc = e == hipSuccess ? sw_align_launch(ctx, lib, n, Q, W) : TDT_OK;
    if (rc == TDT_OK && e == hipSuccess) e = hipEventRecord(ev[1], st);
    if (rc == TDT_OK && e == hipSuccess) rc = sw_reduce_launch(ctx, lib, n, Q, W, A, Out, d_sn);
    if (rc == TDT_OK && e == hipSuccess) e = hipEventRecord(ev[2], st);
    if (rc == TDT_OK && e == hipSuccess) rc = tdt_ctx_sync(ctx);
    (void)hipStreamSynchronize(st);
    for (int k = 0; k < 2 && rc == TDT_OK && e == hipSuccess; k++) {
        float ms = 0;
        e = hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
        sw_last_ms[k] = ms;
    }
    for (int k = 0; k < 3; k++)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    if (d_work) (void)hipFree(d_work);
    if (rc) return rc;
    TDT_HIP(e);
    return TDT_OK;
}

// device milliseconds of this thread's last tdt_sw_align / tdt_sw_align_device that ran: ms2 = the alignment launch, the reduction
extern "C" int tdt_sw_align_timing(double *ms2) {
    if (!ms2) {
        tdt_set_error("tdt_sw_align_timing: bad argument");
        return TDT_E_ARG;
    }
    ms2[0] = sw_last_ms[0], ms2[1] = sw_last_ms[1];
    return TDT_OK;
}

static int sw_check_entry(const char *fn, tdt_ctx *ctx, const tdt_refseq *lib, size_t n, bool in, bool any, bool all, const void *sn, int A) {
    if (!ctx || !lib || !sn || (n && !in) || (any && !all)) {
        tdt_set_error("%s: bad argument", fn);
        return TDT_E_ARG;
    }
    return sw_check(fn, ctx, lib, n, A);
}

// Caller-owned DEVICE arrays: n queries in (d_seq10: TDT_SW_SEQ_WORDS words per query), d_sn_out: TDT_SW_SN_N words, nine result columns
// out.  All nine NULL: the counters alone.  A length above TDT_SW_QMAX is taken as TDT_SW_QMAX, a length of 0 has no positive cell.
extern "C" int tdt_sw_align_device(tdt_ctx *ctx, tdt_refseq *lib, size_t n, const uint64_t *d_seq10, const uint32_t *d_qlen, int A, uint64_t *d_sn_out,
                                   uint32_t *d_family, uint32_t *d_strand, uint32_t *d_score, uint32_t *d_qstart, uint32_t *d_qend, uint32_t *d_fstart,
                                   uint32_t *d_fend, uint32_t *d_second, uint32_t *d_second_family) {
    const bool any = d_family || d_strand || d_score || d_qstart || d_qend || d_fstart || d_fend || d_second || d_second_family;
    const bool all = d_family && d_strand && d_score && d_qstart && d_qend && d_fstart && d_fend && d_second && d_second_family;
    int rc = sw_check_entry("tdt_sw_align_device", ctx, lib, n, d_seq10 && d_qlen, any, all, d_sn_out, A);
    if (rc) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    return sw_run("tdt_sw_align_device", ctx, lib, n, sw_queries{(const ull *)d_seq10, d_qlen, nullptr, nullptr}, A,
                  sw_out{d_family, d_strand, d_score, d_qstart, d_qend, d_fstart, d_fend, d_second, d_second_family}, (ull *)d_sn_out);
}

// The same on HOST arrays: uploaded into a staging buffer that is freed before the return.  A length outside 1 ... TDT_SW_QMAX, or a
// word with a bit set at or beyond its query's last base: TDT_E_RANGE.
extern "C" int tdt_sw_align(tdt_ctx *ctx, tdt_refseq *lib, size_t n, const uint64_t *seq10, const uint32_t *qlen, int A, uint64_t *sn_out, uint32_t *family,
                            uint32_t *strand, uint32_t *score, uint32_t *qstart, uint32_t *qend, uint32_t *fstart, uint32_t *fend, uint32_t *second,
                            uint32_t *second_family) {
    const bool any = family || strand || score || qstart || qend || fstart || fend || second || second_family;
    const bool all = family && strand && score && qstart && qend && fstart && fend && second && second_family;
    int rc = sw_check_entry("tdt_sw_align", ctx, lib, n, seq10 && qlen, any, all, sn_out, A);
    if (rc) return rc;
    for (size_t i = 0; i < n; i++) {
        if (qlen[i] < 1 || qlen[i] > TDT_SW_QMAX) {
            tdt_set_error("tdt_sw_align: query %zu has %u bases (1 ... %d)", i, qlen[i], TDT_SW_QMAX);
            return TDT_E_RANGE;
        }
        for (int w = 0; w < TDT_SW_SEQ_WORDS; w++) {
            const int left = (int)qlen[i] - TDT_CLIP_COLS * w;
            const uint64_t keep = left >= TDT_CLIP_COLS ? (1ull << 56) - 1ull : left > 0 ? (1ull << (2 * left)) - 1ull : 0ull;
            if (seq10[i * TDT_SW_SEQ_WORDS + w] & ~keep) {
                tdt_set_error("tdt_sw_align: word %d of query %zu holds a code beyond its %u bases", w, i, qlen[i]);
                return TDT_E_RANGE;
            }
        }
    }
    TDT_HIP(hipSetDevice(ctx->device));
    struct {
        ull *seq10, *sn;
        unsigned *qlen;
        sw_out O;
        size_t lay(void *base, size_t n, size_t room) {
            tdt_carver cv(base);
            seq10 = cv.take<ull>(n * TDT_SW_SEQ_WORDS), sn = cv.take<ull>(TDT_SW_SN_N), qlen = cv.take<unsigned>(n);
            const size_t head = cv.size;
            return head + O.lay(base ? (char *)base + head : nullptr, room);
        }
    } D;
    const size_t room = any ? n : 0;
    void *d = nullptr;
    if (tdt_dev_malloc(&d, D.lay(nullptr, n, room)) != hipSuccess) {
        tdt_set_error("tdt_sw_align: out of device memory (%zu queries)", n);
        return TDT_E_NOMEM;
    }
    D.lay(d, n, room);
    if (!any) D.O = sw_out{};
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    if (n) {
        e = hipMemcpyAsync(D.seq10, seq10, n * TDT_SW_SEQ_WORDS * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(D.qlen, qlen, n * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    uint64_t res[TDT_SW_SN_N] = {};
    if (e == hipSuccess) {
        rc = sw_run("tdt_sw_align", ctx, lib, n, sw_queries{D.seq10, D.qlen, nullptr, nullptr}, A, D.O, D.sn);
        if (rc == TDT_OK) e = hipMemcpyAsync(res, D.sn, sizeof res, hipMemcpyDeviceToHost, st);
        if (rc == TDT_OK && e == hipSuccess && any && n) {
            uint32_t *dst[9] = {family, strand, score, qstart, qend, fstart, fend, second, second_family};
            const unsigned *src[9] = {D.O.family, D.O.strand, D.O.score, D.O.qstart, D.O.qend, D.O.fstart, D.O.fend, D.O.second, D.O.second_family};
            for (int k = 0; k < 9 && e == hipSuccess; k++) e = hipMemcpyAsync(dst[k], src[k], n * 4, hipMemcpyDeviceToHost, st);
        }
        if (rc == TDT_OK && e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (rc) return rc;
    TDT_HIP(e);
    memcpy(sn_out, res, sizeof res);
    return TDT_OK;
}
