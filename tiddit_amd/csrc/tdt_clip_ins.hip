// Insertion candidates from facing clip sites for gfx950 (TIDDIT_CLIPS_INS) — the extended consensus of a clip site (up to 140 columns,
// five words of 28 columns), the pairs of an R site and an L site that face each other, and the insertion closed where the two
// consensus overlap.  The definition is tiddit_clip_ins.py's (rules 3 to 5).  Integers throughout: device equals definition exactly.
// The extension KEYS (rule 2) are clip_ext_keys' in tdt_clip.hip, and their vote is the clip finish's own, run on the second store.
//   * clip_ext_gather — lane = reported site of the base store.  While the chunk in front has all 28 columns, the row
//     (c << 56 | K1, side) is looked up among the extension store's site rows by binary search and its columns are appended: depth
//     never increases with the column, so a chunk's CLEN can be used as it is, and a chunk without a row (fewer than S events reach
//     it) ends the consensus.  Per site ECLEN and five 64-bit words of 56 bits.
//   * the pair launches, none of whose workgroups waits for another: clip_ins_count<false> counts per tile of KS_TILE rows the facing
//     pairs of each R row — the candidates are the rows in front of it in key order that lie on its contig at P_R - 31 ... P_R (at
//     most 63 rows of distinct (K1, side); the walk is cut at INS_BACK = 66) and the one behind it (the L row at P_R + 1) — and adds
//     the site counters; ks_carry_sum turns the counts into offsets; clip_ins_count<true> writes each pair's two row indices and its
//     TSD at its offset, ascending by (t, P_R, P_L); clip_ins_pairs closes the pairs.
//   * clip_ins_pairs — one wavefront (= one workgroup of 64 lanes) per pair, grid-strided.  Both consensus are repacked from words
//     of 56 bits into one contiguous string of 2-bit codes (five 64-bit words, zero words behind them) in LDS, y reversed, so
//     that for an insertion of l bases x_i faces yr_{i + b - l}: one of the two strings shifted by |b - l| bases against the other.
//     The lanes stride over l = O ... a + b - O; a lane funnel-shifts the words of the shifted string (two neighbouring words each),
//     and per word: XOR, fold of the two bits of a base into one, mask to the overlap, popcount.  The best candidate is one packed
//     key mm << 16 | l under a wave minimum, CLOSURES a wave sum.  Lanes 0 ... 9 then write the ten SEQ words of a closed pair
//     (x up to min(a, l), the reversed y behind it), lane 0 the row's columns and the counters.
#include "tdt_clip_ins.h"
#include "tdt_keyscan.h"

typedef unsigned long long ull;

#define INS_BLOCK 64                          // clip_ins_pairs: one wavefront per pair
#define INS_GRID 4096                         // its workgroups at most (grid-strided over the pairs)
#define INS_BACK 66                           // rows in front of an R row that are looked at, at most
#define INS_WORDS 5                           // 64-bit words of a contiguous consensus (140 bases = 280 bits)
#define INS_LDS_WORDS 12                      // ... and zero words behind them: a shift reads word 4 + 4 + 1 at most

static_assert(TDT_CLIP_EXT_COLS == 140 && TDT_CLIP_EXT_WORDS == 5 && TDT_CLIP_COLS == 28, "five words of 28 columns");
static_assert(TDT_CLIP_INS_MAX_TSD == 32 && 2 * (TDT_CLIP_INS_MAX_TSD - 1) + 1 <= INS_BACK, "the rows in front of an R row that can face it");
static_assert(32 * INS_WORDS >= TDT_CLIP_EXT_COLS && INS_WORDS + (TDT_CLIP_EXT_COLS - 1) / 32 + 1 <= INS_LDS_WORDS, "the funnel shift stays inside the LDS words");
static_assert(2 * TDT_CLIP_EXT_COLS - 8 <= TDT_CLIP_COLS * INS_SEQ_WORDS, "a closed insertion fits its SEQ words");
static_assert(KS_TILE == 4096, "ins_work's tiles");


struct ins_min { template <class T> __device__ static T of(T a, T b) { return b < a ? b : a; } };

__device__ __forceinline__ unsigned ins_cols(unsigned eclen) { return eclen < (unsigned)TDT_CLIP_EXT_COLS ? eclen : (unsigned)TDT_CLIP_EXT_COLS; }

// ---- the extended consensus of the base store's rows
__global__ __launch_bounds__(KS_BLOCK) void clip_ext_gather(int n, const ull *__restrict__ k1, const unsigned *__restrict__ side, const unsigned *__restrict__ clen,
                                                            const ull *__restrict__ cons, int nx, ins_chunks X, unsigned *__restrict__ eclen,
                                                            ull *__restrict__ cons5) {
    const int i = blockIdx.x * KS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const ull key = k1[i], mask56 = (1ull << 56) - 1ull;
    const unsigned sd = side[i] & 1u;
    unsigned prev = clen[i] < (unsigned)TDT_CLIP_COLS ? clen[i] : (unsigned)TDT_CLIP_COLS, total = prev;
    ull *out = cons5 + (size_t)i * TDT_CLIP_EXT_WORDS;
    out[0] = cons[i] & mask56;
    for (int c = 1; c < TDT_CLIP_EXT_WORDS; c++) out[c] = 0;
    for (int c = 1; c < TDT_CLIP_EXT_WORDS && prev == (unsigned)TDT_CLIP_COLS; c++) {
        const ull want = ((ull)c << 56) | key;
        int lo = 0, hi = nx;                                       // the first row that is not below (want, sd)
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            const ull k = X.k1[mid];
            if (k < want || (k == want && (X.side[mid] & 1u) < sd)) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= nx || X.k1[lo] != want || (X.side[lo] & 1u) != sd) break;
        prev = X.clen[lo] < (unsigned)TDT_CLIP_COLS ? X.clen[lo] : (unsigned)TDT_CLIP_COLS;
        out[c] = X.cons[lo] & (prev ? mask56 >> (2u * ((unsigned)TDT_CLIP_COLS - prev)) : 0ull);
        total += prev;
    }
    eclen[i] = total;
}

// ---- the facing pairs of the rows
// whether row j is an L row with K columns or more at (tid, P) with lo <= P <= hi
__device__ __forceinline__ bool ins_faces(const ins_sites &S, int j, unsigned tid, long long lo, long long hi, unsigned K) {
    const ull k = S.k1[j];
    const long long P = (long long)(k & 0xffffffffull);
    return (unsigned)(k >> 32) == tid && P >= lo && P <= hi && (S.side[j] & 1u) == 0u && ins_cols(S.eclen[j]) >= K;
}
// whether row j lies on contig tid at lo or beyond (the walk in front of an R row goes on)
__device__ __forceinline__ bool ins_near(const ins_sites &S, int j, unsigned tid, long long lo) {
    const ull k = S.k1[j];
    return (unsigned)(k >> 32) == tid && (long long)(k & 0xffffffffull) >= lo;
}

// WRITE false: tile_n[tile] = the pairs of the tile's R rows, sn[IN_PAIRS] += them, and the three site counters.  WRITE true: tile_n
// holds the exclusive sums, and every pair's rows and TSD are written at its offset: an R row's pairs ascend by P_L.
template <bool WRITE>
__global__ __launch_bounds__(KS_BLOCK) void clip_ins_count(ins_sites S, int n, unsigned K, int *__restrict__ tile_n, ull *__restrict__ sn, ins_out Out) {
    __shared__ int s[KS_BLOCK / 64];
    const int t = threadIdx.x;
    const int t0 = blockIdx.x * KS_TILE;
    const int row0 = WRITE ? tile_n[blockIdx.x] : 0;
    int pairs = 0;                                                 // (uniform over the workgroup)
    unsigned n_ext = 0, n_left = 0, n_right = 0;
    for (int r = 0; r < KS_TILE / KS_BLOCK; r++) {                 // (uniform: every thread takes every round)
        const int i = t0 + r * KS_BLOCK + t;
        int mine = 0, jlo = i;
        bool behind = false;
        unsigned tid = 0;
        long long PR = 0;
        if (i < n) {
            const unsigned cols = ins_cols(S.eclen[i]), sd = S.side[i] & 1u;
            n_ext += cols > (unsigned)TDT_CLIP_COLS, n_left += !sd && cols >= K, n_right += sd && cols >= K;
            if (sd && cols >= K) {
                const ull k = S.k1[i];
                tid = (unsigned)(k >> 32), PR = (long long)(k & 0xffffffffull);
                const long long lo = PR + 1 - TDT_CLIP_INS_MAX_TSD;
                while (jlo > 0 && i - jlo < INS_BACK && ins_near(S, jlo - 1, tid, lo)) jlo--;
                for (int j = jlo; j < i; j++) mine += ins_faces(S, j, tid, lo, PR, K);
                behind = i + 1 < n && ins_faces(S, i + 1, tid, PR + 1, PR + 1, K);
                mine += behind;
            }
        }
        int all;
        const int incl = ks_block_scan<tdt_sum>(mine, 0, s, t, &all);
        if (WRITE && mine) {
            size_t at = (size_t)row0 + (size_t)(pairs + incl - mine);
            const long long lo = PR + 1 - TDT_CLIP_INS_MAX_TSD;
            for (int j = jlo; j <= i + 1; j++) {
                if (j == i || (j == i + 1 && !behind) || (j < i && !ins_faces(S, j, tid, lo, PR, K))) continue;
                Out.r_row[at] = (unsigned)i, Out.l_row[at] = (unsigned)j;
                Out.tsd[at] = (unsigned)(PR + 1 - (long long)(S.k1[j] & 0xffffffffull));
                at++;
            }
        }
        pairs += all;
    }
    if (!WRITE) {
        n_ext = tdt_wave_reduce<tdt_sum>(n_ext), n_left = tdt_wave_reduce<tdt_sum>(n_left), n_right = tdt_wave_reduce<tdt_sum>(n_right);
        if ((t & 63) == 0) {
            if (n_ext) atomicAdd(&sn[IN_EXTENDED], (ull)n_ext);
            if (n_left) atomicAdd(&sn[IN_LEFT], (ull)n_left);
            if (n_right) atomicAdd(&sn[IN_RIGHT], (ull)n_right);
        }
        if (t == 0) {
            tile_n[blockIdx.x] = pairs;
            if (pairs) atomicAdd(&sn[IN_PAIRS], (ull)pairs);
        }
    }
}

// ---- the closure of the pairs
// base i of a consensus of `cols` columns in words of 56 bits
__device__ __forceinline__ ull ins_code56(const ull *__restrict__ w5, unsigned i) { return (w5[i / TDT_CLIP_COLS] >> (2u * (i % TDT_CLIP_COLS))) & 3ull; }
// word w of the contiguous string s shifted down by t bases (s has zero words behind its last)
__device__ __forceinline__ ull ins_shifted(const ull *s, unsigned t, int w) {
    const unsigned q = t >> 5, r = 2u * (t & 31u);
    const ull lo = s[w + q], hi = s[w + q + 1];
    return r ? (lo >> r) | (hi << (64u - r)) : lo;
}

__global__ __launch_bounds__(INS_BLOCK) void clip_ins_pairs(ins_sites S, int n_pairs, unsigned O, unsigned M, ins_out Out, ull *__restrict__ sn) {
    __shared__ ull s_x[INS_LDS_WORDS], s_y[INS_LDS_WORDS];         // x, and y reversed (yr_k = y_{b-1-k}), contiguous 2-bit codes
    const int lane = threadIdx.x;
    for (int p = blockIdx.x; p < n_pairs; p += gridDim.x) {        // (uniform over the workgroup = the wave)
        const unsigned r = Out.r_row[p], l_ = Out.l_row[p];
        const int a = (int)ins_cols(S.eclen[r]), b = (int)ins_cols(S.eclen[l_]);
        if (lane < 2 * INS_LDS_WORDS) {
            const bool isy = lane >= INS_LDS_WORDS;
            const int w = isy ? lane - INS_LDS_WORDS : lane, cols = isy ? b : a;
            const ull *w5 = S.cons5 + (size_t)(isy ? l_ : r) * TDT_CLIP_EXT_WORDS;
            ull v = 0;
            if (w < INS_WORDS)
                for (int k = 0; k < 32; k++) {
                    const int i = 32 * w + k;
                    if (i < cols) v |= ins_code56(w5, (unsigned)(isy ? cols - 1 - i : i)) << (2 * k);
                }
            (isy ? s_y : s_x)[w] = v;
        }
        __syncthreads();
        unsigned best = 0xffffffffu, closures = 0;
        for (int l = (int)O + lane; l <= a + b - (int)O; l += INS_BLOCK) {
            // x_i faces yr_{i + b - l}: the overlap is columns [0, ov) of x shifted down by max(0, l - b) and yr shifted down by max(0, b - l)
            const int top = a < l ? a : l, ov = top - (l > b ? l - b : 0);
            if (ov < (int)O) continue;
            const unsigned tx = l > b ? (unsigned)(l - b) : 0u, ty = b > l ? (unsigned)(b - l) : 0u;
            unsigned mm = 0;
#pragma unroll
            for (int w = 0; w < INS_WORDS; w++) {
                const int nb = ov - 32 * w;
                const ull z = ins_shifted(s_x, tx, w) ^ ins_shifted(s_y, ty, w);
                const ull mask = nb >= 32 ? ~0ull : nb > 0 ? (1ull << (2 * nb)) - 1ull : 0ull;
                mm += (unsigned)__popcll((z | (z >> 1)) & 0x5555555555555555ull & mask);
            }
            if (mm <= M) {
                const unsigned key = (mm << 16) | (unsigned)l;
                best = key < best ? key : best;
                closures++;
            }
        }
        best = tdt_wave_reduce<ins_min>(best), closures = tdt_wave_reduce<tdt_sum>(closures);
        const bool closed = best != 0xffffffffu;
        const int len = closed ? (int)(best & 0xffffu) : 0, top = a < len ? a : len;
        if (lane < INS_SEQ_WORDS) {
            ull v = 0;
            for (int j = 0; j < TDT_CLIP_COLS; j++) {
                const int i = TDT_CLIP_COLS * lane + j;
                if (i >= len) break;
                const int k = i < top ? i : i + b - len;                             // in x, or in yr (top <= k < b: l <= a + b - O)
                v |= (((i < top ? s_x : s_y)[k >> 5] >> (2 * (k & 31))) & 3ull) << (2 * j);
            }
            Out.seq10[(size_t)p * INS_SEQ_WORDS + lane] = v;
        }
        if (lane == 0) {
            Out.status[p] = closed, Out.len[p] = (unsigned)len, Out.mm[p] = closed ? best >> 16 : 0u, Out.closures[p] = closures;
            if (sn) {
                atomicAdd(&sn[closed ? IN_CLOSED : IN_OPEN], 1ull);
                if (closures > 1) atomicAdd(&sn[IN_MULTI], 1ull);
            }
        }
        __syncthreads();                                           // (the words are the next pair's)
    }
}

// ---- the launches
int ins_check_range(const char *fn, int K, int O, int M) {
    if (K < TDT_CLIP_INS_MIN_COLS || K > TDT_CLIP_EXT_COLS || O < TDT_CLIP_INS_MIN_OVERLAP || O > TDT_CLIP_EXT_COLS || M < 0 || M > TDT_CLIP_INS_MAX_MISMATCH) {
        tdt_set_error("%s: minimum columns %d (%d ... %d), minimum overlap %d (%d ... %d), maximum mismatches %d (0 ... %d)", fn, K, TDT_CLIP_INS_MIN_COLS,
                      TDT_CLIP_EXT_COLS, O, TDT_CLIP_INS_MIN_OVERLAP, TDT_CLIP_EXT_COLS, M, TDT_CLIP_INS_MAX_MISMATCH);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

int ins_gather_launch(tdt_ctx *ctx, size_t n, const ull *k1, const unsigned *side, const unsigned *clen, const ull *cons, size_t nx, ins_chunks X, unsigned *eclen,
                      ull *cons5) {
    if (!n) return TDT_OK;
    hipLaunchKernelGGL(clip_ext_gather, dim3((unsigned)((n + KS_BLOCK - 1) / KS_BLOCK)), dim3(KS_BLOCK), 0, ctx->stream, (int)n, k1, side, clen, cons, (int)nx, X, eclen,
                       cons5);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

int ins_count_launch(tdt_ctx *ctx, size_t n, ins_sites S, int K, ins_work W, ull *sn) {
    if (!n) return TDT_OK;
    const unsigned ntiles = (unsigned)((n + KS_TILE - 1) / KS_TILE);
    hipLaunchKernelGGL(clip_ins_count<false>, dim3(ntiles), dim3(KS_BLOCK), 0, ctx->stream, S, (int)n, (unsigned)K, W.tile_pairs, sn, ins_out{});
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ks_carry_sum, dim3(1), dim3(KS_BLOCK), 0, ctx->stream, W.tile_pairs, (int)ntiles);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

int ins_pairs_launch(tdt_ctx *ctx, size_t n, ins_sites S, int K, int O, int M, ins_work W, size_t n_pairs, ins_out Out, ull *sn) {
    if (!n || !n_pairs) return TDT_OK;
    const unsigned ntiles = (unsigned)((n + KS_TILE - 1) / KS_TILE);
    hipLaunchKernelGGL(clip_ins_count<true>, dim3(ntiles), dim3(KS_BLOCK), 0, ctx->stream, S, (int)n, (unsigned)K, W.tile_pairs, sn, Out);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_ins_pairs, dim3(n_pairs < INS_GRID ? (unsigned)n_pairs : INS_GRID), dim3(INS_BLOCK), 0, ctx->stream, S, (int)n_pairs, (unsigned)O,
                       (unsigned)M, Out, sn);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

// ---- the entries on caller-owned site columns
// One run over DEVICE site columns: count; then, where the caller gave room, the pairs.  d_sn: TDT_CLIP_INS_SN_N device words (zeroed
// here).  *n_pairs in: the room of Out (ignored when `any` is false), out: the pairs.  Too little room: TDT_E_RANGE before anything of
// the caller's is written.  Returns when the launches are done.
static int ins_run(const char *fn, tdt_ctx *ctx, size_t n, ins_sites S, int K, int O, int M, ull *d_sn, bool any, ins_out Out, size_t *n_pairs) {
    hipStream_t st = ctx->stream;
    ins_work W{};
    void *d_work = nullptr;
    if (n && tdt_dev_malloc(&d_work, W.lay(nullptr, n)) != hipSuccess) {
        tdt_set_error("%s: out of device memory (%zu sites)", fn, n);
        return TDT_E_NOMEM;
    }
    W.lay(d_work, n);
    ull pairs = 0;
    hipError_t e = hipMemsetAsync(d_sn, 0, TDT_CLIP_INS_SN_N * 8, st);
    int rc = e == hipSuccess ? ins_count_launch(ctx, n, S, K, W, d_sn) : TDT_OK;
    if (rc == TDT_OK && e == hipSuccess) e = hipMemcpyAsync(&pairs, d_sn + IN_PAIRS, 8, hipMemcpyDeviceToHost, st);
    if (rc == TDT_OK && e == hipSuccess) rc = tdt_ctx_sync(ctx);
    if (rc == TDT_OK && e == hipSuccess && any) {
        if (*n_pairs < (size_t)pairs) {
            tdt_set_error("%s: room for %zu pairs, %llu found", fn, *n_pairs, pairs);
            rc = TDT_E_RANGE;
        } else {
            rc = ins_pairs_launch(ctx, n, S, K, O, M, W, (size_t)pairs, Out, d_sn);
            if (rc == TDT_OK) rc = tdt_ctx_sync(ctx);
        }
    }
    (void)hipStreamSynchronize(st);
    if (d_work) (void)hipFree(d_work);
    if (rc) return rc;
    TDT_HIP(e);
    *n_pairs = (size_t)pairs;
    return TDT_OK;
}

static int ins_check_entry(const char *fn, tdt_ctx *ctx, size_t n, bool in, bool any, bool all, const void *sn, const size_t *n_pairs, int K, int O, int M) {
    if (!ctx || !sn || !n_pairs || n >= (size_t)INS_MAX_SITES || (n && !in) || (any && !all)) {
        tdt_set_error("%s: bad argument", fn);
        return TDT_E_ARG;
    }
    return ins_check_range(fn, K, O, M);
}

// Caller-owned DEVICE arrays: n sites in (cons5: TDT_CLIP_EXT_WORDS words per site), d_sn_out: TDT_CLIP_INS_SN_N words, eight pair
// columns out (d_seq10: TDT_CLIP_INS_SEQ_WORDS words per pair).  All eight NULL: the counters of the sites and the pair count alone.
extern "C" int tdt_clip_ins_sites_device(tdt_ctx *ctx, size_t n, const uint64_t *d_k1, const uint32_t *d_side, const uint32_t *d_eclen, const uint64_t *d_cons5, int K,
                                         int O, int M, uint64_t *d_sn_out, uint32_t *d_r_row, uint32_t *d_l_row, uint32_t *d_tsd, uint32_t *d_status,
                                         uint32_t *d_len, uint32_t *d_mm, uint32_t *d_closures, uint64_t *d_seq10, size_t *n_pairs) {
    const bool any = d_r_row || d_l_row || d_tsd || d_status || d_len || d_mm || d_closures || d_seq10;
    const bool all = d_r_row && d_l_row && d_tsd && d_status && d_len && d_mm && d_closures && d_seq10;
    int rc = ins_check_entry("tdt_clip_ins_sites_device", ctx, n, d_k1 && d_side && d_eclen && d_cons5, any, all, d_sn_out, n_pairs, K, O, M);
    if (rc) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    // (the counters go to a staging line first: a call refused for its room leaves d_sn_out as it was)
    ull *d_sn = nullptr;
    if (tdt_dev_malloc((void **)&d_sn, TDT_CLIP_INS_SN_N * 8) != hipSuccess) {
        tdt_set_error("tdt_clip_ins_sites_device: out of device memory");
        return TDT_E_NOMEM;
    }
    size_t np = *n_pairs;
    rc = ins_run("tdt_clip_ins_sites_device", ctx, n, ins_sites{(const ull *)d_k1, d_side, d_eclen, (const ull *)d_cons5}, K, O, M, d_sn, any,
                 ins_out{d_r_row, d_l_row, d_tsd, d_status, d_len, d_mm, d_closures, (ull *)d_seq10}, &np);
    hipError_t e = hipSuccess;
    if (rc == TDT_OK) {
        e = hipMemcpyAsync(d_sn_out, d_sn, TDT_CLIP_INS_SN_N * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    (void)hipFree(d_sn);
    if (rc) return rc;
    TDT_HIP(e);
    *n_pairs = np;
    return TDT_OK;
}

// The same on HOST arrays: uploaded into a staging buffer that is freed before the return.  The sites must ascend strictly by
// (K1, side): TDT_E_ARG otherwise.
extern "C" int tdt_clip_ins_sites(tdt_ctx *ctx, size_t n, const uint64_t *k1, const uint32_t *side, const uint32_t *eclen, const uint64_t *cons5, int K, int O, int M,
                                  uint64_t *sn_out, uint32_t *r_row, uint32_t *l_row, uint32_t *tsd, uint32_t *status, uint32_t *len, uint32_t *mm,
                                  uint32_t *closures, uint64_t *seq10, size_t *n_pairs) {
    const bool any = r_row || l_row || tsd || status || len || mm || closures || seq10;
    const bool all = r_row && l_row && tsd && status && len && mm && closures && seq10;
    int rc = ins_check_entry("tdt_clip_ins_sites", ctx, n, k1 && side && eclen && cons5, any, all, sn_out, n_pairs, K, O, M);
    if (rc) return rc;
    for (size_t i = 1; i < n; i++)
        if (k1[i] < k1[i - 1] || (k1[i] == k1[i - 1] && (side[i] & 1u) <= (side[i - 1] & 1u))) {
            tdt_set_error("tdt_clip_ins_sites: the sites do not ascend by (K1, side) at %zu", i);
            return TDT_E_ARG;
        }
    TDT_HIP(hipSetDevice(ctx->device));
    const size_t room = any ? *n_pairs : 0;
    struct {
        ull *k1, *cons5, *sn;
        unsigned *side, *eclen;
        ins_out O;
        size_t lay(void *base, size_t n, size_t room) {
            tdt_carver cv(base);
            k1 = cv.take<ull>(n), cons5 = cv.take<ull>(n * TDT_CLIP_EXT_WORDS), sn = cv.take<ull>(TDT_CLIP_INS_SN_N), side = cv.take<unsigned>(n), eclen = cv.take<unsigned>(n);
            const size_t head = cv.size;
            return head + O.lay(base ? (char *)base + head : nullptr, room);
        }
    } D;
    void *d = nullptr;
    if (tdt_dev_malloc(&d, D.lay(nullptr, n, room)) != hipSuccess) {
        tdt_set_error("tdt_clip_ins_sites: out of device memory (%zu sites, %zu pairs)", n, room);
        return TDT_E_NOMEM;
    }
    D.lay(d, n, room);
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    if (n) {
        e = hipMemcpyAsync(D.k1, k1, n * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(D.cons5, cons5, n * TDT_CLIP_EXT_WORDS * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(D.side, side, n * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(D.eclen, eclen, n * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    uint64_t res[TDT_CLIP_INS_SN_N] = {};
    size_t np = room;
    if (e == hipSuccess) {
        rc = ins_run("tdt_clip_ins_sites", ctx, n, ins_sites{D.k1, D.side, D.eclen, D.cons5}, K, O, M, D.sn, any, D.O, &np);
        if (rc == TDT_OK) e = hipMemcpyAsync(res, D.sn, sizeof res, hipMemcpyDeviceToHost, st);
        if (rc == TDT_OK && e == hipSuccess && any && np) {
            uint32_t *dst[7] = {r_row, l_row, tsd, status, len, mm, closures};
            const unsigned *src[7] = {D.O.r_row, D.O.l_row, D.O.tsd, D.O.status, D.O.len, D.O.mm, D.O.closures};
            for (int k = 0; k < 7 && e == hipSuccess; k++) e = hipMemcpyAsync(dst[k], src[k], np * 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(seq10, D.O.seq10, np * INS_SEQ_WORDS * 8, hipMemcpyDeviceToHost, st);
        }
        if (rc == TDT_OK && e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (rc) return rc;
    TDT_HIP(e);
    memcpy(sn_out, res, sizeof res);
    *n_pairs = np;
    return TDT_OK;
}
