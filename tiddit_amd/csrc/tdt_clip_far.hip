// Clip-site consensus placed genome-wide for gfx950 (TIDDIT_CLIPS_FAR) — for every clip site (a row of tdt_clip_finish) the best placement
// of its consensus on ANY loaded contig, on either strand, whose first 16 columns (the SEED) match exactly and whose other columns differ
// in at most M places.  The definition is tiddit_clip_far.py's (rules 1 to 3): a candidate is (t, Q, strand), the reading direction and
// the complement are those of tiddit_clip_align.py, all CLEN bases inside the contig; the best is the minimum of
// (mm, t != tid, |Q - P| on the site's own contig, strand, t, Q) over the candidates with mm <= M, HITS their number.  Integers throughout:
// device equals definition exactly.  The search is turned around against csrc/tdt_clip_align.hip: the reference streams ONCE, the sites
// are a small sorted table every reference position is tested against.
//   * far_seeds — a lane per site: status (rule 1), the slot of the site cleared, and for a searched site TWO table entries, from the
//     same two patterns clip_align_sites builds, both laid over ASCENDING reference bases: kind 0 the pattern the definition reads
//     ascending (seed = its first 16 bases, the window starts at Q), kind 1 the one it reads descending, reversed (seed = its LAST 16
//     bases, the window ends at Q).  An entry is the seed as a 32-bit key of 2 bits per base (the first base on top), the value
//     site << 1 | kind, and the up to 12 other columns as one-hot nibbles in ascending reference order (top-aligned).  A site that is
//     not searched gets two entries with bit 32 set, which sort behind every live one.  Each live key sets its bit of the filter:
//     bit (key * FAR_HASH_MUL mod 2^32) >> (32 - FAR_FILTER_LOG2).
//   * tdt_radix_sort_pairs by the 33 key bits.
//   * far_scan — ONE launch over the whole packed store, guards and unloaded contigs included (their zero nibbles are no base).  The
//     filter (FAR_FILTER_LOG2 = 19: 64 KiB) is copied into LDS once per workgroup; two workgroups fit a CU.  A workgroup takes tiles of
//     FAR_TILE window starts, grid-strided; a lane FAR_RUN = 32 consecutive starts: the two aligned 64-bit words that hold them and the
//     word behind, byte-swapped (base order monotone over the word), each folded ONCE to 32 bits of 2-bit codes and to a word that is
//     non-zero in the nibbles that are not A C G T.  The key of a start is a funnel shift of two folded words; a start with a nibble that
//     is no base in its 16 is no seed (N, IUPAC, the zero of a guard: a window can never run from one contig into the next).  The lane
//     probes the filter; only for a set bit it bounds the equal-key run of the sorted table (binary search), finds the contig of the
//     start (binary search over the offsets) and per entry of the run checks that the whole CLEN window lies inside the contig BEFORE it
//     loads the other columns (at most two words, both holding a base of the window: inside the store), XOR, fold, mask, popcount.
//     A candidate with mm <= M goes into the lane's accumulator (one site, the minimum key, the count); another site flushes it with
//     one 64-bit atomic min and one atomic add.  Behind every tile the wave merges its lanes' accumulators per site before the
//     atomics: a poly-A seed in a poly-A stretch is one pair of atomics per wave and tile, not one per base.
//     The key: mm << 60 | other << 59 | on the site's own contig dist << 2 | strand << 1 | (Q > P)
//                                     | on another contig    strand << 55 | t << 31 | Q
//     (mm <= 12 in 4 bits, dist and Q < 2^31, t < 2^24 = FAR_MAX_CONTIGS), whose minimum is the definition's order: on the own contig t is
//     the site's and Q is P - dist or P + dist.  No workgroup waits for another.
//   * far_rows — a lane per site: the slot becomes the six columns, and the site is added to the counters.
#include "tdt_bam_record.h"
#include "tdt_clip_far.h"

typedef unsigned long long ull;

#define FAR_BLOCK 512
#define FAR_RUN 32                            // window starts of a lane: two aligned 64-bit words
#define FAR_TILE 16384                        // window starts of a workgroup's round
#define FAR_GRID 512                          // workgroups at most (grid-strided over the tiles): two per CU, by the filter's LDS
#define FAR_FILTER_LOG2 19                    // bits of the filter: 64 KiB of LDS
#define FAR_HASH_MUL 2654435761               // bit = (key * FAR_HASH_MUL mod 2^32) >> (32 - FAR_FILTER_LOG2)
#define FAR_FILTER_WORDS (1 << (FAR_FILTER_LOG2 - 5))
#define FAR_SEEDS_BLOCK 256
#define FAR_DEAD (1ull << 32)                 // the key of an entry that is not searched
#define FAR_KEY_MASK 0x1ffffffffull

static_assert(FAR_TILE == FAR_BLOCK * FAR_RUN && FAR_RUN == 32, "a lane takes two words of 16 starts");
static_assert(FAR_FILTER_WORDS <= FAR_FILTER_WORDS_MAX && FAR_FILTER_WORDS % FAR_BLOCK == 0, "the workspace holds the filter; the copy is whole rounds");
static_assert(TDT_CLIP_FAR_SEED == 16, "the seed is one 64-bit word of nibbles, 32 bits of 2-bit codes");
static_assert(TDT_CLIP_COLS == 28, "the other columns are at most 12 nibbles of one 64-bit word");
static_assert(TDT_REF_GUARD >= 16, "a seed of 16 bases cannot span a guard");

enum { FAR_SHORT = 0, FAR_OFF = 1, FAR_SEARCHED = 2 };
enum { FAR_SN_SITES = 0, FAR_SN_SHORT, FAR_SN_OFF, FAR_SN_SEARCHED, FAR_SN_PLACED, FAR_SN_AMBIGUOUS, FAR_SN_UNPLACED, FAR_SN_SAME, FAR_SN_OTHER, FAR_SN_REVERSE,
       FAR_SN_MATED, FAR_SN_N };
static_assert(FAR_SN_N == TDT_CLIP_FAR_SN_N, "SN rows");

struct far_min { template <class T> __device__ static T of(T a, T b) { return b < a ? b : a; } };

// the table as the kernels see it
struct far_tab {
    ull *keys;                                // far_seeds: unsorted; far_scan: sorted
    unsigned *vals;
    ull *tails, *slot_key, *slot_hits, *state;    // state[0]: the live entries
    unsigned *filter;
};

// one bit per nibble of x that is not zero, in the nibble's lowest bit
__device__ __forceinline__ ull far_fold(ull x) { return (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x1111111111111111ull; }

// 16 one-hot nibbles (A C G T = 1 2 4 8) -> 32 bits of 2-bit codes in the same order (a nibble that is no base gives garbage)
__device__ __forceinline__ unsigned far_pack2(ull x) {
    const ull m = 0x1111111111111111ull;
    ull c = (((x >> 1) | (x >> 3)) & m) | ((((x >> 2) | (x >> 3)) & m) << 1);
    c = (c | (c >> 2)) & 0x0f0f0f0f0f0f0f0full;
    c = (c | (c >> 4)) & 0x00ff00ff00ff00ffull;
    c = (c | (c >> 8)) & 0x0000ffff0000ffffull;
    return (unsigned)(c | (c >> 16));
}

__device__ __forceinline__ unsigned far_hash(unsigned key) { return (key * (unsigned)FAR_HASH_MUL) >> (32 - FAR_FILTER_LOG2); }

__global__ __launch_bounds__(FAR_SEEDS_BLOCK) void far_seeds(tdt_refview R, int n, ca_sites S, unsigned K, far_tab T, unsigned *__restrict__ status_out) {
    const int i = blockIdx.x * FAR_SEEDS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const ull k1 = S.k1[i], cs = S.cons[i];
    const unsigned tid = (unsigned)(k1 >> 32), sd = S.side[i] & 1u;
    const long long P = (long long)(k1 & 0xffffffffull);
    const unsigned cl = S.clen[i] < (unsigned)TDT_CLIP_COLS ? S.clen[i] : (unsigned)TDT_CLIP_COLS;
    const long long len = tid < (unsigned)R.n ? (long long)R.len[tid] : -1ll;
    const unsigned status = cl < K ? FAR_SHORT : (len < 0 || P < 1 || P > len) ? FAR_OFF : FAR_SEARCHED;
    status_out[i] = status;
    T.slot_key[i] = ~0ull, T.slot_hits[i] = 0;
    T.vals[2 * i] = 2u * (unsigned)i, T.vals[2 * i + 1] = 2u * (unsigned)i + 1u;
    if (status != FAR_SEARCHED) {
        T.keys[2 * i] = T.keys[2 * i + 1] = FAR_DEAD;
        T.tails[2 * i] = T.tails[2 * i + 1] = 0;
        return;
    }
    // (cl >= K >= 16)
    unsigned ka = 0, kd = 0;
    for (unsigned j = 0; j < 16u; j++) {
        const unsigned c = (unsigned)(cs >> (2u * j)) & 3u;
        ka |= (sd ? c : 3u - c) << (30u - 2u * j);                 // ascending: column j is base j of the window
        kd |= (sd ? 3u - c : c) << (2u * j);                       // descending: column j is base Q - j, the seed's base 15 - j
    }
    const unsigned need = cl - 16u;
    ull ta = 0, td = 0;
    for (unsigned k = 0; k < need; k++) {
        const unsigned ca = (unsigned)(cs >> (2u * (16u + k))) & 3u, cd = (unsigned)(cs >> (2u * (16u + need - 1u - k))) & 3u;
        ta |= (1ull << (sd ? ca : 3u - ca)) << (60u - 4u * k);     // base Q + 16 + k
        td |= (1ull << (sd ? 3u - cd : cd)) << (60u - 4u * k);     // base Q - 15 - need + k
    }
    T.keys[2 * i] = ka, T.keys[2 * i + 1] = kd;
    T.tails[2 * i] = ta, T.tails[2 * i + 1] = td;
    const unsigned ha = far_hash(ka), hd = far_hash(kd);
    atomicOr(&T.filter[ha >> 5], 1u << (ha & 31u));
    atomicOr(&T.filter[hd >> 5], 1u << (hd & 31u));
    atomicAdd(&T.state[0], 2ull);
}

// a lane's accumulator goes to its site's slot
__device__ __forceinline__ void far_flush(const far_tab &T, unsigned site, ull key, ull hits) {
    atomicMin(&T.slot_key[site], key);
    atomicAdd(&T.slot_hits[site], hits);
}

__global__ __launch_bounds__(FAR_BLOCK) void far_scan(tdt_refview R, ull nwords, ca_sites S, far_tab T, unsigned M) {
    __shared__ unsigned s_filter[FAR_FILTER_WORDS];
    const unsigned n_live = (unsigned)T.state[0];                  // (< 2^30)
    if (!n_live) return;                                           // (uniform over the grid: nothing is searched)
    for (int k = threadIdx.x; k < FAR_FILTER_WORDS; k += FAR_BLOCK) s_filter[k] = T.filter[k];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const ull *__restrict__ words = reinterpret_cast<const ull *>(R.store);
    const ull ntiles = (nwords * 16ull + FAR_TILE - 1) / FAR_TILE;
    unsigned acc_site = 0;
    ull acc_key = ~0ull, acc_hits = 0;                             // (acc_hits == 0: the accumulator is empty)
    for (ull tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {    // (uniform over the workgroup)
        const ull w = (tile * FAR_BLOCK + threadIdx.x) * 2ull;     // the lane's first word; its starts are nibbles 16 w ... 16 w + 31
        ull x[3] = {0, 0, 0};
        if (w + 1 < nwords) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(words + w);     // (w is even and the store a device allocation: 16-byte aligned)
            x[0] = __builtin_bswap64(v.x), x[1] = __builtin_bswap64(v.y);
            if (w + 2 < nwords) x[2] = __builtin_bswap64(words[w + 2]);
        } else if (w < nwords) {
            x[0] = __builtin_bswap64(words[w]);
        }
        unsigned hm = 0;                                           // the starts of the run whose filter bit is set
        unsigned p2[3] = {0, 0, 0};
        if (x[0] | x[1]) {                                         // (a start inside zero words is no seed)
            ull bad[3];
#pragma unroll
            for (int k = 0; k < 3; k++) p2[k] = far_pack2(x[k]), bad[k] = tdt_ref_not_acgt(x[k]);
#pragma unroll
            for (int p = 0; p < FAR_RUN; p++) {
                const int a = p >> 4, q = p & 15;
                const ull b = q ? (bad[a] << (4 * q)) | (bad[a + 1] >> (64 - 4 * q)) : bad[a];
                const unsigned key = q ? (p2[a] << (2 * q)) | (p2[a + 1] >> (32 - 2 * q)) : p2[a];
                const unsigned h = far_hash(key);
                if (!b && ((s_filter[h >> 5] >> (h & 31u)) & 1u)) hm |= 1u << p;
            }
        }
        while (hm) {
            const unsigned p = (unsigned)__ffs(hm) - 1u;
            hm &= hm - 1u;
            const unsigned q = p & 15u, k_lo = p < 16u ? p2[0] : p2[1], k_hi = p < 16u ? p2[1] : p2[2];
            const unsigned key = q ? (k_lo << (2u * q)) | (k_hi >> (32u - 2u * q)) : k_lo;
            // ---- the equal-key run of the sorted table
            unsigned lo = 0, hi = n_live;
            while (lo < hi) {
                const unsigned mid = (lo + hi) >> 1;
                if (T.keys[mid] < (ull)key) lo = mid + 1u;
                else hi = mid;
            }
            if (lo >= n_live || T.keys[lo] != (ull)key) continue;  // the filter's false positive
            // ---- the contig of the start: the last one whose offset is not behind it
            const ull g = w * 16ull + p, byte = g >> 1;
            int tl = 0, th = R.n;
            if (th < 1) continue;
            while (th - tl > 1) {
                const int mid = (tl + th) >> 1;
                if (R.off[mid] <= byte) tl = mid;
                else th = mid;
            }
            const ull off = R.off[tl];
            const long long len = (long long)R.len[tl];
            if (byte < off || len < 16) continue;
            const long long pos = (long long)(g - 2ull * off);     // 0-based in the contig
            if (pos + 16 > len) continue;
            for (unsigned e = lo; e < n_live && T.keys[e] == (ull)key; e++) {
                const unsigned v = T.vals[e], site = v >> 1, kind = v & 1u;
                const unsigned cl = S.clen[site] < (unsigned)TDT_CLIP_COLS ? S.clen[site] : (unsigned)TDT_CLIP_COLS;
                const unsigned need = cl - 16u;
                long long Q;
                ull tg;                                            // the store nibble of the first other column, ascending
                if (kind == 0u) {
                    if (pos + (long long)cl > len) continue;       // the window is bases pos + 1 ... pos + cl
                    Q = pos + 1, tg = g + 16ull;
                } else {
                    if (pos < (long long)need) continue;           // the window is bases pos + 16 - cl + 1 ... pos + 16
                    Q = pos + 16, tg = g - need;
                }
                unsigned mm = 0;
                if (need) {
                    const ull wi = tg >> 4;
                    const unsigned r = (unsigned)(tg & 15ull) * 4u;
                    ull y = __builtin_bswap64(words[wi]) << r;
                    if (r + 4u * need > 64u) y |= __builtin_bswap64(words[wi + 1]) >> (64u - r);      // (r > 0 here)
                    mm = (unsigned)__popcll(far_fold(y ^ T.tails[v]) & (0x1111111111111111ull << (64u - 4u * need)));
                }
                if (mm > M) continue;
                const ull k1 = S.k1[site];
                const unsigned tid = (unsigned)(k1 >> 32), sd = S.side[site] & 1u;
                const long long P = (long long)(k1 & 0xffffffffull);
                const ull strand = kind ? sd : sd ^ 1u;            // ascending: forward for R, reverse for L; descending: the other
                const ull c = (unsigned)tl == tid ? ((ull)mm << 60) | ((ull)(Q > P ? Q - P : P - Q) << 2) | (strand << 1) | (ull)(Q > P)
                                                  : ((ull)mm << 60) | (1ull << 59) | (strand << 55) | ((ull)tl << 31) | (ull)Q;
                if (acc_hits && site != acc_site) {
                    far_flush(T, acc_site, acc_key, acc_hits);
                    acc_key = ~0ull, acc_hits = 0;
                }
                acc_site = site, acc_key = c < acc_key ? c : acc_key, acc_hits++;
            }
        }
        // ---- behind the tile (the wave is whole again): the lanes' accumulators merged per site, one pair of atomics each
        ull pending = __ballot(acc_hits != 0);
        while (pending) {                                          // (uniform over the wave)
            const int leader = __ffsll((long long)pending) - 1;
            const unsigned ls = (unsigned)__shfl((int)acc_site, leader);
            const bool mine = acc_hits != 0 && acc_site == ls;
            const ull k = tdt_wave_reduce<far_min>(mine ? acc_key : ~0ull), h = tdt_wave_reduce<tdt_sum>(mine ? acc_hits : 0ull);
            if (lane == leader) far_flush(T, ls, k, h);
            if (mine) acc_key = ~0ull, acc_hits = 0;
            pending = __ballot(acc_hits != 0);
        }
    }
}

__global__ __launch_bounds__(FAR_SEEDS_BLOCK) void far_rows(int n, ca_sites S, far_tab T, far_out O) {
    const int i = blockIdx.x * FAR_SEEDS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned status = O.status[i];
    const ull key = T.slot_key[i], h = T.slot_hits[i], k1 = S.k1[i];
    const bool have = status == FAR_SEARCHED && key != ~0ull;
    unsigned ptid = 0, Q = 0, strand = 0, mm = FAR_NO_MM, hits = 0;
    if (have) {
        mm = (unsigned)(key >> 60);
        hits = h > 0xffffffffull ? 0xffffffffu : (unsigned)h;      // (saturates)
        if ((key >> 59) & 1ull) {
            strand = (unsigned)(key >> 55) & 1u, ptid = (unsigned)(key >> 31) & 0xffffffu, Q = (unsigned)(key & 0x7fffffffull);
        } else {
            const unsigned dist = (unsigned)((key >> 2) & 0x7fffffffull), P = (unsigned)(k1 & 0xffffffffull);
            strand = (unsigned)(key >> 1) & 1u, ptid = (unsigned)(k1 >> 32), Q = (key & 1ull) ? P + dist : P - dist;
        }
    }
    O.ptid[i] = ptid, O.partner[i] = Q, O.strand[i] = strand, O.mm[i] = mm, O.hits[i] = hits;
    if (O.sn) {
        atomicAdd(&O.sn[FAR_SN_SITES], 1ull);
        atomicAdd(&O.sn[FAR_SN_SHORT + status], 1ull);
        if (have) {
            atomicAdd(&O.sn[FAR_SN_PLACED], 1ull);
            if (hits > 1u) atomicAdd(&O.sn[FAR_SN_AMBIGUOUS], 1ull);
            atomicAdd(&O.sn[ptid == (unsigned)(k1 >> 32) ? FAR_SN_SAME : FAR_SN_OTHER], 1ull);
            if (strand) atomicAdd(&O.sn[FAR_SN_REVERSE], 1ull);
        } else if (status == FAR_SEARCHED) {
            atomicAdd(&O.sn[FAR_SN_UNPLACED], 1ull);
        }
    }
}

int far_check_range(const char *fn, const tdt_refseq *ref, size_t n, int K, int M) {
    if (K < TDT_CLIP_FAR_SEED || K > TDT_CLIP_COLS || M < 0 || M > TDT_CLIP_COLS - TDT_CLIP_FAR_SEED) {
        tdt_set_error("%s: minimum columns %d (%d ... %d), maximum mismatches %d (0 ... %d)", fn, K, TDT_CLIP_FAR_SEED, TDT_CLIP_COLS, M,
                      TDT_CLIP_COLS - TDT_CLIP_FAR_SEED);
        return TDT_E_RANGE;
    }
    if (ref->n_contigs > FAR_MAX_CONTIGS || n >= (size_t)FAR_MAX_SITES) {
        tdt_set_error("%s: %d contigs (at most 2^24), %zu sites (fewer than 2^29)", fn, ref->n_contigs, n);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

int far_launch(tdt_ctx *ctx, const tdt_refseq *ref, size_t n, ca_sites S, int K, int M, far_out O, far_work &Wk, hipEvent_t *ev) {
    hipStream_t st = ctx->stream;
    if (!n) {
        for (int k = 0; ev && k < 5; k++) TDT_HIP(hipEventRecord(ev[k], st));
        return TDT_OK;
    }
    const tdt_refview R{ref->d_store, ref->d_off, ref->d_len, ref->n_contigs};
    const unsigned sgrid = (unsigned)((n + FAR_SEEDS_BLOCK - 1) / FAR_SEEDS_BLOCK);
    far_tab T{Wk.keys, Wk.vals, Wk.tails, Wk.slot_key, Wk.slot_hits, Wk.state, Wk.filter};
    if (ev) TDT_HIP(hipEventRecord(ev[0], st));
    TDT_HIP(hipMemsetAsync(Wk.filter, 0, FAR_FILTER_WORDS * 4, st));
    TDT_HIP(hipMemsetAsync(Wk.state, 0, 2 * 8, st));
    hipLaunchKernelGGL(far_seeds, dim3(sgrid), dim3(FAR_SEEDS_BLOCK), 0, st, R, (int)n, S, (unsigned)K, T, O.status);
    TDT_CHECK_LAUNCH();
    if (ev) TDT_HIP(hipEventRecord(ev[1], st));
    const int rc = tdt_radix_sort_pairs(ctx, Wk.keys, Wk.vals, Wk.keys_tmp, Wk.vals_tmp, 2 * n, FAR_KEY_MASK, &T.keys, &T.vals);
    if (rc) return rc;
    if (ev) TDT_HIP(hipEventRecord(ev[2], st));
    const ull nwords = (ull)(ref->bytes / 8);
    const ull ntiles = (nwords * 16ull + FAR_TILE - 1) / FAR_TILE;
    if (ntiles) {
        hipLaunchKernelGGL(far_scan, dim3((unsigned)(ntiles < FAR_GRID ? ntiles : FAR_GRID)), dim3(FAR_BLOCK), 0, st, R, nwords, S, T, (unsigned)M);
        TDT_CHECK_LAUNCH();
    }
    if (ev) TDT_HIP(hipEventRecord(ev[3], st));
    hipLaunchKernelGGL(far_rows, dim3(sgrid), dim3(FAR_SEEDS_BLOCK), 0, st, (int)n, S, T, O);
    TDT_CHECK_LAUNCH();
    if (ev) TDT_HIP(hipEventRecord(ev[4], st));
    return TDT_OK;
}

// the checks the two entries share
static int far_check_entry(const char *fn, tdt_ctx *ctx, tdt_refseq *ref, size_t n, bool pointers, int K, int M) {
    if (!ctx || !ref || ref->ctx->device != ctx->device || n >= (1ull << 31) || (n && !pointers)) {
        tdt_set_error("%s: bad argument", fn);
        return TDT_E_ARG;
    }
    return far_check_range(fn, ref, n, K, M);
}

// the search over device columns with a workspace of its own, freed before the return; returns when the launches are done
static int far_run(const char *fn, tdt_ctx *ctx, tdt_refseq *ref, size_t n, ca_sites S, int K, int M, far_out O) {
    far_work Wk;
    void *d = nullptr;
    if (tdt_dev_malloc(&d, Wk.lay(nullptr, n)) != hipSuccess) {
        tdt_set_error("%s: out of device memory (%zu sites)", fn, n);
        return TDT_E_NOMEM;
    }
    Wk.lay(d, n);
    int rc = far_launch(ctx, ref, n, S, K, M, O, Wk, nullptr);
    const int rs = tdt_ctx_sync(ctx);
    (void)hipFree(d);
    return rc ? rc : rs;
}

// Caller-owned DEVICE arrays of n entries each: the four site columns in, the six columns out.  Returns when the launches are done.
extern "C" int tdt_clip_far_sites_device(tdt_ctx *ctx, tdt_refseq *ref, size_t n, const uint64_t *d_k1, const uint32_t *d_side, const uint32_t *d_clen,
                                         const uint64_t *d_consensus, int K, int M, uint32_t *d_status, uint32_t *d_partner_tid, uint32_t *d_partner,
                                         uint32_t *d_strand, uint32_t *d_mm, uint32_t *d_hits) {
    const bool ptrs = d_k1 && d_side && d_clen && d_consensus && d_status && d_partner_tid && d_partner && d_strand && d_mm && d_hits;
    const int rc = far_check_entry("tdt_clip_far_sites_device", ctx, ref, n, ptrs, K, M);
    if (rc || !n) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    return far_run("tdt_clip_far_sites_device", ctx, ref, n, ca_sites{(const ull *)d_k1, d_side, d_clen, (const ull *)d_consensus}, K, M,
                   far_out{d_status, d_partner_tid, d_partner, d_strand, d_mm, d_hits, nullptr});
}

// The same on HOST arrays: uploaded into a staging buffer that is freed before the return.
extern "C" int tdt_clip_far_sites(tdt_ctx *ctx, tdt_refseq *ref, size_t n, const uint64_t *k1, const uint32_t *side, const uint32_t *clen,
                                  const uint64_t *consensus, int K, int M, uint32_t *status_out, uint32_t *partner_tid_out, uint32_t *partner_out,
                                  uint32_t *strand_out, uint32_t *mm_out, uint32_t *hits_out) {
    const bool ptrs = k1 && side && clen && consensus && status_out && partner_tid_out && partner_out && strand_out && mm_out && hits_out;
    int rc = far_check_entry("tdt_clip_far_sites", ctx, ref, n, ptrs, K, M);
    if (rc || !n) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_carver cv(nullptr);
    cv.take<ull>(n), cv.take<ull>(n);
    for (int k = 0; k < 8; k++) cv.take<unsigned>(n);
    void *d = nullptr;
    if (tdt_dev_malloc(&d, cv.size) != hipSuccess) {
        tdt_set_error("tdt_clip_far_sites: out of device memory (%zu sites)", n);
        return TDT_E_NOMEM;
    }
    tdt_carver at(d);
    ull *d_k1 = at.take<ull>(n), *d_cons = at.take<ull>(n);
    unsigned *d_side = at.take<unsigned>(n), *d_clen = at.take<unsigned>(n), *d_o[6];
    for (int k = 0; k < 6; k++) d_o[k] = at.take<unsigned>(n);
    hipStream_t st = ctx->stream;
    uint32_t *outs[6] = {status_out, partner_tid_out, partner_out, strand_out, mm_out, hits_out};
    hipError_t e = hipMemcpyAsync(d_k1, k1, n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cons, consensus, n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_side, side, n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_clen, clen, n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        rc = far_run("tdt_clip_far_sites", ctx, ref, n, ca_sites{d_k1, d_side, d_clen, d_cons}, K, M, far_out{d_o[0], d_o[1], d_o[2], d_o[3], d_o[4], d_o[5], nullptr});
        for (int k = 0; k < 6 && rc == TDT_OK && e == hipSuccess; k++) e = hipMemcpyAsync(outs[k], d_o[k], n * 4, hipMemcpyDeviceToHost, st);
        if (rc == TDT_OK && e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (rc) return rc;
    TDT_HIP(e);
    return TDT_OK;
}
