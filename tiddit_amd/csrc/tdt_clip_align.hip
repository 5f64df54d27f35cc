// Clip-site consensus realigned to the reference for gfx950 (TIDDIT_CLIPS_ALIGN) — for every clip site (a row of tdt_clip_finish) the
// best placement of its consensus of up to 28 bases on the same contig within W bases of the breakpoint, on either strand.  The
// definition is tiddit_clip_align.py's (rules 1 to 3): a candidate is (Q, strand), column j is compared with ref[Q + j] (R forward,
// L reverse) or ref[Q - j] (R reverse, L forward), with the base itself or its complement; all CLEN bases inside the contig; the best
// is the minimum of (mm, |Q - P|, strand, Q), HITS the candidates with mm <= M.  Integers throughout: device equals definition exactly.
//   * clip_align_sites — ONE launch per job, one workgroup per site (grid-strided over the sites; no workgroup waits for another).
//     The consensus becomes TWO patterns of 4-bit reference codes (A C G T = 1 2 4 8), 128 bits each with column 0 in the top nibble,
//     both laid out over ASCENDING reference bases: the one the definition reads ascending (the bases themselves for R, their
//     complements for L), and the one it reads descending, reversed, whose window starts at Q - CLEN + 1.  So ONE window of the reference
//     serves two candidates: the window that starts at base s is (Q = s) of the first and (Q = s + CLEN - 1) of the second.
//     Lane = window start, the workgroup strides over the starts qlo - CLEN + 1 ... qhi (CA_STRIDE per round; W = 2^20 is 8192 rounds).
//     A lane loads the three aligned 64-bit words that hold its 32 bases, swaps their bytes (base order monotone over the word, as in
//     tdt_ref_left16) and shifts them to its nibble phase; per pattern: XOR, fold every nibble to one bit, mask to CLEN nibbles,
//     popcount.  A code that is not A C G T (N, IUPAC, the zero of a guard) differs from every pattern nibble.
//     A window that is not wholly inside the contig is skipped BEFORE the load: a guard nibble would only count as a mismatch, and
//     the definition has no such candidate; and every load stays inside the store (a start inside the contig reads at most the two
//     guard words behind it).
//     A lane keeps its best candidate as one 64-bit key, mm << 53 | dist << 32 | strand << 31 | Q (mm <= 28 in 5 bits, dist <= 2^20 in
//     21, Q < 2^31), whose minimum is the definition's order, and a hit count; wave reduction, four words of LDS, lane 0 writes the row
//     and adds the site to the counters.
#include "tdt_bam_record.h"
#include "tdt_clip_align.h"

typedef unsigned long long ull;

#define CA_BLOCK 256
#define CA_STRIDE 256                         // window starts of one round of a workgroup: a lane each
#define CA_GRID 4096                          // workgroups at most (grid-strided over the sites): 16 per CU

static_assert(CA_STRIDE == CA_BLOCK, "lane = window start");
static_assert(TDT_CLIP_COLS == 28, "a pattern is 28 nibbles of two 64-bit words");
static_assert(TDT_REF_GUARD >= 16, "a window that starts inside the contig reads at most two words behind its last one");
static_assert(TDT_CLIP_ALIGN_MAX_WINDOW == 1 << 20, "the distance takes 21 bits of the key");

enum { CA_SHORT = 0, CA_OFF = 1, CA_SEARCHED = 2 };
enum { CA_SN_SITES = 0, CA_SN_SHORT, CA_SN_OFF, CA_SN_SEARCHED, CA_SN_ALIGNED, CA_SN_AMBIGUOUS, CA_SN_UNALIGNED, CA_SN_REF, CA_SN_DEL, CA_SN_DUP, CA_SN_INV,
       CA_SN_MATED, CA_SN_N };
static_assert(CA_SN_N == TDT_CLIP_ALIGN_SN_N, "SN rows");

struct ca_min { template <class T> __device__ static T of(T a, T b) { return b < a ? b : a; } };

// one bit per nibble of x that is not zero, in the nibble's lowest bit
__device__ __forceinline__ ull ca_fold(ull x) { return (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x1111111111111111ull; }

__global__ __launch_bounds__(CA_BLOCK) void clip_align_sites(tdt_refview R, int n, ca_sites S, unsigned W, unsigned K, unsigned M, ca_out O) {
    __shared__ ull s_key[CA_BLOCK / 64];
    __shared__ unsigned s_hits[CA_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int s = blockIdx.x; s < n; s += gridDim.x) {              // (uniform over the workgroup)
        const ull k1 = S.k1[s], cs = S.cons[s];
        const unsigned tid = (unsigned)(k1 >> 32), sd = S.side[s] & 1u;
        const long long P = (long long)(k1 & 0xffffffffull);
        const unsigned cl = S.clen[s] < (unsigned)TDT_CLIP_COLS ? S.clen[s] : (unsigned)TDT_CLIP_COLS;
        const long long len = tid < (unsigned)R.n ? (long long)R.len[tid] : -1ll;
        const unsigned status = cl < K ? CA_SHORT : (len < 0 || P < 1 || P > len) ? CA_OFF : CA_SEARCHED;
        ull key = ~0ull;
        unsigned hits = 0;
        if (status == CA_SEARCHED) {                               // (cl >= K >= 1)
            // ---- the two patterns and the mask of the CLEN leading nibbles
            ull ahi = 0, alo = 0, dhi = 0, dlo = 0, mhi = 0, mlo = 0;
            for (unsigned k = 0; k < cl; k++) {
                const unsigned ca = (unsigned)(cs >> (2u * k)) & 3u, cd = (unsigned)(cs >> (2u * (cl - 1u - k))) & 3u;
                const unsigned sh = 60u - 4u * (k & 15u);
                const ull na = (1ull << (sd ? ca : 3u - ca)) << sh, nd = (1ull << (sd ? 3u - cd : cd)) << sh, one = 1ull << sh;
                if (k < 16u) ahi |= na, dhi |= nd, mhi |= one;
                else alo |= na, dlo |= nd, mlo |= one;
            }
            const unsigned str_a = sd ^ 1u, str_d = sd;            // ascending: forward for R, reverse for L; descending: the other
            const long long qlo = P - (long long)W > 1 ? P - (long long)W : 1, qhi = P + (long long)W < len ? P + (long long)W : len;
            const long long s_lo = qlo - (long long)cl + 1, n_starts = qhi - s_lo + 1;    // (<= 2 W + CLEN)
            const ull *__restrict__ words = reinterpret_cast<const ull *>(R.store + R.off[tid]);
            for (long long i = t; i < n_starts; i += CA_STRIDE) {
                const long long st = s_lo + i;                     // the window is bases st ... st + cl - 1, 1-based
                if (st < 1 || st + (long long)cl - 1 > len) continue;
                const ull a = (ull)(st - 1);
                const ull *w = words + (a >> 4);
                const unsigned r = (unsigned)(a & 15ull) * 4u;
                const ull w0 = __builtin_bswap64(w[0]), w1 = __builtin_bswap64(w[1]), w2 = __builtin_bswap64(w[2]);
                const ull hi = r ? (w0 << r) | (w1 >> (64u - r)) : w0, lo = r ? (w1 << r) | (w2 >> (64u - r)) : w1;
                if (st >= qlo) {                                   // Q = st, read ascending
                    const unsigned mm = (unsigned)(__popcll(ca_fold(hi ^ ahi) & mhi) + __popcll(ca_fold(lo ^ alo) & mlo));
                    const ull dist = (ull)(st > P ? st - P : P - st);
                    const ull c = ((ull)mm << 53) | (dist << 32) | ((ull)str_a << 31) | (ull)st;
                    key = c < key ? c : key;
                    hits += mm <= M;
                }
                const long long qd = st + (long long)cl - 1;       // Q = the window's last base, read descending (qd >= qlo: st >= s_lo)
                if (qd <= qhi) {
                    const unsigned mm = (unsigned)(__popcll(ca_fold(hi ^ dhi) & mhi) + __popcll(ca_fold(lo ^ dlo) & mlo));
                    const ull dist = (ull)(qd > P ? qd - P : P - qd);
                    const ull c = ((ull)mm << 53) | (dist << 32) | ((ull)str_d << 31) | (ull)qd;
                    key = c < key ? c : key;
                    hits += mm <= M;
                }
            }
        }
        key = tdt_wave_reduce<ca_min>(key), hits = tdt_wave_reduce<tdt_sum>(hits);
        if (lane == 0) s_key[wave] = key, s_hits[wave] = hits;
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int k = 1; k < CA_BLOCK / 64; k++) key = s_key[k] < key ? s_key[k] : key, hits += s_hits[k];
            const bool have = key != ~0ull;
            const unsigned mm = have ? (unsigned)(key >> 53) : 0xffffffffu, strand = have ? (unsigned)(key >> 31) & 1u : 0u;
            const long long Q = have ? (long long)(key & 0x7fffffffull) : 0;
            O.status[s] = status, O.partner[s] = (unsigned)Q, O.strand[s] = strand, O.mm[s] = mm, O.hits[s] = have ? hits : 0u;
            if (O.sn) {
                atomicAdd(&O.sn[CA_SN_SITES], 1ull);
                atomicAdd(&O.sn[CA_SN_SHORT + status], 1ull);
                if (status == CA_SEARCHED && have && mm <= M) {
                    // rule 4
                    const int type = strand ? CA_SN_INV : sd ? (Q == P + 1 ? CA_SN_REF : Q > P + 1 ? CA_SN_DEL : CA_SN_DUP)
                                                             : (Q == P - 1 ? CA_SN_REF : Q < P - 1 ? CA_SN_DEL : CA_SN_DUP);
                    atomicAdd(&O.sn[CA_SN_ALIGNED], 1ull);
                    if (hits > 1) atomicAdd(&O.sn[CA_SN_AMBIGUOUS], 1ull);
                    atomicAdd(&O.sn[type], 1ull);
                } else if (status == CA_SEARCHED) {
                    atomicAdd(&O.sn[CA_SN_UNALIGNED], 1ull);
                }
            }
        }
        __syncthreads();                                           // (the four words are the next site's)
    }
}

int ca_check_range(const char *fn, int W, int K, int M) {
    if (W < 1 || W > TDT_CLIP_ALIGN_MAX_WINDOW || K < 1 || K > TDT_CLIP_COLS || M < 0 || M > TDT_CLIP_COLS - 1) {
        tdt_set_error("%s: window %d (1 ... 2^20), minimum columns %d (1 ... %d), maximum mismatches %d (0 ... %d)", fn, W, K, TDT_CLIP_COLS, M, TDT_CLIP_COLS - 1);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

int ca_launch(tdt_ctx *ctx, const tdt_refseq *ref, size_t n, ca_sites S, int W, int K, int M, ca_out O) {
    if (!n) return TDT_OK;
    const unsigned grid = n < CA_GRID ? (unsigned)n : CA_GRID;
    hipLaunchKernelGGL(clip_align_sites, dim3(grid), dim3(CA_BLOCK), 0, ctx->stream, tdt_refview{ref->d_store, ref->d_off, ref->d_len, ref->n_contigs}, (int)n, S,
                       (unsigned)W, (unsigned)K, (unsigned)M, O);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

// the checks the two entries share
static int ca_check_entry(const char *fn, tdt_ctx *ctx, tdt_refseq *ref, size_t n, bool pointers, int W, int K, int M) {
    if (!ctx || !ref || ref->ctx->device != ctx->device || n >= (1ull << 31) || (n && !pointers)) {
        tdt_set_error("%s: bad argument", fn);
        return TDT_E_ARG;
    }
    return ca_check_range(fn, W, K, M);
}

// Caller-owned DEVICE arrays of n entries each: the four site columns in, the five columns out.  Returns when the kernel is done.
extern "C" int tdt_clip_align_sites_device(tdt_ctx *ctx, tdt_refseq *ref, size_t n, const uint64_t *d_k1, const uint32_t *d_side, const uint32_t *d_clen,
                                           const uint64_t *d_consensus, int W, int K, int M, uint32_t *d_status, uint32_t *d_partner, uint32_t *d_strand,
                                           uint32_t *d_mm, uint32_t *d_hits) {
    const bool ptrs = d_k1 && d_side && d_clen && d_consensus && d_status && d_partner && d_strand && d_mm && d_hits;
    int rc = ca_check_entry("tdt_clip_align_sites_device", ctx, ref, n, ptrs, W, K, M);
    if (rc || !n) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    rc = ca_launch(ctx, ref, n, ca_sites{(const ull *)d_k1, d_side, d_clen, (const ull *)d_consensus}, W, K, M,
                   ca_out{d_status, d_partner, d_strand, d_mm, d_hits, nullptr});
    return rc ? rc : tdt_ctx_sync(ctx);
}

// The same on HOST arrays: uploaded into a staging buffer that is freed before the return.
extern "C" int tdt_clip_align_sites(tdt_ctx *ctx, tdt_refseq *ref, size_t n, const uint64_t *k1, const uint32_t *side, const uint32_t *clen,
                                    const uint64_t *consensus, int W, int K, int M, uint32_t *status_out, uint32_t *partner_out, uint32_t *strand_out,
                                    uint32_t *mm_out, uint32_t *hits_out) {
    const bool ptrs = k1 && side && clen && consensus && status_out && partner_out && strand_out && mm_out && hits_out;
    int rc = ca_check_entry("tdt_clip_align_sites", ctx, ref, n, ptrs, W, K, M);
    if (rc || !n) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_carver cv(nullptr);
    cv.take<ull>(n), cv.take<ull>(n);
    for (int k = 0; k < 7; k++) cv.take<unsigned>(n);
    void *d = nullptr;
    if (tdt_dev_malloc(&d, cv.size) != hipSuccess) {
        tdt_set_error("tdt_clip_align_sites: out of device memory (%zu sites)", n);
        return TDT_E_NOMEM;
    }
    tdt_carver at(d);
    ull *d_k1 = at.take<ull>(n), *d_cons = at.take<ull>(n);
    unsigned *d_side = at.take<unsigned>(n), *d_clen = at.take<unsigned>(n), *d_o[5];
    for (int k = 0; k < 5; k++) d_o[k] = at.take<unsigned>(n);
    hipStream_t st = ctx->stream;
    uint32_t *outs[5] = {status_out, partner_out, strand_out, mm_out, hits_out};
    hipError_t e = hipMemcpyAsync(d_k1, k1, n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cons, consensus, n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_side, side, n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_clen, clen, n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        rc = ca_launch(ctx, ref, n, ca_sites{d_k1, d_side, d_clen, d_cons}, W, K, M, ca_out{d_o[0], d_o[1], d_o[2], d_o[3], d_o[4], nullptr});
        if (rc == TDT_OK) rc = tdt_ctx_sync(ctx);
        for (int k = 0; k < 5 && rc == TDT_OK && e == hipSuccess; k++) e = hipMemcpyAsync(outs[k], d_o[k], n * 4, hipMemcpyDeviceToHost, st);
        if (rc == TDT_OK && e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (rc) return rc;
    TDT_HIP(e);
    return TDT_OK;
}
