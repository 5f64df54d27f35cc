// Clipped-read breakpoint sites for gfx950 — every reference position where eligible reads of the --sv scan are soft-clipped on one
// side (TIDDIT_CLIPS), with the support by strand and a consensus of the clipped bases beside the breakpoint.  The definition is
// tiddit_clips.py's: per clip of at least min_clip bases K1 = tid << 32 | P (1-based; the first aligned base for a leading clip, the
// last for a trailing one) and K2 = side << 63 | n << 58 | bases << 2 | rev, `bases` = the first n <= 28 clipped bases outward from the
// breakpoint, two bits each; equal (K1, K2 >> 1) is one distinct sequence, equal (K1, side) one site.  Every result is an
// order-independent integer, so it equals the definition exactly.
//   * clip_keys — ONE launch per batch, on the columns and record bytes that are already resident, enqueued beside snv_keys and waiting
//     for nothing.  Lane = read for the filters (flag, tid, mapq: coalesced columns).  The reads that need their bytes are compacted
//     inside the workgroup (tdt_block_slots), then lane = compacted read: the record is bounded with TDT_REC_*, exactly as tdt_snv
//     bounds one; ONE pass over the CIGAR sums its reference and query lengths and looks for an op code above 8; the first two and
//     the last two words decide the clips; up to 28 nibbles per clip are read byte by byte from the sequence (a leading clip is
//     walked backwards from its last base, a trailing one forwards from its first, so both nibble phases occur on both sides), and
//     the walk stops at the first code that is not A C G T.  At most two keys per read are staged in LDS (256 reads x 2 keys x 16 B =
//     8 KB) and appended to the store behind ONE atomic per workgroup; the counters and the sort masks are merged per wave and then
//     over the workgroup, one atomic per workgroup and non-zero word.
//     WHICH reads need their bytes: every eligible one.  The ingest's CIGAR_FIRST / CIGAR_LAST columns do equal the record's own first
//     and last words (tdt_ingest.hip's decode writes `n_cig ? ld_u32(cig) : 0xffffffff` and `n_cig ? ld_u32(cig + 4 * (n_cig - 1)) :
//     0xffffffff`: one word twice for n_cig == 1, an op code of 15 for n_cig == 0), but they cannot stand in for the bytes here: the
//     definition counts malformed, no_sequence and no_alignment over ALL eligible records (an op code above 8 in the middle of a CIGAR,
//     a query length that differs from l_seq), which only the CIGAR itself tells, and the host entry has no such columns.  So the
//     prefilter is the eligibility alone, as in snv_keys, and the cost is one short CIGAR pass per eligible read.
//   * tdt_clip_finish — once per job: ks_finish of tdt_keystore.h with a minimum support of 1: its rows are the distinct sequences in
//     key order with their counts and REV.  The side is the top bit of K2, so a site is a run of consecutive rows.  Then, none of whose
//     workgroups waits for another:
//       - clip_heads<false> counts per tile of KS_TILE rows the site heads (a change of (K1, K2 >> 63)), ks_carry_sum turns the counts
//         into offsets, clip_heads<true> writes the heads' row indices compacted: site s is rows [start[s], start[s + 1]);
//       - clip_vote: one wavefront (= one workgroup of 64 lanes, so the workgroup barrier is the wave's) per site, grid-strided over the
//         sites.  The lanes stride over the site's rows and add each row's count into a [28][4] vote table in LDS (LDS atomics: two rows
//         of one site mostly vote for the same bases); SUPPORT, REV and SEQS come from a wave reduction; lanes 0 ... 27 then take
//         their column's depth and winner (a tie to the smaller code), CLEN is the number of leading columns with depth >= S, the
//         packed consensus an OR, AGREE and TOTAL sums over the wave.  A site of tens of thousands of rows costs its rows / 64 steps;
//       - clip_keep<false> counts per tile the sites with SUPPORT >= S, ks_carry_sum again, clip_keep<true> writes them as rows in
//         key order.
#include <vector>

#include "tdt_keystore.h"

typedef unsigned long long ull;

#define CLIP_BLOCK 256
#define CLIP_K_TILE 256                       // reads of a clip_keys workgroup (one round); it stages at most 2 x that many keys in LDS (8 KB)
#define CLIP_VOTE_BLOCK 64                    // one wavefront per site
#define CLIP_VOTE_GRID 4096                   // workgroups of clip_vote at most (grid-strided over the sites)
#define CLIP_MAX_CONTIGS (1 << 24)
#define CLIP_END_LIMIT 0x7fffffffll           // pos + the CIGAR's reference length is at most this

static_assert(CLIP_K_TILE == CLIP_BLOCK, "one round per workgroup");
static_assert(TDT_CLIP_MAX_PER_READ == 2, "a leading and a trailing clip");
static_assert(TDT_CLIP_COLS == 28 && TDT_CLIP_COLS <= CLIP_VOTE_BLOCK, "56 bits of bases in K2; a lane per column");
static_assert(CLIP_VOTE_BLOCK == 64, "clip_vote's workgroup is one wavefront");

// the SN rows, in the order of the file; the first ten are the push's
enum { SN_RECORDS = 0, SN_ELIGIBLE, SN_MALFORMED, SN_NO_SEQUENCE, SN_NO_ALIGNMENT, SN_SHORT_CLIPS, SN_LEFT_CLIPS, SN_RIGHT_CLIPS, SN_CLIPPED_READS,
       SN_CUT, SN_DISTINCT_SEQS, SN_DISTINCT_SITES, SN_REPORTED, SN_N, SN_PUSH_N = SN_DISTINCT_SEQS };
static_assert(SN_N == TDT_CLIP_SN_N, "SN rows");
enum { ST_OR1 = SN_PUSH_N };                  // OR1, NAND1, OR2, NAND2 behind the push counters; KS_N, KS_OVERFLOW: tdt_keystore.h
static_assert(ST_OR1 + 4 <= KS_N, "state layout");

struct clip_sites {                           // per site (n entries each): what clip_vote writes / what clip_keep<true> keeps
    ull *k1, *cons, *agree, *total;
    unsigned *side, *sup, *rev, *seqs, *clen;
    size_t lay(tdt_carver &cv, size_t n) {
        k1 = cv.take<ull>(n), cons = cv.take<ull>(n), agree = cv.take<ull>(n), total = cv.take<ull>(n);
        side = cv.take<unsigned>(n), sup = cv.take<unsigned>(n), rev = cv.take<unsigned>(n), seqs = cv.take<unsigned>(n), clen = cv.take<unsigned>(n);
        return cv.size;
    }
};

struct tdt_clip {
    tdt_ctx *ctx;
    int n_contigs, min_mapq, min_clip;
    tdt_keystore S;
    tdt_batch_io io;                          // columns + raw bytes of the host entry
    void *d_site;                             // the site launches' buffers (grows)
    size_t site_cap;
    clip_sites rows;                          // the rows of the last finish (inside d_site), n_rows of them
    size_t n_rows;
    hipEvent_t ev[2];
    double ms_sites;
};

struct ClipIn {
    const uint16_t *flag;
    const int32_t *tid, *pos;
    const uint8_t *mapq;
    const uint64_t *rec_off;
    const uint8_t *raw;
};

// the 4-bit code of query base qi of the sequence at raw[seq ...] (the even base in the high nibble)
__device__ __forceinline__ unsigned clip_base(const uint8_t *__restrict__ raw, ull seq, ull qi) {
    const unsigned v = raw[seq + (qi >> 1)];
    return (qi & 1ull) ? v & 0xfu : v >> 4;
}

__global__ __launch_bounds__(CLIP_BLOCK) void clip_keys(ClipIn I, int n, ull raw_len, unsigned min_mapq, unsigned min_clip, ull *__restrict__ k1s,
                                                        ull *__restrict__ k2s, ull cap, ull *__restrict__ st) {
    __shared__ ull s_k1[CLIP_K_TILE * TDT_CLIP_MAX_PER_READ], s_k2[CLIP_K_TILE * TDT_CLIP_MAX_PER_READ];   // the tile's keys, in the order they were made
    __shared__ int s_read[CLIP_BLOCK];
    __shared__ int s_wsum[CLIP_BLOCK / 64], s_wkeys[CLIP_BLOCK / 64];
    __shared__ ull s_cnt[CLIP_BLOCK / 64][SN_PUSH_N + 4];         // per wave: the push counters, then the OR / NAND words
    __shared__ ull s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long lo = (long long)blockIdx.x * CLIP_K_TILE, hi = lo + CLIP_K_TILE < n ? lo + CLIP_K_TILE : n;
    ull cnt[SN_PUSH_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // (short_clips, cut: this lane's; the others: wave-uniform sums of ballots)
    ull or1 = 0, nand1 = 0, or2 = 0, nand2 = 0;                   // (this lane's keys; merged over the wave at the end)
    // ---- lane = read: the filters on the columns
    const long long i = lo + t;
    bool elig = false;
    if (i < hi) elig = (I.flag[i] & 0xF04u) == 0 && I.tid[i] >= 0 && (unsigned)I.mapq[i] >= min_mapq;
    const ull m_rec = __ballot(i < hi), m_el = __ballot(elig);
    cnt[SN_RECORDS] = (ull)__popcll(m_rec);
    cnt[SN_ELIGIBLE] = (ull)__popcll(m_el);
    const tdt_slots S = tdt_block_slots<CLIP_BLOCK / 64>(m_el, s_wsum, lane, wave);
    if (elig) s_read[S.base + tdt_lane_rank(m_el, lane)] = (int)i;
    __syncthreads();
    // ---- lane = compacted read: bound the record, sum its CIGAR, take its clips
    const bool live = t < S.total;
    bool bad = live, noseq = false, noaln = false;
    unsigned nshort = 0, ncut = 0;
    bool ev[2] = {false, false};                                   // the leading clip's event, the trailing clip's
    ull eK1[2] = {0, 0}, eK2[2] = {0, 0};
    const uint8_t *__restrict__ raw = I.raw;
    if (live) {
        const int ri = s_read[t];
        const unsigned rev = ((unsigned)I.flag[ri] >> 4) & 1u;
        const int tid = I.tid[ri], pos = I.pos[ri];
        const ull ro = I.rec_off[ri];
        if (tid < CLIP_MAX_CONTIGS && pos >= 0 && TDT_REC_HEADER_INSIDE(raw_len, ro)) {
            tdt_rec R = TDT_REC_READ(raw, ro);
            const int l_seq = R.l_seq;
            R.l_seq = l_seq < 0 ? 0 : l_seq;                       // (clamped: the body's sum never sees a negative length)
            if (l_seq >= 0 && TDT_REC_FITS(R, raw_len)) {
                const uint8_t *cig = raw + R.cig();
                const unsigned nc = R.n_cig;
                ull rl = 0, ql = 0;
                bool worse = false;
                unsigned w0 = 0, w1 = 0, wy = 0, wz = 0;           // the first two words and the last two (wz the last)
                for (unsigned j = 0; j < nc; j++) {
                    const unsigned w = tdt_ld_u32(cig + 4ull * j), op = w & 0xfu, len = w >> 4;
                    worse |= op > 8;
                    rl += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? (ull)len : 0ull;
                    ql += (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ? (ull)len : 0ull;
                    if (j == 0) w0 = w;
                    if (j == 1) w1 = w;
                    wy = wz;
                    wz = w;
                }
                worse |= (ull)pos + rl > (ull)CLIP_END_LIMIT;
                worse |= l_seq >= 1 && nc >= 1 && ql != (ull)l_seq;
                bad = worse;
                if (!bad) {
                    noseq = nc == 0 || l_seq == 0;
                    noaln = !noseq && rl == 0;
                }
                if (!bad && !noseq && !noaln) {
                    // the CIGAR spans exactly l_seq bases: a leading clip is query [0, len), a trailing one [l_seq - len, l_seq)
                    const ull seq = R.seq();
                    const bool lead = (w0 & 0xfu) == 4u || ((w0 & 0xfu) == 5u && nc >= 2 && (w1 & 0xfu) == 4u);
                    const bool trail = (wz & 0xfu) == 4u || ((wz & 0xfu) == 5u && nc >= 2 && (wy & 0xfu) == 4u);
                    const unsigned llen = ((w0 & 0xfu) == 4u ? w0 : w1) >> 4, tlen = ((wz & 0xfu) == 4u ? wz : wy) >> 4;
#pragma unroll
                    for (int side = 0; side < 2; side++) {
                        const bool has = side ? trail : lead;
                        const unsigned clen = side ? tlen : llen;
                        if (!has) continue;
                        if (clen < min_clip) {
                            nshort++;
                            continue;
                        }
                        const unsigned want = clen < (unsigned)TDT_CLIP_COLS ? clen : (unsigned)TDT_CLIP_COLS;
                        const ull q0 = side ? (ull)l_seq - clen : (ull)clen - 1ull;      // column 0's query index; column j: q0 + j (R), q0 - j (L)
                        unsigned nb = 0;
                        ull bases = 0;
                        while (nb < want) {
                            const unsigned c = clip_base(raw, seq, side ? q0 + nb : q0 - nb);
                            if (__popc(c) != 1) break;
                            bases |= (ull)__builtin_ctz(c) << (2u * nb);
                            nb++;
                        }
                        ncut += nb < want;
                        ev[side] = true;
                        eK1[side] = ((ull)(unsigned)tid << 32) | (side ? (ull)pos + rl : (ull)pos + 1ull);
                        eK2[side] = ((ull)side << 63) | ((ull)nb << 58) | (bases << 2) | (ull)rev;
                    }
                }
            }
        }
    }
    cnt[SN_MALFORMED] = (ull)__popcll(__ballot(live && bad));
    cnt[SN_NO_SEQUENCE] = (ull)__popcll(__ballot(noseq));
    cnt[SN_NO_ALIGNMENT] = (ull)__popcll(__ballot(noaln));
    cnt[SN_LEFT_CLIPS] = (ull)__popcll(__ballot(ev[0]));
    cnt[SN_RIGHT_CLIPS] = (ull)__popcll(__ballot(ev[1]));
    cnt[SN_CLIPPED_READS] = (ull)__popcll(__ballot(ev[0] || ev[1]));
    cnt[SN_SHORT_CLIPS] = tdt_wave_reduce<tdt_sum>((ull)nshort);
    cnt[SN_CUT] = tdt_wave_reduce<tdt_sum>((ull)ncut);
    // ---- the tile's keys in LDS: slots by a prefix sum of the reads' event counts
    const int mine = (int)ev[0] + (int)ev[1];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) s_wkeys[wave] = incl;
    __syncthreads();
    int base = 0, nk = 0;                                          // nk: the keys of the tile (uniform over the workgroup)
#pragma unroll
    for (int w = 0; w < CLIP_BLOCK / 64; w++) {
        base += w < wave ? s_wkeys[w] : 0;
        nk += s_wkeys[w];
    }
    int slot = base + incl - mine;                                 // (+ mine <= nk <= 2 x the reads of the tile)
#pragma unroll
    for (int side = 0; side < 2; side++) {
        if (ev[side]) {
            const ull k1 = eK1[side], k2 = eK2[side];
            or1 |= k1, nand1 |= ~k1, or2 |= k2, nand2 |= ~k2;
            s_k1[slot] = k1;
            s_k2[slot] = k2;
            slot++;
        }
    }
    // ---- the tile's counters: merged per wave, then over the workgroup, ONE atomic per non-zero counter
    or1 = tdt_wave_reduce<tdt_or>(or1), nand1 = tdt_wave_reduce<tdt_or>(nand1), or2 = tdt_wave_reduce<tdt_or>(or2), nand2 = tdt_wave_reduce<tdt_or>(nand2);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SN_PUSH_N; k++) s_cnt[wave][k] = cnt[k];
        s_cnt[wave][SN_PUSH_N] = or1, s_cnt[wave][SN_PUSH_N + 1] = nand1, s_cnt[wave][SN_PUSH_N + 2] = or2, s_cnt[wave][SN_PUSH_N + 3] = nand2;
    }
    __syncthreads();
    if (t == 0) s_base = nk ? atomicAdd(&st[KS_N], (ull)nk) : 0ull;          // the workgroup's slots of the store behind ONE atomic
    if (t < SN_PUSH_N + 4) {
        ull v = 0;
        for (int w = 0; w < CLIP_BLOCK / 64; w++) v = t < SN_PUSH_N ? v + s_cnt[w][t] : v | s_cnt[w][t];
        if (v) {
            if (t < SN_PUSH_N) atomicAdd(&st[t], v);
            else atomicOr(&st[ST_OR1 + (t - SN_PUSH_N)], v);
        }
    }
    __syncthreads();
    for (int k = t; k < nk; k += CLIP_BLOCK) {                     // (consecutive lanes, consecutive slots)
        const ull at = s_base + (ull)k;
        if (at < cap) {
            k1s[at] = s_k1[k];
            k2s[at] = s_k2[k];
        } else {
            st[KS_OVERFLOW] = 1;                                   // (cannot happen: the host reserved 2 slots for every read of the batch)
        }
    }
}

// ---- the sites of the finish's rows (a = K1, b = K2 with bit 0 clear, ascending by (K1, K2); n rows)
__device__ __forceinline__ bool clip_head(const ull *__restrict__ a, const ull *__restrict__ b, int i) {
    return i == 0 || a[i] != a[i - 1] || (b[i] >> 63) != (b[i - 1] >> 63);
}

// WRITE false: tile_n[tile] = the site heads of the tile, out[0] += them.  WRITE true: tile_n holds the exclusive sums and the heads'
// row indices are written to start[], in row order.
template <bool WRITE>
__global__ __launch_bounds__(KS_BLOCK) void clip_heads(const ull *__restrict__ a, const ull *__restrict__ b, int n, int *__restrict__ tile_n,
                                                       ull *__restrict__ out, int *__restrict__ start) {
    __shared__ int s_w[KS_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int t0 = blockIdx.x * KS_TILE;
    const int row0 = WRITE ? tile_n[blockIdx.x] : 0;
    int kept = 0;                                                  // (uniform over the workgroup)
    for (int r = 0; r < KS_TILE / KS_BLOCK; r++) {                 // (uniform: every thread takes every round)
        const int i = t0 + r * KS_BLOCK + t;
        const bool head = i < n && clip_head(a, b, i);
        const ull m = __ballot(head);
        const tdt_slots S = tdt_block_slots<KS_BLOCK / 64>(m, s_w, lane, wave);
        if (WRITE && head) start[row0 + kept + S.base + tdt_lane_rank(m, lane)] = i;       // (< n: a head per site, a site per row at most)
        kept += S.total;
        __syncthreads();                                           // (s_w is the next round's)
    }
    if (!WRITE && t == 0) {
        tile_n[blockIdx.x] = kept;
        if (kept) atomicAdd(&out[0], (ull)kept);
    }
}

// one wavefront per site, grid-strided; n_sites = *out (what clip_heads<false> counted)
__global__ __launch_bounds__(CLIP_VOTE_BLOCK) void clip_vote(const ull *__restrict__ a, const ull *__restrict__ b, const unsigned *__restrict__ r_sup,
                                                             const unsigned *__restrict__ r_rev, int n, const int *__restrict__ start,
                                                             const ull *__restrict__ out, unsigned min_support, clip_sites V) {
    __shared__ unsigned s_votes[TDT_CLIP_COLS * 4];
    const int lane = threadIdx.x;
    const int n_sites = (int)out[0];                               // (<= n < 2^30)
    for (int s = blockIdx.x; s < n_sites; s += gridDim.x) {        // (uniform over the workgroup = the wave)
        const int lo = start[s], hi = s + 1 < n_sites ? start[s + 1] : n;
        for (int k = lane; k < TDT_CLIP_COLS * 4; k += CLIP_VOTE_BLOCK) s_votes[k] = 0;
        __syncthreads();
        unsigned sup = 0, rev = 0, seqs = 0;
        for (int r = lo + lane; r < hi; r += CLIP_VOTE_BLOCK) {    // (strided: a site of any size costs its rows / 64 steps)
            const ull k2 = b[r];
            const unsigned c = r_sup[r], nb = (unsigned)(k2 >> 58) & 31u;
            sup += c, rev += r_rev[r], seqs++;
            for (unsigned j = 0; j < nb && j < (unsigned)TDT_CLIP_COLS; j++) atomicAdd(&s_votes[4 * j + ((unsigned)(k2 >> (2u + 2u * j)) & 3u)], c);
        }
        __syncthreads();
        sup = tdt_wave_reduce<tdt_sum>(sup), rev = tdt_wave_reduce<tdt_sum>(rev), seqs = tdt_wave_reduce<tdt_sum>(seqs);
        unsigned depth = 0, win = 0, best = 0;
        if (lane < TDT_CLIP_COLS) {
#pragma unroll
            for (unsigned c = 0; c < 4; c++) {
                const unsigned v = s_votes[4 * lane + c];
                depth += v;
                if (v > best) best = v, win = c;                   // (a tie stays with the smaller code)
            }
        }
        const ull m_in = __ballot(lane < TDT_CLIP_COLS && depth >= min_support);
        const unsigned clen = (unsigned)__builtin_ctzll(~m_in);    // the leading columns deep enough (bits 28 ... 63 of m_in are clear)
        const bool in = (unsigned)lane < clen;
        const ull cons = tdt_wave_reduce<tdt_or>(in ? (ull)win << (2 * (lane & 31)) : 0ull);
        const ull agree = tdt_wave_reduce<tdt_sum>(in ? (ull)best : 0ull), total = tdt_wave_reduce<tdt_sum>(in ? (ull)depth : 0ull);
        if (lane == 0) {
            V.k1[s] = a[lo];
            V.side[s] = (unsigned)(b[lo] >> 63);
            V.sup[s] = sup, V.rev[s] = rev, V.seqs[s] = seqs, V.clen[s] = clen;
            V.cons[s] = cons, V.agree[s] = agree, V.total[s] = total;
        }
        __syncthreads();                                           // (the table is cleared for the next site behind its last reader)
    }
}

// WRITE false: tile_n[tile] = the sites of the tile with SUPPORT >= min_support, out[1] += them.  WRITE true: tile_n holds the exclusive
// sums and those sites become rows, in key order.  (tiles of sites: ntiles covers the rows, of which there are at least as many)
template <bool WRITE>
__global__ __launch_bounds__(KS_BLOCK) void clip_keep(clip_sites V, const ull *__restrict__ n_sites_, unsigned min_support, int *__restrict__ tile_n,
                                                      ull *__restrict__ out, clip_sites W) {
    __shared__ int s_w[KS_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = (int)n_sites_[0];
    const int t0 = blockIdx.x * KS_TILE;
    const int row0 = WRITE ? tile_n[blockIdx.x] : 0;
    int kept = 0;                                                  // (uniform over the workgroup)
    for (int r = 0; r < KS_TILE / KS_BLOCK; r++) {                 // (uniform: every thread takes every round)
        const int i = t0 + r * KS_BLOCK + t;
        const bool keep = i < n && V.sup[i] >= min_support;
        const ull m = __ballot(keep);
        const tdt_slots S = tdt_block_slots<KS_BLOCK / 64>(m, s_w, lane, wave);
        if (WRITE && keep) {
            const size_t row = (size_t)row0 + (size_t)(kept + S.base + tdt_lane_rank(m, lane));        // (<= i: a row per kept site)
            W.k1[row] = V.k1[i], W.side[row] = V.side[i], W.sup[row] = V.sup[i], W.rev[row] = V.rev[i], W.seqs[row] = V.seqs[i];
            W.clen[row] = V.clen[i], W.cons[row] = V.cons[i], W.agree[row] = V.agree[i], W.total[row] = V.total[i];
        }
        kept += S.total;
        __syncthreads();                                           // (s_w is the next round's)
    }
    if (!WRITE && t == 0) {
        tile_n[blockIdx.x] = kept;
        if (kept) atomicAdd(&out[1], (ull)kept);
    }
}

static void clip_free(tdt_clip *h) {
    ks_free(&h->S);
    if (h->io.d) (void)hipFree(h->io.d);
    if (h->d_site) (void)hipFree(h->d_site);
    for (int k = 0; k < 2; k++)
        if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
    delete h;
}

extern "C" size_t tdt_clip_sn_size(void) { return TDT_CLIP_SN_N; }

extern "C" int tdt_clip_create(tdt_ctx *ctx, int n_contigs, int min_mapq, int min_clip, size_t capacity, tdt_clip **out) {
    if (!ctx || !out || n_contigs < 0) {
        tdt_set_error("tdt_clip_create: bad argument");
        return TDT_E_ARG;
    }
    if (n_contigs > CLIP_MAX_CONTIGS || min_mapq < 0 || min_mapq > 255 || min_clip < 1 || min_clip > TDT_CLIP_MAX_CLIP || capacity >= (1ull << 40)) {
        tdt_set_error("tdt_clip_create: %d contigs (at most 2^24), min_mapq %d (0 ... 255), min_clip %d (1 ... %d), capacity %zu", n_contigs, min_mapq,
                      min_clip, TDT_CLIP_MAX_CLIP, capacity);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_clip *h = new tdt_clip{};
    h->ctx = ctx;
    h->n_contigs = n_contigs;
    h->min_mapq = min_mapq;
    h->min_clip = min_clip;
    int rc = ks_init(&h->S, ctx, "tdt_clip", ST_OR1, capacity);
    if (rc == TDT_OK) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreate(&h->ev[k]);
        if (e != hipSuccess) {
            tdt_set_error("tdt_clip_create: %s", hipGetErrorString(e));
            rc = TDT_E_HIP;
        }
    }
    if (rc) {
        clip_free(h);
        return rc;
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_clip_destroy(tdt_clip *h) {
    if (!h) return TDT_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);        // (no kernel of the stream still writes the store)
    clip_free(h);
    return TDT_OK;
}

extern "C" int tdt_clip_reset(tdt_clip *h) {
    if (!h) {
        tdt_set_error("tdt_clip_reset: bad argument");
        return TDT_E_ARG;
    }
    h->n_rows = 0;
    return ks_reset(&h->S);
}

static int clip_launch(tdt_clip *h, const ClipIn &I, size_t n, size_t raw_len) {
    const size_t room = n * TDT_CLIP_MAX_PER_READ;                 // the bound two clips per read give
    int rc = ks_reserve(&h->S, room);
    if (rc) return rc;
    const dim3 grid((unsigned)((n + CLIP_K_TILE - 1) / CLIP_K_TILE));
    hipLaunchKernelGGL(clip_keys, grid, dim3(CLIP_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, (unsigned)h->min_clip, h->S.k1,
                       h->S.k2, (ull)h->S.cap, h->S.d_state);
    TDT_CHECK_LAUNCH();
    h->S.upper += room;
    h->S.rows_valid = false;
    h->n_rows = 0;
    return TDT_OK;
}

#define CLIP_NEED (TDT_NEED(FLAG) | TDT_NEED(TID) | TDT_NEED(POS) | TDT_NEED(MAPQ) | TDT_NEED(REC_OFF) | TDT_NEED(RAW))

// One batch of the device ingest: d_arrays14 = the pointer table tdt_ingest_arrays filled (TDT_COL_*: a host array of TDT_NCOL device
// pointers).  The launch is enqueued on the context's stream and nothing is waited for — unless the reserve must ask or grow.
extern "C" int tdt_clip_push_device(tdt_clip *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    tdt_batch B;
    const int rc = tdt_batch_view("tdt_clip_push_device", h, d_arrays14, n, raw_len, CLIP_NEED, &B);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    return clip_launch(h, ClipIn{B.flag, B.tid, B.pos, B.mapq, B.rec_off, B.raw}, n, raw_len);
}

// The same kernel on host columns and host record bytes (uploaded into the handle's own block).  The stream is synchronised before the
// return: the caller's arrays are free again.
extern "C" int tdt_clip_push(tdt_clip *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off, size_t n,
                             const uint8_t *raw, size_t raw_len) {
    tdt_batch H{}, B;
    H.flag = flag, H.tid = tid, H.pos = pos, H.mapq = mapq, H.rec_off = rec_off, H.raw = raw;
    int rc = tdt_batch_host("tdt_clip_push", h, H, n, raw_len, CLIP_NEED);
    if (rc == TDT_OK) rc = tdt_batch_offsets_ascend("tdt_clip_push", rec_off, n);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    rc = tdt_batch_upload("tdt_clip_push", h->ctx, &h->io, H, CLIP_NEED, n, raw_len, &B);
    if (rc == TDT_OK) rc = clip_launch(h, ClipIn{B.flag, B.tid, B.pos, B.mapq, B.rec_off, B.raw}, n, raw_len);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

extern "C" int tdt_clip_keys(tdt_clip *h, uint64_t *k1, uint64_t *k2, size_t *n) { return ks_keys(h ? &h->S : nullptr, "tdt_clip", k1, k2, n); }

struct clip_work {
    clip_sites V, W;
    int *start, *tile_heads, *tile_kept;
    ull *d_out;                                   // [0] the sites, [1] the kept ones
    size_t lay(void *base, size_t n, size_t ntiles) {
        tdt_carver cv(base);
        V.lay(cv, n), W.lay(cv, n);
        start = cv.take<int>(n), tile_heads = cv.take<int>(ntiles), tile_kept = cv.take<int>(ntiles), d_out = cv.take<ull>(2);
        return cv.size;
    }
};

// the site launches over the n rows of the keystore's last finish -> got[0] = the sites, got[1] = those with SUPPORT >= min_support
static int clip_sites_of_rows(tdt_clip *h, size_t n_, unsigned min_support, ull *got) {
    tdt_ctx *ctx = h->ctx;
    got[0] = got[1] = 0;
    h->ms_sites = 0;
    h->n_rows = 0;
    if (!n_) return TDT_OK;
    const int n = (int)n_;                                         // (< 2^30: ks_finish refused more)
    const size_t ntiles = (n_ + KS_TILE - 1) / KS_TILE;
    clip_work K;
    const size_t bytes = K.lay(nullptr, n_, ntiles);
    if (bytes > h->site_cap) {
        if (h->d_site) TDT_HIP(hipFree(h->d_site));
        h->d_site = nullptr;
        h->site_cap = 0;
        if (tdt_dev_malloc(&h->d_site, bytes) != hipSuccess) {
            tdt_set_error("tdt_clip_finish: out of device memory (%zu rows)", n_);
            return TDT_E_NOMEM;
        }
        h->site_cap = bytes;
    }
    K.lay(h->d_site, n_, ntiles);
    hipStream_t st = ctx->stream;
    const ull *a = h->S.r_k1, *b = h->S.r_k2;
    const int nt = (int)ntiles;
    const unsigned vgrid = n_ < CLIP_VOTE_GRID ? (unsigned)n_ : CLIP_VOTE_GRID;
    TDT_HIP(hipMemsetAsync(K.d_out, 0, 2 * 8, st));
    TDT_HIP(hipEventRecord(h->ev[0], st));
    hipLaunchKernelGGL(clip_heads<false>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, a, b, n, K.tile_heads, K.d_out, K.start);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ks_carry_sum, dim3(1), dim3(KS_BLOCK), 0, st, K.tile_heads, nt);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_heads<true>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, a, b, n, K.tile_heads, K.d_out, K.start);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_vote, dim3(vgrid), dim3(CLIP_VOTE_BLOCK), 0, st, a, b, (const unsigned *)h->S.r_sup, (const unsigned *)h->S.r_rev, n,
                       (const int *)K.start, (const ull *)K.d_out, min_support, K.V);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_keep<false>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, K.V, (const ull *)K.d_out, min_support, K.tile_kept, K.d_out, K.W);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ks_carry_sum, dim3(1), dim3(KS_BLOCK), 0, st, K.tile_kept, nt);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_keep<true>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, K.V, (const ull *)K.d_out, min_support, K.tile_kept, K.d_out, K.W);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipEventRecord(h->ev[1], st));
    TDT_HIP(hipMemcpyAsync(got, K.d_out, 2 * 8, hipMemcpyDeviceToHost, st));
    const int rc = tdt_ctx_sync(ctx);
    if (rc) return rc;
    float ms = 0;
    TDT_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms_sites = ms;
    h->rows = K.W;
    h->n_rows = (size_t)got[1];
    return TDT_OK;
}

// sn_out: uint64[TDT_CLIP_SN_N], the push counters and the sequences and sites of everything pushed so far; *n_rows: the rows
// tdt_clip_rows will give.  The store is left as it was.
extern "C" int tdt_clip_finish(tdt_clip *h, uint64_t min_support, uint64_t *sn_out, size_t *n_rows) {
    if (!h || !sn_out || !n_rows) {
        tdt_set_error("tdt_clip_finish: bad argument");
        return TDT_E_ARG;
    }
    if (min_support < 1 || min_support > TDT_CLIP_MAX_SUPPORT) {
        tdt_set_error("tdt_clip_finish: min_support %llu (1 ... %d)", (ull)min_support, TDT_CLIP_MAX_SUPPORT);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    ull state[KS_WORDS], seqs[2], sites[2];
    int rc = ks_stored(&h->S, state);
    if (rc == TDT_OK) rc = ks_finish(&h->S, state, 1, seqs);       // (a minimum support of 1: every distinct sequence is a row)
    if (rc == TDT_OK) {
        rc = clip_sites_of_rows(h, h->S.n_rows, (unsigned)min_support, sites);
        if (rc) h->S.rows_valid = false;
    }
    if (rc) return rc;
    uint64_t res[SN_N] = {};
    for (int k = 0; k < SN_PUSH_N; k++) res[k] = state[k];
    res[SN_DISTINCT_SEQS] = seqs[0];
    res[SN_DISTINCT_SITES] = sites[0];
    res[SN_REPORTED] = sites[1];
    memcpy(sn_out, res, sizeof res);
    *n_rows = h->n_rows;
    return TDT_OK;
}

// The rows of the last finish, ascending by (K1, side).  *n in: the room of the nine arrays (ignored when all nine are NULL), out: the
// rows.  A push or a reset since the finish: TDT_E_ARG.  Too little room: TDT_E_RANGE, nothing written.
extern "C" int tdt_clip_rows(tdt_clip *h, uint64_t *k1, uint32_t *side, uint32_t *support, uint32_t *rev, uint32_t *seqs, uint32_t *clen, uint64_t *consensus,
                             uint64_t *agree, uint64_t *total, size_t *n) {
    const bool any = k1 || side || support || rev || seqs || clen || consensus || agree || total;
    if (!h || !n || (any && !(k1 && side && support && rev && seqs && clen && consensus && agree && total))) {
        tdt_set_error("tdt_clip_rows: bad argument");
        return TDT_E_ARG;
    }
    if (!h->S.rows_valid) {
        tdt_set_error("tdt_clip_rows: no finish since the last push or reset");
        return TDT_E_ARG;
    }
    const size_t have = h->n_rows;
    if (any) {
        if (*n < have) {
            tdt_set_error("tdt_clip_rows: room for %zu rows, %zu kept", *n, have);
            return TDT_E_RANGE;
        }
        if (have) {
            TDT_HIP(hipSetDevice(h->ctx->device));
            hipStream_t st = h->ctx->stream;
            const clip_sites &W = h->rows;
            TDT_HIP(hipMemcpyAsync(k1, W.k1, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(side, W.side, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(support, W.sup, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(rev, W.rev, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(seqs, W.seqs, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(clen, W.clen, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(consensus, W.cons, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(agree, W.agree, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(total, W.total, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
        }
    }
    *n = have;
    return TDT_OK;
}

// device milliseconds of the last finish: [0] sort by K2, [1] gather of K1, [2] sort by K1, [3] gather of K2 + the run-length launches,
// [4] the site launches (heads, vote, rows)
extern "C" int tdt_clip_timing(tdt_clip *h, double *ms5) {
    if (!h || !ms5) {
        tdt_set_error("tdt_clip_timing: bad argument");
        return TDT_E_ARG;
    }
    for (int k = 0; k < 4; k++) ms5[k] = h->S.ms[k];
    ms5[4] = h->ms_sites;
    return TDT_OK;
}

// out3: how often the reserve asked the device for the real count, how often it made a bigger store, the store's capacity now
extern "C" int tdt_clip_reserve_stats(tdt_clip *h, uint64_t *out3) {
    if (!h || !out3) {
        tdt_set_error("tdt_clip_reserve_stats: bad argument");
        return TDT_E_ARG;
    }
    out3[0] = h->S.asks, out3[1] = h->S.grows, out3[2] = h->S.cap;
    return TDT_OK;
}
