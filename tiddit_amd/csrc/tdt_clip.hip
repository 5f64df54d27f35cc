// Clipped-read breakpoint sites for gfx950 — every reference position where eligible reads of the --sv scan are soft-clipped on one
// side (TIDDIT_CLIPS), with the support by strand and a consensus of the clipped bases beside the breakpoint.  The definition is
// tiddit_clips.py's: per clip of at least min_clip bases K1 = tid << 32 | P (1-based; the first aligned base for a leading clip, the
// last for a trailing one) and K2 = side << 63 | n << 58 | bases << 2 | rev, `bases` = the first n <= 28 clipped bases outward from the
// breakpoint, two bits each; equal (K1, K2 >> 1) is one distinct sequence, equal (K1, side) one site.  Every result is an
// order-independent integer, so it equals the definition exactly.
//   * clip_keys — ONE launch per batch, on the columns and record bytes that are already resident, enqueued beside snv_keys and waiting
//     for nothing.  The read gate (ks_read_gate), the record open (KS_OPEN) and the key emit (ks_stage, ks_flush) are tdt_keystore.h's,
//     shared with indel_keys and snv_keys.  Behind the gate lane = compacted read: ONE pass over the CIGAR (tdt_cig_span_of<true>,
//     tdt_bam_record.h) sums its reference and query lengths, looks for an op code above 8 and keeps the first two and the last two
//     words, which decide the clips; up to 28 nibbles per clip are read byte by byte from the sequence (tdt_rec_base; a leading clip
//     is walked backwards from its last base, a trailing one forwards from its first, so both nibble phases occur on both sides), and
//     the walk stops at the first code that is not A C G T.  At most two keys per read are staged in LDS (256 reads x 2 keys x 16 B =
//     8 KB) and flushed once.
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
//   * clip_ext_keys — ONE more launch per batch, only on a handle with tdt_clip_ext_enable (TIDDIT_CLIPS_INS), enqueued beside clip_keys
//     and waiting for nothing: the same gate, open and CIGAR pass; for a clip of which more than 28 bases are kept it emits one key per
//     further chunk c = 1 ... 4 of 28 columns, K1 = c << 56 | tid << 32 | P (the tid has 24 bits, the top byte is free) and K2 in
//     clip_keys' layout, into a SECOND key store of the handle, whose reserve, growth and ask-the-device policy are the first one's.
//     At most TDT_CLIP_EXT_MAX_PER_READ = 8 keys per read, staged in LDS: 256 reads x 8 keys x 16 B = 32 KB (34 056 B with the gate's
//     and the flush's words).  That is four workgroups (16 waves) per CU by LDS, half of clip_keys'; a tile of 128 reads would halve
//     the LDS and double the workgroups and their flush atomics for the same waves per CU, and most lanes of this kernel leave at
//     the clip-length test before a base is read, so the tile stays one round of 256.  Malformed, no-sequence and no-alignment reads emit nothing here and are not counted again.
//     With the chunk in K1 a "site" of that store is a (chunk, site), and the finish above — ks_finish with support 1, clip_heads,
//     clip_vote, clip_keep with S — gives each chunk's SUPPORT, CLEN and packed consensus with no new vote kernel
//     (clip_sites_of_rows takes the store and the buffers as arguments).  The gather of the chunks into an extended consensus, the
//     pairing of facing sites and the closure are csrc/tdt_clip_ins.hip's.
#include <vector>

#include "tdt_clip_align.h"
#include "tdt_clip_far.h"
#include "tdt_clip_ins.h"
#include "tdt_swalign.h"
#include "tdt_keystore.h"

typedef unsigned long long ull;

#define CLIP_BLOCK 256
#define CLIP_K_TILE 256                       // reads of a clip_keys workgroup (one round); it stages at most 2 x that many keys in LDS (8 KB)
#define CLIP_VOTE_BLOCK 64                    // one wavefront per site
#define CLIP_VOTE_GRID 4096                   // workgroups of clip_vote at most (grid-strided over the sites)

static_assert(CLIP_K_TILE == CLIP_BLOCK, "one round per workgroup");
static_assert(TDT_CLIP_MAX_PER_READ == 2, "a leading and a trailing clip");
static_assert(TDT_CLIP_COLS == 28 && TDT_CLIP_COLS <= CLIP_VOTE_BLOCK, "56 bits of bases in K2; a lane per column");
static_assert(CLIP_VOTE_BLOCK == 64, "clip_vote's workgroup is one wavefront");
static_assert(TDT_CLIP_EXT_COLS == 5 * TDT_CLIP_COLS && TDT_CLIP_EXT_MAX_PER_READ == 2 * 4, "four further chunks of 28 columns per clip");

// the SN rows, in the order of the file; the first ten are the push's
enum { SN_RECORDS = 0, SN_ELIGIBLE, SN_MALFORMED, SN_NO_SEQUENCE, SN_NO_ALIGNMENT, SN_SHORT_CLIPS, SN_LEFT_CLIPS, SN_RIGHT_CLIPS, SN_CLIPPED_READS,
       SN_CUT, SN_DISTINCT_SEQS, SN_DISTINCT_SITES, SN_REPORTED, SN_N, SN_PUSH_N = SN_DISTINCT_SEQS };
static_assert(SN_N == TDT_CLIP_SN_N, "SN rows");
enum { ST_OR1 = SN_PUSH_N };                  // OR1, NAND1, OR2, NAND2 behind the push counters; KS_N, KS_OVERFLOW: tdt_keystore.h
static_assert(ST_OR1 + 4 <= KS_N, "state layout");
// the push counters of the extension store: the events with a key by side, the clips cut at another base at or beyond column 28
enum { XN_LEFT = 0, XN_RIGHT, XN_CUT, XN_PUSH_N, XT_OR1 = XN_PUSH_N };

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
    void *d_align;                            // tdt_clip_align's five columns and counters (grows)
    size_t align_cap;
    ca_out align;                             // ... of the last tdt_clip_align (inside d_align), n_rows of them; valid while the rows are
    bool align_valid;
    double ms_align;
    void *d_far;                              // tdt_clip_far's six columns, counters and workspace (grows)
    size_t far_cap;
    far_out far;                              // ... of the last tdt_clip_far (inside d_far), n_rows of them; valid while the rows are
    bool far_valid;
    double ms_far[4];
    hipEvent_t ev_far[5];                     // made by the first tdt_clip_far
    // ---- TIDDIT_CLIPS_INS: nothing below is allocated without tdt_clip_ext_enable
    bool ext;
    tdt_keystore X;                           // the extension keys (chunk << 56 | K1, K2)
    void *d_xsite;                            // the site launches' buffers over X's rows (grows)
    size_t xsite_cap;
    clip_sites xrows;                         // the (chunk, site) rows of the last tdt_clip_ins (inside d_xsite), n_xrows of them
    size_t n_xrows;
    double ms_xsites;
    unsigned last_support;                    // the minimum support of the last tdt_clip_finish
    void *d_ins;                              // ECLEN and the five words per row, the pair stage's workspace and counters (grows)
    size_t ins_cap;
    unsigned *ext_eclen;                      // ... of the last tdt_clip_ins (inside d_ins), n_rows of them; valid while the rows are
    ull *ext_cons5;
    void *d_pairs;                            // the pair rows (grows)
    size_t pairs_cap;
    ins_out pairs;                            // ... of the last tdt_clip_ins (inside d_pairs), n_pairs of them
    size_t n_pairs;
    bool ins_valid;
    double ms_ins[3];
    hipEvent_t ev_ins[4];                     // made by tdt_clip_ext_enable
    // ---- TIDDIT_CLIPS_MEI: nothing below is allocated without tdt_clip_mei
    void *d_mei;                              // the query table, the result columns, the offsets and the counters (grows)
    size_t mei_cap;
    sw_table mei_q;                           // ... of the last tdt_clip_mei (inside d_mei), n_mei of them; valid while the pairs are
    sw_out mei_out;
    size_t n_mei;
    bool mei_valid;
    double ms_mei[3];
    hipEvent_t ev_mei[4];                     // made by the first tdt_clip_mei
};

__global__ __launch_bounds__(CLIP_BLOCK) void clip_keys(ks_cols I, int n, ull raw_len, unsigned min_mapq, unsigned min_clip, ull *__restrict__ k1s,
                                                        ull *__restrict__ k2s, ull cap, ull *__restrict__ st) {
    __shared__ ull s_k1[CLIP_K_TILE * TDT_CLIP_MAX_PER_READ], s_k2[CLIP_K_TILE * TDT_CLIP_MAX_PER_READ];   // the tile's keys, in the order they were made
    const long long lo = (long long)blockIdx.x * CLIP_K_TILE, hi = lo + CLIP_K_TILE < n ? lo + CLIP_K_TILE : n;
    ull cnt[SN_PUSH_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // (short_clips, cut: this lane's; the others: wave-uniform sums of ballots)
    // ---- lane = read: the filters on the columns; then lane = compacted read
    const ks_gated G = ks_read_gate<CLIP_BLOCK>(I, lo, hi, min_mapq, cnt[SN_RECORDS], cnt[SN_ELIGIBLE]);
    const bool live = (int)threadIdx.x < G.live;
    bool bad = live, noseq = false, noaln = false;
    unsigned nshort = 0, ncut = 0;
    bool ev[2] = {false, false};                                   // the leading clip's event, the trailing clip's
    ull eK1[2] = {0, 0}, eK2[2] = {0, 0};
    ks_read A{};
    const uint8_t *__restrict__ raw = I.raw;
    if (live && KS_OPEN(A, I, G.read, raw_len)) {
        // ---- the record is bounded: sum its CIGAR, take its clips
        const tdt_rec &R = A.R;
        const int tid = A.tid, pos = A.pos, l_seq = R.l_seq;
        const unsigned nc = R.n_cig;
        const tdt_cig_span C = tdt_cig_span_of<true>(raw + R.cig(), nc);
        const unsigned w0 = C.w0, w1 = C.w1, wy = C.wy, wz = C.wz;  // the first two words and the last two (wz the last)
        const ull rl = C.ref_len;
        bad = C.malformed(pos, l_seq, nc);
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
                    const unsigned c = tdt_rec_base(raw, seq, side ? q0 + nb : q0 - nb);
                    if (__popc(c) != 1) break;
                    bases |= (ull)__builtin_ctz(c) << (2u * nb);
                    nb++;
                }
                ncut += nb < want;
                ev[side] = true;
                eK1[side] = ((ull)(unsigned)tid << 32) | (side ? (ull)pos + rl : (ull)pos + 1ull);
                eK2[side] = ((ull)side << 63) | ((ull)nb << 58) | (bases << 2) | (ull)A.rev;
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
    // ---- the tile's keys in LDS, then the emit (tdt_keystore.h)
    int nk;                                                        // the keys of the tile (uniform over the workgroup)
    int slot = ks_stage<CLIP_BLOCK>((int)ev[0] + (int)ev[1], &nk);        // (+ mine <= nk <= 2 x the reads of the tile)
    ks_masks M;
#pragma unroll
    for (int side = 0; side < 2; side++) {
        if (ev[side]) {
            M.add(eK1[side], eK2[side]);
            s_k1[slot] = eK1[side];
            s_k2[slot] = eK2[side];
            slot++;
        }
    }
    ks_flush<CLIP_BLOCK, SN_PUSH_N>(cnt, M, nk, s_k1, s_k2, k1s, k2s, cap, st);
}

// The extension keys of a batch (see the head of this file).  The gate counts nothing here (records and eligible are clip_keys'), and
// a read that clip_keys calls malformed, without sequence or without alignment is passed over.
__global__ __launch_bounds__(CLIP_BLOCK) void clip_ext_keys(ks_cols I, int n, ull raw_len, unsigned min_mapq, unsigned min_clip, ull *__restrict__ k1s,
                                                            ull *__restrict__ k2s, ull cap, ull *__restrict__ st) {
    __shared__ ull s_k1[CLIP_K_TILE * TDT_CLIP_EXT_MAX_PER_READ], s_k2[CLIP_K_TILE * TDT_CLIP_EXT_MAX_PER_READ];      // 2 x 16 KB
    const long long lo = (long long)blockIdx.x * CLIP_K_TILE, hi = lo + CLIP_K_TILE < n ? lo + CLIP_K_TILE : n;
    ull cnt[XN_PUSH_N] = {0, 0, 0};
    ull records = 0, eligible = 0;                                 // (not counted again)
    const ks_gated G = ks_read_gate<CLIP_BLOCK>(I, lo, hi, min_mapq, records, eligible);
    const bool live = (int)threadIdx.x < G.live;
    unsigned ncut = 0;
    int nE[2] = {0, 0};                                            // the chunks 1 ... nE[side] of a clip have a key
    ull eK1[2] = {0, 0}, eK2[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    ks_read A{};
    const uint8_t *__restrict__ raw = I.raw;
    if (live && KS_OPEN(A, I, G.read, raw_len)) {
        const tdt_rec &R = A.R;
        const int pos = A.pos, l_seq = R.l_seq;
        const unsigned nc = R.n_cig;
        const tdt_cig_span C = tdt_cig_span_of<true>(raw + R.cig(), nc);
        const unsigned w0 = C.w0, w1 = C.w1, wy = C.wy, wz = C.wz;
        const ull rl = C.ref_len;
        if (!C.malformed(pos, l_seq, nc) && nc != 0 && l_seq != 0 && rl != 0) {
            const ull seq = R.seq();
            const bool lead = (w0 & 0xfu) == 4u || ((w0 & 0xfu) == 5u && nc >= 2 && (w1 & 0xfu) == 4u);
            const bool trail = (wz & 0xfu) == 4u || ((wz & 0xfu) == 5u && nc >= 2 && (wy & 0xfu) == 4u);
            const unsigned llen = ((w0 & 0xfu) == 4u ? w0 : w1) >> 4, tlen = ((wz & 0xfu) == 4u ? wz : wy) >> 4;
#pragma unroll
            for (int side = 0; side < 2; side++) {
                const bool has = side ? trail : lead;
                const unsigned clen = side ? tlen : llen;
                if (!has || clen < min_clip || clen <= (unsigned)TDT_CLIP_COLS) continue;       // (no column beyond the 28 of clip_keys)
                const unsigned want = clen < (unsigned)TDT_CLIP_EXT_COLS ? clen : (unsigned)TDT_CLIP_EXT_COLS;
                const ull q0 = side ? (ull)l_seq - clen : (ull)clen - 1ull;      // column j: q0 + j (R), q0 - j (L), as in clip_keys
                unsigned nb = 0;                                   // the columns kept so far
                while (nb < (unsigned)TDT_CLIP_COLS && __popc(tdt_rec_base(raw, seq, side ? q0 + nb : q0 - nb)) == 1) nb++;
                bool full = nb == (unsigned)TDT_CLIP_COLS;         // the chunk in front was full
#pragma unroll
                for (int c = 1; c <= 4; c++) {
                    if (!full) break;
                    const unsigned at = (unsigned)(TDT_CLIP_COLS * c), lim = want > at ? (want - at < (unsigned)TDT_CLIP_COLS ? want - at : (unsigned)TDT_CLIP_COLS) : 0u;
                    unsigned k = 0;
                    ull bases = 0;
                    while (k < lim) {
                        const unsigned code = tdt_rec_base(raw, seq, side ? q0 + at + k : q0 - at - k);
                        if (__popc(code) != 1) break;
                        bases |= (ull)__builtin_ctz(code) << (2u * k);
                        k++;
                    }
                    nb += k;
                    full = k == (unsigned)TDT_CLIP_COLS;
                    if (k) {
                        eK2[side][c - 1] = ((ull)side << 63) | ((ull)k << 58) | (bases << 2) | (ull)A.rev;
                        nE[side] = c;
                    }
                }
                ncut += nb >= (unsigned)TDT_CLIP_COLS && nb < want;
                eK1[side] = ((ull)(unsigned)A.tid << 32) | (side ? (ull)pos + rl : (ull)pos + 1ull);
            }
        }
    }
    cnt[XN_LEFT] = (ull)__popcll(__ballot(nE[0] > 0));
    cnt[XN_RIGHT] = (ull)__popcll(__ballot(nE[1] > 0));
    cnt[XN_CUT] = tdt_wave_reduce<tdt_sum>((ull)ncut);
    int nk;                                                        // the keys of the tile (uniform over the workgroup)
    int slot = ks_stage<CLIP_BLOCK>(nE[0] + nE[1], &nk);           // (+ mine <= nk <= 8 x the reads of the tile)
    ks_masks M;
#pragma unroll
    for (int side = 0; side < 2; side++) {
#pragma unroll
        for (int c = 1; c <= 4; c++) {
            if (c <= nE[side]) {
                const ull k1 = ((ull)c << 56) | eK1[side];
                M.add(k1, eK2[side][c - 1]);
                s_k1[slot] = k1;
                s_k2[slot] = eK2[side][c - 1];
                slot++;
            }
        }
    }
    ks_flush<CLIP_BLOCK, XN_PUSH_N>(cnt, M, nk, s_k1, s_k2, k1s, k2s, cap, st);
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
    if (h->d_align) (void)hipFree(h->d_align);
    if (h->d_far) (void)hipFree(h->d_far);
    if (h->ext) ks_free(&h->X);
    if (h->d_xsite) (void)hipFree(h->d_xsite);
    if (h->d_ins) (void)hipFree(h->d_ins);
    if (h->d_mei) (void)hipFree(h->d_mei);
    for (int k = 0; k < 4; k++)
        if (h->ev_mei[k]) (void)hipEventDestroy(h->ev_mei[k]);
    if (h->d_pairs) (void)hipFree(h->d_pairs);
    for (int k = 0; k < 4; k++)
        if (h->ev_ins[k]) (void)hipEventDestroy(h->ev_ins[k]);
    for (int k = 0; k < 5; k++)
        if (h->ev_far[k]) (void)hipEventDestroy(h->ev_far[k]);
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
    if (!ks_create_in_range(n_contigs, min_mapq, capacity) || min_clip < 1 || min_clip > TDT_CLIP_MAX_CLIP) {
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

extern "C" int tdt_clip_destroy(tdt_clip *h) { return ks_destroy(h, clip_free); }

extern "C" int tdt_clip_reset(tdt_clip *h) {
    if (h) h->n_rows = 0, h->align_valid = h->far_valid = h->ins_valid = h->mei_valid = false;
    if (h && h->ext) {
        const int rc = ks_reset(&h->X);
        if (rc) return rc;
    }
    return ks_reset_checked(h ? &h->S : nullptr, "tdt_clip");
}

// the launch of one batch: TDT_CLIP_MAX_PER_READ slots of the store per read, the bound two clips per read give
static auto clip_launch(tdt_clip *h, size_t n, size_t raw_len) {
    return [=](const ks_cols &I) {
        const int rc = ks_launch(&h->S, n * TDT_CLIP_MAX_PER_READ, [&] {
            const dim3 grid((unsigned)((n + CLIP_K_TILE - 1) / CLIP_K_TILE));
            hipLaunchKernelGGL(clip_keys, grid, dim3(CLIP_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, (unsigned)h->min_clip,
                               h->S.k1, h->S.k2, (ull)h->S.cap, h->S.d_state);
        });
        if (rc == TDT_OK) h->n_rows = 0, h->align_valid = h->far_valid = h->ins_valid = h->mei_valid = false;
        if (rc || !h->ext) return rc;
        // TIDDIT_CLIPS_INS: the extension keys of the same batch into the second store, TDT_CLIP_EXT_MAX_PER_READ slots per read
        return ks_launch(&h->X, n * TDT_CLIP_EXT_MAX_PER_READ, [&] {
            const dim3 grid((unsigned)((n + CLIP_K_TILE - 1) / CLIP_K_TILE));
            hipLaunchKernelGGL(clip_ext_keys, grid, dim3(CLIP_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, (unsigned)h->min_clip,
                               h->X.k1, h->X.k2, (ull)h->X.cap, h->X.d_state);
        });
    };
}

// the two entries of a batch: ks_push_device / ks_push of tdt_keystore.h
extern "C" int tdt_clip_push_device(tdt_clip *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    return ks_push_device("tdt_clip_push_device", h, d_arrays14, n, raw_len, clip_launch(h, n, raw_len));
}

extern "C" int tdt_clip_push(tdt_clip *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off, size_t n,
                             const uint8_t *raw, size_t raw_len) {
    return ks_push("tdt_clip_push", h, ks_cols{flag, tid, pos, mapq, rec_off, raw}, n, raw_len, clip_launch(h, n, raw_len));
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

// where the site launches of one key store leave their rows: the handle's fields for that store (the buffer grows)
struct clip_site_bufs {
    void *&d_site;
    size_t &site_cap;
    clip_sites &rows;
    size_t &n_rows;
    double &ms_sites;
    hipEvent_t *ev;                               // two
};

// the site launches over the n rows of the last finish of the key store S -> got[0] = the sites, got[1] = those with SUPPORT >=
// min_support, which become B.rows.  The handle's two stores each bring their own buffers.
static int clip_sites_of_rows(tdt_ctx *ctx, const tdt_keystore &S, size_t n_, unsigned min_support, clip_site_bufs B, ull *got) {
    got[0] = got[1] = 0;
    B.ms_sites = 0;
    B.n_rows = 0;
    if (!n_) return TDT_OK;
    const int n = (int)n_;                                         // (< 2^30: ks_finish refused more)
    const size_t ntiles = (n_ + KS_TILE - 1) / KS_TILE;
    clip_work K;
    const size_t bytes = K.lay(nullptr, n_, ntiles);
    if (bytes > B.site_cap) {
        if (B.d_site) TDT_HIP(hipFree(B.d_site));
        B.d_site = nullptr;
        B.site_cap = 0;
        if (tdt_dev_malloc(&B.d_site, bytes) != hipSuccess) {
            tdt_set_error("tdt_clip_finish: out of device memory (%zu rows)", n_);
            return TDT_E_NOMEM;
        }
        B.site_cap = bytes;
    }
    K.lay(B.d_site, n_, ntiles);
    hipStream_t st = ctx->stream;
    const ull *a = S.r_k1, *b = S.r_k2;
    const int nt = (int)ntiles;
    const unsigned vgrid = n_ < CLIP_VOTE_GRID ? (unsigned)n_ : CLIP_VOTE_GRID;
    TDT_HIP(hipMemsetAsync(K.d_out, 0, 2 * 8, st));
    TDT_HIP(hipEventRecord(B.ev[0], st));
    hipLaunchKernelGGL(clip_heads<false>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, a, b, n, K.tile_heads, K.d_out, K.start);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ks_carry_sum, dim3(1), dim3(KS_BLOCK), 0, st, K.tile_heads, nt);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_heads<true>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, a, b, n, K.tile_heads, K.d_out, K.start);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_vote, dim3(vgrid), dim3(CLIP_VOTE_BLOCK), 0, st, a, b, (const unsigned *)S.r_sup, (const unsigned *)S.r_rev, n,
                       (const int *)K.start, (const ull *)K.d_out, min_support, K.V);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_keep<false>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, K.V, (const ull *)K.d_out, min_support, K.tile_kept, K.d_out, K.W);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ks_carry_sum, dim3(1), dim3(KS_BLOCK), 0, st, K.tile_kept, nt);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_keep<true>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, K.V, (const ull *)K.d_out, min_support, K.tile_kept, K.d_out, K.W);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipEventRecord(B.ev[1], st));
    TDT_HIP(hipMemcpyAsync(got, K.d_out, 2 * 8, hipMemcpyDeviceToHost, st));
    const int rc = tdt_ctx_sync(ctx);
    if (rc) return rc;
    float ms = 0;
    TDT_HIP(hipEventElapsedTime(&ms, B.ev[0], B.ev[1]));
    B.ms_sites = ms;
    B.rows = K.W;
    B.n_rows = (size_t)got[1];
    return TDT_OK;
}

// sn_out: uint64[TDT_CLIP_SN_N], the push counters and the sequences and sites of everything pushed so far; *n_rows: the rows
// tdt_clip_rows will give.  The store is left as it was.
extern "C" int tdt_clip_finish(tdt_clip *h, uint64_t min_support, uint64_t *sn_out, size_t *n_rows) {
    uint64_t res[SN_N] = {};
    ull seqs[2], sites[2];
    // (a minimum support of 1 for the runs: every distinct sequence is a row)
    int rc = ks_finish_counted(h ? &h->S : nullptr, "tdt_clip", h && sn_out && n_rows, min_support, TDT_CLIP_MAX_SUPPORT, 1, SN_PUSH_N, res, seqs);
    if (rc) return rc;
    h->align_valid = h->far_valid = h->ins_valid = h->mei_valid = false;
    h->last_support = (unsigned)min_support;
    rc = clip_sites_of_rows(h->ctx, h->S, h->S.n_rows, (unsigned)min_support, clip_site_bufs{h->d_site, h->site_cap, h->rows, h->n_rows, h->ms_sites, h->ev}, sites);
    if (rc) {
        h->S.rows_valid = false;
        return rc;
    }
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

// device milliseconds of the last finish: ks_timing's four, then [4] the site launches (heads, vote, rows)
extern "C" int tdt_clip_timing(tdt_clip *h, double *ms5) {
    const int rc = ks_timing(h ? &h->S : nullptr, "tdt_clip", ms5);
    if (rc == TDT_OK) ms5[4] = h->ms_sites;
    return rc;
}

extern "C" int tdt_clip_reserve_stats(tdt_clip *h, uint64_t *out3) { return ks_reserve_stats(h ? &h->S : nullptr, "tdt_clip", out3); }

// ---- the rows of the last finish realigned to the reference (csrc/tdt_clip_align.hip), where they lie: no round trip
struct clip_align_work {
    ca_out O;
    size_t lay(void *base, size_t n) {
        tdt_carver cv(base);
        O.status = cv.take<unsigned>(n), O.partner = cv.take<unsigned>(n), O.strand = cv.take<unsigned>(n), O.mm = cv.take<unsigned>(n);
        O.hits = cv.take<unsigned>(n), O.sn = cv.take<ull>(TDT_CLIP_ALIGN_SN_N);
        return cv.size;
    }
};

// sn_out: uint64[TDT_CLIP_ALIGN_SN_N].  No finish since the last push or reset, or a reference with another contig count: TDT_E_ARG.
extern "C" int tdt_clip_align(tdt_clip *h, tdt_refseq *ref, int W, int K, int M, uint64_t *sn_out) {
    if (!h || !ref || !sn_out || ref->ctx->device != h->ctx->device) {
        tdt_set_error("tdt_clip_align: bad argument");
        return TDT_E_ARG;
    }
    if (!h->S.rows_valid) {
        tdt_set_error("tdt_clip_align: no finish since the last push or reset");
        return TDT_E_ARG;
    }
    if (ref->n_contigs != h->n_contigs) {
        tdt_set_error("tdt_clip_align: the reference has %d contigs, the handle was made for %d", ref->n_contigs, h->n_contigs);
        return TDT_E_ARG;
    }
    int rc = ca_check_range("tdt_clip_align", W, K, M);
    if (rc) return rc;
    TDT_HIP(hipSetDevice(h->ctx->device));
    h->align_valid = false;
    h->ms_align = 0;
    const size_t n = h->n_rows;
    clip_align_work A;
    const size_t bytes = A.lay(nullptr, n);
    if (bytes > h->align_cap) {
        if (h->d_align) TDT_HIP(hipFree(h->d_align));
        h->d_align = nullptr;
        h->align_cap = 0;
        if (tdt_dev_malloc(&h->d_align, bytes) != hipSuccess) {
            tdt_set_error("tdt_clip_align: out of device memory (%zu rows)", n);
            return TDT_E_NOMEM;
        }
        h->align_cap = bytes;
    }
    A.lay(h->d_align, n);
    hipStream_t st = h->ctx->stream;
    uint64_t res[TDT_CLIP_ALIGN_SN_N] = {};
    TDT_HIP(hipMemsetAsync(A.O.sn, 0, sizeof res, st));
    TDT_HIP(hipEventRecord(h->ev[0], st));
    const clip_sites &R = h->rows;
    rc = ca_launch(h->ctx, ref, n, ca_sites{R.k1, R.side, R.clen, R.cons}, W, K, M, A.O);
    if (rc) return rc;
    TDT_HIP(hipEventRecord(h->ev[1], st));
    TDT_HIP(hipMemcpyAsync(res, A.O.sn, sizeof res, hipMemcpyDeviceToHost, st));
    rc = tdt_ctx_sync(h->ctx);
    if (rc) return rc;
    float ms = 0;
    TDT_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms_align = ms;
    h->align = A.O;
    h->align_valid = true;
    memcpy(sn_out, res, sizeof res);
    return TDT_OK;
}

// The five columns of the last tdt_clip_align, in the order of tdt_clip_rows.  *n in: the room of the arrays (ignored when all five are
// NULL), out: the rows.  Too little room: TDT_E_RANGE, nothing written.
extern "C" int tdt_clip_align_rows(tdt_clip *h, uint32_t *status, uint32_t *partner, uint32_t *strand, uint32_t *mm, uint32_t *hits, size_t *n) {
    const bool any = status || partner || strand || mm || hits;
    if (!h || !n || (any && !(status && partner && strand && mm && hits))) {
        tdt_set_error("tdt_clip_align_rows: bad argument");
        return TDT_E_ARG;
    }
    if (!h->S.rows_valid || !h->align_valid) {
        tdt_set_error("tdt_clip_align_rows: no tdt_clip_align since the last push, reset or finish");
        return TDT_E_ARG;
    }
    const size_t have = h->n_rows;
    if (any) {
        if (*n < have) {
            tdt_set_error("tdt_clip_align_rows: room for %zu rows, %zu kept", *n, have);
            return TDT_E_RANGE;
        }
        if (have) {
            TDT_HIP(hipSetDevice(h->ctx->device));
            hipStream_t st = h->ctx->stream;
            const ca_out &O = h->align;
            TDT_HIP(hipMemcpyAsync(status, O.status, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(partner, O.partner, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(strand, O.strand, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(mm, O.mm, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(hits, O.hits, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
        }
    }
    *n = have;
    return TDT_OK;
}

extern "C" int tdt_clip_align_timing(tdt_clip *h, double *ms) {
    if (!h || !ms || !h->S.rows_valid || !h->align_valid) {
        tdt_set_error("tdt_clip_align_timing: bad argument, or no tdt_clip_align since the last push, reset or finish");
        return TDT_E_ARG;
    }
    *ms = h->ms_align;
    return TDT_OK;
}

// ---- the rows of the last finish placed genome-wide (csrc/tdt_clip_far.hip), where they lie: no round trip
struct clip_far_work {
    far_out O;
    far_work Wk;
    size_t lay(void *base, size_t n) {
        tdt_carver cv(base);
        O.status = cv.take<unsigned>(n), O.ptid = cv.take<unsigned>(n), O.partner = cv.take<unsigned>(n), O.strand = cv.take<unsigned>(n);
        O.mm = cv.take<unsigned>(n), O.hits = cv.take<unsigned>(n), O.sn = cv.take<ull>(TDT_CLIP_FAR_SN_N);
        const size_t head = cv.size;
        return head + Wk.lay(base ? (char *)base + head : nullptr, n);
    }
};

// sn_out: uint64[TDT_CLIP_FAR_SN_N].  No finish since the last push or reset, or a reference with another contig count: TDT_E_ARG.
extern "C" int tdt_clip_far(tdt_clip *h, tdt_refseq *ref, int K, int M, uint64_t *sn_out) {
    if (!h || !ref || !sn_out || ref->ctx->device != h->ctx->device) {
        tdt_set_error("tdt_clip_far: bad argument");
        return TDT_E_ARG;
    }
    if (!h->S.rows_valid) {
        tdt_set_error("tdt_clip_far: no finish since the last push or reset");
        return TDT_E_ARG;
    }
    if (ref->n_contigs != h->n_contigs) {
        tdt_set_error("tdt_clip_far: the reference has %d contigs, the handle was made for %d", ref->n_contigs, h->n_contigs);
        return TDT_E_ARG;
    }
    const size_t n = h->n_rows;
    int rc = far_check_range("tdt_clip_far", ref, n, K, M);
    if (rc) return rc;
    TDT_HIP(hipSetDevice(h->ctx->device));
    h->far_valid = false;
    for (int k = 0; k < 4; k++) h->ms_far[k] = 0;
    for (int k = 0; k < 5; k++)
        if (!h->ev_far[k]) TDT_HIP(hipEventCreate(&h->ev_far[k]));
    clip_far_work A;
    const size_t bytes = A.lay(nullptr, n);
    if (bytes > h->far_cap) {
        if (h->d_far) TDT_HIP(hipFree(h->d_far));
        h->d_far = nullptr;
        h->far_cap = 0;
        if (tdt_dev_malloc(&h->d_far, bytes) != hipSuccess) {
            tdt_set_error("tdt_clip_far: out of device memory (%zu rows)", n);
            return TDT_E_NOMEM;
        }
        h->far_cap = bytes;
    }
    A.lay(h->d_far, n);
    hipStream_t st = h->ctx->stream;
    uint64_t res[TDT_CLIP_FAR_SN_N] = {};
    TDT_HIP(hipMemsetAsync(A.O.sn, 0, sizeof res, st));
    const clip_sites &R = h->rows;
    rc = far_launch(h->ctx, ref, n, ca_sites{R.k1, R.side, R.clen, R.cons}, K, M, A.O, A.Wk, h->ev_far);
    if (rc) {
        (void)tdt_ctx_sync(h->ctx);
        return rc;
    }
    TDT_HIP(hipMemcpyAsync(res, A.O.sn, sizeof res, hipMemcpyDeviceToHost, st));
    rc = tdt_ctx_sync(h->ctx);
    if (rc) return rc;
    for (int k = 0; k < 4; k++) {
        float ms = 0;
        TDT_HIP(hipEventElapsedTime(&ms, h->ev_far[k], h->ev_far[k + 1]));
        h->ms_far[k] = ms;
    }
    h->far = A.O;
    h->far_valid = true;
    memcpy(sn_out, res, sizeof res);
    return TDT_OK;
}

// The six columns of the last tdt_clip_far, in the order of tdt_clip_rows.  *n in: the room of the arrays (ignored when all six are
// NULL), out: the rows.  Too little room: TDT_E_RANGE, nothing written.
extern "C" int tdt_clip_far_rows(tdt_clip *h, uint32_t *status, uint32_t *partner_tid, uint32_t *partner, uint32_t *strand, uint32_t *mm, uint32_t *hits,
                                 size_t *n) {
    const bool any = status || partner_tid || partner || strand || mm || hits;
    if (!h || !n || (any && !(status && partner_tid && partner && strand && mm && hits))) {
        tdt_set_error("tdt_clip_far_rows: bad argument");
        return TDT_E_ARG;
    }
    if (!h->S.rows_valid || !h->far_valid) {
        tdt_set_error("tdt_clip_far_rows: no tdt_clip_far since the last push, reset or finish");
        return TDT_E_ARG;
    }
    const size_t have = h->n_rows;
    if (any) {
        if (*n < have) {
            tdt_set_error("tdt_clip_far_rows: room for %zu rows, %zu kept", *n, have);
            return TDT_E_RANGE;
        }
        if (have) {
            TDT_HIP(hipSetDevice(h->ctx->device));
            hipStream_t st = h->ctx->stream;
            const far_out &O = h->far;
            uint32_t *dst[6] = {status, partner_tid, partner, strand, mm, hits};
            const unsigned *src[6] = {O.status, O.ptid, O.partner, O.strand, O.mm, O.hits};
            for (int k = 0; k < 6; k++) TDT_HIP(hipMemcpyAsync(dst[k], src[k], have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
        }
    }
    *n = have;
    return TDT_OK;
}

extern "C" int tdt_clip_far_timing(tdt_clip *h, double *ms4) {
    if (!h || !ms4 || !h->S.rows_valid || !h->far_valid) {
        tdt_set_error("tdt_clip_far_timing: bad argument, or no tdt_clip_far since the last push, reset or finish");
        return TDT_E_ARG;
    }
    for (int k = 0; k < 4; k++) ms4[k] = h->ms_far[k];
    return TDT_OK;
}

// ---- TIDDIT_CLIPS_INS: the second store, and the rows of the last finish extended, paired and closed where they lie (csrc/tdt_clip_ins.hip)
// The store of the extension keys, of `capacity` keys.  Before the first push only (the two stores hold the same reads): a handle that
// has it already, or that has been pushed to, is refused with TDT_E_ARG.
extern "C" int tdt_clip_ext_enable(tdt_clip *h, size_t capacity) {
    if (!h || h->ext || h->S.upper) {
        tdt_set_error("tdt_clip_ext_enable: bad argument, enabled already, or pushed to already");
        return TDT_E_ARG;
    }
    if (capacity >= (1ull << 40)) {
        tdt_set_error("tdt_clip_ext_enable: capacity %zu", capacity);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    int rc = ks_init(&h->X, h->ctx, "tdt_clip_ext", XT_OR1, capacity);
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && rc == TDT_OK && e == hipSuccess; k++) e = hipEventCreate(&h->ev_ins[k]);
    if (rc == TDT_OK && e != hipSuccess) {
        tdt_set_error("tdt_clip_ext_enable: %s", hipGetErrorString(e));
        rc = TDT_E_HIP;
    }
    if (rc) {
        ks_free(&h->X);
        for (int k = 0; k < 4; k++) {
            if (h->ev_ins[k]) (void)hipEventDestroy(h->ev_ins[k]);
            h->ev_ins[k] = nullptr;
        }
        h->X = tdt_keystore{};
        return rc;
    }
    h->ext = true;
    return TDT_OK;
}

extern "C" int tdt_clip_ext_keys(tdt_clip *h, uint64_t *k1, uint64_t *k2, size_t *n) {
    return ks_keys(h && h->ext ? &h->X : nullptr, "tdt_clip_ext", k1, k2, n);
}

struct clip_ins_bufs {
    unsigned *eclen;
    ull *cons5, *sn;
    ins_work Wk;
    size_t lay(void *base, size_t n) {
        tdt_carver cv(base);
        eclen = cv.take<unsigned>(n), cons5 = cv.take<ull>(n * TDT_CLIP_EXT_WORDS), sn = cv.take<ull>(TDT_CLIP_INS_SN_N);
        const size_t head = cv.size;
        return head + Wk.lay(base ? (char *)base + head : nullptr, n);
    }
};

// a buffer of the handle that only grows
static int clip_grow(const char *fn, void **d, size_t *cap, size_t bytes) {
    if (bytes <= *cap) return TDT_OK;
    if (*d) TDT_HIP(hipFree(*d));
    *d = nullptr;
    *cap = 0;
    if (tdt_dev_malloc(d, bytes) != hipSuccess) {
        tdt_set_error("%s: out of device memory (%zu bytes)", fn, bytes);
        return TDT_E_NOMEM;
    }
    *cap = bytes;
    return TDT_OK;
}

// sn_out: uint64[TDT_CLIP_INS_SN_N].  The extension store is finished with the minimum support of the last tdt_clip_finish, its
// chunks are gathered onto that finish's rows, and the rows are paired and closed.  No finish since the last push or reset, or no
// tdt_clip_ext_enable: TDT_E_ARG.
extern "C" int tdt_clip_ins(tdt_clip *h, int K, int O, int M, uint64_t *sn_out) {
    if (!h || !sn_out) {
        tdt_set_error("tdt_clip_ins: bad argument");
        return TDT_E_ARG;
    }
    if (!h->ext || !h->S.rows_valid) {
        tdt_set_error("tdt_clip_ins: %s", h->ext ? "no finish since the last push or reset" : "no tdt_clip_ext_enable");
        return TDT_E_ARG;
    }
    int rc = ins_check_range("tdt_clip_ins", K, O, M);
    if (rc) return rc;
    TDT_HIP(hipSetDevice(h->ctx->device));
    h->ins_valid = h->mei_valid = false;
    h->n_pairs = 0;
    for (int k = 0; k < 3; k++) h->ms_ins[k] = 0;
    hipStream_t st = h->ctx->stream;
    // ---- the extension store's (chunk, site) rows: the finish of the first store, on the second
    ull state[KS_WORDS], runs[2], sites[2];
    rc = ks_stored(&h->X, state);
    if (rc) return rc;
    TDT_HIP(hipEventRecord(h->ev_ins[0], st));
    rc = ks_finish(&h->X, state, 1, runs);
    if (rc == TDT_OK)
        rc = clip_sites_of_rows(h->ctx, h->X, h->X.n_rows, h->last_support, clip_site_bufs{h->d_xsite, h->xsite_cap, h->xrows, h->n_xrows, h->ms_xsites, h->ev}, sites);
    if (rc) return rc;
    // ---- the gather onto the base rows, then the pairs
    const size_t n = h->n_rows;
    clip_ins_bufs A;
    rc = clip_grow("tdt_clip_ins", &h->d_ins, &h->ins_cap, A.lay(nullptr, n));
    if (rc) return rc;
    A.lay(h->d_ins, n);
    uint64_t res[TDT_CLIP_INS_SN_N] = {};
    const clip_sites &R = h->rows, &X = h->xrows;
    TDT_HIP(hipMemsetAsync(A.sn, 0, sizeof res, st));
    TDT_HIP(hipEventRecord(h->ev_ins[1], st));
    rc = ins_gather_launch(h->ctx, n, R.k1, R.side, R.clen, R.cons, h->n_xrows, ins_chunks{X.k1, X.side, X.clen, X.cons}, A.eclen, A.cons5);
    if (rc) return rc;
    TDT_HIP(hipEventRecord(h->ev_ins[2], st));
    const ins_sites S{R.k1, R.side, A.eclen, A.cons5};
    rc = ins_count_launch(h->ctx, n, S, K, A.Wk, A.sn);
    if (rc) return rc;
    TDT_HIP(hipMemcpyAsync(res, A.sn, sizeof res, hipMemcpyDeviceToHost, st));
    rc = tdt_ctx_sync(h->ctx);
    if (rc) return rc;
    const size_t np = (size_t)res[IN_PAIRS];                              // (the pairs: rows for them are made now)
    ins_out P{};
    rc = clip_grow("tdt_clip_ins", &h->d_pairs, &h->pairs_cap, P.lay(nullptr, np));
    if (rc) return rc;
    P.lay(h->d_pairs, np);
    rc = ins_pairs_launch(h->ctx, n, S, K, O, M, A.Wk, np, P, A.sn);
    if (rc) return rc;
    TDT_HIP(hipEventRecord(h->ev_ins[3], st));
    TDT_HIP(hipMemcpyAsync(res, A.sn, sizeof res, hipMemcpyDeviceToHost, st));
    rc = tdt_ctx_sync(h->ctx);
    if (rc) return rc;
    for (int k = 0; k < 3; k++) {
        float ms = 0;
        TDT_HIP(hipEventElapsedTime(&ms, h->ev_ins[k], h->ev_ins[k + 1]));
        h->ms_ins[k] = ms;
    }
    res[IN_EXT_LEFT] = state[XN_LEFT], res[IN_EXT_RIGHT] = state[XN_RIGHT], res[IN_EXT_KEYS] = state[KS_N], res[IN_CUT] = state[XN_CUT];
    h->ext_eclen = A.eclen, h->ext_cons5 = A.cons5;
    h->pairs = P;
    h->n_pairs = np;
    h->ins_valid = true;
    memcpy(sn_out, res, sizeof res);
    return TDT_OK;
}

// ECLEN and the five words of every row of the last finish, as the last tdt_clip_ins gathered them, in the order of tdt_clip_rows.
// *n in: the room of the arrays (ignored when both are NULL), out: the rows.  Too little room: TDT_E_RANGE, nothing written.
extern "C" int tdt_clip_ext_rows(tdt_clip *h, uint32_t *eclen, uint64_t *cons5, size_t *n) {
    if (!h || !n || ((eclen || cons5) && !(eclen && cons5))) {
        tdt_set_error("tdt_clip_ext_rows: bad argument");
        return TDT_E_ARG;
    }
    if (!h->S.rows_valid || !h->ins_valid) {
        tdt_set_error("tdt_clip_ext_rows: no tdt_clip_ins since the last push, reset or finish");
        return TDT_E_ARG;
    }
    const size_t have = h->n_rows;
    if (eclen) {
        if (*n < have) {
            tdt_set_error("tdt_clip_ext_rows: room for %zu rows, %zu kept", *n, have);
            return TDT_E_RANGE;
        }
        if (have) {
            TDT_HIP(hipSetDevice(h->ctx->device));
            hipStream_t st = h->ctx->stream;
            TDT_HIP(hipMemcpyAsync(eclen, h->ext_eclen, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(cons5, h->ext_cons5, have * TDT_CLIP_EXT_WORDS * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
        }
    }
    *n = have;
    return TDT_OK;
}

// The pairs of the last tdt_clip_ins, ascending by (t, P_R, P_L): the two rows' indices into tdt_clip_rows, TSD, status (1 closed),
// LEN, MISMATCH, CLOSURES and TDT_CLIP_INS_SEQ_WORDS words of SEQ.  *n in: the room of the arrays (ignored when all eight are NULL),
// out: the pairs.  Too little room: TDT_E_RANGE, nothing written.
extern "C" int tdt_clip_ins_rows(tdt_clip *h, uint32_t *r_row, uint32_t *l_row, uint32_t *tsd, uint32_t *status, uint32_t *len, uint32_t *mm, uint32_t *closures,
                                 uint64_t *seq10, size_t *n) {
    const bool any = r_row || l_row || tsd || status || len || mm || closures || seq10;
    if (!h || !n || (any && !(r_row && l_row && tsd && status && len && mm && closures && seq10))) {
        tdt_set_error("tdt_clip_ins_rows: bad argument");
        return TDT_E_ARG;
    }
    if (!h->S.rows_valid || !h->ins_valid) {
        tdt_set_error("tdt_clip_ins_rows: no tdt_clip_ins since the last push, reset or finish");
        return TDT_E_ARG;
    }
    const size_t have = h->n_pairs;
    if (any) {
        if (*n < have) {
            tdt_set_error("tdt_clip_ins_rows: room for %zu pairs, %zu kept", *n, have);
            return TDT_E_RANGE;
        }
        if (have) {
            TDT_HIP(hipSetDevice(h->ctx->device));
            hipStream_t st = h->ctx->stream;
            const ins_out &P = h->pairs;
            uint32_t *dst[7] = {r_row, l_row, tsd, status, len, mm, closures};
            const unsigned *src[7] = {P.r_row, P.l_row, P.tsd, P.status, P.len, P.mm, P.closures};
            for (int k = 0; k < 7; k++) TDT_HIP(hipMemcpyAsync(dst[k], src[k], have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(seq10, P.seq10, have * INS_SEQ_WORDS * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
        }
    }
    *n = have;
    return TDT_OK;
}

// device milliseconds of the last tdt_clip_ins: ms3 = the extension store's finish (sort, run lengths, site launches), the gather,
// the pair launches (count, offsets, rows, closure)
extern "C" int tdt_clip_ins_timing(tdt_clip *h, double *ms3) {
    if (!h || !ms3 || !h->S.rows_valid || !h->ins_valid) {
        tdt_set_error("tdt_clip_ins_timing: bad argument, or no tdt_clip_ins since the last push, reset or finish");
        return TDT_E_ARG;
    }
    for (int k = 0; k < 3; k++) ms3[k] = h->ms_ins[k];
    return TDT_OK;
}

// ---- TIDDIT_CLIPS_MEI: the pair rows of the last tdt_clip_ins named against a family library where they lie (csrc/tdt_swalign.hip)
struct clip_mei_bufs {
    int *off;
    ull *sn;
    sw_table Q;
    sw_out O;
    size_t lay(void *base, size_t n_pairs) {                       // (room for two queries per pair)
        tdt_carver cv(base);
        off = cv.take<int>(n_pairs + 1), sn = cv.take<ull>(TDT_SW_SN_N);
        size_t head = cv.size;
        head += Q.lay(base ? (char *)base + head : nullptr, 2 * n_pairs);
        return head + O.lay(base ? (char *)base + head : nullptr, 2 * n_pairs);
    }
};

// sn_out: uint64[TDT_SW_SN_N].  lib: the family library, every sequence loaded; it is read, not kept.  No tdt_clip_ins since the last
// push, reset or finish: TDT_E_ARG.
extern "C" int tdt_clip_mei(tdt_clip *h, tdt_refseq *lib, int A, uint64_t *sn_out) {
    if (!h || !lib || !sn_out) {
        tdt_set_error("tdt_clip_mei: bad argument");
        return TDT_E_ARG;
    }
    if (!h->S.rows_valid || !h->ins_valid) {
        tdt_set_error("tdt_clip_mei: no tdt_clip_ins since the last push, reset or finish");
        return TDT_E_ARG;
    }
    const size_t np = h->n_pairs;
    int rc = sw_check("tdt_clip_mei", h->ctx, lib, 2 * np, A);
    if (rc) return rc;
    TDT_HIP(hipSetDevice(h->ctx->device));
    h->mei_valid = false;
    h->n_mei = 0;
    for (int k = 0; k < 3; k++) h->ms_mei[k] = 0;
    for (int k = 0; k < 4; k++)
        if (!h->ev_mei[k]) TDT_HIP(hipEventCreate(&h->ev_mei[k]));
    hipStream_t st = h->ctx->stream;
    clip_mei_bufs B;
    rc = clip_grow("tdt_clip_mei", &h->d_mei, &h->mei_cap, B.lay(nullptr, np));
    if (rc) return rc;
    B.lay(h->d_mei, np);
    uint64_t res[TDT_SW_SN_N] = {};
    int nq = 0;
    const ins_sites S{h->rows.k1, h->rows.side, h->ext_eclen, h->ext_cons5};
    TDT_HIP(hipMemsetAsync(B.sn, 0, sizeof res, st));
    TDT_HIP(hipEventRecord(h->ev_mei[0], st));
    rc = sw_offsets_launch(h->ctx, np, h->pairs.status, B.off);
    if (rc == TDT_OK) rc = sw_build_launch(h->ctx, S, np, h->pairs, B.off, B.Q);
    if (rc) return rc;
    TDT_HIP(hipEventRecord(h->ev_mei[1], st));
    TDT_HIP(hipMemcpyAsync(&nq, B.off + np, 4, hipMemcpyDeviceToHost, st));
    rc = tdt_ctx_sync(h->ctx);
    if (rc) return rc;
    const sw_queries Q{B.Q.seq10, B.Q.qlen, B.Q.pair, B.Q.part};
    sw_work W{};
    void *d_work = nullptr;
    const size_t problems = (size_t)nq * 2 * (size_t)lib->n_contigs;
    if (nq && tdt_dev_malloc(&d_work, W.lay(nullptr, problems)) != hipSuccess) {
        tdt_set_error("tdt_clip_mei: out of device memory (%zu problems)", problems);
        return TDT_E_NOMEM;
    }
    W.lay(d_work, problems);
    hipError_t e = hipSuccess;
    rc = sw_align_launch(h->ctx, lib, (size_t)nq, Q, W);
    if (rc == TDT_OK) e = hipEventRecord(h->ev_mei[2], st);
    if (rc == TDT_OK && e == hipSuccess) rc = sw_reduce_launch(h->ctx, lib, (size_t)nq, Q, W, A, B.O, B.sn);
    if (rc == TDT_OK && e == hipSuccess) e = hipEventRecord(h->ev_mei[3], st);
    if (rc == TDT_OK && e == hipSuccess) e = hipMemcpyAsync(res, B.sn, sizeof res, hipMemcpyDeviceToHost, st);
    if (rc == TDT_OK && e == hipSuccess) rc = tdt_ctx_sync(h->ctx);
    (void)hipStreamSynchronize(st);
    if (d_work) (void)hipFree(d_work);
    if (rc) return rc;
    TDT_HIP(e);
    for (int k = 0; k < 3; k++) {
        float ms = 0;
        TDT_HIP(hipEventElapsedTime(&ms, h->ev_mei[k], h->ev_mei[k + 1]));
        h->ms_mei[k] = ms;
    }
    h->mei_q = B.Q, h->mei_out = B.O;
    h->n_mei = (size_t)nq;
    h->mei_valid = true;
    memcpy(sn_out, res, sizeof res);
    return TDT_OK;
}

// The queries of the last tdt_clip_mei, in the order of the pair rows (an OPEN pair's LEFT query, then its RIGHT query): the pair row,
// the part, the length and the nine result columns.  *n in: the room of the arrays (ignored when all twelve are NULL), out: the
// queries.  Too little room: TDT_E_RANGE, nothing written.
extern "C" int tdt_clip_mei_rows(tdt_clip *h, uint32_t *pair, uint32_t *part, uint32_t *qlen, uint32_t *family, uint32_t *strand, uint32_t *score, uint32_t *qstart,
                                 uint32_t *qend, uint32_t *fstart, uint32_t *fend, uint32_t *second, uint32_t *second_family, size_t *n) {
    uint32_t *dst[12] = {pair, part, qlen, family, strand, score, qstart, qend, fstart, fend, second, second_family};
    int given = 0;
    for (int k = 0; k < 12; k++) given += dst[k] != nullptr;
    if (!h || !n || (given && given != 12)) {
        tdt_set_error("tdt_clip_mei_rows: bad argument");
        return TDT_E_ARG;
    }
    if (!h->S.rows_valid || !h->ins_valid || !h->mei_valid) {
        tdt_set_error("tdt_clip_mei_rows: no tdt_clip_mei since the last push, reset, finish or tdt_clip_ins");
        return TDT_E_ARG;
    }
    const size_t have = h->n_mei;
    if (given) {
        if (*n < have) {
            tdt_set_error("tdt_clip_mei_rows: room for %zu queries, %zu kept", *n, have);
            return TDT_E_RANGE;
        }
        if (have) {
            TDT_HIP(hipSetDevice(h->ctx->device));
            hipStream_t st = h->ctx->stream;
            const sw_table &Q = h->mei_q;
            const sw_out &O = h->mei_out;
            const unsigned *src[12] = {Q.pair, Q.part, Q.qlen, O.family, O.strand, O.score, O.qstart, O.qend, O.fstart, O.fend, O.second, O.second_family};
            for (int k = 0; k < 12; k++) TDT_HIP(hipMemcpyAsync(dst[k], src[k], have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
        }
    }
    *n = have;
    return TDT_OK;
}

// device milliseconds of the last tdt_clip_mei: ms3 = the query build (offsets, table), the alignment launch, the reduction
extern "C" int tdt_clip_mei_timing(tdt_clip *h, double *ms3) {
    if (!h || !ms3 || !h->S.rows_valid || !h->ins_valid || !h->mei_valid) {
        tdt_set_error("tdt_clip_mei_timing: bad argument, or no tdt_clip_mei since the last push, reset, finish or tdt_clip_ins");
        return TDT_E_ARG;
    }
    for (int k = 0; k < 3; k++) ms3[k] = h->ms_mei[k];
    return TDT_OK;
}
