// Small-indel candidates for gfx950 — every distinct insertion or deletion the reads of the --sv scan carry in their CIGARs
// (TIDDIT_INDELS), with its support by strand.  The definition is tiddit_indels.py's: per keyed event K1 = tid << 32 | P and
// K2 = type << 63 | len << 47 | kind << 45 | payload << 1 | rev; the sets of equal (K1, K2 >> 1) are the distinct events.  Every result
// is an order-independent integer, so it equals the definition exactly.
//   * indel_keys — ONE launch per batch, on the columns and record bytes that are already resident.  Lane = read for the filters (flag,
//     tid, mapq: coalesced columns); the eligible reads are compacted inside the workgroup as dup_keys compacts its reads, then lane =
//     compacted read: the record is bounded exactly as tdt_dup / tdt_qc / tdt_alleles bound one, its CIGAR is walked ONCE with the op in
//     front and the op behind at hand (the flank test), and its at most INDEL_MAX_PER_READ keyed events stay in registers (P, len and
//     type, the query offset: three words each).  A fifth keyed event is counted and not kept; the walk goes on to its end, because an op
//     code above 8 or a P outside [1, 2^31) further on still makes the record malformed.  Malformed / noisy / ok is decided behind the
//     walk: a read gives all of its events or none.  Only then are the inserted bases read (4-bit codes at the query offset the walk
//     summed) — the first kernel here that emits a variable number of items per read.  A workgroup owns INDEL_K_TILE consecutive reads,
//     INDEL_BLOCK at a time; a round's keys go behind the tile's earlier ones in LDS (slots by a prefix sum of the reads' event counts)
//     and the tile's keys are appended to the store (two uint64 columns in HBM) behind ONE atomic.  The counters and the OR of the keys
//     and of their complements are merged per wave and then over the workgroup: one atomic per workgroup and non-zero word.
//     The host knows only an upper bound of the keys stored (INDEL_MAX_PER_READ per read): room for it is reserved BEFORE the launch,
//     and a growth first asks the device for the real count (dup_reserve's policy).  The kernel still tests every slot against the
//     capacity it was given and raises a flag instead of writing.
//   * tdt_indel_finish — once per job: the LSD sort of tdt_dup_finish (sort (K2, index); gather K1; sort (K1[perm], perm), stable;
//     gather K2), then the runs of equal (K1, K2 >> 1) in plain launches, none of whose workgroups waits for another: indel_tile_heads
//     notes each tile's last run head and last FULL-key head (a change of (K1, K2), strand included), indel_carry (one workgroup)
//     carries both across the tiles, indel_runs<false> measures every run at its END — size = position - last head + 1; the sort puts
//     rev = 0 first, so REV = position - last full-key head + 1 when the last member has bit 0 set, else 0 — and counts the runs it keeps
//     per tile, indel_carry_sum turns those counts into offsets, indel_runs<true> writes the kept runs as rows in key order.
#include "tdt_batch.h"
#include "tdt_bam_record.h"
#include "tdt_refseq.h"

#include <vector>

typedef unsigned long long ull;

#define INDEL_BLOCK 256
#define INDEL_K_TILE 512                      // reads of an indel_keys workgroup; it stages at most 4 x that many keys in LDS (32 KB)
#define INDEL_TILE 4096                       // keys of a run-length workgroup: INDEL_BLOCK lanes, INDEL_TILE / INDEL_BLOCK rounds
#define INDEL_MAX_CONTIGS (1 << 24)
#define INDEL_P_LIMIT (1ll << 31)
#define INDEL_NORM_MAX_SHIFT TDT_INDEL_NORM_MAX_SHIFT   // CAP: no event is shifted further left than this (64 word steps)
#define INDEL_PACK_MAX 22                     // the longest insertion whose bases fit the 44-bit payload, two bits each

static_assert(INDEL_TILE % INDEL_BLOCK == 0 && INDEL_K_TILE % INDEL_BLOCK == 0, "whole rounds");
static_assert(TDT_INDEL_MAX_PER_READ == 4, "the events of a read are four register triples");

// the SN rows, in the order of the file; the first nine are the push's
enum { SN_RECORDS = 0, SN_ELIGIBLE, SN_MALFORMED, SN_UNANCHORED, SN_TOO_LONG, SN_NOISY, SN_READS_WITH_EVENTS, SN_INSERTIONS, SN_DELETIONS,
       SN_DISTINCT, SN_REPORTED, SN_N, SN_PUSH_N = SN_DISTINCT };
static_assert(SN_N == TDT_INDEL_SN_N, "SN rows");
// the state words behind the push counters: the OR of the keys and of their complements; the number of keys stored, in a cache line of its own
// (and, words of their own in the counters' line, what the left-normalisation counted: events shifted, shifts that stopped at CAP, events
// off the reference — the line of ST_N stays the store-slot atomic's alone)
enum { ST_OR1 = SN_PUSH_N, ST_NAND1, ST_OR2, ST_NAND2, ST_SHIFTED, ST_CAPPED, ST_OFFREF, ST_N = 16, ST_OVERFLOW, ST_WORDS = 32 };
static_assert(ST_OFFREF < ST_N && ST_N * 8 % 128 == 0, "state layout");
static_assert(INDEL_NORM_MAX_SHIFT % 16 == 0, "CAP is whole word steps");

struct tdt_indel {
    tdt_ctx *ctx;
    int n_contigs, min_mapq;
    tdt_refseq *ref;                          // attached by tdt_indel_set_reference (not owned); NULL: keys as the aligner placed them
    ull *k1, *k2;                             // the store: cap entries each
    size_t cap, upper;                        // upper: no more than this many keys are stored (the device knows how many)
    ull *d_state;                             // ST_WORDS
    tdt_batch_io io;                          // columns + raw bytes of the host entry
    void *d_work;                             // the finish's buffers (grows)
    size_t work_cap;
    ull *r_k1, *r_k2;                         // the rows of the last finish (inside d_work), n_rows of them
    unsigned *r_sup, *r_rev;
    size_t n_rows;
    bool rows_valid;
    ull asks, grows;                          // how often the reserve asked the device for the real count / made a bigger store
    hipEvent_t ev[5];
    double ms[4];
};

struct IndelIn {
    const uint16_t *flag;
    const int32_t *tid, *pos;
    const uint8_t *mapq;
    const uint64_t *rec_off;
    const uint8_t *raw;
};

__device__ __forceinline__ bool indel_is_match(unsigned op) { return op == 0 || op == 7 || op == 8; }

// K2 of an insertion of len bases at query offset q of a sequence of l_seq bases at raw[seq ...]
__device__ __forceinline__ ull indel_ins_key(const uint8_t *__restrict__ raw, ull seq, unsigned q, unsigned len, int l_seq) {
    const ull head = (1ull << 63) | ((ull)len << 47);
    if ((ull)q + len > (ull)l_seq) return head | (2ull << 45);              // (the span is not inside the sequence: SEQ *)
    ull h = 0xcbf29ce484222325ull, pack = 0;
    bool acgt = len <= INDEL_PACK_MAX;
    for (unsigned i = 0; i < len; i++) {
        const unsigned at = q + i;
        const unsigned b = (raw[seq + (at >> 1)] >> ((at & 1u) ? 0 : 4)) & 0xfu;
        h = (h ^ (ull)b) * 0x100000001b3ull;
        const unsigned code = b == 1 ? 0u : b == 2 ? 1u : b == 4 ? 2u : 3u;
        acgt = acgt && (b == 1 || b == 2 || b == 4 || b == 8);
        if (i < INDEL_PACK_MAX) pack |= (ull)code << (2 * i);
    }
    if (acgt) return head | (pack << 1);
    return head | (1ull << 45) | (((h ^ (h >> 44)) & ((1ull << 44) - 1ull)) << 1);
}

// ---- the left-normalisation (NORM): tiddit_indels.left_normalise on the resident reference
// How far the event at P = p (n bases; an insertion's bases at query offset q of the sequence at raw[seq ...], its span inside the
// sequence) moves left: the largest k <= min(CAP, p - 1) with, for every j < k, a_j == b_j and a_j one of A C G T, where
// a_j = ref[p - j - 1] and b_j = ref[p - j - 1 + n] — but S[n - 1 - j] for an insertion while j < n.  16 bases per step: the window of
// the 16 bases ending at p - k - 1 against the window n bases to its right (or the read's own nibbles going left), XOR, OR the
// mask of the non-ACGT nibbles, one count of trailing zeros.  Every window lies inside the contig or its zero guard, and a zero nibble
// stops the run.
__device__ __forceinline__ unsigned indel_shift(const uint8_t *__restrict__ store, ull off, unsigned p, unsigned n, bool ins,
                                                const uint8_t *__restrict__ raw, ull seq, unsigned q) {
    const unsigned kmax = p - 1u < INDEL_NORM_MAX_SHIFT ? p - 1u : INDEL_NORM_MAX_SHIFT;       // (p >= 1)
    const ull g0 = off * 2ull + (ull)p;                            // the store nibble of base p
    unsigned k = 0;
    if (ins) {
        const unsigned lim = n < kmax ? n : kmax;
        while (k < lim) {
            const unsigned m = lim - k < 16u ? lim - k : 16u;
            const ull x = tdt_ref_left16(store, g0 - k - 1ull);
            ull y = 0;
            for (unsigned t = 0; t < m; t++) {
                const unsigned at = q + n - 1u - k - t;
                y |= (ull)((raw[seq + (at >> 1)] >> ((at & 1u) ? 0 : 4)) & 0xfu) << (4u * t);
            }
            ull stop = (x ^ y) | tdt_ref_not_acgt(x);
            if (m < 16u) stop |= ~0ull << (4u * m);
            const unsigned run = stop ? (unsigned)__builtin_ctzll(stop) >> 2 : 16u;
            k += run;
            if (run < m) return k;
        }
        if (k < n) return k;                                       // (k == kmax: the bound, not a mismatch, ended it)
    }
    while (k < kmax) {
        const ull x = tdt_ref_left16(store, g0 - k - 1ull), y = tdt_ref_left16(store, g0 - k - 1ull + n);
        const ull stop = (x ^ y) | tdt_ref_not_acgt(x);
        const unsigned run = stop ? (unsigned)__builtin_ctzll(stop) >> 2 : 16u;
        k += run;
        if (run < 16u) break;
    }
    return k < kmax ? k : kmax;
}

// K2 of that insertion after k > 0 shifts: code i of the rotated allele is ref[p - k + i] for i < k and S[i - k] behind it
__device__ __forceinline__ ull indel_ins_key_rotated(const uint8_t *__restrict__ raw, ull seq, unsigned q, unsigned len, const uint8_t *__restrict__ store,
                                                     ull off, unsigned p, unsigned k) {
    const ull head = (1ull << 63) | ((ull)len << 47);
    ull h = 0xcbf29ce484222325ull, pack = 0;
    bool acgt = len <= INDEL_PACK_MAX;
    for (unsigned i = 0; i < len; i++) {
        const unsigned at = q + i - k;                             // (used where i >= k)
        const unsigned b = i < k ? tdt_ref_code(store, off, (long long)p - k + i) : (raw[seq + (at >> 1)] >> ((at & 1u) ? 0 : 4)) & 0xfu;
        h = (h ^ (ull)b) * 0x100000001b3ull;
        const unsigned code = b == 1 ? 0u : b == 2 ? 1u : b == 4 ? 2u : 3u;
        acgt = acgt && (b == 1 || b == 2 || b == 4 || b == 8);
        if (i < INDEL_PACK_MAX) pack |= (ull)code << (2 * i);
    }
    if (acgt) return head | (pack << 1);
    return head | (1ull << 45) | (((h ^ (h >> 44)) & ((1ull << 44) - 1ull)) << 1);
}

// NORM false is the kernel of TIDDIT_INDELS alone; NORM true shifts a read's events between the walk and the keying (Rf: the reference)
template <bool NORM>
__global__ __launch_bounds__(INDEL_BLOCK) void indel_keys(IndelIn I, int n, ull raw_len, unsigned min_mapq, ull *__restrict__ k1s, ull *__restrict__ k2s,
                                                          ull cap, ull *__restrict__ st, tdt_refview Rf) {
    __shared__ ull s_k1[INDEL_K_TILE * TDT_INDEL_MAX_PER_READ], s_k2[INDEL_K_TILE * TDT_INDEL_MAX_PER_READ];   // the tile's keys, in the order they were made
    __shared__ int s_read[INDEL_BLOCK];
    __shared__ int s_wsum[INDEL_BLOCK / 64], s_wkeys[INDEL_BLOCK / 64];
    __shared__ ull s_cnt[INDEL_BLOCK / 64][SN_PUSH_N + 4];        // per wave: the push counters, then the OR / NAND words
    __shared__ ull s_base;
    __shared__ ull s_norm[NORM ? INDEL_BLOCK / 64 : 1][3];         // per wave: shifted, capped, off the reference
    ull nshift = 0, ncap = 0, noff = 0;                            // (this lane's)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long lo = (long long)blockIdx.x * INDEL_K_TILE, hi = lo + INDEL_K_TILE < n ? lo + INDEL_K_TILE : n;
    ull cnt[SN_PUSH_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0};             // (records .. noisy, reads_with_events: wave-uniform sums of ballots; the others: this lane's)
    ull or1 = 0, nand1 = 0, or2 = 0, nand2 = 0;                   // (this lane's keys; merged over the wave at the end)
    int nk = 0;                                                   // keys of the tile so far (uniform over the workgroup)
    for (long long first = lo; first < hi; first += INDEL_BLOCK) {       // (uniform: the bounds are the workgroup's)
        // ---- lane = read: the filters on the columns
        const long long i = first + t;
        bool elig = false;
        if (i < hi) elig = (I.flag[i] & 0xF04u) == 0 && I.tid[i] >= 0 && (unsigned)I.mapq[i] >= min_mapq;
        const ull m_rec = __ballot(i < hi), m_el = __ballot(elig);
        cnt[SN_RECORDS] += (ull)__popcll(m_rec);
        cnt[SN_ELIGIBLE] += (ull)__popcll(m_el);
        const tdt_slots S = tdt_block_slots<INDEL_BLOCK / 64>(m_el, s_wsum, lane, wave);
        if (elig) s_read[S.base + tdt_lane_rank(m_el, lane)] = (int)i;
        __syncthreads();
        // ---- lane = compacted read: bound the record, walk its CIGAR once
        const bool live = t < S.total;
        bool bad = live;
        unsigned ne = 0, un = 0, tl = 0;                           // keyed events seen (all of them), unanchored, too long
        unsigned eP[TDT_INDEL_MAX_PER_READ] = {0, 0, 0, 0}, eL[TDT_INDEL_MAX_PER_READ] = {0, 0, 0, 0}, eQ[TDT_INDEL_MAX_PER_READ] = {0, 0, 0, 0};
        unsigned rev = 0;
        int tid = 0, l_seq = 0;
        ull seq = 0;
        const uint8_t *__restrict__ raw = I.raw;
        if (live) {
            const int ri = s_read[t];
            rev = ((unsigned)I.flag[ri] >> 4) & 1u;
            tid = I.tid[ri];
            const int pos = I.pos[ri];
            const ull ro = I.rec_off[ri];
            if (tid < INDEL_MAX_CONTIGS && pos >= 0 && TDT_REC_HEADER_INSIDE(raw_len, ro)) {
                tdt_rec R = TDT_REC_READ(raw, ro);
                l_seq = R.l_seq;
                R.l_seq = l_seq < 0 ? 0 : l_seq;                   // (clamped: the body's sum never sees a negative length)
                if (l_seq >= 0 && TDT_REC_FITS(R, raw_len)) {
                    bad = false;
                    seq = R.seq();
                    const uint8_t *cig = raw + R.cig();
                    long long r = pos, q = 0;
                    unsigned prev = 9u;                            // (no op in front: no match code)
                    unsigned cw = R.n_cig ? tdt_ld_u32(cig) : 0u;
                    for (unsigned j = 0; j < R.n_cig; j++) {
                        const bool has_next = j + 1 < R.n_cig;
                        const unsigned nw = has_next ? tdt_ld_u32(cig + 4ull * (j + 1)) : 0u;
                        const unsigned nop = has_next ? nw & 0xfu : 9u;
                        const unsigned op = cw & 0xfu, len = cw >> 4;
                        bad |= op > 8;
                        if (op == 1 || op == 2) {
                            if (!(indel_is_match(prev) && indel_is_match(nop)) || len == 0) {
                                un++;
                            } else if (len >= TDT_INDEL_MAX_LEN) {
                                tl++;
                            } else {
                                bad |= r < 1 || r >= INDEL_P_LIMIT;
                                const unsigned qs = q > 0x7fffffffll ? 0x7fffffffu : (unsigned)q;      // (saturated: such a span lies outside any l_seq)
#pragma unroll
                                for (int k = 0; k < TDT_INDEL_MAX_PER_READ; k++)
                                    if (ne == (unsigned)k) eP[k] = (unsigned)r, eL[k] = (len << 1) | (op == 1 ? 1u : 0u), eQ[k] = qs;
                                ne++;
                            }
                        }
                        r += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? (long long)len : 0;
                        q += (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ? (long long)len : 0;
                        prev = op;
                        cw = nw;
                    }
                }
            }
        }
        const bool walked = live && !bad, noisy = walked && ne > TDT_INDEL_MAX_PER_READ, ok = walked && !noisy;
        cnt[SN_MALFORMED] += (ull)__popcll(__ballot(live && bad));
        cnt[SN_NOISY] += (ull)__popcll(__ballot(noisy));
        cnt[SN_READS_WITH_EVENTS] += (ull)__popcll(__ballot(ok && ne > 0));
        if (walked) cnt[SN_UNANCHORED] += un, cnt[SN_TOO_LONG] += tl;
        // ---- NORM: every event of an ok read moves as far left as the reference lets it (lanes shift by different amounts: each runs
        // its own short loop; a lane without events does nothing)
        unsigned eK[TDT_INDEL_MAX_PER_READ] = {0, 0, 0, 0};
        ull roff = 0;
        if constexpr (NORM) {
            if (ok && ne > 0) {
                const int rlen = tid < Rf.n ? Rf.len[tid] : -1;    // (< 0: the contig is not loaded)
                if (rlen >= 0) roff = Rf.off[tid];
#pragma unroll
                for (int k = 0; k < TDT_INDEL_MAX_PER_READ; k++) {
                    if ((unsigned)k < ne) {
                        const unsigned len = eL[k] >> 1;
                        const bool ins = eL[k] & 1u;
                        if (ins && (ull)eQ[k] + len > (ull)l_seq) continue;                      // (SEQ *: never shifted, not counted)
                        if (rlen < 0 || (ull)eP[k] + (ins ? 0ull : (ull)len) > (ull)rlen) {
                            noff++;
                            continue;
                        }
                        const unsigned ks = indel_shift(Rf.store, roff, eP[k], len, ins, raw, seq, eQ[k]);
                        eK[k] = ks;
                        nshift += ks > 0;
                        ncap += ks == INDEL_NORM_MAX_SHIFT;
                    }
                }
            }
        }
        // ---- the round's keys behind the tile's earlier ones, in LDS: slots by a prefix sum of the reads' event counts
        const int mine = ok ? (int)ne : 0;
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o);
            if (lane >= o) incl += u;
        }
        if (lane == 63) s_wkeys[wave] = incl;
        __syncthreads();
        int base = nk, total = 0;
#pragma unroll
        for (int w = 0; w < INDEL_BLOCK / 64; w++) {
            base += w < wave ? s_wkeys[w] : 0;
            total += s_wkeys[w];
        }
        int slot = base + incl - mine;                             // (+ mine <= nk + total <= 4 x the reads of the tile so far)
#pragma unroll
        for (int k = 0; k < TDT_INDEL_MAX_PER_READ; k++) {
            if (k < mine) {
                const unsigned len = eL[k] >> 1;
                const ull k1 = ((ull)(unsigned)tid << 32) | (ull)(NORM ? eP[k] - eK[k] : eP[k]);
                ull k2;
                if (eL[k] & 1u) {
                    if (NORM && eK[k]) k2 = indel_ins_key_rotated(raw, seq, eQ[k], len, Rf.store, roff, eP[k], eK[k]) | rev;
                    else k2 = indel_ins_key(raw, seq, eQ[k], len, l_seq) | rev;
                    cnt[SN_INSERTIONS]++;
                } else {
                    k2 = ((ull)len << 47) | rev;
                    cnt[SN_DELETIONS]++;
                }
                or1 |= k1, nand1 |= ~k1, or2 |= k2, nand2 |= ~k2;
                s_k1[slot + k] = k1;
                s_k2[slot + k] = k2;
            }
        }
        nk += total;
    }
    // ---- the tile's counters: merged per wave, then over the workgroup, ONE atomic per non-zero counter
    cnt[SN_UNANCHORED] = tdt_wave_reduce<tdt_sum>(cnt[SN_UNANCHORED]), cnt[SN_TOO_LONG] = tdt_wave_reduce<tdt_sum>(cnt[SN_TOO_LONG]);
    cnt[SN_INSERTIONS] = tdt_wave_reduce<tdt_sum>(cnt[SN_INSERTIONS]), cnt[SN_DELETIONS] = tdt_wave_reduce<tdt_sum>(cnt[SN_DELETIONS]);
    or1 = tdt_wave_reduce<tdt_or>(or1), nand1 = tdt_wave_reduce<tdt_or>(nand1), or2 = tdt_wave_reduce<tdt_or>(or2), nand2 = tdt_wave_reduce<tdt_or>(nand2);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SN_PUSH_N; k++) s_cnt[wave][k] = cnt[k];
        s_cnt[wave][SN_PUSH_N] = or1, s_cnt[wave][SN_PUSH_N + 1] = nand1, s_cnt[wave][SN_PUSH_N + 2] = or2, s_cnt[wave][SN_PUSH_N + 3] = nand2;
    }
    if constexpr (NORM) {
        nshift = tdt_wave_reduce<tdt_sum>(nshift), ncap = tdt_wave_reduce<tdt_sum>(ncap), noff = tdt_wave_reduce<tdt_sum>(noff);
        if (lane == 0) s_norm[wave][0] = nshift, s_norm[wave][1] = ncap, s_norm[wave][2] = noff;
    }
    __syncthreads();
    if constexpr (NORM) {
        if (t >= 64 && t < 64 + 3) {                               // (a wave the push counters' atomics leave idle)
            ull v = 0;
            for (int w = 0; w < INDEL_BLOCK / 64; w++) v += s_norm[w][t - 64];
            if (v) atomicAdd(&st[ST_SHIFTED + (t - 64)], v);
        }
    }
    if (t == 0) s_base = nk ? atomicAdd(&st[ST_N], (ull)nk) : 0ull;        // the workgroup's slots of the store behind ONE atomic
    if (t < SN_PUSH_N + 4) {
        ull v = 0;
        for (int w = 0; w < INDEL_BLOCK / 64; w++) v = t < SN_PUSH_N ? v + s_cnt[w][t] : v | s_cnt[w][t];
        if (v) {
            if (t < SN_PUSH_N) atomicAdd(&st[t], v);
            else atomicOr(&st[ST_OR1 + (t - SN_PUSH_N)], v);
        }
    }
    __syncthreads();
    for (int k = t; k < nk; k += INDEL_BLOCK) {                    // (consecutive lanes, consecutive slots)
        const ull slot = s_base + (ull)k;
        if (slot < cap) {
            k1s[slot] = s_k1[k];
            k2s[slot] = s_k2[k];
        } else {
            st[ST_OVERFLOW] = 1;                                   // (cannot happen: the host reserved 4 slots for every read of the batch)
        }
    }
}

// ---- the finish
__global__ __launch_bounds__(INDEL_BLOCK) void indel_iota(unsigned *__restrict__ v, int n) {
    const int i = blockIdx.x * INDEL_BLOCK + threadIdx.x;
    if (i < n) v[i] = (unsigned)i;
}

__global__ __launch_bounds__(INDEL_BLOCK) void indel_gather(ull *__restrict__ dst, const ull *__restrict__ src, const unsigned *__restrict__ perm, int n) {
    const int i = blockIdx.x * INDEL_BLOCK + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

// inclusive scan over the workgroup's 256 threads, in thread order (Op: tdt_max or tdt_sum; `none` its neutral element);
// *total = the reduction of all (s: INDEL_BLOCK / 64 words)
template <class Op> __device__ __forceinline__ int indel_block_scan(int v, int none, int *s, int t, int *total) {
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v = Op::of(v, u);
    }
    if (lane == 63) s[wave] = v;
    __syncthreads();
    int all = none;
#pragma unroll
    for (int w = 0; w < INDEL_BLOCK / 64; w++) {
        const int c = s[w];
        if (w < wave) v = Op::of(v, c);
        all = Op::of(all, c);
    }
    __syncthreads();
    *total = all;
    return v;
}

// a run head: the first key, or a key whose (K1, K2 >> 1) differs from the one in front of it; a full head: (K1, K2) differs
__device__ __forceinline__ bool indel_head(const ull *__restrict__ a, const ull *__restrict__ b, int i) {
    return i == 0 || a[i] != a[i - 1] || (b[i] >> 1) != (b[i - 1] >> 1);
}
__device__ __forceinline__ bool indel_full_head(const ull *__restrict__ a, const ull *__restrict__ b, int i) {
    return i == 0 || a[i] != a[i - 1] || b[i] != b[i - 1];
}

// tile_last[tile] = the position of the tile's last run head, tile_last[ntiles + tile] = of its last full head; -1 when it has none
__global__ __launch_bounds__(INDEL_BLOCK) void indel_tile_heads(const ull *__restrict__ a, const ull *__restrict__ b, int n, int ntiles,
                                                                int *__restrict__ tile_last) {
    __shared__ int s[INDEL_BLOCK / 64];
    const int t = threadIdx.x;
    const int t0 = blockIdx.x * INDEL_TILE;
    int best = -1, bestf = -1;
    for (int r = 0; r < INDEL_TILE / INDEL_BLOCK; r++) {
        const int i = t0 + r * INDEL_BLOCK + t;
        if (i < n) {
            if (indel_head(a, b, i)) best = i;                     // (i grows with r)
            if (indel_full_head(a, b, i)) bestf = i;
        }
    }
    int all, allf;
    (void)indel_block_scan<tdt_max>(best, -1, s, t, &all);
    (void)indel_block_scan<tdt_max>(bestf, -1, s, t, &allf);
    if (t == 0) tile_last[blockIdx.x] = all, tile_last[ntiles + blockIdx.x] = allf;
}

// ONE workgroup: both halves of tile_last become running maxima over the tiles
__global__ __launch_bounds__(INDEL_BLOCK) void indel_carry(int *__restrict__ tile_last, int ntiles) {
    __shared__ int s[INDEL_BLOCK / 64];
    const int t = threadIdx.x;
    for (int half = 0; half < 2; half++) {
        int *v_ = tile_last + (size_t)half * ntiles;
        int running = -1;
        for (int c = 0; c < ntiles; c += INDEL_BLOCK) {            // (uniform)
            const int k = c + t;
            int all;
            int v = indel_block_scan<tdt_max>(k < ntiles ? v_[k] : -1, -1, s, t, &all);
            v = v > running ? v : running;
            if (k < ntiles) v_[k] = v;
            running = all > running ? all : running;
        }
    }
}

// ONE workgroup: tile_kept[k] = the kept runs of the tiles in front of tile k (an exclusive sum; the total is below 2^30)
__global__ __launch_bounds__(INDEL_BLOCK) void indel_carry_sum(int *__restrict__ tile_kept, int ntiles) {
    __shared__ int s[INDEL_BLOCK / 64];
    const int t = threadIdx.x;
    int running = 0;
    for (int c = 0; c < ntiles; c += INDEL_BLOCK) {                // (uniform)
        const int k = c + t;
        const int mine = k < ntiles ? tile_kept[k] : 0;
        int all;
        const int v = indel_block_scan<tdt_sum>(mine, 0, s, t, &all);
        if (k < ntiles) tile_kept[k] = running + v - mine;
        running += all;
    }
}

// every run measured at its end.  WRITE false: tile_kept[tile] = the runs of the tile with size >= min_support, out[0] += its runs,
// out[1] += the kept ones.  WRITE true: tile_kept holds the exclusive sums and the kept runs become rows, in key order.
template <bool WRITE>
__global__ __launch_bounds__(INDEL_BLOCK) void indel_runs(const ull *__restrict__ a, const ull *__restrict__ b, int n, int ntiles,
                                                          const int *__restrict__ tile_last, int *__restrict__ tile_kept, unsigned min_support,
                                                          ull *__restrict__ out, ull *__restrict__ r_k1, ull *__restrict__ r_k2,
                                                          unsigned *__restrict__ r_sup, unsigned *__restrict__ r_rev) {
    __shared__ int s[INDEL_BLOCK / 64];
    __shared__ int s_w[INDEL_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int t0 = blockIdx.x * INDEL_TILE;
    int running = blockIdx.x ? tile_last[blockIdx.x - 1] : -1, runningf = blockIdx.x ? tile_last[ntiles + blockIdx.x - 1] : -1;
    int kept = 0, runs = 0;                                        // (uniform over the workgroup)
    const int row0 = WRITE ? tile_kept[blockIdx.x] : 0;
    for (int r = 0; r < INDEL_TILE / INDEL_BLOCK; r++) {           // (uniform: every thread takes every round)
        const int i = t0 + r * INDEL_BLOCK + t;
        const bool valid = i < n;
        ull ka = 0, kb = 0;
        bool head = false, fhead = false, end = false;
        if (valid) {
            ka = a[i];
            kb = b[i];
            head = indel_head(a, b, i);
            fhead = indel_full_head(a, b, i);
            end = i == n - 1 || a[i + 1] != ka || (b[i + 1] >> 1) != (kb >> 1);
        }
        int all, allf;
        int last = indel_block_scan<tdt_max>(head ? i : -1, -1, s, t, &all);
        int lastf = indel_block_scan<tdt_max>(fhead ? i : -1, -1, s, t, &allf);
        last = last > running ? last : running;
        lastf = lastf > runningf ? lastf : runningf;
        running = all > running ? all : running;
        runningf = allf > runningf ? allf : runningf;
        const unsigned size = end ? (unsigned)(i - last + 1) : 0u;
        const bool keep = end && size >= min_support;
        const ull m_keep = __ballot(keep), m_end = __ballot(end);
        const tdt_slots S = tdt_block_slots<INDEL_BLOCK / 64>(m_keep, s_w, lane, wave);
        if (WRITE && keep) {
            const size_t row = (size_t)row0 + (size_t)(kept + S.base + tdt_lane_rank(m_keep, lane));       // (< n: a row per run)
            r_k1[row] = ka;
            r_k2[row] = kb & ~1ull;
            r_sup[row] = size;
            r_rev[row] = (kb & 1ull) ? (unsigned)(i - lastf + 1) : 0u;
        }
        kept += S.total;
        if (!WRITE) {
            const tdt_slots E = tdt_block_slots<INDEL_BLOCK / 64>(m_end, s, lane, wave);
            runs += E.total;
            __syncthreads();                                       // (s is the next round's scan buffer)
        }
    }
    if (!WRITE && t == 0) {
        tile_kept[blockIdx.x] = kept;
        if (runs) atomicAdd(&out[0], (ull)runs);
        if (kept) atomicAdd(&out[1], (ull)kept);
    }
}

static void indel_free(tdt_indel *h) {
    if (h->k1) (void)hipFree(h->k1);
    if (h->k2) (void)hipFree(h->k2);
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->io.d) (void)hipFree(h->io.d);
    if (h->d_work) (void)hipFree(h->d_work);
    for (int k = 0; k < 5; k++)
        if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
    delete h;
}

// two device arrays of `cap` store entries; on failure nothing is left allocated
static hipError_t indel_alloc_store(size_t cap, ull **k1, ull **k2) {
    *k1 = *k2 = nullptr;
    if (tdt_dev_malloc((void **)k1, cap * 8) == hipSuccess && tdt_dev_malloc((void **)k2, cap * 8) == hipSuccess) return hipSuccess;
    if (*k1) (void)hipFree(*k1);
    if (*k2) (void)hipFree(*k2);
    *k1 = *k2 = nullptr;
    return hipErrorOutOfMemory;
}

extern "C" size_t tdt_indel_sn_size(void) { return TDT_INDEL_SN_N; }

extern "C" int tdt_indel_create(tdt_ctx *ctx, int n_contigs, int min_mapq, size_t capacity, tdt_indel **out) {
    if (!ctx || !out || n_contigs < 0) {
        tdt_set_error("tdt_indel_create: bad argument");
        return TDT_E_ARG;
    }
    if (n_contigs > INDEL_MAX_CONTIGS || min_mapq < 0 || min_mapq > 255 || capacity >= (1ull << 40)) {
        tdt_set_error("tdt_indel_create: %d contigs (at most 2^24), min_mapq %d (0 ... 255), capacity %zu", n_contigs, min_mapq, capacity);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_indel *h = new tdt_indel{};
    h->ctx = ctx;
    h->n_contigs = n_contigs;
    h->min_mapq = min_mapq;
    if (tdt_dev_malloc((void **)&h->d_state, ST_WORDS * 8) != hipSuccess || (capacity && indel_alloc_store(capacity, &h->k1, &h->k2) != hipSuccess)) {
        indel_free(h);
        tdt_set_error("tdt_indel_create: out of device memory (%zu keys)", capacity);
        return TDT_E_NOMEM;
    }
    h->cap = capacity;
    hipError_t e = hipMemsetAsync(h->d_state, 0, ST_WORDS * 8, ctx->stream);
    for (int k = 0; k < 5 && e == hipSuccess; k++) e = hipEventCreate(&h->ev[k]);
    if (e != hipSuccess) {
        indel_free(h);
        TDT_HIP(e);
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_indel_destroy(tdt_indel *h) {
    if (!h) return TDT_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);        // (no kernel of the stream still writes the store)
    indel_free(h);
    return TDT_OK;
}

extern "C" int tdt_indel_reset(tdt_indel *h) {
    if (!h) {
        tdt_set_error("tdt_indel_reset: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    TDT_HIP(hipMemsetAsync(h->d_state, 0, ST_WORDS * 8, h->ctx->stream));
    h->upper = 0;
    h->n_rows = 0;
    h->rows_valid = false;
    return TDT_OK;
}

// how many keys the store holds (the stream is synchronised)
static int indel_stored(tdt_indel *h, ull *state) {
    hipStream_t st = h->ctx->stream;
    TDT_HIP(hipMemcpyAsync(state, h->d_state, ST_WORDS * 8, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    if (state[ST_OVERFLOW] || state[ST_N] > h->cap) {
        tdt_set_error("tdt_indel: the key store overflowed (%llu keys, capacity %zu)", state[ST_N], h->cap);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

// room for `more` keys behind the (at most) h->upper stored ones, as dup_reserve makes it: a growth first asks the device how many
// keys there really are; then a bigger store (1.5 x), the keys so far copied over on the device, the old one freed once the copy is done.
static int indel_reserve(tdt_indel *h, size_t more) {
    if (h->upper + more <= h->cap) return TDT_OK;
    ull state[ST_WORDS];
    int rc = indel_stored(h, state);
    if (rc) return rc;
    h->asks++;
    h->upper = (size_t)state[ST_N];
    if (h->upper + more <= h->cap) return TDT_OK;
    size_t want = h->cap + h->cap / 2;
    if (want < h->upper + more) want = h->upper + more;
    ull *k1, *k2;
    if (indel_alloc_store(want, &k1, &k2) != hipSuccess) {
        tdt_set_error("tdt_indel: out of device memory growing to %zu keys", want);
        return TDT_E_NOMEM;
    }
    hipStream_t st = h->ctx->stream;
    hipError_t e = hipSuccess;
    if (h->upper) {
        e = hipMemcpyAsync(k1, h->k1, h->upper * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(k2, h->k2, h->upper * 8, hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(k1), (void)hipFree(k2);
        TDT_HIP(e);
    }
    if (h->k1) (void)hipFree(h->k1);
    if (h->k2) (void)hipFree(h->k2);
    h->k1 = k1, h->k2 = k2;
    h->cap = want;
    h->grows++;
    return TDT_OK;
}

static int indel_launch(tdt_indel *h, const IndelIn &I, size_t n, size_t raw_len) {
    const size_t room = n * TDT_INDEL_MAX_PER_READ;                // the bound a read's cap gives
    int rc = indel_reserve(h, room);
    if (rc) return rc;
    const dim3 grid((unsigned)((n + INDEL_K_TILE - 1) / INDEL_K_TILE));
    if (h->ref)
        hipLaunchKernelGGL(indel_keys<true>, grid, dim3(INDEL_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, h->k1, h->k2,
                           (ull)h->cap, h->d_state, tdt_refview{h->ref->d_store, h->ref->d_off, h->ref->d_len, h->ref->n_contigs});
    else
        hipLaunchKernelGGL(indel_keys<false>, grid, dim3(INDEL_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, h->k1, h->k2,
                           (ull)h->cap, h->d_state, tdt_refview{nullptr, nullptr, nullptr, 0});
    TDT_CHECK_LAUNCH();
    h->upper += room;
    h->rows_valid = false;
    return TDT_OK;
}

#define INDEL_NEED (TDT_NEED(FLAG) | TDT_NEED(TID) | TDT_NEED(POS) | TDT_NEED(MAPQ) | TDT_NEED(REC_OFF) | TDT_NEED(RAW))

// One batch of the device ingest: d_arrays14 = the pointer table tdt_ingest_arrays filled (TDT_COL_*: a host array of TDT_NCOL device
// pointers).  The launch is enqueued on the context's stream and nothing is waited for — unless the reserve must ask or grow.
extern "C" int tdt_indel_push_device(tdt_indel *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    tdt_batch B;
    const int rc = tdt_batch_view("tdt_indel_push_device", h, d_arrays14, n, raw_len, INDEL_NEED, &B);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    return indel_launch(h, IndelIn{B.flag, B.tid, B.pos, B.mapq, B.rec_off, B.raw}, n, raw_len);
}

// The same kernel on host columns and host record bytes (uploaded into the handle's own block).  The stream is synchronised before the
// return: the caller's arrays are free again.
extern "C" int tdt_indel_push(tdt_indel *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off,
                              size_t n, const uint8_t *raw, size_t raw_len) {
    tdt_batch H{}, B;
    H.flag = flag, H.tid = tid, H.pos = pos, H.mapq = mapq, H.rec_off = rec_off, H.raw = raw;
    int rc = tdt_batch_host("tdt_indel_push", h, H, n, raw_len, INDEL_NEED);
    if (rc == TDT_OK) rc = tdt_batch_offsets_ascend("tdt_indel_push", rec_off, n);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    rc = tdt_batch_upload("tdt_indel_push", h->ctx, &h->io, H, INDEL_NEED, n, raw_len, &B);
    if (rc == TDT_OK) rc = indel_launch(h, IndelIn{B.flag, B.tid, B.pos, B.mapq, B.rec_off, B.raw}, n, raw_len);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

// The store read out, in the order it lies in HBM.  On entry *n = the room of the two arrays (ignored when both are NULL: the call then
// only reports the count); on return *n = the keys stored.  Too little room: TDT_E_RANGE, nothing written.
extern "C" int tdt_indel_keys(tdt_indel *h, uint64_t *k1, uint64_t *k2, size_t *n) {
    if (!h || !n || ((k1 || k2) && !(k1 && k2))) {
        tdt_set_error("tdt_indel_keys: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    ull state[ST_WORDS];
    int rc = indel_stored(h, state);
    if (rc) return rc;
    const size_t have = (size_t)state[ST_N];
    if (k1) {
        if (*n < have) {
            tdt_set_error("tdt_indel_keys: room for %zu keys, %zu stored", *n, have);
            return TDT_E_RANGE;
        }
        hipStream_t st = h->ctx->stream;
        if (have) {
            TDT_HIP(hipMemcpyAsync(k1, h->k1, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(k2, h->k2, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
        }
    }
    *n = have;
    return TDT_OK;
}

struct IndelWork {
    ull *ka, *kb, *d_out, *r_k1, *r_k2;
    unsigned *ia, *ib, *r_sup, *r_rev;
    int *tile_last, *tile_kept;
    size_t lay(void *base, size_t n, size_t ntiles) {
        tdt_carver cv(base);
        ka = cv.take<ull>(n), kb = cv.take<ull>(n), ia = cv.take<unsigned>(n), ib = cv.take<unsigned>(n);
        r_k1 = cv.take<ull>(n), r_k2 = cv.take<ull>(n), r_sup = cv.take<unsigned>(n), r_rev = cv.take<unsigned>(n);
        tile_last = cv.take<int>(2 * ntiles), tile_kept = cv.take<int>(ntiles), d_out = cv.take<ull>(2);
        return cv.size;
    }
};

// the sort mask of a key column: every bit from the lowest to the highest one that differs between two stored keys (one run of set
// bits: at most eight digits, whatever a hashed payload looks like)
static ull indel_mask(ull differ) {
    if (!differ) return 0;
    const int lo = __builtin_ctzll(differ), hi = 63 - __builtin_clzll(differ);
    return (hi == 63 ? ~0ull : (1ull << (hi + 1)) - 1ull) & ~((1ull << lo) - 1ull);
}

// sn_out: uint64[TDT_INDEL_SN_N], the push counters and the sets of everything pushed so far; *n_rows: the rows tdt_indel_rows will
// give.  The store is left as it was.
extern "C" int tdt_indel_finish(tdt_indel *h, uint64_t min_support, uint64_t *sn_out, size_t *n_rows) {
    if (!h || !sn_out || !n_rows) {
        tdt_set_error("tdt_indel_finish: bad argument");
        return TDT_E_ARG;
    }
    if (min_support < 1 || min_support > TDT_INDEL_MAX_SUPPORT) {
        tdt_set_error("tdt_indel_finish: min_support %llu (1 ... %d)", (ull)min_support, TDT_INDEL_MAX_SUPPORT);
        return TDT_E_RANGE;
    }
    tdt_ctx *ctx = h->ctx;
    TDT_HIP(hipSetDevice(ctx->device));
    ull state[ST_WORDS];
    int rc = indel_stored(h, state);
    if (rc) return rc;
    const size_t n_ = (size_t)state[ST_N];
    if (n_ >= (1ull << 30)) {
        tdt_set_error("tdt_indel_finish: %zu keys; the sort handles fewer than 2^30", n_);
        return TDT_E_RANGE;
    }
    uint64_t res[SN_N] = {};
    for (int k = 0; k < SN_PUSH_N; k++) res[k] = state[k];
    for (int k = 0; k < 4; k++) h->ms[k] = 0;
    h->rows_valid = false;
    h->n_rows = 0;
    if (n_) {
        const int n = (int)n_;
        const size_t ntiles = (n_ + INDEL_TILE - 1) / INDEL_TILE;
        IndelWork W;
        const size_t bytes = W.lay(nullptr, n_, ntiles);
        if (bytes > h->work_cap) {
            if (h->d_work) TDT_HIP(hipFree(h->d_work));
            h->d_work = nullptr;
            h->work_cap = 0;
            if (tdt_dev_malloc(&h->d_work, bytes) != hipSuccess) {
                tdt_set_error("tdt_indel_finish: out of device memory (%zu keys)", n_);
                return TDT_E_NOMEM;
            }
            h->work_cap = bytes;
        }
        W.lay(h->d_work, n_, ntiles);
        hipStream_t st = ctx->stream;
        const unsigned grid = (unsigned)((n_ + INDEL_BLOCK - 1) / INDEL_BLOCK);
        TDT_HIP(hipMemsetAsync(W.d_out, 0, 2 * 8, st));
        TDT_HIP(hipMemcpyAsync(W.ka, h->k2, n_ * 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(indel_iota, dim3(grid), dim3(INDEL_BLOCK), 0, st, W.ia, n);
        TDT_CHECK_LAUNCH();
        // PRECONDITION of tdt_radix_sort_pairs: the key bits outside the mask are equal in ALL keys.  The push kept the OR of the keys
        // and of their complements: a bit differs exactly when it is set in both, and indel_mask covers every such bit.
        const ull mask1 = indel_mask(state[ST_OR1] & state[ST_NAND1]), mask2 = indel_mask(state[ST_OR2] & state[ST_NAND2]);
        ull *k2s, *k1s;
        unsigned *perm, *perm2;
        TDT_HIP(hipEventRecord(h->ev[0], st));
        rc = tdt_radix_sort_pairs(ctx, W.ka, W.ia, W.kb, W.ib, n_, mask2, &k2s, &perm);
        if (rc) return rc;
        TDT_HIP(hipEventRecord(h->ev[1], st));
        ull *free_k = k2s == W.ka ? W.kb : W.ka;                   // (the sorted K2 are not needed again: K2 comes from the store below)
        unsigned *free_i = perm == W.ia ? W.ib : W.ia;
        hipLaunchKernelGGL(indel_gather, dim3(grid), dim3(INDEL_BLOCK), 0, st, free_k, (const ull *)h->k1, (const unsigned *)perm, n);
        TDT_CHECK_LAUNCH();
        TDT_HIP(hipEventRecord(h->ev[2], st));
        rc = tdt_radix_sort_pairs(ctx, free_k, perm, k2s, free_i, n_, mask1, &k1s, &perm2);           // (the same precondition, mask1)
        if (rc) return rc;
        TDT_HIP(hipEventRecord(h->ev[3], st));
        ull *k2f = k1s == W.ka ? W.kb : W.ka;
        const int nt = (int)ntiles;
        hipLaunchKernelGGL(indel_gather, dim3(grid), dim3(INDEL_BLOCK), 0, st, k2f, (const ull *)h->k2, (const unsigned *)perm2, n);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(indel_tile_heads, dim3((unsigned)ntiles), dim3(INDEL_BLOCK), 0, st, (const ull *)k1s, (const ull *)k2f, n, nt, W.tile_last);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(indel_carry, dim3(1), dim3(INDEL_BLOCK), 0, st, W.tile_last, nt);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(indel_runs<false>, dim3((unsigned)ntiles), dim3(INDEL_BLOCK), 0, st, (const ull *)k1s, (const ull *)k2f, n, nt,
                           (const int *)W.tile_last, W.tile_kept, (unsigned)min_support, W.d_out, W.r_k1, W.r_k2, W.r_sup, W.r_rev);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(indel_carry_sum, dim3(1), dim3(INDEL_BLOCK), 0, st, W.tile_kept, nt);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(indel_runs<true>, dim3((unsigned)ntiles), dim3(INDEL_BLOCK), 0, st, (const ull *)k1s, (const ull *)k2f, n, nt,
                           (const int *)W.tile_last, W.tile_kept, (unsigned)min_support, W.d_out, W.r_k1, W.r_k2, W.r_sup, W.r_rev);
        TDT_CHECK_LAUNCH();
        TDT_HIP(hipEventRecord(h->ev[4], st));
        ull got[2] = {0, 0};
        TDT_HIP(hipMemcpyAsync(got, W.d_out, 2 * 8, hipMemcpyDeviceToHost, st));
        rc = tdt_ctx_sync(ctx);                                    // (also reports the sort's bounded-spin word)
        if (rc) return rc;
        res[SN_DISTINCT] = got[0];
        res[SN_REPORTED] = got[1];
        for (int k = 0; k < 4; k++) {
            float ms = 0;
            TDT_HIP(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
            h->ms[k] = ms;
        }
        h->r_k1 = W.r_k1, h->r_k2 = W.r_k2, h->r_sup = W.r_sup, h->r_rev = W.r_rev;
        h->n_rows = (size_t)got[1];
    }
    h->rows_valid = true;
    memcpy(sn_out, res, sizeof res);
    *n_rows = h->n_rows;
    return TDT_OK;
}

// The rows of the last finish, ascending by (K1, K2 >> 1): K1, K2 with bit 0 clear, SUPPORT, REV.  *n in: the room of the four arrays
// (ignored when all four are NULL), out: the rows.  A push or a reset since the finish: TDT_E_ARG.  Too little room: TDT_E_RANGE.
extern "C" int tdt_indel_rows(tdt_indel *h, uint64_t *k1, uint64_t *k2, uint32_t *support, uint32_t *rev, size_t *n) {
    const bool any = k1 || k2 || support || rev;
    if (!h || !n || (any && !(k1 && k2 && support && rev))) {
        tdt_set_error("tdt_indel_rows: bad argument");
        return TDT_E_ARG;
    }
    if (!h->rows_valid) {
        tdt_set_error("tdt_indel_rows: no finish since the last push or reset");
        return TDT_E_ARG;
    }
    const size_t have = h->n_rows;
    if (any) {
        if (*n < have) {
            tdt_set_error("tdt_indel_rows: room for %zu rows, %zu kept", *n, have);
            return TDT_E_RANGE;
        }
        if (have) {
            TDT_HIP(hipSetDevice(h->ctx->device));
            hipStream_t st = h->ctx->stream;
            TDT_HIP(hipMemcpyAsync(k1, h->r_k1, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(k2, h->r_k2, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(support, h->r_sup, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(rev, h->r_rev, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
        }
    }
    *n = have;
    return TDT_OK;
}

// device milliseconds of the last finish: [0] sort by K2, [1] gather of K1, [2] sort by K1, [3] gather of K2 + the run-length launches
extern "C" int tdt_indel_timing(tdt_indel *h, double *ms4) {
    if (!h || !ms4) {
        tdt_set_error("tdt_indel_timing: bad argument");
        return TDT_E_ARG;
    }
    for (int k = 0; k < 4; k++) ms4[k] = h->ms[k];
    return TDT_OK;
}

// out3: how often the reserve asked the device for the real count, how often it made a bigger store, the store's capacity now
extern "C" int tdt_indel_reserve_stats(tdt_indel *h, uint64_t *out3) {
    if (!h || !out3) {
        tdt_set_error("tdt_indel_reserve_stats: bad argument");
        return TDT_E_ARG;
    }
    out3[0] = h->asks, out3[1] = h->grows, out3[2] = h->cap;
    return TDT_OK;
}

// The reference the pushes from here on normalise against (tdt_refseq.hip; it must outlive the handle or be detached first, and lie on
// the handle's device); NULL detaches it: the keys are again what they are without one.  The store and the counters stay as they are.
extern "C" int tdt_indel_set_reference(tdt_indel *h, tdt_refseq *ref) {
    if (!h || (ref && ref->ctx->device != h->ctx->device)) {
        tdt_set_error("tdt_indel_set_reference: bad argument");
        return TDT_E_ARG;
    }
    h->ref = ref;
    return TDT_OK;
}

// out3: what the pushes with a reference attached counted since the last reset — events shifted (k > 0), shifts that stopped at
// INDEL_NORM_MAX_SHIFT, events off the reference (contig not loaded, or the event reaches beyond its end).  The stream is synchronised.
extern "C" int tdt_indel_norm_stats(tdt_indel *h, uint64_t *out3) {
    if (!h || !out3) {
        tdt_set_error("tdt_indel_norm_stats: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    ull state[ST_WORDS];
    const int rc = indel_stored(h, state);
    if (rc) return rc;
    out3[0] = state[ST_SHIFTED], out3[1] = state[ST_CAPPED], out3[2] = state[ST_OFFREF];
    return TDT_OK;
}
