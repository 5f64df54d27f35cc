// Duplicate metrics for gfx950 — how many duplicates the library of the --sv scan HAS (TIDDIT_DUPS=1), recomputed from the reads' unclipped
// 5' ends.  The definition is tiddit_dup.py's: per read a key (K1 = tid << 34 | E << 1 | rev, K2 = 0 for a fragment, 1 << 58 | mate_tid
// << 34 | ME << 1 | mrev for the carrier of a pair), the sets of equal (K1, K2) counted by size.  Every result is an order-independent
// integer, so it equals the definition exactly.
//   * dup_keys — ONE launch per batch, on the columns and record bytes that are already resident.  Lane = read for the filters and the
//     carrier rule (flag, tid, pos, mate_tid, mate_pos: coalesced columns); the reads that need their bytes — fragments and carriers,
//     about half of a paired file — are compacted inside the workgroup as al_count compacts its reads, then lane = compacted read:
//     the record is bounded exactly as tdt_qc / tdt_alleles bound one (nothing outside [rec_off, rec_off + 4 + block_size), itself
//     inside raw_len, is read afterwards), its CIGAR is walked ONCE (op codes, leading and trailing clip sums) and, for a carrier, its
//     aux fields ONCE for the first MC:Z — the first kernel here that walks aux fields.  A workgroup owns DUP_K_TILE consecutive reads,
//     DUP_BLOCK at a time; the keys of a round are compacted again behind the tile's earlier ones in LDS, and the tile's keys are
//     appended to the store (two uint64 columns and the 0x400 bit, in HBM) behind ONE atomic that reserves the workgroup's slots,
//     consecutive lanes writing consecutive slots: the store is in stream order, not file order, and nothing downstream depends on its
//     order.  The SN counters are ballots summed in wave-uniform registers, merged per wave and then over the workgroup: one atomic per
//     workgroup and non-zero counter.  (All of them share a cache line: one atomic per WAVE and counter, 820 000 of a 5.3-M read batch,
//     took 4.6 ms there — profiles/dup_240mb.md.)  The OR of the keys and of their complements is kept the same way: the bits that
//     differ between any two keys of the job, which is what the sort's masks must cover.
//     The store grows as tdt_evstore grows (1.5 x, copied on the device).  The host knows only an upper bound of the keys stored (a read
//     gives at most one): room for it is reserved BEFORE the launch, and a growth first asks the device for the real count.  The
//     kernel still tests every slot against the capacity it was given and raises a flag instead of writing: it never reads or writes
//     beyond capacity.
//   * tdt_dup_finish — once per job: an LSD sort of the whole store with tdt_radix_sort_pairs (sort (K2, index); gather K1 by the
//     permutation; sort (K1[perm], perm), stable), a gather of K2 into the final order, then the run lengths of equal (K1, K2) in
//     three plain launches: dup_tile_heads notes each tile's last run head, dup_carry (one workgroup) carries the heads across the
//     tiles, dup_runs measures every run at its END (position - last head + 1) and adds it to an LDS histogram whose non-zero words
//     leave by 64-bit atomics.  No workgroup of these kernels waits for another, and no loop is as long as a run: one run of n equal
//     keys costs what n distinct keys cost.
#include "tdt_batch.h"
#include "tdt_bam_record.h"

#include <vector>

typedef unsigned long long ull;

#define DUP_BLOCK 256
#define DUP_K_TILE 2048                       // reads of a dup_keys workgroup (and the most keys it stages in LDS: 34 KB)
#define DUP_TILE 4096                         // keys of a run-length workgroup: DUP_BLOCK lanes, DUP_TILE / DUP_BLOCK rounds
#define DUP_BIAS (1ll << 28)
#define DUP_E_LIMIT (1ll << 33)
#define DUP_MAX_CONTIGS (1 << 24)
#define DUP_PAIR_BIT (1ull << 58)
#define DUP_NUM_LIMIT (1u << 28)              // an MC number of this or more makes the text unusable

static_assert(TDT_DUP_TOTAL == TDT_DUP_OFF_HIST + 2 * TDT_DUP_HIST_MAX && TDT_DUP_OFF_HIST == TDT_DUP_SN_N, "the layout of include/tiddit_hip.h");
static_assert(DUP_TILE % DUP_BLOCK == 0 && DUP_K_TILE % DUP_BLOCK == 0, "whole rounds");

// the SN rows, in the order of the file; the first eight are the push's
enum { SN_RECORDS = 0, SN_ELIGIBLE, SN_MALFORMED, SN_FRAGMENTS, SN_PAIRS, SN_PAIR_MATES, SN_PAIRS_NO_MC, SN_FLAGGED, SN_FRAGMENT_SETS, SN_PAIR_SETS,
       SN_FRAGMENT_DUPS, SN_PAIR_DUPS, SN_N, SN_PUSH_N = SN_FRAGMENT_SETS };
static_assert(SN_N == TDT_DUP_SN_N, "SN rows");
// the state words behind the push counters: the OR of the keys and of their complements; the number of keys stored, which every
// workgroup adds to and waits for, in a cache line of its own
enum { ST_OR1 = SN_PUSH_N, ST_NAND1, ST_OR2, ST_NAND2, ST_N = 16, ST_OVERFLOW, ST_WORDS = 32 };
static_assert(ST_NAND2 < ST_N && ST_N * 8 % 128 == 0, "state layout");

struct tdt_dup {
    tdt_ctx *ctx;
    int n_contigs;
    long long max_len;
    ull *k1, *k2;                             // the store: cap entries each
    uint8_t *marked;
    size_t cap, upper;                        // upper: no more than this many keys are stored (the device knows how many)
    ull *d_state;                             // ST_WORDS
    tdt_batch_io io;                          // columns + raw bytes of the host entry
    void *d_work;                             // the finish's buffers (grows)
    size_t work_cap;
    hipEvent_t ev[5];
    double ms[4];
};

struct DupIn {
    const uint16_t *flag;
    const int32_t *tid, *pos, *end, *mate_tid, *mate_pos;
    const uint64_t *rec_off;
    const uint8_t *raw;
};

__device__ __forceinline__ bool dup_is_pair(unsigned f, int mtid) { return (f & 0x1u) && !(f & 0x8u) && mtid >= 0; }

// The first MC:Z of the aux fields raw[p, e): true when its text is usable, then the mate's clip sums and reference length.
__device__ __forceinline__ bool dup_mate_cigar(const uint8_t *__restrict__ raw, ull p, const ull e, ull &mlead, ull &mtrail, ull &mref) {
    while (p + 3 <= e) {
        const unsigned c0 = raw[p], c1 = raw[p + 1], ty = raw[p + 2];
        p += 3;
        const unsigned sz = (ty == 'A' || ty == 'c' || ty == 'C') ? 1u : (ty == 's' || ty == 'S') ? 2u : (ty == 'i' || ty == 'I' || ty == 'f') ? 4u : 0u;
        if (sz) {
            if (p + sz > e) return false;
            p += sz;
        } else if (ty == 'Z' || ty == 'H') {
            if (c0 == 'M' && c1 == 'C' && ty == 'Z') {
                bool valid = true, seen = false;
                unsigned num = 0, digits = 0, nops = 0;
                ull lead = 0, trail = 0, ref = 0;
                unsigned ch = 1;
                while (p < e && (ch = raw[p]) != 0) {
                    p++;
                    if (!valid) continue;
                    if (ch >= '0' && ch <= '9') {
                        const ull v = (ull)num * 10 + (ch - '0');
                        num = v > DUP_NUM_LIMIT ? DUP_NUM_LIMIT : (unsigned)v;      // (saturates)
                        digits++;
                        continue;
                    }
                    const bool clip = ch == 'S' || ch == 'H', onref = ch == 'M' || ch == 'D' || ch == 'N' || ch == '=' || ch == 'X';
                    if (!(clip || onref || ch == 'I' || ch == 'P') || !digits || num >= DUP_NUM_LIMIT) {
                        valid = false;
                        continue;
                    }
                    if (clip) {
                        if (seen) trail += num;
                        else lead += num;
                    } else {
                        seen = true;
                        trail = 0;
                        if (onref) ref += num;
                    }
                    nops++;
                    num = digits = 0;
                }
                if (ch != 0) return false;                                          // (no NUL inside the block)
                mlead = lead, mtrail = trail, mref = ref;
                return valid && nops && !digits;                                    // the first MC:Z wins, usable or not
            }
            while (p < e && raw[p] != 0) p++;
            if (p >= e) return false;
            p++;
        } else if (ty == 'B') {
            if (p + 5 > e) return false;
            const unsigned sub = raw[p];
            const unsigned bsz = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
            if (!bsz) return false;
            const ull bytes = 5ull + (ull)tdt_ld_u32(raw + p + 1) * bsz;
            if (p + bytes > e) return false;
            p += bytes;
        } else {
            return false;
        }
    }
    return false;
}

__global__ __launch_bounds__(DUP_BLOCK) void dup_keys(DupIn I, int n, ull raw_len, ull *__restrict__ k1s, ull *__restrict__ k2s,
                                                      uint8_t *__restrict__ ms, ull cap, ull *__restrict__ st) {
    __shared__ ull s_k1[DUP_K_TILE], s_k2[DUP_K_TILE];            // the tile's keys, in the order they were made (a read gives at most one)
    __shared__ uint8_t s_m[DUP_K_TILE];
    __shared__ int s_read[DUP_BLOCK];
    __shared__ int s_wsum[DUP_BLOCK / 64], s_wkeys[DUP_BLOCK / 64];
    __shared__ ull s_cnt[DUP_BLOCK / 64][SN_PUSH_N + 4];          // per wave: the push counters, then the OR / NAND words
    __shared__ ull s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long lo = (long long)blockIdx.x * DUP_K_TILE, hi = lo + DUP_K_TILE < n ? lo + DUP_K_TILE : n;
    ull cnt[SN_PUSH_N] = {0, 0, 0, 0, 0, 0, 0, 0};                // (wave-uniform: sums of ballots)
    ull or1 = 0, nand1 = 0, or2 = 0, nand2 = 0;                   // (this lane's keys; merged over the wave at the end)
    int nk = 0;                                                   // keys of the tile so far (uniform over the workgroup)
    for (long long first = lo; first < hi; first += DUP_BLOCK) {  // (uniform: the bounds are the workgroup's)
        // ---- lane = read: eligibility and the carrier rule on the columns
        const long long i = first + t;
        bool elig = false, need = false;
        if (i < hi) {
            const unsigned f = I.flag[i];
            const int tid = I.tid[i];
            if ((f & 0xB04u) == 0 && tid >= 0) {
                elig = need = true;
                const int mtid = I.mate_tid[i];
                if (dup_is_pair(f, mtid)) {
                    const int pos = I.pos[i], mpos = I.mate_pos[i];
                    need = tid < mtid || (tid == mtid && (pos < mpos || (pos == mpos && (f & 0x40u))));
                }
            }
        }
        const ull m_rec = __ballot(i < hi), m_el = __ballot(elig), m_need = __ballot(need);
        cnt[SN_RECORDS] += (ull)__popcll(m_rec);
        cnt[SN_ELIGIBLE] += (ull)__popcll(m_el);
        cnt[SN_PAIR_MATES] += (ull)__popcll(m_el & ~m_need);
        const tdt_slots S = tdt_block_slots<DUP_BLOCK / 64>(m_need, s_wsum, lane, wave);
        if (need) s_read[S.base + tdt_lane_rank(m_need, lane)] = (int)i;
        __syncthreads();
        // ---- lane = compacted read: bound the record, walk its CIGAR once and (a carrier) its aux fields once
        const bool live = t < S.total;
        bool ok = false, pair = false, no_mc = false;
        unsigned f = 0;
        ull k1 = 0, k2 = 0;
        if (live) {
            const int ri = s_read[t];
            f = I.flag[ri];
            const int tid = I.tid[ri], mtid = I.mate_tid[ri];
            pair = dup_is_pair(f, mtid);
            const ull ro = I.rec_off[ri];
            if (tid < DUP_MAX_CONTIGS && !(pair && mtid >= DUP_MAX_CONTIGS) && TDT_REC_HEADER_INSIDE(raw_len, ro)) {
                const uint8_t *__restrict__ raw = I.raw;
                tdt_rec R = TDT_REC_READ(raw, ro);
                const int l_seq = R.l_seq;
                R.l_seq = l_seq < 0 ? 0 : l_seq;                   // (clamped: the body's sum never sees a negative length)
                if (l_seq >= 0 && TDT_REC_FITS(R, raw_len)) {
                    const uint8_t *cig = raw + R.cig();
                    bool bad = false, seen = false;
                    ull lead = 0, trail = 0;
                    for (unsigned j = 0; j < R.n_cig; j++) {
                        const unsigned cw = tdt_ld_u32(cig + 4ull * j), op = cw & 0xf, len = cw >> 4;
                        bad |= op > 8;
                        if (op == 4 || op == 5) {
                            if (seen) trail += len;
                            else lead += len;
                        } else {
                            seen = true;
                            trail = 0;
                        }
                    }
                    const unsigned rev = (f >> 4) & 1u;
                    const long long E = (rev ? (long long)I.end[ri] - 1 + (long long)trail : (long long)I.pos[ri] - (long long)lead) + DUP_BIAS;
                    bad |= E < 0 || E >= DUP_E_LIMIT;
                    if (!bad) {
                        k1 = ((ull)tid << 34) | ((ull)E << 1) | rev;
                        if (pair) {
                            const long long mpos = I.mate_pos[ri];
                            const unsigned mrev = (f >> 5) & 1u;
                            ull mlead = 0, mtrail = 0, mref = 0;
                            long long mend5 = mpos;
                            if (dup_mate_cigar(raw, R.aux(), R.end(), mlead, mtrail, mref))
                                mend5 = mrev ? mpos + (long long)(mref ? mref : 1) - 1 + (long long)mtrail : mpos - (long long)mlead;
                            else
                                no_mc = true;
                            const long long ME = mend5 + DUP_BIAS;
                            bad = ME < 0 || ME >= DUP_E_LIMIT;
                            k2 = DUP_PAIR_BIT | ((ull)mtid << 34) | ((ull)ME << 1) | mrev;
                        }
                    }
                    ok = !bad;
                }
            }
        }
        const ull m_ok = __ballot(ok), m_pair = __ballot(ok && pair);
        cnt[SN_MALFORMED] += (ull)__popcll(__ballot(live && !ok));
        cnt[SN_FRAGMENTS] += (ull)__popcll(m_ok & ~m_pair);
        cnt[SN_PAIRS] += (ull)__popcll(m_pair);
        cnt[SN_PAIRS_NO_MC] += (ull)__popcll(__ballot(ok && pair && no_mc));
        cnt[SN_FLAGGED] += (ull)__popcll(__ballot(ok && (f & 0x400u)));
        if (ok) or1 |= k1, nand1 |= ~k1, or2 |= k2, nand2 |= ~k2;
        // ---- the round's keys behind the tile's earlier ones, in LDS
        const tdt_slots K = tdt_block_slots<DUP_BLOCK / 64>(m_ok, s_wkeys, lane, wave);
        if (ok) {
            const int slot = nk + K.base + tdt_lane_rank(m_ok, lane);      // (< DUP_K_TILE: at most one key per read of the tile)
            s_k1[slot] = k1;
            s_k2[slot] = k2;
            s_m[slot] = (f & 0x400u) ? 1 : 0;
        }
        nk += K.total;
    }
    // ---- the tile's counters: merged per wave, then over the workgroup, ONE atomic per non-zero counter
    or1 = tdt_wave_reduce<tdt_or>(or1), nand1 = tdt_wave_reduce<tdt_or>(nand1), or2 = tdt_wave_reduce<tdt_or>(or2), nand2 = tdt_wave_reduce<tdt_or>(nand2);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SN_PUSH_N; k++) s_cnt[wave][k] = cnt[k];
        s_cnt[wave][SN_PUSH_N] = or1, s_cnt[wave][SN_PUSH_N + 1] = nand1, s_cnt[wave][SN_PUSH_N + 2] = or2, s_cnt[wave][SN_PUSH_N + 3] = nand2;
    }
    __syncthreads();
    if (t == 0) s_base = nk ? atomicAdd(&st[ST_N], (ull)nk) : 0ull;        // the workgroup's slots of the store behind ONE atomic
    if (t < SN_PUSH_N + 4) {
        ull v = 0;
        for (int w = 0; w < DUP_BLOCK / 64; w++) v = t < SN_PUSH_N ? v + s_cnt[w][t] : v | s_cnt[w][t];
        if (v) {
            if (t < SN_PUSH_N) atomicAdd(&st[t], v);
            else atomicOr(&st[ST_OR1 + (t - SN_PUSH_N)], v);
        }
    }
    __syncthreads();
    for (int k = t; k < nk; k += DUP_BLOCK) {                      // (consecutive lanes, consecutive slots)
        const ull slot = s_base + (ull)k;
        if (slot < cap) {
            k1s[slot] = s_k1[k];
            k2s[slot] = s_k2[k];
            ms[slot] = s_m[k];
        } else {
            st[ST_OVERFLOW] = 1;                                   // (cannot happen: the host reserved room for every read of the batch)
        }
    }
}

// ---- the finish
__global__ __launch_bounds__(DUP_BLOCK) void dup_iota(unsigned *__restrict__ v, int n) {
    const int i = blockIdx.x * DUP_BLOCK + threadIdx.x;
    if (i < n) v[i] = (unsigned)i;
}

__global__ __launch_bounds__(DUP_BLOCK) void dup_gather(ull *__restrict__ dst, const ull *__restrict__ src, const unsigned *__restrict__ perm, int n) {
    const int i = blockIdx.x * DUP_BLOCK + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

// inclusive running maximum over the workgroup's 256 threads, in thread order; *total = the maximum of all (s: DUP_BLOCK / 64 words)
__device__ __forceinline__ int dup_block_max_scan(int v, int *s, int t, int *total) {
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v = u > v ? u : v;
    }
    if (lane == 63) s[wave] = v;
    __syncthreads();
    int all = -1;
#pragma unroll
    for (int w = 0; w < DUP_BLOCK / 64; w++) {
        const int c = s[w];
        if (w < wave) v = c > v ? c : v;
        all = c > all ? c : all;
    }
    __syncthreads();
    *total = all;
    return v;
}

// a run head: the first key, or a key that differs from the one in front of it
__device__ __forceinline__ bool dup_head(const ull *__restrict__ a, const ull *__restrict__ b, int i) {
    return i == 0 || a[i] != a[i - 1] || b[i] != b[i - 1];
}

// tile_last[tile] = the position of the tile's last run head, -1 when it has none
__global__ __launch_bounds__(DUP_BLOCK) void dup_tile_heads(const ull *__restrict__ a, const ull *__restrict__ b, int n, int *__restrict__ tile_last) {
    __shared__ int s[DUP_BLOCK / 64];
    const int t = threadIdx.x;
    const int t0 = blockIdx.x * DUP_TILE;
    int best = -1;
    for (int r = 0; r < DUP_TILE / DUP_BLOCK; r++) {
        const int i = t0 + r * DUP_BLOCK + t;
        if (i < n && dup_head(a, b, i)) best = i;                 // (i grows with r)
    }
    int all;
    (void)dup_block_max_scan(best, s, t, &all);
    if (t == 0) tile_last[blockIdx.x] = all;
}

// ONE workgroup: tile_last[k] = the last run head at or in front of tile k's end (a running maximum over the tiles)
__global__ __launch_bounds__(DUP_BLOCK) void dup_carry(int *__restrict__ tile_last, int ntiles) {
    __shared__ int s[DUP_BLOCK / 64];
    const int t = threadIdx.x;
    int running = -1;
    for (int c = 0; c < ntiles; c += DUP_BLOCK) {                 // (uniform)
        const int k = c + t;
        int all;
        int v = dup_block_max_scan(k < ntiles ? tile_last[k] : -1, s, t, &all);
        v = v > running ? v : running;
        if (k < ntiles) tile_last[k] = v;
        running = all > running ? all : running;
    }
}

// every run measured at its end: length = position - last head + 1; out: the finish's share of the counter array
__global__ __launch_bounds__(DUP_BLOCK) void dup_runs(const ull *__restrict__ a, const ull *__restrict__ b, int n, const int *__restrict__ tile_last,
                                                      ull *__restrict__ out) {
    __shared__ unsigned s_hist[2 * TDT_DUP_HIST_MAX];             // a tile ends at most DUP_TILE runs: no word can wrap
    __shared__ ull s_acc[4];                                       // sets: pair, fragment; duplicates: pair, fragment
    __shared__ int s[DUP_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63;
    for (int k = t; k < 2 * TDT_DUP_HIST_MAX; k += DUP_BLOCK) s_hist[k] = 0;
    if (t < 4) s_acc[t] = 0;
    __syncthreads();
    const int t0 = blockIdx.x * DUP_TILE;
    int running = blockIdx.x ? tile_last[blockIdx.x - 1] : -1;
    for (int r = 0; r < DUP_TILE / DUP_BLOCK; r++) {              // (uniform: every thread takes every round)
        const int i = t0 + r * DUP_BLOCK + t;
        const bool valid = i < n;
        ull ka = 0, kb = 0;
        bool head = false, end = false;
        if (valid) {
            ka = a[i];
            kb = b[i];
            head = dup_head(a, b, i);
            end = i == n - 1 || a[i + 1] != ka || b[i + 1] != kb;
        }
        int all;
        int last = dup_block_max_scan(head ? i : -1, s, t, &all);
        last = last > running ? last : running;
        running = all > running ? all : running;
        const unsigned frag = (kb & DUP_PAIR_BIT) ? 0u : 1u;
        const unsigned len = end ? (unsigned)(i - last + 1) : 0u;
        // (most sets of real data are single reads: those of a wave are counted by two ballots)
        const ull m1p = __ballot(end && len == 1 && !frag), m1f = __ballot(end && len == 1 && frag);
        if (lane == 0) {
            if (m1p) atomicAdd(&s_hist[0], (unsigned)__popcll(m1p));
            if (m1f) atomicAdd(&s_hist[1], (unsigned)__popcll(m1f));
        }
        if (end && len > 1) {
            atomicAdd(&s_hist[2 * ((len > TDT_DUP_HIST_MAX ? TDT_DUP_HIST_MAX : len) - 1) + frag], 1u);
            atomicAdd(&s_acc[2 + frag], (ull)(len - 1));
        }
    }
    __syncthreads();
    for (int k = t; k < 2 * TDT_DUP_HIST_MAX; k += DUP_BLOCK) {
        const unsigned v = s_hist[k];
        if (v) {
            atomicAdd(&out[TDT_DUP_OFF_HIST + k], (ull)v);
            atomicAdd(&s_acc[k & 1], (ull)v);
        }
    }
    __syncthreads();
    if (t < 4 && s_acc[t]) atomicAdd(&out[t == 0 ? SN_PAIR_SETS : t == 1 ? SN_FRAGMENT_SETS : t == 2 ? SN_PAIR_DUPS : SN_FRAGMENT_DUPS], s_acc[t]);
}

static void dup_free(tdt_dup *h) {
    if (h->k1) (void)hipFree(h->k1);
    if (h->k2) (void)hipFree(h->k2);
    if (h->marked) (void)hipFree(h->marked);
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->io.d) (void)hipFree(h->io.d);
    if (h->d_work) (void)hipFree(h->d_work);
    for (int k = 0; k < 5; k++)
        if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
    delete h;
}

// three device arrays of `cap` store entries; on failure nothing is left allocated
static hipError_t dup_alloc_store(size_t cap, ull **k1, ull **k2, uint8_t **m) {
    *k1 = *k2 = nullptr;
    *m = nullptr;
    if (tdt_dev_malloc((void **)k1, cap * 8) == hipSuccess && tdt_dev_malloc((void **)k2, cap * 8) == hipSuccess &&
        tdt_dev_malloc((void **)m, cap) == hipSuccess)
        return hipSuccess;
    if (*k1) (void)hipFree(*k1);
    if (*k2) (void)hipFree(*k2);
    *k1 = *k2 = nullptr;
    return hipErrorOutOfMemory;
}

extern "C" size_t tdt_dup_size(void) { return TDT_DUP_TOTAL; }

extern "C" int tdt_dup_create(tdt_ctx *ctx, int n_contigs, int64_t max_contig_len, size_t capacity, tdt_dup **out) {
    if (!ctx || !out || n_contigs < 0 || max_contig_len < 0) {
        tdt_set_error("tdt_dup_create: bad argument");
        return TDT_E_ARG;
    }
    if (n_contigs > DUP_MAX_CONTIGS || max_contig_len > 0x7fffffffll || capacity >= (1ull << 40)) {
        tdt_set_error("tdt_dup_create: %d contigs (at most 2^24), longest %lld (below 2^31), capacity %zu", n_contigs, (long long)max_contig_len, capacity);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_dup *h = new tdt_dup{};
    h->ctx = ctx;
    h->n_contigs = n_contigs;
    h->max_len = max_contig_len;
    if (tdt_dev_malloc((void **)&h->d_state, ST_WORDS * 8) != hipSuccess ||
        (capacity && dup_alloc_store(capacity, &h->k1, &h->k2, &h->marked) != hipSuccess)) {
        dup_free(h);
        tdt_set_error("tdt_dup_create: out of device memory (%zu keys)", capacity);
        return TDT_E_NOMEM;
    }
    h->cap = capacity;
    hipError_t e = hipMemsetAsync(h->d_state, 0, ST_WORDS * 8, ctx->stream);
    for (int k = 0; k < 5 && e == hipSuccess; k++) e = hipEventCreate(&h->ev[k]);
    if (e != hipSuccess) {
        dup_free(h);
        TDT_HIP(e);
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_dup_destroy(tdt_dup *h) {
    if (!h) return TDT_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);        // (no kernel of the stream still writes the store)
    dup_free(h);
    return TDT_OK;
}

extern "C" int tdt_dup_reset(tdt_dup *h) {
    if (!h) {
        tdt_set_error("tdt_dup_reset: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    TDT_HIP(hipMemsetAsync(h->d_state, 0, ST_WORDS * 8, h->ctx->stream));
    h->upper = 0;
    return TDT_OK;
}

// how many keys the store holds (the stream is synchronised)
static int dup_stored(tdt_dup *h, ull *state) {
    hipStream_t st = h->ctx->stream;
    TDT_HIP(hipMemcpyAsync(state, h->d_state, ST_WORDS * 8, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    if (state[ST_OVERFLOW] || state[ST_N] > h->cap) {
        tdt_set_error("tdt_dup: the key store overflowed (%llu keys, capacity %zu)", state[ST_N], h->cap);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

// room for `more` keys behind the (at most) h->upper stored ones: as tdt_evstore grows — a bigger store, the keys so far copied over on the
// device, the old one freed once the copy is done.  A growth first asks the device how many keys there really are.
static int dup_reserve(tdt_dup *h, size_t more) {
    if (h->upper + more <= h->cap) return TDT_OK;
    ull state[ST_WORDS];
    int rc = dup_stored(h, state);
    if (rc) return rc;
    h->upper = (size_t)state[ST_N];
    if (h->upper + more <= h->cap) return TDT_OK;
    size_t want = h->cap + h->cap / 2;
    if (want < h->upper + more) want = h->upper + more;
    ull *k1, *k2;
    uint8_t *m;
    if (dup_alloc_store(want, &k1, &k2, &m) != hipSuccess) {
        tdt_set_error("tdt_dup: out of device memory growing to %zu keys", want);
        return TDT_E_NOMEM;
    }
    hipStream_t st = h->ctx->stream;
    hipError_t e = hipSuccess;
    if (h->upper) {
        e = hipMemcpyAsync(k1, h->k1, h->upper * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(k2, h->k2, h->upper * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(m, h->marked, h->upper, hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(k1), (void)hipFree(k2), (void)hipFree(m);
        TDT_HIP(e);
    }
    if (h->k1) (void)hipFree(h->k1);
    if (h->k2) (void)hipFree(h->k2);
    if (h->marked) (void)hipFree(h->marked);
    h->k1 = k1, h->k2 = k2, h->marked = m;
    h->cap = want;
    return TDT_OK;
}

static int dup_launch(tdt_dup *h, const DupIn &I, size_t n, size_t raw_len) {
    int rc = dup_reserve(h, n);
    if (rc) return rc;
    hipLaunchKernelGGL(dup_keys, dim3((unsigned)((n + DUP_K_TILE - 1) / DUP_K_TILE)), dim3(DUP_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len,
                       h->k1, h->k2, h->marked, (ull)h->cap, h->d_state);
    TDT_CHECK_LAUNCH();
    h->upper += n;
    return TDT_OK;
}

#define DUP_NEED (TDT_NEED(FLAG) | TDT_NEED(TID) | TDT_NEED(POS) | TDT_NEED(END) | TDT_NEED(MATE_TID) | TDT_NEED(MATE_POS) | TDT_NEED(REC_OFF) | TDT_NEED(RAW))

// One batch of the device ingest: d_arrays14 = the pointer table tdt_ingest_arrays filled (TDT_COL_*: a host array of TDT_NCOL device
// pointers).  The launch is enqueued on the context's stream and nothing is waited for — unless the store must grow.
extern "C" int tdt_dup_push_device(tdt_dup *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    tdt_batch B;
    const int rc = tdt_batch_view("tdt_dup_push_device", h, d_arrays14, n, raw_len, DUP_NEED, &B);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    return dup_launch(h, DupIn{B.flag, B.tid, B.pos, B.end, B.mate_tid, B.mate_pos, B.rec_off, B.raw}, n, raw_len);
}

// The same kernel on host columns and host record bytes (uploaded into the handle's own block).  The stream is synchronised before the
// return: the caller's arrays are free again.
extern "C" int tdt_dup_push(tdt_dup *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const int32_t *end, const int32_t *mate_tid,
                            const int32_t *mate_pos, const uint64_t *rec_off, size_t n, const uint8_t *raw, size_t raw_len) {
    tdt_batch H{}, B;
    H.flag = flag, H.tid = tid, H.pos = pos, H.end = end, H.mate_tid = mate_tid, H.mate_pos = mate_pos, H.rec_off = rec_off, H.raw = raw;
    int rc = tdt_batch_host("tdt_dup_push", h, H, n, raw_len, DUP_NEED);
    if (rc == TDT_OK) rc = tdt_batch_offsets_ascend("tdt_dup_push", rec_off, n);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    rc = tdt_batch_upload("tdt_dup_push", h->ctx, &h->io, H, DUP_NEED, n, raw_len, &B);
    if (rc == TDT_OK) rc = dup_launch(h, DupIn{B.flag, B.tid, B.pos, B.end, B.mate_tid, B.mate_pos, B.rec_off, B.raw}, n, raw_len);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

// The store read out, in the order it lies in HBM.  On entry *n = the room of the three arrays (ignored when all three are NULL: the
// call then only reports the count); on return *n = the keys stored.  Too little room: TDT_E_RANGE, nothing written.
extern "C" int tdt_dup_keys(tdt_dup *h, uint64_t *k1, uint64_t *k2, uint8_t *marked, size_t *n) {
    if (!h || !n || ((k1 || k2 || marked) && !(k1 && k2 && marked))) {
        tdt_set_error("tdt_dup_keys: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    ull state[ST_WORDS];
    int rc = dup_stored(h, state);
    if (rc) return rc;
    const size_t have = (size_t)state[ST_N];
    if (k1) {
        if (*n < have) {
            tdt_set_error("tdt_dup_keys: room for %zu keys, %zu stored", *n, have);
            return TDT_E_RANGE;
        }
        hipStream_t st = h->ctx->stream;
        if (have) {
            TDT_HIP(hipMemcpyAsync(k1, h->k1, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(k2, h->k2, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(marked, h->marked, have, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
        }
    }
    *n = have;
    return TDT_OK;
}

struct DupWork {
    ull *ka, *kb, *d_out;
    unsigned *ia, *ib;
    int *tile_last;
    size_t lay(void *base, size_t n, size_t ntiles) {
        tdt_carver cv(base);
        ka = cv.take<ull>(n), kb = cv.take<ull>(n), ia = cv.take<unsigned>(n), ib = cv.take<unsigned>(n);
        tile_last = cv.take<int>(ntiles), d_out = cv.take<ull>(TDT_DUP_TOTAL);
        return cv.size;
    }
};

// the sort mask of one key column: its strand bit, the end field (what the header allows: the longest contig and a clip of DUP_BIAS on
// either side of it — widened to the highest bit that DOES differ between two stored keys, which adversarial records can push beyond
// that), the contig field (the contig count, widened the same way); `differ`: the bits that differ between two keys of the column
static ull dup_mask(ull differ, int n_contigs, long long max_len) {
    int ebits = tdt_ceil_log2_u64((uint64_t)max_len + 2ull * (uint64_t)DUP_BIAS + 1ull);
    if (ebits > 33) ebits = 33;
    for (int b = 32; b >= ebits; b--)
        if ((differ >> (1 + b)) & 1ull) {
            ebits = b + 1;
            break;
        }
    int tbits = tdt_ceil_log2_u64((uint64_t)(n_contigs > 1 ? n_contigs : 1));
    for (int b = 23; b >= tbits; b--)
        if ((differ >> (34 + b)) & 1ull) {
            tbits = b + 1;
            break;
        }
    return 1ull | (((1ull << ebits) - 1ull) << 1) | (((1ull << tbits) - 1ull) << 34);
}

// uint64[TDT_DUP_TOTAL]: the push counters and the sets of everything pushed so far.  The store is left as it was.
extern "C" int tdt_dup_finish(tdt_dup *h, uint64_t *out) {
    if (!h || !out) {
        tdt_set_error("tdt_dup_finish: bad argument");
        return TDT_E_ARG;
    }
    tdt_ctx *ctx = h->ctx;
    TDT_HIP(hipSetDevice(ctx->device));
    ull state[ST_WORDS];
    int rc = dup_stored(h, state);
    if (rc) return rc;
    const size_t n_ = (size_t)state[ST_N];
    if (n_ >= (1ull << 30)) {
        tdt_set_error("tdt_dup_finish: %zu keys; the sort handles fewer than 2^30", n_);
        return TDT_E_RANGE;
    }
    std::vector<uint64_t> res(TDT_DUP_TOTAL, 0);
    for (int k = 0; k < SN_PUSH_N; k++) res[k] = state[k];
    for (int k = 0; k < 4; k++) h->ms[k] = 0;
    if (n_) {
        const int n = (int)n_;
        const size_t ntiles = (n_ + DUP_TILE - 1) / DUP_TILE;
        DupWork W;
        const size_t bytes = W.lay(nullptr, n_, ntiles);
        if (bytes > h->work_cap) {
            if (h->d_work) TDT_HIP(hipFree(h->d_work));
            h->d_work = nullptr;
            h->work_cap = 0;
            if (tdt_dev_malloc(&h->d_work, bytes) != hipSuccess) {
                tdt_set_error("tdt_dup_finish: out of device memory (%zu keys)", n_);
                return TDT_E_NOMEM;
            }
            h->work_cap = bytes;
        }
        W.lay(h->d_work, n_, ntiles);
        hipStream_t st = ctx->stream;
        const unsigned grid = (unsigned)((n_ + DUP_BLOCK - 1) / DUP_BLOCK);
        TDT_HIP(hipMemsetAsync(W.d_out, 0, (size_t)TDT_DUP_TOTAL * 8, st));
        TDT_HIP(hipMemcpyAsync(W.ka, h->k2, n_ * 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(dup_iota, dim3(grid), dim3(DUP_BLOCK), 0, st, W.ia, n);
        TDT_CHECK_LAUNCH();
        // PRECONDITION of tdt_radix_sort_pairs: the key bits outside the mask are equal in ALL keys (it rebuilds them from keys[0]).  The
        // masks cover every bit that differs between two stored keys: the push kept the OR of the keys and of their complements, a bit
        // differs exactly when it is set in both, and dup_mask covers each such bit of the strand, end and contig fields; bit 58 is the
        // only other bit a K2 can have.
        const ull mask1 = dup_mask(state[ST_OR1] & state[ST_NAND1], h->n_contigs, h->max_len);
        const ull mask2 = dup_mask(state[ST_OR2] & state[ST_NAND2], h->n_contigs, h->max_len) | DUP_PAIR_BIT;
        if (((state[ST_OR1] & state[ST_NAND1]) & ~mask1) || ((state[ST_OR2] & state[ST_NAND2]) & ~mask2)) {
            tdt_set_error("tdt_dup_finish: key bits outside the sort masks differ");       // (cannot happen: the keys have no other fields)
            return TDT_E_RANGE;
        }
        ull *k2s, *k1s;
        unsigned *perm, *perm2;
        TDT_HIP(hipEventRecord(h->ev[0], st));
        rc = tdt_radix_sort_pairs(ctx, W.ka, W.ia, W.kb, W.ib, n_, mask2, &k2s, &perm);
        if (rc) return rc;
        TDT_HIP(hipEventRecord(h->ev[1], st));
        ull *free_k = k2s == W.ka ? W.kb : W.ka;                   // (the sorted K2 are not needed again: K2 comes from the store below)
        unsigned *free_i = perm == W.ia ? W.ib : W.ia;
        hipLaunchKernelGGL(dup_gather, dim3(grid), dim3(DUP_BLOCK), 0, st, free_k, (const ull *)h->k1, (const unsigned *)perm, n);
        TDT_CHECK_LAUNCH();
        TDT_HIP(hipEventRecord(h->ev[2], st));
        rc = tdt_radix_sort_pairs(ctx, free_k, perm, k2s, free_i, n_, mask1, &k1s, &perm2);           // (the same precondition, mask1)
        if (rc) return rc;
        TDT_HIP(hipEventRecord(h->ev[3], st));
        ull *k2f = k1s == W.ka ? W.kb : W.ka;
        hipLaunchKernelGGL(dup_gather, dim3(grid), dim3(DUP_BLOCK), 0, st, k2f, (const ull *)h->k2, (const unsigned *)perm2, n);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(dup_tile_heads, dim3((unsigned)ntiles), dim3(DUP_BLOCK), 0, st, (const ull *)k1s, (const ull *)k2f, n, W.tile_last);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(dup_carry, dim3(1), dim3(DUP_BLOCK), 0, st, W.tile_last, (int)ntiles);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(dup_runs, dim3((unsigned)ntiles), dim3(DUP_BLOCK), 0, st, (const ull *)k1s, (const ull *)k2f, n, (const int *)W.tile_last,
                           W.d_out);
        TDT_CHECK_LAUNCH();
        TDT_HIP(hipEventRecord(h->ev[4], st));
        std::vector<uint64_t> got(TDT_DUP_TOTAL);
        TDT_HIP(hipMemcpyAsync(got.data(), W.d_out, (size_t)TDT_DUP_TOTAL * 8, hipMemcpyDeviceToHost, st));
        rc = tdt_ctx_sync(ctx);                                    // (also reports the sort's bounded-spin word)
        if (rc) return rc;
        for (int k = SN_PUSH_N; k < TDT_DUP_TOTAL; k++) res[k] = got[k];
        for (int k = 0; k < 4; k++) {
            float ms = 0;
            TDT_HIP(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
            h->ms[k] = ms;
        }
    }
    memcpy(out, res.data(), (size_t)TDT_DUP_TOTAL * 8);
    return TDT_OK;
}

// device milliseconds of the last finish: [0] sort by K2, [1] gather of K1, [2] sort by K1, [3] gather of K2 + the three run-length launches
extern "C" int tdt_dup_timing(tdt_dup *h, double *ms4) {
    if (!h || !ms4) {
        tdt_set_error("tdt_dup_timing: bad argument");
        return TDT_E_ARG;
    }
    for (int k = 0; k < 4; k++) ms4[k] = h->ms[k];
    return TDT_OK;
}
