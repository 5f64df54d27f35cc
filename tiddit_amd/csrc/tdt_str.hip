// Tandem repeats at known loci for gfx950 — the repeat lengths the reads of the --sv scan show at the loci of a catalogue (TIDDIT_STR).
// The definition is tiddit_str.py's: per (eligible read, one of the first four loci in its reach) one outcome, keyed K1 = the locus index
// and K2 = kind << 33 | L << 1 | rev; the sets of equal (K1, K2 >> 1) are what the genotype rule reads.  Every result is an
// order-independent integer, so it equals the definition exactly.
//   * A handle keeps the loci table in HBM (starts, ends, packed motifs, contig offsets: tdt_alleles.hip's way of keeping known sites) and
//     a key store (tdt_keystore.h: the store, its reserve, the push path's checks, the sort and run-length finish, the read-outs).
//   * str_keys — ONE launch per batch, a workgroup per STR_BLOCK reads, on the columns and record bytes that are already resident.
//     Lane = read for the gate (ks_read_gate); a live lane finds the loci [lo, hi) in reach by two lower bounds (the first end >= pos,
//     the first start > end: starts and ends both ascend).  The reads that have one — a few per cent — are compacted once more within the
//     workgroup, so the record bytes of the others are never touched.  Lane = compacted read: the record is opened (KS_OPEN), its CIGAR
//     walked ONCE for all of its at most STR_MAX_PER_READ loci (their anchors' query indices stay in registers), then the outcome per
//     locus.  The two run counts compare 16 bases per step: the read's nibbles as a 64-bit word brought to the run's phase
//     (str_word16) XOR a 16-nibble word of the motif rotated to the step's phase (str_pattern; 16 mod m is not 0 for m = 3, 5, 6, so
//     the phase moves from step to step); the first non-zero nibble ends the run — counted from the low end going right, from the high
//     end going left.  No load leaves [rec_off, rec_off + 4 + block_size): str_word16 takes the record's end and reads bytes at or
//     behind it as zero.  The keys are staged in LDS (STR_BLOCK x 4 keys x 16 B = 16 KB) and appended with ks_stage / ks_flush: ONE atomic
//     per workgroup on the store's slot counter.  The host reserves STR_MAX_PER_READ slots per read BEFORE the launch (ks_launch).
//   * The gate needs the batch's END column, which ks_cols does not carry: the two push entries of this file are built round
//     tdt_batch_view / tdt_batch_host / tdt_batch_upload with KS_NEED | TDT_NEED(END) and pass that pointer beside the ks_cols.
// The compiler's resource report for str_keys (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage):
//   VGPRs 93, AGPRs 0, SGPRs 74, scratch 0 bytes/lane, no spills, LDS 21016 bytes/workgroup, occupancy 5 waves/SIMD.
#include "tdt_keystore.h"

typedef unsigned long long ull;

#define STR_BLOCK 256
#define STR_MAX_PER_READ TDT_STR_MAX_PER_READ
static_assert(STR_BLOCK == KS_BLOCK && STR_MAX_PER_READ == 4, "a read's loci are four register sets; the staged keys are 256 x 4 x 16 B");

// the SN rows, in the order of the file: all of them are the push's
enum { SN_RECORDS = 0, SN_ELIGIBLE, SN_IN_REACH, SN_MALFORMED, SN_NO_ALIGNMENT, SN_NO_SEQUENCE, SN_SPAN, SN_LEFT, SN_RIGHT, SN_UNANCHORED, SN_OVER_CAP,
       SN_N, SN_PUSH_N = SN_N };
static_assert(SN_N == TDT_STR_SN_N, "SN rows");
enum { ST_OR1 = SN_PUSH_N };                    // the OR / NAND words behind the push counters (four words, below KS_N)
static_assert(ST_OR1 + 4 <= KS_N, "state layout");
enum { K_SPAN = 0, K_LEFT_CLOSED, K_LEFT_OPEN, K_RIGHT_CLOSED, K_RIGHT_OPEN };

struct str_table {                            // the kernel's view of the loci (device pointers)
    const int32_t *ls, *le;                   // starts, ends: 0-based half-open, contig-major, both ascending per contig
    const uint32_t *motif;                    // m | code_0 << 4 | code_1 << 8 ...
    const long long *off;                     // n_contigs + 1
    int n_contigs;
};

struct tdt_str {
    tdt_ctx *ctx;
    int n_contigs, flank, min_mapq;
    size_t nl;
    int32_t *d_ls, *d_le;
    uint32_t *d_motif;
    long long *d_off;
    tdt_keystore S;                           // the keys, the state line, the finish's buffers and rows
    tdt_batch_io io;                          // columns + raw bytes of the host entry
};

// first index in [lo, hi) whose entry is >= v
__device__ __forceinline__ long long str_lower_bound(const int32_t *__restrict__ s, long long lo, long long hi, long long v) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)s[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool str_is_match(unsigned op) { return op == 0 || op == 7 || op == 8; }

// The 4-bit codes of the query bases [at, at + 16) of the sequence at raw[seq ...] as one word, base at + i in bits 4 i ... 4 i + 3.
// Nine bytes from raw[seq + at / 2] on; a byte at or behind `lim` (the record's end) is not loaded and reads as zero.  What lies behind
// the sequence's last base inside the record (the qualities) comes along: the caller masks the nibbles it does not own.
__device__ __forceinline__ ull str_word16(const uint8_t *__restrict__ raw, ull seq, ull lim, unsigned at) {
    const ull p = seq + (at >> 1);
    ull w = 0;
    unsigned b8 = 0;
    if (p + 9 <= lim) {
        __builtin_memcpy(&w, raw + p, 8);
        b8 = raw[p + 8];
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (p + k < lim) w |= (ull)raw[p + k] << (8 * k);
    }
    w = ((w >> 4) & 0x0f0f0f0f0f0f0f0full) | ((w & 0x0f0f0f0f0f0f0f0full) << 4);      // (the even base is a byte's HIGH nibble)
    if (at & 1u) w = (w >> 4) | ((ull)(b8 >> 4) << 60);
    return w;
}

// 16 nibbles of the motif from letter `phase` (< m) on: nibble i = code[(phase + i) mod m]; u = the m codes, letter 0 lowest
__device__ __forceinline__ ull str_pattern(ull u, unsigned m, unsigned phase) {
    const unsigned bits = 4u * m;
    ull w = ((u >> (4u * phase)) | (u << (bits - 4u * phase))) & ((1ull << bits) - 1ull);
    unsigned sh = bits;
#pragma unroll
    for (int k = 0; k < 4; k++) {                                  // (m = 1: 4, 8, 16, 32 bits; m = 6: 24, 48)
        if (sh < 64u) w |= w << sh;
        sh <<= 1;
    }
    return w;
}

// LEFT: the largest n with, for every i < n, q0 + i < l_seq and code(q0 + i) == motif[i mod m]
__device__ __forceinline__ unsigned str_run_right(const uint8_t *__restrict__ raw, ull seq, ull lim, unsigned q0, unsigned l_seq, ull u, unsigned m) {
    unsigned n = 0, phase = 0;
    while (q0 + n < l_seq) {
        const unsigned left = l_seq - (q0 + n);
        ull x = str_word16(raw, seq, lim, q0 + n) ^ str_pattern(u, m, phase);
        if (left < 16u) x |= ~0ull << (4u * left);
        const unsigned run = x ? (unsigned)__builtin_ctzll(x) >> 2 : 16u;
        n += run;
        if (run < 16u) break;
        phase = (phase + 16u) % m;
    }
    return n;
}

// RIGHT: the largest n with, for every j < n, qb - 1 - j >= 0 and code(qb - 1 - j) == motif[(last - j) mod m], last = (e - 1 - s) mod m.
// A step's window is the 16 bases that END at qb - 1 - n, the run counted from the word's high end; in front of base 0 the window holds
// nibbles nobody owns, which end the run.
__device__ __forceinline__ unsigned str_run_left(const uint8_t *__restrict__ raw, ull seq, ull lim, int qb, ull u, unsigned m, unsigned last) {
    unsigned n = 0;
    while ((int)n < qb) {
        const int q1 = qb - 1 - (int)n, start = q1 - 15;
        const unsigned have = q1 + 1 < 16 ? (unsigned)(q1 + 1) : 16u;
        const ull w = start >= 0 ? str_word16(raw, seq, lim, (unsigned)start) : str_word16(raw, seq, lim, 0u) << (4u * (unsigned)(-start));
        const unsigned phase = (last + m - (n + 15u) % m) % m;    // the letter of the window's lowest nibble: (last - n - 15) mod m
        ull x = w ^ str_pattern(u, m, phase);
        if (have < 16u) x |= (1ull << (4u * (16u - have))) - 1ull;
        const unsigned run = x ? (unsigned)__builtin_clzll(x) >> 2 : 16u;
        n += run;
        if (run < 16u) break;
    }
    return n;
}

__global__ __launch_bounds__(STR_BLOCK) void str_keys(ks_cols I, const int32_t *__restrict__ endc, int n, ull raw_len, unsigned min_mapq, int flank, str_table T,
                                                      ull *__restrict__ k1s, ull *__restrict__ k2s, ull cap, ull *__restrict__ st) {
    __shared__ ull s_k1[STR_BLOCK * STR_MAX_PER_READ], s_k2[STR_BLOCK * STR_MAX_PER_READ];      // the workgroup's keys, in thread order
    __shared__ int s_read[STR_BLOCK], s_lo[STR_BLOCK], s_nin[STR_BLOCK];                         // the reads with a locus in reach
    __shared__ int s_wsum[STR_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long first = (long long)blockIdx.x * STR_BLOCK, hi_read = first + STR_BLOCK < n ? first + STR_BLOCK : n;
    ull cnt[SN_PUSH_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // (records .. no_sequence: wave-uniform sums of ballots; the others: this lane's)
    ks_masks M;
    // ---- lane = read: the filters on the columns; a live lane's loci in reach, s <= end and e >= pos
    const ks_gated G = ks_read_gate<STR_BLOCK>(I, first, hi_read, min_mapq, cnt[SN_RECORDS], cnt[SN_ELIGIBLE]);
    long long lo = 0, hi = 0;
    if (t < G.live) {
        const int c = I.tid[G.read];
        if (c < T.n_contigs) {
            const long long o0 = T.off[c], o1 = T.off[c + 1];
            if (o1 > o0) {
                lo = str_lower_bound(T.le, o0, o1, (long long)I.pos[G.read]);
                hi = lo < o1 ? str_lower_bound(T.ls, lo, o1, (long long)endc[G.read] + 1) : lo;      // (starts ascend: nothing in front of lo is asked)
            }
        }
    }
    // ---- the reads that have one, compacted in read order
    const bool has = hi > lo;
    const ull m_has = __ballot(has);
    cnt[SN_IN_REACH] += (ull)__popcll(m_has);
    const tdt_slots C = tdt_block_slots<STR_BLOCK / 64>(m_has, s_wsum, lane, wave);
    if (has) {
        const int k = C.base + tdt_lane_rank(m_has, lane);
        s_read[k] = G.read;
        s_lo[k] = (int)lo;                                          // (a locus index: below 2^24)
        s_nin[k] = (int)(hi - lo);
    }
    __syncthreads();
    // ---- lane = compacted read: open the record, walk its CIGAR once for all of its loci
    const bool live = t < C.total;
    bool bad = false, noal = false, noseq = false;
    int l0 = 0, nh = 0, over = 0;
    int qa0 = -1, qa1 = -1, qa2 = -1, qa3 = -1, qb0 = -1, qb1 = -1, qb2 = -1, qb3 = -1;
    int S0 = 0, S1 = 0, S2 = 0, S3 = 0, E0 = -1, E1 = -1, E2 = -1, E3 = -1;        // (no locus: anchors at -1, which no operation covers)
    int l_seq = 0, end = 0;
    ull seq = 0, lim = 0;
    ks_read A{};
    const uint8_t *__restrict__ raw = I.raw;
    if (live) {
        const int ri = s_read[t];
        l0 = s_lo[t];
        const int nin = s_nin[t];
        nh = nin < STR_MAX_PER_READ ? nin : STR_MAX_PER_READ;
        over = nin - nh;
        end = endc[ri];
        bad = true;
        if (KS_OPEN(A, I, ri, raw_len)) {
            const tdt_rec &R = A.R;
            bad = false;
            noal = R.n_cig == 0;
            noseq = !noal && R.l_seq == 0;
            if (!noal && !noseq) {
                l_seq = R.l_seq;
                seq = R.seq();
                lim = R.end();
                S0 = T.ls[l0], E0 = T.le[l0];
                if (nh > 1) S1 = T.ls[l0 + 1], E1 = T.le[l0 + 1];
                if (nh > 2) S2 = T.ls[l0 + 2], E2 = T.le[l0 + 2];
                if (nh > 3) S3 = T.ls[l0 + 3], E3 = T.le[l0 + 3];
                const uint8_t *cig = raw + R.cig();
                long long r = A.pos, q = 0;
                for (unsigned j = 0; j < R.n_cig; j++) {
                    const unsigned cw = tdt_ld_u32(cig + 4ull * j), op = cw & 0xfu, len = cw >> 4;
                    bad |= op > 8;
                    if (str_is_match(op)) {
                        // the query index of reference base x when this operation covers it (saturated: such an index is >= any l_seq)
#define STR_ANCHOR(x, out)                                                                                                               \
    {                                                                                                                                    \
        const long long d = (long long)(x) - r;                                                                                          \
        if (d >= 0 && d < (long long)len) out = q + d > 0x7fffffffll ? 0x7fffffff : (int)(q + d);                                         \
    }
                        STR_ANCHOR(S0 - 1, qa0) STR_ANCHOR(E0, qb0) STR_ANCHOR(S1 - 1, qa1) STR_ANCHOR(E1, qb1)
                        STR_ANCHOR(S2 - 1, qa2) STR_ANCHOR(E2, qb2) STR_ANCHOR(S3 - 1, qa3) STR_ANCHOR(E3, qb3)
#undef STR_ANCHOR
                    }
                    r += tdt_cig_on_ref(op) ? (long long)len : 0;
                    q += tdt_cig_on_query(op) ? (long long)len : 0;
                }
                bad |= qa0 >= l_seq || qa1 >= l_seq || qa2 >= l_seq || qa3 >= l_seq || qb0 >= l_seq || qb1 >= l_seq || qb2 >= l_seq || qb3 >= l_seq;
            }
        }
    }
    const bool ok = live && !bad && !noal && !noseq;
    cnt[SN_MALFORMED] += (ull)__popcll(__ballot(live && bad));
    cnt[SN_NO_ALIGNMENT] += (ull)__popcll(__ballot(live && !bad && noal));
    cnt[SN_NO_SEQUENCE] += (ull)__popcll(__ballot(live && !bad && noseq));
    // ---- the outcome per locus: at most four keys, in registers until the stage has handed out the slots
    ull key0 = 0, key1 = 0, key2 = 0, key3 = 0;
    unsigned valid = 0;
    if (ok) {
        cnt[SN_OVER_CAP] += (ull)over;
        const int pos = A.pos;
#define STR_OUTCOME(k, S, E, qa, qb, key)                                                                                                \
    if (k < nh) {                                                                                                                        \
        const bool left = pos <= S - flank && qa >= 0, right = (long long)end >= (long long)E + flank && qb >= 0;                         \
        const unsigned mw = T.motif[l0 + k], m = mw & 0xfu;                                                                              \
        const ull u = (ull)(mw >> 4);                                                                                                    \
        if (left && right) {                                                                                                             \
            key = ((ull)K_SPAN << 33) | ((ull)(unsigned)(qb - qa - 1) << 1) | A.rev;                                                     \
            cnt[SN_SPAN]++;                                                                                                              \
            valid |= 1u << k;                                                                                                            \
        } else if (left) {                                                                                                               \
            const unsigned L = str_run_right(raw, seq, lim, (unsigned)qa + 1u, (unsigned)l_seq, u, m);                                   \
            key = ((ull)((unsigned)qa + 1u + L == (unsigned)l_seq ? K_LEFT_OPEN : K_LEFT_CLOSED) << 33) | ((ull)L << 1) | A.rev;         \
            cnt[SN_LEFT]++;                                                                                                              \
            valid |= 1u << k;                                                                                                            \
        } else if (right) {                                                                                                              \
            const unsigned L = str_run_left(raw, seq, lim, qb, u, m, (unsigned)(E - 1 - S) % m);                                         \
            key = ((ull)((int)L == qb ? K_RIGHT_OPEN : K_RIGHT_CLOSED) << 33) | ((ull)L << 1) | A.rev;                                   \
            cnt[SN_RIGHT]++;                                                                                                             \
            valid |= 1u << k;                                                                                                            \
        } else {                                                                                                                         \
            cnt[SN_UNANCHORED]++;                                                                                                        \
        }                                                                                                                                \
    }
        STR_OUTCOME(0, S0, E0, qa0, qb0, key0)
        STR_OUTCOME(1, S1, E1, qa1, qb1, key1)
        STR_OUTCOME(2, S2, E2, qa2, qb2, key2)
        STR_OUTCOME(3, S3, E3, qa3, qb3, key3)
#undef STR_OUTCOME
    }
    // ---- the keys into LDS at the slots the stage hands out, then the emit (tdt_keystore.h)
    int total;
    int slot = ks_stage<STR_BLOCK>(__popc(valid), &total);          // (+ mine <= total <= 4 x STR_BLOCK)
#define STR_PUT(k, key)                                                                                                                  \
    if (valid & (1u << k)) {                                                                                                             \
        const ull k1 = (ull)(unsigned)(l0 + k);                                                                                          \
        M.add(k1, key);                                                                                                                  \
        s_k1[slot] = k1;                                                                                                                 \
        s_k2[slot] = key;                                                                                                                \
        slot++;                                                                                                                          \
    }
    STR_PUT(0, key0) STR_PUT(1, key1) STR_PUT(2, key2) STR_PUT(3, key3)
#undef STR_PUT
    cnt[SN_SPAN] = tdt_wave_reduce<tdt_sum>(cnt[SN_SPAN]), cnt[SN_LEFT] = tdt_wave_reduce<tdt_sum>(cnt[SN_LEFT]);
    cnt[SN_RIGHT] = tdt_wave_reduce<tdt_sum>(cnt[SN_RIGHT]), cnt[SN_UNANCHORED] = tdt_wave_reduce<tdt_sum>(cnt[SN_UNANCHORED]);
    cnt[SN_OVER_CAP] = tdt_wave_reduce<tdt_sum>(cnt[SN_OVER_CAP]);
    ks_flush<STR_BLOCK, SN_PUSH_N>(cnt, M, total, s_k1, s_k2, k1s, k2s, cap, st);
}

// ---- the handle: the store, its reserve and the finish are tdt_keystore.h's
static void str_free(tdt_str *h) {
    ks_free(&h->S);
    if (h->d_ls) (void)hipFree(h->d_ls);
    if (h->d_le) (void)hipFree(h->d_le);
    if (h->d_motif) (void)hipFree(h->d_motif);
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->io.d) (void)hipFree(h->io.d);
    delete h;
}

extern "C" size_t tdt_str_sn_size(void) { return TDT_STR_SN_N; }

// a packed motif: m in 1 ... 6, its m codes each one of 1 2 4 8, nothing behind them
static bool str_motif_ok(uint32_t w) {
    const unsigned m = w & 0xfu;
    if (m < 1 || m > TDT_STR_MAX_MOTIF) return false;
    for (unsigned i = 0; i < 7; i++) {
        const unsigned c = (w >> (4 + 4 * i)) & 0xfu;
        if (i < m ? !(c == 1 || c == 2 || c == 4 || c == 8) : c != 0) return false;
    }
    return true;
}

extern "C" int tdt_str_create(tdt_ctx *ctx, const int32_t *lstart, const int32_t *lend, const uint32_t *motif, const int64_t *loc_off, int n_contigs,
                              int flank, int min_mapq, size_t capacity, tdt_str **out) {
    if (!ctx || !out || n_contigs < 0 || !loc_off || loc_off[0] != 0) {
        tdt_set_error("tdt_str_create: bad argument");
        return TDT_E_ARG;
    }
    if (!ks_create_in_range(n_contigs, min_mapq, capacity) || flank < 1 || flank > TDT_STR_MAX_FLANK) {
        tdt_set_error("tdt_str_create: %d contigs (at most 2^24), flank %d (1 ... %d), min_mapq %d (0 ... 255), capacity %zu", n_contigs, flank,
                      TDT_STR_MAX_FLANK, min_mapq, capacity);
        return TDT_E_RANGE;
    }
    for (int c = 0; c < n_contigs; c++) {
        if (loc_off[c + 1] < loc_off[c]) {
            tdt_set_error("tdt_str_create: locus offsets must not decrease (contig %d)", c);
            return TDT_E_ARG;
        }
    }
    const int64_t nl64 = loc_off[n_contigs];
    if (nl64 > TDT_STR_MAX_LOCI) {
        tdt_set_error("tdt_str_create: %lld loci; the handle keeps at most 2^24", (long long)nl64);
        return TDT_E_RANGE;
    }
    const size_t nl = (size_t)nl64;
    if (nl && !(lstart && lend && motif)) {
        tdt_set_error("tdt_str_create: bad argument");
        return TDT_E_ARG;
    }
    for (int c = 0; c < n_contigs; c++) {
        for (int64_t k = loc_off[c]; k < loc_off[c + 1]; k++) {
            if (lstart[k] < 1 || lend[k] <= lstart[k] || lend[k] == 0x7fffffff || (k > loc_off[c] && lstart[k] < lend[k - 1] + 1)) {
                tdt_set_error("tdt_str_create: the loci of contig %d must have 1 <= start < end and start >= the end in front + 1 (locus %lld)", c, (long long)k);
                return TDT_E_ARG;
            }
            if (!str_motif_ok(motif[k])) {
                tdt_set_error("tdt_str_create: locus %lld: not a packed motif of 1 ... %d codes of A C G T", (long long)k, TDT_STR_MAX_MOTIF);
                return TDT_E_ARG;
            }
        }
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_str *h = new tdt_str{};
    h->ctx = ctx;
    h->n_contigs = n_contigs;
    h->flank = flank;
    h->min_mapq = min_mapq;
    h->nl = nl;
    const size_t N = nl ? nl : 1;
    if (tdt_dev_malloc((void **)&h->d_ls, N * 4) != hipSuccess || tdt_dev_malloc((void **)&h->d_le, N * 4) != hipSuccess ||
        tdt_dev_malloc((void **)&h->d_motif, N * 4) != hipSuccess || tdt_dev_malloc((void **)&h->d_off, (size_t)(n_contigs + 1) * 8) != hipSuccess) {
        str_free(h);
        tdt_set_error("tdt_str_create: out of device memory (%zu loci)", nl);
        return TDT_E_NOMEM;
    }
    hipStream_t st = ctx->stream;
    auto body = [&]() -> int {
        const int rc = ks_init(&h->S, ctx, "tdt_str", ST_OR1, capacity);
        if (rc) return rc;
        if (nl) {
            TDT_HIP(hipMemcpyAsync(h->d_ls, lstart, nl * 4, hipMemcpyHostToDevice, st));
            TDT_HIP(hipMemcpyAsync(h->d_le, lend, nl * 4, hipMemcpyHostToDevice, st));
            TDT_HIP(hipMemcpyAsync(h->d_motif, motif, nl * 4, hipMemcpyHostToDevice, st));
        }
        TDT_HIP(hipMemcpyAsync(h->d_off, loc_off, (size_t)(n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
        TDT_HIP(hipStreamSynchronize(st));             // (the host arrays are free again)
        return TDT_OK;
    };
    const int rc = body();
    if (rc) {
        str_free(h);
        return rc;
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_str_destroy(tdt_str *h) { return ks_destroy(h, str_free); }

extern "C" int tdt_str_reset(tdt_str *h) { return ks_reset_checked(h ? &h->S : nullptr, "tdt_str"); }

#define STR_NEED (KS_NEED | TDT_NEED(END))

// the launch of one batch B (device columns): STR_MAX_PER_READ slots of the store per read, the bound a read's cap gives
static int str_launch(tdt_str *h, const tdt_batch &B, size_t n, size_t raw_len) {
    return ks_launch(&h->S, n * STR_MAX_PER_READ, [&] {
        hipLaunchKernelGGL(str_keys, dim3((unsigned)((n + STR_BLOCK - 1) / STR_BLOCK)), dim3(STR_BLOCK), 0, h->ctx->stream, ks_cols_of(B), B.end, (int)n,
                           (ull)raw_len, (unsigned)h->min_mapq, h->flank, str_table{h->d_ls, h->d_le, h->d_motif, h->d_off, h->n_contigs}, h->S.k1, h->S.k2,
                           (ull)h->S.cap, h->S.d_state);
    });
}

// One batch of the device ingest: d_arrays14 = the pointer table tdt_ingest_arrays filled (TDT_COL_*).  The launch is enqueued on the
// context's stream and nothing is waited for — unless the reserve must ask or grow.
extern "C" int tdt_str_push_device(tdt_str *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    tdt_batch B;
    const int rc = tdt_batch_view("tdt_str_push_device", h, d_arrays14, n, raw_len, STR_NEED, &B);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    return str_launch(h, B, n, raw_len);
}

// The same kernel on host columns and host record bytes, uploaded into the handle's own block.  The stream is synchronised before the
// return: the caller's arrays are free again.
extern "C" int tdt_str_push(tdt_str *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint8_t *mapq,
                            const uint64_t *rec_off, size_t n, const uint8_t *raw, size_t raw_len) {
    tdt_batch H{}, B;
    H.flag = flag, H.tid = tid, H.pos = pos, H.end = end, H.mapq = mapq, H.rec_off = rec_off, H.raw = raw;
    int rc = tdt_batch_host("tdt_str_push", h, H, n, raw_len, STR_NEED);
    if (rc == TDT_OK) rc = tdt_batch_offsets_ascend("tdt_str_push", rec_off, n);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    rc = tdt_batch_upload("tdt_str_push", h->ctx, &h->io, H, STR_NEED, n, raw_len, &B);
    if (rc == TDT_OK) rc = str_launch(h, B, n, raw_len);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

// The store read out, in the order it lies in HBM (ks_keys' convention for *n)
extern "C" int tdt_str_keys(tdt_str *h, uint64_t *k1, uint64_t *k2, size_t *n) { return ks_keys(h ? &h->S : nullptr, "tdt_str", k1, k2, n); }

// sn_out: uint64[TDT_STR_SN_N], the push counters of everything pushed so far; *n_rows: the sets, every one of which tdt_str_rows will
// give (no reporting threshold: the genotype rule reads them all).  The store is left as it was.
extern "C" int tdt_str_finish(tdt_str *h, uint64_t *sn_out, size_t *n_rows) {
    uint64_t res[SN_N] = {};
    ull got[2];
    const int rc = ks_finish_counted(h ? &h->S : nullptr, "tdt_str", h && sn_out && n_rows, 1, 1, 1, SN_PUSH_N, res, got);
    if (rc) return rc;
    memcpy(sn_out, res, sizeof res);
    *n_rows = h->S.n_rows;
    return TDT_OK;
}

// The rows of the last finish, ascending by (K1, K2 >> 1): K1, K2 with bit 0 clear, SUPPORT, REV (ks_rows' convention for *n)
extern "C" int tdt_str_rows(tdt_str *h, uint64_t *k1, uint64_t *k2, uint32_t *support, uint32_t *rev, size_t *n) {
    return ks_rows(h ? &h->S : nullptr, "tdt_str", k1, k2, support, rev, n);
}

extern "C" int tdt_str_timing(tdt_str *h, double *ms4) { return ks_timing(h ? &h->S : nullptr, "tdt_str", ms4); }

extern "C" int tdt_str_reserve_stats(tdt_str *h, uint64_t *out3) { return ks_reserve_stats(h ? &h->S : nullptr, "tdt_str", out3); }
