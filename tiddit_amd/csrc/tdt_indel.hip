// Small-indel candidates for gfx950 — every distinct insertion or deletion the reads of the --sv scan carry in their CIGARs
// (TIDDIT_INDELS), with its support by strand.  The definition is tiddit_indels.py's: per keyed event K1 = tid << 32 | P and
// K2 = type << 63 | len << 47 | kind << 45 | payload << 1 | rev; the sets of equal (K1, K2 >> 1) are the distinct events.  Every result
// is an order-independent integer, so it equals the definition exactly.
//   * indel_keys — ONE launch per batch, on the columns and record bytes that are already resident.  The read gate (ks_read_gate), the
//     record open (KS_OPEN) and the key emit (ks_stage, ks_flush) are tdt_keystore.h's, shared with snv_keys and clip_keys; what is
//     this kernel's own: behind the gate lane = compacted read, the CIGAR is walked ONCE with the op in front and the op behind at
//     hand (the flank test), and the at most INDEL_MAX_PER_READ keyed events stay in registers (P, len and type, the query offset:
//     three words each).  A fifth keyed event is counted and not kept; the walk goes on to its end, because an op code above 8 or a P
//     outside [1, 2^31) further on still makes the record malformed.  Malformed / noisy / ok is decided behind the walk: a read gives
//     all of its events or none.  Only then are the inserted bases read (tdt_rec_base at the query offset the walk summed).  A
//     workgroup owns INDEL_K_TILE consecutive reads, INDEL_BLOCK at a time: the gate and the stage run once per round, a round's keys
//     go behind the tile's earlier ones in LDS, and ONE flush appends the tile's keys to the store.  NORM's three counters ride on the
//     flush's barriers.  The host reserves INDEL_MAX_PER_READ slots per read BEFORE the launch (ks_launch).
//   * tdt_indel_finish — once per job: the two stable sorts, the gathers and the run-length launches of tdt_keystore.h (ks_finish);
//     the store, its reserve, the push path of the two entries and the read-outs are that header's too.
#include <vector>

#include "tdt_keystore.h"
#include "tdt_refseq.h"

typedef unsigned long long ull;

#define INDEL_BLOCK 256
#define INDEL_K_TILE 512                      // reads of an indel_keys workgroup; it stages at most 4 x that many keys in LDS (32 KB)
#define INDEL_TILE 4096                       // keys of a run-length workgroup (KS_TILE of tdt_keystore.h)
static_assert(INDEL_TILE == KS_TILE && INDEL_BLOCK == KS_BLOCK, "the run-length tile is the key store's");
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
enum { ST_OR1 = SN_PUSH_N, ST_NAND1, ST_OR2, ST_NAND2, ST_SHIFTED, ST_CAPPED, ST_OFFREF, ST_N = KS_N, ST_OVERFLOW = KS_OVERFLOW, ST_WORDS = KS_WORDS };
static_assert(ST_OFFREF < ST_N && ST_N * 8 % 128 == 0, "state layout");
static_assert(INDEL_NORM_MAX_SHIFT % 16 == 0, "CAP is whole word steps");

struct tdt_indel {
    tdt_ctx *ctx;
    int n_contigs, min_mapq;
    tdt_refseq *ref;                          // attached by tdt_indel_set_reference (not owned); NULL: keys as the aligner placed them
    tdt_keystore S;                           // the keys, the state line (ST_WORDS), the finish's buffers and rows
    tdt_batch_io io;                          // columns + raw bytes of the host entry
};

__device__ __forceinline__ bool indel_is_match(unsigned op) { return op == 0 || op == 7 || op == 8; }

// K2 of an insertion of len bases at query offset q of a sequence of l_seq bases at raw[seq ...]
__device__ __forceinline__ ull indel_ins_key(const uint8_t *__restrict__ raw, ull seq, unsigned q, unsigned len, int l_seq) {
    const ull head = (1ull << 63) | ((ull)len << 47);
    if ((ull)q + len > (ull)l_seq) return head | (2ull << 45);              // (the span is not inside the sequence: SEQ *)
    ull h = 0xcbf29ce484222325ull, pack = 0;
    bool acgt = len <= INDEL_PACK_MAX;
    for (unsigned i = 0; i < len; i++) {
        const unsigned b = tdt_rec_base(raw, seq, q + i);
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
            for (unsigned t = 0; t < m; t++) y |= (ull)tdt_rec_base(raw, seq, q + n - 1u - k - t) << (4u * t);
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
        const unsigned b = i < k ? tdt_ref_code(store, off, (long long)p - k + i) : tdt_rec_base(raw, seq, q + i - k);
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
__global__ __launch_bounds__(INDEL_BLOCK) void indel_keys(ks_cols I, int n, ull raw_len, unsigned min_mapq, ull *__restrict__ k1s, ull *__restrict__ k2s,
                                                          ull cap, ull *__restrict__ st, tdt_refview Rf) {
    __shared__ ull s_k1[INDEL_K_TILE * TDT_INDEL_MAX_PER_READ], s_k2[INDEL_K_TILE * TDT_INDEL_MAX_PER_READ];   // the tile's keys, in the order they were made
    __shared__ ull s_norm[NORM ? INDEL_BLOCK / 64 : 1][3];         // per wave: shifted, capped, off the reference
    ull nshift = 0, ncap = 0, noff = 0;                            // (this lane's)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long lo = (long long)blockIdx.x * INDEL_K_TILE, hi = lo + INDEL_K_TILE < n ? lo + INDEL_K_TILE : n;
    ull cnt[SN_PUSH_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0};             // (records .. noisy, reads_with_events: wave-uniform sums of ballots; the others: this lane's)
    ks_masks M;
    int nk = 0;                                                   // keys of the tile so far (uniform over the workgroup)
    for (long long first = lo; first < hi; first += INDEL_BLOCK) {       // (uniform: the bounds are the workgroup's)
        // ---- lane = read: the filters on the columns; then lane = compacted read: bound the record, walk its CIGAR once
        const ks_gated G = ks_read_gate<INDEL_BLOCK>(I, first, hi, min_mapq, cnt[SN_RECORDS], cnt[SN_ELIGIBLE]);
        const bool live = t < G.live;
        bool bad = live;
        unsigned ne = 0, un = 0, tl = 0;                           // keyed events seen (all of them), unanchored, too long
        unsigned eP[TDT_INDEL_MAX_PER_READ] = {0, 0, 0, 0}, eL[TDT_INDEL_MAX_PER_READ] = {0, 0, 0, 0}, eQ[TDT_INDEL_MAX_PER_READ] = {0, 0, 0, 0};
        int l_seq = 0;
        ull seq = 0;
        ks_read A{};
        const uint8_t *__restrict__ raw = I.raw;
        if (live && KS_OPEN(A, I, G.read, raw_len)) {
            const tdt_rec &R = A.R;
            bad = false;
            l_seq = R.l_seq;
            seq = R.seq();
            const uint8_t *cig = raw + R.cig();
            long long r = A.pos, q = 0;
            unsigned prev = 9u;                                    // (no op in front: no match code)
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
                r += tdt_cig_on_ref(op) ? (long long)len : 0;
                q += tdt_cig_on_query(op) ? (long long)len : 0;
                prev = op;
                cw = nw;
            }
        }
        const int tid = A.tid;
        const unsigned rev = A.rev;
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
        // ---- the round's keys behind the tile's earlier ones, in LDS
        const int mine = ok ? (int)ne : 0;
        int total;
        const int slot = nk + ks_stage<INDEL_BLOCK>(mine, &total);      // (+ mine <= nk + total <= 4 x the reads of the tile so far)
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
                M.add(k1, k2);
                s_k1[slot + k] = k1;
                s_k2[slot + k] = k2;
            }
        }
        nk += total;
    }
    // ---- the lane sums over the wave, then the emit (tdt_keystore.h); NORM's three counters ride on its barriers
    cnt[SN_UNANCHORED] = tdt_wave_reduce<tdt_sum>(cnt[SN_UNANCHORED]), cnt[SN_TOO_LONG] = tdt_wave_reduce<tdt_sum>(cnt[SN_TOO_LONG]);
    cnt[SN_INSERTIONS] = tdt_wave_reduce<tdt_sum>(cnt[SN_INSERTIONS]), cnt[SN_DELETIONS] = tdt_wave_reduce<tdt_sum>(cnt[SN_DELETIONS]);
    if constexpr (NORM) {
        nshift = tdt_wave_reduce<tdt_sum>(nshift), ncap = tdt_wave_reduce<tdt_sum>(ncap), noff = tdt_wave_reduce<tdt_sum>(noff);
        if (lane == 0) s_norm[wave][0] = nshift, s_norm[wave][1] = ncap, s_norm[wave][2] = noff;
    }
    ks_flush<INDEL_BLOCK, SN_PUSH_N>(cnt, M, nk, s_k1, s_k2, k1s, k2s, cap, st);
    if constexpr (NORM) ks_flush_extra<INDEL_BLOCK, 3>(s_norm, st, ST_SHIFTED);
}

// ---- the handle: the store, its reserve and the finish are tdt_keystore.h's
static void indel_free(tdt_indel *h) {
    ks_free(&h->S);
    if (h->io.d) (void)hipFree(h->io.d);
    delete h;
}

extern "C" size_t tdt_indel_sn_size(void) { return TDT_INDEL_SN_N; }

extern "C" int tdt_indel_create(tdt_ctx *ctx, int n_contigs, int min_mapq, size_t capacity, tdt_indel **out) {
    if (!ctx || !out || n_contigs < 0) {
        tdt_set_error("tdt_indel_create: bad argument");
        return TDT_E_ARG;
    }
    if (!ks_create_in_range(n_contigs, min_mapq, capacity)) {
        tdt_set_error("tdt_indel_create: %d contigs (at most 2^24), min_mapq %d (0 ... 255), capacity %zu", n_contigs, min_mapq, capacity);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_indel *h = new tdt_indel{};
    h->ctx = ctx;
    h->n_contigs = n_contigs;
    h->min_mapq = min_mapq;
    const int rc = ks_init(&h->S, ctx, "tdt_indel", ST_OR1, capacity);
    if (rc) {
        indel_free(h);
        return rc;
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_indel_destroy(tdt_indel *h) { return ks_destroy(h, indel_free); }

extern "C" int tdt_indel_reset(tdt_indel *h) { return ks_reset_checked(h ? &h->S : nullptr, "tdt_indel"); }

// the launch of one batch: TDT_INDEL_MAX_PER_READ slots of the store per read, the bound a read's cap gives
static auto indel_launch(tdt_indel *h, size_t n, size_t raw_len) {
    return [=](const ks_cols &I) {
        return ks_launch(&h->S, n * TDT_INDEL_MAX_PER_READ, [&] {
            const dim3 grid((unsigned)((n + INDEL_K_TILE - 1) / INDEL_K_TILE));
            if (h->ref)
                hipLaunchKernelGGL(indel_keys<true>, grid, dim3(INDEL_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, h->S.k1, h->S.k2,
                                   (ull)h->S.cap, h->S.d_state, tdt_refview{h->ref->d_store, h->ref->d_off, h->ref->d_len, h->ref->n_contigs});
            else
                hipLaunchKernelGGL(indel_keys<false>, grid, dim3(INDEL_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, h->S.k1, h->S.k2,
                                   (ull)h->S.cap, h->S.d_state, tdt_refview{nullptr, nullptr, nullptr, 0});
        });
    };
}

// the two entries of a batch: ks_push_device / ks_push of tdt_keystore.h
extern "C" int tdt_indel_push_device(tdt_indel *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    return ks_push_device("tdt_indel_push_device", h, d_arrays14, n, raw_len, indel_launch(h, n, raw_len));
}

extern "C" int tdt_indel_push(tdt_indel *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off,
                              size_t n, const uint8_t *raw, size_t raw_len) {
    return ks_push("tdt_indel_push", h, ks_cols{flag, tid, pos, mapq, rec_off, raw}, n, raw_len, indel_launch(h, n, raw_len));
}

// The store read out, in the order it lies in HBM.  On entry *n = the room of the two arrays (ignored when both are NULL: the call then
// only reports the count); on return *n = the keys stored.  Too little room: TDT_E_RANGE, nothing written.
extern "C" int tdt_indel_keys(tdt_indel *h, uint64_t *k1, uint64_t *k2, size_t *n) { return ks_keys(h ? &h->S : nullptr, "tdt_indel", k1, k2, n); }

// sn_out: uint64[TDT_INDEL_SN_N], the push counters and the sets of everything pushed so far; *n_rows: the rows tdt_indel_rows will
// give.  The store is left as it was.
extern "C" int tdt_indel_finish(tdt_indel *h, uint64_t min_support, uint64_t *sn_out, size_t *n_rows) {
    uint64_t res[SN_N] = {};
    ull got[2];
    const int rc = ks_finish_counted(h ? &h->S : nullptr, "tdt_indel", h && sn_out && n_rows, min_support, TDT_INDEL_MAX_SUPPORT, min_support, SN_PUSH_N, res, got);
    if (rc) return rc;
    res[SN_DISTINCT] = got[0];
    res[SN_REPORTED] = got[1];
    memcpy(sn_out, res, sizeof res);
    *n_rows = h->S.n_rows;
    return TDT_OK;
}

// The rows of the last finish, ascending by (K1, K2 >> 1): K1, K2 with bit 0 clear, SUPPORT, REV.  *n in: the room of the four arrays
// (ignored when all four are NULL), out: the rows.  A push or a reset since the finish: TDT_E_ARG.  Too little room: TDT_E_RANGE.
extern "C" int tdt_indel_rows(tdt_indel *h, uint64_t *k1, uint64_t *k2, uint32_t *support, uint32_t *rev, size_t *n) {
    return ks_rows(h ? &h->S : nullptr, "tdt_indel", k1, k2, support, rev, n);
}

extern "C" int tdt_indel_timing(tdt_indel *h, double *ms4) { return ks_timing(h ? &h->S : nullptr, "tdt_indel", ms4); }

extern "C" int tdt_indel_reserve_stats(tdt_indel *h, uint64_t *out3) { return ks_reserve_stats(h ? &h->S : nullptr, "tdt_indel", out3); }

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
    const int rc = ks_stored(&h->S, state);
    if (rc) return rc;
    out3[0] = state[ST_SHIFTED], out3[1] = state[ST_CAPPED], out3[2] = state[ST_OFFREF];
    return TDT_OK;
}
