// SNV candidates for gfx950 — every position where eligible reads of the --sv scan carry a base that differs from the resident
// reference (TIDDIT_SNVS), with its support by strand.  The definition is tiddit_snvs.py's: per keyed event K1 = tid << 32 | P (1-based)
// and K2 = ref2 << 3 | alt2 << 1 | rev; the sets of equal (K1, K2 >> 1) are the distinct events.  Every result is an order-independent
// integer, so it equals the definition exactly.
//   * snv_keys — ONE launch per batch, on the columns and record bytes that are already resident, enqueued beside indel_keys and waiting
//     for nothing.  The read gate (ks_read_gate), the record open (KS_OPEN) and the key emit (ks_stage, ks_flush) are tdt_keystore.h's,
//     shared with indel_keys and clip_keys.  Behind the gate lane = compacted read:
//       - a first pass over the CIGAR (tdt_cig_span_of, tdt_bam_record.h) sums its reference and query lengths and looks for an op
//         code above 8: malformed / no sequence / off the reference are decided BEFORE a base is read, so the walk only ever sees a
//         record whose CIGAR spans exactly l_seq bases of the sequence and lies inside a loaded contig;
//       - the walk compares 16 bases per step: the read's 16 nibbles at query offset q and the reference's 16 at position r as two 64-bit
//         words, both byte-swapped so that the first base is the top nibble whatever the parity of q and of r (the two stores keep the
//         even base in the high nibble; an odd start shifts one nibble in from the ninth byte / the second word: the alignment
//         indel_shift solves for the left-normalisation).  XOR; a zero word — the overwhelmingly common case — costs nothing more.  Only a
//         non-zero nibble gets the ACGT test (one bit set on both sides) and, when it passes, its one quality byte.  The last partial
//         step of an operation is masked, and the read-side load takes single bytes where nine would reach past the record's qualities:
//         nothing outside the record, let alone outside raw[0, raw_len), is read.  The reference side needs no such care: a contig ends
//         in whole words behind TDT_REF_GUARD zero bytes;
//       - at most TDT_SNV_MAX_PER_READ events stay in registers (P: a word each; the two base codes: four bits each of one word).  A
//         ninth is counted and not kept; the walk runs to its end, because aligned_bases and low_quality count for noisy reads too.
//     A workgroup owns SNV_K_TILE = SNV_BLOCK consecutive reads; its keys are staged in LDS (256 reads x 8 keys x 16 B = 32 KB, with the
//     gate's and the emit's 1.5 KB 34280 bytes: four workgroups = 16 waves fit a CU's 160 KB) and flushed once.
//     THE CHOICE lane = compacted read (not a group of lanes per read): a short read is 10 word steps, and the word compare leaves a lane
//     two loads and one XOR per step, so a group of lanes would spend more on merging the group's events, cap and counters across
//     lanes than the walk costs; the bytes of one record are read by one lane in consecutive steps, so each cache line is fetched once
//     and reused from L1/L2 (the batch's raw bytes are streamed exactly once either way); and 256 independent walks per workgroup at 16
//     waves per CU keep many loads in flight.  Measured (profiles/snvs_240mb.md): 1.09 ms per batch of 5.3 M 150-bp reads, 1.3 TB/s of
//     record bytes = 0.22 of a streaming read — latency bound (a lane's steps depend on its own scattered loads), not memory bound, and
//     hidden under the next span's inflate in the job (+1.0 ms of scan stage).  A group of lanes per read is the shape to try if that
//     ever shows; long reads (thousands of steps per lane, unequal lengths inside a wave) would need it and are out of scope (the cap of 8).
//     The host knows only an upper bound of the keys stored (TDT_SNV_MAX_PER_READ per read = 128 B of store per read of a batch, held as
//     headroom): room for it is reserved BEFORE the launch (ks_launch).
//   * tdt_snv_finish — once per job: ks_finish of tdt_keystore.h, the finish the indel store has.  K2 differs in at most 5 bits, so its
//     sort is one digit launch.
#include <vector>

#include "tdt_keystore.h"
#include "tdt_refseq.h"

typedef unsigned long long ull;

#define SNV_BLOCK 256
#define SNV_K_TILE 256                        // reads of a snv_keys workgroup (one round); it stages at most 8 x that many keys in LDS (32 KB)

static_assert(SNV_K_TILE == SNV_BLOCK, "one round per workgroup");
static_assert(TDT_SNV_MAX_PER_READ == 8, "the base codes of a read's events are eight nibbles of one word");
static_assert(SNV_K_TILE * TDT_SNV_MAX_PER_READ * 16 <= 64 * 1024, "the staging stays at or under 64 KB of LDS");

// the SN rows, in the order of the file; the first ten are the push's
enum { SN_RECORDS = 0, SN_ELIGIBLE, SN_MALFORMED, SN_NO_SEQUENCE, SN_OFF_REFERENCE, SN_ALIGNED_BASES, SN_LOW_QUALITY, SN_NOISY, SN_READS_WITH_EVENTS,
       SN_MISMATCHES, SN_DISTINCT, SN_REPORTED, SN_N, SN_PUSH_N = SN_DISTINCT };
static_assert(SN_N == TDT_SNV_SN_N, "SN rows");
enum { ST_OR1 = SN_PUSH_N };                  // OR1, NAND1, OR2, NAND2 behind the push counters; KS_N, KS_OVERFLOW: tdt_keystore.h
static_assert(ST_OR1 + 4 <= KS_N, "state layout");

struct tdt_snv {
    tdt_ctx *ctx;
    int n_contigs, min_mapq, min_bq;
    tdt_refseq *ref;                          // not owned; it outlives the handle
    tdt_keystore S;
    tdt_batch_io io;                          // columns + raw bytes of the host entry
};

// the 16 nibbles that START at nibble `phase` (0 or 1) of raw[b]: nibble 15 - t of the result, counted from the low end, is base t.
// Bytes at lim and beyond are not read (they count as zero; the caller masks those bases away).
__device__ __forceinline__ ull snv_read16(const uint8_t *__restrict__ raw, ull b, unsigned phase, ull lim) {
    ull w = 0;
    unsigned extra = 0;
    if (b + 9 <= lim) {
        __builtin_memcpy(&w, raw + b, 8);                          // (records are not aligned)
        extra = raw[b + 8];
    } else {
        for (unsigned k = 0; k < 9; k++) {
            if (b + k < lim) {
                const unsigned v = raw[b + k];
                if (k < 8) w |= (ull)v << (8 * k);
                else extra = v;
            }
        }
    }
    w = __builtin_bswap64(w);
    return phase ? (w << 4) | (ull)(extra >> 4) : w;
}

__global__ __launch_bounds__(SNV_BLOCK) void snv_keys(ks_cols I, int n, ull raw_len, unsigned min_mapq, unsigned min_bq, ull *__restrict__ k1s,
                                                      ull *__restrict__ k2s, ull cap, ull *__restrict__ st, tdt_refview Rf) {
    __shared__ ull s_k1[SNV_K_TILE * TDT_SNV_MAX_PER_READ], s_k2[SNV_K_TILE * TDT_SNV_MAX_PER_READ];       // the tile's keys, in the order they were made
    const long long lo = (long long)blockIdx.x * SNV_K_TILE, hi = lo + SNV_K_TILE < n ? lo + SNV_K_TILE : n;
    ull cnt[SN_PUSH_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // (aligned_bases, low_quality, mismatches: this lane's; the others: wave-uniform sums of ballots)
    // ---- lane = read: the filters on the columns; then lane = compacted read
    const ks_gated G = ks_read_gate<SNV_BLOCK>(I, lo, hi, min_mapq, cnt[SN_RECORDS], cnt[SN_ELIGIBLE]);
    const bool live = (int)threadIdx.x < G.live;
    bool bad = live, noseq = false, offref = false, walked = false;
    unsigned ne = 0;                                               // keyed events seen (all of them)
    unsigned eP[TDT_SNV_MAX_PER_READ] = {0, 0, 0, 0, 0, 0, 0, 0}, eC = 0;      // P; ref2 << 2 | alt2, four bits per event
    ks_read A{};
    const uint8_t *__restrict__ raw = I.raw;
    if (live && KS_OPEN(A, I, G.read, raw_len)) {
        // ---- the record is bounded: sum its CIGAR, walk it against the reference
        const tdt_rec &R = A.R;
        const int tid = A.tid, pos = A.pos, l_seq = R.l_seq;
        const uint8_t *cig = raw + R.cig();
        const tdt_cig_span C = tdt_cig_span_of(cig, R.n_cig);
        const ull rl = C.ref_len;
        bad = C.malformed(pos, l_seq, R.n_cig);
        if (!bad) {
            const int rlen = tid < Rf.n ? Rf.len[tid] : -1;       // (< 0: the contig is not loaded)
            noseq = R.n_cig == 0 || l_seq == 0;
            offref = !noseq && (rlen < 0 || (ull)pos + rl > (ull)rlen);
            walked = !noseq && !offref;
        }
        if (walked) {
            // every M = X base lies inside [0, l_seq) of the sequence and inside [0, rlen) of the contig
            const ull seq = R.seq(), qual = R.qual(), lim = qual + (ull)l_seq;
            const ull g0 = Rf.off[tid] * 2ull;                    // the store nibble of base 0 of the contig
            ull r = (ull)pos, q = 0;
            for (unsigned j = 0; j < R.n_cig; j++) {
                const unsigned w = tdt_ld_u32(cig + 4ull * j), op = w & 0xfu, len = w >> 4;
                if (op == 0 || op == 7 || op == 8) {
                    cnt[SN_ALIGNED_BASES] += len;
                    for (unsigned s = 0; s < len; s += 16u) {
                        const unsigned m = len - s < 16u ? len - s : 16u;
                        const ull qs = q + s;
                        const ull rd = snv_read16(raw, seq + (qs >> 1), (unsigned)(qs & 1ull), lim);
                        const ull rf = tdt_ref_left16(Rf.store, g0 + r + s + 15ull);
                        ull x = rd ^ rf;
                        if (m < 16u) x &= ~0ull << (4u * (16u - m));
                        while (x) {                              // (rare: a non-zero nibble)
                            const unsigned k = (unsigned)__builtin_clzll(x) >> 2, sh = 60u - 4u * k;
                            const unsigned c = (unsigned)(rd >> sh) & 0xfu, g = (unsigned)(rf >> sh) & 0xfu;
                            x &= ~(0xfull << sh);
                            if (__popc(c) == 1 && __popc(g) == 1) {          // (both one of A C G T, and they differ)
                                const unsigned b = raw[qual + qs + k];
                                if (b != 0xffu && b < min_bq) {
                                    cnt[SN_LOW_QUALITY]++;
                                } else {
                                    const unsigned code = ((unsigned)__builtin_ctz(g) << 2) | (unsigned)__builtin_ctz(c);
#pragma unroll
                                    for (int e = 0; e < TDT_SNV_MAX_PER_READ; e++)
                                        if (ne == (unsigned)e) eP[e] = (unsigned)(r + s + k + 1ull), eC |= code << (4 * e);
                                    ne++;
                                }
                            }
                        }
                    }
                }
                r += tdt_cig_on_ref(op) ? (ull)len : 0ull;
                q += tdt_cig_on_query(op) ? (ull)len : 0ull;
            }
        }
    }
    const bool noisy = walked && ne > TDT_SNV_MAX_PER_READ, ok = walked && !noisy;
    cnt[SN_MALFORMED] = (ull)__popcll(__ballot(live && bad));
    cnt[SN_NO_SEQUENCE] = (ull)__popcll(__ballot(noseq));
    cnt[SN_OFF_REFERENCE] = (ull)__popcll(__ballot(offref));
    cnt[SN_NOISY] = (ull)__popcll(__ballot(noisy));
    cnt[SN_READS_WITH_EVENTS] = (ull)__popcll(__ballot(ok && ne > 0));
    // ---- the tile's keys in LDS, then the emit (tdt_keystore.h)
    const int mine = ok ? (int)ne : 0;
    cnt[SN_MISMATCHES] = (ull)mine;
    int nk;                                                        // the keys of the tile (uniform over the workgroup)
    const int slot = ks_stage<SNV_BLOCK>(mine, &nk);    // (+ mine <= nk <= 8 x the reads of the tile)
    ks_masks M;
#pragma unroll
    for (int e = 0; e < TDT_SNV_MAX_PER_READ; e++) {
        if (e < mine) {
            const ull k1 = ((ull)(unsigned)A.tid << 32) | (ull)eP[e];
            const ull k2 = ((ull)((eC >> (4 * e)) & 0xfu) << 1) | (ull)A.rev;
            M.add(k1, k2);
            s_k1[slot + e] = k1;
            s_k2[slot + e] = k2;
        }
    }
    cnt[SN_ALIGNED_BASES] = tdt_wave_reduce<tdt_sum>(cnt[SN_ALIGNED_BASES]), cnt[SN_LOW_QUALITY] = tdt_wave_reduce<tdt_sum>(cnt[SN_LOW_QUALITY]);
    cnt[SN_MISMATCHES] = tdt_wave_reduce<tdt_sum>(cnt[SN_MISMATCHES]);
    ks_flush<SNV_BLOCK, SN_PUSH_N>(cnt, M, nk, s_k1, s_k2, k1s, k2s, cap, st);
}

static void snv_free(tdt_snv *h) {
    ks_free(&h->S);
    if (h->io.d) (void)hipFree(h->io.d);
    delete h;
}

extern "C" size_t tdt_snv_sn_size(void) { return TDT_SNV_SN_N; }

extern "C" int tdt_snv_create(tdt_ctx *ctx, int n_contigs, int min_mapq, int min_bq, size_t capacity, tdt_refseq *ref, tdt_snv **out) {
    if (!ctx || !out || !ref || n_contigs < 0 || ref->ctx->device != ctx->device) {
        tdt_set_error("tdt_snv_create: bad argument");
        return TDT_E_ARG;
    }
    if (!ks_create_in_range(n_contigs, min_mapq, capacity) || min_bq < 0 || min_bq > TDT_SNV_MAX_BQ) {
        tdt_set_error("tdt_snv_create: %d contigs (at most 2^24), min_mapq %d (0 ... 255), min_bq %d (0 ... %d), capacity %zu", n_contigs, min_mapq, min_bq,
                      TDT_SNV_MAX_BQ, capacity);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_snv *h = new tdt_snv{};
    h->ctx = ctx;
    h->n_contigs = n_contigs;
    h->min_mapq = min_mapq;
    h->min_bq = min_bq;
    h->ref = ref;
    const int rc = ks_init(&h->S, ctx, "tdt_snv", ST_OR1, capacity);
    if (rc) {
        snv_free(h);
        return rc;
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_snv_destroy(tdt_snv *h) { return ks_destroy(h, snv_free); }

extern "C" int tdt_snv_reset(tdt_snv *h) { return ks_reset_checked(h ? &h->S : nullptr, "tdt_snv"); }

// the launch of one batch: TDT_SNV_MAX_PER_READ slots of the store per read, the bound a read's cap gives
static auto snv_launch(tdt_snv *h, size_t n, size_t raw_len) {
    return [=](const ks_cols &I) {
        return ks_launch(&h->S, n * TDT_SNV_MAX_PER_READ, [&] {
            const dim3 grid((unsigned)((n + SNV_K_TILE - 1) / SNV_K_TILE));
            hipLaunchKernelGGL(snv_keys, grid, dim3(SNV_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, (unsigned)h->min_bq,
                               h->S.k1, h->S.k2, (ull)h->S.cap, h->S.d_state, tdt_refview{h->ref->d_store, h->ref->d_off, h->ref->d_len, h->ref->n_contigs});
        });
    };
}

// the two entries of a batch: ks_push_device / ks_push of tdt_keystore.h
extern "C" int tdt_snv_push_device(tdt_snv *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    return ks_push_device("tdt_snv_push_device", h, d_arrays14, n, raw_len, snv_launch(h, n, raw_len));
}

extern "C" int tdt_snv_push(tdt_snv *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off, size_t n,
                            const uint8_t *raw, size_t raw_len) {
    return ks_push("tdt_snv_push", h, ks_cols{flag, tid, pos, mapq, rec_off, raw}, n, raw_len, snv_launch(h, n, raw_len));
}

extern "C" int tdt_snv_keys(tdt_snv *h, uint64_t *k1, uint64_t *k2, size_t *n) { return ks_keys(h ? &h->S : nullptr, "tdt_snv", k1, k2, n); }

// sn_out: uint64[TDT_SNV_SN_N], the push counters and the sets of everything pushed so far; *n_rows: the rows tdt_snv_rows will give.
// The store is left as it was.
extern "C" int tdt_snv_finish(tdt_snv *h, uint64_t min_support, uint64_t *sn_out, size_t *n_rows) {
    uint64_t res[SN_N] = {};
    ull got[2];
    const int rc = ks_finish_counted(h ? &h->S : nullptr, "tdt_snv", h && sn_out && n_rows, min_support, TDT_SNV_MAX_SUPPORT, min_support, SN_PUSH_N, res, got);
    if (rc) return rc;
    res[SN_DISTINCT] = got[0];
    res[SN_REPORTED] = got[1];
    memcpy(sn_out, res, sizeof res);
    *n_rows = h->S.n_rows;
    return TDT_OK;
}

extern "C" int tdt_snv_rows(tdt_snv *h, uint64_t *k1, uint64_t *k2, uint32_t *support, uint32_t *rev, size_t *n) {
    return ks_rows(h ? &h->S : nullptr, "tdt_snv", k1, k2, support, rev, n);
}

extern "C" int tdt_snv_timing(tdt_snv *h, double *ms4) { return ks_timing(h ? &h->S : nullptr, "tdt_snv", ms4); }

extern "C" int tdt_snv_reserve_stats(tdt_snv *h, uint64_t *out3) { return ks_reserve_stats(h ? &h->S : nullptr, "tdt_snv", out3); }
