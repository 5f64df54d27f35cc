// SNV candidates for gfx950 — every position where eligible reads of the --sv scan carry a base that differs from the resident
// reference (TIDDIT_SNVS), with its support by strand.  The definition is tiddit_snvs.py's: per keyed event K1 = tid << 32 | P (1-based)
// and K2 = ref2 << 3 | alt2 << 1 | rev; the sets of equal (K1, K2 >> 1) are the distinct events.  Every result is an order-independent
// integer, so it equals the definition exactly.
//   * snv_keys — ONE launch per batch, on the columns and record bytes that are already resident, enqueued beside indel_keys and waiting
//     for nothing.  Lane = read for the filters (flag, tid, mapq: coalesced columns); the eligible reads are compacted inside the workgroup
//     (tdt_block_slots, as indel_keys compacts its reads), then lane = compacted read:
//       - the record is bounded with TDT_REC_*, exactly as tdt_indel bounds one;
//       - a first pass over the CIGAR sums its reference and query lengths and looks for an op code above 8: malformed / no sequence /
//         off the reference are decided BEFORE a base is read, so the walk only ever sees a record whose CIGAR spans exactly l_seq bases
//         of the sequence and lies inside a loaded contig;
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
//     A workgroup owns SNV_K_TILE = SNV_BLOCK consecutive reads; its keys are staged in LDS (slots by a prefix sum of the reads' event
//     counts: 256 reads x 8 keys x 16 B = 32 KB, a fifth of the CU's 160 KB, so five workgroups = 20 waves fit a CU) and appended to the
//     store behind ONE atomic.  The counters and the OR of the keys and of their complements (the sort masks) are merged per wave and
//     then over the workgroup: one atomic per workgroup and non-zero word.
//     THE CHOICE lane = compacted read (not a group of lanes per read): a short read is 10 word steps, and the word compare leaves a lane
//     two loads and one XOR per step, so a group of lanes would spend more on merging the group's events, cap and counters across
//     lanes than the walk costs; the bytes of one record are read by one lane in consecutive steps, so each cache line is fetched once
//     and reused from L1/L2 (the batch's raw bytes are streamed exactly once either way); and 256 independent walks per workgroup at 20
//     waves per CU keep many loads in flight.  Measured (profiles/snvs_240mb.md): 1.09 ms per batch of 5.3 M 150-bp reads, 1.3 TB/s of
//     record bytes = 0.22 of a streaming read — latency bound (a lane's steps depend on its own scattered loads), not memory bound, and
//     hidden under the next span's inflate in the job (+1.0 ms of scan stage).  A group of lanes per read is the shape to try if that
//     ever shows; long reads (thousands of steps per lane, unequal lengths inside a wave) would need it and are out of scope (the cap of 8).
//     The host knows only an upper bound of the keys stored (TDT_SNV_MAX_PER_READ per read = 128 B of store per read of a batch, held as
//     headroom): room for it is reserved BEFORE the launch, and a growth first asks the device for the real count (indel_reserve's
//     policy, ks_reserve).  The kernel still tests every slot against the capacity it was given and raises a flag instead of writing.
//   * tdt_snv_finish — once per job: ks_finish of tdt_keystore.h, the finish the indel store has.  K2 differs in at most 5 bits, so its
//     sort is one digit launch.
#include <vector>

#include "tdt_keystore.h"
#include "tdt_refseq.h"

typedef unsigned long long ull;

#define SNV_BLOCK 256
#define SNV_K_TILE 256                        // reads of a snv_keys workgroup (one round); it stages at most 8 x that many keys in LDS (32 KB)
#define SNV_MAX_CONTIGS (1 << 24)
#define SNV_END_LIMIT 0x7fffffffll            // pos + the CIGAR's reference length is at most this

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

struct SnvIn {
    const uint16_t *flag;
    const int32_t *tid, *pos;
    const uint8_t *mapq;
    const uint64_t *rec_off;
    const uint8_t *raw;
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

__global__ __launch_bounds__(SNV_BLOCK) void snv_keys(SnvIn I, int n, ull raw_len, unsigned min_mapq, unsigned min_bq, ull *__restrict__ k1s,
                                                      ull *__restrict__ k2s, ull cap, ull *__restrict__ st, tdt_refview Rf) {
    __shared__ ull s_k1[SNV_K_TILE * TDT_SNV_MAX_PER_READ], s_k2[SNV_K_TILE * TDT_SNV_MAX_PER_READ];       // the tile's keys, in the order they were made
    __shared__ int s_read[SNV_BLOCK];
    __shared__ int s_wsum[SNV_BLOCK / 64], s_wkeys[SNV_BLOCK / 64];
    __shared__ ull s_cnt[SNV_BLOCK / 64][SN_PUSH_N + 4];          // per wave: the push counters, then the OR / NAND words
    __shared__ ull s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long lo = (long long)blockIdx.x * SNV_K_TILE, hi = lo + SNV_K_TILE < n ? lo + SNV_K_TILE : n;
    ull cnt[SN_PUSH_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // (aligned_bases, low_quality, mismatches: this lane's; the others: wave-uniform sums of ballots)
    ull or1 = 0, nand1 = 0, or2 = 0, nand2 = 0;                   // (this lane's keys; merged over the wave at the end)
    // ---- lane = read: the filters on the columns
    const long long i = lo + t;
    bool elig = false;
    if (i < hi) elig = (I.flag[i] & 0xF04u) == 0 && I.tid[i] >= 0 && (unsigned)I.mapq[i] >= min_mapq;
    const ull m_rec = __ballot(i < hi), m_el = __ballot(elig);
    cnt[SN_RECORDS] = (ull)__popcll(m_rec);
    cnt[SN_ELIGIBLE] = (ull)__popcll(m_el);
    const tdt_slots S = tdt_block_slots<SNV_BLOCK / 64>(m_el, s_wsum, lane, wave);
    if (elig) s_read[S.base + tdt_lane_rank(m_el, lane)] = (int)i;
    __syncthreads();
    // ---- lane = compacted read: bound the record, sum its CIGAR, walk it against the reference
    const bool live = t < S.total;
    bool bad = live, noseq = false, offref = false, walked = false;
    unsigned ne = 0;                                               // keyed events seen (all of them)
    unsigned eP[TDT_SNV_MAX_PER_READ] = {0, 0, 0, 0, 0, 0, 0, 0}, eC = 0;      // P; ref2 << 2 | alt2, four bits per event
    unsigned rev = 0;
    int tid = 0;
    const uint8_t *__restrict__ raw = I.raw;
    if (live) {
        const int ri = s_read[t];
        rev = ((unsigned)I.flag[ri] >> 4) & 1u;
        tid = I.tid[ri];
        const int pos = I.pos[ri];
        const ull ro = I.rec_off[ri];
        if (tid < SNV_MAX_CONTIGS && pos >= 0 && TDT_REC_HEADER_INSIDE(raw_len, ro)) {
            tdt_rec R = TDT_REC_READ(raw, ro);
            const int l_seq = R.l_seq;
            R.l_seq = l_seq < 0 ? 0 : l_seq;                       // (clamped: the body's sum never sees a negative length)
            if (l_seq >= 0 && TDT_REC_FITS(R, raw_len)) {
                const uint8_t *cig = raw + R.cig();
                ull rl = 0, ql = 0;
                bool worse = false;
                for (unsigned j = 0; j < R.n_cig; j++) {
                    const unsigned w = tdt_ld_u32(cig + 4ull * j), op = w & 0xfu, len = w >> 4;
                    worse |= op > 8;
                    rl += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? (ull)len : 0ull;
                    ql += (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ? (ull)len : 0ull;
                }
                worse |= (ull)pos + rl > (ull)SNV_END_LIMIT;
                worse |= l_seq >= 1 && R.n_cig >= 1 && ql != (ull)l_seq;
                bad = worse;
                if (!bad) {
                    const int rlen = tid < Rf.n ? Rf.len[tid] : -1;                   // (< 0: the contig is not loaded)
                    noseq = R.n_cig == 0 || l_seq == 0;
                    offref = !noseq && (rlen < 0 || (ull)pos + rl > (ull)rlen);
                    walked = !noseq && !offref;
                }
                if (walked) {
                    // every M = X base lies inside [0, l_seq) of the sequence and inside [0, rlen) of the contig
                    const ull seq = R.seq(), qual = R.qual(), lim = qual + (ull)l_seq;
                    const ull g0 = Rf.off[tid] * 2ull;                                // the store nibble of base 0 of the contig
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
                                while (x) {                                          // (rare: a non-zero nibble)
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
                        r += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? (ull)len : 0ull;
                        q += (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ? (ull)len : 0ull;
                    }
                }
            }
        }
    }
    const bool noisy = walked && ne > TDT_SNV_MAX_PER_READ, ok = walked && !noisy;
    cnt[SN_MALFORMED] = (ull)__popcll(__ballot(live && bad));
    cnt[SN_NO_SEQUENCE] = (ull)__popcll(__ballot(noseq));
    cnt[SN_OFF_REFERENCE] = (ull)__popcll(__ballot(offref));
    cnt[SN_NOISY] = (ull)__popcll(__ballot(noisy));
    cnt[SN_READS_WITH_EVENTS] = (ull)__popcll(__ballot(ok && ne > 0));
    // ---- the tile's keys in LDS: slots by a prefix sum of the reads' event counts
    const int mine = ok ? (int)ne : 0;
    cnt[SN_MISMATCHES] = (ull)mine;
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
    for (int w = 0; w < SNV_BLOCK / 64; w++) {
        base += w < wave ? s_wkeys[w] : 0;
        nk += s_wkeys[w];
    }
    const int slot = base + incl - mine;                           // (+ mine <= nk <= 8 x the reads of the tile)
#pragma unroll
    for (int e = 0; e < TDT_SNV_MAX_PER_READ; e++) {
        if (e < mine) {
            const ull k1 = ((ull)(unsigned)tid << 32) | (ull)eP[e];
            const ull k2 = ((ull)((eC >> (4 * e)) & 0xfu) << 1) | (ull)rev;
            or1 |= k1, nand1 |= ~k1, or2 |= k2, nand2 |= ~k2;
            s_k1[slot + e] = k1;
            s_k2[slot + e] = k2;
        }
    }
    // ---- the tile's counters: merged per wave, then over the workgroup, ONE atomic per non-zero counter
    cnt[SN_ALIGNED_BASES] = tdt_wave_reduce<tdt_sum>(cnt[SN_ALIGNED_BASES]), cnt[SN_LOW_QUALITY] = tdt_wave_reduce<tdt_sum>(cnt[SN_LOW_QUALITY]);
    cnt[SN_MISMATCHES] = tdt_wave_reduce<tdt_sum>(cnt[SN_MISMATCHES]);
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
        for (int w = 0; w < SNV_BLOCK / 64; w++) v = t < SN_PUSH_N ? v + s_cnt[w][t] : v | s_cnt[w][t];
        if (v) {
            if (t < SN_PUSH_N) atomicAdd(&st[t], v);
            else atomicOr(&st[ST_OR1 + (t - SN_PUSH_N)], v);
        }
    }
    __syncthreads();
    for (int k = t; k < nk; k += SNV_BLOCK) {                      // (consecutive lanes, consecutive slots)
        const ull at = s_base + (ull)k;
        if (at < cap) {
            k1s[at] = s_k1[k];
            k2s[at] = s_k2[k];
        } else {
            st[KS_OVERFLOW] = 1;                                   // (cannot happen: the host reserved 8 slots for every read of the batch)
        }
    }
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
    if (n_contigs > SNV_MAX_CONTIGS || min_mapq < 0 || min_mapq > 255 || min_bq < 0 || min_bq > TDT_SNV_MAX_BQ || capacity >= (1ull << 40)) {
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

extern "C" int tdt_snv_destroy(tdt_snv *h) {
    if (!h) return TDT_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);        // (no kernel of the stream still writes the store)
    snv_free(h);
    return TDT_OK;
}

extern "C" int tdt_snv_reset(tdt_snv *h) {
    if (!h) {
        tdt_set_error("tdt_snv_reset: bad argument");
        return TDT_E_ARG;
    }
    return ks_reset(&h->S);
}

static int snv_launch(tdt_snv *h, const SnvIn &I, size_t n, size_t raw_len) {
    const size_t room = n * TDT_SNV_MAX_PER_READ;                  // the bound a read's cap gives
    int rc = ks_reserve(&h->S, room);
    if (rc) return rc;
    const dim3 grid((unsigned)((n + SNV_K_TILE - 1) / SNV_K_TILE));
    hipLaunchKernelGGL(snv_keys, grid, dim3(SNV_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, (unsigned)h->min_bq, h->S.k1,
                       h->S.k2, (ull)h->S.cap, h->S.d_state, tdt_refview{h->ref->d_store, h->ref->d_off, h->ref->d_len, h->ref->n_contigs});
    TDT_CHECK_LAUNCH();
    h->S.upper += room;
    h->S.rows_valid = false;
    return TDT_OK;
}

#define SNV_NEED (TDT_NEED(FLAG) | TDT_NEED(TID) | TDT_NEED(POS) | TDT_NEED(MAPQ) | TDT_NEED(REC_OFF) | TDT_NEED(RAW))

// One batch of the device ingest: d_arrays14 = the pointer table tdt_ingest_arrays filled (TDT_COL_*: a host array of TDT_NCOL device
// pointers).  The launch is enqueued on the context's stream and nothing is waited for — unless the reserve must ask or grow.
extern "C" int tdt_snv_push_device(tdt_snv *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    tdt_batch B;
    const int rc = tdt_batch_view("tdt_snv_push_device", h, d_arrays14, n, raw_len, SNV_NEED, &B);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    return snv_launch(h, SnvIn{B.flag, B.tid, B.pos, B.mapq, B.rec_off, B.raw}, n, raw_len);
}

// The same kernel on host columns and host record bytes (uploaded into the handle's own block).  The stream is synchronised before the
// return: the caller's arrays are free again.
extern "C" int tdt_snv_push(tdt_snv *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off, size_t n,
                            const uint8_t *raw, size_t raw_len) {
    tdt_batch H{}, B;
    H.flag = flag, H.tid = tid, H.pos = pos, H.mapq = mapq, H.rec_off = rec_off, H.raw = raw;
    int rc = tdt_batch_host("tdt_snv_push", h, H, n, raw_len, SNV_NEED);
    if (rc == TDT_OK) rc = tdt_batch_offsets_ascend("tdt_snv_push", rec_off, n);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    rc = tdt_batch_upload("tdt_snv_push", h->ctx, &h->io, H, SNV_NEED, n, raw_len, &B);
    if (rc == TDT_OK) rc = snv_launch(h, SnvIn{B.flag, B.tid, B.pos, B.mapq, B.rec_off, B.raw}, n, raw_len);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

extern "C" int tdt_snv_keys(tdt_snv *h, uint64_t *k1, uint64_t *k2, size_t *n) { return ks_keys(h ? &h->S : nullptr, "tdt_snv", k1, k2, n); }

// sn_out: uint64[TDT_SNV_SN_N], the push counters and the sets of everything pushed so far; *n_rows: the rows tdt_snv_rows will give.
// The store is left as it was.
extern "C" int tdt_snv_finish(tdt_snv *h, uint64_t min_support, uint64_t *sn_out, size_t *n_rows) {
    if (!h || !sn_out || !n_rows) {
        tdt_set_error("tdt_snv_finish: bad argument");
        return TDT_E_ARG;
    }
    if (min_support < 1 || min_support > TDT_SNV_MAX_SUPPORT) {
        tdt_set_error("tdt_snv_finish: min_support %llu (1 ... %d)", (ull)min_support, TDT_SNV_MAX_SUPPORT);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    ull state[KS_WORDS], got[2];
    int rc = ks_stored(&h->S, state);
    if (rc == TDT_OK) rc = ks_finish(&h->S, state, min_support, got);
    if (rc) return rc;
    uint64_t res[SN_N] = {};
    for (int k = 0; k < SN_PUSH_N; k++) res[k] = state[k];
    res[SN_DISTINCT] = got[0];
    res[SN_REPORTED] = got[1];
    memcpy(sn_out, res, sizeof res);
    *n_rows = h->S.n_rows;
    return TDT_OK;
}

extern "C" int tdt_snv_rows(tdt_snv *h, uint64_t *k1, uint64_t *k2, uint32_t *support, uint32_t *rev, size_t *n) {
    return ks_rows(h ? &h->S : nullptr, "tdt_snv", k1, k2, support, rev, n);
}

// device milliseconds of the last finish: [0] sort by K2, [1] gather of K1, [2] sort by K1, [3] gather of K2 + the run-length launches
extern "C" int tdt_snv_timing(tdt_snv *h, double *ms4) {
    if (!h || !ms4) {
        tdt_set_error("tdt_snv_timing: bad argument");
        return TDT_E_ARG;
    }
    for (int k = 0; k < 4; k++) ms4[k] = h->S.ms[k];
    return TDT_OK;
}

// out3: how often the reserve asked the device for the real count, how often it made a bigger store, the store's capacity now
extern "C" int tdt_snv_reserve_stats(tdt_snv *h, uint64_t *out3) {
    if (!h || !out3) {
        tdt_set_error("tdt_snv_reserve_stats: bad argument");
        return TDT_E_ARG;
    }
    out3[0] = h->S.asks, out3[1] = h->S.grows, out3[2] = h->S.cap;
    return TDT_OK;
}
