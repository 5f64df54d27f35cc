// Read-level QC tables for gfx950 — what the reads of the --sv scan look like (TIDDIT_QC=1): flag counts, MAPQ, read lengths, insert
// sizes, per-cycle base composition and quality, the quality histogram, GC per read, CIGAR sums and indel lengths.  The definition is
// tiddit_qc.py's; every counter is an order-independent uint64 sum, so the result equals the per-read definition exactly.
// A handle keeps the one counter array (TDT_QC_TOTAL uint64, the layout of include/tiddit_hip.h) in HBM; a batch costs TWO launches over
// columns and raw record bytes that are already resident:
//   * qc_fields — lane = read on the coalesced columns (flag, mapq, tid, mate_tid, tlen, l_seq).  A workgroup owns QC_F_TILE consecutive
//     reads and an LDS image of SN / MAPQ / RL / IS (27 KB of uint32).  The flag counters are ballots (one LDS add per wave and counter);
//     the keyed histograms merge the equal keys of a wave before ONE lane adds their number (real data puts most of a wave on mapq 60 and
//     on a few dozen insert sizes), QC_MERGE_ROUNDS leaders at the most, the lanes left after them add for themselves.  A read adds at
//     most one to any counter and a launch holds fewer than 2^31 reads: no uint32 of the image can wrap.
//   * qc_bases — the first kernel here that streams every sequence and quality byte.  A workgroup owns QC_B_TILE consecutive reads, dealt
//     to its four waves in groups of 64 (wave w: groups w, w + 4, ...): a 20-kb read costs what 80 reads of 150 bases cost and holds
//     ONE wave of ONE small tile for that long, not a workgroup of lanes waiting for one lane's loop.  (The groups are dealt, not drawn
//     from an LDS ticket: a loop that leaves on a value one lane fetched is, to the compiler, a loop whose lanes may leave one by one,
//     and it was compiled into one where lanes 1 .. 63 went round again without lane 0 and read its ticket as 0 — for ever.  Every loop
//     and branch of this kernel that the whole wave takes is on a scalar: readfirstlane / readlane, ballots.)  Per group: lane = read for the header (the record is bounded exactly as tdt_alleles bounds one; nothing outside
//     [rec_off, rec_off + 4 + block_size), itself inside raw_len, is read afterwards), then WAVE = read, lanes along the bytes: a lane
//     takes one sequence byte (two bases) and its two quality bytes, 128 bases per step, a long read is a loop of the same wave.  The
//     lanes of a step fall on different cycle rows of the LDS CYC image (row stride 7 dwords: 32 neighbouring rows, 32 banks).  Cycles
//     at and beyond QC_CYCLES share one row: those are counted by ballots in wave-uniform registers and added once per read, not 20 000
//     times to one LDS word.  gc, q20, q30 are ballot sums; equal quality values of a step are merged like the keys above (binned
//     qualities put a wave on four values).  The CIGAR is read twice, lanes along its operations: once for an op code above 8 (the
//     record then counts nothing), once to add.
//     What can grow by more than one per read is uint64 in LDS (SN, QUAL, the shared last row).  The uint32 words: a CYC cell below
//     QC_CYCLES takes one base of a read (+1, qual_sum +255 at the most), a GCR cell one read, an ID cell up to 65535 operations of a
//     read: at most 65535 * QC_B_TILE < 2^32 between the zeroing and the flush of a workgroup.  QC_B_TILE is that bound.
//   * either kernel ends with its workgroup adding the non-zero words of its image to the global array by 64-bit atomics.
#include "tdt_batch.h"
#include "tdt_bam_record.h"

typedef unsigned long long ull;

#define QC_CYCLES 512
#define QC_IS_MAX 2000
#define QC_ID_MAX 64
#define QC_BLOCK 256
#define QC_F_TILE 4096                        // reads of a qc_fields workgroup
#define QC_B_TILE 1024                        // reads of a qc_bases workgroup between zeroing and flush: 65535 * QC_B_TILE < 2^32
#define QC_MERGE_ROUNDS 4

static_assert(TDT_QC_OFF_MAPQ == TDT_QC_SN_N && TDT_QC_OFF_RL == TDT_QC_OFF_MAPQ + 256 && TDT_QC_OFF_IS == TDT_QC_OFF_RL + QC_CYCLES + 1 &&
              TDT_QC_OFF_CYC == TDT_QC_OFF_IS + 3 * (QC_IS_MAX + 1) && TDT_QC_OFF_QUAL == TDT_QC_OFF_CYC + 7 * (QC_CYCLES + 1) &&
              TDT_QC_OFF_GCR == TDT_QC_OFF_QUAL + 256 && TDT_QC_OFF_ID == TDT_QC_OFF_GCR + 101 && TDT_QC_TOTAL == TDT_QC_OFF_ID + 2 * QC_ID_MAX,
              "the layout of include/tiddit_hip.h is the one of these constants");
static_assert(65535ull * QC_B_TILE < (1ull << 32) && 255ull * QC_B_TILE < (1ull << 32), "a uint32 LDS word cannot wrap inside a tile");

// the SN rows, in the order of the file
enum { SN_RECORDS = 0, SN_SECONDARY, SN_SUPPLEMENTARY, SN_PRIMARY, SN_QC_FAIL, SN_DUPLICATE, SN_UNMAPPED, SN_MAPPED, SN_PAIRED, SN_READ1, SN_READ2,
       SN_PROPER_PAIR, SN_MATE_UNMAPPED, SN_BOTH_MAPPED, SN_MATE_OTHER, SN_MATE_OTHER_Q5, SN_REVERSE, SN_MAPQ0, SN_MALFORMED, SN_BASES,
       SN_NO_SEQ, SN_NO_QUAL, SN_Q20, SN_Q30, SN_ALIGNED, SN_SOFT, SN_HARD, SN_INSERTED, SN_DELETED, SN_SKIPPED, SN_INSERTIONS, SN_DELETIONS,
       SN_CLIPPED, SN_N };
static_assert(SN_N == TDT_QC_SN_N, "SN rows");

struct tdt_qc {
    tdt_ctx *ctx;
    ull *d_cnt;                               // TDT_QC_TOTAL
    tdt_batch_io io;                          // columns + raw bytes of the host entry
};

struct QcIn {
    const uint16_t *flag;
    const uint8_t *mapq;
    const int32_t *tid, *mate_tid, *tlen, *l_seq;
    const uint64_t *rec_off;
    const uint8_t *raw;
};

// The value lane k holds, in a scalar register: what the wave branches and loops on must be uniform FOR THE COMPILER too (see qc_bases
// above).  A value that comes out of __shfl is a vector register to it.
__device__ __forceinline__ unsigned qc_lane(unsigned v, int k) { return (unsigned)__builtin_amdgcn_readlane((int)v, k); }
__device__ __forceinline__ ull qc_lane64(ull v, int k) { return (ull)qc_lane((unsigned)v, k) | ((ull)qc_lane((unsigned)(v >> 32), k) << 32); }

// tab[key] += 1 for every lane with `on`, the equal keys of the wave merged: called by all 64 lanes together
template <class T> __device__ __forceinline__ void qc_add_merged(T *tab, unsigned key, bool on, int lane) {
    ull todo = __ballot(on);
    for (int r = 0; r < QC_MERGE_ROUNDS && todo; r++) {             // (uniform: every lane holds the same mask)
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned lk = qc_lane(key, leader);
        const ull same = __ballot(on && key == lk);
        if (lane == leader) atomicAdd(&tab[lk], (T)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&tab[key], (T)1);
}

__global__ __launch_bounds__(QC_BLOCK) void qc_fields(QcIn I, int n, ull *__restrict__ g) {
    __shared__ unsigned s[TDT_QC_OFF_CYC];                           // SN, MAPQ, RL, IS at their global indices
    const int t = threadIdx.x, lane = t & 63;
    for (int k = t; k < TDT_QC_OFF_CYC; k += QC_BLOCK) s[k] = 0;
    __syncthreads();
    const long long lo = (long long)blockIdx.x * QC_F_TILE, hi = lo + QC_F_TILE < n ? lo + QC_F_TILE : n;
    for (long long base = lo; base < hi; base += QC_BLOCK) {
        const long long i = base + t;
        const bool on = i < hi;
        unsigned f = 0, q = 0;
        int tid = 0, mtid = 0, tlen = 0, lseq = 0;
        if (on) {
            f = I.flag[i];
            q = I.mapq[i];
            tid = I.tid[i];
            mtid = I.mate_tid[i];
            tlen = I.tlen[i];
            lseq = I.l_seq[i];
        }
        const bool prim = on && (f & 0x900u) == 0, mapped = prim && !(f & 0x4u), paired = prim && (f & 0x1u);
        const bool both = paired && !(f & 0xCu), other = both && mtid != tid, inS = on && (f & 0xB00u) == 0;
#define QC_SN(idx, cond)                                                \
        {                                                               \
            const ull m_ = __ballot(cond);                              \
            if (lane == 0 && m_) atomicAdd(&s[idx], (unsigned)__popcll(m_)); \
        }
        QC_SN(SN_RECORDS, on)
        QC_SN(SN_SECONDARY, on && (f & 0x100u))
        QC_SN(SN_SUPPLEMENTARY, on && (f & 0x800u))
        QC_SN(SN_PRIMARY, prim)
        QC_SN(SN_QC_FAIL, prim && (f & 0x200u))
        QC_SN(SN_DUPLICATE, prim && (f & 0x400u))
        QC_SN(SN_UNMAPPED, prim && (f & 0x4u))
        QC_SN(SN_MAPPED, mapped)
        QC_SN(SN_PAIRED, paired)
        QC_SN(SN_READ1, prim && (f & 0x40u))
        QC_SN(SN_READ2, prim && (f & 0x80u))
        QC_SN(SN_PROPER_PAIR, paired && (f & 0x2u))
        QC_SN(SN_MATE_UNMAPPED, paired && (f & 0x8u))
        QC_SN(SN_BOTH_MAPPED, both)
        QC_SN(SN_MATE_OTHER, other)
        QC_SN(SN_MATE_OTHER_Q5, other && q >= 5)
        QC_SN(SN_REVERSE, mapped && (f & 0x10u))
        QC_SN(SN_MAPQ0, mapped && q == 0)
#undef QC_SN
        qc_add_merged(s, TDT_QC_OFF_MAPQ + q, mapped, lane);
        const int rl = lseq < 0 ? 0 : lseq > QC_CYCLES ? QC_CYCLES : lseq;
        qc_add_merged(s, TDT_QC_OFF_RL + (unsigned)rl, inS, lane);
        const bool is_on = inS && (f & 0x1u) && !(f & 0xCu) && mtid == tid && tlen > 0;
        const unsigned col = (!(f & 0x10u) && (f & 0x20u)) ? 0u : ((f & 0x10u) && !(f & 0x20u)) ? 1u : 2u;
        const unsigned row = tlen > QC_IS_MAX ? QC_IS_MAX : (tlen > 0 ? (unsigned)tlen : 0u);
        qc_add_merged(s, TDT_QC_OFF_IS + row * 3u + col, is_on, lane);
    }
    __syncthreads();
    for (int k = t; k < TDT_QC_OFF_CYC; k += QC_BLOCK) {
        const unsigned v = s[k];
        if (v) atomicAdd(&g[k], (ull)v);
    }
}

__global__ __launch_bounds__(QC_BLOCK) void qc_bases(QcIn I, int n, ull raw_len, ull *__restrict__ g) {
    __shared__ unsigned s_cyc[QC_CYCLES * 7], s_gcr[101], s_id[QC_ID_MAX * 2];
    __shared__ ull s_sn[SN_N], s_qual[256], s_last[7];
    const int t = threadIdx.x, lane = t & 63;
    for (int k = t; k < QC_CYCLES * 7; k += QC_BLOCK) s_cyc[k] = 0;
    if (t < 101) s_gcr[t] = 0;
    if (t < QC_ID_MAX * 2) s_id[t] = 0;
    if (t < SN_N) s_sn[t] = 0;
    s_qual[t] = 0;
    if (t < 7) s_last[t] = 0;
    __syncthreads();
    const long long lo = (long long)blockIdx.x * QC_B_TILE, hi = lo + QC_B_TILE < n ? lo + QC_B_TILE : n;
    const uint8_t *__restrict__ raw = I.raw;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);         // (a scalar: the loops below branch on scalars only)
    for (long long first = lo + wave * 64; first < hi; first += QC_BLOCK) {      // the tile's groups of 64 reads, dealt round the waves
        // ---- lane = read: the flag, the header, the bounds
        const long long i = first + lane;
        bool inS = false, bad = false, hasq = false;
        unsigned f = 0, n_cig = 0;
        int l_seq = 0;
        ull cig_off = 0;
        if (i < hi) {
            f = I.flag[i];
            if ((f & 0xB00u) == 0) {
                inS = true;
                bad = true;
                const ull ro = I.rec_off[i];
                if (TDT_REC_HEADER_INSIDE(raw_len, ro)) {
                    const tdt_rec R = TDT_REC_READ(raw, ro);
                    n_cig = R.n_cig;
                    l_seq = R.l_seq;
                    if (l_seq >= 0 && TDT_REC_FITS(R, raw_len)) {
                        bad = false;
                        cig_off = R.cig();
                        if (l_seq > 0) hasq = raw[R.qual()] != 0xff;    // (the first quality byte says whether the read has any)
                    }
                }
            }
        }
        // (wave-uniform sums of the group, added to the image once)
        ull a_bad = (ull)__popcll(__ballot(inS && bad)), a_bases = 0, a_noseq = 0, a_noqual = 0, a_q20 = 0, a_q30 = 0, a_clipped = 0;
        ull live = __ballot(inS && !bad);
        while (live) {                                               // (uniform) ---- wave = read, lanes along its bytes
            const int k = __ffsll((long long)live) - 1;
            live &= live - 1;
            const ull r_cig = qc_lane64(cig_off, k);
            const unsigned r_ncig = qc_lane(n_cig, k), r_f = qc_lane(f, k);
            const long long L = (int)qc_lane((unsigned)l_seq, k);
            const bool r_hasq = qc_lane((unsigned)hasq, k) != 0;
            const uint8_t *cig = raw + r_cig, *seq = cig + 4ull * r_ncig, *qual = seq + (L + 1) / 2;
            bool badop = false;
            for (unsigned j0 = 0; j0 < r_ncig; j0 += 64) {
                const unsigned j = j0 + lane;
                if (j < r_ncig) badop |= (tdt_ld_u32(cig + 4ull * j) & 0xf) > 8;
            }
            if (__any(badop)) {
                a_bad++;
                continue;
            }
            const bool rev = r_f & 0x10u;
            a_bases += (ull)L;
            if (L == 0) a_noseq++;
            else if (!r_hasq) a_noqual++;
            if (!(r_f & 0x4u) && r_ncig) {
                bool clip = false;
                for (unsigned j0 = 0; j0 < r_ncig; j0 += 64) {
                    const unsigned j = j0 + lane;
                    if (j < r_ncig) {
                        const unsigned cw = tdt_ld_u32(cig + 4ull * j), op = cw & 0xf, len = cw >> 4;
                        const int sn = (op == 0 || op == 7 || op == 8) ? SN_ALIGNED : op == 1 ? SN_INSERTED : op == 2 ? SN_DELETED : op == 3 ? SN_SKIPPED
                                     : op == 4 ? SN_SOFT : op == 5 ? SN_HARD : -1;
                        if (sn >= 0 && len) atomicAdd(&s_sn[sn], (ull)len);
                        if ((op == 1 || op == 2) && len) {
                            atomicAdd(&s_sn[op == 1 ? SN_INSERTIONS : SN_DELETIONS], 1ull);
                            atomicAdd(&s_id[((len > QC_ID_MAX ? QC_ID_MAX : len) - 1) * 2 + (op == 2)], 1u);
                        }
                        clip |= op == 4 || op == 5;
                    }
                }
                if (__any(clip)) a_clipped++;
            }
            ull gc = 0, last_q = 0;                                  // last_q: this lane's share of the shared row's qual_sum
            unsigned last_c[5] = {0, 0, 0, 0, 0};
            for (long long b0 = 0; b0 < L; b0 += 128) {              // (uniform)
                const long long i0 = b0 + 2 * lane;
                const bool v0 = i0 < L, v1 = i0 + 1 < L;             // (v1 false on the odd last base: the pad nibble is not a base)
                const unsigned sb = v0 ? seq[i0 >> 1] : 0u;
                unsigned qq[2] = {0, 0};
                if (r_hasq) {
                    if (v0) qq[0] = qual[i0];
                    if (v1) qq[1] = qual[i0 + 1];
                }
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const bool v = h ? v1 : v0;
                    const unsigned nib = h ? (sb & 0xf) : (sb >> 4), q = qq[h];
                    unsigned col = nib == 1 ? 0u : nib == 2 ? 1u : nib == 4 ? 2u : nib == 8 ? 3u : 4u;
                    if (rev && col < 4) col = 3 - col;               // A <-> T, C <-> G
                    gc += (ull)__popcll(__ballot(v && (nib == 2 || nib == 4)));
                    const long long idx = i0 + h, cyc = rev ? L - 1 - idx : idx;
                    const bool head = v && cyc < QC_CYCLES, tail = v && cyc >= QC_CYCLES;
                    if (head) {
                        atomicAdd(&s_cyc[cyc * 7 + col], 1u);
                        if (r_hasq) {
                            atomicAdd(&s_cyc[cyc * 7 + 5], q);
                            atomicAdd(&s_cyc[cyc * 7 + 6], 1u);
                        }
                    }
                    if (__any(tail)) {
#pragma unroll
                        for (unsigned c = 0; c < 5; c++) last_c[c] += (unsigned)__popcll(__ballot(tail && col == c));
                        if (tail) last_q += q;
                    }
                    if (r_hasq) {
                        a_q20 += (ull)__popcll(__ballot(v && q >= 20));
                        a_q30 += (ull)__popcll(__ballot(v && q >= 30));
                        qc_add_merged(s_qual, q, v, lane);
                    }
                }
            }
            if (L > QC_CYCLES) {
                last_q = tdt_wave_reduce<tdt_sum>(last_q);
                if (lane == 0) {
#pragma unroll
                    for (int c = 0; c < 5; c++)
                        if (last_c[c]) atomicAdd(&s_last[c], (ull)last_c[c]);
                    if (r_hasq) {
                        atomicAdd(&s_last[5], last_q);
                        atomicAdd(&s_last[6], (ull)(L - QC_CYCLES));
                    }
                }
            }
            if (L > 0 && lane == 0) atomicAdd(&s_gcr[(unsigned)(100ull * gc / (ull)L)], 1u);
        }
        if (lane == 0) {
            if (a_bad) atomicAdd(&s_sn[SN_MALFORMED], a_bad);
            if (a_bases) atomicAdd(&s_sn[SN_BASES], a_bases);
            if (a_noseq) atomicAdd(&s_sn[SN_NO_SEQ], a_noseq);
            if (a_noqual) atomicAdd(&s_sn[SN_NO_QUAL], a_noqual);
            if (a_q20) atomicAdd(&s_sn[SN_Q20], a_q20);
            if (a_q30) atomicAdd(&s_sn[SN_Q30], a_q30);
            if (a_clipped) atomicAdd(&s_sn[SN_CLIPPED], a_clipped);
        }
    }
    __syncthreads();
    for (int k = t; k < QC_CYCLES * 7; k += QC_BLOCK) {
        const unsigned v = s_cyc[k];
        if (v) atomicAdd(&g[TDT_QC_OFF_CYC + k], (ull)v);
    }
    if (t < 7 && s_last[t]) atomicAdd(&g[TDT_QC_OFF_CYC + QC_CYCLES * 7 + t], s_last[t]);
    if (t < 101 && s_gcr[t]) atomicAdd(&g[TDT_QC_OFF_GCR + t], (ull)s_gcr[t]);
    if (t < QC_ID_MAX * 2 && s_id[t]) atomicAdd(&g[TDT_QC_OFF_ID + t], (ull)s_id[t]);
    if (t < SN_N && s_sn[t]) atomicAdd(&g[t], s_sn[t]);
    if (s_qual[t]) atomicAdd(&g[TDT_QC_OFF_QUAL + t], s_qual[t]);
}

static void qc_free(tdt_qc *h) {
    if (h->d_cnt) (void)hipFree(h->d_cnt);
    if (h->io.d) (void)hipFree(h->io.d);
    delete h;
}

extern "C" size_t tdt_qc_size(void) { return TDT_QC_TOTAL; }

extern "C" int tdt_qc_create(tdt_ctx *ctx, tdt_qc **out) {
    if (!ctx || !out) {
        tdt_set_error("tdt_qc_create: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_qc *h = new tdt_qc{ctx, nullptr, {nullptr, 0}};
    if (tdt_dev_malloc((void **)&h->d_cnt, (size_t)TDT_QC_TOTAL * 8) != hipSuccess) {
        qc_free(h);
        tdt_set_error("tdt_qc_create: out of device memory");
        return TDT_E_NOMEM;
    }
    const hipError_t e = hipMemsetAsync(h->d_cnt, 0, (size_t)TDT_QC_TOTAL * 8, ctx->stream);
    if (e != hipSuccess) {
        qc_free(h);
        TDT_HIP(e);
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_qc_destroy(tdt_qc *h) {
    if (!h) return TDT_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);        // (no kernel of the stream still adds to the counters)
    qc_free(h);
    return TDT_OK;
}

extern "C" int tdt_qc_reset(tdt_qc *h) {
    if (!h) {
        tdt_set_error("tdt_qc_reset: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    TDT_HIP(hipMemsetAsync(h->d_cnt, 0, (size_t)TDT_QC_TOTAL * 8, h->ctx->stream));
    return TDT_OK;
}

static int qc_launch(tdt_qc *h, const QcIn &I, size_t n, size_t raw_len) {
    hipStream_t st = h->ctx->stream;
    hipLaunchKernelGGL(qc_fields, dim3((unsigned)((n + QC_F_TILE - 1) / QC_F_TILE)), dim3(QC_BLOCK), 0, st, I, (int)n, h->d_cnt);
    TDT_CHECK_LAUNCH();
    hipLaunchKernelGGL(qc_bases, dim3((unsigned)((n + QC_B_TILE - 1) / QC_B_TILE)), dim3(QC_BLOCK), 0, st, I, (int)n, (ull)raw_len, h->d_cnt);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

#define QC_NEED (TDT_NEED(FLAG) | TDT_NEED(MAPQ) | TDT_NEED(TID) | TDT_NEED(MATE_TID) | TDT_NEED(TLEN) | TDT_NEED(L_SEQ) | TDT_NEED(REC_OFF) | TDT_NEED(RAW))

// One batch of the device ingest: d_arrays14 = the pointer table tdt_ingest_arrays filled (TDT_COL_*: a host array of TDT_NCOL device
// pointers).  The two launches are enqueued on the context's stream; nothing is waited for and nothing is allocated.
extern "C" int tdt_qc_push_device(tdt_qc *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    tdt_batch B;
    const int rc = tdt_batch_view("tdt_qc_push_device", h, d_arrays14, n, raw_len, QC_NEED, &B);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    return qc_launch(h, QcIn{B.flag, B.mapq, B.tid, B.mate_tid, B.tlen, B.l_seq, B.rec_off, B.raw}, n, raw_len);
}

// The same kernels on host columns and host record bytes (uploaded into the handle's own block).  The stream is synchronised before the
// return: the caller's arrays are free again.
extern "C" int tdt_qc_push(tdt_qc *h, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *mate_tid, const int32_t *tlen,
                           const int32_t *l_seq, const uint64_t *rec_off, size_t n, const uint8_t *raw, size_t raw_len) {
    tdt_batch H{}, B;
    H.flag = flag, H.mapq = mapq, H.tid = tid, H.mate_tid = mate_tid, H.tlen = tlen, H.l_seq = l_seq, H.rec_off = rec_off, H.raw = raw;
    int rc = tdt_batch_host("tdt_qc_push", h, H, n, raw_len, QC_NEED);
    if (rc == TDT_OK) rc = tdt_batch_offsets_ascend("tdt_qc_push", rec_off, n);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    rc = tdt_batch_upload("tdt_qc_push", h->ctx, &h->io, H, QC_NEED, n, raw_len, &B);
    if (rc == TDT_OK) rc = qc_launch(h, QcIn{B.flag, B.mapq, B.tid, B.mate_tid, B.tlen, B.l_seq, B.rec_off, B.raw}, n, raw_len);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

// uint64[TDT_QC_TOTAL] to the host, behind everything pushed so far
extern "C" int tdt_qc_counts(tdt_qc *h, uint64_t *out) {
    if (!h || !out) {
        tdt_set_error("tdt_qc_counts: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    TDT_HIP(hipMemcpyAsync(out, h->d_cnt, (size_t)TDT_QC_TOTAL * 8, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}

// ... to device memory.  The stream is synchronised before the return.
extern "C" int tdt_qc_counts_device(tdt_qc *h, uint64_t *d_out) {
    if (!h || !d_out || ((uintptr_t)d_out & 7)) {
        tdt_set_error("tdt_qc_counts_device: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    TDT_HIP(hipMemcpyAsync(d_out, h->d_cnt, (size_t)TDT_QC_TOTAL * 8, hipMemcpyDeviceToDevice, st));
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}
