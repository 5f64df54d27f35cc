// Exact per-base depth for gfx950 — the number of eligible reads of the --sv scan with an aligned base (M = X) at every reference
// position, CIGAR-exact (a deletion or a skip covers nothing), and the genotype rule of TIDDIT_SMALL_VCF gathered from it.  The
// definition is tiddit_pileup.py's (spans_of_read, depth_of) and tiddit_small_vcf.py's (genotype); every result is an order-independent
// integer, so it equals the definition exactly.
//   * the array: ONE int32 per reference base plus a guard slot per contig, N = sum(lengths) + n_contigs slots (4 B per base: 12.4 GB
//     for a 3.1-Gb genome, hence 64-bit indices everywhere), contig t at off[t], zeroed at create and at reset.  It is allocated in
//     whole tiles of PILE_TILE slots, so the scan launches load and store 16 bytes without a tail; the slots behind N stay zero.
//   * pile_spans — ONE launch per batch, on the columns and record bytes that are already resident, enqueued beside snv_keys and
//     indel_keys and waiting for nothing: there is no store, so no reserve and no ask.  The read gate (ks_read_gate) and the record
//     open (KS_OPEN) are the keyed consumers'; behind them lane = compacted read.  A first pass over the CIGAR (tdt_cig_span_of)
//     decides malformed BEFORE anything is added; the walk then merges touching M = X stretches in registers and hands out one span at
//     a time: the wave loops while any lane still has one, and per round every lane adds +1 at off + start and -1 at off + end (a
//     span ending at the contig's length puts its -1 into the guard).  There is no cap on the spans of a read.
//     THE MERGE of equal addresses: the compacted reads of a workgroup keep the batch's order, which is the file's, so in
//     coordinate-sorted input equal starts (and, for equal read lengths, equal ends) sit in NEIGHBOURING lanes.  A lane whose address
//     differs from the lane below it is a head; the ballot of the heads gives every head the length of its run, and only heads issue
//     the atomic, with the run's length.  That is one shuffle and one ballot per round whatever the depth (the leader loop of al_count
//     costs a shuffle and a ballot per DISTINCT address, up to 64 per round, where most starts of a 30x library differ); equal
//     addresses in lanes that are not neighbours (unsorted input) are added by more than one atomic, which is the same sum.
//     The atomics return nothing.  Measured (profiles/small_vcf_240mb.md): 0.36 ms per batch of 5.3 M 150-bp reads, beside 0.25 ms of
//     indel_keys and 1.06 ms of snv_keys on the same batches, and the job's scan stage stays inside the spread of the runs without the
//     switch — so the per-workgroup LDS window with a flush of its non-zero words, the allowed second step, was not built.
//   Resources (the compiler's remarks, gfx950): pile_spans 38 VGPRs, 1264 B of LDS; pile_tile_sums 36 VGPRs, 16 B; pile_tile_scan 34 VGPRs,
//   16 B; pile_genotype 21 VGPRs, none; ks_carry_sum 22 VGPRs, 16 B; no scratch in any of them, 8 waves per SIMD each.
//   * tdt_pile_finish — once per job: the in-place inclusive prefix sum over all the slots in three plain launches, none of whose
//     workgroups waits for another: pile_tile_sums (a sum per tile), ks_carry_sum (tdt_keyscan.h: one workgroup turns the tile sums
//     into the sums in front of each tile), pile_tile_scan (scan and write).  The array is read twice and written once.
//   * pile_genotype — one launch per table, lane = row: DP0 gathered at (tid, P - 1), then OTHER, the three PL, GT, GQ and the
//     support-above-depth flag of tiddit_small_vcf.genotype, in 64-bit integers.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"                 // (the gate, the open and the push path are used; the store is not)
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "tdt_keystore.h"
#pragma clang diagnostic pop

typedef unsigned long long ull;

#define PILE_BLOCK 256
#define PILE_TILE 8192                        // slots of a scan workgroup: KS_BLOCK lanes x 4 slots (16 bytes) x PILE_ROUNDS rounds
#define PILE_ROUNDS (PILE_TILE / (KS_BLOCK * 4))
static_assert(PILE_TILE % (KS_BLOCK * 4) == 0, "whole rounds of 16-byte loads");

// the SN rows, in the order of tiddit_pileup.SN
enum { PN_RECORDS = 0, PN_ELIGIBLE, PN_MALFORMED, PN_NO_CIGAR, PN_SPANS, PN_COVERED, PN_CLAMPED, PN_N };
static_assert(PN_N == TDT_PILE_SN_N, "SN rows");

struct tdt_pile {
    tdt_ctx *ctx;
    int n_contigs, min_mapq;
    ull n_slots, n_tiles;                     // N; the tiles the array is allocated in
    int *d;                                   // n_tiles * PILE_TILE slots
    ull *d_off;                               // n_contigs: the first slot of each contig
    int *d_len;                               // n_contigs
    int *d_tile;                              // n_tiles: the scan's tile sums
    ull *d_state;                             // PN_N counters
    std::vector<ull> off;
    std::vector<int> len;
    bool finished;
    tdt_batch_io io;                          // columns + raw bytes of the host entry
    tdt_batch_io rows;                        // the rows and results of the host genotype entry
    hipEvent_t ev[6];
    double ms[4];                             // tile sums, carry, scan + write, the last genotype launch
};

// +sign x (the lanes of the run) at d[key], issued by the run's head: a run = neighbouring lanes with the same key (~0: no span)
__device__ __forceinline__ void pile_add(int *__restrict__ d, ull key, int sign, int lane) {
    const ull below = __shfl_up(key, 1);
    const bool head = lane == 0 || key != below;
    const ull heads = __ballot(head);
    if (head && key != ~0ull) {
        const ull above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int run = above ? __builtin_ctzll(above) + 1 : 64 - lane;
        (void)__hip_atomic_fetch_add(&d[key], sign * run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(PILE_BLOCK) void pile_spans(ks_cols I, int n, ull raw_len, unsigned min_mapq, int n_contigs, const ull *__restrict__ off,
                                                         const int *__restrict__ len, int *__restrict__ d, ull *__restrict__ st) {
    __shared__ ull s_cnt[PILE_BLOCK / 64][PN_N];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long lo = (long long)blockIdx.x * PILE_BLOCK, hi = lo + PILE_BLOCK < n ? lo + PILE_BLOCK : n;
    ull cnt[PN_N] = {0, 0, 0, 0, 0, 0, 0};
    // ---- lane = read: the filters on the columns; then lane = compacted read
    const ks_gated G = ks_read_gate<PILE_BLOCK>(I, lo, hi, min_mapq, cnt[PN_RECORDS], cnt[PN_ELIGIBLE]);
    const bool live = t < G.live;
    bool bad = live, nocig = false, more = false;
    ks_read A{};
    const uint8_t *__restrict__ raw = I.raw;
    const uint8_t *cig = raw;
    unsigned n_cig = 0, clen = 0;
    ull base = 0;
    if (live && KS_OPEN(A, I, G.read, raw_len)) {
        // ---- the record is bounded: sum its CIGAR first, so that a malformed record adds nothing
        cig = raw + A.R.cig();
        const tdt_cig_span C = tdt_cig_span_of(cig, A.R.n_cig);
        bad = C.malformed(A.pos, A.R.l_seq, A.R.n_cig) || A.tid >= n_contigs;
        if (!bad) {
            nocig = A.R.n_cig == 0;
            more = !nocig;
        }
        if (more) n_cig = A.R.n_cig, base = off[A.tid], clen = (unsigned)len[A.tid];
    }
    // ---- the walk: r < 2^31 throughout (pos + the reference length is at most 2^31 - 1)
    unsigned j = 0, r = (unsigned)A.pos, cs = 0, ce = 0;
    bool open = false;
    while (__any(more)) {                                          // (uniform: one span of every lane that still has one per round)
        bool have = false;
        unsigned s = 0, e = 0;
        if (more) {
            while (j < n_cig) {
                const unsigned w = tdt_ld_u32(cig + 4ull * j), op = w & 0xfu, l = w >> 4;
                j++;
                if (op == 0 || op == 7 || op == 8) {
                    if (l) {
                        const bool split = open && r != ce;
                        if (split) s = cs, e = ce, have = true;
                        if (split || !open) cs = r;
                        open = true;
                        r += l;
                        ce = r;
                        if (split) break;
                    }
                } else if (op == 2 || op == 3) {
                    r += l;
                }
            }
            if (!have) {                                           // (the CIGAR is at its end)
                if (open) s = cs, e = ce, have = true, open = false;
                more = false;
            }
        }
        // every span is clamped to [0, the contig's length]; one that is empty behind that is dropped
        if (have) {
            const bool cut = e > clen;
            cnt[PN_CLAMPED] += cut ? 1 : 0;
            e = cut ? clen : e;
            have = s < e;                                          // (s >= clen: dropped, and cut counted it)
        }
        if (have) cnt[PN_SPANS]++, cnt[PN_COVERED] += (ull)(e - s);
        // (base + s <= base + clen - 1 and base + e <= base + clen, the contig's guard: inside the array)
        pile_add(d, have ? base + s : ~0ull, 1, lane);
        pile_add(d, have ? base + e : ~0ull, -1, lane);
    }
    // ---- the push counters: one atomic per workgroup and non-zero word
    cnt[PN_MALFORMED] = (ull)__popcll(__ballot(live && bad));
    cnt[PN_NO_CIGAR] = (ull)__popcll(__ballot(nocig));
    cnt[PN_SPANS] = tdt_wave_reduce<tdt_sum>(cnt[PN_SPANS]), cnt[PN_COVERED] = tdt_wave_reduce<tdt_sum>(cnt[PN_COVERED]);
    cnt[PN_CLAMPED] = tdt_wave_reduce<tdt_sum>(cnt[PN_CLAMPED]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < PN_N; k++) s_cnt[wave][k] = cnt[k];
    }
    __syncthreads();
    if (t < PN_N) {
        ull v = 0;
        for (int w = 0; w < PILE_BLOCK / 64; w++) v += s_cnt[w][t];
        if (v) atomicAdd(&st[t], v);
    }
}

// ---- the scan.  tile_sum[tile] = the sum of the tile's slots
__global__ __launch_bounds__(KS_BLOCK) void pile_tile_sums(const int *__restrict__ d, int *__restrict__ tile_sum) {
    __shared__ int s[KS_BLOCK / 64];
    const int t = threadIdx.x;
    const int4 *__restrict__ p = (const int4 *)(d + (ull)blockIdx.x * PILE_TILE);
    int acc = 0;
#pragma unroll
    for (int r = 0; r < PILE_ROUNDS; r++) {
        const int4 v = p[r * KS_BLOCK + t];
        acc += v.x + v.y + v.z + v.w;
    }
    acc = tdt_wave_reduce<tdt_sum>(acc);
    if ((t & 63) == 0) s[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        int all = 0;
        for (int w = 0; w < KS_BLOCK / 64; w++) all += s[w];
        tile_sum[blockIdx.x] = all;
    }
}

// every slot becomes the sum of all slots up to and including it; tile_sum holds the sums in front of each tile (ks_carry_sum)
__global__ __launch_bounds__(KS_BLOCK) void pile_tile_scan(int *__restrict__ d, const int *__restrict__ tile_sum) {
    __shared__ int s[KS_BLOCK / 64];
    const int t = threadIdx.x;
    int4 *__restrict__ p = (int4 *)(d + (ull)blockIdx.x * PILE_TILE);
    int running = tile_sum[blockIdx.x];
    for (int r = 0; r < PILE_ROUNDS; r++) {                        // (uniform: every thread takes every round)
        int4 v = p[r * KS_BLOCK + t];
        v.y += v.x, v.z += v.y, v.w += v.z;
        int all;
        const int incl = ks_block_scan<tdt_sum>(v.w, 0, s, t, &all);
        const int add = running + incl - v.w;
        v.x += add, v.y += add, v.z += add, v.w += add;
        p[r * KS_BLOCK + t] = v;
        running += all;
    }
}

// ---- the genotype rule, lane = row: out8[row] = DP0, OTHER, PL0, PL1, PL2, GT, GQ, support above depth
__global__ __launch_bounds__(KS_BLOCK) void pile_genotype(const ull *__restrict__ k1, const unsigned *__restrict__ support, int n, int n_contigs,
                                                          const ull *__restrict__ off, const int *__restrict__ len, const int *__restrict__ d,
                                                          uint4 *__restrict__ out8) {
    const int i = blockIdx.x * KS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const ull k = k1[i];
    const ull tid = k >> 32, P = k & 0xffffffffull;
    ull dp0 = 0;
    if (tid < (ull)n_contigs && P >= 1 && P <= (ull)len[tid]) dp0 = (ull)(unsigned)d[off[tid] + P - 1];
    const ull alt = support[i], other = dp0 > alt ? dp0 - alt : 0ull;
    const ull L0 = 20ull * alt, L1 = 3ull * (alt + other), L2 = 20ull * other;
    ull m = L0 < L1 ? L0 : L1;
    m = L2 < m ? L2 : m;
    const unsigned gt = L0 == m ? 0u : L1 == m ? 1u : 2u;
    const ull a = L0 - m, b = L1 - m, c = L2 - m;
    const ull p0 = a < 9999 ? a : 9999, p1 = b < 9999 ? b : 9999, p2 = c < 9999 ? c : 9999;
    // the second smallest of three: the sum less the smallest and the largest
    const ull mn = p0 < p1 ? (p0 < p2 ? p0 : p2) : (p1 < p2 ? p1 : p2), mx = p0 > p1 ? (p0 > p2 ? p0 : p2) : (p1 > p2 ? p1 : p2);
    const ull second = p0 + p1 + p2 - mn - mx;
    out8[2 * (size_t)i] = uint4{(unsigned)dp0, (unsigned)other, (unsigned)p0, (unsigned)p1};
    out8[2 * (size_t)i + 1] = uint4{(unsigned)p2, gt, (unsigned)(second < 99 ? second : 99), alt > dp0 ? 1u : 0u};
}

static void pile_free(tdt_pile *h) {
    if (h->d) (void)hipFree(h->d);
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_len) (void)hipFree(h->d_len);
    if (h->d_tile) (void)hipFree(h->d_tile);
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->io.d) (void)hipFree(h->io.d);
    if (h->rows.d) (void)hipFree(h->rows.d);
    for (int k = 0; k < 6; k++)
        if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
    delete h;
}

extern "C" size_t tdt_pile_sn_size(void) { return TDT_PILE_SN_N; }

extern "C" int tdt_pile_create(tdt_ctx *ctx, int n_contigs, const int64_t *lengths, int min_mapq, tdt_pile **out) {
    if (!ctx || !out || n_contigs < 0 || (n_contigs && !lengths)) {
        tdt_set_error("tdt_pile_create: bad argument");
        return TDT_E_ARG;
    }
    bool in_range = n_contigs < KS_MAX_CONTIGS && min_mapq >= 0 && min_mapq <= 255;
    for (int k = 0; in_range && k < n_contigs; k++) in_range = lengths[k] >= 0 && lengths[k] < (1ll << 31);
    if (!in_range) {
        tdt_set_error("tdt_pile_create: %d contigs (fewer than 2^24), every length 0 ... 2^31 - 1, min_mapq %d (0 ... 255)", n_contigs, min_mapq);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_pile *h = new tdt_pile{};
    h->ctx = ctx;
    h->n_contigs = n_contigs;
    h->min_mapq = min_mapq;
    ull at = 0;
    for (int k = 0; k < n_contigs; k++) {
        h->off.push_back(at);
        h->len.push_back((int)lengths[k]);
        at += (ull)lengths[k] + 1;                                 // (the guard)
    }
    h->n_slots = at;
    h->n_tiles = (at + PILE_TILE - 1) / PILE_TILE;
    if (h->n_tiles == 0) h->n_tiles = 1;
    const size_t nc = n_contigs ? (size_t)n_contigs : 1;
    bool ok = h->n_tiles < (1ull << 31);                           // (a launch's grid, ks_carry_sum's int)
    ok = ok && tdt_dev_malloc((void **)&h->d, (size_t)h->n_tiles * PILE_TILE * 4) == hipSuccess;
    ok = ok && tdt_dev_malloc((void **)&h->d_off, nc * 8) == hipSuccess && tdt_dev_malloc((void **)&h->d_len, nc * 4) == hipSuccess;
    ok = ok && tdt_dev_malloc((void **)&h->d_tile, (size_t)h->n_tiles * 4) == hipSuccess && tdt_dev_malloc((void **)&h->d_state, PN_N * 8) == hipSuccess;
    if (!ok) {
        tdt_set_error("tdt_pile_create: out of device memory (%llu slots of 4 bytes)", h->n_slots);
        pile_free(h);
        return TDT_E_NOMEM;
    }
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemsetAsync(h->d, 0, (size_t)h->n_tiles * PILE_TILE * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_state, 0, PN_N * 8, st);
    if (e == hipSuccess && n_contigs) e = hipMemcpyAsync(h->d_off, h->off.data(), nc * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_contigs) e = hipMemcpyAsync(h->d_len, h->len.data(), nc * 4, hipMemcpyHostToDevice, st);
    for (int k = 0; k < 6 && e == hipSuccess; k++) e = hipEventCreate(&h->ev[k]);
    if (e == hipSuccess) e = hipStreamSynchronize(st);             // (the two tables are the handle's own vectors; simpler to be done with them here)
    if (e != hipSuccess) {
        pile_free(h);
        TDT_HIP(e);
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_pile_destroy(tdt_pile *h) { return ks_destroy(h, pile_free); }

extern "C" int tdt_pile_reset(tdt_pile *h) {
    if (!h) {
        tdt_set_error("tdt_pile_reset: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    TDT_HIP(hipMemsetAsync(h->d, 0, (size_t)h->n_tiles * PILE_TILE * 4, h->ctx->stream));
    TDT_HIP(hipMemsetAsync(h->d_state, 0, PN_N * 8, h->ctx->stream));
    h->finished = false;
    for (int k = 0; k < 4; k++) h->ms[k] = 0;
    return TDT_OK;
}

// the launch of one batch
static auto pile_launch(tdt_pile *h, size_t n, size_t raw_len) {
    return [=](const ks_cols &I) {
        const dim3 grid((unsigned)((n + PILE_BLOCK - 1) / PILE_BLOCK));
        hipLaunchKernelGGL(pile_spans, grid, dim3(PILE_BLOCK), 0, h->ctx->stream, I, (int)n, (ull)raw_len, (unsigned)h->min_mapq, h->n_contigs,
                           (const ull *)h->d_off, (const int *)h->d_len, h->d, h->d_state);
        TDT_CHECK_LAUNCH();
        return TDT_OK;
    };
}

// after the finish the slots hold depths, not differences: a push is refused until the reset
static int pile_still_open(const char *fn, const tdt_pile *h) {
    if (!h || !h->finished) return TDT_OK;
    tdt_set_error("%s: the handle is finished; reset it first", fn);
    return TDT_E_ARG;
}

// the two entries of a batch: ks_push_device / ks_push of tdt_keystore.h
extern "C" int tdt_pile_push_device(tdt_pile *h, const void *const *d_arrays14, size_t n, size_t raw_len) {
    const int rc = pile_still_open("tdt_pile_push_device", h);
    return rc ? rc : ks_push_device("tdt_pile_push_device", h, d_arrays14, n, raw_len, pile_launch(h, n, raw_len));
}

extern "C" int tdt_pile_push(tdt_pile *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off, size_t n,
                             const uint8_t *raw, size_t raw_len) {
    const int rc = pile_still_open("tdt_pile_push", h);
    return rc ? rc : ks_push("tdt_pile_push", h, ks_cols{flag, tid, pos, mapq, rec_off, raw}, n, raw_len, pile_launch(h, n, raw_len));
}

// sn_out: uint64[TDT_PILE_SN_N], the counters of everything pushed so far (the stream is synchronised)
extern "C" int tdt_pile_counters(tdt_pile *h, uint64_t *sn_out) {
    if (!h || !sn_out) {
        tdt_set_error("tdt_pile_counters: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    ull res[PN_N];
    TDT_HIP(hipMemcpyAsync(res, h->d_state, sizeof res, hipMemcpyDeviceToHost, h->ctx->stream));
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    memcpy(sn_out, res, sizeof res);
    return TDT_OK;
}

// The differences become depths.  Every span adds +1 and -1 inside its own contig's slots, the guard included, so every contig's
// differences sum to ZERO: the sum in front of a contig's first slot is zero, and the ONE scan over all the slots is each contig's own
// scan — no segment flags.  (A second finish without a reset changes nothing.)
extern "C" int tdt_pile_finish(tdt_pile *h) {
    if (!h) {
        tdt_set_error("tdt_pile_finish: bad argument");
        return TDT_E_ARG;
    }
    if (h->finished) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const unsigned grid = (unsigned)h->n_tiles;
    TDT_HIP(hipEventRecord(h->ev[0], st));
    hipLaunchKernelGGL(pile_tile_sums, dim3(grid), dim3(KS_BLOCK), 0, st, (const int *)h->d, h->d_tile);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipEventRecord(h->ev[1], st));
    hipLaunchKernelGGL(ks_carry_sum, dim3(1), dim3(KS_BLOCK), 0, st, h->d_tile, (int)h->n_tiles);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipEventRecord(h->ev[2], st));
    hipLaunchKernelGGL(pile_tile_scan, dim3(grid), dim3(KS_BLOCK), 0, st, h->d, (const int *)h->d_tile);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipEventRecord(h->ev[3], st));
    TDT_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 3; k++) {
        float ms = 0;
        TDT_HIP(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
        h->ms[k] = ms;
    }
    h->finished = true;
    return TDT_OK;
}

// out[n] = the depths of contig tid from base start on
extern "C" int tdt_pile_depth(tdt_pile *h, int tid, int64_t start, int64_t n, uint32_t *out) {
    if (!h || (n > 0 && !out) || !h->finished) {
        tdt_set_error(h && !h->finished ? "tdt_pile_depth: no finish since the create or the last reset" : "tdt_pile_depth: bad argument");
        return TDT_E_ARG;
    }
    if (tid < 0 || tid >= h->n_contigs || start < 0 || n < 0 || start > (int64_t)h->len[tid] || n > (int64_t)h->len[tid] - start) {
        tdt_set_error("tdt_pile_depth: contig %d, bases [%lld, %lld + %lld) outside the contig", tid, (long long)start, (long long)start, (long long)n);
        return TDT_E_RANGE;
    }
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    TDT_HIP(hipMemcpyAsync(out, h->d + h->off[tid] + (ull)start, (size_t)n * 4, hipMemcpyDeviceToHost, h->ctx->stream));
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

static int pile_genotype_launch(tdt_pile *h, const ull *d_k1, const unsigned *d_support, size_t n, uint32_t *d_out8) {
    hipStream_t st = h->ctx->stream;
    TDT_HIP(hipEventRecord(h->ev[4], st));
    hipLaunchKernelGGL(pile_genotype, dim3((unsigned)((n + KS_BLOCK - 1) / KS_BLOCK)), dim3(KS_BLOCK), 0, st, d_k1, d_support, (int)n, h->n_contigs,
                       (const ull *)h->d_off, (const int *)h->d_len, (const int *)h->d, (uint4 *)d_out8);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipEventRecord(h->ev[5], st));
    return TDT_OK;
}

static int pile_genotype_refuse(const char *fn, const tdt_pile *h, const void *k1, const void *support, size_t n, const void *out8) {
    if (!h || n >= 0x7fffffffull || (n && (!k1 || !support || !out8))) {
        tdt_set_error("%s: bad argument", fn);
        return TDT_E_ARG;
    }
    if (!h->finished) {
        tdt_set_error("%s: no finish since the create or the last reset", fn);
        return TDT_E_ARG;
    }
    return TDT_OK;
}

// rows in device memory (d_out8: 32 bytes per row, on a 16-byte boundary); enqueued, nothing is waited for
extern "C" int tdt_pile_genotype_device(tdt_pile *h, const uint64_t *d_k1, const uint32_t *d_support, size_t n, uint32_t *d_out8) {
    const int rc = pile_genotype_refuse("tdt_pile_genotype_device", h, d_k1, d_support, n, d_out8);
    if (rc || n == 0) return rc;
    if ((uintptr_t)d_out8 & 15) {
        tdt_set_error("tdt_pile_genotype_device: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    return pile_genotype_launch(h, (const ull *)d_k1, d_support, n, d_out8);
}

// rows in host memory: uploaded into the handle's own block, the same kernel, the results copied back
extern "C" int tdt_pile_genotype(tdt_pile *h, const uint64_t *k1, const uint32_t *support, size_t n, uint32_t *out8) {
    int rc = pile_genotype_refuse("tdt_pile_genotype", h, k1, support, n, out8);
    if (rc || n == 0) return rc;
    TDT_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    struct {
        ull *k1;
        unsigned *sup;
        uint32_t *out;
        size_t lay(void *base, size_t n) {
            tdt_carver cv(base);
            k1 = cv.take<ull>(n), sup = cv.take<unsigned>(n), out = cv.take<uint32_t>(8 * n);
            return cv.size;
        }
    } W;
    const size_t bytes = W.lay(nullptr, n);
    if (bytes > h->rows.cap) {
        TDT_HIP(hipStreamSynchronize(st));
        if (h->rows.d) TDT_HIP(hipFree(h->rows.d));
        h->rows.d = nullptr;
        h->rows.cap = 0;
        if (tdt_dev_malloc(&h->rows.d, bytes) != hipSuccess) {
            tdt_set_error("tdt_pile_genotype: out of device memory (%zu rows)", n);
            return TDT_E_NOMEM;
        }
        h->rows.cap = bytes;
    }
    W.lay(h->rows.d, n);
    TDT_HIP(hipMemcpyAsync(W.k1, k1, n * 8, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(W.sup, support, n * 4, hipMemcpyHostToDevice, st));
    rc = pile_genotype_launch(h, W.k1, W.sup, n, W.out);
    if (rc) return rc;
    TDT_HIP(hipMemcpyAsync(out8, W.out, n * 32, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    float ms = 0;
    TDT_HIP(hipEventElapsedTime(&ms, h->ev[4], h->ev[5]));
    h->ms[3] = ms;
    return TDT_OK;
}

// device milliseconds: [0] the tile sums, [1] the carry, [2] the scan and write of the last finish, [3] the last tdt_pile_genotype launch
extern "C" int tdt_pile_timing(tdt_pile *h, double *ms4) {
    if (!h || !ms4) {
        tdt_set_error("tdt_pile_timing: bad argument");
        return TDT_E_ARG;
    }
    for (int k = 0; k < 4; k++) ms4[k] = h->ms[k];
    return TDT_OK;
}
