// A store of (K1, K2) keys in HBM, the push into it and its finish, written once for the consumers of the --sv scan that key events and
// count the sets of equal keys (tdt_indel.hip, tdt_snv.hip, tdt_clip.hip; each translation unit instantiates its own copy: everything here
// has internal linkage).
//   * the store: two uint64 columns of `cap` entries and a state line of KS_WORDS words — the consumer's push counters in front, the OR
//     of the keys and of their complements at or1 ... or1 + 3 (K1, ~K1, K2, ~K2), the number of keys stored at KS_N in a cache line of its
//     own, the overflow flag at KS_OVERFLOW.  The host knows only an upper bound of the keys stored: ks_reserve makes room BEFORE a launch,
//     and a growth first asks the device for the real count (dup_reserve's policy).
//   * the push — device side: the read gate (ks_read_gate), the record open (KS_OPEN) and the key emit (ks_stage, ks_flush), which write
//     the state line laid out here; host side: ks_launch round a consumer's launch, ks_push_device / ks_push for its two entries, and the
//     small entries of a handle (ks_finish_counted, ks_timing, ks_reserve_stats, ks_reset_checked, ks_destroy).
//   * ks_finish — once per job: the LSD sort of tdt_dup_finish (sort (K2, index); gather K1; sort (K1[perm], perm), stable; gather K2),
//     then the runs of equal (K1, K2 >> 1) in plain launches, none of whose workgroups waits for another: ks_tile_heads notes each
//     tile's last run head and last FULL-key head (a change of (K1, K2), bit 0 included), ks_carry (one workgroup) carries both across
//     the tiles, ks_runs<false> measures every run at its END — size = position - last head + 1; the sort puts bit 0 = 0 first, so REV =
//     position - last full-key head + 1 when the last member has bit 0 set, else 0 — and counts the runs it keeps per tile,
//     ks_carry_sum turns those counts into offsets, ks_runs<true> writes the kept runs as rows in key order.
#pragma once
#include "tdt_batch.h"
#include "tdt_bam_record.h"

#define KS_BLOCK 256
#define KS_TILE 4096                          // keys of a run-length workgroup: KS_BLOCK lanes, KS_TILE / KS_BLOCK rounds
#include "tdt_keyscan.h"                      // ks_block_scan, ks_carry_sum: in a header of their own, for launches that have no store

namespace {

enum { KS_N = 16, KS_OVERFLOW, KS_WORDS = 32 };
static_assert(KS_N * 8 % 128 == 0, "the store-slot atomic has a cache line of its own");

struct tdt_keystore {
    tdt_ctx *ctx;
    const char *name;                         // the consumer's prefix in error texts ("tdt_indel")
    int or1;                                  // where the OR / NAND words lie in the state line (four words, below KS_N)
    ks_ull *k1, *k2;                          // the store: cap entries each
    size_t cap, upper;                        // upper: no more than this many keys are stored (the device knows how many)
    ks_ull *d_state;                          // KS_WORDS
    void *d_work;                             // the finish's buffers (grows)
    size_t work_cap;
    ks_ull *r_k1, *r_k2;                      // the rows of the last finish (inside d_work), n_rows of them
    unsigned *r_sup, *r_rev;
    size_t n_rows;
    bool rows_valid;
    ks_ull asks, grows;                       // how often the reserve asked the device for the real count / made a bigger store
    hipEvent_t ev[5];
    double ms[4];
};

__global__ __launch_bounds__(KS_BLOCK) void ks_iota(unsigned *__restrict__ v, int n) {
    const int i = blockIdx.x * KS_BLOCK + threadIdx.x;
    if (i < n) v[i] = (unsigned)i;
}

__global__ __launch_bounds__(KS_BLOCK) void ks_gather(ks_ull *__restrict__ dst, const ks_ull *__restrict__ src, const unsigned *__restrict__ perm, int n) {
    const int i = blockIdx.x * KS_BLOCK + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

// ---- the push side: what every *_keys kernel does in front of and behind its own walk of a record
#define KS_MAX_CONTIGS (1 << 24)              // K1 = tid << 32 | P: a tid of 2^24 or more is malformed

struct ks_cols {                              // the kernel argument: the six columns of a batch a keyed consumer reads (device pointers)
    const uint16_t *flag;
    const int32_t *tid, *pos;
    const uint8_t *mapq;
    const uint64_t *rec_off;
    const uint8_t *raw;
};
#define KS_NEED (TDT_NEED(FLAG) | TDT_NEED(TID) | TDT_NEED(POS) | TDT_NEED(MAPQ) | TDT_NEED(REC_OFF) | TDT_NEED(RAW))
static inline ks_cols ks_cols_of(const tdt_batch &B) { return ks_cols{B.flag, B.tid, B.pos, B.mapq, B.rec_off, B.raw}; }

// THE READ GATE, lane = read: reads [first, first + BLOCK) below hi pass the filters on the coalesced columns (flag, tid, mapq), the
// two ballots ADD to records / eligible (wave-uniform), and the eligible reads are compacted into s_read in thread order.  Called by
// every thread; two barriers inside (tdt_block_slots' and the one behind the writes of s_read).  -> live: the eligible reads of the
// workgroup; thread t < live owns read `read`.  (The LDS of the gate, the stage and the flush is their own: BLOCK + 2 * BLOCK / 64
// ints, BLOCK / 64 * (NCNT + 4) + 1 words.)
struct ks_gated { int live, read; };
template <int BLOCK>
__device__ __forceinline__ ks_gated ks_read_gate(const ks_cols &I, long long first, long long hi, unsigned min_mapq, ks_ull &records, ks_ull &eligible) {
    __shared__ int s_read[BLOCK], s_wsum[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long i = first + t;
    bool elig = false;
    if (i < hi) elig = (I.flag[i] & 0xF04u) == 0 && I.tid[i] >= 0 && (unsigned)I.mapq[i] >= min_mapq;
    const ks_ull m_rec = __ballot(i < hi), m_el = __ballot(elig);
    records += (ks_ull)__popcll(m_rec);
    eligible += (ks_ull)__popcll(m_el);
    const tdt_slots S = tdt_block_slots<BLOCK / 64>(m_el, s_wsum, lane, wave);
    if (elig) s_read[S.base + tdt_lane_rank(m_el, lane)] = (int)i;
    __syncthreads();
    return ks_gated{S.total, t < S.total ? s_read[t] : 0};
}

// THE RECORD OPEN behind the gate, for a live lane: rev, tid and pos from the columns, then the record bounded with TDT_REC_*.  true:
// tid < 2^24, pos >= 0, the header inside raw, l_seq >= 0 and the body fits — A.R is the record.  false: malformed, A.R is not to be
// used.  A MACRO for the reason written above TDT_REC_*: as a __forceinline__ function its `&&` reaches the caller as selects, and
// indel_keys<false> was 2 % slower on the one batch of the bench file where it is slowest (profiles/keyed_emit_240mb.md).
struct ks_read {
    tdt_rec R;
    int tid, pos;
    unsigned rev;
};
#define KS_OPEN(A, I, ri, raw_len)                                                                                                       \
    ((A).rev = ((unsigned)(I).flag[ri] >> 4) & 1u, (A).tid = (I).tid[ri], (A).pos = (I).pos[ri], (A).R.ro = (I).rec_off[ri],              \
     (A).tid < KS_MAX_CONTIGS && (A).pos >= 0 && TDT_REC_HEADER_INSIDE(raw_len, (A).R.ro) &&                                             \
         ((A).R = TDT_REC_READ((I).raw, (A).R.ro), (A).R.l_seq >= 0 && TDT_REC_FITS((A).R, raw_len)))

// THE KEY EMIT of a workgroup of BLOCK threads with NCNT push counters, which lie in front of the state line with the OR / NAND words
// behind them (tdt_keystore::or1 == NCNT).  The consumer keeps what is its own: which counters are ballots and which lane sums, and
// how a key is built.  It stages its keys in LDS of its own (s_k1 / s_k2) at the slots ks_stage hands out, ORs them into a ks_masks, and ends
// with ks_flush.
struct ks_masks {                                                  // the OR of this lane's keys and of their complements (the sort masks)
    ks_ull or1 = 0, nand1 = 0, or2 = 0, nand2 = 0;
    __device__ __forceinline__ void add(ks_ull k1, ks_ull k2) { or1 |= k1, nand1 |= ~k1, or2 |= k2, nand2 |= ~k2; }
};

// STAGE: each lane's key count `mine` -> its first slot among the workgroup's keys of this call, in thread order; *total = all of
// them (uniform).  Called by every thread; ONE barrier inside.
template <int BLOCK> __device__ __forceinline__ int ks_stage(int mine, int *total) {
    __shared__ int s_wkeys[BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) s_wkeys[wave] = incl;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) {
        base += w < wave ? s_wkeys[w] : 0;
        all += s_wkeys[w];
    }
    *total = all;
    return base + incl - mine;
}

// FLUSH: cnt[] = this wave's push counters (wave-uniform: the consumer reduced its lane sums), M = this lane's masks, nk = the staged
// keys (uniform over the workgroup).  The masks are merged over the wave, the waves' rows over the workgroup: ONE atomic per workgroup
// and non-zero word (add for a counter, OR for a mask), ONE atomicAdd on KS_N for the workgroup's slots of the store, then the append —
// every slot is tested against the capacity, and a slot beyond it raises KS_OVERFLOW instead of being written (cannot happen: the
// host reserved the per-read cap for every read of the batch).  Called by every thread; two barriers inside.
template <int BLOCK, int NCNT>
__device__ __forceinline__ void ks_flush(const ks_ull (&cnt)[NCNT], ks_masks M, int nk, const ks_ull *s_k1, const ks_ull *s_k2, ks_ull *__restrict__ k1s,
                                         ks_ull *__restrict__ k2s, ks_ull cap, ks_ull *__restrict__ st) {
    static_assert(NCNT + 4 <= KS_N && NCNT + 4 <= BLOCK, "state layout");
    __shared__ ks_ull s_cnt[BLOCK / 64][NCNT + 4];                  // per wave: the push counters, then the OR / NAND words
    __shared__ ks_ull s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    M.or1 = tdt_wave_reduce<tdt_or>(M.or1), M.nand1 = tdt_wave_reduce<tdt_or>(M.nand1);
    M.or2 = tdt_wave_reduce<tdt_or>(M.or2), M.nand2 = tdt_wave_reduce<tdt_or>(M.nand2);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NCNT; k++) s_cnt[wave][k] = cnt[k];
        s_cnt[wave][NCNT] = M.or1, s_cnt[wave][NCNT + 1] = M.nand1, s_cnt[wave][NCNT + 2] = M.or2, s_cnt[wave][NCNT + 3] = M.nand2;
    }
    __syncthreads();
    if (t == 0) s_base = nk ? atomicAdd(&st[KS_N], (ks_ull)nk) : 0ull;
    if (t < NCNT + 4) {
        ks_ull v = 0;
        for (int w = 0; w < BLOCK / 64; w++) v = t < NCNT ? v + s_cnt[w][t] : v | s_cnt[w][t];
        if (v) {
            if (t < NCNT) atomicAdd(&st[t], v);
            else atomicOr(&st[t], v);
        }
    }
    __syncthreads();
    for (int k = t; k < nk; k += BLOCK) {                          // (consecutive lanes, consecutive slots)
        const ks_ull at = s_base + (ks_ull)k;
        if (at < cap) {
            k1s[at] = s_k1[k];
            k2s[at] = s_k2[k];
        } else {
            st[KS_OVERFLOW] = 1;
        }
    }
}

// NX further counters of a consumer at st[at ...] (below KS_N), per wave in s_x: written before ks_flush and added behind it, so its
// barriers stand between.  One atomic per non-zero word, from a wave the push counters' atomics leave idle.
template <int BLOCK, int NX> __device__ __forceinline__ void ks_flush_extra(const ks_ull (&s_x)[BLOCK / 64][NX], ks_ull *__restrict__ st, int at) {
    static_assert(BLOCK >= 128 && NX <= 64, "the second wave");
    const int t = threadIdx.x;
    if (t >= 64 && t < 64 + NX) {
        ks_ull v = 0;
        for (int w = 0; w < BLOCK / 64; w++) v += s_x[w][t - 64];
        if (v) atomicAdd(&st[at + (t - 64)], v);
    }
}

// a run head: the first key, or a key whose (K1, K2 >> 1) differs from the one in front of it; a full head: (K1, K2) differs
__device__ __forceinline__ bool ks_head(const ks_ull *__restrict__ a, const ks_ull *__restrict__ b, int i) {
    return i == 0 || a[i] != a[i - 1] || (b[i] >> 1) != (b[i - 1] >> 1);
}
__device__ __forceinline__ bool ks_full_head(const ks_ull *__restrict__ a, const ks_ull *__restrict__ b, int i) {
    return i == 0 || a[i] != a[i - 1] || b[i] != b[i - 1];
}

// tile_last[tile] = the position of the tile's last run head, tile_last[ntiles + tile] = of its last full head; -1 when it has none
__global__ __launch_bounds__(KS_BLOCK) void ks_tile_heads(const ks_ull *__restrict__ a, const ks_ull *__restrict__ b, int n, int ntiles,
                                                          int *__restrict__ tile_last) {
    __shared__ int s[KS_BLOCK / 64];
    const int t = threadIdx.x;
    const int t0 = blockIdx.x * KS_TILE;
    int best = -1, bestf = -1;
    for (int r = 0; r < KS_TILE / KS_BLOCK; r++) {
        const int i = t0 + r * KS_BLOCK + t;
        if (i < n) {
            if (ks_head(a, b, i)) best = i;                        // (i grows with r)
            if (ks_full_head(a, b, i)) bestf = i;
        }
    }
    int all, allf;
    (void)ks_block_scan<tdt_max>(best, -1, s, t, &all);
    (void)ks_block_scan<tdt_max>(bestf, -1, s, t, &allf);
    if (t == 0) tile_last[blockIdx.x] = all, tile_last[ntiles + blockIdx.x] = allf;
}

// ONE workgroup: both halves of tile_last become running maxima over the tiles
__global__ __launch_bounds__(KS_BLOCK) void ks_carry(int *__restrict__ tile_last, int ntiles) {
    __shared__ int s[KS_BLOCK / 64];
    const int t = threadIdx.x;
    for (int half = 0; half < 2; half++) {
        int *v_ = tile_last + (size_t)half * ntiles;
        int running = -1;
        for (int c = 0; c < ntiles; c += KS_BLOCK) {               // (uniform)
            const int k = c + t;
            int all;
            int v = ks_block_scan<tdt_max>(k < ntiles ? v_[k] : -1, -1, s, t, &all);
            v = v > running ? v : running;
            if (k < ntiles) v_[k] = v;
            running = all > running ? all : running;
        }
    }
}

// every run measured at its end.  WRITE false: tile_kept[tile] = the runs of the tile with size >= min_support, out[0] += its runs,
// out[1] += the kept ones.  WRITE true: tile_kept holds the exclusive sums and the kept runs become rows, in key order.
template <bool WRITE>
__global__ __launch_bounds__(KS_BLOCK) void ks_runs(const ks_ull *__restrict__ a, const ks_ull *__restrict__ b, int n, int ntiles,
                                                    const int *__restrict__ tile_last, int *__restrict__ tile_kept, unsigned min_support,
                                                    ks_ull *__restrict__ out, ks_ull *__restrict__ r_k1, ks_ull *__restrict__ r_k2,
                                                    unsigned *__restrict__ r_sup, unsigned *__restrict__ r_rev) {
    __shared__ int s[KS_BLOCK / 64];
    __shared__ int s_w[KS_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int t0 = blockIdx.x * KS_TILE;
    int running = blockIdx.x ? tile_last[blockIdx.x - 1] : -1, runningf = blockIdx.x ? tile_last[ntiles + blockIdx.x - 1] : -1;
    int kept = 0, runs = 0;                                        // (uniform over the workgroup)
    const int row0 = WRITE ? tile_kept[blockIdx.x] : 0;
    for (int r = 0; r < KS_TILE / KS_BLOCK; r++) {                 // (uniform: every thread takes every round)
        const int i = t0 + r * KS_BLOCK + t;
        const bool valid = i < n;
        ks_ull ka = 0, kb = 0;
        bool head = false, fhead = false, end = false;
        if (valid) {
            ka = a[i];
            kb = b[i];
            head = ks_head(a, b, i);
            fhead = ks_full_head(a, b, i);
            end = i == n - 1 || a[i + 1] != ka || (b[i + 1] >> 1) != (kb >> 1);
        }
        int all, allf;
        int last = ks_block_scan<tdt_max>(head ? i : -1, -1, s, t, &all);
        int lastf = ks_block_scan<tdt_max>(fhead ? i : -1, -1, s, t, &allf);
        last = last > running ? last : running;
        lastf = lastf > runningf ? lastf : runningf;
        running = all > running ? all : running;
        runningf = allf > runningf ? allf : runningf;
        const unsigned size = end ? (unsigned)(i - last + 1) : 0u;
        const bool keep = end && size >= min_support;
        const ks_ull m_keep = __ballot(keep), m_end = __ballot(end);
        const tdt_slots S = tdt_block_slots<KS_BLOCK / 64>(m_keep, s_w, lane, wave);
        if (WRITE && keep) {
            const size_t row = (size_t)row0 + (size_t)(kept + S.base + tdt_lane_rank(m_keep, lane));       // (< n: a row per run)
            r_k1[row] = ka;
            r_k2[row] = kb & ~1ull;
            r_sup[row] = size;
            r_rev[row] = (kb & 1ull) ? (unsigned)(i - lastf + 1) : 0u;
        }
        kept += S.total;
        if (!WRITE) {
            const tdt_slots E = tdt_block_slots<KS_BLOCK / 64>(m_end, s, lane, wave);
            runs += E.total;
            __syncthreads();                                       // (s is the next round's scan buffer)
        }
    }
    if (!WRITE && t == 0) {
        tile_kept[blockIdx.x] = kept;
        if (runs) atomicAdd(&out[0], (ks_ull)runs);
        if (kept) atomicAdd(&out[1], (ks_ull)kept);
    }
}

// everything the store owns (the struct itself is the consumer's)
void ks_free(tdt_keystore *h) {
    if (h->k1) (void)hipFree(h->k1);
    if (h->k2) (void)hipFree(h->k2);
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->d_work) (void)hipFree(h->d_work);
    for (int k = 0; k < 5; k++)
        if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
    h->k1 = h->k2 = h->d_state = nullptr;
    h->d_work = nullptr;
    for (int k = 0; k < 5; k++) h->ev[k] = nullptr;
}

// two device arrays of `cap` store entries; on failure nothing is left allocated
hipError_t ks_alloc_store(size_t cap, ks_ull **k1, ks_ull **k2) {
    *k1 = *k2 = nullptr;
    if (tdt_dev_malloc((void **)k1, cap * 8) == hipSuccess && tdt_dev_malloc((void **)k2, cap * 8) == hipSuccess) return hipSuccess;
    if (*k1) (void)hipFree(*k1);
    if (*k2) (void)hipFree(*k2);
    *k1 = *k2 = nullptr;
    return hipErrorOutOfMemory;
}

// a zeroed struct becomes a store of `capacity` keys; on failure the caller calls ks_free.  (the device is set)
int ks_init(tdt_keystore *h, tdt_ctx *ctx, const char *name, int or1, size_t capacity) {
    h->ctx = ctx;
    h->name = name;
    h->or1 = or1;
    if (tdt_dev_malloc((void **)&h->d_state, KS_WORDS * 8) != hipSuccess || (capacity && ks_alloc_store(capacity, &h->k1, &h->k2) != hipSuccess)) {
        tdt_set_error("%s_create: out of device memory (%zu keys)", name, capacity);
        return TDT_E_NOMEM;
    }
    h->cap = capacity;
    hipError_t e = hipMemsetAsync(h->d_state, 0, KS_WORDS * 8, ctx->stream);
    for (int k = 0; k < 5 && e == hipSuccess; k++) e = hipEventCreate(&h->ev[k]);
    TDT_HIP(e);
    return TDT_OK;
}

int ks_reset(tdt_keystore *h) {
    TDT_HIP(hipSetDevice(h->ctx->device));
    TDT_HIP(hipMemsetAsync(h->d_state, 0, KS_WORDS * 8, h->ctx->stream));
    h->upper = 0;
    h->n_rows = 0;
    h->rows_valid = false;
    return TDT_OK;
}

// how many keys the store holds (the stream is synchronised)
int ks_stored(tdt_keystore *h, ks_ull *state) {
    hipStream_t st = h->ctx->stream;
    TDT_HIP(hipMemcpyAsync(state, h->d_state, KS_WORDS * 8, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    if (state[KS_OVERFLOW] || state[KS_N] > h->cap) {
        tdt_set_error("%s: the key store overflowed (%llu keys, capacity %zu)", h->name, state[KS_N], h->cap);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

// room for `more` keys behind the (at most) h->upper stored ones, as dup_reserve makes it: a growth first asks the device how many
// keys there really are; then a bigger store (1.5 x), the keys so far copied over on the device, the old one freed once the copy is done.
int ks_reserve(tdt_keystore *h, size_t more) {
    if (h->upper + more <= h->cap) return TDT_OK;
    ks_ull state[KS_WORDS];
    int rc = ks_stored(h, state);
    if (rc) return rc;
    h->asks++;
    h->upper = (size_t)state[KS_N];
    if (h->upper + more <= h->cap) return TDT_OK;
    size_t want = h->cap + h->cap / 2;
    if (want < h->upper + more) want = h->upper + more;
    ks_ull *k1, *k2;
    if (ks_alloc_store(want, &k1, &k2) != hipSuccess) {
        tdt_set_error("%s: out of device memory growing to %zu keys", h->name, want);
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

// The store read out, in the order it lies in HBM.  On entry *n = the room of the two arrays (ignored when both are NULL: the call then
// only reports the count); on return *n = the keys stored.  Too little room: TDT_E_RANGE, nothing written.  (h may be NULL: refused)
int ks_keys(tdt_keystore *h, const char *name, uint64_t *k1, uint64_t *k2, size_t *n) {
    if (!h || !n || ((k1 || k2) && !(k1 && k2))) {
        tdt_set_error("%s_keys: bad argument", name);
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    ks_ull state[KS_WORDS];
    int rc = ks_stored(h, state);
    if (rc) return rc;
    const size_t have = (size_t)state[KS_N];
    if (k1) {
        if (*n < have) {
            tdt_set_error("%s_keys: room for %zu keys, %zu stored", name, *n, have);
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

struct ks_work {
    ks_ull *ka, *kb, *d_out, *r_k1, *r_k2;
    unsigned *ia, *ib, *r_sup, *r_rev;
    int *tile_last, *tile_kept;
    size_t lay(void *base, size_t n, size_t ntiles) {
        tdt_carver cv(base);
        ka = cv.take<ks_ull>(n), kb = cv.take<ks_ull>(n), ia = cv.take<unsigned>(n), ib = cv.take<unsigned>(n);
        r_k1 = cv.take<ks_ull>(n), r_k2 = cv.take<ks_ull>(n), r_sup = cv.take<unsigned>(n), r_rev = cv.take<unsigned>(n);
        tile_last = cv.take<int>(2 * ntiles), tile_kept = cv.take<int>(ntiles), d_out = cv.take<ks_ull>(2);
        return cv.size;
    }
};

// the sort mask of a key column: every bit from the lowest to the highest one that differs between two stored keys (one run of set
// bits: at most eight digits, whatever a hashed payload looks like)
ks_ull ks_mask(ks_ull differ) {
    if (!differ) return 0;
    const int lo = __builtin_ctzll(differ), hi = 63 - __builtin_clzll(differ);
    return (hi == 63 ? ~0ull : (1ull << (hi + 1)) - 1ull) & ~((1ull << lo) - 1ull);
}

// The sets of everything pushed so far: state[KS_WORDS] = the state line as ks_stored read it (the caller refused what it refuses
// and set the device); got[0] = the sets, got[1] = those with min_support members or more, which tdt_*_rows will give.  The store is
// left as it was.
int ks_finish(tdt_keystore *h, const ks_ull *state, uint64_t min_support, ks_ull *got) {
    tdt_ctx *ctx = h->ctx;
    const size_t n_ = (size_t)state[KS_N];
    if (n_ >= (1ull << 30)) {
        tdt_set_error("%s_finish: %zu keys; the sort handles fewer than 2^30", h->name, n_);
        return TDT_E_RANGE;
    }
    got[0] = got[1] = 0;
    for (int k = 0; k < 4; k++) h->ms[k] = 0;
    h->rows_valid = false;
    h->n_rows = 0;
    if (n_) {
        const int n = (int)n_;
        const size_t ntiles = (n_ + KS_TILE - 1) / KS_TILE;
        ks_work W;
        const size_t bytes = W.lay(nullptr, n_, ntiles);
        if (bytes > h->work_cap) {
            if (h->d_work) TDT_HIP(hipFree(h->d_work));
            h->d_work = nullptr;
            h->work_cap = 0;
            if (tdt_dev_malloc(&h->d_work, bytes) != hipSuccess) {
                tdt_set_error("%s_finish: out of device memory (%zu keys)", h->name, n_);
                return TDT_E_NOMEM;
            }
            h->work_cap = bytes;
        }
        W.lay(h->d_work, n_, ntiles);
        hipStream_t st = ctx->stream;
        const unsigned grid = (unsigned)((n_ + KS_BLOCK - 1) / KS_BLOCK);
        TDT_HIP(hipMemsetAsync(W.d_out, 0, 2 * 8, st));
        TDT_HIP(hipMemcpyAsync(W.ka, h->k2, n_ * 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(ks_iota, dim3(grid), dim3(KS_BLOCK), 0, st, W.ia, n);
        TDT_CHECK_LAUNCH();
        // PRECONDITION of tdt_radix_sort_pairs: the key bits outside the mask are equal in ALL keys.  The push kept the OR of the keys
        // and of their complements: a bit differs exactly when it is set in both, and ks_mask covers every such bit.
        const ks_ull mask1 = ks_mask(state[h->or1] & state[h->or1 + 1]), mask2 = ks_mask(state[h->or1 + 2] & state[h->or1 + 3]);
        ks_ull *k2s, *k1s;
        unsigned *perm, *perm2;
        TDT_HIP(hipEventRecord(h->ev[0], st));
        int rc = tdt_radix_sort_pairs(ctx, W.ka, W.ia, W.kb, W.ib, n_, mask2, &k2s, &perm);
        if (rc) return rc;
        TDT_HIP(hipEventRecord(h->ev[1], st));
        ks_ull *free_k = k2s == W.ka ? W.kb : W.ka;                // (the sorted K2 are not needed again: K2 comes from the store below)
        unsigned *free_i = perm == W.ia ? W.ib : W.ia;
        hipLaunchKernelGGL(ks_gather, dim3(grid), dim3(KS_BLOCK), 0, st, free_k, (const ks_ull *)h->k1, (const unsigned *)perm, n);
        TDT_CHECK_LAUNCH();
        TDT_HIP(hipEventRecord(h->ev[2], st));
        rc = tdt_radix_sort_pairs(ctx, free_k, perm, k2s, free_i, n_, mask1, &k1s, &perm2);            // (the same precondition, mask1)
        if (rc) return rc;
        TDT_HIP(hipEventRecord(h->ev[3], st));
        ks_ull *k2f = k1s == W.ka ? W.kb : W.ka;
        const int nt = (int)ntiles;
        hipLaunchKernelGGL(ks_gather, dim3(grid), dim3(KS_BLOCK), 0, st, k2f, (const ks_ull *)h->k2, (const unsigned *)perm2, n);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(ks_tile_heads, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, (const ks_ull *)k1s, (const ks_ull *)k2f, n, nt, W.tile_last);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(ks_carry, dim3(1), dim3(KS_BLOCK), 0, st, W.tile_last, nt);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(ks_runs<false>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, (const ks_ull *)k1s, (const ks_ull *)k2f, n, nt,
                           (const int *)W.tile_last, W.tile_kept, (unsigned)min_support, W.d_out, W.r_k1, W.r_k2, W.r_sup, W.r_rev);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(ks_carry_sum, dim3(1), dim3(KS_BLOCK), 0, st, W.tile_kept, nt);
        TDT_CHECK_LAUNCH();
        hipLaunchKernelGGL(ks_runs<true>, dim3((unsigned)ntiles), dim3(KS_BLOCK), 0, st, (const ks_ull *)k1s, (const ks_ull *)k2f, n, nt,
                           (const int *)W.tile_last, W.tile_kept, (unsigned)min_support, W.d_out, W.r_k1, W.r_k2, W.r_sup, W.r_rev);
        TDT_CHECK_LAUNCH();
        TDT_HIP(hipEventRecord(h->ev[4], st));
        TDT_HIP(hipMemcpyAsync(got, W.d_out, 2 * 8, hipMemcpyDeviceToHost, st));
        rc = tdt_ctx_sync(ctx);                                    // (also reports the sort's bounded-spin word)
        if (rc) return rc;
        for (int k = 0; k < 4; k++) {
            float ms = 0;
            TDT_HIP(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
            h->ms[k] = ms;
        }
        h->r_k1 = W.r_k1, h->r_k2 = W.r_k2, h->r_sup = W.r_sup, h->r_rev = W.r_rev;
        h->n_rows = (size_t)got[1];
    }
    h->rows_valid = true;
    return TDT_OK;
}

// The rows of the last finish, ascending by (K1, K2 >> 1): K1, K2 with bit 0 clear, SUPPORT, REV.  *n in: the room of the four arrays
// (ignored when all four are NULL), out: the rows.  A push or a reset since the finish: TDT_E_ARG.  Too little room: TDT_E_RANGE.
int ks_rows(tdt_keystore *h, const char *name, uint64_t *k1, uint64_t *k2, uint32_t *support, uint32_t *rev, size_t *n) {
    const bool any = k1 || k2 || support || rev;
    if (!h || !n || (any && !(k1 && k2 && support && rev))) {
        tdt_set_error("%s_rows: bad argument", name);
        return TDT_E_ARG;
    }
    if (!h->rows_valid) {
        tdt_set_error("%s_rows: no finish since the last push or reset", name);
        return TDT_E_ARG;
    }
    const size_t have = h->n_rows;
    if (any) {
        if (*n < have) {
            tdt_set_error("%s_rows: room for %zu rows, %zu kept", name, *n, have);
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

// ---- the push path and the small entries of a consumer's handle H: H has `ctx`, the store `S` and the host entry's block `io`.  A
// handle may be NULL wherever the C entry refuses one; `name` is the consumer's prefix ("tdt_indel"), `fn` a whole entry name.

// around a consumer's launch: room for the `room` keys the batch can give at most is reserved BEFORE it; behind it the bound grows
// and the rows of an earlier finish are gone.  launch(): enqueues the kernel (it reads S->k1, S->k2, S->cap only now)
template <class Launch> int ks_launch(tdt_keystore *S, size_t room, Launch launch) {
    const int rc = ks_reserve(S, room);
    if (rc) return rc;
    launch();
    TDT_CHECK_LAUNCH();
    S->upper += room;
    S->rows_valid = false;
    return TDT_OK;
}

// One batch of the device ingest: table = the pointer table tdt_ingest_arrays filled (TDT_COL_*: a host array of TDT_NCOL device
// pointers).  launch(I) is the consumer's ks_launch on the columns I; it is enqueued on the context's stream and nothing is waited
// for — unless the reserve must ask or grow.
template <class H, class Launch> int ks_push_device(const char *fn, H *h, const void *const *table, size_t n, size_t raw_len, Launch launch) {
    tdt_batch B;
    const int rc = tdt_batch_view(fn, h, table, n, raw_len, KS_NEED, &B);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    return launch(ks_cols_of(B));
}

// The same kernel on host columns and host record bytes (C: the caller's HOST pointers), uploaded into the handle's own block.  The
// stream is synchronised before the return: the caller's arrays are free again.
template <class H, class Launch> int ks_push(const char *fn, H *h, const ks_cols &C, size_t n, size_t raw_len, Launch launch) {
    tdt_batch host{}, B;
    host.flag = C.flag, host.tid = C.tid, host.pos = C.pos, host.mapq = C.mapq, host.rec_off = C.rec_off, host.raw = C.raw;
    int rc = tdt_batch_host(fn, h, host, n, raw_len, KS_NEED);
    if (rc == TDT_OK) rc = tdt_batch_offsets_ascend(fn, C.rec_off, n);
    if (rc) return rc;
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    rc = tdt_batch_upload(fn, h->ctx, &h->io, host, KS_NEED, n, raw_len, &B);
    if (rc == TDT_OK) rc = launch(ks_cols_of(B));
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

// what every create checks behind its arguments (the error text is the consumer's: its own parameters stand in the middle of it)
bool ks_create_in_range(int n_contigs, int min_mapq, size_t capacity) {
    return n_contigs <= KS_MAX_CONTIGS && min_mapq >= 0 && min_mapq <= 255 && capacity < (1ull << 40);
}

// The front of every finish: ok = the entry's pointer arguments are there; min_support in 1 ... max_support; then the state line and
// ks_finish with `run_support`.  res[0, push_n) = the push counters (the SN rows' first), got = what ks_finish counted.
int ks_finish_counted(tdt_keystore *S, const char *name, bool ok, uint64_t min_support, int max_support, uint64_t run_support, int push_n, uint64_t *res,
                      ks_ull *got) {
    if (!ok) {
        tdt_set_error("%s_finish: bad argument", name);
        return TDT_E_ARG;
    }
    if (min_support < 1 || min_support > (uint64_t)max_support) {
        tdt_set_error("%s_finish: min_support %llu (1 ... %d)", name, (ks_ull)min_support, max_support);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(S->ctx->device));
    ks_ull state[KS_WORDS];
    int rc = ks_stored(S, state);
    if (rc == TDT_OK) rc = ks_finish(S, state, run_support, got);
    if (rc) return rc;
    for (int k = 0; k < push_n; k++) res[k] = state[k];
    return TDT_OK;
}

int ks_reset_checked(tdt_keystore *S, const char *name) {
    if (S) return ks_reset(S);
    tdt_set_error("%s_reset: bad argument", name);
    return TDT_E_ARG;
}

// device milliseconds of the last finish: [0] sort by K2, [1] gather of K1, [2] sort by K1, [3] gather of K2 + the run-length launches
int ks_timing(const tdt_keystore *S, const char *name, double *ms4) {
    if (!S || !ms4) {
        tdt_set_error("%s_timing: bad argument", name);
        return TDT_E_ARG;
    }
    for (int k = 0; k < 4; k++) ms4[k] = S->ms[k];
    return TDT_OK;
}

// out3: how often the reserve asked the device for the real count, how often it made a bigger store, the store's capacity now
int ks_reserve_stats(const tdt_keystore *S, const char *name, uint64_t *out3) {
    if (!S || !out3) {
        tdt_set_error("%s_reserve_stats: bad argument", name);
        return TDT_E_ARG;
    }
    out3[0] = S->asks, out3[1] = S->grows, out3[2] = S->cap;
    return TDT_OK;
}

// the stream is drained (no kernel of it still writes the store), then free_(h) frees the store, the block and the handle
template <class H> int ks_destroy(H *h, void (*free_)(H *)) {
    if (!h) return TDT_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    free_(h);
    return TDT_OK;
}

}  // namespace
