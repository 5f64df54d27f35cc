// A store of (K1, K2) keys in HBM and its finish, written once for the consumers of the --sv scan that key events and count the sets of
// equal keys (tdt_indel.hip, tdt_snv.hip; each translation unit instantiates its own copy: everything here has internal linkage).
//   * the store: two uint64 columns of `cap` entries and a state line of KS_WORDS words — the consumer's push counters in front, the OR
//     of the keys and of their complements at or1 ... or1 + 3 (K1, ~K1, K2, ~K2), the number of keys stored at KS_N in a cache line of its
//     own, the overflow flag at KS_OVERFLOW.  The host knows only an upper bound of the keys stored: ks_reserve makes room BEFORE a launch,
//     and a growth first asks the device for the real count (dup_reserve's policy).
//   * ks_finish — once per job: the LSD sort of tdt_dup_finish (sort (K2, index); gather K1; sort (K1[perm], perm), stable; gather K2),
//     then the runs of equal (K1, K2 >> 1) in plain launches, none of whose workgroups waits for another: ks_tile_heads notes each
//     tile's last run head and last FULL-key head (a change of (K1, K2), bit 0 included), ks_carry (one workgroup) carries both across
//     the tiles, ks_runs<false> measures every run at its END — size = position - last head + 1; the sort puts bit 0 = 0 first, so REV =
//     position - last full-key head + 1 when the last member has bit 0 set, else 0 — and counts the runs it keeps per tile,
//     ks_carry_sum turns those counts into offsets, ks_runs<true> writes the kept runs as rows in key order.
#pragma once
#include "tdt_batch.h"
#include "tdt_bam_record.h"

namespace {

typedef unsigned long long ks_ull;

#define KS_BLOCK 256
#define KS_TILE 4096                          // keys of a run-length workgroup: KS_BLOCK lanes, KS_TILE / KS_BLOCK rounds
enum { KS_N = 16, KS_OVERFLOW, KS_WORDS = 32 };
static_assert(KS_TILE % KS_BLOCK == 0, "whole rounds");
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

// inclusive scan over the workgroup's 256 threads, in thread order (Op: tdt_max or tdt_sum; `none` its neutral element);
// *total = the reduction of all (s: KS_BLOCK / 64 words)
template <class Op> __device__ __forceinline__ int ks_block_scan(int v, int none, int *s, int t, int *total) {
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
    for (int w = 0; w < KS_BLOCK / 64; w++) {
        const int c = s[w];
        if (w < wave) v = Op::of(v, c);
        all = Op::of(all, c);
    }
    __syncthreads();
    *total = all;
    return v;
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

// ONE workgroup: tile_kept[k] = the kept runs of the tiles in front of tile k (an exclusive sum; the total is below 2^30)
__global__ __launch_bounds__(KS_BLOCK) void ks_carry_sum(int *__restrict__ tile_kept, int ntiles) {
    __shared__ int s[KS_BLOCK / 64];
    const int t = threadIdx.x;
    int running = 0;
    for (int c = 0; c < ntiles; c += KS_BLOCK) {                   // (uniform)
        const int k = c + t;
        const int mine = k < ntiles ? tile_kept[k] : 0;
        int all;
        const int v = ks_block_scan<tdt_sum>(mine, 0, s, t, &all);
        if (k < ntiles) tile_kept[k] = running + v - mine;
        running += all;
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

}  // namespace
