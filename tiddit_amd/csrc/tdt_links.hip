// Link counts per SV site for gfx950 — how many discordant-pair and split-read signals of this sample join the two regions of a
// site that was called elsewhere (TIDDIT_GENOTYPE): DV / RV of the genotyped record.
// The signals are the rows of the cluster table (tdt_sigtab_cluster_table: per (chrA, chrB) bucket the written discordant
// fragments, then the split fragments, posA / posB as tiddit_cluster.pyx:47-105 picks them).  A handle keeps them in HBM as ONE
// 8-byte record per signal, {posA, posB | kind << 30}, every bucket sorted by posA.  ONE WAVE answers one site:
//   * the rows with startA <= posA <= endA are [lo, hi) of the bucket: two 64-ary lower bounds in lock step (tdt_search.h);
//   * lane = row, 64 rows per step, one coalesced 8-byte load each; startB <= posB <= endB is tested per row and the row is
//     counted under its kind (0 pair, 1 split; 2, an assembly contig, under neither);
//   * the two per-lane counters are reduced over the wave and lane 0 writes them.
// Both outputs are order-independent integer sums: the result equals the double loop over the table exactly.
#include "tdt_common.h"
#include "tdt_search.h"

typedef unsigned long long ull;

#define LK_POS_BITS 30
#define LK_POS_MASK ((1 << LK_POS_BITS) - 1)

struct tdt_links {
    tdt_ctx *ctx;
    int nb;
    size_t n;
    int2 *rec;                 // n records, bucket-major, every bucket ascending in posA
    long long *d_off;          // nb + 1 bucket offsets
    int *d_bad;
    void *d_io;                // sites + counts of the host entry (grows)
    size_t io_cap;
};

// key = bucket << 32 | (posA - amin), value = signal index; the bucket by binary search over the offsets (empty buckets are skipped:
// the last b with off[b] <= i)
__global__ __launch_bounds__(256) void lk_make_keys(const int32_t *__restrict__ posA, int n, const long long *__restrict__ off, int nb,
                                                    long long amin, ull *__restrict__ keys, unsigned *__restrict__ vals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = nb;       // off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    keys[i] = ((ull)(unsigned)lo << 32) | (ull)(unsigned)((long long)posA[i] - amin);
    vals[i] = (unsigned)i;
}

__global__ __launch_bounds__(256) void lk_pack(const ull *__restrict__ keys, const unsigned *__restrict__ vals, const int32_t *__restrict__ posB,
                                               const uint8_t *__restrict__ kind, int n, long long amin, int2 *__restrict__ rec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned v = vals[i];
    const int a = (int)((long long)(unsigned)(keys[i] & 0xffffffffull) + amin);
    rec[i] = make_int2(a, (int)((unsigned)posB[v] | ((unsigned)kind[v] << LK_POS_BITS)));
}

// One wave per site; sites = int32[ns][6] {bucket, startA, endA, startB, endB, 0}, out = int64[ns][2] {pairs, splits}.
// CHECK (the device-site entry, whose sites the host never sees): a site naming no bucket, or with start > end, writes zeros and
// leaves the lowest such site index in *bad; the wave's branch is uniform (one site per wave).
template <bool CHECK>
__global__ __launch_bounds__(256) void links_count(const int2 *__restrict__ rec, const long long *__restrict__ off, int nb,
                                                   const int32_t *__restrict__ sites, int ns, long long *__restrict__ out,
                                                   int *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= ns) return;
    const int2 *S = reinterpret_cast<const int2 *>(sites) + 3 * (size_t)q;        // (24 bytes per site: three 8-byte loads)
    const int2 s0 = S[0], s1 = S[1], s2 = S[2];
    const int bucket = s0.x, startA = s0.y, endA = s1.x, startB = s1.y, endB = s2.x;
    const bool wrong = CHECK && (bucket < -1 || bucket >= nb || startA > endA || startB > endB);
    if (wrong || bucket == -1) {                                                  // -1: no signal joins these two contigs
        if (lane < 2) out[(size_t)q * 2 + lane] = 0;
        if (wrong && lane == 0) atomicMin(bad, q);
        return;
    }
    const long long o = off[bucket];
    const int n = (int)(off[bucket + 1] - o);
    const int2 *__restrict__ R = rec + o;
    int lo, hi;                // posA >= startA  <=>  i >= lo;   posA <= endA  <=>  i < hi
    rg_lower_bound2<2>(reinterpret_cast<const int32_t *>(R), n, (long long)startA, (long long)endA + 1, lane, lo, hi);
    unsigned dv = 0, rv = 0;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const bool in = i0 + lane < hi;
        const int2 r = R[in ? i0 + lane : lo];
        const int pb = r.y & LK_POS_MASK;
        const unsigned k = (unsigned)r.y >> LK_POS_BITS;
        const bool hit = in && pb >= startB && pb <= endB;
        dv += (hit && k == 0u) ? 1u : 0u;
        rv += (hit && k == 1u) ? 1u : 0u;
    }
    for (int d = 32; d > 0; d >>= 1) {
        dv += __shfl_xor(dv, d);
        rv += __shfl_xor(rv, d);
    }
    if (lane == 0) {
        out[(size_t)q * 2] = dv;
        out[(size_t)q * 2 + 1] = rv;
    }
}

static void lk_free(tdt_links *h) {
    if (h->rec) (void)hipFree(h->rec);
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_bad) (void)hipFree(h->d_bad);
    if (h->d_io) (void)hipFree(h->d_io);
    delete h;
}

extern "C" int tdt_links_create(tdt_ctx *ctx, const int32_t *posA, const int32_t *posB, const uint8_t *kind, const int64_t *bucket_off, int nb,
                                tdt_links **out) {
    if (!ctx || !out || nb < 0 || !bucket_off || bucket_off[0] != 0) {
        tdt_set_error("tdt_links_create: bad argument");
        return TDT_E_ARG;
    }
    for (int b = 0; b < nb; b++) {
        if (bucket_off[b + 1] < bucket_off[b]) {
            tdt_set_error("tdt_links_create: bucket offsets must not decrease (bucket %d)", b);
            return TDT_E_ARG;
        }
    }
    const int64_t n64 = bucket_off[nb];
    if (n64 >= (1ll << 30)) {
        tdt_set_error("tdt_links_create: %lld signals; the handle keeps fewer than 2^30", (long long)n64);
        return TDT_E_RANGE;
    }
    const size_t n = (size_t)n64;
    if (n && (!posA || !posB || !kind)) {
        tdt_set_error("tdt_links_create: bad argument");
        return TDT_E_ARG;
    }
    long long amin = 0, amax = 0;
    for (size_t i = 0; i < n; i++) {
        if (posB[i] < 0 || posB[i] > LK_POS_MASK || kind[i] > 2) {
            tdt_set_error("tdt_links_create: signal %zu (posB %d, kind %d) outside the record's domain (0 <= posB < 2^30, kind 0..2)", i,
                          posB[i], (int)kind[i]);
            return TDT_E_UNSUPPORTED;
        }
        if (!i || posA[i] < amin) amin = posA[i];
        if (!i || posA[i] > amax) amax = posA[i];
    }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_links *h = new tdt_links{ctx, nb, n, nullptr, nullptr, nullptr, nullptr, 0};
    const size_t N = n ? n : 1;
    if (tdt_dev_malloc((void **)&h->rec, N * sizeof(int2)) != hipSuccess ||
        tdt_dev_malloc((void **)&h->d_off, (size_t)(nb + 1) * 8) != hipSuccess || tdt_dev_malloc((void **)&h->d_bad, 256) != hipSuccess) {
        lk_free(h);
        tdt_set_error("tdt_links_create: out of device memory (%zu signals)", n);
        return TDT_E_NOMEM;
    }
    hipStream_t st = ctx->stream;
    // the columns, two key and two value buffers: one block that lives for this call only
    const size_t a4 = (N * 4 + 255) & ~(size_t)255, a1 = (N + 255) & ~(size_t)255, a8 = (N * 8 + 255) & ~(size_t)255;
    char *tmp = nullptr;
    int rc = TDT_OK;
    auto body = [&]() -> int {
        TDT_HIP(hipMemcpyAsync(h->d_off, bucket_off, (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, st));
        if (n) {
            if (tdt_dev_malloc((void **)&tmp, 4 * a4 + a1 + 2 * a8) != hipSuccess) {
                tdt_set_error("tdt_links_create: out of device memory sorting %zu signals", n);
                return TDT_E_NOMEM;
            }
            char *p = tmp;
            int32_t *da = (int32_t *)p; p += a4;
            int32_t *db = (int32_t *)p; p += a4;
            unsigned *dv0 = (unsigned *)p; p += a4;
            unsigned *dv1 = (unsigned *)p; p += a4;
            ull *dk0 = (ull *)p; p += a8;
            ull *dk1 = (ull *)p; p += a8;
            uint8_t *dkind = (uint8_t *)p;
            TDT_HIP(hipMemcpyAsync(da, posA, n * 4, hipMemcpyHostToDevice, st));
            TDT_HIP(hipMemcpyAsync(db, posB, n * 4, hipMemcpyHostToDevice, st));
            TDT_HIP(hipMemcpyAsync(dkind, kind, n, hipMemcpyHostToDevice, st));
            const int blocks = (int)((n + 255) / 256);
            hipLaunchKernelGGL(lk_make_keys, dim3(blocks), dim3(256), 0, st, (const int32_t *)da, (int)n, (const long long *)h->d_off, nb, amin,
                               dk0, dv0);
            TDT_CHECK_LAUNCH();
            // only the bits that can differ are sorted: the posA span and the bucket index.  tdt_radix_sort_pairs rebuilds the high key
            // word from keys[0] when no mask bit lies above bit 31 (its narrow mode): that is the case here only for nb <= 1, where
            // every key's high word is the one bucket index 0 — equal in all keys, as the sort requires.
            ull *ks = nullptr;
            unsigned *vs = nullptr;
            int r = tdt_radix_sort_pairs(ctx, dk0, dv0, dk1, dv1, n, tdt_sort_mask((uint64_t)(amax - amin) + 1, (uint64_t)nb), &ks, &vs);
            if (r) return r;
            hipLaunchKernelGGL(lk_pack, dim3(blocks), dim3(256), 0, st, (const ull *)ks, (const unsigned *)vs, (const int32_t *)db,
                               (const uint8_t *)dkind, (int)n, amin, h->rec);
            TDT_CHECK_LAUNCH();
        }
        TDT_HIP(hipStreamSynchronize(st));             // (the host columns and the block below are free again)
        return TDT_OK;
    };
    rc = body();
    if (tmp) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(tmp);
    }
    if (rc) {
        lk_free(h);
        return rc;
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_links_destroy(tdt_links *h) {
    if (!h) return TDT_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);          // (no kernel of the stream still reads the records)
    lk_free(h);
    return TDT_OK;
}

extern "C" int tdt_links_count(tdt_links *h, const int32_t *sites, size_t ns, int64_t *out) {
    if (!h || ns >= 0x7fffffffull || (ns && (!sites || !out))) {
        tdt_set_error("tdt_links_count: bad argument");
        return TDT_E_ARG;
    }
    for (size_t q = 0; q < ns; q++) {
        const int32_t *s = sites + 6 * q;
        if (s[0] < -1 || s[0] >= h->nb) {
            tdt_set_error("tdt_links_count: site %zu names bucket %d of %d", q, s[0], h->nb);
            return TDT_E_RANGE;
        }
        if (s[1] > s[2] || s[3] > s[4]) {
            tdt_set_error("tdt_links_count: site %zu has start > end (A %d..%d, B %d..%d)", q, s[1], s[2], s[3], s[4]);
            return TDT_E_ARG;
        }
    }
    if (ns == 0) return TDT_OK;
    tdt_ctx *ctx = h->ctx;
    TDT_HIP(hipSetDevice(ctx->device));
    const size_t sb = (ns * 24 + 255) & ~(size_t)255;
    if (sb + ns * 16 > h->io_cap) {
        TDT_HIP(hipStreamSynchronize(ctx->stream));
        if (h->d_io) TDT_HIP(hipFree(h->d_io));
        h->d_io = nullptr;
        h->io_cap = 0;
        if (tdt_dev_malloc(&h->d_io, sb + ns * 16) != hipSuccess) {
            tdt_set_error("tdt_links_count: out of device memory (%zu sites)", ns);
            return TDT_E_NOMEM;
        }
        h->io_cap = sb + ns * 16;
    }
    int32_t *ds = (int32_t *)h->d_io;
    long long *dout = (long long *)((char *)h->d_io + sb);
    hipStream_t st = ctx->stream;
    TDT_HIP(hipMemcpyAsync(ds, sites, ns * 24, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(links_count<false>, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, st, (const int2 *)h->rec, (const long long *)h->d_off,
                       h->nb, (const int32_t *)ds, (int)ns, dout, (int *)nullptr);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipMemcpyAsync(out, dout, ns * 16, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}

// The same counts with the sites and the output on the device.  The kernel checks every site (bucket index, start <= end): a bad
// site gets zeros and the call returns TDT_E_RANGE naming the first one.  The stream is synchronised before the return.
extern "C" int tdt_links_count_device(tdt_links *h, const int32_t *d_sites, size_t ns, int64_t *d_out) {
    if (!h || ns >= 0x7fffffffull || (ns && (!d_sites || !d_out)) || ((uintptr_t)d_sites & 7) || ((uintptr_t)d_out & 7)) {
        tdt_set_error("tdt_links_count_device: bad argument");
        return TDT_E_ARG;
    }
    if (ns == 0) return TDT_OK;
    tdt_ctx *ctx = h->ctx;
    TDT_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int bad = 0x7fffffff;                          // (a host word: the stream is synchronised before it goes out of scope)
    TDT_HIP(hipMemcpyAsync(h->d_bad, &bad, sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(links_count<true>, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, st, (const int2 *)h->rec, (const long long *)h->d_off,
                       h->nb, d_sites, (int)ns, (long long *)d_out, h->d_bad);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipMemcpyAsync(&bad, h->d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    if (bad != 0x7fffffff) {
        int32_t s[6] = {0, 0, 0, 0, 0, 0};
        TDT_HIP(hipMemcpy(s, d_sites + 6 * (size_t)bad, sizeof(s), hipMemcpyDeviceToHost));
        tdt_set_error("tdt_links_count_device: site %d (bucket %d of %d, A %d..%d, B %d..%d) is not a valid site", bad, s[0], h->nb, s[1], s[2],
                      s[3], s[4]);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}
