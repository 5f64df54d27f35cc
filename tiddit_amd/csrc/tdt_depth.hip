// Order statistics of the coverage bins for the depth fold-changes of genotyped SV sites (TIDDIT_GENOTYPE_DEPTH, tiddit_depth.py),
// gfx950: the medians of 10^4 .. 10^5 short windows of bins in one launch, and the 101 GC-class medians of every contig.
//
// Non-negative doubles order like their bit patterns, so every k-th smallest value is found by the 8-pass radix SELECT of
// tdt_median.hip (top byte first: a 256-bucket histogram of the candidates that still match the prefix, then the bucket that
// holds rank k) — no sort, and only the two middle order statistics of every window or class leave the device: the host forms
// an even count's median from them with numpy, which makes it numpy.median bit for bit.  -0.0 is read as +0.0; negative values
// and NaN coverage are not supported (a bin's coverage is a sum of non-negative terms).
//
// A window is a row {off, first1, last1, first2, last2, cls} of int64: the bins off + first1 .. off + last1 and
// off + first2 .. off + last2 (both ends inclusive, {-1, -1} = no such range; the two flanks of a site are one window) taken as one
// set.  A bin is usable when gc != -1 — zero coverage counts.  cls == -1: the values are cov[bin].  cls >= 0: the values are
// class_med[cls][gc[bin]] (the contig's GC-class medians, looked up instead of gathered), and a bin whose class median is NaN
// (an empty class) is not usable either.
//   dp_windows_short  one wavefront per window of at most DP_WINDOW_LIMIT bins, ALL of them in one launch: the usable keys are
//                     compacted into LDS (8 KB) once and both selects read them there.
//   dp_windows_long   one workgroup per longer window: the same select over the bins in HBM, both ranks in one set of 8 passes.
//   dp_class_medians  one workgroup per (contig, lower | upper middle): a [101][256] histogram of 32-bit counters (101 KB of the
//                     CU's 160 KB LDS) serves all classes in each of the 8 passes over the contig's bins.  The two middles are two
//                     workgroups rather than one with 16-bit counters: a class of a human chromosome holds far more than 65535
//                     bins, and the second workgroup runs on another CU at the same time.
#include "tdt_common.h"

#define DP_WINDOW_LIMIT 1024       // bins (both ranges together) up to which a window is selected in LDS by one wavefront
#define DP_CLASSES 101             // GC classes 0 .. 100 (per cent)
#define DP_LONG_THREADS 256
#define DP_CLASS_THREADS 1024

typedef unsigned long long ull;

struct DpWindow {
    long long off, first1, last1, first2, last2, cls;
};

__host__ __device__ static inline bool dp_range_ok(long long off, long long first, long long last, long long n) {
    return (first == -1 && last == -1) || (first >= 0 && first <= last && last < n - off);
}

__host__ __device__ static inline bool dp_window_ok(const DpWindow &w, long long n, long long ncls) {
    return w.off >= 0 && w.off <= n && dp_range_ok(w.off, w.first1, w.last1, n) && dp_range_ok(w.off, w.first2, w.last2, n) &&
           w.cls >= -1 && w.cls < ncls;
}

// bin i's key, false when the bin is not usable
__device__ static inline bool dp_key(const double *__restrict__ cov, const signed char *__restrict__ gc, const double *__restrict__ cmed,
                                     long long cls, long long i, ull &key) {
    const int g = gc[i];
    if (g == -1) return false;
    double v;
    if (cls < 0) {
        v = cov[i];
    } else {
        if (g < 0 || g >= DP_CLASSES) return false;
        v = cmed[cls * DP_CLASSES + g];
        if (v != v) return false;               // an empty class has no median
    }
    key = (ull)__double_as_longlong(v + 0.0);   // (-0.0 + 0.0 is +0.0)
    return true;
}

// one wavefront: the sum of hist[256]
__device__ static inline unsigned dp_total(const unsigned *hist, int lane) {
    unsigned s = hist[4 * lane] + hist[4 * lane + 1] + hist[4 * lane + 2] + hist[4 * lane + 3];
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

// one wavefront: the bucket of hist[256] that holds rank k (k < the histogram's sum); k becomes the rank inside that bucket
__device__ static inline unsigned dp_pick(const unsigned *hist, unsigned &k, int lane) {
    const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
    const unsigned s = c0 + c1 + c2 + c3;
    unsigned incl = s;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const unsigned excl = incl - s;
    const bool mine = k >= excl && k < incl;    // exactly one lane
    unsigned b = 0, nk = 0;
    if (mine) {
        const unsigned r = k - excl;
        if (r < c0) { b = 0; nk = r; }
        else if (r < c0 + c1) { b = 1; nk = r - c0; }
        else if (r < c0 + c1 + c2) { b = 2; nk = r - c0 - c1; }
        else { b = 3; nk = r - c0 - c1 - c2; }
        b += 4u * (unsigned)lane;
    }
    const ull m = __ballot(mine);
    const int src = m ? __ffsll((long long)m) - 1 : 0;
    k = __shfl(nk, src);
    return __shfl(b, src);
}

// one wavefront: the k-th smallest (k = 0 ..) of keys[0 .. n) in LDS
__device__ static ull dp_select_lds(const ull *keys, unsigned n, unsigned k, unsigned *hist, int lane) {
    ull prefix = 0;
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        const ull himask = pass ? (~0ull << (shift + 8)) : 0ull;
        for (int i = lane; i < 256; i += 64) hist[i] = 0;
        __syncthreads();
        for (unsigned i = lane; i < n; i += 64) {
            const ull key = keys[i];
            if (((key ^ prefix) & himask) == 0) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        prefix |= (ull)dp_pick(hist, k, lane) << shift;
        __syncthreads();
    }
    return prefix;
}

__global__ __launch_bounds__(64) void dp_windows_short(const double *__restrict__ cov, const signed char *__restrict__ gc, long long n,
                                                        const DpWindow *__restrict__ table, int nq, const double *__restrict__ cmed, int ncls,
                                                        double *__restrict__ lower, double *__restrict__ upper, long long *__restrict__ count,
                                                        int *__restrict__ bad) {
    __shared__ ull keys[DP_WINDOW_LIMIT];
    __shared__ unsigned hist[256];
    __shared__ unsigned s_n;
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= nq) return;
    const DpWindow w = table[q];
    if (!dp_window_ok(w, n, ncls)) {              // (the device entry's table: zeros, and the call names the first such window)
        if (lane == 0) {
            count[q] = 0;
            lower[q] = 0.0;
            upper[q] = 0.0;
            if (bad) atomicMin(bad, q);
        }
        return;
    }
    const long long len1 = w.first1 < 0 ? 0 : w.last1 - w.first1 + 1, len2 = w.first2 < 0 ? 0 : w.last2 - w.first2 + 1;
    if (len1 + len2 > DP_WINDOW_LIMIT) return;    // dp_windows_long's
    const int len = (int)(len1 + len2);
    if (lane == 0) s_n = 0;
    __syncthreads();
    for (int j = lane; j < len; j += 64) {
        const long long i = w.off + (j < len1 ? w.first1 + j : w.first2 + (j - len1));
        ull key;
        if (dp_key(cov, gc, cmed, w.cls, i, key)) keys[atomicAdd(&s_n, 1u)] = key;    // (a select does not mind the order)
    }
    __syncthreads();
    const unsigned m = s_n;
    ull lo = 0, hi = 0;
    if (m) {
        lo = dp_select_lds(keys, m, (m - 1) / 2, hist, lane);
        hi = (m & 1u) ? lo : dp_select_lds(keys, m, m / 2, hist, lane);
    }
    if (lane == 0) {
        count[q] = (long long)m;
        lower[q] = __longlong_as_double((long long)lo);
        upper[q] = __longlong_as_double((long long)hi);
    }
}

__global__ __launch_bounds__(DP_LONG_THREADS) void dp_windows_long(const double *__restrict__ cov, const signed char *__restrict__ gc, long long n,
                                                                    const DpWindow *__restrict__ table, int nq, const double *__restrict__ cmed,
                                                                    int ncls, double *__restrict__ lower, double *__restrict__ upper,
                                                                    long long *__restrict__ count) {
    __shared__ unsigned hist[2][256];
    __shared__ ull s_prefix[2];
    __shared__ unsigned s_total;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (q >= nq) return;
    const DpWindow w = table[q];
    if (!dp_window_ok(w, n, ncls)) return;        // (dp_windows_short has answered it)
    const long long len1 = w.first1 < 0 ? 0 : w.last1 - w.first1 + 1, len2 = w.first2 < 0 ? 0 : w.last2 - w.first2 + 1;
    const long long len = len1 + len2;
    if (len <= DP_WINDOW_LIMIT) return;
    if (tid < 2) s_prefix[tid] = 0;
    unsigned k0 = 0, k1 = 0;                      // (wave 0's: the ranks still to find)
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        const ull himask = pass ? (~0ull << (shift + 8)) : 0ull;
        hist[0][tid] = 0;
        hist[1][tid] = 0;
        __syncthreads();
        const ull p0 = s_prefix[0], p1 = s_prefix[1];
        for (long long j = tid; j < len; j += DP_LONG_THREADS) {
            const long long i = w.off + (j < len1 ? w.first1 + j : w.first2 + (j - len1));
            ull key;
            if (dp_key(cov, gc, cmed, w.cls, i, key)) {
                const unsigned b = (unsigned)(key >> shift) & 255u;
                if (((key ^ p0) & himask) == 0) atomicAdd(&hist[0][b], 1u);
                if (((key ^ p1) & himask) == 0) atomicAdd(&hist[1][b], 1u);
            }
        }
        __syncthreads();
        if (tid < 64) {
            if (pass == 0) {
                const unsigned total = dp_total(hist[0], tid);
                k0 = total ? (total - 1) / 2 : 0;
                k1 = total / 2;
                if (tid == 0) s_total = total;
            }
            const unsigned b0 = dp_pick(hist[0], k0, tid), b1 = dp_pick(hist[1], k1, tid);
            if (tid == 0) {
                s_prefix[0] = p0 | ((ull)b0 << shift);
                s_prefix[1] = p1 | ((ull)b1 << shift);
            }
        }
        __syncthreads();
        if (s_total == 0) break;                  // (uniform: nothing usable)
    }
    if (tid == 0) {
        const bool any = s_total != 0;
        count[q] = (long long)s_total;
        lower[q] = any ? __longlong_as_double((long long)s_prefix[0]) : 0.0;
        upper[q] = any ? __longlong_as_double((long long)s_prefix[1]) : 0.0;
    }
}

// blockIdx.x = 0: the lower middle (and the counts), 1: the upper middle; blockIdx.y = the segment.  out[seg][101].
__global__ __launch_bounds__(DP_CLASS_THREADS) void dp_class_medians(const double *__restrict__ cov, const signed char *__restrict__ gc,
                                                                      const long long *__restrict__ seg, double *__restrict__ lower,
                                                                      double *__restrict__ upper, long long *__restrict__ count) {
    extern __shared__ unsigned dp_hist[];         // [DP_CLASSES][256]
    __shared__ ull s_prefix[DP_CLASSES];
    __shared__ unsigned s_k[DP_CLASSES], s_cnt[DP_CLASSES];
    const int which = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long o = seg[2 * s], len = seg[2 * s + 1];
    if (tid < DP_CLASSES) {
        s_prefix[tid] = 0;
        s_k[tid] = 0;
        s_cnt[tid] = 0;
    }
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        const ull himask = pass ? (~0ull << (shift + 8)) : 0ull;
        for (int i = tid; i < DP_CLASSES * 256; i += DP_CLASS_THREADS) dp_hist[i] = 0;
        __syncthreads();
        for (long long i = tid; i < len; i += DP_CLASS_THREADS) {
            const unsigned g = (unsigned)(int)gc[o + i];
            if (g < (unsigned)DP_CLASSES) {       // (-1 and anything outside 0 .. 100 is in no class)
                const double c = cov[o + i];
                if (c > 0) {
                    const ull key = (ull)__double_as_longlong(c);
                    if (((key ^ s_prefix[g]) & himask) == 0) atomicAdd(&dp_hist[g * 256u + ((unsigned)(key >> shift) & 255u)], 1u);
                }
            }
        }
        __syncthreads();
        for (int g = wave; g < DP_CLASSES; g += DP_CLASS_THREADS / 64) {
            const unsigned *h = dp_hist + g * 256;
            unsigned total, k;
            if (pass == 0) {
                total = dp_total(h, lane);
                k = total ? (which ? total / 2 : (total - 1) / 2) : 0;
            } else {
                total = s_cnt[g];
                k = s_k[g];
            }
            if (total) {                          // (uniform in the wavefront)
                const unsigned b = dp_pick(h, k, lane);
                if (lane == 0) {
                    s_prefix[g] |= (ull)b << shift;
                    s_k[g] = k;
                    s_cnt[g] = total;
                }
            }
        }
        __syncthreads();
    }
    if (tid < DP_CLASSES) {
        const size_t at = (size_t)s * DP_CLASSES + tid;
        const double v = s_cnt[tid] ? __longlong_as_double((long long)s_prefix[tid]) : 0.0;
        if (which == 0) {
            lower[at] = v;
            count[at] = (long long)s_cnt[tid];
        } else {
            upper[at] = v;
        }
    }
}

// ---- window medians -----------------------------------------------------------------------------------------------------------
static int dp_windows_launch(tdt_ctx *ctx, const double *d_cov, const int8_t *d_gc, long long n, const int64_t *d_table, size_t nq,
                             const double *d_cmed, int ncls, double *d_lower, double *d_upper, int64_t *d_count, int *d_bad, bool any_long) {
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(dp_windows_short, dim3((unsigned)nq), dim3(64), 0, st, d_cov, (const signed char *)d_gc, n, (const DpWindow *)d_table,
                       (int)nq, d_cmed, ncls, d_lower, d_upper, (long long *)d_count, d_bad);
    if (any_long)
        hipLaunchKernelGGL(dp_windows_long, dim3((unsigned)nq), dim3(DP_LONG_THREADS), 0, st, d_cov, (const signed char *)d_gc, n,
                           (const DpWindow *)d_table, (int)nq, d_cmed, ncls, d_lower, d_upper, (long long *)d_count);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

static bool dp_misaligned(const void *p) { return ((uintptr_t)p & 7) != 0; }

extern "C" int tdt_window_medians(tdt_ctx *ctx, const double *cov, const int8_t *gc, int64_t n, const int64_t *table, size_t nq,
                                  const double *class_med, int ncls, double *lower, double *upper, int64_t *count) {
    if (!ctx || nq >= 0x7fffffffull || n < 0 || ncls < 0) {
        tdt_set_error("tdt_window_medians: bad argument");
        return TDT_E_ARG;
    }
    if (nq == 0) return TDT_OK;
    if (!table || !lower || !upper || !count || (n && (!cov || !gc)) || (ncls && !class_med) || dp_misaligned(cov) || dp_misaligned(table) ||
        dp_misaligned(class_med) || dp_misaligned(lower) || dp_misaligned(upper) || dp_misaligned(count)) {
        tdt_set_error("tdt_window_medians: a null or misaligned pointer");
        return TDT_E_ARG;
    }
    if (n >= 0x7fffffffll) {
        tdt_set_error("tdt_window_medians: %lld bins (2^31 - 1 or more)", (long long)n);
        return TDT_E_RANGE;
    }
    bool any_long = false;
    for (size_t q = 0; q < nq; q++) {
        DpWindow w;
        memcpy(&w, table + 6 * q, sizeof(w));
        if (w.first1 > w.last1 || w.first2 > w.last2) {
            tdt_set_error("tdt_window_medians: window %zu has first > last (%lld..%lld, %lld..%lld)", q, w.first1, w.last1, w.first2, w.last2);
            return TDT_E_ARG;
        }
        if (!dp_window_ok(w, n, ncls)) {
            tdt_set_error("tdt_window_medians: window %zu (offset %lld, bins %lld..%lld and %lld..%lld, class row %lld of %d) lies outside the %lld bins",
                          q, w.off, w.first1, w.last1, w.first2, w.last2, w.cls, ncls, (long long)n);
            return TDT_E_RANGE;
        }
        const long long len = (w.first1 < 0 ? 0 : w.last1 - w.first1 + 1) + (w.first2 < 0 ? 0 : w.last2 - w.first2 + 1);
        any_long = any_long || len > DP_WINDOW_LIMIT;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n, a8 = (N * 8 + 255) & ~(size_t)255, a1 = (N + 255) & ~(size_t)255, at = (nq * 48 + 255) & ~(size_t)255;
    const size_t ac = ((size_t)ncls * DP_CLASSES * 8 + 255) & ~(size_t)255, ao = (nq * 8 + 255) & ~(size_t)255;
    void *d = nullptr;
    int rc = tdt_scratch(ctx, 10, a8 + a1 + at + ac + 3 * ao + 256, &d);
    if (rc) return rc;
    char *p = (char *)d;
    double *d_cov = (double *)p; p += a8;
    int8_t *d_gc = (int8_t *)p; p += a1;
    int64_t *d_table = (int64_t *)p; p += at;
    double *d_cmed = (double *)p; p += ac;
    double *d_lower = (double *)p; p += ao;
    double *d_upper = (double *)p; p += ao;
    int64_t *d_count = (int64_t *)p;
    hipStream_t st = ctx->stream;
    if (N) {
        TDT_HIP(hipMemcpyAsync(d_cov, cov, N * 8, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(d_gc, gc, N, hipMemcpyHostToDevice, st));
    }
    TDT_HIP(hipMemcpyAsync(d_table, table, nq * 48, hipMemcpyHostToDevice, st));
    if (ncls) TDT_HIP(hipMemcpyAsync(d_cmed, class_med, (size_t)ncls * DP_CLASSES * 8, hipMemcpyHostToDevice, st));
    rc = dp_windows_launch(ctx, d_cov, d_gc, n, d_table, nq, d_cmed, ncls, d_lower, d_upper, d_count, nullptr, any_long);
    if (rc) return rc;
    TDT_HIP(hipMemcpyAsync(lower, d_lower, nq * 8, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipMemcpyAsync(upper, d_upper, nq * 8, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipMemcpyAsync(count, d_count, nq * 8, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}

// The same with everything in HBM.  The kernel checks every window: a refused one gets zeros and the call returns TDT_E_RANGE naming
// the first.  The stream is synchronised before the return.
extern "C" int tdt_window_medians_device(tdt_ctx *ctx, const double *d_cov, const int8_t *d_gc, int64_t n, const int64_t *d_table, size_t nq,
                                         const double *d_class_med, int ncls, double *d_lower, double *d_upper, int64_t *d_count) {
    if (!ctx || nq >= 0x7fffffffull || n < 0 || ncls < 0) {
        tdt_set_error("tdt_window_medians_device: bad argument");
        return TDT_E_ARG;
    }
    if (nq == 0) return TDT_OK;
    if (!d_table || !d_lower || !d_upper || !d_count || (n && (!d_cov || !d_gc)) || (ncls && !d_class_med) || dp_misaligned(d_cov) ||
        dp_misaligned(d_table) || dp_misaligned(d_class_med) || dp_misaligned(d_lower) || dp_misaligned(d_upper) || dp_misaligned(d_count)) {
        tdt_set_error("tdt_window_medians_device: a null or misaligned pointer");
        return TDT_E_ARG;
    }
    if (n >= 0x7fffffffll) {
        tdt_set_error("tdt_window_medians_device: %lld bins (2^31 - 1 or more)", (long long)n);
        return TDT_E_RANGE;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    void *d = nullptr;
    int rc = tdt_scratch(ctx, 10, 256, &d);
    if (rc) return rc;
    int *d_bad = (int *)d;
    hipStream_t st = ctx->stream;
    int bad = 0x7fffffff;                          // (a host word: the stream is synchronised before it goes out of scope)
    TDT_HIP(hipMemcpyAsync(d_bad, &bad, sizeof(int), hipMemcpyHostToDevice, st));
    rc = dp_windows_launch(ctx, d_cov, d_gc, n, d_table, nq, d_class_med, ncls, d_lower, d_upper, d_count, d_bad, true);
    if (rc) return rc;
    TDT_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    if (bad != 0x7fffffff) {
        tdt_set_error("tdt_window_medians_device: window %d is not a valid window of the %lld bins", bad, (long long)n);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

// ---- GC-class medians ---------------------------------------------------------------------------------------------------------
static int dp_check_segments(const char *who, int64_t n, const int64_t *seg, int nseg) {
    for (int s = 0; s < nseg; s++) {
        if (seg[2 * s + 1] < 0) {
            tdt_set_error("%s: segment %d has a negative length", who, s);
            return TDT_E_ARG;
        }
        if (seg[2 * s] < 0 || seg[2 * s] > n || seg[2 * s + 1] > n - seg[2 * s]) {
            tdt_set_error("%s: segment %d (offset %lld, %lld bins) lies outside the %lld bins", who, s, (long long)seg[2 * s],
                          (long long)seg[2 * s + 1], (long long)n);
            return TDT_E_RANGE;
        }
    }
    return TDT_OK;
}

static int dp_classes_launch(tdt_ctx *ctx, const double *d_cov, const int8_t *d_gc, const long long *d_seg, int nseg, double *d_lower,
                             double *d_upper, int64_t *d_count) {
    const size_t lds = (size_t)DP_CLASSES * 256 * sizeof(unsigned);
    TDT_HIP(hipFuncSetAttribute((const void *)dp_class_medians, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(dp_class_medians, dim3(2, (unsigned)nseg), dim3(DP_CLASS_THREADS), lds, ctx->stream, d_cov, (const signed char *)d_gc, d_seg,
                       d_lower, d_upper, (long long *)d_count);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

extern "C" int tdt_gc_class_medians_device(tdt_ctx *ctx, const double *d_cov, const int8_t *d_gc, int64_t n, const int64_t *seg, int nseg,
                                           double *d_lower, double *d_upper, int64_t *d_count) {
    if (!ctx || nseg < 0 || nseg > 65535 || n < 0) {
        tdt_set_error("tdt_gc_class_medians_device: bad argument");
        return TDT_E_ARG;
    }
    if (nseg == 0) return TDT_OK;
    if (!seg || !d_lower || !d_upper || !d_count || (n && (!d_cov || !d_gc)) || dp_misaligned(d_cov) || dp_misaligned(d_lower) ||
        dp_misaligned(d_upper) || dp_misaligned(d_count)) {
        tdt_set_error("tdt_gc_class_medians_device: a null or misaligned pointer");
        return TDT_E_ARG;
    }
    int rc = dp_check_segments("tdt_gc_class_medians_device", n, seg, nseg);
    if (rc) return rc;
    for (int s = 0; s < nseg; s++)
        if (seg[2 * s + 1] >= 0xffffffffll) {
            tdt_set_error("tdt_gc_class_medians_device: segment %d has 2^32 - 1 bins or more", s);
            return TDT_E_RANGE;
        }
    TDT_HIP(hipSetDevice(ctx->device));
    void *d = nullptr;
    rc = tdt_scratch(ctx, 10, (size_t)nseg * 16 + 256, &d);
    if (rc) return rc;
    long long *d_seg = (long long *)((char *)d + 256);     // (the first 256 bytes are tdt_window_medians_device's word)
    hipStream_t st = ctx->stream;
    TDT_HIP(hipMemcpyAsync(d_seg, seg, (size_t)nseg * 16, hipMemcpyHostToDevice, st));
    rc = dp_classes_launch(ctx, d_cov, d_gc, d_seg, nseg, d_lower, d_upper, d_count);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}

extern "C" int tdt_gc_class_medians(tdt_ctx *ctx, const double *cov, const int8_t *gc, int64_t n, const int64_t *seg, int nseg, double *lower,
                                    double *upper, int64_t *count) {
    if (!ctx || nseg < 0 || nseg > 65535 || n < 0) {
        tdt_set_error("tdt_gc_class_medians: bad argument");
        return TDT_E_ARG;
    }
    if (nseg == 0) return TDT_OK;
    if (!seg || !lower || !upper || !count || (n && (!cov || !gc)) || dp_misaligned(cov) || dp_misaligned(seg) || dp_misaligned(lower) ||
        dp_misaligned(upper) || dp_misaligned(count)) {
        tdt_set_error("tdt_gc_class_medians: a null or misaligned pointer");
        return TDT_E_ARG;
    }
    int rc = dp_check_segments("tdt_gc_class_medians", n, seg, nseg);
    if (rc) return rc;
    for (int s = 0; s < nseg; s++)
        if (seg[2 * s + 1] >= 0xffffffffll) {
            tdt_set_error("tdt_gc_class_medians: segment %d has 2^32 - 1 bins or more", s);
            return TDT_E_RANGE;
        }
    TDT_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n, a8 = (N * 8 + 255) & ~(size_t)255, a1 = (N + 255) & ~(size_t)255, as = ((size_t)nseg * 16 + 255) & ~(size_t)255;
    const size_t ao = ((size_t)nseg * DP_CLASSES * 8 + 255) & ~(size_t)255;
    void *d = nullptr;
    rc = tdt_scratch(ctx, 10, a8 + a1 + as + 3 * ao + 256, &d);
    if (rc) return rc;
    char *p = (char *)d;
    double *d_cov = (double *)p; p += a8;
    int8_t *d_gc = (int8_t *)p; p += a1;
    long long *d_seg = (long long *)p; p += as;
    double *d_lower = (double *)p; p += ao;
    double *d_upper = (double *)p; p += ao;
    int64_t *d_count = (int64_t *)p;
    hipStream_t st = ctx->stream;
    if (N) {
        TDT_HIP(hipMemcpyAsync(d_cov, cov, N * 8, hipMemcpyHostToDevice, st));
        TDT_HIP(hipMemcpyAsync(d_gc, gc, N, hipMemcpyHostToDevice, st));
    }
    TDT_HIP(hipMemcpyAsync(d_seg, seg, (size_t)nseg * 16, hipMemcpyHostToDevice, st));
    rc = dp_classes_launch(ctx, d_cov, d_gc, d_seg, nseg, d_lower, d_upper, d_count);
    if (rc) return rc;
    const size_t ob = (size_t)nseg * DP_CLASSES * 8;
    TDT_HIP(hipMemcpyAsync(lower, d_lower, ob, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipMemcpyAsync(upper, d_upper, ob, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipMemcpyAsync(count, d_count, ob, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}
