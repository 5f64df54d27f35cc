// Signal clustering ("DBSCAN") for gfx950 (MI355X).
//
// The reference's DBSCAN.py is two 1-D sliding-window passes driven by a sequential run-labelling
// state machine (x_coordinate_clustering DBSCAN.py:33-64, y_coordinate_clustering :66-123).  Its
// closed form is data parallel:
//   x pass   p[i]  = (i <= n-m) && max_{j in (i, min(i+m,n-1)]} |x_j - x_i| < eps
//            runs  = maximal stretches of consecutive true p, numbered 0,1,.. (an inclusive scan of run starts)
//            lab[k]= id of the run holding j* = the largest j <= k with p[j], if k - j* <= m-1, else -1
//   y pass   every x-cluster is a contiguous index range; its members are stably sorted by y, the
//            same run labelling is applied with window m-1, sub-run 1 keeps the x id and sub-run
//            s > 1 becomes (R-1) + #extra sub-runs of earlier x-clusters + (s-1).
// All of it is integer compares, prefix sums and a segmented sort: HBM/latency-bound, no MFMA.
// Several independent (chrA,chrB) buckets are processed by the same launches (ids restart per bucket).
// ---- measurement builds declare themselves (tdt_build_flags): the macros this file was compiled with, before any default is set
extern const char *const tdt_variant_dbscan;
const char *const tdt_variant_dbscan = ""
#ifdef DT_FTPB
    " DT_FTPB"
#endif
#ifdef DT_NW
    " DT_NW"
#endif
#ifdef DT_THREADS
    " DT_THREADS"
#endif
#ifdef DBF_THREADS
    " DBF_THREADS"
#endif
    ;

#include "tdt_common.h"
#include <chrono>

#include <atomic>
#include <thread>

#include <algorithm>
#include <cmath>

#define DB_THREADS 256
#define DB_ITEMS 4
#define DB_TILE (DB_THREADS * DB_ITEMS)
#define DB_SMALL 128  // x-clusters up to this many members are y-sorted by in-kernel rank counting


// The bucket of position i when the wave's lanes hold positions inside [first, last] (first / last the same in every lane): the search
// is done ONCE, on the scalar unit, for `first`; a wave of 64-128 consecutive positions almost never contains a bucket boundary (300
// buckets in 10 M signals), and then one more scalar load settles it.  Lanes of a wave that does contain boundaries step forward from
// the first position's bucket.  (Per-lane binary searches — nine dependent vector loads per point — were what dbt_finish took 33 us for
// where the one-bucket dbt_finish1 takes 14.)
__device__ __forceinline__ int db_bucket_wave(const int *__restrict__ boff, int nb, int first, int last, int i) {
    if (nb == 1) return 0;
    const int f = __builtin_amdgcn_readfirstlane(first), l = __builtin_amdgcn_readfirstlane(last);
    int lo = 0, hi = nb;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (boff[mid] <= f) lo = mid;
        else hi = mid;
    }
    int b = lo;
    if (lo + 1 < nb && boff[lo + 1] <= l)                  // (wave-uniform) a boundary inside the wave's range
        while (b + 1 < nb && boff[b + 1] <= i) b++;
    return b;
}
// largest b in [0, nb) with boff[b] <= i
__device__ __forceinline__ int db_bucket(const int *__restrict__ boff, int nb, int i) {
    if (nb == 1) return 0;
    int lo = 0, hi = nb;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (boff[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ unsigned db_absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

#include "tdt_dbscan_fused.h"
#include "tdt_dbscan_tile.h"

// ---------------------------------------------------------------------------------------- scan
// In-place inclusive scan of a u32 array: reduce tiles -> scan the tile sums (one block) -> apply.
__global__ __launch_bounds__(DB_THREADS) void scan_reduce(const unsigned *__restrict__ v, int n, unsigned *__restrict__ tsum) {
    __shared__ unsigned red[DB_THREADS / 64];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * DB_TILE + tid * DB_ITEMS;
    unsigned s = 0;
    if (i0 + DB_ITEMS <= n) {
        const uint4 q = *reinterpret_cast<const uint4 *>(v + i0);
        s = q.x + q.y + q.z + q.w;
    } else {
        for (int j = 0; j < DB_ITEMS; j++)
            if (i0 + j < n) s += v[i0 + j];
    }
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) tsum[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// exclusive scan of tsum[0..nt) in place, single workgroup of 1024 threads
__global__ __launch_bounds__(1024) void scan_tiles(unsigned *tsum, int nt) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < nt; base += 1024) {
        const int i = base + tid;
        const unsigned v = i < nt ? tsum[i] : 0;
        unsigned s = v;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        unsigned woff = 0;
        for (int w = 0; w < wave; w++) woff += wsum[w];
        const unsigned carry = carry_s;
        if (i < nt) tsum[i] = carry + woff + s - v;
        __syncthreads();
        if (tid == 1023) carry_s = carry + woff + s;
        __syncthreads();
    }
}

__global__ __launch_bounds__(DB_THREADS) void scan_apply(unsigned *__restrict__ v, int n, const unsigned *__restrict__ tsum) {
    __shared__ unsigned wsum[DB_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * DB_TILE + tid * DB_ITEMS;
    unsigned a[DB_ITEMS];
    const bool full = i0 + DB_ITEMS <= n;
    if (full) {
        const uint4 q = *reinterpret_cast<const uint4 *>(v + i0);
        a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w;
    } else {
        for (int j = 0; j < DB_ITEMS; j++) a[j] = i0 + j < n ? v[i0 + j] : 0;
    }
    a[1] += a[0]; a[2] += a[1]; a[3] += a[2];
    unsigned s = a[3];
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(s, d);
        if (lane >= d) s += t;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    unsigned off = tsum[blockIdx.x] + s - a[3];
    for (int w = 0; w < wave; w++) off += wsum[w];
    if (full) {
        *reinterpret_cast<uint4 *>(v + i0) = make_uint4(a[0] + off, a[1] + off, a[2] + off, a[3] + off);
    } else {
        for (int j = 0; j < DB_ITEMS; j++)
            if (i0 + j < n) v[i0 + j] = a[j] + off;
    }
}

// -------------------------------------------------------------------------------------- x pass
// p[i] (DBSCAN.py:41-51) and run-start flags (the `cluster` boolean of :52-62)
__global__ __launch_bounds__(DB_THREADS) void dbx_flags(const unsigned *__restrict__ x, int n, const int *__restrict__ boff,
                                                        int nb, unsigned long long eps, int m,
                                                        unsigned char *__restrict__ px, unsigned *__restrict__ sx) {
    const int i0 = (blockIdx.x * DB_THREADS + threadIdx.x) * DB_ITEMS;
    if (i0 >= n) return;
    int b = db_bucket(boff, nb, i0 > 0 ? i0 - 1 : 0);
    bool prev = false;
    for (int i = (i0 > 0 ? i0 - 1 : 0); i < i0 + DB_ITEMS && i < n; i++) {
        while (i >= boff[b + 1]) b++;
        const int bend = boff[b + 1];
        bool p = false;
        if (i + m <= bend) {  // the loop `for i in range(0, len(data)-m+1)` (:39)
            const int hi = min(i + m, bend - 1);  // data[i+1:i+m+1] truncates at the array end (:43)
            const unsigned xi = x[i];
            unsigned maxd = 0;
            for (int j = i + 1; j <= hi; j++) maxd = max(maxd, db_absdiff(x[j], xi));
            p = (unsigned long long)maxd < eps;
        }
        if (i >= i0) {
            px[i] = p;
            sx[i] = (p && !prev) ? 1u : 0u;
        }
        prev = p;
    }
}

// lab[k] = (scan of run starts at j*) - 1; also the number of runs before every bucket
__global__ __launch_bounds__(DB_THREADS) void dbx_labels(const unsigned char *__restrict__ px, const unsigned *__restrict__ sx_incl,
                                                         int n, int m, const int *__restrict__ boff, int nb,
                                                         int *__restrict__ xlab, unsigned *__restrict__ runbase) {
    const int k = blockIdx.x * DB_THREADS + threadIdx.x;
    if (k >= n) return;
    int lab = -1;
    for (int j = k; j >= 0 && j > k - m; j--) {
        if (px[j]) {
            lab = (int)sx_incl[j] - 1;
            break;
        }
    }
    xlab[k] = lab;
    const int b = db_bucket(boff, nb, k);
    if (k + 1 == boff[b + 1]) {
        const unsigned s = sx_incl[k];
        for (int bb = b + 1; bb <= nb && boff[bb] == k + 1; bb++) runbase[bb] = s;
    }
}

__global__ __launch_bounds__(DB_THREADS) void db_segments(const int *__restrict__ xlab, int n, int *__restrict__ seg_start,
                                                          int *__restrict__ seg_end) {
    const int k = blockIdx.x * DB_THREADS + threadIdx.x;
    if (k >= n) return;
    const int l = xlab[k];
    if (l < 0) return;
    if (k == 0 || xlab[k - 1] != l) seg_start[l] = k;
    if (k == n - 1 || xlab[k + 1] != l) seg_end[l] = k + 1;
}

// x-only result (x_coordinate_clustering's return value)
__global__ __launch_bounds__(DB_THREADS) void dbx_final(const int *__restrict__ xlab, int n, const int *__restrict__ boff, int nb,
                                                        const unsigned *__restrict__ runbase, double *__restrict__ labels,
                                                        long long *__restrict__ last_id) {
    const int k = blockIdx.x * DB_THREADS + threadIdx.x;
    if (k < nb && last_id) last_id[k] = (long long)(runbase[k + 1] - runbase[k]) - 1;
    if (k >= n) return;
    const int l = xlab[k];
    labels[k] = l < 0 ? -1.0 : (double)(l - (int)runbase[db_bucket(boff, nb, k)]);
}

// One word back to the host without a stream synchronisation: the value goes to pinned host memory, then a sequence number;
// the host spins on the sequence number (a hipStreamSynchronize wake-up costs ~40 us, a third of a 5 M-point pass).
__global__ void db_signal_host(const unsigned *__restrict__ word, volatile unsigned *host, unsigned seq) {
    host[0] = *word;
    __threadfence_system();
    host[1] = seq;
}

// -------------------------------------------------------------------------------------- y pass
// stable sort by y inside every x-cluster (DBSCAN.py:76-81): rank counting for small clusters; members of
// larger clusters are flagged and go through the radix sort below
__global__ __launch_bounds__(DB_THREADS) void dby_rank(const int *__restrict__ xlab, const unsigned *__restrict__ y, int n,
                                                       const int *__restrict__ seg_start, const int *__restrict__ seg_end,
                                                       unsigned *__restrict__ ys, unsigned *__restrict__ ord,
                                                       unsigned *__restrict__ lflag, unsigned *__restrict__ anylarge) {
    const int k = blockIdx.x * DB_THREADS + threadIdx.x;
    if (k >= n) return;
    const int l = xlab[k];
    unsigned large = 0;
    if (l < 0) {
        ys[k] = 0;
        ord[k] = k;
    } else {
        const int s0 = seg_start[l], s1 = seg_end[l];
        const unsigned yk = y[k];
        if (s1 - s0 <= DB_SMALL) {
            int rank = 0;
            // rank = members sorting before k.  The wave runs as long as its largest cluster, so the cost is loop
            // overhead x trip count: 4 members per trip (clamped loads, no per-member branch)
            for (int j = s0; j < s1; j += 4) {
                const unsigned v0 = y[j], v1 = y[min(j + 1, s1 - 1)], v2 = y[min(j + 2, s1 - 1)], v3 = y[min(j + 3, s1 - 1)];
                rank += (v0 < yk) || (v0 == yk && j < k);
                rank += (j + 1 < s1) && ((v1 < yk) || (v1 == yk && j + 1 < k));
                rank += (j + 2 < s1) && ((v2 < yk) || (v2 == yk && j + 2 < k));
                rank += (j + 3 < s1) && ((v3 < yk) || (v3 == yk && j + 3 < k));
            }
            ys[s0 + rank] = yk;
            ord[s0 + rank] = k;
        } else {
            large = 1;
            ys[k] = yk;   // placeholders: the speculative y pass runs before the large clusters are sorted and must
            ord[k] = k;   // scatter in bounds; dby_large_scatter overwrites both
            if (k == s0) *anylarge = 1u;
        }
    }
    lflag[k] = large;
}

// members of large clusters, compacted in position order: key = cluster id << 32 | y, value = position
__global__ __launch_bounds__(DB_THREADS) void dby_large_compact(const int *__restrict__ xlab, const unsigned *__restrict__ y, int n,
                                                                const unsigned *__restrict__ lincl, unsigned long long *__restrict__ ck,
                                                                unsigned *__restrict__ cv, unsigned *__restrict__ cpos) {
    const int k = blockIdx.x * DB_THREADS + threadIdx.x;
    if (k >= n) return;
    const unsigned inc = lincl[k], prev = k ? lincl[k - 1] : 0u;
    if (inc != prev) {
        ck[prev] = ((unsigned long long)(unsigned)xlab[k] << 32) | y[k];
        cv[prev] = (unsigned)k;
        cpos[prev] = (unsigned)k;
    }
}

// clusters are contiguous and the compaction kept position order, so the j-th sorted pair belongs at the j-th position
__global__ __launch_bounds__(DB_THREADS) void dby_large_scatter(const unsigned long long *__restrict__ ksorted, const unsigned *__restrict__ vsorted,
                                                                const unsigned *__restrict__ cpos, int nl, unsigned *__restrict__ ys,
                                                                unsigned *__restrict__ ord) {
    const int j = blockIdx.x * DB_THREADS + threadIdx.x;
    if (j >= nl) return;
    const unsigned p = cpos[j];
    ys[p] = (unsigned)ksorted[j];
    ord[p] = vsorted[j];
}

// window test on the sorted y of each x-cluster (DBSCAN.py:90-99) and sub-run starts (:101-110)
__global__ __launch_bounds__(DB_THREADS) void dby_flags(const int *__restrict__ xlab, int n, const int *__restrict__ seg_start,
                                                        const int *__restrict__ seg_end, const unsigned *__restrict__ ys,
                                                        unsigned long long eps, int m, unsigned char *__restrict__ py,
                                                        unsigned *__restrict__ sy) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    const int l = xlab[i];
    bool p = false, prev = false;
    if (l >= 0) {
        const int s0 = seg_start[l], s1 = seg_end[l];
        if (i + m <= s1) p = (unsigned long long)(ys[i + m - 1] - ys[i]) < eps;  // next = y[i+1:i+m], sorted => max is the last
        if (i > s0 && (i - 1) + m <= s1) prev = (unsigned long long)(ys[i + m - 2] - ys[i - 1]) < eps;
    }
    py[i] = p;
    sy[i] = (p && !prev) ? 1u : 0u;
}

// extra sub-runs of every x-cluster, stored at the cluster's first position (`cluster_id += sub_cluster_id-1`, :121-122)
__global__ __launch_bounds__(DB_THREADS) void dby_extras(const int *__restrict__ xlab, int n, const int *__restrict__ seg_start,
                                                         const int *__restrict__ seg_end, const unsigned *__restrict__ sy_incl,
                                                         unsigned *__restrict__ ex) {
    const int k = blockIdx.x * DB_THREADS + threadIdx.x;
    if (k >= n) return;
    const int l = xlab[k];
    unsigned e = 0;
    if (l >= 0 && seg_start[l] == k) {
        const unsigned sr = sy_incl[seg_end[l] - 1] - (k > 0 ? sy_incl[k - 1] : 0u);
        e = sr > 1 ? sr - 1 : 0;
    }
    ex[k] = e;
}

// relabel (DBSCAN.py:112-119) and scatter back to the input order
__global__ __launch_bounds__(DB_THREADS) void dby_final(const int *__restrict__ xlab, int n, int m, const int *__restrict__ seg_start,
                                                        const unsigned char *__restrict__ py, const unsigned *__restrict__ sy_incl,
                                                        const unsigned *__restrict__ ex_incl, const unsigned *__restrict__ ord,
                                                        const int *__restrict__ boff, int nb, const unsigned *__restrict__ runbase,
                                                        double *__restrict__ labels, long long *__restrict__ last_id) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i < nb && last_id) {
        const int b0 = boff[i], b1 = boff[i + 1];
        const long long extras = (long long)(b1 > 0 ? ex_incl[b1 - 1] : 0u) - (long long)(b0 > 0 ? ex_incl[b0 - 1] : 0u);
        last_id[i] = (long long)(runbase[i + 1] - runbase[i]) - 1 + extras;
    }
    if (i >= n) return;
    const int l = xlab[i];
    if (l < 0) {
        labels[i] = -1.0;  // ord[i] == i for noise
        return;
    }
    double lab = -1.0;
    for (int j = i; j >= 0 && j > i - m; j--) {
        if (py[j]) {
            const int s0 = seg_start[l];
            const unsigned s = sy_incl[j] - (s0 > 0 ? sy_incl[s0 - 1] : 0u);
            const int b = db_bucket(boff, nb, i);
            const unsigned rb = runbase[b];
            if (s == 1) {
                lab = (double)((unsigned)l - rb);
            } else {
                const int b0 = boff[b];
                const unsigned xoff = (s0 > 0 ? ex_incl[s0 - 1] : 0u) - (b0 > 0 ? ex_incl[b0 - 1] : 0u);
                lab = (double)((long long)(runbase[b + 1] - rb) - 1 + (long long)xoff + (long long)(s - 1));
            }
            break;
        }
    }
    labels[ord[i]] = lab;
}

// ------------------------------------------------------------------------------------------ host
int tdt_scan_u32_inclusive(tdt_ctx *ctx, unsigned *d_v, int n, unsigned *d_tsum) {
    const int nt = (n + DB_TILE - 1) / DB_TILE;
    hipLaunchKernelGGL(scan_reduce, dim3(nt), dim3(DB_THREADS), 0, ctx->stream, (const unsigned *)d_v, n, d_tsum);
    hipLaunchKernelGGL(scan_tiles, dim3(1), dim3(1024), 0, ctx->stream, d_tsum, nt);
    hipLaunchKernelGGL(scan_apply, dim3(nt), dim3(DB_THREADS), 0, ctx->stream, d_v, n, (const unsigned *)d_tsum);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

// ---- the pinned status block of the context, {value, sequence number}: one word back from the device without a stream
// synchronisation (a hipStreamSynchronize wake-up costs ~40 us, a third of a 5 M-point pass).  The host picks a sequence number and
// clears the block (db_word_arm), a kernel of the pass stores the value, a system fence and then the number (dt_signal_host,
// db_signal_host), and the host spins on the number (db_word_wait).
struct DbHostWord {
    volatile unsigned *w = nullptr;
    unsigned seq = 0;
};

static int db_word_arm(tdt_ctx *ctx, DbHostWord *hw) {
    static std::atomic<unsigned> counter{0};
    void *hp = nullptr;
    const int rc = tdt_pinned(ctx, 2, 64, &hp);
    if (rc) return rc;
    hw->w = (volatile unsigned *)hp;
    hw->seq = ++counter;
    if (hw->seq == 0) hw->seq = ++counter;              // never 0: that is what the block is cleared to
    hw->w[1] = 0;
    return TDT_OK;
}

static int db_word_wait(tdt_ctx *ctx, const DbHostWord &hw, unsigned *value) {
    bool seen = false;
    for (long spin = 0; spin < 4000000; spin++) {       // a few milliseconds at most, then the ordinary wait
        if (hw.w[1] == hw.seq) {
            seen = true;
            break;
        }
        __builtin_ia32_pause();
    }
    if (!seen) TDT_HIP(hipStreamSynchronize(ctx->stream));
    *value = hw.w[0];
    return TDT_OK;
}

// ---- workspaces (tdt_carver: size and pointers from the one list)
// slot 3: the bucket offsets and everything routes 2 and 3 keep per point.  Every call asks for it up front, whichever route it
// takes, so the buffers a context holds after a call do not depend on the route.
struct DbWork {
    int *boff;
    unsigned *runbase, *cnt, *tsum;
    unsigned char *px, *py;
    unsigned *sx, *sy, *ex;
    int *xlab, *seg0, *seg1;
    unsigned *ys, *ord;
    unsigned long long *key, *ksorted;           // the large clusters' sort: keys in / out, values in / out, positions, flags
    unsigned *v0, *v1, *cpos, *lflag;
    size_t lay(void *base, int n, int nb) {
        tdt_carver c(base);
        const size_t N = (size_t)(n ? n : 1);
        boff = c.take<int>((size_t)nb + 1), runbase = c.take<unsigned>((size_t)nb + 1), cnt = c.take<unsigned>(64);
        tsum = c.take<unsigned>((N + DB_TILE - 1) / DB_TILE);
        px = c.take<unsigned char>(N), py = c.take<unsigned char>(N);
        sx = c.take<unsigned>(N), sy = c.take<unsigned>(N), ex = c.take<unsigned>(N);
        xlab = c.take<int>(N), seg0 = c.take<int>(N), seg1 = c.take<int>(N);
        ys = c.take<unsigned>(N), ord = c.take<unsigned>(N);
        key = c.take<unsigned long long>(N), ksorted = c.take<unsigned long long>(N);
        v0 = c.take<unsigned>(N), v1 = c.take<unsigned>(N), cpos = c.take<unsigned>(N), lflag = c.take<unsigned>(N);
        return c.size;
    }
};

// slot 20: what the tile-resident pass keeps from call to call — the status block its kernels re-zero themselves and the two
// group-sum arrays that alternate by call parity.  A fixed size, so the block never moves once it exists.
struct DtState {
    unsigned *flags, *grp[2];
    size_t lay(void *base) {
        tdt_carver c(base);
        flags = c.take<unsigned>(64), grp[0] = c.take<unsigned>((size_t)2 * DT_GRPMAX), grp[1] = c.take<unsigned>((size_t)2 * DT_GRPMAX);
        return c.size;
    }
};

// slot 21: the tile-resident pass's arrays of one call.  ONE layout for every caller: the finish kernel of a pass that does not
// stand decodes whatever an earlier call left in `code`.
struct DtWork {
    unsigned short *code;
    unsigned *brun, *bext, *aggR, *aggE, *runbase, *extbase;
    size_t lay(void *base, int n, int nb) {
        tdt_carver c(base);
        const size_t ntt = ((size_t)n + DT_T - 1) / DT_T;
        code = c.take<unsigned short>((size_t)n + 8);
        brun = c.take<unsigned>((size_t)nb + 1), bext = c.take<unsigned>((size_t)nb + 1);
        aggR = c.take<unsigned>(ntt), aggE = c.take<unsigned>(ntt);
        runbase = c.take<unsigned>((size_t)nb + 1), extbase = c.take<unsigned>((size_t)nb + 1);
        return c.size;
    }
};

// slot 8: the ballot masks of route 2.  Whole tiles: its kernels store all 64 words of their tile (+ 2 guard words).
struct DbfWork {
    DbfCtl *ctl;
    ull *agg_x, *agg_1, *agg_2, *PM, *PY, *HM, *BM, *EM, *S1M, *FM;
    size_t lay(void *base, int ntf) {
        tdt_carver c(base);
        const size_t nw = (size_t)ntf * DBF_WORDS + 2;
        ctl = c.take<DbfCtl>(1);
        agg_x = c.take<ull>(ntf), agg_1 = c.take<ull>(ntf), agg_2 = c.take<ull>(ntf);
        PM = c.take<ull>(nw), PY = c.take<ull>(nw), HM = c.take<ull>(nw), BM = c.take<ull>(nw);
        EM = c.take<ull>(nw), S1M = c.take<ull>(nw), FM = c.take<ull>(nw);
        return c.size;
    }
};

// ---- route 1: the tile-resident pass (tdt_dbscan_tile.h) — dbt_tile, then dbt_finish1 (one bucket) or dbt_scan + dbt_finish.
// The one driver of both its users: tdt_dbscan_device, and tdt_dbscan_y_device with caller-supplied x labels in place of x (d_xlab
// non-null: one bucket, extra sub-runs numbered from id_base).  d_boff is read by the kernels for nb > 1 only.
// *stands == false: an x-cluster was too large for this pass — the labels were NOT produced and the caller takes another route.
// Only one-bucket calls (caller-labels calls are such) use the group sums, so only they flip the parity of ctx->tile_calls.
static int db_tile_pass(tdt_ctx *ctx, const unsigned *d_x, const unsigned *d_y, int n, const int *d_boff, int nb, uint64_t eps, int m,
                        int mode, const int *d_xlab, long long id_base, double *d_labels, long long *d_last_id, bool *stands) {
    hipStream_t st = ctx->stream;
    const int ntt = (n + DT_T - 1) / DT_T;
    DtState S;
    DtWork W;
    int rc = tdt_scratch_layout(ctx, 20, S);
    if (rc) return rc;
    rc = tdt_scratch_layout(ctx, 21, W, n, nb);
    if (rc) return rc;
    if (ctx->tile_flags_zeroed != S.flags) {       // first use of this block; afterwards the kernel that reports the status re-zeroes it
        TDT_HIP(hipMemsetAsync(S.flags, 0, DtState().lay(nullptr), st));
        ctx->tile_flags_zeroed = S.flags;
    }
    const bool odd = nb == 1 && (ctx->tile_calls++ & 1u) != 0;
    DtParams TP;
    TP.x = d_xlab ? (const unsigned *)d_xlab : d_x, TP.y = d_y, TP.n = n;
    TP.boff = d_boff, TP.nb = nb;
    TP.eps32 = eps > 0xffffffffull ? 0xffffffffu : (unsigned)eps, TP.wide = eps > 0xffffffffull, TP.m = m;
    TP.code = W.code, TP.aggR = W.aggR, TP.aggE = W.aggE, TP.brun = W.brun, TP.bext = W.bext;
    TP.flags = S.flags, TP.grp = S.grp[odd];
    DbHostWord hw;
    rc = db_word_arm(ctx, &hw);
    if (rc) return rc;
    if (d_xlab) hipLaunchKernelGGL((dbt_tile<true, false, true>), dim3(ntt), dim3(DT_THREADS), 0, st, TP);
    else if (nb == 1 && mode == 0) hipLaunchKernelGGL((dbt_tile<true, false>), dim3(ntt), dim3(DT_THREADS), 0, st, TP);
    else if (nb == 1) hipLaunchKernelGGL((dbt_tile<true, true>), dim3(ntt), dim3(DT_THREADS), 0, st, TP);
    else if (mode == 0) hipLaunchKernelGGL((dbt_tile<false, false>), dim3(ntt), dim3(DT_THREADS), 0, st, TP);
    else hipLaunchKernelGGL((dbt_tile<false, true>), dim3(ntt), dim3(DT_THREADS), 0, st, TP);
    TDT_CHECK_LAUNCH();
    // the kernel behind dbt_tile stores the word that says whether the pass stands as soon as the tile kernel is done
    if (nb == 1) {
        ctx->tile_groups_max = std::max(ctx->tile_groups_max, (ntt + DT_GRP - 1) / DT_GRP);
        hipLaunchKernelGGL(dbt_finish1, dim3((ntt + DT_FTPB - 1) / DT_FTPB), dim3(256), 0, st, (const unsigned short *)W.code, d_labels, n, d_xlab,
                           (const unsigned *)W.aggR, (const unsigned *)W.aggE, ntt, (const unsigned *)TP.grp, S.grp[!odd], ctx->tile_groups_max,
                           d_last_id, id_base, d_xlab ? 1 : 0, S.flags, hw.w, hw.seq);
    } else {
        hipLaunchKernelGGL(dbt_scan, dim3(1), dim3(1024), 0, st, W.aggR, W.aggE, ntt, d_boff, nb, n, (const unsigned *)W.brun,
                           (const unsigned *)W.bext, W.runbase, W.extbase, d_last_id, mode, S.flags, hw.w, hw.seq);
        hipLaunchKernelGGL(dbt_finish, dim3((n + 1023) / 1024), dim3(256), 0, st, (const unsigned short *)W.code, d_labels, n, (const unsigned *)W.aggR,
                           (const unsigned *)W.aggE, d_boff, nb, (const unsigned *)W.runbase, (const unsigned *)W.extbase);
    }
    TDT_CHECK_LAUNCH();
    unsigned too_large = 0;
    rc = db_word_wait(ctx, hw, &too_large);
    *stands = too_large == 0;
    return rc;
}

// ---- what one tdt_dbscan_device call works on: its arguments, the arrays of slot 3, and whether the bucket offsets are uploaded yet
struct DbCall {
    tdt_ctx *ctx;
    const unsigned *x, *y;
    int n;
    const int64_t *bucket_off;
    int nb;
    unsigned long long eps;
    int m, mode;
    double *labels;
    long long *last_id;
    DbWork w;
    bool staged;                     // db_stage_buckets has run
    int blocks1() const { return n ? (n + DB_THREADS - 1) / DB_THREADS : 1; }            // a thread per point
    int blocks_nb() const { return (std::max(n, nb) + DB_THREADS - 1) / DB_THREADS; }    // ... or per bucket, whichever are more
};

// bucket offsets to the device, staged through pinned memory so that the copy is truly asynchronous; run bases and counters zeroed.
// (Not needed by the one-bucket tile-resident pass, which therefore never waits for the stream.)
static int db_stage_buckets(DbCall &c) {
    if (c.staged) return TDT_OK;
    c.staged = true;
    hipStream_t st = c.ctx->stream;
    const size_t bytes = (size_t)(c.nb + 1) * 4;
    void *h_stage = nullptr;
    const int rc = tdt_pinned(c.ctx, 0, bytes + 64, &h_stage);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(st));  // previous call may still be reading the pinned block
    int *h_boff = (int *)h_stage;
    for (int b = 0; b <= c.nb; b++) h_boff[b] = (int)c.bucket_off[b];
    TDT_HIP(hipMemcpyAsync(c.w.boff, h_boff, bytes, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemsetAsync(c.w.runbase, 0, bytes, st));
    TDT_HIP(hipMemsetAsync(c.w.cnt, 0, 256, st));
    return TDT_OK;
}

// the x-only result from the x labels of route 2 or 3 (n_labelled = 0: an empty input, every bucket reports cluster_id -1)
static int db_x_result(const DbCall &c, int n_labelled) {
    hipLaunchKernelGGL(dbx_final, dim3(c.blocks_nb()), dim3(DB_THREADS), 0, c.ctx->stream, (const int *)c.w.xlab, n_labelled, (const int *)c.w.boff,
                       c.nb, (const unsigned *)c.w.runbase, c.labels, c.last_id);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

// y-sort of the clusters larger than DB_SMALL (runs only when dby_rank flagged any)
static int db_sort_large(const DbCall &c) {
    tdt_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    const DbWork &w = c.w;
    const int n = c.n;
    int rc = tdt_scan_u32_inclusive(ctx, w.lflag, n, w.tsum);
    if (rc) return rc;
    unsigned nl = 0;
    TDT_HIP(hipMemcpyAsync(&nl, w.lflag + (n - 1), 4, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    if (!nl) return TDT_OK;
    hipLaunchKernelGGL(dby_large_compact, dim3(c.blocks1()), dim3(DB_THREADS), 0, st, (const int *)w.xlab, c.y, n, (const unsigned *)w.lflag, w.key, w.v0,
                       w.cpos);
    TDT_CHECK_LAUNCH();
    unsigned long long *ks = nullptr;
    unsigned *vs = nullptr;
    // y: all 32 bits; cluster id < number of runs <= n
    rc = tdt_radix_sort_pairs(ctx, w.key, w.v0, w.ksorted, w.v1, nl, tdt_sort_mask(1ull << 32, (uint64_t)n + 1), &ks, &vs);
    if (rc) return rc;
    hipLaunchKernelGGL(dby_large_scatter, dim3((nl + DB_THREADS - 1) / DB_THREADS), dim3(DB_THREADS), 0, st, (const unsigned long long *)ks,
                       (const unsigned *)vs, (const unsigned *)w.cpos, (int)nl, w.ys, w.ord);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

// ---- route 2: ballot-mask tiles (tdt_dbscan_fused.h), cross-tile prefixes from a one-workgroup scan between launches.  Takes what
// route 1 does not: an x-cluster of more than DB_SMALL members, n >= 0x7fff0000.
static int db_route_masks(const DbCall &c) {
    tdt_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    const DbWork &w = c.w;
    const int n = c.n, nb = c.nb, m = c.m;
    const int ntf = (n + DBF_TILE - 1) / DBF_TILE;
    const dim3 grid(ntf), block(DBF_THREADS);
    DbfWork F;
    int rc = tdt_scratch_layout(ctx, 8, F, ntf);
    if (rc) return rc;
    // (the control word and the three guard words of the mask arrays are zeroed by tile 0 of dbm_x_masks)
    if (nb == 1 && m <= 4)
        hipLaunchKernelGGL(dbm_x_masks<true>, grid, block, 0, st, c.x, n, (const int *)w.boff, nb, c.eps, m, F.PM, F.agg_x, F.PY, F.ctl);
    else
        hipLaunchKernelGGL(dbm_x_masks<false>, grid, block, 0, st, c.x, n, (const int *)w.boff, nb, c.eps, m, F.PM, F.agg_x, F.PY, F.ctl);
    if (ntf > DBM_INLINE_PREFIX_MAX) hipLaunchKernelGGL(tile_scan, dim3(1), dim3(1024), 0, st, F.agg_x, ntf);
    hipLaunchKernelGGL(dbm_x_labels, grid, block, 0, st, (const ull *)F.PM, (const ull *)F.agg_x, n, (const int *)w.boff, nb, m, w.xlab, w.runbase,
                       w.seg0, w.seg1);
    TDT_CHECK_LAUNCH();
    if (c.mode == 1) return db_x_result(c, n);
    hipLaunchKernelGGL(dby_rank, dim3(c.blocks1()), dim3(DB_THREADS), 0, st, (const int *)w.xlab, c.y, n, (const int *)w.seg0, (const int *)w.seg1,
                       w.ys, w.ord, w.lflag, &F.ctl->nlarge);
    TDT_CHECK_LAUNCH();
    // The y pass is enqueued right away on the assumption that no x-cluster exceeded DB_SMALL members (the
    // usual case), so the GPU never idles on a mid-pipeline readback; the counter is checked afterwards
    // and only then are the large clusters sorted and the y pass repeated.
    for (int attempt = 0; attempt < 2; attempt++) {
        hipLaunchKernelGGL(dbm_y_masks, grid, block, 0, st, (const int *)w.xlab, (const unsigned *)w.ys, n, (const int *)w.boff, nb, c.eps, m, F.PY,
                           F.HM, F.BM, F.agg_1);
        if (ntf > DBM_INLINE_PREFIX_MAX) hipLaunchKernelGGL(tile_scan, dim3(1), dim3(1024), 0, st, F.agg_1, ntf);
        hipLaunchKernelGGL(dbm_y_mid, grid, block, 0, st, (const ull *)F.PY, (const ull *)F.HM, (const ull *)F.BM, (const ull *)F.agg_1, n, m, F.EM,
                           F.S1M, F.FM, F.agg_2);
        if (ntf > DBM_INLINE_PREFIX_MAX) hipLaunchKernelGGL(tile_scan, dim3(1), dim3(1024), 0, st, F.agg_2, ntf);
        hipLaunchKernelGGL(dbm_y_final, grid, block, 0, st, (const int *)w.xlab, (const unsigned *)w.ord, (const ull *)F.BM, (const ull *)F.EM,
                           (const ull *)F.S1M, (const ull *)F.FM, (const ull *)F.agg_2, n, (const int *)w.boff, nb, (const unsigned *)w.runbase,
                           c.labels, c.last_id);
        TDT_CHECK_LAUNCH();
        if (attempt == 1) break;
        DbHostWord hw;
        rc = db_word_arm(ctx, &hw);
        if (rc) return rc;
        hipLaunchKernelGGL(db_signal_host, dim3(1), dim3(1), 0, st, (const unsigned *)&F.ctl->nlarge, hw.w, hw.seq);
        TDT_CHECK_LAUNCH();
        unsigned nlarge = 0;
        rc = db_word_wait(ctx, hw, &nlarge);
        if (rc) return rc;
        if (!nlarge) break;
        rc = db_sort_large(c);
        if (rc) return rc;
    }
    if (c.last_id && nb > 1)
        hipLaunchKernelGGL(dbf_empty_buckets, dim3((nb + 255) / 256), dim3(256), 0, st, (const int *)w.boff, nb, c.last_id);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

// ---- route 3: m > DBF_M_MAX — byte flags, a launch per step, three global scans
static int db_route_scans(const DbCall &c) {
    tdt_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    const DbWork &w = c.w;
    const int n = c.n, nb = c.nb, m = c.m;
    const dim3 grid1(c.blocks1()), grid4((n + DB_TILE - 1) / DB_TILE), block(DB_THREADS);
    hipLaunchKernelGGL(dbx_flags, grid4, block, 0, st, c.x, n, (const int *)w.boff, nb, c.eps, m, w.px, w.sx);
    TDT_CHECK_LAUNCH();
    int rc = tdt_scan_u32_inclusive(ctx, w.sx, n, w.tsum);
    if (rc) return rc;
    hipLaunchKernelGGL(dbx_labels, grid1, block, 0, st, (const unsigned char *)w.px, (const unsigned *)w.sx, n, m, (const int *)w.boff, nb, w.xlab,
                       w.runbase);
    TDT_CHECK_LAUNCH();
    if (c.mode == 1) return db_x_result(c, n);
    hipLaunchKernelGGL(db_segments, grid1, block, 0, st, (const int *)w.xlab, n, w.seg0, w.seg1);
    hipLaunchKernelGGL(dby_rank, grid1, block, 0, st, (const int *)w.xlab, c.y, n, (const int *)w.seg0, (const int *)w.seg1, w.ys, w.ord, w.lflag,
                       w.cnt);
    TDT_CHECK_LAUNCH();
    // x-clusters larger than DB_SMALL: one 4-byte readback decides whether the radix sort runs
    unsigned nlarge = 0;
    TDT_HIP(hipMemcpyAsync(&nlarge, w.cnt, 4, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    if (nlarge) {
        rc = db_sort_large(c);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(dby_flags, grid1, block, 0, st, (const int *)w.xlab, n, (const int *)w.seg0, (const int *)w.seg1, (const unsigned *)w.ys, c.eps,
                       m, w.py, w.sy);
    TDT_CHECK_LAUNCH();
    rc = tdt_scan_u32_inclusive(ctx, w.sy, n, w.tsum);
    if (rc) return rc;
    hipLaunchKernelGGL(dby_extras, grid1, block, 0, st, (const int *)w.xlab, n, (const int *)w.seg0, (const int *)w.seg1, (const unsigned *)w.sy,
                       w.ex);
    TDT_CHECK_LAUNCH();
    rc = tdt_scan_u32_inclusive(ctx, w.ex, n, w.tsum);
    if (rc) return rc;
    hipLaunchKernelGGL(dby_final, dim3(c.blocks_nb()), block, 0, st, (const int *)w.xlab, n, m, (const int *)w.seg0, (const unsigned char *)w.py,
                       (const unsigned *)w.sy, (const unsigned *)w.ex, (const unsigned *)w.ord, (const int *)w.boff, nb,
                       (const unsigned *)w.runbase, c.labels, c.last_id);
    TDT_CHECK_LAUNCH();
    return TDT_OK;
}

// validation, the empty input, and the dispatch: route 1 where it applies — and stands —, else route 2, or route 3 for m > DBF_M_MAX
extern "C" int tdt_dbscan_device(tdt_ctx *ctx, const uint32_t *d_x, const uint32_t *d_y, size_t n_, const int64_t *bucket_off,
                                 int nb, uint64_t eps, int m, int mode, double *d_labels, int64_t *d_last_id) {
    if (!ctx || nb < 1 || !bucket_off || m < 2 || (mode != 0 && mode != 1)) {
        tdt_set_error("tdt_dbscan_device: bad argument (m must be >= 2: the reference's max() of an empty window raises)");
        return TDT_E_ARG;
    }
    if (n_ >= 0x7fffffffull) {
        tdt_set_error("tdt_dbscan_device: n too large");
        return TDT_E_UNSUPPORTED;
    }
    const int n = (int)n_;
    if (bucket_off[0] != 0 || bucket_off[nb] != (int64_t)n) {
        tdt_set_error("tdt_dbscan_device: bucket_off must start at 0 and end at n");
        return TDT_E_ARG;
    }
    for (int b = 0; b < nb; b++)
        if (bucket_off[b + 1] < bucket_off[b]) {
            tdt_set_error("tdt_dbscan_device: bucket_off must be non-decreasing");
            return TDT_E_ARG;
        }
    TDT_HIP(hipSetDevice(ctx->device));
    DbCall c{ctx, d_x, d_y, n, bucket_off, nb, eps, m, mode, d_labels, (long long *)d_last_id, {}, false};
    int rc = tdt_scratch_layout(ctx, 3, c.w, n, nb);
    if (rc) return rc;
    if (n == 0) {
        rc = db_stage_buckets(c);
        return rc ? rc : db_x_result(c, 0);
    }
    const bool fused = m <= DBF_M_MAX;
    if (fused && n < 0x7fff0000) {
        if (nb > 1) {
            rc = db_stage_buckets(c);
            if (rc) return rc;
        }
        bool stands = false;
        rc = db_tile_pass(ctx, d_x, d_y, n, c.w.boff, nb, eps, m, mode, nullptr, 0ll, d_labels, c.last_id, &stands);
        if (rc || stands) return rc;
    }
    rc = db_stage_buckets(c);
    if (rc) return rc;
    return fused ? db_route_masks(c) : db_route_scans(c);
}

// ---- what the host entries of int64 columns share: device coordinates are uint32 offsets from the column minimum
static void db_column_range(const int64_t *col, size_t n, size_t stride, int64_t *lo, int64_t *hi) {
    *lo = *hi = col[0];
    for (size_t i = 0; i < n; i++) {
        *lo = std::min(*lo, col[i * stride]);
        *hi = std::max(*hi, col[i * stride]);
    }
}

// two 32-bit columns of n values, fill(i, a, b) giving row i, through pinned block 1 to the head of scratch slot 5 (dev_bytes in all)
template <class F>
static int db_stage_columns(tdt_ctx *ctx, size_t n, size_t dev_bytes, F &&fill, uint32_t **d0, uint32_t **d1) {
    void *h = nullptr, *d = nullptr;
    int rc = tdt_pinned(ctx, 1, n * 8 + 64, &h);
    if (rc) return rc;
    rc = tdt_scratch(ctx, 5, dev_bytes, &d);
    if (rc) return rc;
    uint32_t *h0 = (uint32_t *)h, *h1 = h0 + n;
    for (size_t i = 0; i < n; i++) fill(i, h0[i], h1[i]);
    *d0 = (uint32_t *)d;
    *d1 = *d0 + n;
    TDT_HIP(hipMemcpyAsync(d, h, n * 8, hipMemcpyHostToDevice, ctx->stream));
    return TDT_OK;
}

// the labels and the last id, home once the stream is done
static int db_result_home(tdt_ctx *ctx, const double *d_labels, size_t n, const void *d_last, double *labels, int64_t *last_id) {
    long long lid = -1;
    TDT_HIP(hipStreamSynchronize(ctx->stream));
    TDT_HIP(hipMemcpy(labels, d_labels, n * 8, hipMemcpyDeviceToHost));
    TDT_HIP(hipMemcpy(&lid, d_last, 8, hipMemcpyDeviceToHost));
    if (last_id) *last_id = lid;
    return TDT_OK;
}

extern "C" int tdt_dbscan(tdt_ctx *ctx, const int64_t *data, size_t n, size_t stride, double eps, int m, int mode,
                          double *labels, int64_t *last_id) {
    if (!ctx || (n && (!data || !labels)) || stride < 1 || (mode == 0 && stride < 2)) {
        tdt_set_error("tdt_dbscan: bad argument");
        return TDT_E_ARG;
    }
    if (m < 2) {
        tdt_set_error("tdt_dbscan: m must be >= 2 (the reference raises ValueError: max() arg is an empty sequence)");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    if (n == 0) {
        if (last_id) *last_id = -1;
        return TDT_OK;
    }
    int64_t xmin, xmax, ymin = 0, ymax = 0;
    db_column_range(data, n, stride, &xmin, &xmax);
    if (stride >= 2) db_column_range(data + 1, n, stride, &ymin, &ymax);
    int rc = tdt_check_span("tdt_dbscan", xmin, xmax);
    if (!rc) rc = tdt_check_span("tdt_dbscan", ymin, ymax);
    if (rc) return rc;
    uint32_t *dx = nullptr, *dy = nullptr;
    rc = db_stage_columns(ctx, n, n * 16 + 64, [&](size_t i, uint32_t &a, uint32_t &b) {
        a = (uint32_t)(data[i * stride] - xmin);
        b = stride >= 2 ? (uint32_t)(data[i * stride + 1] - ymin) : 0u;
    }, &dx, &dy);
    if (rc) return rc;
    const int64_t boff[2] = {0, (int64_t)n};
    void *dlast = nullptr;
    rc = tdt_scratch(ctx, 6, n * 8 + 64, &dlast);
    if (rc) return rc;
    double *dl = (double *)dlast;
    int64_t *dlid = (int64_t *)((char *)dlast + n * 8);
    rc = tdt_dbscan_device(ctx, dx, dy, n, boff, 1, tdt_eps_u64(eps), m, mode, dl, dlid);
    if (rc) return rc;
    return db_result_home(ctx, dl, n, dlid, labels, last_id);
}

// ---- y pass on caller-supplied x labels (DBSCAN.y_coordinate_clustering, DBSCAN.py:66-123) -------------------------------------
// d_xlab: int32 labels, -1 = unlabelled, every label value one contiguous index range, values ascending along the array (what
// x_coordinate_clustering returns, for any eps / m).  Sub-run 1 of a cluster keeps its label, extra sub-runs get cluster_id + 1,
// cluster_id + 2, ... in cluster order; *d_last_id = the final cluster_id.  *too_large != 0: a cluster has more than DB_SMALL
// members (or m > 64) — the labels were NOT produced; the caller takes another route.
extern "C" int tdt_dbscan_y_device(tdt_ctx *ctx, const int32_t *d_xlab, const uint32_t *d_y, size_t n_, uint64_t eps, int m, int64_t cluster_id,
                                   double *d_labels, int64_t *d_last_id, int *too_large) {
    if (!ctx || !too_large || m < 2 || (n_ && (!d_xlab || !d_y || !d_labels))) {
        tdt_set_error("tdt_dbscan_y_device: bad argument");
        return TDT_E_ARG;
    }
    *too_large = 0;
    if (n_ >= 0x7fff0000ull || m > DBF_M_MAX) {
        *too_large = 1;
        return TDT_OK;
    }
    if (n_ == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(ctx->device));
    bool stands = false;
    const int rc = db_tile_pass(ctx, nullptr, d_y, (int)n_, nullptr, 1, eps, m, 0, d_xlab, (long long)cluster_id, d_labels, (long long *)d_last_id,
                                &stands);
    if (rc) return rc;
    if (!stands) *too_large = 1;
    return TDT_OK;
}

extern "C" int tdt_dbscan_y(tdt_ctx *ctx, const int64_t *data, size_t n, size_t stride, double eps, int m, int64_t cluster_id, double *labels,
                            int64_t *last_id) {
    if (!ctx || stride < 2 || (n && (!data || !labels))) {
        tdt_set_error("tdt_dbscan_y: bad argument");
        return TDT_E_ARG;
    }
    if (m < 2) {
        tdt_set_error("tdt_dbscan_y: m must be >= 2");
        return TDT_E_ARG;
    }
    if (last_id) *last_id = cluster_id;
    if (n == 0) return TDT_OK;
    if (n >= 0x7fff0000ull) {
        tdt_set_error("tdt_dbscan_y: n too large");
        return TDT_E_UNSUPPORTED;
    }
    TDT_HIP(hipSetDevice(ctx->device));
    // the labels this path takes: integers >= -1, every value one contiguous range, 0, 1, 2, ... along the array (the reference visits
    // `set(clusters)` — ascending for such values — and selects members by value; other label arrays are not reproduced here)
    long long next = 0, cur = -2;
    for (size_t i = 0; i < n; i++) {
        const double v = labels[i];
        const long long l = (long long)v;
        if ((double)l != v || l < -1 || l > 0x7ffffff0ll) {
            tdt_set_error("tdt_dbscan_y: label %g at %zu is not an integer in [-1, 2^31)", v, i);
            return TDT_E_UNSUPPORTED;
        }
        if (l == cur) continue;
        if (l >= 0) {
            if (l != next) {
                tdt_set_error("tdt_dbscan_y: labels must number contiguous clusters 0, 1, 2, ... along the array (label %lld at %zu, expected %lld)", l, i, next);
                return TDT_E_UNSUPPORTED;
            }
            next++;
        }
        cur = l;
    }
    if (cluster_id < next - 1) {
        // extra sub-runs would be numbered cluster_id + k <= the largest label: the reference's later `clusters == cluster` masks pick
        // them up again (DBSCAN.py:72,115) — not the closed form of this path
        tdt_set_error("tdt_dbscan_y: cluster_id %lld is below the largest label %lld (ids would collide with clusters not visited yet)",
                      (long long)cluster_id, next - 1);
        return TDT_E_UNSUPPORTED;
    }
    int64_t ymin, ymax;
    db_column_range(data + 1, n, stride, &ymin, &ymax);
    int rc = tdt_check_span("tdt_dbscan_y", ymin, ymax);
    if (rc) return rc;
    // slot 5: the y column and the labels as int32, then the float64 labels of the result
    uint32_t *dy = nullptr, *dl = nullptr;
    rc = db_stage_columns(ctx, n, n * 16 + 256, [&](size_t i, uint32_t &a, uint32_t &b) {
        a = (uint32_t)(data[i * stride + 1] - ymin);
        b = (uint32_t)(int32_t)labels[i];
    }, &dy, &dl);
    if (rc) return rc;
    double *dlab = (double *)((char *)dy + ((n * 8 + 255) & ~(size_t)255));
    void *dlast = nullptr;
    rc = tdt_scratch(ctx, 6, 64, &dlast);
    if (rc) return rc;
    int large = 0;
    rc = tdt_dbscan_y_device(ctx, (const int32_t *)dl, dy, n, tdt_eps_u64(eps), m, cluster_id, dlab, (int64_t *)dlast, &large);
    if (rc) return rc;
    if (large) {
        tdt_set_error("tdt_dbscan_y: an x-cluster has more than %d members (or m > %d): not on the caller-supplied-labels path", DB_SMALL, DBF_M_MAX);
        return TDT_E_UNSUPPORTED;
    }
    return db_result_home(ctx, dlab, n, dlast, labels, last_id);
}

// -------------------------------------------------------------------- sort + cluster in one call
__global__ __launch_bounds__(DB_THREADS) void sd_make_keys(const unsigned *__restrict__ x, int n, const int *__restrict__ boff, int nb,
                                                           unsigned long long *__restrict__ key, unsigned *__restrict__ val) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    const int w0 = i & ~63;                                        // the wave's 64 consecutive positions
    if (i >= n) return;
    key[i] = ((unsigned long long)(unsigned)db_bucket_wave(boff, nb, w0, min(w0 + 63, n - 1), i) << 32) | x[i];   // stable sort => ties keep signal order
    val[i] = (unsigned)i;
}

__global__ __launch_bounds__(DB_THREADS) void sd_unpack(const unsigned long long *__restrict__ ksorted, const unsigned *__restrict__ vsorted,
                                                        const unsigned *__restrict__ y, int n, unsigned *__restrict__ xs,
                                                        unsigned *__restrict__ ysrt, unsigned *__restrict__ perm) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned src = vsorted[i];
    xs[i] = (unsigned)ksorted[i];
    ysrt[i] = y[src];
    perm[i] = src;
}

// labels on the wire: -1 or an id below 2^31, so 4 bytes each cross PCIe and the host widens them again (exact)
__global__ __launch_bounds__(DB_THREADS) void sd_labels_i32(const double *__restrict__ lab, int n, int *__restrict__ out) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i < n) out[i] = (int)lab[i];
}

// ---- what the two sort-then-cluster entries (tdt_sort_dbscan_ex, tdt_cluster_columns) share
// the argument checks; *empty: no signals — every bucket reports no runs and cluster_id -1, and the call is done
static int sc_check(const char *who, bool pointers_ok, size_t n, const int64_t *bucket_off, int nb, int m, int64_t *runs_out, int64_t *last_out,
                    bool *empty) {
    if (!pointers_ok || nb < 1 || !bucket_off) {
        tdt_set_error("%s: bad argument", who);
        return TDT_E_ARG;
    }
    if (m < 2) {
        tdt_set_error("%s: m must be >= 2", who);
        return TDT_E_ARG;
    }
    if (n >= 0x7fffffffull || bucket_off[0] != 0 || bucket_off[nb] != (int64_t)n) {
        tdt_set_error("%s: bad bucket offsets / n", who);
        return TDT_E_ARG;
    }
    *empty = n == 0;
    for (int b = 0; *empty && b < nb; b++) {
        if (runs_out) runs_out[b] = 0;
        if (last_out) last_out[b] = -1;
    }
    return TDT_OK;
}

// slot 5 of the two entries: the two columns as they arrive, the sorted columns, the sort's pairs, `aux` (the order, or the int32
// labels in signal order), the float64 labels, the bucket offsets and, where asked for, per bucket the x pass's and the full pass's
// last id.  (The last 256 bytes are slack these requests have always had.)
struct ScWork {
    unsigned *in0, *in1, *xs, *ys, *v0, *v1, *aux;
    unsigned long long *k0, *k1;
    double *lab;
    int *boff;
    long long *cnt;
    size_t lay(void *base, size_t n, int nb, bool counts) {
        tdt_carver c(base);
        in0 = c.take<unsigned>(n), in1 = c.take<unsigned>(n), xs = c.take<unsigned>(n), ys = c.take<unsigned>(n);
        v0 = c.take<unsigned>(n), v1 = c.take<unsigned>(n), aux = c.take<unsigned>(n);
        k0 = c.take<unsigned long long>(n), k1 = c.take<unsigned long long>(n);
        lab = c.take<double>(n);
        boff = c.take<int>((size_t)nb + 1);
        cnt = counts ? c.take<long long>((size_t)nb * 2 + 8) : nullptr;
        c.take<char>(256);
        return c.size;
    }
};

// [0, n) cut into nth ranges, fn(t, i0, i1) on a host thread each (the caller's own takes the first)
static int sc_host_threads(size_t n, size_t grain) {
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)tdt_host_thread_count(), n / grain + 1));
}
template <class F>
static void sc_host_ranges(size_t n, int nth, F &&fn) {
    std::vector<std::thread> th;
    for (int t = 1; t < nth; t++) th.emplace_back([&fn, n, nth, t] { fn(t, n * (size_t)t / nth, n * (size_t)(t + 1) / nth); });
    fn(0, 0, n / nth);
    for (auto &x : th) x.join();
}

// cluster the sorted columns.  d_cnt (null: the caller wants neither) gets per bucket the last id of the x pass alone — run only
// where `runs` are wanted: its cluster_id is the number of x-runs - 1 (DBSCAN.py:33-64) — and behind them the last ids of the full pass
static int sc_cluster_sorted(tdt_ctx *ctx, const unsigned *d_xs, const unsigned *d_ys, size_t n, const int64_t *bucket_off, int nb, double eps, int m,
                             bool runs, double *d_lab, long long *d_cnt) {
    if (runs) {
        const int rc = tdt_dbscan_device(ctx, d_xs, d_ys, n, bucket_off, nb, tdt_eps_u64(eps), m, 1, d_lab, (int64_t *)d_cnt);
        if (rc) return rc;
    }
    return tdt_dbscan_device(ctx, d_xs, d_ys, n, bucket_off, nb, tdt_eps_u64(eps), m, 0, d_lab, d_cnt ? (int64_t *)(d_cnt + nb) : nullptr);
}

// the counts' way home: their copy is enqueued (sc_counts_fetch), and once the stream has been waited for they go to the caller
static int sc_counts_fetch(tdt_ctx *ctx, const long long *d_cnt, int nb, std::vector<long long> &hc) {
    hc.assign((size_t)nb * 2, 0);
    if (d_cnt) TDT_HIP(hipMemcpyAsync(hc.data(), d_cnt, (size_t)nb * 16, hipMemcpyDeviceToHost, ctx->stream));
    return TDT_OK;
}
static void sc_counts_report(const std::vector<long long> &hc, int nb, int64_t *runs_out, int64_t *last_out) {
    for (int b = 0; b < nb; b++) {
        if (runs_out) runs_out[b] = hc[b] + 1;
        if (last_out) last_out[b] = hc[nb + b];
    }
}

extern "C" int tdt_sort_dbscan(tdt_ctx *ctx, const int64_t *posA, const int64_t *posB, size_t n, const int64_t *bucket_off, int nb,
                               double eps, int m, uint32_t *perm_out, double *labels_out) {
    return tdt_sort_dbscan_ex(ctx, posA, posB, n, bucket_off, nb, eps, m, perm_out, labels_out, nullptr, nullptr);
}

// the same call, also reporting per bucket the number of x-runs (DBSCAN.py:33-64: the x pass's cluster_id + 1) and the final
// cluster_id of DBSCAN.main — what a caller that cut one bucket into pieces needs to re-base the pieces' ids (dist.py)
extern "C" int tdt_sort_dbscan_ex(tdt_ctx *ctx, const int64_t *posA, const int64_t *posB, size_t n, const int64_t *bucket_off, int nb,
                                  double eps, int m, uint32_t *perm_out, double *labels_out, int64_t *runs_out, int64_t *last_out) {
    bool empty = false;
    int rc = sc_check("tdt_sort_dbscan", ctx && (!n || (posA && posB && perm_out && labels_out)), n, bucket_off, nb, m, runs_out, last_out, &empty);
    if (rc || empty) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    // column ranges and the 32-bit offsets: host passes over n elements, spread over the host threads
    const int nth = sc_host_threads(n, 1u << 16);
    std::vector<int64_t> lo_a(nth), hi_a(nth), lo_b(nth), hi_b(nth);
    sc_host_ranges(n, nth, [&](int t, size_t i0, size_t i1) {
        int64_t a0 = posA[0], a1 = posA[0], b0 = posB[0], b1 = posB[0];
        for (size_t i = i0; i < i1; i++) {
            a0 = std::min(a0, posA[i]);
            a1 = std::max(a1, posA[i]);
            b0 = std::min(b0, posB[i]);
            b1 = std::max(b1, posB[i]);
        }
        lo_a[t] = a0; hi_a[t] = a1; lo_b[t] = b0; hi_b[t] = b1;
    });
    const int64_t amin = *std::min_element(lo_a.begin(), lo_a.end()), amax = *std::max_element(hi_a.begin(), hi_a.end());
    const int64_t bmin = *std::min_element(lo_b.begin(), lo_b.end()), bmax = *std::max_element(hi_b.begin(), hi_b.end());
    rc = tdt_check_span("tdt_sort_dbscan", amin, amax);
    if (!rc) rc = tdt_check_span("tdt_sort_dbscan", bmin, bmax);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    void *h = nullptr;
    const size_t hb = n * 12 + (size_t)(nb + 1) * 4 + 64;     // in: two 32-bit columns; out: labels (8 B) + order (4 B) per signal
    rc = tdt_pinned(ctx, 1, hb, &h);
    if (rc) return rc;
    ScWork W;                                                 // aux: the order
    rc = tdt_scratch_layout(ctx, 5, W, n, nb, false);
    if (rc) return rc;
    uint32_t *hx = (uint32_t *)h, *hy = hx + n;
    int *hboff = (int *)((char *)h + n * 12);
    sc_host_ranges(n, nth, [&](int, size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            hx[i] = (uint32_t)(posA[i] - amin);
            hy[i] = (uint32_t)(posB[i] - bmin);
        }
    });
    for (int b = 0; b <= nb; b++) hboff[b] = (int)bucket_off[b];
    TDT_HIP(hipMemcpyAsync(W.in0, hx, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(W.in1, hy, n * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(W.boff, hboff, (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, st));
    const int blocks = ((int)n + DB_THREADS - 1) / DB_THREADS;
    hipLaunchKernelGGL(sd_make_keys, dim3(blocks), dim3(DB_THREADS), 0, st, (const unsigned *)W.in0, (int)n, (const int *)W.boff, nb, W.k0, W.v0);
    TDT_CHECK_LAUNCH();
    // only the digits that can differ are sorted: the posA span and the bucket index
    unsigned long long *ks = nullptr;
    unsigned *vs = nullptr;
    rc = tdt_radix_sort_pairs(ctx, W.k0, W.v0, W.k1, W.v1, n, tdt_sort_mask((uint64_t)(amax - amin) + 1, (uint64_t)nb), &ks, &vs);
    if (rc) return rc;
    hipLaunchKernelGGL(sd_unpack, dim3(blocks), dim3(DB_THREADS), 0, st, (const unsigned long long *)ks, (const unsigned *)vs,
                       (const unsigned *)W.in1, (int)n, W.xs, W.ys, W.aux);
    TDT_CHECK_LAUNCH();
    long long *dcnt = nullptr;
    if (runs_out || last_out) {
        void *dc = nullptr;
        rc = tdt_scratch(ctx, 6, (size_t)nb * 16 + 64, &dc);
        if (rc) return rc;
        dcnt = (long long *)dc;
    }
    rc = sc_cluster_sorted(ctx, W.xs, W.ys, n, bucket_off, nb, eps, m, runs_out != nullptr, W.lab, dcnt);
    if (rc) return rc;
    // results come back through the pinned block (its input columns are consumed by now), labels as int32 (v0 is free again), then go
    // to the caller's arrays on the host threads
    int *dlab32 = (int *)W.v0;
    hipLaunchKernelGGL(sd_labels_i32, dim3(blocks), dim3(DB_THREADS), 0, st, (const double *)W.lab, (int)n, dlab32);
    TDT_CHECK_LAUNCH();
    int *hlab = (int *)h;
    uint32_t *hperm = (uint32_t *)((char *)h + n * 4);
    std::vector<long long> hc;
    TDT_HIP(hipMemcpyAsync(hlab, dlab32, n * 4, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipMemcpyAsync(hperm, W.aux, n * 4, hipMemcpyDeviceToHost, st));
    rc = sc_counts_fetch(ctx, dcnt, nb, hc);
    if (rc) return rc;
    TDT_HIP(hipStreamSynchronize(st));
    sc_counts_report(hc, nb, runs_out, last_out);
    sc_host_ranges(n, nth, [&](int, size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) labels_out[i] = (double)hlab[i];
        memcpy(perm_out + i0, hperm + i0, (i1 - i0) * 4);
    });
    return TDT_OK;
}

// ---- the same, without host passes: 32-bit columns in (straight from the parsed signal tables), int32 labels in SIGNAL order out.
// Keys are (bucket << 32 | posA biased to unsigned); only the digits that can differ are sorted (max_pos bounds posA, e.g. the longest
// contig).  The posB column travels on the copy stream while the posA digits are being sorted; labels are scattered back to signal
// order on the device, so 4 B/signal return.  Pinned caller memory (tdt_host_alloc) is read and written by DMA directly; pageable
// memory goes through the context's pinned block.
__global__ __launch_bounds__(DB_THREADS) void sc_make_keys(const int *__restrict__ a, int n, const int *__restrict__ boff, int nb,
                                                           unsigned long long *__restrict__ key, unsigned *__restrict__ val) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    const int w0 = i & ~63;                                        // the wave's 64 consecutive positions
    if (i >= n) return;
    key[i] = ((unsigned long long)(unsigned)db_bucket_wave(boff, nb, w0, min(w0 + 63, n - 1), i) << 32) | ((unsigned)a[i] ^ 0x80000000u);   // order of signed values
    val[i] = (unsigned)i;
}

__global__ __launch_bounds__(DB_THREADS) void sc_unpack(const unsigned long long *__restrict__ ksorted, const unsigned *__restrict__ vsorted,
                                                        const int *__restrict__ b, int n, unsigned *__restrict__ xs, unsigned *__restrict__ ysrt) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    xs[i] = (unsigned)ksorted[i];
    ysrt[i] = (unsigned)b[vsorted[i]] ^ 0x80000000u;
}

__global__ __launch_bounds__(DB_THREADS) void sc_scatter_labels(const double *__restrict__ lab, const unsigned *__restrict__ perm, int n,
                                                                int *__restrict__ out) {
    const int i = blockIdx.x * DB_THREADS + threadIdx.x;
    if (i < n) out[perm[i]] = (int)lab[i];
}

static bool sc_is_pinned(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

extern "C" int tdt_cluster_columns(tdt_ctx *ctx, const int32_t *posA, const int32_t *posB, size_t n, const int64_t *bucket_off, int nb,
                                   double eps, int m, int64_t max_pos, int32_t *labels_by_signal, int64_t *runs_out, int64_t *last_out) {
    bool empty = false;
    int rc = sc_check("tdt_cluster_columns", ctx && (!n || (posA && posB && labels_by_signal)), n, bucket_off, nb, m, runs_out, last_out, &empty);
    if (rc || empty) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream, cs = ctx->copy_stream;
    static const bool cc_timing = getenv("TIDDIT_CC_TIMING") != nullptr;          // host clock at the call's seams, to stderr
    double tm[12];
    int ntm = 0;
    auto mark = [&]() {
        if (cc_timing && ntm < 12) tm[ntm++] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
    };
    mark();
    ScWork W;                                                 // aux: the int32 labels in signal order
    rc = tdt_scratch_layout(ctx, 5, W, n, nb, true);
    if (rc) return rc;
    const int *da = (const int *)W.in0, *db = (const int *)W.in1;
    long long *dcnt = (runs_out || last_out) ? W.cnt : nullptr;
    // staging only for pageable caller memory
    mark();
    const bool pin_in = sc_is_pinned(posA) && sc_is_pinned(posB), pin_out = sc_is_pinned(labels_by_signal);
    mark();
    void *h = nullptr;
    rc = tdt_pinned(ctx, 1, n * 8 + (size_t)(nb + 1) * 4 + 64, &h);
    if (rc) return rc;
    int *hboff = (int *)((char *)h + n * 8);
    TDT_HIP(hipStreamSynchronize(st));                       // an earlier call may still be using the pinned block / the scratch
    mark();
    for (int b = 0; b <= nb; b++) hboff[b] = (int)bucket_off[b];
    const int32_t *srcA = posA, *srcB = posB;
    if (!pin_in) {
        sc_host_ranges(n, sc_host_threads(n, 1u << 18), [&](int, size_t i0, size_t i1) {
            memcpy((int *)h + i0, posA + i0, (i1 - i0) * 4);
            memcpy((int *)h + n + i0, posB + i0, (i1 - i0) * 4);
        });
        srcA = (const int32_t *)h;
        srcB = (const int32_t *)h + n;
    }
    TDT_HIP(hipMemcpyAsync(W.boff, hboff, (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(W.in0, srcA, n * 4, hipMemcpyHostToDevice, st));
    // posB rides along with the sort of the posA digits — but only once posA has crossed: two copies in the same direction share the
    // link, and the sort waits for posA alone (started together both took 0.70 ms per 20 MB; in sequence posA is there after 0.36)
    TDT_HIP(hipEventRecord(ctx->ev[2], st));
    TDT_HIP(hipStreamWaitEvent(cs, ctx->ev[2], 0));
    TDT_HIP(hipMemcpyAsync(W.in1, srcB, n * 4, hipMemcpyHostToDevice, cs));
    TDT_HIP(hipEventRecord(ctx->ev[3], cs));
    mark();
    const int blocks = ((int)n + DB_THREADS - 1) / DB_THREADS;
    hipLaunchKernelGGL(sc_make_keys, dim3(blocks), dim3(DB_THREADS), 0, st, da, (int)n, (const int *)W.boff, nb, W.k0, W.v0);
    TDT_CHECK_LAUNCH();
    // biased keys: non-negative positions are 0x80000000 + pos, so the top bit is constant and only the digits of the bound's span
    // differ; no bound given: all 32 bits (negative values included)
    const uint64_t span = max_pos <= 0 ? 1ull << 32 : max_pos < 0x7fffffffll ? (uint64_t)max_pos + 1 : 0x80000000ull;
    unsigned long long *ks = nullptr;
    unsigned *vs = nullptr;
    rc = tdt_radix_sort_pairs(ctx, W.k0, W.v0, W.k1, W.v1, n, tdt_sort_mask(span, (uint64_t)nb), &ks, &vs);
    if (rc) return rc;
    mark();
    TDT_HIP(hipStreamWaitEvent(st, ctx->ev[3], 0));
    hipLaunchKernelGGL(sc_unpack, dim3(blocks), dim3(DB_THREADS), 0, st, (const unsigned long long *)ks, (const unsigned *)vs, db, (int)n, W.xs, W.ys);
    TDT_CHECK_LAUNCH();
    rc = sc_cluster_sorted(ctx, W.xs, W.ys, n, bucket_off, nb, eps, m, runs_out != nullptr, W.lab, dcnt);
    if (rc) return rc;
    mark();
    int *dlab32 = (int *)W.aux;
    hipLaunchKernelGGL(sc_scatter_labels, dim3(blocks), dim3(DB_THREADS), 0, st, (const double *)W.lab, (const unsigned *)vs, (int)n, dlab32);
    TDT_CHECK_LAUNCH();
    int *dst = pin_out ? labels_by_signal : (int *)h;
    TDT_HIP(hipMemcpyAsync(dst, dlab32, n * 4, hipMemcpyDeviceToHost, st));
    std::vector<long long> hc;
    rc = sc_counts_fetch(ctx, dcnt, nb, hc);
    if (rc) return rc;
    mark();
    TDT_HIP(hipStreamSynchronize(st));
    mark();
    if (!pin_out) memcpy(labels_by_signal, h, n * 4);
    sc_counts_report(hc, nb, runs_out, last_out);
    if (cc_timing) {
        fprintf(stderr, "tdt_cluster_columns n=%zu nb=%d us:", n, nb);
        for (int i = 1; i < ntm; i++) fprintf(stderr, " %.0f", tm[i] - tm[i - 1]);
        fprintf(stderr, "  (scratch | pinned? | pinned block + sync | copies issued | keys + sort issued | unpack + clustering | scatter + D2H issued | wait)\n");
    }
    return TDT_OK;
}

// pinned host memory for callers that build their columns in place (numpy arrays over it: tiddit_amd/hostutil.py)
extern "C" int tdt_host_alloc(size_t bytes, void **out) {
    if (!out) return TDT_E_ARG;
    *out = nullptr;
    if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        tdt_set_error("tdt_host_alloc: pinned allocation of %zu bytes failed", bytes);
        return TDT_E_NOMEM;
    }
    return TDT_OK;
}
extern "C" int tdt_host_free(void *p) {
    if (p) (void)hipHostFree(p);
    return TDT_OK;
}
