// Per-contig depth distributions from the evidence store (TIDDIT_DEPTH_DIST, tiddit_depth_dist.py), gfx950: for every contig the number
// of bases at depth exactly d (d < DD_CAP), at DD_CAP or more, the sum of all depths, the maximum and the minimum depth — per BASE,
// which the 50-bp coverage bins cannot give.  The depth of base b of a contig of LN bases is the number of its records with
//   bits & (TDT_EV_UNMAPPED | TDT_EV_DUPLICATE | TDT_EV_LOW_Q) == 0   and   start <= b < min(end, LN)
// (the store's `end` is the exclusive reference end, so this is the half-open interval the scan's own coverage adds).
//
// ONE launch covers all contigs.  A workgroup owns one tile [lo, hi) of DD_TILE bases of one contig row:
//   1. the records that can reach the tile have start in [lo - max_span, hi): two 64-ary searches on the sorted starts (tdt_search.h);
//   2. every kept record that overlaps the tile adds +1 at max(start, lo) - lo and -1 at min(end, LN, hi) - lo of a difference array
//      in LDS (a read that reaches the tile's end needs no -1);
//   3. the prefix sum of the difference array is the depth of every base: each wavefront owns a quarter of the tile, the quarters'
//      totals (one pass of plain sums, one barrier) are the carries, then each wavefront scans its quarter 64 bases at a time;
//   4. depth is constant between two records' ends, so a wavefront books a whole RUN of equal depths with one LDS atomic (a ballot
//      finds the run heads) into the histogram of min(depth, DD_CAP); sum, max and min stay in registers;
//   5. the non-zero histogram entries and the sum go to the contig's global row by 64-bit atomic adds, max and min by atomic max / min.
// A tile that no record can reach is DD_TILE bases of depth 0: one atomic add, no LDS.
//
// LDS: DD_TILE * 4 bytes of differences + (DD_CAP + 1) * 4 of histogram = 36.1 KB with DD_TILE 8192 — four workgroups of a CU's
// 160 KB, so that two are resident with room to spare whatever else runs beside them; a tile twice as long would halve the searches
// per base and leave room for two only.
#include "tdt_common.h"
#include "tdt_search.h"

#define DD_CAP 1000                // depths DD_CAP and above share the last bin
#define DD_TILE 8192               // bases per workgroup
#define DD_THREADS 256
#define DD_WAVES (DD_THREADS / 64)
#define DD_QUARTER (DD_TILE / DD_WAVES)      // bases one wavefront scans
#define DD_ROW (DD_CAP + 4)                  // hist[0 .. DD_CAP], sum, max, min

typedef unsigned long long ull;

// rows of zeros; the minimum starts at the largest value where a tile will lower it (a contig of no bases keeps 0)
__global__ __launch_bounds__(256) void depth_dist_init(const long long *__restrict__ ctab, int n_contigs, ull *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_contigs * DD_ROW) return;
    const size_t c = i / DD_ROW, k = i % DD_ROW;
    out[i] = (k == DD_CAP + 3 && ctab[5 * c + 4] > 0) ? 0x7fffffffffffffffull : 0ull;
}

// tile_first[c] = the first tile of contig row c in the grid, tile_first[n_contigs] = the grid
__global__ __launch_bounds__(DD_THREADS) void depth_dist_tiles(const int4 *__restrict__ rec, const long long *__restrict__ ctab,
                                                               const long long *__restrict__ tile_first, int n_contigs,
                                                               ull *__restrict__ out) {
    __shared__ int diff[DD_TILE];
    __shared__ unsigned hist[DD_CAP + 1];
    __shared__ int wave_sum[DD_WAVES];
    __shared__ ull s_sum;
    __shared__ int s_max, s_min;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int c = 0;                                             // the last row with tile_first[c] <= blockIdx.x (uniform; rows of no bases own no tile)
    for (int b = n_contigs; b - c > 1;) {
        const int m = (c + b) >> 1;
        if (tile_first[m] <= (long long)blockIdx.x) c = m; else b = m;
    }
    const long long *C = ctab + 5 * (size_t)c;            // (offset, n, max span, tid, length)
    const int4 *__restrict__ R = rec + C[0];
    const int n = (int)C[1];
    const long long LN = C[4];
    const long long lo = ((long long)blockIdx.x - tile_first[c]) * DD_TILE;
    const long long hi = lo + DD_TILE < LN ? lo + DD_TILE : LN;
    ull *row = out + (size_t)c * DD_ROW;
    int i0, i1;                                            // every wavefront searches for itself: the probes are the same cache lines
    rg_lower_bound2<4>(reinterpret_cast<const int32_t *>(R), n, lo - C[2], hi, lane, i0, i1);
    if (i1 <= i0) {                                        // (uniform) nothing can reach the tile: hi - lo bases of depth 0
        if (tid == 0) {
            atomicAdd(row, (ull)(hi - lo));
            atomicMin(row + DD_CAP + 3, 0ull);
        }
        return;
    }
    for (int i = tid; i < DD_TILE; i += DD_THREADS) diff[i] = 0;
    for (int i = tid; i <= DD_CAP; i += DD_THREADS) hist[i] = 0;
    if (tid == 0) {
        s_sum = 0;
        s_max = 0;
        s_min = 0x7fffffff;
    }
    __syncthreads();
    for (int i = i0 + tid; i < i1; i += DD_THREADS) {
        const int4 r = R[i];
        const bool keep = !((unsigned)r.w & (TDT_EV_UNMAPPED | TDT_EV_DUPLICATE | TDT_EV_LOW_Q));
        const long long e = (long long)r.y < LN ? (long long)r.y : LN;
        const long long a = (long long)r.x > lo ? (long long)r.x : lo, b = e < hi ? e : hi;
        if (keep && a < b) {                               // lo <= a < b <= hi: both indices lie inside the tile
            atomicAdd(&diff[a - lo], 1);
            if (b < hi) atomicAdd(&diff[b - lo], -1);
        }
    }
    __syncthreads();
    const int q0 = wave * DD_QUARTER;
    int part = 0;
    for (int k = lane; k < DD_QUARTER; k += 64) part += diff[q0 + k];
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d);
    if (lane == 0) wave_sum[wave] = part;
    __syncthreads();
    int carry = 0;                                         // the depth at the last base before this wavefront's quarter
    for (int w = 0; w < wave; w++) carry += wave_sum[w];
    const int len = (int)(hi - lo);
    ull sum = 0;
    int mx = 0, mn = 0x7fffffff;
    for (int k = q0; k < q0 + DD_QUARTER && k < len; k += 64) {       // (uniform per wavefront)
        int v = diff[k + lane];
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        const int depth = carry + v;
        carry = __shfl(depth, 63);
        const int nv = len - k < 64 ? len - k : 64;        // the lanes that are bases of the tile (a prefix of the wavefront)
        const bool valid = lane < nv;
        const int prev = __shfl_up(depth, 1);
        const ull heads = __ballot(valid && (lane == 0 || depth != prev));
        if (valid) {
            sum += (ull)depth;
            mx = depth > mx ? depth : mx;
            mn = depth < mn ? depth : mn;
            if ((heads >> lane) & 1ull) {                  // the first base of a run of equal depths books the whole run
                const ull rest = lane == 63 ? 0ull : heads >> (lane + 1);
                const int next = rest ? lane + 1 + (__ffsll((long long)rest) - 1) : nv;
                atomicAdd(&hist[depth < DD_CAP ? depth : DD_CAP], (unsigned)(next - lane));
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d);
        mx = max(mx, __shfl_xor(mx, d));
        mn = min(mn, __shfl_xor(mn, d));
    }
    if (lane == 0) {
        atomicAdd(&s_sum, sum);
        atomicMax(&s_max, mx);
        atomicMin(&s_min, mn);
    }
    __syncthreads();
    for (int i = tid; i <= DD_CAP; i += DD_THREADS) {
        const unsigned h = hist[i];
        if (h) atomicAdd(row + i, (ull)h);
    }
    if (tid == 0) {
        if (s_sum) atomicAdd(row + DD_CAP + 1, s_sum);
        atomicMax(row + DD_CAP + 2, (ull)s_max);
        atomicMin(row + DD_CAP + 3, (ull)s_min);
    }
}

extern "C" int tdt_depth_dist(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, int cap, int64_t *out) {
    if (!ctx || !s || n_contigs < 0 || (n_contigs && (!contigs || !out))) {
        tdt_set_error("tdt_depth_dist: bad argument");
        return TDT_E_ARG;
    }
    if (cap != DD_CAP) {
        tdt_set_error("tdt_depth_dist: cap %d, the library was built with DD_CAP %d", cap, DD_CAP);
        return TDT_E_ARG;
    }
    int rc = tdt_evstore_check_rows("tdt_depth_dist", s, contigs, n_contigs);
    if (rc) return rc;
    if (n_contigs == 0) return TDT_OK;
    std::vector<long long> first((size_t)n_contigs + 1);
    long long tiles = 0;
    for (int c = 0; c < n_contigs; c++) {
        first[c] = tiles;
        const int64_t ln = contigs[5 * (size_t)c + 4];
        tiles += ln / DD_TILE + (ln % DD_TILE ? 1 : 0);
        if (tiles >= 0x7fffffffll) {
            tdt_set_error("tdt_depth_dist: the contigs up to row %d hold 2^31 - 1 tiles of %d bases or more", c, DD_TILE);
            return TDT_E_RANGE;
        }
    }
    first[n_contigs] = tiles;
    TDT_HIP(hipSetDevice(ctx->device));
    if (ctx != s->ctx) TDT_HIP(hipStreamSynchronize(s->ctx->stream));       // (the packs of another context's stream are complete)
    const size_t ct = ((size_t)n_contigs * 40 + 255) & ~(size_t)255, tf = (((size_t)n_contigs + 1) * 8 + 255) & ~(size_t)255;
    const size_t ob = (size_t)n_contigs * DD_ROW * 8;
    void *d = nullptr;
    rc = tdt_scratch(ctx, 28, ct + tf + ob, &d);
    if (rc) return rc;
    long long *dct = (long long *)d;
    long long *dtf = (long long *)((char *)d + ct);
    ull *dout = (ull *)((char *)d + ct + tf);
    hipStream_t st = ctx->stream;
    TDT_HIP(hipMemcpyAsync(dct, contigs, (size_t)n_contigs * 40, hipMemcpyHostToDevice, st));
    TDT_HIP(hipMemcpyAsync(dtf, first.data(), ((size_t)n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(depth_dist_init, dim3((unsigned)(((size_t)n_contigs * DD_ROW + 255) / 256)), dim3(256), 0, st, dct, n_contigs, dout);
    if (tiles)
        hipLaunchKernelGGL(depth_dist_tiles, dim3((unsigned)tiles), dim3(DD_THREADS), 0, st, s->rec, dct, dtf, n_contigs, dout);
    TDT_CHECK_LAUNCH();
    TDT_HIP(hipMemcpyAsync(out, dout, ob, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));          // (also: `first` and the caller's table are host memory the copies above read)
    return TDT_OK;
}
