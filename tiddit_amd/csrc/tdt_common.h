// Internal shared definitions for libtiddit_hip.so (gfx950 only; no portability layer).
#pragma once
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/tiddit_hip.h"

#define TDT_WAVE 64

void tdt_set_error(const char *fmt, ...);

#define TDT_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            tdt_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return TDT_E_HIP;                                                                 \
        }                                                                                     \
    } while (0)

#define TDT_CHECK_LAUNCH() TDT_HIP(hipGetLastError())

// Grow-only device / pinned-host scratch buffers owned by a context.
struct tdt_buf {
    void *p = nullptr;
    size_t cap = 0;
};

enum { TDT_NSCRATCH = 30, TDT_NPINNED = 4 };

struct tdt_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;    // stream in use (own_stream or an adopted one)
    hipStream_t copy_stream = nullptr;
    hipStream_t back_stream = nullptr;   // device-to-host copies that must not queue behind the launch stream's next kernels (tdt_signal_scan_result)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int num_cu = 256;
    tdt_buf scratch[TDT_NSCRATCH];
    tdt_buf pinned[TDT_NPINNED];
    int *d_async_err = nullptr;  // device word kernels OR into (bounded-spin timeouts); checked by tdt_ctx_sync
    unsigned tile_calls = 0;             // clustering: parity selects one of two group-sum arrays
    int tile_groups_max = 0;             // ... and how many of their entries have ever been used
    void *tile_flags_zeroed = nullptr;   // clustering: the status block that has been zeroed once (its users re-zero it themselves)
    // tdt_signal_scan -> tdt_signal_scan_result: what the last scan of THIS context selected (pointers into its scratch slots)
    size_t scan_n_sel = 0, scan_raw_bytes = 0;
    void *scan_meta = nullptr, *scan_size = nullptr, *scan_bytes = nullptr;
};

// Device allocations of the library outside the ingest's own buffers: hipMalloc, and where that fails once more after the ingest's
// buffer cache (tdt_ingest.hip) has gone back to the driver — the cache must never be what makes another allocator fail.
hipError_t tdt_dev_malloc(void **p, size_t bytes);
size_t tdt_dev_cache_flush(int device);      // device < 0: every device; returns the bytes released (callers hold no cached pointer)
size_t tdt_dev_cache_held(int device);
int tdt_scratch(tdt_ctx *ctx, int slot, size_t bytes, void **out);
int tdt_pinned(tdt_ctx *ctx, int slot, size_t bytes, void **out);

static inline int tdt_ceil_log2_u64(uint64_t v) {
    int l = 0;
    while ((1ull << l) < v) l++;
    return l;
}

// ---- one description of a workspace serves its size AND its pointers.  A layout is a struct of pointers with a
// `size_t lay(void *base, ...)` that takes its arrays from a tdt_carver in order and returns the carver's size: run on a null base it
// only measures, run on the allocation it hands the pointers out (tdt_scratch_layout does both), so the two cannot disagree.
struct tdt_carver {
    char *base;
    size_t size = 0;
    explicit tdt_carver(void *b) : base((char *)b) {}
    template <class T> T *take(size_t count) {             // `count` elements of T, starting on a 256-byte boundary
        T *r = base ? (T *)(base + size) : nullptr;
        size += (count * sizeof(T) + 255) & ~(size_t)255;
        return r;
    }
};
template <class L, class... A> static inline int tdt_scratch_layout(tdt_ctx *ctx, int slot, L &l, A... a) {
    void *base = nullptr;
    const int rc = tdt_scratch(ctx, slot, l.lay(nullptr, a...), &base);
    if (rc == TDT_OK) l.lay(base, a...);
    return rc;
}

// ---- internal entry points used across translation units
// tdt_sort.hip.  Stable sort of n (u64 key, u32 value) pairs by the key bits set in `bitmask`.  PRECONDITION: the key bits outside the
// mask are equal in all keys (callers pass tdt_sort_mask of what can differ) — and the sort relies on it: when no mask bit lies above
// bit 31 and more than one digit is sorted (narrow mode), the keys travel as 32-bit words between the first and the last digit and the
// high word of every output key is rebuilt from keys[0].  keys/vals and the *_tmp buffers ping-pong; where the result lies comes back
// through out_keys / out_vals.
int tdt_radix_sort_pairs(tdt_ctx *ctx, unsigned long long *keys, unsigned *vals, unsigned long long *keys_tmp, unsigned *vals_tmp,
                         size_t n, unsigned long long bitmask, unsigned long long **out_keys, unsigned **out_vals);
// the bits that can differ among keys `hi << 32 | lo` with lo < lo_values <= 2^32 and hi < hi_values <= 2^31
static inline unsigned long long tdt_sort_mask(uint64_t lo_values, uint64_t hi_values) {
    return ((1ull << tdt_ceil_log2_u64(lo_values)) - 1ull) | (((1ull << tdt_ceil_log2_u64(hi_values)) - 1ull) << 32);
}
// tdt_dbscan.hip.  In-place inclusive scan of d_v[0..n); d_tsum: ceil(n / 1024) words of scratch.
int tdt_scan_u32_inclusive(tdt_ctx *ctx, unsigned *d_v, int n, unsigned *d_tsum);
// tdt_region.hip.  The evidence store: every placed record of the scan as int4 {start, end, mate_pos, bits}, in file order.
struct tdt_evstore {
    tdt_ctx *ctx;
    int n_contigs;
    int min_q;
    long long max_ins;
    int4 *rec;
    size_t n, cap;
    int *d_span;      // per contig: max(end - start) over its records (atomicMax in the pack kernel)
    double junction_ms = 0;   // tdt_junction.hip: the device time of the last junction_support launch over this store
};
// every row {offset, n, max span, tid, contig length} of a contig table lies inside the store, else TDT_E_RANGE naming `fn`
int tdt_evstore_check_rows(const char *fn, const tdt_evstore *s, const int64_t *contigs, int n_contigs);

// ---- what every clustering entry of host int64 columns applies: device coordinates are uint32 offsets from the column minimum
static inline int tdt_check_span(const char *who, int64_t lo, int64_t hi) {
    if ((unsigned __int128)((__int128)hi - lo) <= 0xfffffffeull) return TDT_OK;
    tdt_set_error("%s: coordinate span >= 2^32 is outside the device path's domain", who);
    return TDT_E_UNSUPPORTED;
}
// ... and eps as the integer bound of the window test.  numpy: int64 distance < python number  <=>  d < ceil(eps) for integer d >= 0
static inline uint64_t tdt_eps_u64(double eps) {
    if (!(eps > 0)) return 0;  // also NaN: nothing is ever < NaN
    return eps >= 8589934592.0 ? 1ull << 33 : (uint64_t)ceil(eps);
}

#include "tdt_cov_record.h"      // the 8-byte coverage records (packed / binned): their own header, so that the profiles know when they changed

// ---- BGZF block table shared by the host scan (tdt_bgzf.hip), the device inflate (tdt_inflate.hip) and the ingest (tdt_ingest.hip)
struct BzDesc {
    unsigned long long in_off, out_off;   // payload offset in the compressed buffer, block offset in the output
    unsigned in_len, isize, crc, pad;
};
// tdt_split_fields (tdt_format.hip) / the signal tables (tdt_sigtab.hip)
struct TdtSplitOut {
    int32_t status;        // 0: SA mapQ below min_q (no row, :40-41), 1: fields valid, 2: not handled here
    int32_t read_start, read_end;      // reference_start + 1, reference_end + 1 of the read (:60-61)
    int32_t split_pos, sa_split;       // before the swap (:62-116)
    int32_t seg_start, seg_end;        // the SA segment's reference_start (the tag's POS, stored raw, :13) and reference_end
    uint32_t chr_off, chr_len;         // the SA contig name inside raw
    uint8_t is_reverse, sa_minus, pad[2];
};
void tdt_split_one(const uint8_t *meta, const uint32_t *raw_end, const uint8_t *raw, size_t raw_len, uint32_t r, int min_q, TdtSplitOut &o);

int tdt_host_thread_count();
int tdt_bz_hop(const uint8_t *p, size_t avail, size_t *bsize, size_t *pay_off, size_t *pay_len, uint32_t *isize);
int tdt_bz_block_table(const uint8_t *comp, size_t len, std::vector<BzDesc> &blocks, size_t *produced);
int tdt_bz_launch(tdt_ctx *ctx, const unsigned char *d_comp, const BzDesc *d_blocks, size_t nblocks, unsigned char *d_out, bool check_crc,
                  unsigned *d_status, unsigned *d_summary);
int tdt_bz_launch_on(tdt_ctx *ctx, hipStream_t st, int reserve, const unsigned char *d_comp, const BzDesc *d_blocks, size_t nblocks,
                     unsigned char *d_out, bool check_crc, unsigned *d_status, unsigned *d_summary);
const char *tdt_bz_err_name(unsigned e);
