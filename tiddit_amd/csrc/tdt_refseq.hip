// The reference sequence, resident in HBM (tdt_refseq.h has the layout): what a reference-aware kernel of the --sv scan reads — the first
// one is indel_keys<true>, the left-normalisation of TIDDIT_INDELS_NORM.
//   * ref_pack — ONE launch per contig, on the contig's bytes exactly as FastaFile.fetch_raw returns them (line ends in place, LF or
//     CRLF): base b sits at byte tdt_fasta_map::byte_of(b), the mapping gc_fasta_bins uses.  Lane = 16 consecutive bases = ONE 64-bit
//     store; a workgroup packs REF_TILE bases.  A lane divides once (the line of its first base) and then walks the bytes, stepping over
//     a line end where its column runs out.  Letters map to BAM's 4-bit codes in either case, every other byte to 15 (N), through a
//     256-byte table staged in LDS; the nibbles behind the contig's last base stay zero.
//   * the handle owns the store and the per-contig table (offset, length); the lengths are fixed at its creation, so the store is
//     allocated and zeroed ONCE and a load only writes its own contig's words — the guard bytes stay zero whatever is loaded beside them.
#include "tdt_refseq.h"
#include "tdt_fasta_map.h"

typedef unsigned long long ull;

#define REF_BLOCK 256
#define REF_TILE 4096                         // bases of a ref_pack workgroup: REF_BLOCK lanes, 16 bases each
#define REF_MAX_CONTIGS (1 << 24)

static_assert(REF_TILE == REF_BLOCK * 16, "a lane packs 16 bases");
static_assert(TDT_REF_GUARD % 8 == 0 && TDT_REF_GUARD >= 8, "contigs start on 8-byte boundaries behind their guard");

struct RefLut {
    uint8_t v[256];
};
static constexpr RefLut ref_make_lut() {
    RefLut t{};
    const char *codes = "=ACMGRSVTWYHKDBN";
    for (int i = 0; i < 256; i++) t.v[i] = 15;
    for (int c = 1; c < 16; c++) {
        t.v[(int)codes[c]] = (uint8_t)c;
        t.v[(int)codes[c] | 0x20] = (uint8_t)c;
    }
    return t;
}
__constant__ RefLut ref_lut = ref_make_lut();

__global__ __launch_bounds__(REF_BLOCK) void ref_pack(const uint8_t *__restrict__ raw, long long nbytes, unsigned len, tdt_fasta_map map,
                                                      ull *__restrict__ words, unsigned nwords) {
    __shared__ uint8_t s_lut[256];
    s_lut[threadIdx.x] = ref_lut.v[threadIdx.x];
    __syncthreads();
    const unsigned w = blockIdx.x * REF_BLOCK + threadIdx.x;
    if (w >= nwords) return;
    const unsigned b0 = w * 16u;                                   // (< len <= 2^31 - 1)
    const unsigned line = map.line_of(b0);
    unsigned col = b0 - line * map.linebases;
    long long at = (long long)line * map.linewidth + col;
    const unsigned todo = len - b0 < 16u ? len - b0 : 16u;
    ull v = 0;
    for (unsigned i = 0; i < todo; i++) {
        const unsigned code = at < nbytes ? s_lut[raw[at]] : 15u;   // (at < nbytes: the host checked that nbytes holds len bases)
        v |= (ull)code << (8u * (i >> 1) + ((i & 1u) ? 0u : 4u));  // (byte i / 2 of the word in memory, the even base in its high nibble)
        at++;
        if (++col == map.linebases) col = 0, at += map.linewidth - map.linebases;
    }
    words[w] = v;
}

static void refseq_free(tdt_refseq *h) {
    if (h->d_store) (void)hipFree(h->d_store);
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_len) (void)hipFree(h->d_len);
    delete h;
}

extern "C" int tdt_refseq_create(tdt_ctx *ctx, int n_contigs, const int64_t *lengths, tdt_refseq **out) {
    if (!ctx || !out || n_contigs < 0 || n_contigs > REF_MAX_CONTIGS || (n_contigs && !lengths)) {
        tdt_set_error("tdt_refseq_create: bad argument");
        return TDT_E_ARG;
    }
    for (int c = 0; c < n_contigs; c++)
        if (lengths[c] < 0 || lengths[c] >= (1ll << 31)) {
            tdt_set_error("tdt_refseq_create: contig %d has %lld bases (0 ... 2^31 - 1)", c, (long long)lengths[c]);
            return TDT_E_ARG;
        }
    TDT_HIP(hipSetDevice(ctx->device));
    tdt_refseq *h = new tdt_refseq{};
    h->ctx = ctx;
    h->n_contigs = n_contigs;
    h->off.resize((size_t)n_contigs), h->len.resize((size_t)n_contigs), h->loaded.assign((size_t)n_contigs, 0);
    size_t cur = TDT_REF_GUARD;
    for (int c = 0; c < n_contigs; c++) {
        h->off[c] = cur;
        h->len[c] = lengths[c];
        cur += (((size_t)lengths[c] + 15) / 16) * 8 + TDT_REF_GUARD;
    }
    h->bytes = cur;
    const size_t nt = n_contigs ? (size_t)n_contigs : 1;
    if (tdt_dev_malloc((void **)&h->d_store, h->bytes) != hipSuccess || tdt_dev_malloc((void **)&h->d_off, nt * 8) != hipSuccess ||
        tdt_dev_malloc((void **)&h->d_len, nt * 4) != hipSuccess) {
        const size_t bytes = h->bytes;
        refseq_free(h);
        tdt_set_error("tdt_refseq_create: out of device memory (%zu bytes)", bytes);
        return TDT_E_NOMEM;
    }
    hipError_t e = hipMemsetAsync(h->d_store, 0, h->bytes, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_len, 0xff, nt * 4, ctx->stream);                 // (-1: not loaded)
    if (e == hipSuccess && n_contigs) e = hipMemcpyAsync(h->d_off, h->off.data(), nt * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);                                   // (h->off is pageable host memory)
    if (e != hipSuccess) {
        refseq_free(h);
        TDT_HIP(e);
    }
    *out = h;
    return TDT_OK;
}

extern "C" int tdt_refseq_destroy(tdt_refseq *h) {
    if (!h) return TDT_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);        // (no kernel of the stream still reads the store)
    refseq_free(h);
    return TDT_OK;
}

// the checks both loads share; *m the layout's map
static int refseq_check_load(const char *fn, tdt_refseq *h, int tid, const void *raw, int64_t nbytes, int64_t length, int linebases, int linewidth,
                             tdt_fasta_map *m) {
    if (!h || nbytes < 0 || length < 0 || (length > 0 && !raw)) {
        tdt_set_error("%s: bad argument", fn);
        return TDT_E_ARG;
    }
    if (tid < 0 || tid >= h->n_contigs) {
        tdt_set_error("%s: contig %d is outside the table (%d contigs)", fn, tid, h->n_contigs);
        return TDT_E_ARG;
    }
    if (length != h->len[tid]) {
        tdt_set_error("%s: contig %d has %lld bases, the handle was made for %lld", fn, tid, (long long)length, h->len[tid]);
        return TDT_E_ARG;
    }
    if (h->loaded[tid]) {
        tdt_set_error("%s: contig %d is already loaded", fn, tid);
        return TDT_E_ARG;
    }
    m->linebases = m->linewidth = 1, m->magic = 0, m->shift = -1;
    if (length == 0) return TDT_OK;
    if (!tdt_fasta_layout_ok(length, linebases, linewidth)) {
        tdt_set_error("%s: unsupported layout (linebases %d, linewidth %d, len %lld)", fn, linebases, linewidth, (long long)length);
        return TDT_E_UNSUPPORTED;
    }
    if (nbytes < tdt_fasta_bytes(length, linebases, linewidth)) {
        tdt_set_error("%s: %lld bytes cannot hold %lld bases at %d/%d per line", fn, (long long)nbytes, (long long)length, linebases, linewidth);
        return TDT_E_ARG;
    }
    if (!tdt_fasta_map_make(linebases, linewidth, m)) {
        tdt_set_error("%s: line length %d has no 32-bit reciprocal", fn, linebases);
        return TDT_E_UNSUPPORTED;
    }
    return TDT_OK;
}

// the launch and the table entry behind it (all on the context's stream)
static int refseq_pack(tdt_refseq *h, int tid, const uint8_t *d_raw, int64_t nbytes, int64_t length, const tdt_fasta_map &m) {
    hipStream_t st = h->ctx->stream;
    const unsigned nwords = (unsigned)((length + 15) / 16);
    if (nwords) {
        hipLaunchKernelGGL(ref_pack, dim3((nwords + REF_BLOCK - 1) / REF_BLOCK), dim3(REF_BLOCK), 0, st, d_raw, (long long)nbytes, (unsigned)length, m,
                           reinterpret_cast<ull *>(h->d_store + h->off[tid]), nwords);
        TDT_CHECK_LAUNCH();
    }
    const int len32 = (int)length;
    TDT_HIP(hipMemcpyAsync(h->d_len + tid, &len32, 4, hipMemcpyHostToDevice, st));
    TDT_HIP(hipStreamSynchronize(st));                                                            // (len32 is a local; and the caller's bytes are free again)
    h->loaded[tid] = 1;
    return TDT_OK;
}

// One contig from caller-owned DEVICE bytes: `d_raw` = the contig's bytes exactly as in the file (nbytes of them, line ends included),
// `length` bases, `linebases` bases and `linewidth` bytes per full line (the .fai columns).  Returns when the contig is packed.
extern "C" int tdt_refseq_load_fasta_device(tdt_refseq *h, int tid, const uint8_t *d_raw, int64_t nbytes, int64_t length, int linebases, int linewidth) {
    tdt_fasta_map m;
    int rc = refseq_check_load("tdt_refseq_load_fasta_device", h, tid, d_raw, nbytes, length, linebases, linewidth, &m);
    if (rc) return rc;
    TDT_HIP(hipSetDevice(h->ctx->device));
    return refseq_pack(h, tid, d_raw, nbytes, length, m);
}

// The same from HOST bytes: uploaded into a staging buffer that is freed before the return.
extern "C" int tdt_refseq_load_fasta(tdt_refseq *h, int tid, const uint8_t *raw, int64_t nbytes, int64_t length, int linebases, int linewidth) {
    tdt_fasta_map m;
    int rc = refseq_check_load("tdt_refseq_load_fasta", h, tid, raw, nbytes, length, linebases, linewidth, &m);
    if (rc) return rc;
    TDT_HIP(hipSetDevice(h->ctx->device));
    void *d_raw = nullptr;
    if (length) {
        const size_t need = (size_t)tdt_fasta_bytes(length, linebases, linewidth);
        if (tdt_dev_malloc(&d_raw, need) != hipSuccess) {
            tdt_set_error("tdt_refseq_load_fasta: out of device memory (%zu bytes of staging)", need);
            return TDT_E_NOMEM;
        }
        const hipError_t e = hipMemcpyAsync(d_raw, raw, need, hipMemcpyHostToDevice, h->ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(d_raw);
            TDT_HIP(e);
        }
        nbytes = (int64_t)need;
    }
    rc = refseq_pack(h, tid, (const uint8_t *)d_raw, nbytes, length, m);
    if (d_raw) {
        (void)hipStreamSynchronize(h->ctx->stream);
        (void)hipFree(d_raw);
    }
    return rc;
}

// n codes of contig tid from base start on, one per output byte.  A fetch outside the contig, or of a contig that is not loaded:
// TDT_E_ARG, nothing written.
extern "C" int tdt_refseq_fetch(tdt_refseq *h, int tid, int64_t start, int64_t n, uint8_t *codes_out) {
    if (!h || n < 0 || start < 0 || (n > 0 && !codes_out)) {
        tdt_set_error("tdt_refseq_fetch: bad argument");
        return TDT_E_ARG;
    }
    if (tid < 0 || tid >= h->n_contigs || !h->loaded[tid] || start > h->len[tid] || n > h->len[tid] - start) {
        tdt_set_error("tdt_refseq_fetch: [%lld, %lld + %lld) of contig %d is outside what is loaded", (long long)start, (long long)start, (long long)n, tid);
        return TDT_E_ARG;
    }
    if (n == 0) return TDT_OK;
    TDT_HIP(hipSetDevice(h->ctx->device));
    const size_t b0 = (size_t)start / 2, b1 = (size_t)(start + n + 1) / 2;
    std::vector<uint8_t> packed(b1 - b0);
    TDT_HIP(hipMemcpyAsync(packed.data(), h->d_store + h->off[tid] + b0, b1 - b0, hipMemcpyDeviceToHost, h->ctx->stream));
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    for (int64_t i = 0; i < n; i++) {
        const size_t b = (size_t)(start + i);
        codes_out[i] = (packed[b / 2 - b0] >> ((b & 1) ? 0 : 4)) & 0xf;
    }
    return TDT_OK;
}

// For tests: the words of a contig that is NOT loaded yet (its own words only, never a guard byte) filled with `byte`, so that a load
// behind it shows that ref_pack writes every nibble of them, the ones behind the last base included.
extern "C" int tdt_debug_refseq_fill(tdt_refseq *h, int tid, int byte) {
    if (!h || tid < 0 || tid >= h->n_contigs || h->loaded[tid]) {
        tdt_set_error("tdt_debug_refseq_fill: bad argument");
        return TDT_E_ARG;
    }
    TDT_HIP(hipSetDevice(h->ctx->device));
    const size_t n = (size_t)((h->len[tid] + 15) / 16) * 8;
    if (n) TDT_HIP(hipMemsetAsync(h->d_store + h->off[tid], byte, n, h->ctx->stream));
    TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    return TDT_OK;
}

// The layout, for tests and tools: out[0] = the store's bytes, out[1] = TDT_REF_GUARD, out[2] = the bases of a ref_pack workgroup; and,
// where they are given, every contig's byte offset and the store itself (room for out[0] bytes).
extern "C" int tdt_refseq_layout(tdt_refseq *h, uint64_t *out3, uint64_t *offsets, uint8_t *store_out) {
    if (!h || !out3) {
        tdt_set_error("tdt_refseq_layout: bad argument");
        return TDT_E_ARG;
    }
    if (store_out) {
        TDT_HIP(hipSetDevice(h->ctx->device));
        TDT_HIP(hipMemcpyAsync(store_out, h->d_store, h->bytes, hipMemcpyDeviceToHost, h->ctx->stream));
        TDT_HIP(hipStreamSynchronize(h->ctx->stream));
    }
    out3[0] = h->bytes, out3[1] = TDT_REF_GUARD, out3[2] = REF_TILE;
    for (int c = 0; offsets && c < h->n_contigs; c++) offsets[c] = h->off[c];
    return TDT_OK;
}
