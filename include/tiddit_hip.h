/*
 * tiddit_hip.h — C ABI of libtiddit_hip.so, the MI355X (gfx950) implementation of TIDDIT's
 * signal-aggregation and clustering hot path.
 *
 * The reference (SciLifeLab/TIDDIT v3.9.5) has no FFI: its boundary for this path is the Python
 * module-function level.  Each entry point below names the reference interface
 * it replaces (file:line under tiddit/); the tiddit_amd python modules bind them with ctypes and re-exports the
 * reference's own function names/signatures (see INTEGRATION.md for the binding a maintainer adds).
 *
 * Conventions
 *   - plain C: opaque handles, pointers + sizes, no C++/torch types.
 *   - every function returns 0 (TDT_OK) or a negative TDT_E_* code; tdt_last_error() gives the
 *     message of the last failure on the calling thread.
 *   - `h_*` / unprefixed pointers are caller-owned HOST memory; `d_*` pointers are caller-owned
 *     DEVICE memory on the context's GPU.  Calls taking only d_* pointers are asynchronous on the
 *     context stream (tdt_ctx_stream); calls that return results to host memory synchronise.
 *   - coordinates are 0-based; `end` is exclusive (htslib bam_endpos / pysam reference_end).
 *   - there is NO CPU fallback: without a usable GPU tdt_ctx_create fails.
 */
#ifndef TIDDIT_HIP_H
#define TIDDIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDT_OK 0
#define TDT_E_ARG (-1)      /* bad argument (null pointer, bin_size <= 0, m < 2, ...)              */
#define TDT_E_HIP (-2)      /* a HIP runtime call failed (message in tdt_last_error)               */
#define TDT_E_RANGE (-3)    /* a read indexes a bin outside its contig (reference: IndexError)     */
#define TDT_E_INEXACT (-4)  /* a bin left the exact-arithmetic domain (|acc| >= 2^53)              */
#define TDT_E_NOMEM (-5)
#define TDT_E_UNSUPPORTED (-6) /* input outside the device path's domain (e.g. coordinate span >= 2^32) */
#define TDT_E_KEY (-7)      /* a name that is not in the table (reference: KeyError); tdt_last_error() = the name */

typedef struct tdt_ctx tdt_ctx;
typedef struct tdt_cov tdt_cov;

/* ---- context ------------------------------------------------------------------------------ */
int tdt_version(void);
/* The measurement macros the library was compiled with, space separated ("" = the product build).  Ablation builds (tools/build_variant.sh)
 * exist to price parts of a kernel and may compute wrong results; tiddit_amd._native refuses to load a library that reports any unless
 * TIDDIT_ALLOW_VARIANT=1. */
const char *tdt_build_flags(void);
const char *tdt_last_error(void);
int tdt_device_count(int *count);
int tdt_ctx_create(int device, tdt_ctx **out);
void tdt_ctx_destroy(tdt_ctx *ctx);
int tdt_ctx_sync(tdt_ctx *ctx);
/* The hipStream_t all asynchronous work of this context is enqueued on (as void*). */
void *tdt_ctx_stream(tdt_ctx *ctx);
/* Enqueue work on an externally owned hipStream_t (e.g. torch's current stream); 0 restores the
 * context's own stream. */
int tdt_ctx_set_stream(tdt_ctx *ctx, void *hip_stream);
/* Make the context's device the calling thread's current one: for a helper thread of the caller that pins host memory (tdt_host_alloc)
 * before it has called anything else of the library (bamio's file-reading thread). */
int tdt_ctx_bind_thread(tdt_ctx *ctx);

/* ---- binned read-depth histogram ---------------------------------------------------------- *
 * Replaces tiddit_coverage.create_coverage (tiddit_coverage.pyx:10-21), the per-read
 * update_coverage calls (tiddit_coverage.pyx:48-74) driven by __main__.py:229-242 (--cov) and
 * tiddit_signal.pyx:169-182 (--sv), including their read filter
 *     keep iff !(flag & 0x4) && !(flag & 0x400) && mapq >= min_q .
 * Bins are bit-identical to the reference's float64 arrays: every per-read contribution
 * float32(bases)/float32(den) is added as an exact 2^-S fixed-point int64 (S from tdt_cov_scale_bits). */
int tdt_cov_create(tdt_ctx *ctx, const int64_t *contig_len, int n_contigs, int bin_size, tdt_cov **out);
void tdt_cov_destroy(tdt_cov *cov);
/* bins = ceil(LN/bin_size); end_bin_size = LN - (bins-1)*bin_size      (tiddit_coverage.pyx:15-17) */
int tdt_cov_nbins(tdt_cov *cov, int tid, int64_t *nbins, int *end_bin_size);
int tdt_cov_scale_bits(tdt_cov *cov);
/* zero all accumulators (a fresh create_coverage) */
int tdt_cov_reset(tdt_cov *cov);
/* Add n alignment records of contig `tid`.  Host arrays are staged through pinned memory and copied
 * with hipMemcpyAsync (double-buffered), the kernel applies the read filter on device. */
int tdt_cov_push(tdt_cov *cov, int tid, const int32_t *start, const int32_t *end, const uint8_t *mapq,
                 const uint16_t *flag, size_t n, int min_q);
/* Same with device-resident arrays (asynchronous). */
int tdt_cov_push_device(tdt_cov *cov, int tid, const int32_t *d_start, const int32_t *d_end, const uint8_t *d_mapq,
                        const uint16_t *d_flag, size_t n, int min_q);
/* Several contigs' device-resident streams in ONE launch (no inter-launch gaps or tails): item i adds
 * n[i] records of contig tids[i]; the pointer arrays are HOST arrays of device pointers. */
int tdt_cov_push_device_multi(tdt_cov *cov, int n_items, const int *tids, const int32_t *const *d_start,
                              const int32_t *const *d_end, const uint8_t *const *d_mapq, const uint16_t *const *d_flag,
                              const size_t *n, int min_q);
/* The same with PACKED records — 8 bytes per read instead of 11: low word = reference_start (int32), high word =
 * span:24 | min(mapq,63):6 | unmapped(0x4):1 | duplicate(0x400):1, span = reference_end - reference_start (0xffffff: the true end
 * is read from d_end[i], which may otherwise be NULL).  This is the layout a producer that already sits on the device (the ingest
 * kernel) hands over; tdt_cov_pack_device converts the four arrays.  min_q > 63 is TDT_E_UNSUPPORTED here. */
int tdt_cov_pack_device(tdt_ctx *ctx, const int32_t *d_start, const int32_t *d_end, const uint8_t *d_mapq, const uint16_t *d_flag, size_t n,
                        uint64_t *d_packed);
int tdt_cov_push_packed_device_multi(tdt_cov *cov, int n_items, const int *tids, const uint64_t *const *d_packed, const int32_t *const *d_end,
                                     const size_t *n, int min_q);
/* BINNED records — 8 bytes per read, made for THIS histogram's bin size (2 <= bin_size < 1024, else TDT_E_UNSUPPORTED): low word =
 * first_bin << 2 | shape (0 one bin, 1 two bins [up to 256 for bins <= 128 bp], 2 replay literally, 3 invalid), high word = the filter
 * byte of the packed record | the two table indices bases_first_bin / bases_last_bin of tiddit_coverage.pyx:53-63 (csrc/tdt_common.h:
 * cov_bin_record).  The division, the bin split and the validity checks are done once when the record is written — by the ingest kernel
 * (tdt_ingest_bin_for) or by tdt_cov_pack_binned_device from the four arrays — and leave the accumulation launch.  d_start / d_end serve
 * the reads replayed literally (shape 2) and must be given. */
int tdt_cov_pack_binned_device(tdt_cov *cov, int tid, const int32_t *d_start, const int32_t *d_end, const uint8_t *d_mapq, const uint16_t *d_flag,
                               size_t n, uint64_t *d_binned);
int tdt_cov_push_binned_device_multi(tdt_cov *cov, int n_items, const int *tids, const uint64_t *const *d_binned, const int32_t *const *d_start,
                                     const int32_t *const *d_end, const size_t *n, int min_q);
/* All contigs at once: d_out holds tdt_cov_total_bins doubles, contig tid starts at tdt_cov_offset(tid)
 * (contigs are padded to 16-byte boundaries). */
int tdt_cov_total_bins(tdt_cov *cov, int64_t *total);
int tdt_cov_offset(tdt_cov *cov, int tid, int64_t *off);
int tdt_cov_finish_all_device(tdt_cov *cov, double *d_out);
/* the same into HOST memory: out = float64[tdt_cov_total_bins], contig t at out + tdt_cov_offset(t) — one launch, one copy, one wait for
 * a header of thousands of contigs (tiddit_coverage.pyx:10-21 creates one array per @SQ line) */
int tdt_cov_finish_all(tdt_cov *c, double *out);
/* Convert contig tid's accumulators to float64 bins (exact), copy to host / leave on device.
 * Returns TDT_E_RANGE / TDT_E_INEXACT if any pushed read / bin violated the domain. */
int tdt_cov_finish(tdt_cov *cov, int tid, double *out_bins);
int tdt_cov_finish_device(tdt_cov *cov, int tid, double *d_out_bins);
/* Number of reads that passed the filter so far (all contigs); synchronises. */
int tdt_cov_kept(tdt_cov *cov, int64_t *kept);

/* ---- binned GC / N-mask histogram ---------------------------------------------------------- *
 * Replaces tiddit_gc.binned_gc's per-character loop (tiddit_gc.pyx:14-31): out[bin] = -1 if
 * n/bin_size > n_cutoff else round_half_even(100*gc/chars); chars = bytes actually in the bin. */
int tdt_gc_bins(tdt_ctx *ctx, const uint8_t *seq, int64_t len, int bin_size, double n_cutoff, int8_t *out);
/* d_seq must be 16-byte aligned; asynchronous. */
int tdt_gc_bins_device(tdt_ctx *ctx, const uint8_t *d_seq, int64_t len, int bin_size, double n_cutoff, int8_t *d_out);
/* The same bins straight from the FASTA bytes of a contig, line ends still in place (what pysam.FastaFile.fetch hides,
 * tiddit_gc.pyx:14-19): raw = the nbytes the contig occupies in the file, len bases, linebases / linewidth as in the
 * .fai index.  TDT_E_UNSUPPORTED for layouts the kernel does not take (bins > 2048, contigs >= 2^31 bases, line ends
 * longer than two bytes): strip the line ends on the host and call tdt_gc_bins then. */
int tdt_gc_bins_fasta(tdt_ctx *ctx, const uint8_t *raw, int64_t nbytes, int64_t len, int linebases, int linewidth, int bin_size,
                      double n_cutoff, int8_t *out);
int tdt_gc_bins_fasta_device(tdt_ctx *ctx, const uint8_t *d_raw, int64_t nbytes, int64_t len, int linebases, int linewidth, int bin_size,
                             double n_cutoff, int8_t *d_out);
/* tiddit_gc.main's loop (tiddit_gc.pyx:35-42) over MANY contigs in one call: `raw` = the FASTA bytes of n contigs, contig i at raw_off[i]
 * (a multiple of 16) for raw_len[i] bytes, len[i] bases at linebases[i] / linewidth[i] per line; its int8 bins are written to
 * out + out_off[i].  One copy in, one launch per contig, one copy out, one wait (a GRCh38-shaped reference has 3 366 contigs). */
int tdt_gc_bins_fasta_many(tdt_ctx *ctx, const uint8_t *raw, int64_t nbytes, int n, const int64_t *raw_off, const int64_t *raw_len,
                           const int64_t *len, const int32_t *linebases, const int32_t *linewidth, int bin_size, double n_cutoff,
                           int8_t *out, const int64_t *out_off, int64_t out_bytes);

/* ---- signal clustering ("DBSCAN") ----------------------------------------------------------- *
 * Replaces DBSCAN.x_coordinate_clustering (DBSCAN.py:33-64), y_coordinate_clustering (:66-123) and
 * main (:125-129).  `data` is the reference's row-major int64 [n, stride] array (column 0 = posA,
 * column 1 = posB) in the order the caller would hand to DBSCAN.main; labels come back as float64
 * in that same order, exactly as the reference returns them.  eps is compared like numpy compares
 * an int64 distance with the Python number: d < eps.
 *   mode 0: main (x then y);  mode 1: x pass only.  *last_id receives the final cluster_id. */
int tdt_dbscan(tdt_ctx *ctx, const int64_t *data, size_t n, size_t stride, double eps, int m, int mode,
               double *labels, int64_t *last_id);
/* DBSCAN.y_coordinate_clustering(data, eps, m, cluster_id, clusters) (DBSCAN.py:66-123) on caller-supplied x labels: `labels` holds
 * them on entry (float64: -1 or the cluster numbers 0, 1, 2, ... — every number one contiguous range, ascending along the array, as
 * x_coordinate_clustering returns them for any eps / m) and the relabelled result on return; sub-run 1 of a cluster keeps its label,
 * extra sub-runs get cluster_id + 1, cluster_id + 2, ...; *last_id = the returned cluster_id.  TDT_E_UNSUPPORTED for label arrays of
 * another shape, for a cluster_id below the largest label (the ids produced would collide with clusters not visited yet), for
 * clusters above 128 members and for m > 64: tdt_dbscan_y_segments takes those. */
int tdt_dbscan_y(tdt_ctx *ctx, const int64_t *data, size_t n, size_t stride, double eps, int m, int64_t cluster_id, double *labels,
                 int64_t *last_id);
/* The same pass for ARBITRARY label arrays (the reference selects a cluster's members by value, DBSCAN.py:68-75: any size, any
 * values, not necessarily contiguous).  The caller lists the members of all clusters it wants visited: y[i] (posB), seg[i] = the
 * cluster's position in the visiting order (0 .. nseg-1; the reference's order is Python's set() iteration, which the Python
 * front end supplies), keep[i] = the member's current label.  out[i] = keep[i] for sub-run 1, cluster_id + (extra sub-runs of the
 * segments visited before) + s - 1 for sub-run s > 1, -1 otherwise; *last_id = the final cluster_id (:112-122).  The segments are
 * treated as independent, which is what the reference does as long as no produced id equals a value still to be visited; callers
 * replay one segment per call otherwise (tiddit_amd/DBSCAN.py). */
int tdt_dbscan_y_segments(tdt_ctx *ctx, const int64_t *y, const int32_t *seg, const double *keep, size_t n, int nseg, double eps, int m,
                          int64_t cluster_id, double *out, int64_t *last_id);
int tdt_dbscan_y_device(tdt_ctx *ctx, const int32_t *d_xlab, const uint32_t *d_y, size_t n, uint64_t eps, int m, int64_t cluster_id,
                        double *d_labels, int64_t *d_last_id, int *too_large);
/* Device-resident batch: nb independent buckets ((chrA,chrB) pairs), bucket b owning points
 * [bucket_off[b], bucket_off[b+1]) of d_x/d_y (uint32 coordinates, each bucket in DBSCAN.main input
 * order).  bucket_off is a HOST array of nb+1 offsets.  Labels (float64, ids restart per bucket)
 * are written to d_labels; per-bucket final cluster_id to d_last_id (int64[nb], may be NULL).
 * Asynchronous unless large x-clusters need the segmented sort (one 8-byte readback). */
int tdt_dbscan_device(tdt_ctx *ctx, const uint32_t *d_x, const uint32_t *d_y, size_t n, const int64_t *bucket_off,
                      int nb, uint64_t eps, int m, int mode, double *d_labels, int64_t *d_last_id);
/* tiddit_cluster.pyx:152-154 in one call: stable sort of each bucket by posA, then DBSCAN.main.
 * perm_out[i] = index (within the whole input) of the point at sorted position i. */
int tdt_sort_dbscan(tdt_ctx *ctx, const int64_t *posA, const int64_t *posB, size_t n, const int64_t *bucket_off, int nb,
                    double eps, int m, uint32_t *perm_out, double *labels_out);
/* The same call, also reporting per bucket the number of x-runs (x_coordinate_clustering's cluster_id + 1, DBSCAN.py:33-64) in
 * runs_out[nb] and DBSCAN.main's final cluster_id in last_out[nb] (either may be NULL): what a caller that cut ONE oversized
 * bucket into pieces at gaps >= eps needs to re-base the pieces' ids (DBSCAN.py:112-122 numbers extra sub-runs after ALL x-runs). */
int tdt_sort_dbscan_ex(tdt_ctx *ctx, const int64_t *posA, const int64_t *posB, size_t n, const int64_t *bucket_off, int nb,
                       double eps, int m, uint32_t *perm_out, double *labels_out, int64_t *runs_out, int64_t *last_out);
/* The same for 32-bit columns (alignment positions are below 2^31), without any host pass over the data: labels come back as int32 in
 * SIGNAL order (labels_by_signal[i] = cluster of the i-th input signal, -1 = noise), 4 bytes per signal over PCIe.  max_pos bounds posA
 * (e.g. the longest contig; <= 0: unknown) so that only the digits that can differ are sorted.  Columns and labels in pinned memory
 * (tdt_host_alloc) are moved by DMA directly; pageable memory is staged.  runs_out / last_out as in tdt_sort_dbscan_ex (may be NULL). */
int tdt_cluster_columns(tdt_ctx *ctx, const int32_t *posA, const int32_t *posB, size_t n, const int64_t *bucket_off, int nb, double eps, int m,
                        int64_t max_pos, int32_t *labels_by_signal, int64_t *runs_out, int64_t *last_out);
int tdt_host_alloc(size_t bytes, void **out);     /* pinned host memory */
int tdt_host_free(void *p);

/* ---- multi-GPU exchange (one process per GPU, RCCL over xGMI) ------------------------------------- *
 * The clustering path shards by (chrA,chrB) bucket (tiddit_cluster.pyx:140-154 keeps no cross-bucket state): every rank
 * clusters its buckets with tdt_dbscan_device / tdt_sort_dbscan and ONE variable-count all-gather of the label arrays gives
 * every rank the whole cluster set.  When one BAM is read as byte-range shards (tdt_ingest_push_bounded) every rank bins
 * its reads into a full-genome histogram and ONE sum all-reduce of the float64 bins finishes it — the bins are multiples of
 * 2^-S below 2^53, so the sum is exact and bit-identical to the single-GPU result.
 * tdt_comm_unique_id: rank 0 obtains the 128-byte RCCL id and hands it to the other ranks by whatever channel launched them
 * (MPI, a file, torch.distributed); tdt_comm_init is collective over the `world` ranks, each with its own context/GPU.
 * tdt_allgatherv: rank r contributes counts[r] elements of elem_bytes; they arrive at d_recv + displs[r]*elem_bytes on every
 * rank (counts/displs are HOST arrays, identical on all ranks; counts[rank] == send_count).  Both calls are asynchronous on the
 * context stream.  RCCL is bound at run time (an instance already in the process, e.g. PyTorch's, is reused). */
typedef struct tdt_comm tdt_comm;
int tdt_comm_unique_id(uint8_t *id128);
int tdt_comm_init(tdt_ctx *ctx, const uint8_t *id128, int rank, int world, tdt_comm **out);
int tdt_comm_destroy(tdt_comm *comm);
int tdt_allgatherv(tdt_comm *comm, const void *d_send, size_t send_count, void *d_recv, const size_t *counts, const size_t *displs,
                   int elem_bytes);
int tdt_allreduce_sum_f64(tdt_comm *comm, double *d_buf, size_t n);
/* The broadcasts tdt_allgatherv issues, as a pure host function (no RCCL, no GPU): ops[k] = root rank, destination byte range in
 * d_recv, and whether this rank reads its send buffer (it is the root).  Empty contributions issue nothing; overlapping ranges and
 * ranges beyond recv_capacity_bytes (0 = not checked) are refused.  ops must hold `world` entries. */
typedef struct tdt_gather_op {
    int root;
    int from_send;
    size_t offset_bytes;
    size_t nbytes;
} tdt_gather_op;
int tdt_allgatherv_plan(int rank, int world, const size_t *counts, const size_t *displs, int elem_bytes, size_t recv_capacity_bytes,
                        tdt_gather_op *ops, int *n_ops);

/* ---- discordant-pair candidate selection ------------------------------------------------------ *
 * Replaces the per-read predicate chain of tiddit_signal.worker (tiddit_signal.pyx:171-211): a read is a
 * discordant-pair signal iff its contig is processed (contig_ok[tid], = LN >= min_contig) and it is mapped,
 * not duplicate, primary, mapq >= min_q, paired with a mapped mate, and |tlen| > max_ins or the mate lies on
 * another contig.  The indices of the selected reads are returned in stream order (wavefront compaction). */
int tdt_signal_select(tdt_ctx *ctx, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *mate_tid,
                      const int32_t *tlen, size_t n, const uint8_t *contig_ok, int n_contigs, int min_q, int64_t max_ins,
                      uint32_t *out_idx, size_t *out_count);
int tdt_signal_select_device(tdt_ctx *ctx, const uint16_t *d_flag, const uint8_t *d_mapq, const int32_t *d_tid,
                             const int32_t *d_mate_tid, const int32_t *d_tlen, size_t n, const uint8_t *d_contig_ok, int n_contigs,
                             int min_q, int64_t max_ins, uint32_t *d_out_idx, uint64_t *d_count);

/* The WHOLE per-read chain of tiddit_signal.worker (tiddit_signal.pyx:171-221) on a decoded batch resident in HBM.  d_arrays14 =
 * the pointer table of tdt_ingest_arrays (TDT_COL_*: tdt_bam_decode's field order, then the raw record bytes); contig_ok is a HOST array.
 * Every read gets an action byte — 2: clipped read for local assembly (:190-197), 4: carries an SA tag, SA_analysis is called
 * (:199-202), 8: a discordant-pair row is appended (:204-221) — and the reads with any bit set are compacted in stream order
 * with their fields and raw record bytes, so that the host touches only those.  tdt_signal_scan returns how many (*n_sel) and
 * their total record bytes; tdt_signal_scan_result copies them out: meta = n_sel records of 28 bytes {uint32 index in the
 * batch; int32 tid, pos, end, mate_tid, sa_rel (offset of the SA:Z string inside the record, -1 without); uint16 flag; uint8
 * action; uint8 0}, raw_end[k] = end offset of record k inside raw (record k starts at raw_end[k-1], its block_size field
 * first).  The result of the calling thread's last scan is kept until its next one. */
int tdt_signal_scan(tdt_ctx *ctx, const void *const *d_arrays14, size_t n, const uint8_t *contig_ok, int n_contigs, int min_q, int64_t max_ins,
                    int min_anchor_len, int min_clip_len, size_t *n_sel, size_t *raw_bytes);
int tdt_signal_scan_result(tdt_ctx *ctx, void *meta, uint32_t *raw_end, uint8_t *raw);
/* The clips.append entries of worker (:192-197) as text: for the selected records `which[0..m)` (indices into the arrays of
 * tdt_signal_scan_result) `>query_name|contig|pos+1\nSEQUENCE\n`, concatenated.  Two-call protocol like tdt_format_coverage. */
int tdt_format_clips(const void *meta, const uint32_t *raw_end, const uint8_t *raw, const uint32_t *which, size_t m, const char *contig,
                     char *out, size_t out_cap, size_t *out_len);

/* ---- signal tables (host, no Python in the per-row path) ------------------------------------------ *
 * Replaces, for the discordant / split / clipped reads tdt_signal_scan selected:
 *   - the merge loop of tiddit_signal.main (tiddit_signal.pyx:246-284: data[chrA][chrB][fragment], splits[..] +=) and its three
 *     writers (:298-332: discordants_{sample}.tab, splits_{sample}.tab, the clip FASTA files),
 *   - the signal table of tiddit_cluster.main (tiddit_cluster.pyx:47-105: find_discordant_pos :7-37, the clip QUIRK :67-70),
 *   - the per-row half of its regrouping (:156-254): which signals make up which candidate, in the reference's insertion order.
 * One table per job, used by one thread at a time.  names = the header's contig names, NUL-terminated, back to back, in header
 * order; contigs >= min_contig are main()'s `chromosomes`.  Byte-identical output for coordinate-sorted AND unsorted input (see
 * csrc/tdt_sigtab.hip).  TDT_E_KEY where the reference raises KeyError (a split row whose chrB is not in the header). */
int tdt_sigtab_create(const char *names, const int64_t *lengths, int n_contigs, int64_t min_contig, void **out);
void tdt_sigtab_destroy(void *t);
/* the arrays of tdt_signal_scan_result, batch by batch in file order.  *stopped == n_sel: done; else the index of a split read whose
 * SA tag tdt_split_fields does not take — hand its row over with tdt_sigtab_add_split_row (or drop it) and call again with
 * resume = *stopped + 1. */
int tdt_sigtab_add(void *t, const void *meta, const uint32_t *raw_end, const uint8_t *raw, size_t n_sel, size_t raw_len, int min_q, size_t resume,
                   size_t *stopped);
int tdt_sigtab_add_split_row(void *t, int tid, const char *chrA, const char *chrB, const char *qname, const int64_t *six, int is_reverse, int sa_minus);
int tdt_sigtab_add_clips(void *t, int tid, const char *bytes, size_t len);
int tdt_sigtab_clips(void *t, int tid, const char **ptr, size_t *len);      /* clips/{contig}.fa of one contig (valid until the table changes) */
int tdt_sigtab_stats(void *t, int64_t *out8);
/* the row log as one blob (N-rank job: rows travel to the owner rank of their chrA; owner == NULL: all rows) — two-call protocol */
int tdt_sigtab_export(void *t, const int32_t *owner, int dest, void *out, size_t cap, size_t *need);
int tdt_sigtab_import(void *t, const void *blob, size_t len);
int tdt_sigtab_format(void *t, size_t *n_segments_disc, size_t *n_segments_split);
/* kind 0 = discordants, 1 = splits; segments: 5 int64 per contig pair with rows (chrA id, chrB id, offset, length, rows) */
int tdt_sigtab_text(void *t, int kind, const char **ptr, size_t *len, int64_t *segments);
/* bytes per contig of one output — what 0: the rows of discordants_{sample}.tab with that chrA, 1: splits_{sample}.tab, 2: the contig's
 * clip FASTA — and one such block written at `offset` of an open file: a file is its blocks in header order, so N ranks place theirs */
int tdt_sigtab_sizes(void *t, int what, int64_t *out_per_contig);
int tdt_sigtab_pwrite(void *t, int what, int contig, int fd, int64_t offset);
int tdt_sigtab_cluster_table(void *t, int is_mp, int64_t min_contig, size_t *n_signals, int *n_buckets);
int tdt_sigtab_cluster_columns(void *t, int32_t *posA, int32_t *posB, int64_t *bucket_off, int32_t *bucket_a, int32_t *bucket_b);
/* one byte per row of the cluster table, in the order of tdt_sigtab_cluster_columns: 0 = discordant pair, 1 = split read */
int tdt_sigtab_cluster_kinds(void *t, uint8_t *kind);
int tdt_sigtab_regroup(void *t, const int32_t *labels, size_t *n_candidates, size_t *n_members, size_t *name_bytes);
int tdt_sigtab_regroup_result(void *t, int32_t *cand4, int32_t *startA, int32_t *endA, int32_t *startB, int32_t *endB, int32_t *posA, int32_t *posB,
                              uint8_t *oriA, uint8_t *oriB, char *names);

/* ---- masked medians of the coverage bins -------------------------------------------------------- *
 * Replaces the per-bin Python loop + numpy.median of determine_ploidy (tiddit_coverage_analysis.pyx:14-27).
 * cov/gc are the concatenated float64 bins / int8 GC bins; segment s = [seg_off[2s], seg_off[2s+1]) (segments may
 * overlap: per-contig segments plus one covering everything).  For every segment the selected values are
 * { cov[i] : cov[i] > 0 and gc[i] != -1 }; count[s] = how many, lower[s]/upper[s] = the two middle order statistics
 * (equal for odd counts) — numpy.median is their mean.  Radix select on the device, no sort. */
int tdt_masked_medians(tdt_ctx *ctx, const double *cov, const int8_t *gc, const int64_t *seg_off, int nseg, double *lower,
                       double *upper, int64_t *count);
/* The same for data in n_parts separate host arrays (determine_ploidy's per-contig arrays): results 0 .. n_parts-1 are the parts' medians,
 * result n_parts the median over all of them; every part is copied to the device from where it lies. */
int tdt_masked_medians_parts(tdt_ctx *ctx, const double *const *cov_parts, const int8_t *const *gc_parts, const int64_t *part_len, int n_parts,
                             double *lower, double *upper, int64_t *count);

/* ---- library statistics on the device (tiddit_stats.statistics, tiddit_stats.py:5-78) ------------------------- *
 * tdt_stats_push_device takes the decoded field arrays of one ingest batch (device pointers) and applies the sampling loop (:17-47):
 * placed reads are numbered across batches, the cut-off after n_reads is honoured to the read, the insert sizes of the passing
 * pairs are appended in order to a device list; *done = the sample is complete.  tdt_stats_counts: sampled, sum and count of the
 * read lengths, innie, outtie, number and sum of the insert sizes (+ 2 per-batch figures).  tdt_stats_moments: numpy's
 * mean((x - mean)^2) of the list (numpy.std = its square root; numpy's summation order reproduced) and the two order statistics
 * k0 <= k1 that numpy.percentile interpolates between (radix select).  Everything is bit-identical to the numpy calls (:52-56). */
typedef struct tdt_stats tdt_stats;
int tdt_stats_create(tdt_ctx *ctx, int64_t n_reads, int min_mapq, int64_t max_ins_len, tdt_stats **out);
int tdt_stats_destroy(tdt_stats *s);
int tdt_stats_push_device(tdt_stats *s, const int32_t *d_tid, const int32_t *d_pos, const int32_t *d_mate_tid, const int32_t *d_mate_pos,
                          const int32_t *d_tlen, const int32_t *d_l_seq, const uint16_t *d_flag, const uint8_t *d_mapq, size_t n, int *done);
int tdt_stats_counts(tdt_stats *s, int64_t *counts9);
int tdt_stats_moments(tdt_stats *s, double mean, int64_t k0, int64_t k1, double *mean_sqdev, int32_t *order0, int32_t *order1);

/* ---- region means of the coverage bins per SV candidate --------------------------------------------- *
 * Replaces the per-candidate numpy.average calls of tiddit_variant.define_variant (tiddit_variant.pyx:265-283: avg_a / avg_b over
 * the 50-bp bins [start/50, end/50]; :307-315: covM over the bins between the breakpoints with gc != -1).  cov / gc are the
 * concatenated float64 coverage bins / int8 GC bins; segment q = [seg_lo[q], seg_hi[q]) indexes them (seg_lo/seg_hi/masked are
 * HOST arrays in both entry points); masked[q] != 0 keeps only the bins with gc > -1 (order preserved).  mean[q] equals
 * numpy.average of that slice BIT FOR BIT (numpy's chunked pairwise summation order is reproduced), NaN for an empty one;
 * count[q] = number of bins averaged (the reference falls back to the contig's coverage when covM has <= 4 of them). */
int tdt_segment_means(tdt_ctx *ctx, const double *cov, const int8_t *gc, int64_t total, const int64_t *seg_lo, const int64_t *seg_hi,
                      const uint8_t *masked, size_t nq, double *mean, int64_t *count);
int tdt_segment_means_device(tdt_ctx *ctx, const double *d_cov, const int8_t *d_gc, const int64_t *seg_lo, const int64_t *seg_hi,
                             const uint8_t *masked, size_t nq, double *d_mean, int64_t *d_count);

/* ---- regional evidence counts per SV candidate --------------------------------------------------- *
 * Replaces the per-candidate BAM re-scan of tiddit_variant.get_region (tiddit_variant.pyx:54-151).  The arrays
 * are ONE contig's coordinate-sorted alignment records (has_sa[i] != 0 iff the record carries an SA tag, tid = the
 * contig's id for the `next_reference_name != reference_name` test).  Query q = (start, end, bp) as in the
 * reference call get_region(samfile, chr, start, end, bp, min_q, max_ins, ...).  out[q*7 + ...] =
 * bases, n_reads, low_q, n_discs, n_splits, crossing_f, crossing_r  (the reference then returns
 * coverage = bases/(end-start+1) and frac_low_q = low_q/n_reads). */
int tdt_region_counts(tdt_ctx *ctx, const int32_t *start, const int32_t *end, const uint8_t *mapq, const uint16_t *flag,
                      const int32_t *mate_tid, const int32_t *mate_pos, const int32_t *tlen, const uint8_t *has_sa, size_t n, int tid,
                      int64_t contig_length, const int32_t *q_start, const int32_t *q_end, const int32_t *q_bp, size_t nq, int min_q,
                      int64_t max_ins, int64_t *out);
int tdt_region_counts_device(tdt_ctx *ctx, const int32_t *d_start, const int32_t *d_end, const uint8_t *d_mapq, const uint16_t *d_flag,
                             const int32_t *d_mate_tid, const int32_t *d_mate_pos, const int32_t *d_tlen, const uint8_t *d_has_sa,
                             size_t n, int tid, int max_span, int64_t contig_length, const int32_t *d_q_start, const int32_t *d_q_end,
                             const int32_t *d_q_bp, size_t nq, int min_q, int64_t max_ins, int64_t *d_out);

/* ---- the evidence store: the scan's placed records packed for the variant stage ----------------------------------- *
 * Filled batch by batch during the signal scan (tdt_evstore_append_device: device field arrays of one decoded batch, whose first n
 * records are placed, tid >= 0; tdt_evstore_append: the same from host arrays, uploaded first).  Records are appended in file
 * order, so each contig of a coordinate-sorted file is one contiguous, sorted range; the caller keeps the ranges.  One record =
 * 16 bytes {int32 start, int32 end, int32 mate_pos, uint8 bits, 3 bytes zero}; bits = TDT_EV_* below, LOW_Q / DISCORDANT
 * evaluated with the store's min_q / max_ins (|tlen| > max_ins or mate_tid != tid).  The buffer grows on the device (a bigger
 * allocation and a device copy) when a batch does not fit.  tdt_evstore_spans: per contig max(end - start), int32[n_contigs]. */
#define TDT_EV_UNMAPPED 0x04u
#define TDT_EV_MATE_UNMAPPED 0x08u
#define TDT_EV_DUPLICATE 0x01u
#define TDT_EV_HAS_SA 0x02u
#define TDT_EV_LOW_Q 0x10u
#define TDT_EV_DISCORDANT 0x20u
typedef struct tdt_evstore tdt_evstore;
int tdt_evstore_create(tdt_ctx *ctx, int n_contigs, int min_q, int64_t max_ins, size_t capacity, tdt_evstore **out);
int tdt_evstore_destroy(tdt_evstore *s);
int tdt_evstore_append_device(tdt_evstore *s, const int32_t *d_tid, const int32_t *d_pos, const int32_t *d_end, const uint8_t *d_mapq,
                              const uint16_t *d_flag, const int32_t *d_mate_tid, const int32_t *d_mate_pos, const int32_t *d_tlen,
                              const int64_t *d_sa_off, size_t n);
int tdt_evstore_append(tdt_evstore *s, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint8_t *mapq, const uint16_t *flag,
                       const int32_t *mate_tid, const int32_t *mate_pos, const int32_t *tlen, const int64_t *sa_off, size_t n);
int tdt_evstore_info(tdt_evstore *s, size_t *n, size_t *capacity, void **d_records);
int tdt_evstore_spans(tdt_evstore *s, int32_t *spans);
/* get_region's seven sums (as tdt_region_counts) for every query of every contig in ONE launch over the store.  contigs =
 * int64[n_contigs][5] (offset, n, max span, tid, contig length) of the store's ranges; queries = int32[nq][4] (contig row, start,
 * end, bp); out = int64[nq][7].  Host arrays.  TDT_E_ARG when min_q / max_ins are not the ones the store was packed with,
 * TDT_E_RANGE when a row lies outside the store or a query names no row. */
int tdt_region_counts_packed(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, const int32_t *queries, size_t nq,
                             int min_q, int64_t max_ins, int64_t *out);
/* The same counts with device queries and a device output (what a broadcast delivers and a reduce sends on): d_queries =
 * int32[nq][4] in HBM, 16-byte aligned; d_out = int64[nq][7] in HBM; contigs = the host table as above, validated on the host.  The
 * kernel checks every query's row: a query naming no row gets zeros, and the call returns TDT_E_RANGE naming the first such query.
 * The library's stream is synchronised before the return.  TDT_E_ARG as above for other min_q / max_ins. */
int tdt_region_counts_packed_device(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, const int32_t *d_queries,
                                    size_t nq, int min_q, int64_t max_ins, int64_t *d_out);

/* ---- per-contig depth distributions from the evidence store (TIDDIT_DEPTH_DIST) ------------------------------- *
 * The depth of base b (0 <= b < LN) of a contig is the number of its records with none of TDT_EV_UNMAPPED, TDT_EV_DUPLICATE,
 * TDT_EV_LOW_Q and start <= b < min(end, LN) — the store's end is the exclusive reference end; a record with end <= start covers
 * nothing.  contigs = int64[n_contigs][5] (offset, n, max span, tid, contig length), the table of tdt_region_counts_packed, validated
 * the same way; out = int64[n_contigs][cap + 4] on the host, per row: the bases at depth exactly d for d < cap, the bases at depth
 * cap or more, the uncapped sum of all depths, the maximum depth, the minimum depth (a row of no records: out[0] = LN, the rest 0).
 * One launch over all contigs, one workgroup per tile of DD_TILE bases: a difference array and a histogram in LDS, 64-bit atomics
 * into the contig's row (csrc/tdt_depth_dist.hip).  cap must be the library's DD_CAP (1000).  TDT_E_ARG for a null pointer or another
 * cap, TDT_E_RANGE for a row outside the store, a negative length or 2^31 - 1 tiles or more — all before anything is launched, the
 * output untouched; n_contigs == 0 returns TDT_OK.  The context's stream is synchronised before the return. */
int tdt_depth_dist(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, int cap, int64_t *out);

/* ---- reference support at clip-site junctions from the evidence store (TIDDIT_CLIPS_VCF) ------------------------ *
 * For every boundary b (0-based: b bases lie left of the cut) of a contig of LN bases and the flank F, over the contig's records with
 * e = min(end, LN) and end > start: left = the records with start <= b - F < e (0 when b - F < 0), right = those with
 * start <= b + F - 1 < e (0 when b + F > LN), span = those with both — each over the records with none of TDT_EV_UNMAPPED,
 * TDT_EV_DUPLICATE, TDT_EV_LOW_Q — and span_lowq = the records with both whose only one of those bits is TDT_EV_LOW_Q.  b outside
 * 0 ... LN is legal and follows the same rule.  All arithmetic is 64-bit.  contigs = int64[n_contigs][5] (offset, n, max span, tid,
 * contig length), the table of tdt_region_counts_packed, validated the same way; boundaries = int32[nb][2] (contig row, b), 8-byte
 * aligned; out = int64[nb][4] (left, right, span, span_lowq).  Host arrays.  One launch over all boundaries, one wavefront per
 * boundary (csrc/tdt_junction.hip).  TDT_E_ARG for a null or misaligned pointer or F outside 1 ... 1000, TDT_E_RANGE for a row
 * outside the store, a negative length or a boundary that names no row — all before anything is launched, the output untouched;
 * nb == 0 returns TDT_OK.  The context's stream is synchronised before the return. */
int tdt_junction_support(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, const int32_t *boundaries, size_t nb, int F,
                         int64_t *out);
/* The same counts with the boundaries and the output in HBM (d_boundaries 8-byte aligned; d_out int64[nb][4]); contigs = the host
 * table as above, validated on the host.  The kernel checks every boundary's row: a boundary naming no row gets zeros, and the call
 * returns TDT_E_RANGE naming the first such boundary.  The context's stream is synchronised before the return. */
int tdt_junction_support_device(tdt_ctx *ctx, tdt_evstore *s, const int64_t *contigs, int n_contigs, const int32_t *d_boundaries, size_t nb,
                                int F, int64_t *d_out);
/* the device milliseconds of the last of the two calls above that launched over this store (the kernel alone, between two events) */
int tdt_junction_timing(tdt_evstore *s, double *ms);

/* ---- order statistics for the depth fold-changes of genotyped sites (TIDDIT_GENOTYPE_DEPTH) ------------ *
 * cov / gc are the concatenated float64 coverage bins / int8 GC bins (n of them, n < 2^31 - 1; coverage is non-negative, -0.0 reads
 * as +0.0).  Radix select on the bit patterns (csrc/tdt_depth.hip): lower / upper are the two middle order statistics (equal for an
 * odd count, 0 for an empty selection), count the number of values selected — numpy.median is numpy.mean([lower, upper]).
 * tdt_window_medians: table = int64[nq][6] rows {off, first1, last1, first2, last2, cls}: the bins off + first1 .. off + last1 and
 * off + first2 .. off + last2 (inclusive; {-1, -1} = no such range) as ONE set, of which the bins with gc != -1 are selected (zero
 * coverage counts).  cls == -1: the values are cov[bin]; 0 <= cls < ncls: the values are class_med[cls][gc[bin]] (class_med =
 * float64[ncls][101], e.g. tdt_gc_class_medians' medians) and a bin whose entry is NaN is not selected either.  Windows of at most
 * DP_WINDOW_LIMIT bins are answered by one wavefront each, all in one launch; longer ones by one workgroup each in a second.
 * Refused before anything is launched: a null or misaligned (8 bytes) pointer and first > last (TDT_E_ARG), an offset, bin or class
 * row outside the arrays (TDT_E_RANGE); nq == 0 returns TDT_OK whatever the pointers.  tdt_window_medians_device: everything in HBM;
 * the kernel makes the range checks — a refused window gets zeros and the call returns TDT_E_RANGE naming the first one.
 * tdt_gc_class_medians: seg = int64[nseg][2] {offset, bins} (a HOST array in both entries); for segment s and class g = 0 .. 100
 * the values { cov[i] : gc[i] == g and cov[i] > 0 }; outputs [nseg][101].  One workgroup per segment and middle, a [101][256]
 * histogram in LDS, 8 passes over the segment.  All four synchronise the context's stream before they return. */
int tdt_window_medians(tdt_ctx *ctx, const double *cov, const int8_t *gc, int64_t n, const int64_t *table, size_t nq, const double *class_med,
                       int ncls, double *lower, double *upper, int64_t *count);
int tdt_window_medians_device(tdt_ctx *ctx, const double *d_cov, const int8_t *d_gc, int64_t n, const int64_t *d_table, size_t nq,
                              const double *d_class_med, int ncls, double *d_lower, double *d_upper, int64_t *d_count);
int tdt_gc_class_medians(tdt_ctx *ctx, const double *cov, const int8_t *gc, int64_t n, const int64_t *seg, int nseg, double *lower,
                         double *upper, int64_t *count);
int tdt_gc_class_medians_device(tdt_ctx *ctx, const double *d_cov, const int8_t *d_gc, int64_t n, const int64_t *seg, int nseg,
                                double *d_lower, double *d_upper, int64_t *d_count);

/* ---- copy-number segments from the depth bins (TIDDIT_CNV; tiddit_amd/tiddit_cnv.py has the definition) ------------- *
 * tdt_cnv_bins: cov / gc are the concatenated float64 coverage bins / int8 GC bins of the processed contigs (n of them, n < 2^31 - 1);
 * table = int64[nseg][5] rows {off, nb, K, P, toff} (a HOST array in both entries): the contig's bins off .. off + nb - 1, K of them
 * (1 .. 64) to a CNV bin, its ploidy P (1 .. 6), and toff = the index of its first CNV bin in x, which must be the sum of
 * ceil(nb / K) over the rows before it.  E = float64[nseg][101]: the expected depth of a 50-bp bin of GC class g of row s.  CNV bin
 * t of a row covers its bins tK .. min((t + 1)K, nb) - 1; the usable ones have gc in 0 .. 100 (n_t of them).  2 n_t < K: x = -1.
 * Otherwise x = min(8 unit, (int)rint((obs / exp) * (double)(P unit))) with obs / exp the float64 sums of cov / E[s][gc] over the
 * usable bins, added left to right by one lane.  x = int32[sum of ceil(nb / K)].
 * tdt_cnv_viterbi: x as above (x < 0 = masked), n = its length; table = int64[nseg][3] rows {toff, T, P} (HOST), contiguous from 0
 * and summing to n, P in 0 .. 7.  state = int8[n]: for every row the minimum-cost path over the states 0 .. 7 of the chain
 * V_0(k) = e_0(k) + (k == P ? 0 : lambda), V_t(k) = e_t(k) + min(V_{t-1}(k), min_i V_{t-1}(i) + lambda), e_t(k) =
 * min(cap, (x_t - unit k)^2) or 0 for a masked bin, end cost V_{T-1}(k) + (k == P ? 0 : lambda); ties go to staying
 * (V_{t-1}(k) <= m + lambda) and to the lowest state.  int64 costs; the chain is cut into chunks of CNV_CHUNK bins whose (min,+)
 * matrices are stitched, which gives the sequential result exactly (csrc/tdt_cnv.hip).  unit in 1 .. 2^20, cap and lambda in
 * 0 .. 2^28.  All contigs in one call.
 * All four: TDT_E_ARG for a null context, a negative count, a parameter outside its range and — unless n == 0 or nseg == 0, which
 * return TDT_OK — a null or misaligned pointer (8 bytes for float64 / int64, 4 for int32); TDT_E_RANGE for a row outside the
 * arrays or not following the row before it; all before anything is launched, the outputs untouched.  The _device entries take
 * cov, gc, E, x, state in HBM.  The context's stream is synchronised before the return. */
int tdt_cnv_bins(tdt_ctx *ctx, const double *cov, const int8_t *gc, int64_t n, const int64_t *table, int nseg, const double *E, int unit,
                 int32_t *x);
int tdt_cnv_bins_device(tdt_ctx *ctx, const double *d_cov, const int8_t *d_gc, int64_t n, const int64_t *table, int nseg, const double *d_E,
                        int unit, int32_t *d_x);
int tdt_cnv_viterbi(tdt_ctx *ctx, const int32_t *x, int64_t n, const int64_t *table, int nseg, int unit, int64_t cap, int64_t lambda,
                    int8_t *state);
int tdt_cnv_viterbi_device(tdt_ctx *ctx, const int32_t *d_x, int64_t n, const int64_t *table, int nseg, int unit, int64_t cap, int64_t lambda,
                           int8_t *d_state);

/* ---- allele-specific copy number (TIDDIT_ASCN; tiddit_amd/tiddit_ascn.py has the definition) -------------------------- *
 * tdt_ascn_emissions: counts = uint32[nsites][8], the counter table of tdt_alleles_counts; site_pos = int32[nsites], its positions
 * (0-based, sorted inside every row's range); cols = uint8[nsites][2], the counter columns (0 .. 7) of the site's REF and ALT; x =
 * int32[total], the CNV bins of tdt_cnv_bins (x < 0 = masked).  table = int64[nseg][5] rows {site_lo, site_hi, toff, T, W} (a HOST
 * array in both entries): the contig's sites site_lo .. site_hi - 1, its T bins of W bp (1 .. 3200) from bin toff, contiguous from 0
 * and summing to total.  Bin t of a row holds its sites with t W <= pos < (t + 1) W, found with two lower bounds.  A site with
 * n = ref_n + alt_n >= min_n is informative: beta = (min(ref_n, alt_n) * bu) / n in 64 bits, h = min(acap, beta^2), and for state k =
 * (c, m) of the 16 (c = 0 .. 6, 0 <= m <= c / 2, c ascending, then m) g(k) = h if m == 0, else min(min(acap, (beta - (bu m) / c)^2),
 * h + hom).  E[t][k] = (x_t < 0 ? 0 : min(cap, (x_t - unit c)^2)) + the sum of g(k) over the bin's informative sites; nsite[t] = their
 * number, sum_beta[t] = the sum of their beta.  unit in 1 .. 2^20, cap in 0 .. 2^28, bu in 1 .. 2^15, acap in 0 .. 2^16, hom in
 * 0 .. 2^28, min_n >= 1.  E = int32[total][16], nsite = int32[total], sum_beta = int32[total].  Positions that repeat inside a row are
 * outside the contract (an emission may pass 2^31); the host entry refuses a column above 7 (TDT_E_RANGE), the device entry reads its
 * low three bits.
 * tdt_hmm16_viterbi: e = int32[n][16], the emissions of n bins; table = int64[nseg][3] rows {toff, T, home} (HOST), contiguous from 0
 * and summing to n, home in 0 .. 15.  state = int8[n]: for every row the minimum-cost path over the 16 states of the chain
 * V_0(k) = e_0(k) + (k == home ? 0 : lambda), V_t(k) = e_t(k) + min(V_{t-1}(k), min_i V_{t-1}(i) + lambda), end cost V_{T-1}(k) +
 * (k == home ? 0 : lambda); ties go to staying (V_{t-1}(k) <= m + lambda) and to the lowest state.  int64 costs, chunks of 256 bins
 * whose (min,+) matrices are stitched: the sequential result exactly (csrc/tdt_ascn.hip).  lambda in 0 .. 2^28; emissions outside
 * 0 .. 2^28 are outside the contract — the host entry refuses them (TDT_E_RANGE), the device entry does not look.
 * All four: TDT_E_ARG for a null context, a negative count, a parameter outside its range and — unless the bins or nseg are 0, which
 * return TDT_OK — a null or misaligned pointer (8 bytes for int64, 4 for int32 / uint32); TDT_E_RANGE for a row outside the arrays or
 * not following the row before it; all before anything is launched, the outputs untouched.  The _device entries take every array but
 * table in HBM.  The context's stream is synchronised before the return. */
int tdt_ascn_emissions(tdt_ctx *ctx, const uint32_t *counts, const int32_t *site_pos, const uint8_t *cols, int64_t nsites, const int32_t *x,
                       int64_t total, const int64_t *table, int nseg, int unit, int64_t cap, int bu, int acap, int hom, int min_n, int32_t *E,
                       int32_t *nsite, int32_t *sum_beta);
int tdt_ascn_emissions_device(tdt_ctx *ctx, const uint32_t *d_counts, const int32_t *d_site_pos, const uint8_t *d_cols, int64_t nsites,
                              const int32_t *d_x, int64_t total, const int64_t *table, int nseg, int unit, int64_t cap, int bu, int acap, int hom,
                              int min_n, int32_t *d_E, int32_t *d_nsite, int32_t *d_sum_beta);
int tdt_hmm16_viterbi(tdt_ctx *ctx, const int32_t *e, int64_t n, const int64_t *table, int nseg, int64_t lambda, int8_t *state);
int tdt_hmm16_viterbi_device(tdt_ctx *ctx, const int32_t *d_e, int64_t n, const int64_t *table, int nseg, int64_t lambda, int8_t *d_state);

/* ---- link counts of SV sites (TIDDIT_GENOTYPE) ------------------------------------------------------- *
 * How many signals of the cluster table join the two regions of a site: for site {bucket, startA, endA, startB, endB} the rows of
 * that (chrA, chrB) bucket with startA <= posA <= endA and startB <= posB <= endB, counted per kind — out[0] the discordant pairs
 * (kind 0), out[1] the split reads (kind 1); rows of kind 2 (assembly contigs) are counted in neither.  Buckets and the A/B
 * orientation of a row are those of tdt_sigtab_cluster_table, so signals on contigs below its min_contig are in no bucket and count
 * as zero; the caller flips a site whose contigs are in the other order.
 * tdt_links_create: host columns (pinned or not) posA / posB / kind of bucket_off[nb] signals, bucket_off = int64[nb + 1] starting
 * at 0 and not decreasing.  The columns are uploaded, every bucket is sorted by posA on the device and ONE 8-byte record per signal
 * {posA, posB | kind << 30} stays in HBM: TDT_E_UNSUPPORTED for a posB outside [0, 2^30) or a kind above 2, TDT_E_RANGE for 2^30
 * signals or more.  tdt_links_count: sites = int32[ns][6] {bucket, startA, endA, startB, endB, 0} and out = int64[ns][2] on the
 * host; one launch, one wave per site.  bucket -1 (no signals between these contigs) gives zeros.  Refused on the host, before
 * anything is launched: start > end (TDT_E_ARG), a bucket below -1 or >= nb (TDT_E_RANGE); ns == 0 returns TDT_OK.
 * tdt_links_count_device: sites and counts in HBM (8-byte aligned); the kernel makes the same checks — a refused site gets zeros and
 * the call returns TDT_E_RANGE naming the first one.  Both synchronise the context's stream before they return. */
typedef struct tdt_links tdt_links;
int tdt_links_create(tdt_ctx *ctx, const int32_t *posA, const int32_t *posB, const uint8_t *kind, const int64_t *bucket_off, int nb,
                     tdt_links **out);
int tdt_links_destroy(tdt_links *h);
int tdt_links_count(tdt_links *h, const int32_t *sites, size_t ns, int64_t *out);
int tdt_links_count_device(tdt_links *h, const int32_t *d_sites, size_t ns, int64_t *d_out);

/* ---- coverage table text (host, threaded) ----------------------------------------------------------- *
 * The row loop of print_coverage (tiddit_coverage.pyx:30-44) for one contig: kind 0 = bed rows
 * `name \t 1+i*bin \t (i+1)*bin+1 \t value \n` (last row ends at contig_len), kind 1 = wig values, one per line.
 * Values are written exactly like Python's `"{}".format(numpy.float64)`.  Two-call protocol: out == NULL returns the
 * size in *out_len; then call again with a buffer of at least that many bytes. */
/* The numeric half of tiddit_signal.SA_analysis (tiddit_signal.pyx:11-145) for the selected records `which` (those carrying an SA tag):
 * out[k] = {int32 status (0: SA mapQ below min_q, 1: valid, 2: unusual tag — run the literal code), read_start, read_end, split_pos,
 * sa_split (before the swap), seg_start, seg_end, uint32 chr_off, chr_len (the SA contig name inside raw), uint8 is_reverse, sa_minus,
 * 2 pad} — 40 bytes.  The contig-name order and the swap (:118-140) are string decisions left to the caller.  Host function. */
int tdt_split_fields(const void *meta, const uint32_t *raw_end, const uint8_t *raw, size_t raw_len, const uint32_t *which, size_t m, int min_q, void *out);
int tdt_format_coverage(const double *values, size_t n, const char *name, int64_t bin_size, int64_t contig_len, int kind, char *out,
                        size_t out_cap, size_t *out_len);

/* FASTA index: writes `fai_path` in samtools faidx format (name, bases, offset of the first base, bases per line, bytes per
 * line) — what the reference obtains from pysam.faidx when the .fai is missing (__main__.py:95-97). */
int tdt_fasta_write_fai(const char *fasta_path, const char *fai_path);

/* ---- BGZF inflate (host, threaded) ---------------------------------------------------------------- *
 * Replaces pysam/htslib's block reader (`pysam.AlignmentFile(bam, "r", threads=n)`, tiddit_signal.pyx:159,
 * __main__.py:224).  tdt_bgzf_scan hops the block headers of `comp[0..len)`: it reports how many WHOLE blocks are
 * present, their compressed size (`consumed`) and what they inflate to (`produced`, never more than max_out).
 * tdt_bgzf_inflate inflates exactly such a span (len = consumed, out_len = produced) on `threads` host threads
 * (<= 0: tdt_host_threads' value), every block straight to its final offset, CRC32 and ISIZE verified.
 * tdt_host_threads(n) sets the worker count for the host stages (n <= 0: query only) and returns the previous
 * value; default min(hardware threads, 64) or $TIDDIT_HOST_THREADS. */
int tdt_host_threads(int n);
int tdt_bgzf_scan(const uint8_t *comp, size_t len, size_t max_out, size_t *n_blocks, size_t *consumed, size_t *produced);
int tdt_bgzf_inflate(const uint8_t *comp, size_t len, uint8_t *out, size_t out_len, int threads);

/* Same contract as tdt_bgzf_inflate, but the blocks are inflated ON THE DEVICE (one wavefront per block, CRC32 and ISIZE
 * verified there): `comp` is a host pointer to whole BGZF blocks; `out` is a host buffer, or a device pointer when
 * out_on_device != 0 (the record decode and the histogram kernels then read it in place). */
int tdt_bgzf_inflate_hbm(tdt_ctx *ctx, const uint8_t *comp, size_t len, uint8_t *out, size_t out_len, int out_on_device);

/* ---- BAM ingest on the device ------------------------------------------------------------------------ *
 * The per-read attribute access of the reference's loops (`for read in samfile.fetch(until_eof=True)`,
 * __main__.py:229-240, tiddit_signal.pyx:169-221) as one call per batch of BGZF blocks: inflate, find the records,
 * decode the packed arrays — all in HBM.  n_ref = number of @SQ contigs (record sanity check).
 * tdt_ingest_push: `comp` = `len` bytes of WHOLE BGZF blocks (host memory, see tdt_bgzf_scan); `skip` = inflated bytes
 * in front of the first record (the BAM header; first call only).  The incomplete record at the end of the batch is
 * kept and prepended to the next call.  Records are located by parallel per-segment guesses that the host confirms
 * against the block_size chain; a batch that cannot be confirmed is chased serially on the host instead (counted in
 * tdt_ingest_carry's host_chases) — the result is the sequential decode either way.  After a push has returned an error
 * the stream position is undefined: further pushes on that object are refused.  tdt_ingest_arrays: device pointers, valid until the next push, in tdt_bam_decode's
 * output order (tid, pos, end, mapq, flag, mate_tid, mate_pos, tlen, l_seq, cigar_first, cigar_last, rec_off, sa_off)
 * followed by the batch's raw record bytes (rec_off / sa_off index into them) — the TDT_COL_* below, the ONE statement of that
 * order: every reader of the table indexes it by these names.  tdt_ingest_edges: record indices
 * where the contig id changes (*n = (size_t)-1 when there are more than 8191, i.e. the input is not coordinate
 * sorted).  tdt_ingest_carry: bytes of the pending partial record (0 after a well-formed file). */
enum { TDT_COL_TID = 0, TDT_COL_POS, TDT_COL_END, TDT_COL_MAPQ, TDT_COL_FLAG, TDT_COL_MATE_TID, TDT_COL_MATE_POS, TDT_COL_TLEN, TDT_COL_L_SEQ,
       TDT_COL_CIGAR_FIRST, TDT_COL_CIGAR_LAST, TDT_COL_REC_OFF, TDT_COL_SA_OFF, TDT_COL_RAW, TDT_NCOL };
typedef struct tdt_ingest tdt_ingest;
int tdt_ingest_create(tdt_ctx *ctx, int n_ref, tdt_ingest **out);
int tdt_ingest_destroy(tdt_ingest *g);
int tdt_ingest_push(tdt_ingest *g, const uint8_t *comp, size_t len, size_t skip, size_t *n_records);
/* Sharded reads (one process per GPU on one file).  skip = (size_t)-1: the stream starts at a BGZF block somewhere
 * inside the file and the first record is located by the guess (*first_off = its inflated offset).  own_bytes: the
 * first own_bytes inflated bytes of this call belong to this shard, the blocks after them only complete its last
 * record; records starting at or beyond own_bytes are left to the next shard and *next_off = offset of the first of
 * them from that boundary.  The caller checks next_off of shard r against first_off of shard r+1: shard 0 starts from
 * the header (exact), so agreement at every seam makes the whole decode exact.  A bounded push ends the stream. */
int tdt_ingest_push_bounded(tdt_ingest *g, const uint8_t *comp, size_t len, size_t skip, size_t own_bytes, size_t *n_records,
                            size_t *first_off, size_t *next_off);
/* Optional overlap: start the host-to-device copy of the NEXT span (pinned memory) on the copy stream; the next push of
 * exactly this (pointer, len) finds it there, so the transfer hides behind the kernels of the push issued in between. */
int tdt_ingest_prefetch(tdt_ingest *g, const uint8_t *comp, size_t len);
int tdt_ingest_arrays(tdt_ingest *g, const void **out14, size_t *raw_len);
int tdt_ingest_edges(tdt_ingest *g, uint32_t *edges, size_t cap, size_t *n);
/* the contig id of the run that starts at edges[k], for every k tdt_ingest_edges reported (up to 8191 runs per batch: a GRCh38-shaped
 * file has ~1 900 contigs with reads) */
int tdt_ingest_edge_tids(tdt_ingest *g, int32_t *tids, size_t cap);
/* device pointer of the batch's PACKED coverage records (see tdt_cov_push_packed_device_multi), valid until the next push */
int tdt_ingest_packed(tdt_ingest *g, const uint64_t **d_packed);
/* From the next push on the reader writes BINNED records for `cov` (NULL: the generic packed records again) into the column
 * tdt_ingest_packed returns; *binned = 1 when it does (0: that histogram's bin size has no binned form, the column stays generic). */
int tdt_ingest_bin_for(tdt_ingest *g, tdt_cov *cov, int *binned);
/* A SECOND histogram for the same pass (`tiddit --sv` writing the --cov track from its scan): from the next push on the field-decode
 * kernel writes one more 8-byte coverage record per read, for `cov`, from the fields it already holds — BINNED records when `cov`'s bin
 * size has a binned form (*binned = 1), the generic packed records otherwise (*binned = 0).  The column is independent of
 * tdt_ingest_bin_for's.  cov == NULL detaches: the reader then launches the kernels it launched before and allocates nothing for the
 * column.  tdt_ingest_packed_second: the column's device pointer (NULL: the batch was decoded with nothing attached); it lives and
 * dies with the batch's other arrays (next push / tdt_ingest_retain + tdt_ingest_release). */
int tdt_ingest_second_for(tdt_ingest *g, tdt_cov *cov, int *binned);
int tdt_ingest_packed_second(tdt_ingest *g, const uint64_t **d_packed);
/* Enqueue the FIRST HALF of a coming span's push — its copy (or the prefetched one), its block table, the inflate + CRC kernels and the
 * copy of their status word — on the reader's own (low-priority) inflate streams, without waiting for anything.  A span inflates into an
 * output buffer of its own, a fixed gap into it (1 MB; TIDDIT_INGEST_GAP), and the partial record the batch before it ends with is copied
 * in front of the output by the push itself (a record longer than the gap moves the output once): so a span's inflate depends on NOTHING
 * the launch stream holds and may be started as soon as the span is in host memory — before the push of the span in front of it, while
 * the current batch's consumers run; the chip then never leaves the inflate kernel, and the record search, field decode and the caller's
 * kernels of batch k run beside span k+1's inflate.  At most two spans may be begun beyond the current batch; their pushes must follow in
 * the same order with exactly these (pointer, length) pairs.  The current batch (field arrays AND raw bytes) stays valid until the next
 * push; tdt_ingest_retain may be called with spans begun ahead.  (htslib's reader threads decompress ahead of the consumer in the same way.) */
int tdt_ingest_push_ahead(tdt_ingest *g, const uint8_t *comp, size_t len);
/* Keep the current batch beyond the next push: its device buffers (everything tdt_ingest_arrays / tdt_ingest_packed returned) move into
 * *handle and stay valid until tdt_ingest_release; the reader continues with fresh buffers.  Used by `tiddit --sv` to scan the batches its
 * library statistics were sampled from without reading and inflating them a second time. */
/* Where the last push spent its time (ms): [0] BGZF block table (host), [1] host-to-device copy of the span (the prefetch copy when
 * [6] = 1: it ran on the copy stream behind the previous batch's kernels), [2] inflate + CRC kernels of the span (elapsed on its inflate
 * stream: it overlaps the previous span's tail and the launch stream's kernels), [3] record-finding kernels, [4] chain check (host),
 * [5] field decode kernel, [6] prefetched, [7] wall time of the push call itself (the first half of a span begun ahead lies outside
 * it).  The figures are those of the CURRENT batch: spans begun ahead since its push do not disturb them. */
int tdt_ingest_timing(tdt_ingest *g, double *out8);
typedef struct tdt_retained tdt_retained;
int tdt_ingest_retain(tdt_ingest *g, tdt_retained **handle);
int tdt_ingest_release(tdt_retained *handle);
int tdt_ingest_carry(tdt_ingest *g, size_t *bytes, size_t *host_chases);
/* The readers' device buffers (hundreds of MB to GB each) are kept in a per-device cache between readers and retained batches instead
 * of going back to the driver (bounded: a quarter of the device's memory, at most 64 GB; TIDDIT_INGEST_CACHE_MB=<n> sets it, 0 switches
 * it off).  The library returns the cache to the driver by itself when any of its own device allocations fails and when the device's
 * last context is destroyed; an application that shares the device with other allocators (PyTorch, RCCL) calls this between jobs.
 * *released (may be NULL) = bytes handed back.  No counterpart in the reference (htslib keeps its buffers on the host). */
int tdt_device_cache_flush(tdt_ctx *ctx, uint64_t *released);
uint64_t tdt_device_cache_bytes(tdt_ctx *ctx);
/* Test hook: the next n device allocations of the library are refused once, as if the driver were out of memory, and take the
 * library's own way out (the cache goes back to the driver, the allocation is tried again — also when the cache held nothing, so the
 * hook never turns an allocation into a failure).  n = 0: off. */
void tdt_debug_fail_next_malloc(int n);
int tdt_copy_to_host(tdt_ctx *ctx, void *dst, const void *d_src, size_t bytes);
/* Measurement aid (bench.py, tools/calib_stream.py): what a plain streaming read of `bytes` of device memory reaches on this device — every
 * lane four 16-byte loads in flight, nothing written; `workgroups_per_cu` workgroups of 256 threads per CU walk the buffer grid-stride
 * (blocked = 0) or each its own contiguous share (blocked = 1: the way cov_accumulate's workgroups own 256 KB of reads each); best and mean
 * launch time over `reps` launches after one untimed pass (HIP events on the context's stream).  The roofline object of the bench quotes
 * the best of a small sweep beside the data sheet's 8 TB/s. */
int tdt_calib_stream_read(tdt_ctx *ctx, const void *d_buf, size_t bytes, int reps, int workgroups_per_cu, int blocked, double *best_ms,
                          double *mean_ms);

/* ---- allele counts at known SNV sites (TIDDIT_ALLELES) ------------------------------------------------- *
 * No counterpart in the reference; the definition is tiddit_amd/tiddit_alleles.py's.  A handle keeps the sites of every contig
 * (site_pos: 0-based, per contig sorted and unique, contig-major; site_off[n_contigs + 1]) and per site eight zeroed uint32 counters
 * A C G T N DEL SKIP LOWBQ in HBM.  A push adds one batch of reads: the filters (tid, flag & 0xF04, mapq >= min_q) are tested on the
 * field columns; a read with a site in [pos, end) has its record (at raw + rec_off: block_size, fixed fields, name, CIGAR, 4-bit
 * sequence, qualities) bounded against its own block_size and raw_len and then walked.  A record that fails the bounds, holds an op
 * code above 8 or is asked for a query base at or beyond l_seq counts nothing and adds one to `malformed`; nothing outside
 * [raw, raw + raw_len) is ever read.  More than 2^32 - 1 reads on one site are outside the contract (the counters wrap).
 * The push of device arrays takes the pointer table tdt_ingest_arrays filled (TDT_COL_*), is enqueued on the context's stream and waits for nothing; the
 * push of host arrays uploads them, runs the same kernel and returns when it is done.  Refusals: TDT_E_ARG (null pointers, offsets
 * that decrease, sites not sorted / unique / >= 0, n >= 2^31), TDT_E_RANGE (min_bq outside 0 ... 93, 2^28 sites or more); a refused
 * call leaves its outputs untouched.  The read-out calls synchronise the stream; either of their last two pointers may be NULL. */
typedef struct tdt_alleles tdt_alleles;
int tdt_alleles_create(tdt_ctx *ctx, const int32_t *site_pos, const int64_t *site_off, int n_contigs, int min_q, int min_bq,
                       tdt_alleles **out);
int tdt_alleles_destroy(tdt_alleles *h);
int tdt_alleles_reset(tdt_alleles *h);
int tdt_alleles_push_device(tdt_alleles *h, const void *const *d_arrays14, size_t n, size_t raw_len);
int tdt_alleles_push(tdt_alleles *h, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint8_t *mapq, const uint16_t *flag,
                     const uint64_t *rec_off, size_t n, const uint8_t *raw, size_t raw_len);
int tdt_alleles_counts(tdt_alleles *h, uint32_t *out, uint64_t *reads_used, uint64_t *malformed);
int tdt_alleles_counts_device(tdt_alleles *h, uint32_t *d_out, uint64_t *d_stat2);

/* ---- read-backed phasing of the known SNV sites (TIDDIT_PHASE) ------------------------------------------ *
 * No counterpart in the reference; the definition is tiddit_amd/tiddit_phase.py's.  tdt_alleles_phase_enable gives an allele handle a
 * store of observation keys beside its counters: every push of the handle then costs one more launch (phase_keys) on the batch it has
 * just counted.  site_codes = one byte per device site, ref2 | alt2 << 2 (A C G T = 0 1 2 3) or 0xff for a site that is not phaseable;
 * a read's first TDT_PHASE_MAX_OBS observations give the keys K1 = FNV-1a-64(read name) & (2^hash_bits - 1), K2 = site << 1 | allele.
 * Enabled twice, behind a push, or with n_sites that is not the handle's: TDT_E_ARG; hash_bits outside 1 ... 64, min_q outside 0 ... 255:
 * TDT_E_RANGE.  tdt_alleles_reset empties the store too.
 * tdt_alleles_phase_finish(het_flags: HOST, one byte per site; min_link = S): the fragment rows, the links between consecutive clean
 * heterozygous rows of a fragment, the link rows (N, TRANS) in (j, i) order, the maximum spanning forest of the eligible links, the check
 * of the others.  got[TDT_PHASE_GOT_N] = malformed reads_used observations capped_reads | fragment_rows discordant_rows
 * cross_contig_pairs links weak_links forest_edges agree conflict phased_sites blocks | the Boruvka rounds run.  The stores are left as
 * they were.  The read-outs give the last finish: per site (root = the block's lowest site or -1, phase), the blocks (first site, last
 * site, sites, eligible links, agree, conflict; ascending), the link rows with their forest flag; a push or reset since: TDT_E_ARG; too
 * little room (*n in = room, out = count; all-NULL arrays ask for the count alone): TDT_E_RANGE, nothing written.  Every entry without
 * tdt_alleles_phase_enable: TDT_E_ARG.
 * tdt_phase_forest: the graph stage alone on ANY link rows (j, i, N, TRANS; row = the index) over n_sites sites: root int32[n_sites],
 * phase uint8[n_sites], edge_used uint8[n_links], agree / conflict uint32[n_sites] at each block's lowest site.  An end outside
 * [0, n_sites), two equal ends or TRANS > N: TDT_E_ARG; 2^31 sites or links or more, min_link outside 1 ... 2^31 - 1: TDT_E_RANGE. */
#define TDT_PHASE_MAX_OBS 8
#define TDT_PHASE_PUSH_N 4
#define TDT_PHASE_GOT_N 15
int tdt_alleles_phase_enable(tdt_alleles *h, const uint8_t *site_codes, size_t n_sites, size_t capacity, int hash_bits);
int tdt_alleles_phase_keys(tdt_alleles *h, uint64_t *k1, uint64_t *k2, size_t *n);
int tdt_alleles_phase_finish(tdt_alleles *h, const uint8_t *het_flags, uint64_t min_link, uint64_t *got);
int tdt_alleles_phase_sites(tdt_alleles *h, int32_t *root, uint8_t *phase, size_t n);
int tdt_alleles_phase_blocks(tdt_alleles *h, int32_t *start, int32_t *end, uint32_t *sites, uint32_t *edges, uint32_t *agree, uint32_t *conflict,
                             size_t *n);
int tdt_alleles_phase_links(tdt_alleles *h, uint32_t *j, uint32_t *i, uint32_t *n_, uint32_t *trans, uint8_t *edge_used, size_t *n);
int tdt_alleles_phase_timing(tdt_alleles *h, double *ms5);
int tdt_alleles_phase_reserve_stats(tdt_alleles *h, uint64_t *out3);
int tdt_phase_forest(tdt_ctx *ctx, const int32_t *j, const int32_t *i, const uint32_t *n, const uint32_t *trans, size_t n_links, size_t n_sites,
                     uint64_t min_link, int32_t *root, uint8_t *phase, uint8_t *edge_used, uint32_t *agree, uint32_t *conflict);
int tdt_phase_forest_device(tdt_ctx *ctx, const int32_t *d_j, const int32_t *d_i, const uint32_t *d_n, const uint32_t *d_trans, size_t n_links,
                            size_t n_sites, uint64_t min_link, int32_t *d_root, uint8_t *d_phase, uint8_t *d_edge_used, uint32_t *d_agree,
                            uint32_t *d_conflict);

/* ---- read-level QC tables (TIDDIT_QC) ------------------------------------------------------------------ *
 * No counterpart in the reference (its users run `samtools flagstat` / `samtools stats`, one more pass over the file); the definition
 * is tiddit_amd/tiddit_qc.py's.  A handle keeps ONE array of TDT_QC_TOTAL zeroed uint64 counters in HBM, in sections (row-major):
 *   SN    [TDT_QC_SN_N]   records secondary supplementary | primary qc_fail duplicate unmapped mapped paired read1 read2 proper_pair
 *                         mate_unmapped both_mapped mate_other_contig mate_other_contig_mapq5 reverse mapq0 | malformed bases
 *                         reads_no_seq reads_no_qual bases_q20 bases_q30 aligned_bases soft_clipped_bases hard_clipped_bases
 *                         inserted_bases deleted_bases skipped_bases insertions deletions reads_clipped
 *   MAPQ  [256]           mapped primary records by mapq
 *   RL    [512 + 1]       records with flag & 0xB00 == 0 ("S") by min(l_seq, 512)
 *   IS    [2000 + 1][3]   S, paired, both mapped, mate_tid == tid, tlen > 0, by min(tlen, 2000): inward outward same
 *   CYC   [512 + 1][7]    per cycle (read orientation; the cycles from 512 share the last row): A C G T other qual_sum qual_n
 *   QUAL  [256]           every quality byte of the reads with qualities
 *   GCR   [101]           reads with l_seq > 0 by (100 * gc) / l_seq
 *   ID    [64][2]         insertion / deletion events of the mapped reads by min(len, 64) - 1
 * SN up to mapq0, MAPQ, RL and IS come from the field columns alone.  Everything else is read from the bytes of the records of S, each
 * bounded first as tdt_alleles bounds one (rec_off + 36 <= raw_len, 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <=
 * block_size, rec_off + 4 + block_size <= raw_len; l_seq is the record's own): a record that fails, or holds a CIGAR op code above 8,
 * adds one to `malformed` and nothing else from its bytes; nothing outside [raw, raw + raw_len) is ever read.
 * tdt_qc_push_device takes the pointer table tdt_ingest_arrays filled (TDT_COL_*), enqueues two launches on the context's stream, waits for nothing
 * and allocates nothing; tdt_qc_push uploads host columns, runs the same kernels and returns when they are done.  Refusals: TDT_E_ARG
 * (null pointers, record offsets that decrease, n >= 2^31, a misaligned device output); a refused call leaves its outputs untouched.
 * The read-out calls synchronise the stream.  tdt_qc_size() = TDT_QC_TOTAL. */
#define TDT_QC_SN_N 33
#define TDT_QC_OFF_SN 0
#define TDT_QC_OFF_MAPQ 33
#define TDT_QC_OFF_RL 289
#define TDT_QC_OFF_IS 802
#define TDT_QC_OFF_CYC 6805
#define TDT_QC_OFF_QUAL 10396
#define TDT_QC_OFF_GCR 10652
#define TDT_QC_OFF_ID 10753
#define TDT_QC_TOTAL 10881
typedef struct tdt_qc tdt_qc;
int tdt_qc_create(tdt_ctx *ctx, tdt_qc **out);
int tdt_qc_destroy(tdt_qc *h);
int tdt_qc_reset(tdt_qc *h);
int tdt_qc_push_device(tdt_qc *h, const void *const *d_arrays14, size_t n, size_t raw_len);
int tdt_qc_push(tdt_qc *h, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *mate_tid, const int32_t *tlen,
                const int32_t *l_seq, const uint64_t *rec_off, size_t n, const uint8_t *raw, size_t raw_len);
int tdt_qc_counts(tdt_qc *h, uint64_t *out);
int tdt_qc_counts_device(tdt_qc *h, uint64_t *d_out);
size_t tdt_qc_size(void);

/* ---- duplicate metrics and library size (TIDDIT_DUPS) -------------------------------------------------- *
 * No counterpart in the reference (its users run Picard MarkDuplicates / samtools markdup, one more pass over the file); the
 * definition is tiddit_amd/tiddit_dup.py's.  A handle keeps a store of keys in HBM — per keyed read K1 = tid << 34 | E << 1 | rev,
 * K2 = 0 (a fragment) or 1 << 58 | mate_tid << 34 | ME << 1 | mrev (the carrier of a pair), and the read's 0x400 bit — and ONE array of
 * TDT_DUP_TOTAL uint64 counters (row-major):
 *   SN    [TDT_DUP_SN_N]  records eligible malformed fragments pairs pair_mates pairs_no_mc flagged | fragment_sets pair_sets
 *                         fragment_duplicates pair_duplicates
 *   HIST  [1024][2]       sets of equal (K1, K2) by min(size, 1024) - 1: pair_sets fragment_sets
 * A push adds one batch of reads, one launch: eligibility (flag & 0xB04 == 0, tid >= 0) and the carrier rule are tested on the field
 * columns; a fragment or carrier has its record bounded as tdt_alleles bounds one (rec_off + 36 <= raw_len, 32 + l_read_name +
 * 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size, rec_off + 4 + block_size <= raw_len), its CIGAR walked for the clip sums and, a
 * carrier, its aux fields for the first MC:Z.  A record that fails the bounds, holds an op code above 8, a contig id of 2^24 or more, or
 * an end outside [0, 2^33) after the bias of 2^28 adds one to `malformed` and gets no key; nothing outside [raw, raw + raw_len) is ever
 * read.  The store grows by itself (1.5 x) and is in stream order, not file order.  tdt_dup_push_device takes the pointer table
 * tdt_ingest_arrays filled (TDT_COL_*), enqueues the launch on the context's stream and waits for nothing unless the store must grow; tdt_dup_push
 * uploads host columns, runs the same kernel and returns when it is done.  tdt_dup_finish sorts the store (two stable radix sorts and a
 * gather), measures the runs of equal keys and returns the whole counter array; the store is left as it was, so pushes may go on and a
 * second finish gives the same answer.  tdt_dup_keys reads the store out (*n in: room of the arrays, out: keys stored; all three arrays
 * NULL: the count alone).  tdt_dup_timing: device milliseconds of the last finish (sort by K2, gather, sort by K1, run lengths).
 * Refusals: TDT_E_ARG (null pointers, record offsets that decrease, n >= 2^31), TDT_E_RANGE (more than 2^24 contigs, too little room
 * in tdt_dup_keys, 2^30 keys or more at the finish: the sort's limit); a refused call leaves its outputs untouched.  The read-out calls
 * synchronise the stream.  tdt_dup_size() = TDT_DUP_TOTAL. */
#define TDT_DUP_SN_N 12
#define TDT_DUP_OFF_HIST 12
#define TDT_DUP_HIST_MAX 1024
#define TDT_DUP_TOTAL 2060
typedef struct tdt_dup tdt_dup;
int tdt_dup_create(tdt_ctx *ctx, int n_contigs, int64_t max_contig_len, size_t capacity, tdt_dup **out);
int tdt_dup_destroy(tdt_dup *h);
int tdt_dup_reset(tdt_dup *h);
int tdt_dup_push_device(tdt_dup *h, const void *const *d_arrays14, size_t n, size_t raw_len);
int tdt_dup_push(tdt_dup *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const int32_t *end, const int32_t *mate_tid,
                 const int32_t *mate_pos, const uint64_t *rec_off, size_t n, const uint8_t *raw, size_t raw_len);
int tdt_dup_keys(tdt_dup *h, uint64_t *k1, uint64_t *k2, uint8_t *marked, size_t *n);
int tdt_dup_finish(tdt_dup *h, uint64_t *out);
int tdt_dup_timing(tdt_dup *h, double *ms4);
size_t tdt_dup_size(void);

/* ---- small-indel candidates (TIDDIT_INDELS) ------------------------------------------------------------ *
 * No counterpart in the reference (its signals start at discordant pairs and split reads); the definition is
 * tiddit_amd/tiddit_indels.py's.  A handle keeps a store of keys in HBM — per keyed event (a flanked I or D operation of an eligible
 * read's CIGAR, 1 <= len < TDT_INDEL_MAX_LEN) K1 = tid << 32 | P and K2 = type << 63 | len << 47 | kind << 45 | payload << 1 | rev —
 * and TDT_INDEL_SN_N uint64 counters:
 *   SN    records eligible malformed unanchored too_long noisy_reads reads_with_events insertions deletions | distinct_events
 *         reported_events
 * A push adds one batch of reads, one launch: eligibility (flag & 0xF04 == 0, tid >= 0, mapq >= min_mapq) is tested on the field
 * columns; an eligible read has its record bounded as tdt_dup bounds one and its CIGAR walked once.  A record that fails the bounds,
 * holds an op code above 8, has a tid of 2^24 or more, a negative pos, or a keyed event with P outside [1, 2^31) adds one to `malformed`
 * and gives nothing else; a read with more than TDT_INDEL_MAX_PER_READ keyed events adds one to `noisy_reads` and gives no key; nothing
 * outside [raw, raw + raw_len) is ever read.  The store grows by itself (1.5 x) and is in stream order, not file order: before each
 * launch room for TDT_INDEL_MAX_PER_READ keys per read is reserved, and a reserve that does not fit first asks the device how many keys
 * there really are.  tdt_indel_push_device takes the pointer table tdt_ingest_arrays filled (TDT_COL_*), enqueues the launch on the
 * context's stream and waits for nothing unless the reserve must ask or grow; tdt_indel_push uploads host columns, runs the same kernel
 * and returns when it is done.  tdt_indel_finish sorts the store (two stable radix sorts and a gather), measures the runs of equal
 * (K1, K2 >> 1) — SUPPORT their size, REV the members with bit 0 set — fills sn_out[TDT_INDEL_SN_N] and keeps the runs with SUPPORT >=
 * min_support as rows, ascending by key; the store is left as it was, so pushes may go on and another finish, with any min_support,
 * gives the definition's answer.  tdt_indel_rows reads those rows out (K1, K2 with bit 0 clear, SUPPORT, REV; *n in: room of the arrays,
 * out: rows; all four arrays NULL: the count alone); tdt_indel_keys the store (the same convention).  tdt_indel_timing: device
 * milliseconds of the last finish (sort by K2, gather, sort by K1, run lengths and rows).  tdt_indel_reserve_stats: out3 = how often
 * the reserve asked the device, how often the store grew, its capacity now.
 * Refusals: TDT_E_ARG (null pointers, record offsets that decrease, n >= 2^31, tdt_indel_rows without a finish since the last push or
 * reset), TDT_E_RANGE (more than 2^24 contigs, min_mapq outside 0 ... 255, min_support outside 1 ... TDT_INDEL_MAX_SUPPORT, too little
 * room in tdt_indel_keys / tdt_indel_rows, 2^30 keys or more at the finish: the sort's limit); a refused call leaves its outputs
 * untouched.  The read-out calls synchronise the stream.  tdt_indel_sn_size() = TDT_INDEL_SN_N. */
#define TDT_INDEL_SN_N 11
#define TDT_INDEL_MAX_PER_READ 4
#define TDT_INDEL_MAX_LEN 65536
#define TDT_INDEL_MAX_SUPPORT 1000000
typedef struct tdt_indel tdt_indel;
int tdt_indel_create(tdt_ctx *ctx, int n_contigs, int min_mapq, size_t capacity, tdt_indel **out);
int tdt_indel_destroy(tdt_indel *h);
int tdt_indel_reset(tdt_indel *h);
int tdt_indel_push_device(tdt_indel *h, const void *const *d_arrays14, size_t n, size_t raw_len);
int tdt_indel_push(tdt_indel *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off,
                   size_t n, const uint8_t *raw, size_t raw_len);
int tdt_indel_keys(tdt_indel *h, uint64_t *k1, uint64_t *k2, size_t *n);
int tdt_indel_finish(tdt_indel *h, uint64_t min_support, uint64_t *sn_out, size_t *n_rows);
int tdt_indel_rows(tdt_indel *h, uint64_t *k1, uint64_t *k2, uint32_t *support, uint32_t *rev, size_t *n);
int tdt_indel_timing(tdt_indel *h, double *ms4);
int tdt_indel_reserve_stats(tdt_indel *h, uint64_t *out3);
size_t tdt_indel_sn_size(void);

/* ---- the resident reference sequence ------------------------------------------------------------------ *
 * The reference in HBM for the kernels of the --sv scan that need it (csrc/tdt_refseq.hip).  A handle owns ONE buffer of 4-bit base
 * codes, BAM's own ("=ACMGRSVTWYHKDBN"), two bases per byte with the even base in the high nibble — a record's sequence layout, so a
 * read's nibble and a reference nibble compare directly — and a table of every contig's byte offset and length.  Every contig starts on
 * an 8-byte boundary and has at least 8 zero bytes in front of it and behind it: code 0 is no base, a comparison that runs off a contig
 * stops there, and whole 64-bit words can be loaded at either end without a bounds branch.  The lengths are fixed by tdt_refseq_create
 * (each 0 ... 2^31 - 1, at most 2^24 contigs); the store is allocated and zeroed there.
 * tdt_refseq_load_fasta packs ONE contig from host bytes exactly as they are in the FASTA file (line ends included, LF or CRLF:
 * `linebases` bases and `linewidth` bytes per full line, the .fai columns; the layouts tdt_gc_bins_fasta_device takes, TDT_E_UNSUPPORTED
 * for the others): uploaded, packed by one launch (a lane = 16 bases = one 64-bit store), the staging buffer freed.
 * tdt_refseq_load_fasta_device does the same on caller-owned device bytes.  Letters map to their code in either case, every other byte
 * to 15 (N).  Both return when the contig is packed.  tdt_refseq_fetch: n codes from base `start` on, one per output byte.
 * tdt_refseq_layout: out3 = the store's bytes, the guard bytes between contigs, the bases one workgroup of the pack kernel takes;
 * offsets (or NULL): every contig's byte offset; store_out (or NULL): the whole store, room for out3[0] bytes.
 * Refusals, TDT_E_ARG: null pointers, a tid outside the table, a length that differs from the one given at create, a contig loaded
 * twice, too few bytes for the length, a fetch outside the contig or of a contig that is not loaded, a contig of 2^31 bases or more.
 * A refused call leaves its outputs and the store untouched. */
typedef struct tdt_refseq tdt_refseq;
int tdt_refseq_create(tdt_ctx *ctx, int n_contigs, const int64_t *lengths, tdt_refseq **out);
int tdt_refseq_destroy(tdt_refseq *h);
int tdt_refseq_load_fasta(tdt_refseq *h, int tid, const uint8_t *raw, int64_t nbytes, int64_t length, int linebases, int linewidth);
int tdt_refseq_load_fasta_device(tdt_refseq *h, int tid, const uint8_t *d_raw, int64_t nbytes, int64_t length, int linebases, int linewidth);
int tdt_refseq_fetch(tdt_refseq *h, int tid, int64_t start, int64_t n, uint8_t *codes_out);
int tdt_refseq_layout(tdt_refseq *h, uint64_t *out3, uint64_t *offsets, uint8_t *store_out);
/* tests only: the store words of a contig that is not loaded yet (never a guard byte) filled with `byte` — a load behind it must
 * overwrite every nibble of them.  TDT_E_ARG: a tid outside the table, a contig that is loaded. */
int tdt_debug_refseq_fill(tdt_refseq *h, int tid, int byte);

/* ---- small-indel candidates, left-normalised (TIDDIT_INDELS_NORM) -------------------------------------- *
 * tdt_indel_set_reference attaches a resident reference to a tdt_indel handle (NULL detaches it; the reference is not owned, must lie
 * on the handle's device and outlive the attachment).  With one attached, a push moves every keyed event of an OK read as far left as
 * the reference allows before its keys are made — tiddit_amd/tiddit_indels.py: left_normalise; at most TDT_INDEL_NORM_MAX_SHIFT bases,
 * never to a P below 1, only across A C G T — and an insertion's payload is that of the rotated allele.  Without one the push is the
 * kernel it always was.  tdt_indel_norm_stats: out3 = events shifted, shifts that stopped at the cap, events off the reference (contig
 * not loaded, or the event reaches beyond the contig's end: key unchanged), since the last reset; it synchronises the stream.  The
 * eleven SN counters, the store, the finish and the rows are unchanged.  TDT_E_ARG: null pointers, a reference of another device. */
#define TDT_INDEL_NORM_MAX_SHIFT 1024
int tdt_indel_set_reference(tdt_indel *h, tdt_refseq *ref);
int tdt_indel_norm_stats(tdt_indel *h, uint64_t *out3);

/* ---- tandem repeats at known loci (TIDDIT_STR) --------------------------------------------------------------- *
 * The repeat lengths the reads of the --sv scan show at the loci of a catalogue (csrc/tdt_str.hip); the definition is
 * tiddit_amd/tiddit_str.py's.  A handle keeps the loci table in HBM — lstart / lend: int32, 0-based half-open, contig-major, per contig
 * 1 <= start < end and start >= the end in front + 1, so both ascend; motif: one uint32 per locus, the motif's length m (1 ...
 * TDT_STR_MAX_MOTIF) in bits 0 ... 3 and the BAM 4-bit code (1 2 4 8) of its letter i in bits 4 + 4 i ...; loc_off: int64[n_contigs + 1],
 * loc_off[0] == 0 — and a store of keys: per (eligible read, one of the first TDT_STR_MAX_PER_READ loci in its reach) with an outcome
 * K1 = the locus index and K2 = kind << 33 | L << 1 | rev (kind 0: the read spans the locus with `flank` aligned bases on both sides,
 * L = the query bases between the two anchor bases; 1 / 2: anchored on the left, L = how far the read's bases repeat the motif behind
 * the anchor, closed / open at the read's end; 3 / 4: the same from the right anchor leftwards), and TDT_STR_SN_N uint64 push
 * counters: records, eligible, in_reach, malformed, no_alignment, no_sequence, span_keys, left_keys, right_keys, unanchored, over_cap.
 * A read with no locus in reach never has its bytes looked at; nothing outside raw[0, raw_len) is ever read.  Before every launch room
 * for TDT_STR_MAX_PER_READ keys per read is reserved.  tdt_str_push_device takes the pointer table tdt_ingest_arrays filled (TDT_COL_*;
 * it reads the END column beside the keyed consumers' six), enqueues the launch on the context's stream and waits for nothing unless
 * the reserve must ask or grow; tdt_str_push uploads host columns, runs the same kernel and returns when it is done.  tdt_str_finish
 * sorts the store and measures the runs of equal (K1, K2 >> 1) as tdt_indel_finish does, fills sn_out[TDT_STR_SN_N] and keeps EVERY
 * set as a row (it has no reporting threshold); the store is left as it was.  tdt_str_rows / _keys / _timing / _reserve_stats: as
 * tdt_indel's.  Refusals: TDT_E_ARG (null pointers, loc_off[0] != 0 or offsets that decrease, loci that break the table's rules, a
 * motif outside its form, record offsets that decrease, n >= 2^31, tdt_str_rows without a finish since the last push or reset),
 * TDT_E_RANGE (more than 2^24 contigs or loci, flank outside 1 ... TDT_STR_MAX_FLANK, min_mapq outside 0 ... 255, too little room in
 * tdt_str_keys / tdt_str_rows, 2^30 keys or more at the finish); a refused call leaves its outputs untouched.  The read-out calls
 * synchronise the stream.  tdt_str_sn_size() = TDT_STR_SN_N. */
#define TDT_STR_SN_N 11
#define TDT_STR_MAX_PER_READ 4
#define TDT_STR_MAX_MOTIF 6
#define TDT_STR_MAX_FLANK 100
#define TDT_STR_MAX_LOCI (1 << 24)
typedef struct tdt_str tdt_str;
int tdt_str_create(tdt_ctx *ctx, const int32_t *lstart, const int32_t *lend, const uint32_t *motif, const int64_t *loc_off, int n_contigs,
                   int flank, int min_mapq, size_t capacity, tdt_str **out);
int tdt_str_destroy(tdt_str *h);
int tdt_str_reset(tdt_str *h);
int tdt_str_push_device(tdt_str *h, const void *const *d_arrays14, size_t n, size_t raw_len);
int tdt_str_push(tdt_str *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint8_t *mapq,
                 const uint64_t *rec_off, size_t n, const uint8_t *raw, size_t raw_len);
int tdt_str_keys(tdt_str *h, uint64_t *k1, uint64_t *k2, size_t *n);
int tdt_str_finish(tdt_str *h, uint64_t *sn_out, size_t *n_rows);
int tdt_str_rows(tdt_str *h, uint64_t *k1, uint64_t *k2, uint32_t *support, uint32_t *rev, size_t *n);
int tdt_str_timing(tdt_str *h, double *ms4);
int tdt_str_reserve_stats(tdt_str *h, uint64_t *out3);
size_t tdt_str_sn_size(void);

/* ---- SNV candidates (TIDDIT_SNVS) ------------------------------------------------------------------------ *
 * Every position where eligible reads carry a base that differs from the resident reference (csrc/tdt_snv.hip); the definition is
 * tiddit_amd/tiddit_snvs.py's.  A handle keeps a store of keys in HBM — per keyed event (an M / = / X base of an eligible read whose
 * 4-bit code and the reference's are both one of A C G T and differ, with a quality of at least min_bq or the absent-quality byte 0xff)
 * K1 = tid << 32 | P (1-based) and K2 = ref2 << 3 | alt2 << 1 | rev, A C G T = 0 1 2 3 — and TDT_SNV_SN_N uint64 counters:
 *   [0] records  [1] eligible  [2] malformed  [3] no_sequence  [4] off_reference  [5] aligned_bases  [6] low_quality  [7] noisy_reads
 *   [8] reads_with_events  [9] mismatches  [10] distinct_events  [11] reported_events
 * A record is eligible when flag & 0xF04 == 0, tid >= 0 and mapq >= min_mapq; the bytes of the others are never read.  A malformed
 * record (the record bound of tdt_indel fails, an op code above 8, tid >= 2^24, pos < 0, pos + the CIGAR's reference length above
 * 2^31 - 1, a CIGAR whose query length differs from l_seq when both are given) adds one to `malformed` and gives nothing else; one
 * without CIGAR or sequence counts as `no_sequence`; one on a contig that is not loaded or reaching beyond its end as `off_reference`; a
 * read with more than TDT_SNV_MAX_PER_READ keyed events adds one to `noisy_reads` and gives no key.  Nothing outside raw[0, raw_len) is
 * ever read.  The reference (tdt_refseq) is given at create, is not owned, must lie on the context's device and outlive the handle.
 * `capacity` is the store's first size in keys; it grows (1.5 x).  Before each launch room for TDT_SNV_MAX_PER_READ keys per read is
 * reserved — 128 bytes of store per read of a batch, held as headroom — and a reserve that does not fit first asks the device how many
 * keys there really are.  tdt_snv_push_device takes the pointer table tdt_ingest_arrays filled (TDT_COL_*), enqueues the launch on the
 * context's stream and waits for nothing unless the reserve must ask or grow; tdt_snv_push uploads host columns, runs the same kernel
 * and returns when it is done.  tdt_snv_finish sorts the store (two stable radix sorts and a gather: the finish of tdt_indel_finish),
 * measures the runs of equal (K1, K2 >> 1) — SUPPORT their size, REV the members with bit 0 set — fills sn_out[TDT_SNV_SN_N] and keeps
 * the runs with SUPPORT >= min_support as rows in key order; the store is left as it was.  tdt_snv_rows reads those rows out (K1, K2
 * with bit 0 clear, SUPPORT, REV; *n in: room of the arrays, out: rows; all four arrays NULL: the count alone); tdt_snv_keys the store
 * (the same convention).  tdt_snv_timing: device milliseconds of the last finish (sort by K2, gather, sort by K1, run lengths and
 * rows).  tdt_snv_reserve_stats: out3 = how often the reserve asked, how often the store grew, its capacity now.
 * Refusals: TDT_E_ARG (null pointers, a reference of another device, record offsets that decrease, n >= 2^31, tdt_snv_rows without a
 * finish since the last push or reset), TDT_E_RANGE (more than 2^24 contigs, min_mapq outside 0 ... 255, min_bq outside 0 ...
 * TDT_SNV_MAX_BQ, min_support outside 1 ... TDT_SNV_MAX_SUPPORT, too little room in tdt_snv_keys / tdt_snv_rows, 2^30 keys or more at
 * the finish: the sort's limit); a refused call leaves its outputs untouched.  The read-out calls synchronise the stream.
 * tdt_snv_sn_size() = TDT_SNV_SN_N. */
#define TDT_SNV_SN_N 12
#define TDT_SNV_MAX_PER_READ 8
#define TDT_SNV_MAX_BQ 93
#define TDT_SNV_MAX_SUPPORT 1000000
typedef struct tdt_snv tdt_snv;
int tdt_snv_create(tdt_ctx *ctx, int n_contigs, int min_mapq, int min_bq, size_t capacity, tdt_refseq *ref, tdt_snv **out);
int tdt_snv_destroy(tdt_snv *h);
int tdt_snv_reset(tdt_snv *h);
int tdt_snv_push_device(tdt_snv *h, const void *const *d_arrays14, size_t n, size_t raw_len);
int tdt_snv_push(tdt_snv *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off,
                 size_t n, const uint8_t *raw, size_t raw_len);
int tdt_snv_keys(tdt_snv *h, uint64_t *k1, uint64_t *k2, size_t *n);
int tdt_snv_finish(tdt_snv *h, uint64_t min_support, uint64_t *sn_out, size_t *n_rows);
int tdt_snv_rows(tdt_snv *h, uint64_t *k1, uint64_t *k2, uint32_t *support, uint32_t *rev, size_t *n);
int tdt_snv_timing(tdt_snv *h, double *ms4);
int tdt_snv_reserve_stats(tdt_snv *h, uint64_t *out3);
size_t tdt_snv_sn_size(void);

/* ---- clipped-read breakpoint sites (TIDDIT_CLIPS) -------------------------------------------------------- *
 * Every reference position where eligible reads are soft-clipped on one side, with a consensus of the clipped bases beside the
 * breakpoint (csrc/tdt_clip.hip); the definition is tiddit_amd/tiddit_clips.py's.  A handle keeps a store of keys in HBM — per clip of at
 * least min_clip bases (the S at CIGAR index 0, or 1 behind an H; the S at the last index, or the last but one in front of an H)
 * K1 = tid << 32 | P (1-based: the first aligned base for a leading clip, the last for a trailing one) and
 * K2 = side << 63 | n << 58 | bases << 2 | rev, `bases` the first n <= TDT_CLIP_COLS clipped bases outward from the breakpoint, two bits
 * each, A C G T = 0 1 2 3, cut at the first other code — and TDT_CLIP_SN_N uint64 counters:
 *   [0] records  [1] eligible  [2] malformed  [3] no_sequence  [4] no_alignment  [5] short_clips  [6] left_clips  [7] right_clips
 *   [8] clipped_reads  [9] cut_at_other_base  [10] distinct_sequences  [11] distinct_sites  [12] reported_sites
 * ([10] ... [12] are the finish's).  Eligible: flag & 0xF04 == 0, tid >= 0, mapq >= min_mapq.  An eligible record is bounded and judged
 * malformed exactly as tdt_snv does it; one without CIGAR or sequence counts as `no_sequence`, one whose CIGAR has a reference length
 * of 0 as `no_alignment`.  Nothing outside raw[0, raw_len) is ever read.  `capacity` is the store's first size in keys; it grows
 * (1.5 x).  Before each launch room for TDT_CLIP_MAX_PER_READ keys per read is reserved, and a reserve that does not fit first asks the
 * device how many keys there really are.  tdt_clip_push_device takes the pointer table tdt_ingest_arrays filled (TDT_COL_*), enqueues
 * the launch on the context's stream and waits for nothing unless the reserve must ask or grow; tdt_clip_push uploads host columns, runs
 * the same kernel and returns when it is done.  tdt_clip_finish sorts the store (the finish of tdt_snv_finish, with a minimum support
 * of 1: its rows are the distinct sequences (K1, K2 >> 1)), finds the sites — runs of equal (K1, side) — and per site SUPPORT, REV, SEQS
 * and a vote per column: depth_j = the events with n > j, CLEN = the leading columns with depth_j >= min_support, the consensus base of
 * a column the one with the most votes (a tie to the smaller code), AGREE / TOTAL the winning votes / the depths summed over the CLEN
 * columns.  It fills sn_out[TDT_CLIP_SN_N] and keeps the sites with SUPPORT >= min_support as rows in key order; the store is left as it
 * was.  tdt_clip_rows reads those rows out (K1, side, SUPPORT, REV, SEQS, CLEN, the consensus packed like `bases`, AGREE, TOTAL; *n in:
 * room of the arrays, out: rows; all nine arrays NULL: the count alone); tdt_clip_keys the store (the same convention).
 * tdt_clip_timing: device milliseconds of the last finish (sort by K2, gather, sort by K1, run lengths and rows, the site launches).
 * tdt_clip_reserve_stats: out3 = how often the reserve asked, how often the store grew, its capacity now.
 * Refusals: TDT_E_ARG (null pointers, record offsets that decrease, n >= 2^31, tdt_clip_rows without a finish since the last push or
 * reset), TDT_E_RANGE (more than 2^24 contigs, min_mapq outside 0 ... 255, min_clip outside 1 ... TDT_CLIP_MAX_CLIP, min_support outside
 * 1 ... TDT_CLIP_MAX_SUPPORT, too little room in tdt_clip_keys / tdt_clip_rows, 2^30 keys or more at the finish: the sort's limit); a
 * refused call leaves its outputs untouched.  The read-out calls synchronise the stream.  tdt_clip_sn_size() = TDT_CLIP_SN_N. */
#define TDT_CLIP_SN_N 13
#define TDT_CLIP_MAX_PER_READ 2
#define TDT_CLIP_COLS 28
#define TDT_CLIP_MAX_CLIP 65535
#define TDT_CLIP_MAX_SUPPORT 1000000
typedef struct tdt_clip tdt_clip;
int tdt_clip_create(tdt_ctx *ctx, int n_contigs, int min_mapq, int min_clip, size_t capacity, tdt_clip **out);
int tdt_clip_destroy(tdt_clip *h);
int tdt_clip_reset(tdt_clip *h);
int tdt_clip_push_device(tdt_clip *h, const void *const *d_arrays14, size_t n, size_t raw_len);
int tdt_clip_push(tdt_clip *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off,
                  size_t n, const uint8_t *raw, size_t raw_len);
int tdt_clip_keys(tdt_clip *h, uint64_t *k1, uint64_t *k2, size_t *n);
int tdt_clip_finish(tdt_clip *h, uint64_t min_support, uint64_t *sn_out, size_t *n_rows);
int tdt_clip_rows(tdt_clip *h, uint64_t *k1, uint32_t *side, uint32_t *support, uint32_t *rev, uint32_t *seqs, uint32_t *clen, uint64_t *consensus,
                  uint64_t *agree, uint64_t *total, size_t *n);
int tdt_clip_timing(tdt_clip *h, double *ms5);
int tdt_clip_reserve_stats(tdt_clip *h, uint64_t *out3);
size_t tdt_clip_sn_size(void);

/* ---- clip-site consensus realigned to the reference (TIDDIT_CLIPS_ALIGN) ---------------------------------- *
 * For every clip site (K1 = tid << 32 | P, side 0 = L / 1 = R, CLEN, the consensus packed as tdt_clip_rows gives it) the best exact
 * placement of its CLEN consensus bases on the same contig of a tdt_refseq within W bases of P, on either strand
 * (csrc/tdt_clip_align.hip); the definition is tiddit_amd/tiddit_clip_align.py's.  Per site five uint32: status (0 short_consensus:
 * CLEN < K; 1 off_reference: the contig is outside the table or not loaded, or P outside 1 ... len; 2 searched), PARTNER (the best
 * candidate's Q, 1-based), strand (0 forward, 1 reverse complement), its mismatches, and HITS (the candidates with at most M
 * mismatches).  The best candidate is the minimum of (mismatches, |Q - P|, strand, Q); a searched site without any candidate, and a
 * site that is not searched, has PARTNER 0, strand 0, mismatches 0xffffffff and HITS 0.  A CLEN above TDT_CLIP_COLS is taken as
 * TDT_CLIP_COLS, of the side only bit 0.  tdt_clip_align_sites takes host arrays of n sites, tdt_clip_align_sites_device caller-owned
 * device arrays; both return when the kernel is done.  tdt_clip_align searches the rows of the handle's last tdt_clip_finish where they
 * lie in HBM, keeps the five columns on the device for tdt_clip_align_rows (*n in: room of the arrays, out: rows; all five NULL: the
 * count alone) and fills sn_out[TDT_CLIP_ALIGN_SN_N]:
 *   [0] sites  [1] short_consensus  [2] off_reference  [3] searched  [4] aligned  [5] ambiguous  [6] unaligned  [7] ref  [8] del
 *   [9] dup  [10] inv  [11] mated (always 0 here: mates are the host's, rule 5 of the definition)
 * tdt_clip_align_timing: device milliseconds of the last tdt_clip_align's kernel.  The reference is not owned and must lie on the
 * context's device.  Refusals: TDT_E_ARG (null pointers, n >= 2^31, a reference of another device, for the handle a reference with
 * another contig count, tdt_clip_align without a finish since the last push or reset, tdt_clip_align_rows / _timing without a
 * tdt_clip_align since then), TDT_E_RANGE (W outside 1 ... TDT_CLIP_ALIGN_MAX_WINDOW, K outside 1 ... TDT_CLIP_COLS, M outside
 * 0 ... TDT_CLIP_COLS - 1, too little room in tdt_clip_align_rows); a refused call leaves its outputs untouched. */
#define TDT_CLIP_ALIGN_SN_N 12
#define TDT_CLIP_ALIGN_MAX_WINDOW (1 << 20)
int tdt_clip_align_sites(tdt_ctx *ctx, tdt_refseq *ref, size_t n, const uint64_t *k1, const uint32_t *side, const uint32_t *clen, const uint64_t *consensus,
                         int W, int K, int M, uint32_t *status_out, uint32_t *partner_out, uint32_t *strand_out, uint32_t *mm_out, uint32_t *hits_out);
int tdt_clip_align_sites_device(tdt_ctx *ctx, tdt_refseq *ref, size_t n, const uint64_t *d_k1, const uint32_t *d_side, const uint32_t *d_clen,
                                const uint64_t *d_consensus, int W, int K, int M, uint32_t *d_status, uint32_t *d_partner, uint32_t *d_strand,
                                uint32_t *d_mm, uint32_t *d_hits);
int tdt_clip_align(tdt_clip *h, tdt_refseq *ref, int W, int K, int M, uint64_t *sn_out);
int tdt_clip_align_rows(tdt_clip *h, uint32_t *status, uint32_t *partner, uint32_t *strand, uint32_t *mm, uint32_t *hits, size_t *n);
int tdt_clip_align_timing(tdt_clip *h, double *ms);

/* ---- clip-site consensus placed genome-wide by a seeded search (TIDDIT_CLIPS_FAR) -------------------------- *
 * For every clip site (the four columns of the tdt_clip_align_* entries) the best placement of its CLEN consensus bases on ANY loaded
 * contig of a tdt_refseq, on either strand, whose first TDT_CLIP_FAR_SEED columns match exactly and whose other columns differ in at
 * most M places (csrc/tdt_clip_far.hip: the reference streams once against a sorted seed table of the sites); the definition is
 * tiddit_amd/tiddit_clip_far.py's.  Per site six uint32: status (0 short_consensus: CLEN < K; 1 off_reference: the site's own contig
 * is outside the table or not loaded, or P outside 1 ... len; 2 searched), the partner's contig, PARTNER (the best candidate's Q,
 * 1-based), strand (0 forward, 1 reverse complement), its mismatches, and HITS (the candidates with at most M mismatches; it
 * saturates at 0xffffffff).  The best candidate is the minimum of (mismatches, another contig than the site's, |Q - P| on the site's
 * own, strand, contig, Q) over those candidates; a searched site without one, and a site that is not searched, has contig 0, PARTNER 0,
 * strand 0, mismatches 0xffffffff and HITS 0.  A CLEN above TDT_CLIP_COLS is taken as TDT_CLIP_COLS, of the side only bit 0.
 * tdt_clip_far_sites takes host arrays of n sites, tdt_clip_far_sites_device caller-owned device arrays; both return when the launches
 * are done.  tdt_clip_far searches the rows of the handle's last tdt_clip_finish where they lie in HBM, keeps the six columns on the
 * device for tdt_clip_far_rows (*n in: room of the arrays, out: rows; all six NULL: the count alone) and fills
 * sn_out[TDT_CLIP_FAR_SN_N]:
 *   [0] sites  [1] short_consensus  [2] off_reference  [3] searched  [4] placed  [5] ambiguous  [6] unplaced  [7] same_contig
 *   [8] other_contig  [9] reverse  [10] mated (always 0 here: mates are the host's, rule 5 of the definition)
 * tdt_clip_far_timing: device milliseconds of the last tdt_clip_far: ms4 = seeds and filter, sort, scan, rows.  The reference is not
 * owned and must lie on the context's device; it and tdt_clip_align share one.  The candidate's 64-bit key holds the contig in 24
 * bits and a site takes two entries of the sort.  Refusals: TDT_E_ARG (null pointers, n >= 2^31, a reference of another device, for
 * the handle a reference with another contig count, tdt_clip_far without a finish since the last push or reset, tdt_clip_far_rows /
 * _timing without a tdt_clip_far since then), TDT_E_RANGE (K outside TDT_CLIP_FAR_SEED ... TDT_CLIP_COLS, M outside
 * 0 ... TDT_CLIP_COLS - TDT_CLIP_FAR_SEED, a reference of more than 2^24 contigs, 2^29 sites or more, too little room in
 * tdt_clip_far_rows); a refused call leaves its outputs untouched. */
#define TDT_CLIP_FAR_SN_N 11
#define TDT_CLIP_FAR_SEED 16
int tdt_clip_far_sites(tdt_ctx *ctx, tdt_refseq *ref, size_t n, const uint64_t *k1, const uint32_t *side, const uint32_t *clen, const uint64_t *consensus,
                       int K, int M, uint32_t *status_out, uint32_t *partner_tid_out, uint32_t *partner_out, uint32_t *strand_out, uint32_t *mm_out,
                       uint32_t *hits_out);
int tdt_clip_far_sites_device(tdt_ctx *ctx, tdt_refseq *ref, size_t n, const uint64_t *d_k1, const uint32_t *d_side, const uint32_t *d_clen,
                              const uint64_t *d_consensus, int K, int M, uint32_t *d_status, uint32_t *d_partner_tid, uint32_t *d_partner,
                              uint32_t *d_strand, uint32_t *d_mm, uint32_t *d_hits);
int tdt_clip_far(tdt_clip *h, tdt_refseq *ref, int K, int M, uint64_t *sn_out);
int tdt_clip_far_rows(tdt_clip *h, uint32_t *status, uint32_t *partner_tid, uint32_t *partner, uint32_t *strand, uint32_t *mm, uint32_t *hits, size_t *n);
int tdt_clip_far_timing(tdt_clip *h, double *ms4);

/* ---- insertion candidates from facing clip sites (TIDDIT_CLIPS_INS) --------------------------------------- *
 * The clipped bases of a clip site beyond TDT_CLIP_COLS columns, up to TDT_CLIP_EXT_COLS, and the insertion that an R site and an L
 * site facing each other close where their extended consensus overlap (csrc/tdt_clip_ins.hip, the extension keys in
 * csrc/tdt_clip.hip); the definition is tiddit_amd/tiddit_clip_ins.py's.  tdt_clip_ext_enable gives a tdt_clip handle a SECOND key
 * store of `capacity` keys, before its first push: every push then also stores, per clip of which more than 28 bases are kept, one key
 * per further chunk c = 1 ... 4 of 28 columns, K1 = c << 56 | tid << 32 | P and K2 in the layout of the first store (at most
 * TDT_CLIP_EXT_MAX_PER_READ keys per read; the store reserves and grows as the first does).  tdt_clip_ext_keys reads that store out in
 * the convention of tdt_clip_keys.  tdt_clip_ins runs on the rows of the handle's last tdt_clip_finish where they lie in HBM, with that
 * finish's minimum support S: the second store is finished as the first was (a chunk's row has SUPPORT >= S), the chunks are gathered
 * onto the rows (ECLEN, and TDT_CLIP_EXT_WORDS words of 56 bits per row: columns 28 w ... 28 w + 27 in word w), and every R row with
 * ECLEN >= K is paired with every L row with ECLEN >= K on its contig at P_R + 1 - d, 0 <= d <= TDT_CLIP_INS_MAX_TSD.  Per pair, for
 * l in O ... a + b - O (a, b the two ECLEN): the overlap o = min(a, l) - max(0, l - b) and its mismatches; an l with o >= O and at most
 * M mismatches is a closure, the best one the minimum of (mismatches, l).  It fills sn_out[TDT_CLIP_INS_SN_N]:
 *   [0] ext_left_events  [1] ext_right_events  [2] ext_keys  [3] cut_beyond_28  [4] sites_extended  [5] left_sites  [6] right_sites
 *   [7] pairs  [8] closed  [9] open  [10] closed_multi
 * tdt_clip_ext_rows reads ECLEN and the words of every row out, in the order of tdt_clip_rows; tdt_clip_ins_rows the pairs, ascending
 * by (contig, P_R, P_L): the two rows' indices, TSD = d, status (1 closed, 0 open), LEN, MISMATCH and CLOSURES (LEN and MISMATCH 0
 * for an open pair) and TDT_CLIP_INS_SEQ_WORDS words of 56 bits of the closed sequence (zero for an open pair); for both *n in: the room
 * of the arrays, out: the rows; every array NULL: the count alone.  tdt_clip_ins_timing: device milliseconds of the last tdt_clip_ins:
 * ms3 = the second store's finish, the gather, the pair launches.  tdt_clip_ins_sites takes host arrays of n sites (k1, side, eclen,
 * cons5) that ascend strictly by (K1, side), tdt_clip_ins_sites_device caller-owned device arrays (outputs and sn_out on the device
 * too; their order is the caller's to keep); *n_pairs in: the room of the eight pair arrays, out: the pairs; all eight NULL: the pair
 * count and the counters [4] ... [7] alone.  An ECLEN above TDT_CLIP_EXT_COLS is taken as TDT_CLIP_EXT_COLS, of the side only bit 0.
 * Refusals: TDT_E_ARG (null pointers, some but not all output arrays, host sites that do not ascend, tdt_clip_ext_enable twice or
 * behind a push, tdt_clip_ext_keys / tdt_clip_ins without tdt_clip_ext_enable, tdt_clip_ins without a finish since the last push or
 * reset, the read-outs and the timing without a tdt_clip_ins since then), TDT_E_RANGE (K outside TDT_CLIP_INS_MIN_COLS ...
 * TDT_CLIP_EXT_COLS, O outside TDT_CLIP_INS_MIN_OVERLAP ... TDT_CLIP_EXT_COLS, M outside 0 ... TDT_CLIP_INS_MAX_MISMATCH, too little
 * room); a refused call leaves its outputs untouched. */
#define TDT_CLIP_EXT_COLS 140
#define TDT_CLIP_EXT_WORDS 5
#define TDT_CLIP_EXT_MAX_PER_READ 8
#define TDT_CLIP_INS_SN_N 11
#define TDT_CLIP_INS_MAX_TSD 32
#define TDT_CLIP_INS_SEQ_WORDS 10
#define TDT_CLIP_INS_MIN_COLS 10
#define TDT_CLIP_INS_MIN_OVERLAP 8
#define TDT_CLIP_INS_MAX_MISMATCH 8
int tdt_clip_ext_enable(tdt_clip *h, size_t capacity);
int tdt_clip_ext_keys(tdt_clip *h, uint64_t *k1, uint64_t *k2, size_t *n);
int tdt_clip_ins(tdt_clip *h, int K, int O, int M, uint64_t *sn_out);
int tdt_clip_ext_rows(tdt_clip *h, uint32_t *eclen, uint64_t *cons5, size_t *n);
int tdt_clip_ins_rows(tdt_clip *h, uint32_t *r_row, uint32_t *l_row, uint32_t *tsd, uint32_t *status, uint32_t *len, uint32_t *mm, uint32_t *closures,
                      uint64_t *seq10, size_t *n);
int tdt_clip_ins_timing(tdt_clip *h, double *ms3);
int tdt_clip_ins_sites(tdt_ctx *ctx, size_t n, const uint64_t *k1, const uint32_t *side, const uint32_t *eclen, const uint64_t *cons5, int K, int O, int M,
                       uint64_t *sn_out, uint32_t *r_row, uint32_t *l_row, uint32_t *tsd, uint32_t *status, uint32_t *len, uint32_t *mm, uint32_t *closures,
                       uint64_t *seq10, size_t *n_pairs);
int tdt_clip_ins_sites_device(tdt_ctx *ctx, size_t n, const uint64_t *d_k1, const uint32_t *d_side, const uint32_t *d_eclen, const uint64_t *d_cons5, int K,
                              int O, int M, uint64_t *d_sn_out, uint32_t *d_r_row, uint32_t *d_l_row, uint32_t *d_tsd, uint32_t *d_status, uint32_t *d_len,
                              uint32_t *d_mm, uint32_t *d_closures, uint64_t *d_seq10, size_t *n_pairs);

/* ---- TIDDIT_CLIPS_MEI: gapped local alignment of short queries to a family library ------------------------------------------ *
 * Smith-Waterman with affine gaps (Gotoh) of n queries against every sequence of a library, on both strands, with an integer
 * tie rule that makes the result unique (csrc/tdt_swalign.hip); the definition is tiddit_amd/tiddit_clip_mei.py's.  The LIBRARY is a
 * tdt_refseq handle of its own whose every sequence is loaded (tdt_refseq_load_fasta): 1 ... TDT_SW_LIB_MAX_SEQS sequences of
 * 1 ... TDT_SW_LIB_MAX_BASES bases, TDT_SW_LIB_MAX_BASES in all; a problem reads exactly its sequence's bases.  A QUERY is 1 ...
 * TDT_SW_QMAX bases A C G T = 0 1 2 3 in TDT_SW_SEQ_WORDS words of 56 bits, column 28 w + j in bits 2j + 1 : 2j of word w, zero behind
 * its last base.  Scores: match +TDT_SW_MATCH, mismatch -TDT_SW_MISMATCH, a gap of k bases -(TDT_SW_GAP_OPEN + k TDT_SW_GAP_EXTEND), a
 * library base that is not A C G T -TDT_SW_OTHER against anything.  Per query the nine result columns: family (0xffffffff and zeros
 * behind it when no cell is positive), strand (1: the query's reverse complement aligned), score, qstart, qend (1-based, in the query
 * as given), fstart, fend (1-based), second (the best score among the other sequences, 0) and second_family (0xffffffff).  The columns
 * are written whatever A is; A (TDT_SW_MIN_SCORE_LO ... TDT_SW_QMAX) decides the counters sn_out[TDT_SW_SN_N]: queries, closed_queries,
 * left_queries, right_queries, named (score >= A), unnamed, reverse, ambiguous (named, second == score), pairs_named, pairs_conflict.
 * tdt_sw_align takes host arrays, tdt_sw_align_device caller-owned device arrays (outputs and sn_out on the device too; a length
 * above TDT_SW_QMAX is taken as TDT_SW_QMAX there); both take every query as a closed pair of its own.  All nine columns NULL: the
 * counters alone.  tdt_sw_align_timing: device milliseconds of the calling thread's last run of either: ms2 = the alignment launch, the
 * reduction.  tdt_clip_mei runs on the pair rows of the handle's last tdt_clip_ins where they lie in HBM: a CLOSED pair gives one
 * query (its SEQ), an OPEN pair two (its R site's consensus, then its L site's, both in reference direction); an OPEN pair is named
 * when a part is and the named parts agree in family and strand, else it is a conflict.  tdt_clip_mei_rows reads out, per query, the
 * pair row, the part (0 SEQ, 1 LEFT, 2 RIGHT), the length and the nine columns; *n in: the room of the arrays, out: the queries; every
 * array NULL: the count alone.  tdt_clip_mei_timing: device milliseconds of the last tdt_clip_mei: ms3 = the query build, the alignment
 * launch, the reduction.  Refusals: TDT_E_ARG (null pointers, some but not all output arrays, a library on another device or with a
 * sequence that is not loaded, tdt_clip_mei without a tdt_clip_ins since the last push, reset or finish, the read-outs without a
 * tdt_clip_mei since then), TDT_E_RANGE (A, a host query's length, a host query word with a bit set at or behind its last base, the
 * library limits, 2^31 problems or more, too little room); a refused call leaves its outputs untouched. */
#define TDT_SW_QMAX 280
#define TDT_SW_SEQ_WORDS 10
#define TDT_SW_SN_N 10
#define TDT_SW_MIN_SCORE_LO 12
#define TDT_SW_LIB_MAX_SEQS 4096
#define TDT_SW_LIB_MAX_BASES (1 << 20)
#define TDT_SW_MATCH 1
#define TDT_SW_MISMATCH 4
#define TDT_SW_GAP_OPEN 6
#define TDT_SW_GAP_EXTEND 1
#define TDT_SW_OTHER 1
int tdt_sw_align(tdt_ctx *ctx, tdt_refseq *lib, size_t n, const uint64_t *seq10, const uint32_t *qlen, int A, uint64_t *sn_out, uint32_t *family,
                 uint32_t *strand, uint32_t *score, uint32_t *qstart, uint32_t *qend, uint32_t *fstart, uint32_t *fend, uint32_t *second,
                 uint32_t *second_family);
int tdt_sw_align_device(tdt_ctx *ctx, tdt_refseq *lib, size_t n, const uint64_t *d_seq10, const uint32_t *d_qlen, int A, uint64_t *d_sn_out,
                        uint32_t *d_family, uint32_t *d_strand, uint32_t *d_score, uint32_t *d_qstart, uint32_t *d_qend, uint32_t *d_fstart,
                        uint32_t *d_fend, uint32_t *d_second, uint32_t *d_second_family);
int tdt_sw_align_timing(double *ms2);
int tdt_clip_mei(tdt_clip *h, tdt_refseq *lib, int A, uint64_t *sn_out);
int tdt_clip_mei_rows(tdt_clip *h, uint32_t *pair, uint32_t *part, uint32_t *qlen, uint32_t *family, uint32_t *strand, uint32_t *score, uint32_t *qstart,
                      uint32_t *qend, uint32_t *fstart, uint32_t *fend, uint32_t *second, uint32_t *second_family, size_t *n);
int tdt_clip_mei_timing(tdt_clip *h, double *ms3);

/* ---- exact per-base depth and the small-variant genotypes (TIDDIT_SMALL_VCF) ---------------------------- *
 * The number of eligible reads with an aligned base (M = X) at every reference position, CIGAR-exact (csrc/tdt_pileup.hip); the
 * definition is tiddit_amd/tiddit_pileup.py's, the genotype rule tiddit_amd/tiddit_small_vcf.py's.  A handle keeps ONE int32 per
 * reference base plus a guard slot per contig in HBM (4 bytes per base; zeroed at create and reset) and TDT_PILE_SN_N uint64 counters:
 *   [0] records  [1] eligible  [2] malformed  [3] no_cigar  [4] spans  [5] covered_bases  [6] clamped_spans
 * Eligible: flag & 0xF04 == 0, tid >= 0, mapq >= min_mapq.  An eligible record is bounded and judged malformed exactly as tdt_snv does
 * it, and also when tid >= n_contigs; a malformed record adds one to `malformed` and nothing else, one without CIGAR to `no_cigar`.
 * Touching M = X stretches are one span; every span is clamped to the contig (`clamped_spans`: cut or dropped) and adds +1 at its
 * start and -1 at its end.  Nothing outside raw[0, raw_len) is ever read.  The push entries take what tdt_snv's take: the device entry
 * enqueues one launch on the context's stream and waits for nothing, the host entry uploads, runs the same kernel and returns when it
 * is done.  tdt_pile_finish turns the differences into depths (an in-place prefix sum over all slots, three launches) and returns
 * when it is done; a second finish changes nothing.  Behind it tdt_pile_depth reads out[n] depths of contig tid from base start on, and
 * tdt_pile_genotype / tdt_pile_genotype_device take n rows (K1 = tid << 32 | P with P 1-based, SUPPORT) from host / device memory and
 * write eight uint32 per row to out8 (device: on a 16-byte boundary; enqueued, nothing is waited for):
 *   [0] DP0 = depth[tid][P - 1], 0 outside the contig  [1] OTHER  [2] PL 0/0  [3] PL 0/1  [4] PL 1/1  [5] GT index  [6] GQ
 *   [7] 1 when SUPPORT > DP0.
 * tdt_pile_counters synchronises the stream.  tdt_pile_timing: device milliseconds of the last finish's three launches (tile sums,
 * carry, scan and write) and of the last tdt_pile_genotype launch.
 * Refusals: TDT_E_ARG (null pointers, record offsets that decrease, n >= 2^31, a push behind the finish without a reset,
 * tdt_pile_depth or a genotype entry before the finish), TDT_E_RANGE (2^24 contigs or more, a length of 2^31 or more, min_mapq outside
 * 0 ... 255, a range of tdt_pile_depth outside the contig), TDT_E_NOMEM; a refused call leaves its outputs untouched.
 * tdt_pile_sn_size() = TDT_PILE_SN_N. */
#define TDT_PILE_SN_N 7
typedef struct tdt_pile tdt_pile;
int tdt_pile_create(tdt_ctx *ctx, int n_contigs, const int64_t *lengths, int min_mapq, tdt_pile **out);
int tdt_pile_destroy(tdt_pile *h);
int tdt_pile_reset(tdt_pile *h);
int tdt_pile_push_device(tdt_pile *h, const void *const *d_arrays14, size_t n, size_t raw_len);
int tdt_pile_push(tdt_pile *h, const uint16_t *flag, const int32_t *tid, const int32_t *pos, const uint8_t *mapq, const uint64_t *rec_off,
                  size_t n, const uint8_t *raw, size_t raw_len);
int tdt_pile_finish(tdt_pile *h);
int tdt_pile_depth(tdt_pile *h, int tid, int64_t start, int64_t n, uint32_t *out);
int tdt_pile_genotype(tdt_pile *h, const uint64_t *k1, const uint32_t *support, size_t n, uint32_t *out8);
int tdt_pile_genotype_device(tdt_pile *h, const uint64_t *d_k1, const uint32_t *d_support, size_t n, uint32_t *d_out8);
int tdt_pile_counters(tdt_pile *h, uint64_t *sn_out);
int tdt_pile_timing(tdt_pile *h, double *ms4);
size_t tdt_pile_sn_size(void);

/* ---- alignment-record decode (host) ---------------------------------------------------------- *
 * Replaces the per-read pysam attribute access that feeds the path (read.reference_start,
 * reference_end, mapq, flag, next_reference_id, next_reference_start, isize, cigartuples[0]/[-1],
 * has_tag("SA") — __main__.py:229-240, tiddit_signal.pyx:169-221).  `buf` is uncompressed BAM record
 * data (after the header), starting at a record boundary.  Decodes up to max_records whole records into
 * the caller's arrays (any output pointer may be NULL); *consumed = bytes of whole records decoded.
 * end = htslib bam_endpos(); cigar_first/cigar_last = raw (len<<4|op) words or 0xffffffff without CIGAR;
 * rec_off = byte offset of each record (at its block_size field); sa_off = offset of the SA:Z string or -1. */
int tdt_bam_decode(const uint8_t *buf, size_t len, size_t max_records, size_t *consumed, size_t *n_records,
                   int32_t *tid, int32_t *pos, int32_t *end, uint8_t *mapq, uint16_t *flag, int32_t *mate_tid,
                   int32_t *mate_pos, int32_t *tlen, int32_t *l_seq, uint32_t *cigar_first, uint32_t *cigar_last,
                   uint64_t *rec_off, int64_t *sa_off);

/* ---- library statistics (host) ------------------------------------------------------------------------ *
 * The sampling loop of tiddit_stats.statistics (tiddit_stats.py:17-47) over decoded field arrays: state[0] n_sampled, [1] sum of read
 * lengths, [2] read lengths counted, [3] innie, [4] outtie, [5] done (n_sampled > n_reads) carry over from batch to batch (zero them
 * first); the template lengths of the pairs that pass every test are appended to out_tlen (room for n), *n_out = how many. */
int tdt_stats_scan(const int32_t *tid, const int32_t *pos, const int32_t *mate_tid, const int32_t *mate_pos, const int32_t *tlen,
                   const int32_t *l_seq, const uint16_t *flag, const uint8_t *mapq, size_t n, int64_t n_reads, int min_mapq,
                   int64_t max_ins_len, int64_t *state, int32_t *out_tlen, size_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* TIDDIT_HIP_H */
