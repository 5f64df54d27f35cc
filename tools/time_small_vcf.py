"""What the genotyped small-variant VCF of `tiddit --sv` (TIDDIT_SMALL_VCF) costs the job: `tiddit --sv --skip_assembly` with
TIDDIT_SNVS + TIDDIT_INDELS + TIDDIT_INDELS_NORM, without and with the switch, interleaved, in one process — the whole job's wall and the
scan stage both ways (with the spread of the runs without the switch), the new stage timer of the pushes, the three launches of the
prefix sum (HIP events round them inside tdt_pile_finish), the two genotype launches, the host text and the array's bytes.  The yardstick
is the same job without the switch in the same process, never an absolute number.  `pile_spans` is also timed per batch between device
events on the context's stream, beside `indel_keys` (left-normalising) and `snv_keys` on the same batches (best of 4, the stream idle
around each), and the prefix sum's launches are set against a plain streaming read measured in the same process (tdt_calib_stream_read,
the kernel of tools/calib_stream.py, over a buffer of the array's size).  Writes the record to profiles/small_vcf_<mb>mb.md (or --out)
and prints one JSON line.

The synthetic file's reads are cut from the reference the job loads (bench.py's file), so few SNV rows are made: what the record measures
is the depth of every read, not a gather over millions of rows.

usage: python tools/time_small_vcf.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--out FILE.md]
(--mb: bench.py's synthetic file of that genome size, made at $TIDDIT_BENCH_TMP/tiddit_bench_sv_<mb>/ when it is not there)"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from time_cov_track import bench_file  # noqa: E402  (the same synthetic file)

MODES = ("off", "on")
BASE = {"TIDDIT_SNVS": "1", "TIDDIT_INDELS": "1", "TIDDIT_INDELS_NORM": "1"}
KEYS = (("scan", "signal extraction + coverage"), ("push", "pileup spans (push)"), ("snv push", "snv keys (push)"), ("indel push", "indel keys (push)"),
        ("ingest wait", "ingest (inflate + decode, device)"), ("stage", "small variants ({o}.small.vcf)"),
        ("depth", "small vcf depth (device: prefix sum over the difference array)"), ("tile sums", "pile tile sums (device time)"),
        ("carry", "pile carry (device time)"), ("scan write", "pile scan + write (device time)"),
        ("genotypes", "small vcf genotypes (device: one gather launch per table, rows up and down)"),
        ("gt snv", "pile_genotype, snv rows (device time)"), ("gt indel", "pile_genotype, indel rows (device time)"), ("text", "small vcf text (host)"))
LABELS = {"wall": "whole job", "scan": "scan stage", "push": "new stage timer (pile_spans pushes, host side)", "snv push": "snv pushes, host side",
          "indel push": "indel pushes, host side", "ingest wait": "scan: waited for the ingest", "stage": "small-vcf stage (prefix sum, genotypes, file)",
          "depth": "stage: tdt_pile_finish (host clock, returns when done)", "tile sums": "stage: pile_tile_sums (device)", "carry": "stage: ks_carry_sum (device)",
          "scan write": "stage: pile_tile_scan (device)", "genotypes": "stage: the two genotype calls (host clock, rows up and down)",
          "gt snv": "stage: pile_genotype, snv rows (device)", "gt indel": "stage: pile_genotype, indel rows (device)", "text": "stage: records' text and file (host)"}


def kernels_alone(bam, fasta, min_mapq, min_bq):
    """every batch of the file through the three pushes, each between two device events on the context's stream with the stream idle
    around it -> per batch (reads, raw bytes, ms of pile_spans, indel_keys, snv_keys), best of 4"""
    import torch
    from tiddit_amd import bamio, refseq, tiddit_indels, tiddit_pileup, tiddit_snvs
    from tiddit_amd.fasta import FastaFile
    rd = bamio.DeviceBamReader(bam)
    ctx = rd.ctx
    stream = torch.cuda.ExternalStream(int(ctx.lib.tdt_ctx_stream(ctx.handle)))
    ref = refseq.load_for_bam(FastaFile(fasta), list(rd.references), list(rd.lengths), ctx=ctx)[0]
    pile = tiddit_pileup.PileupDepth(rd.lengths, min_mapq, ctx=ctx)
    snv = indel = None
    rows = []

    def timed(h):
        best = None
        for _ in range(4):                               # (the first one warms up)
            h.reset()
            ctx.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h.push_device_batch(b)
            e1.record(stream)
            ctx.sync()
            ms = e0.elapsed_time(e1)
            best = ms if best is None or ms < best else best
        return best
    try:
        for b in rd.batches():
            if snv is None:                              # (room for the largest batch's bound: no reserve asks or grows inside the timing)
                snv = tiddit_snvs.SnvCounter(len(rd.references), ref, min_mapq, min_bq, capacity=8 * len(b) + 4096, ctx=ctx)
                indel = tiddit_indels.IndelCounter(len(rd.references), min_mapq, capacity=4 * len(b) + 4096, ctx=ctx)
                indel.set_reference(ref)
            rows.append({"reads": len(b), "raw_bytes": int(b._raw_len), "pile_ms": timed(pile), "indel_ms": timed(indel), "snv_ms": timed(snv)})
    finally:
        for h in (pile, snv, indel):
            if h is not None:
                h.close()
        ref.close()
        rd.close()
    return rows


def stream_read(ctx, nbytes):
    """a plain streaming read of ``nbytes`` in this process -> (best ms, mean ms) of 10"""
    import torch
    buf = torch.empty(max(nbytes // 8, 1 << 20), dtype=torch.int64, device="cuda")
    buf.random_(0, 1 << 40)
    torch.cuda.synchronize()
    best, mean = ctypes.c_double(0), ctypes.c_double(0)
    from tiddit_amd import _native
    _native.check(ctx.lib.tdt_calib_stream_read(ctx.handle, buf.data_ptr(), buf.numel() * 8, 10, 8, 0, ctypes.byref(best), ctypes.byref(mean)))
    return best.value, mean.value, buf.numel() * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    print("file: %s" % a.bam, file=sys.stderr, flush=True)
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native
    ctx = _native.default_context()
    runs = {m: [] for m in MODES}
    header, n_records, array_bytes = {}, 0, 0
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                os.environ.update(BASE)
                os.environ.pop("TIDDIT_SMALL_VCF", None)
                if mode == "on":
                    os.environ["TIDDIT_SMALL_VCF"] = "1"
                buf = io.StringIO()
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(buf):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    for k in tuple(BASE) + ("TIDDIT_SMALL_VCF",):
                        os.environ.pop(k, None)
                Sx = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
                rec = {"wall": time.perf_counter() - t0}
                rec.update({short: Sx[key] for short, key in KEYS if key in Sx})
                assert os.path.exists(out + ".small.vcf") == (mode == "on")
                if i:
                    runs[mode].append(rec)
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "on" and i == a.reps:
                    lines = open(out + ".small.vcf").read().split("\n")
                    header = {l[len("##small_vcf_"):].split("=")[0]: int(l.split("=")[1]) for l in lines if l.startswith("##small_vcf_")}
                    n_records = sum(1 for l in lines if l and not l.startswith("#"))
                    array_bytes = cli.STAGE_NOTES.get("small vcf: depth array (bytes)", 0)
    alone = kernels_alone(a.bam, a.ref, 20, 20)
    sr_best, sr_mean, sr_bytes = stream_read(ctx, array_bytes)
    stream_gbs = sr_bytes / sr_mean / 1e6

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = ["wall"] + [short for short, _ in KEYS]
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "header": header, "records": n_records, "array_bytes": array_bytes,
           "median_s": {m: {k: med(m, k) for k in keys} for m in MODES}, "runs": runs, "kernels_alone": alone,
           "stream_read": {"bytes": sr_bytes, "best_ms": sr_best, "mean_ms": sr_mean, "GBs": stream_gbs}}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "small_vcf" + ("_%dmb.md" % a.mb if a.mb else ".md"))
    with open(path, "w") as f:
        f.write("# The genotyped small-variant VCF of `tiddit --sv` (`TIDDIT_SMALL_VCF=1`)\n\n")
        f.write("File: `%s` (%.0f MB), its reads cut from the reference the job loads.  `tools/time_small_vcf.py`: one process, after one warm-up round %d "
                "rounds of { `--sv --skip_assembly` with `TIDDIT_SNVS=1 TIDDIT_INDELS=1 TIDDIT_INDELS_NORM=1`, the same with `TIDDIT_SMALL_VCF=1` }, "
                "interleaved.  Wall seconds unless a row says device; the yardstick is the off job of the same process; no threshold was fixed in advance, "
                "this is what was measured.\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in MODES:
            for key in keys:
                if med(mode, key) is None:
                    continue
                f.write("| %s: %s | %s | %.5f |\n" % (mode, LABELS[key], " | ".join("%.5f" % r[key] for r in runs[mode]), med(mode, key)))
        off = [r["scan"] for r in runs["off"]]
        offw = [r["wall"] for r in runs["off"]]
        d_scan, spread = med("on", "scan") - med("off", "scan"), max(off) - min(off)
        f.write("\nScan stage, off runs: spread %.4f s (min %.4f, max %.4f).  Scan stage, on against the off median: %+.4f s — %s the spread of the off runs.  "
                "Whole job, off runs: spread %.4f s.  Whole job, on against the off median: %+.4f s.\n" % (
                    spread, min(off), max(off), d_scan, "INSIDE" if abs(d_scan) <= spread else "OUTSIDE", max(offw) - min(offw), med("on", "wall") - med("off", "wall")))
        f.write("\nThe array: %d bytes in HBM (4 per reference base and contig guard).  The file: %s; %d records in the VCF.\n" % (
            array_bytes, ", ".join("%s %d" % kv for kv in header.items()), n_records))
        if med("on", "tile sums") is not None:
            ts, cy, sw = (med("on", k) * 1e3 for k in ("tile sums", "carry", "scan write"))
            f.write("\nThe prefix sum on the device: pile_tile_sums %.4f ms (reads the array once: %.0f GB/s), ks_carry_sum %.4f ms, pile_tile_scan %.4f ms "
                    "(reads and writes it once: %.0f GB/s of traffic).  A plain streaming read of %d bytes in this process (tdt_calib_stream_read, 8 workgroups "
                    "per CU, mean of 10): %.4f ms = %.0f GB/s; pile_tile_sums runs at %.2f of it, the three launches together move 3 x the array in %.4f ms = "
                    "%.2f of it.  (Both buffers had just been written when they were read: what the last-level cache still held of them is in both numbers.)\n" % (ts, array_bytes / ts / 1e6, cy, sw, 2 * array_bytes / sw / 1e6, sr_bytes, sr_mean, stream_gbs,
                                       (array_bytes / ts / 1e6) / stream_gbs, ts + cy + sw, (3 * array_bytes / (ts + cy + sw) / 1e6) / stream_gbs))
        f.write("\n`pile_spans` beside `indel_keys` (left-normalising) and `snv_keys` on the same batches: each launch between two device events on the "
                "context's stream, the stream idle around it, best of 4:\n\n| batch | reads | raw MB | pile_spans ms | indel_keys ms | snv_keys ms | pile_spans reads per us |\n"
                "|---|---|---|---|---|---|---|\n")
        for k, r in enumerate(alone):
            f.write("| %d | %d | %.1f | %.3f | %.3f | %.3f | %.0f |\n" % (k, r["reads"], r["raw_bytes"] / 1e6, r["pile_ms"], r["indel_ms"], r["snv_ms"],
                                                                       r["reads"] / (r["pile_ms"] * 1e3)))
        f.write("\nNot measured by this record: real libraries (their indel density, a gather over millions of rows, a 3.1-Gb array), long reads, N ranks "
                "(refused).  A per-workgroup LDS window for `pile_spans` was not built.\n")


if __name__ == "__main__":
    main()
