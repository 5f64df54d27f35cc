"""What the clipped-read breakpoint sites of `tiddit --sv` (TIDDIT_CLIPS) cost the job: `tiddit --sv --skip_assembly` with the switch off
and on, interleaved, in one process — the whole job's wall and the scan stage off and on (with the spread of the off runs beside every
figure), the new stage timer (the pushes' host side: it also holds the waits of a reserve that has to ask the device), the finish stage
split into its two sorts, the gather, the run-length launches and the site launches (heads, vote, rows; HIP events round them inside
tdt_clip_finish), the keys stored and how often the reserve asked the device or grew the store.  The yardstick is the same job without
the switch in the same process, never an absolute number.  `clip_keys` is also timed alone (host clock around launch and sync, the
stream idle, best of 4) on every batch of the file.  Writes the record to profiles/clips_<mb>mb.md (or --out) and prints one JSON line.

With --align the record is about TIDDIT_CLIPS_ALIGN instead: the job with the switches off, with TIDDIT_CLIPS alone and with the aligned
job, interleaved in one process, and the aligned job at W = 2^20; written to profiles/clips_align_<mb>mb.md.

With --far the record is about TIDDIT_CLIPS_FAR: the job with the switches off, with TIDDIT_CLIPS alone and with the far job, interleaved
in one process; `far_scan`'s device time against `clip_align_sites` at W = 2^20 on the same sites scaled to the genome's length (the
brute-force alternative) and against a plain streaming read of the packed store's bytes; written to profiles/clips_far_<mb>mb.md.

With --ins the record is about TIDDIT_CLIPS_INS: the job with the switches off, with TIDDIT_CLIPS alone and with the extension store and
the pair stage, interleaved in one process; the push of every batch with and without `clip_ext_keys` beside `clip_keys` (the stream idle,
best of 4); the device events of the extension finish, the gather and the pair launches; written to profiles/clips_ins_<mb>mb.md.

With --vcf the record is about TIDDIT_CLIPS_VCF: the job with the switches off, with the four clip switches and with the junction VCF
beside them, interleaved in one process — the yardstick is the four-switch job and its own run-to-run spread; the stage's host parts and
`junction_support`'s device time; then the kernel alone on one boundary per 10 kb over a store built from the file; written to
profiles/clips_vcf_<mb>mb.md.

With --mei the record is about TIDDIT_CLIPS_MEI: the job with the switches off, with the four clip switches and with a generated 16-kb
family library beside them, interleaved in one process — the yardstick is the four-switch job and its own run-to-run spread; then the
alignment kernel alone, by device events, on generated tables of 1024 queries of 272 and of 60 bases against that library: cell updates
per second and the share of lanes that held a column; written to profiles/clips_mei_<mb>mb.md.

usage: python tools/time_clips.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--switch 1] [--align [--align-switch 1]] [--far [--far-switch 1]]
                                  [--ins [--ins-switch 1]] [--vcf [--vcf-switch 1]] [--mei] [--out FILE.md]
(--mb: bench.py's synthetic file of that genome size, made at $TIDDIT_BENCH_TMP/tiddit_bench_sv_<mb>/ when it is not there)"""
import argparse
import contextlib
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
KEYS = (("scan", "signal extraction + coverage"), ("push", "clip keys (push)"), ("ingest wait", "ingest (inflate + decode, device)"),
        ("finish", "clip sites ({o}.clips.tab)"), ("device", "clip sites (device: two sorts, gather, run lengths, site heads, vote, rows)"),
        ("sort K2", "clip sort by K2 (device time)"), ("gather", "clip gather of K1 (device time)"), ("sort K1", "clip sort by K1 (device time)"),
        ("runs", "clip run lengths + rows (device time)"), ("sites", "clip site heads + vote + site rows (device time)"), ("text", "clip table text (host)"))
LABELS = {"wall": "whole job", "scan": "scan stage", "push": "new stage timer (pushes, host side, reserve waits included)",
          "ingest wait": "scan: waited for the ingest", "finish": "finish stage (sort, run lengths, vote, rows, file)",
          "device": "finish: the calls into the library", "sort K2": "finish: sort by K2 (device)", "gather": "finish: gather of K1 (device)",
          "sort K1": "finish: sort by K1 (device)", "runs": "finish: gather of K2 + run-length and row launches (device)",
          "sites": "finish: site heads, vote and site rows, seven launches (device)", "text": "finish: file text"}
NOTES = ("clip store: reserves that asked the device", "clip store: growths", "clip store: capacity (keys)", "clip store: keys")


def keys_alone(bam, min_mapq, min_clip, ext=False):
    """every batch of the file through tdt_clip_push_device with the stream idle around it -> per batch (reads, raw bytes, ms of the launch);
    ``ext``: on a handle with the extension store, so the push is `clip_keys` and `clip_ext_keys`"""
    from tiddit_amd import bamio, tiddit_clips
    rd = bamio.DeviceBamReader(bam)
    h = None
    rows = []
    try:
        for b in rd.batches():
            if h is None:                                # (room for the largest batch's bound: no reserve asks or grows inside the timing)
                h = tiddit_clips.ClipCounter(len(rd.references), min_mapq, min_clip, capacity=2 * len(b) + 4096, ctx=rd.ctx)
                if ext:
                    h.enable_ext(8 * len(b) + 4096)
            rd.ctx.sync()
            best = None
            for _ in range(4):                           # (the first one warms up)
                h.reset()
                rd.ctx.sync()
                t0 = time.perf_counter()
                h.push_device_batch(b)
                rd.ctx.sync()
                dt = time.perf_counter() - t0
                best = dt if best is None or dt < best else best
            rows.append({"reads": len(b), "raw_bytes": int(b._raw_len), "ms": best * 1e3})
    finally:
        if h is not None:
            h.close()
        rd.close()
    return rows


ALIGN_MODES = ("off", "clips", "align")
ALIGN_KEYS = (("scan", "signal extraction + coverage"), ("reference", "reference into HBM (TIDDIT_CLIPS_ALIGN)"), ("clip stage", "clip sites ({o}.clips.tab)"),
              ("align", "clip align (device: one workgroup per site over the packed reference)"), ("kernel", "clip align kernel (device time)"),
              ("align text", "clip align mates + table text (host)"))
ALIGN_LABELS = {"wall": "whole job", "scan": "scan stage", "reference": "reference into HBM (read, upload, pack)", "clip stage": "clip stage (finish, align, files)",
                "align": "align: the calls into the library (launch, wait, five columns read out)", "kernel": "align: `clip_align_sites` (device)",
                "align text": "align: mates and file text (host)"}


def _one_job(cli, ctx, bam, ref, out, clips=None, align=None, far=None, keys=None, ins=None, vcf=None, mei=None):
    """one `--sv --skip_assembly` job in this process -> its wall seconds and stage seconds by short name"""
    for k, v in (("TIDDIT_CLIPS", clips), ("TIDDIT_CLIPS_ALIGN", align), ("TIDDIT_CLIPS_FAR", far), ("TIDDIT_CLIPS_INS", ins), ("TIDDIT_CLIPS_VCF", vcf),
                 ("TIDDIT_CLIPS_MEI", mei)):
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    t0 = time.perf_counter()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            cli.main(["--sv", "--bam", bam, "--ref", ref, "-o", out, "--skip_assembly", "--force_overwrite"])
        ctx.sync()
    finally:
        os.environ.pop("TIDDIT_CLIPS", None)
        os.environ.pop("TIDDIT_CLIPS_ALIGN", None)
        os.environ.pop("TIDDIT_CLIPS_FAR", None)
        os.environ.pop("TIDDIT_CLIPS_INS", None)
        os.environ.pop("TIDDIT_CLIPS_VCF", None)
        os.environ.pop("TIDDIT_CLIPS_MEI", None)
    Sx = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
    rec = {"wall": time.perf_counter() - t0}
    rec.update({short: Sx[key] for short, key in (keys or ALIGN_KEYS) if key in Sx})
    return rec


VCF_MODES = ("off", "four", "vcf")
VCF_KEYS = (("scan", "signal extraction + coverage"), ("clip stage", "clip sites ({o}.clips.tab)"), ("vcf", "clip junction vcf ({o}.clips.vcf)"),
            ("junctions", "clip vcf junctions (host)"), ("support", "clip vcf support (device: one wavefront per boundary over the evidence store)"),
            ("kernel", "clip vcf junction_support kernel (device time)"), ("vcf text", "clip vcf text (host)"))
VCF_LABELS = {"wall": "whole job", "scan": "scan stage", "clip stage": "clip stage (finish, align, far, ins, files)", "vcf": "vcf stage (junctions, support, file)",
              "junctions": "vcf: rows to junctions (host)", "support": "vcf: the call into the library (table, upload, launch, wait)",
              "kernel": "vcf: `junction_support` (device)", "vcf text": "vcf: records and file text (host)"}


def main_vcf(a):
    """--vcf: the job with the switches off, with the four clip switches and with TIDDIT_CLIPS_VCF beside them, interleaved in one process,
    medians of --reps; then `junction_support` alone on a synthetic boundary list, one boundary per 10 kb, over a store built from the file"""
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, tiddit_clip_vcf, tiddit_region
    ctx = _native.default_context()
    F = tiddit_clip_vcf.parse_switch(a.vcf_switch)
    runs = {m: [] for m in VCF_MODES}
    header = {}
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up)
            for mode in VCF_MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                on = mode != "off"
                rec = _one_job(cli, ctx, a.bam, a.ref, out, a.switch if on else None, a.align_switch if on else None, a.far_switch if on else None, VCF_KEYS,
                               a.ins_switch if on else None, a.vcf_switch if mode == "vcf" else None)
                assert os.path.exists(out + ".clips.vcf") == (mode == "vcf") and os.path.exists(out + ".clips.ins.tab") == on
                if i:
                    runs[mode].append(rec)
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "vcf" and i == a.reps:
                    header = {l[len("##clips_vcf_"):].split("=")[0]: int(l.split("=")[1]) for l in open(out + ".clips.vcf").read().split("\n") if l.startswith("##clips_vcf_")}
    # the kernel alone, on real work: one boundary per 10 kb of every contig over the file's store
    store = tiddit_region.build_store(a.bam, 5, 100000)
    try:
        bounds = [(t, b) for t, ln in enumerate(store.lengths) for b in range(5000, ln, 10000)]
        table = store.contig_table()
        alone = []
        for _ in range(5):                                # (the first one warms up)
            t0 = time.perf_counter()
            counts = store.junction_support(bounds, F, table=table)
            alone.append({"call_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": store.junction_ms()})
        alone = alone[1:]
        n_records, max_span = int(store.n), int(table[:, 2].max()) if len(table) else 0
        crossed = int(counts[:, 2].sum())
    finally:
        store.close()
    keys = ["wall"] + [short for short, _ in VCF_KEYS]
    med = lambda mode, key: statistics.median([r[key] for r in runs[mode] if r.get(key) is not None] or [float("nan")])
    sp = lambda mode, key: (lambda v: (max(v) - min(v), min(v), max(v)))([r[key] for r in runs[mode]])
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "switches": [a.switch, a.align_switch, a.far_switch, a.ins_switch, a.vcf_switch],
           "flank": F, "header": header, "median_s": {m: {k: med(m, k) for k in keys if any(k in r for r in runs[m])} for m in runs},
           "four_wall_spread_s": sp("four", "wall")[0], "four_scan_spread_s": sp("four", "scan")[0], "runs": runs,
           "alone": {"boundaries": len(bounds), "records": n_records, "max_span": max_span, "span_sum": crossed, "calls": alone}}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "clips_vcf" + ("_%dmb.md" % a.mb if a.mb else ".md"))
    with open(path, "w") as f:
        f.write("# Genotyped VCF of the clip-site junctions (`TIDDIT_CLIPS=%s TIDDIT_CLIPS_ALIGN=%s TIDDIT_CLIPS_FAR=%s TIDDIT_CLIPS_INS=%s TIDDIT_CLIPS_VCF=%s`)\n\n"
                % (a.switch, a.align_switch, a.far_switch, a.ins_switch, a.vcf_switch))
        f.write("File: `%s` (%.0f MB).  `tools/time_clips.py --vcf`: one process, after one warm-up round %d rounds of { switches off, the four clip switches, the "
                "four and `TIDDIT_CLIPS_VCF` }, interleaved.  Wall seconds unless a row says device.  The yardstick is the four-switch job of the same process — "
                "the job as it was before this switch existed — and the spread of its runs; no number was fixed in advance, this is what was measured.\n\n" % (
                    os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in runs:
            for key in keys:
                if not any(key in r for r in runs[mode]):
                    continue
                f.write("| %s: %s | %s | %.5f |\n" % (mode, VCF_LABELS[key], " | ".join("%.5f" % r.get(key, float("nan")) for r in runs[mode]), med(mode, key)))
        f.write("\nScan stage, vcf against the four-switch median: %+.4f s; the four-switch runs' spread is %.4f s (min %.4f, max %.4f).  Whole job: %+.4f s; spread "
                "%.4f s (min %.4f, max %.4f).  The off runs' whole-job spread is %.4f s.\n" % (
                    (med("vcf", "scan") - med("four", "scan"),) + sp("four", "scan") + (med("vcf", "wall") - med("four", "wall"),) + sp("four", "wall") +
                    (sp("off", "wall")[0],)))
        f.write("\nThe claim was that the scan stage stays inside the spread of the runs without the switch: the stage runs behind the scan and adds no launch per "
                "batch, but the scan now also packs its evidence store (one `evidence_pack` launch per batch, as for `TIDDIT_DEPTH_DIST`).  The scan stage's "
                "difference above against the spread beside it is the answer this file gives: inside the spread supports the claim for this file, outside it "
                "retracts it.  Here: %s.\n" % (
                    "inside the spread, the claim stands for this file" if abs(med("vcf", "scan") - med("four", "scan")) <= sp("four", "scan")[0] else
                    "OUTSIDE the spread, the claim is retracted for this file: the scan stage pays for packing the evidence store, what `TIDDIT_DEPTH_DIST` and "
                    "`TIDDIT_VARIANTS` pay when they are on; the stage behind the scan is the `vcf` rows above"))
        f.write("\nThe file's header: %s.  The synthetic file's reads are cut from the reference in one piece (`synth_bam.write_wgs_sv_bam` with `ref_seqs`), a clip "
                "included, so it yields no junction (what places, places as `REF`), no boundary, and the stage costs its set-up only: `junction_support` is "
                "launched only when there is a boundary, so the `kernel` row is absent when the header says 0 records.\n" % (
                    ", ".join("%s %d" % kv for kv in header.items())))
        kms, cms = [c["kernel_ms"] for c in alone], [c["call_ms"] for c in alone]
        f.write("\n`junction_support` alone, on real work: a store built from the same file (%d records, max span %d), one boundary per 10 kb of every contig (%d "
                "boundaries, flank %d; %d reads cross them in all), 4 calls after a warm-up: the kernel between its two events %s ms (median %.4f), the whole "
                "call — contig table, upload of table and boundaries, launch, copy back, wait — %s ms (median %.4f) on the host clock.  One wavefront per "
                "boundary reads its bracket of 16-byte records once: with brackets of a few hundred records this is a latency figure (the 64-ary search's "
                "dependent loads, then one or a few strided loads per lane), not a bandwidth one.\n" % (
                    n_records, max_span, len(bounds), F, crossed, ", ".join("%.4f" % v for v in kms), statistics.median(kms), ", ".join("%.3f" % v for v in cms),
                    statistics.median(cms)))
        f.write("\nNot measured by this record: real libraries (junctions by the thousand, deep coverage: brackets of tens of thousands of records per boundary, "
                "long reads with a large max span), the kernel under a profiler, 3 Gb.\n")


MEI_MODES = ("off", "four", "mei")
MEI_KEYS = (("scan", "signal extraction + coverage"), ("clip stage", "clip sites ({o}.clips.tab)"), ("library", "clip mei library (read, upload, pack)"),
            ("mei", "clip mei (device: query build, alignment, reduction)"), ("build", "clip mei query build (device time)"),
            ("kernel", "clip mei gapped alignment (one wavefront per query, strand and family) (device time)"), ("reduce", "clip mei reduction (device time)"),
            ("mei text", "clip mei table text (host)"))
MEI_LABELS = {"wall": "whole job", "scan": "scan stage", "clip stage": "clip stage (finish, align, far, ins, mei, files)",
              "library": "mei: the library into its own handle (read, upload, pack)", "mei": "mei: the calls into the library (launches, waits, columns read out)",
              "build": "mei: `sw_count`, `ks_carry_sum`, `sw_build` (device)", "kernel": "mei: `sw_align_wave` (device)", "reduce": "mei: `sw_reduce` (device)",
              "mei text": "mei: file text (host)"}
MEI_FAMILIES = (("AluGen", 300), ("SvaGen", 2000), ("L1Gen", 6100), ("HervGen", 7600))     # 16 kb in the proportions of the families the switch is for


def _generated_library(path):
    import numpy
    lib = [(n, "".join("ACGT"[i] for i in numpy.random.RandomState(4000 + k).randint(0, 4, ln))) for k, (n, ln) in enumerate(MEI_FAMILIES)]
    with open(path, "w") as f:
        for n, t in lib:
            f.write(">%s\n%s\n" % (n, "\n".join(t[i:i + 60] for i in range(0, len(t), 60))))
    return lib


def _generated_queries(lib, n, length, seed):
    """n queries of ``length`` bases cut from the library at random, one base in twenty substituted, on either strand -> codes"""
    import numpy
    rs = numpy.random.RandomState(seed)
    out = []
    for _ in range(n):
        t = lib[rs.randint(len(lib))][1]
        at = rs.randint(0, len(t) - length + 1)
        q = numpy.array(["ACGT".index(c) for c in t[at:at + length]])
        hit = rs.randint(0, 20, length) == 0
        q[hit] = rs.randint(0, 4, int(hit.sum()))
        out.append((3 - q[::-1] if rs.randint(2) else q).tolist())
    return out


def main_mei(a):
    """--mei: the job with the switches off, with the four clip switches and with TIDDIT_CLIPS_MEI beside them, interleaved in one process,
    medians of --reps; then `sw_align_wave` alone on generated query tables, by device events"""
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, fasta, refseq, tiddit_clip_mei as M
    ctx = _native.default_context()
    runs = {m: [] for m in MEI_MODES}
    table = {}
    alone = []
    with tempfile.TemporaryDirectory() as d:
        lib_path = os.path.join(d, "families.fa")
        lib = _generated_library(lib_path)
        for i in range(a.reps + 1):                       # (the first round warms up)
            for mode in MEI_MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                on = mode != "off"
                rec = _one_job(cli, ctx, a.bam, a.ref, out, a.switch if on else None, a.align_switch if on else None, a.far_switch if on else None, MEI_KEYS,
                               a.ins_switch if on else None, None, lib_path if mode == "mei" else None)
                assert os.path.exists(out + ".clips.mei.tab") == (mode == "mei") and os.path.exists(out + ".clips.ins.tab") == on
                if i:
                    runs[mode].append(rec)
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "mei" and i == a.reps:
                    table = {l.split("\t")[1]: int(l.split("\t")[2]) for l in open(out + ".clips.mei.tab").read().split("\n") if l.startswith("SN\t")}
        # the kernel alone: 1024 generated queries of 272 and of 60 bases against the same library, device events round the launch
        handle = refseq.load_all(fasta.FastaFile(lib_path), ctx=ctx)
        bases = sum(len(t) for _, t in lib)
        try:
            for length in (272, 60):
                seq10, qlen = M.query_columns(_generated_queries(lib, 1024, length, 4100 + length))
                ms = []
                for _ in range(5):                        # (the first one warms up)
                    sn, cols = M.sw_align(seq10, qlen, handle, ctx=ctx, device=True)
                    ms.append(M.sw_align_timing(ctx).tolist())
                ms = ms[1:]
                cpl = (length + 63) // 64
                cells = 1024 * 2 * bases * length
                k = statistics.median(m[0] for m in ms)
                alone.append({"length": length, "queries": 1024, "cells": cells, "kernel_ms": [m[0] for m in ms], "reduce_ms": [m[1] for m in ms],
                              "cell_updates_per_s": cells / (k * 1e-3), "columns_per_lane": cpl, "lanes_with_a_column": (length + cpl - 1) // cpl,
                              "share_of_lane_columns_held": length / (64.0 * cpl), "named": int(sn[M.SN_INDEX["named"]]),
                              "median_score": float(statistics.median(cols[2].tolist()))})
        finally:
            handle.close()
    keys = ["wall"] + [short for short, _ in MEI_KEYS]
    med = lambda mode, key: statistics.median([r[key] for r in runs[mode] if r.get(key) is not None] or [float("nan")])
    sp = lambda mode, key: (lambda v: (max(v) - min(v), min(v), max(v)))([r[key] for r in runs[mode]])
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "switches": [a.switch, a.align_switch, a.far_switch, a.ins_switch],
           "library": MEI_FAMILIES, "SN": table, "median_s": {m: {k: med(m, k) for k in keys if any(k in r for r in runs[m])} for m in runs},
           "four_wall_spread_s": sp("four", "wall")[0], "four_scan_spread_s": sp("four", "scan")[0], "runs": runs, "alone": alone}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "clips_mei" + ("_%dmb.md" % a.mb if a.mb else ".md"))
    with open(path, "w") as f:
        f.write("# Inserted sequences named against a family library (`TIDDIT_CLIPS=%s TIDDIT_CLIPS_ALIGN=%s TIDDIT_CLIPS_FAR=%s TIDDIT_CLIPS_INS=%s TIDDIT_CLIPS_MEI=library.fa`)\n\n"
                % (a.switch, a.align_switch, a.far_switch, a.ins_switch))
        f.write("File: `%s` (%.0f MB).  `tools/time_clips.py --mei`: one process, after one warm-up round %d rounds of { switches off, the four clip switches, the "
                "four and `TIDDIT_CLIPS_MEI` on a generated library of %d bases (%s) }, interleaved.  Wall seconds unless a row says device.  The yardstick is the "
                "four-switch job of the same process and the spread of its runs; no number was fixed in advance, this is what was measured.\n\n" % (
                    os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, a.reps, bases,
                    ", ".join("%s %d" % kv for kv in MEI_FAMILIES)))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in runs:
            for key in keys:
                if not any(key in r for r in runs[mode]):
                    continue
                f.write("| %s: %s | %s | %.5f |\n" % (mode, MEI_LABELS[key], " | ".join("%.5f" % r.get(key, float("nan")) for r in runs[mode]), med(mode, key)))
        inside = abs(med("mei", "scan") - med("four", "scan")) <= sp("four", "scan")[0]
        f.write("\nScan stage, mei against the four-switch median: %+.4f s; the four-switch runs' spread is %.4f s (min %.4f, max %.4f).  Whole job: %+.4f s; spread "
                "%.4f s (min %.4f, max %.4f).  The off runs' whole-job spread is %.4f s.\n" % (
                    (med("mei", "scan") - med("four", "scan"),) + sp("four", "scan") + (med("mei", "wall") - med("four", "wall"),) + sp("four", "wall") +
                    (sp("off", "wall")[0],)))
        f.write("\nThe only claim checked here is that the scan stage stays inside that spread, because the stage runs behind the scan and adds no launch per "
                "batch.  Here: %s.\n" % ("inside the spread, the claim stands for this file" if inside else
                                        "OUTSIDE the spread: the claim is not supported by this run, although the switch changes nothing the scan runs"))
        f.write("\nThe file's counters: %s.  The synthetic file's reads are cut from the reference in one piece, so it yields no pair and no query: the job rows "
                "are the cost of the stage's set-up (the library read, uploaded and packed into its own handle, the query build's launches, the file), not of any "
                "alignment — `sw_align_wave` is launched only when there is a query.\n" % ", ".join("%s %d" % kv for kv in table.items()))
        f.write("\n`sw_align_wave` alone, between two device events, 4 runs after a warm-up, through `tdt_sw_align_device` (1024 queries cut from the library, one base "
                "in twenty substituted, either strand; 2 x 4 = 8 problems per query, one wavefront each):\n\n| query bases | columns per lane | lanes with a column | share "
                "of the 64 x columns held | cell updates | kernel ms (4 runs) | median | cell updates per s | reduction ms (median) |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in alone:
            f.write("| %d | %d | %d of 64 | %.3f | %.3g | %s | %.3f | %.3g | %.4f |\n" % (
                r["length"], r["columns_per_lane"], r["lanes_with_a_column"], r["share_of_lane_columns_held"], r["cells"], ", ".join("%.3f" % v for v in r["kernel_ms"]),
                statistics.median(r["kernel_ms"]), r["cell_updates_per_s"], statistics.median(r["reduce_ms"])))
        f.write("\nA cell update is the definition's: three 64-bit keys (`H`, `E`, `F`), each penalty a 64-bit compare, select and subtract, each maximum a 64-bit "
                "compare and two selects; per step a lane also pays two 64-bit cross-lane shifts and one 32-bit cross-lane read, whatever its columns.  What bounds "
                "the rate was not measured (no profiler run): the kernel reads a nibble per family base and writes 12 bytes per problem, so it is not the memory; "
                "the longest problem (the %d-base family, %d + lanes steps by one wavefront) sets the tail of the launch, and 8192 problems over 256 compute units "
                "x 4 SIMDs leave most SIMDs with 8 resident waves at the start and few at the end.  No target was set for this rate and nothing in the tree did this "
                "work before.\n" % (max(ln for _, ln in MEI_FAMILIES), max(ln for _, ln in MEI_FAMILIES)))
        f.write("\nNot measured by this record: a real library's divergence (real consensus against real insertions align with many more gaps and lower scores "
                "than one substitution in twenty) and real insertion counts (the job part ran without a single query); libraries beyond 16 kb; the kernel under a "
                "profiler.\n")


INS_MODES = ("off", "clips", "ins")
INS_KEYS = (("scan", "signal extraction + coverage"), ("push", "clip keys (push)"), ("ingest wait", "ingest (inflate + decode, device)"),
            ("clip stage", "clip sites ({o}.clips.tab)"), ("ins", "clip ins (device: extension finish, gather, pairs)"),
            ("ext finish", "clip ins extension finish (sort, run lengths, vote) (device time)"), ("gather", "clip ins gather of the extended consensus (device time)"),
            ("pairs", "clip ins pair count + closure (device time)"), ("ins text", "clip ins table text (host)"))
INS_LABELS = {"wall": "whole job", "scan": "scan stage", "push": "stage timer of the pushes (host side, reserve waits included)",
              "ingest wait": "scan: waited for the ingest", "clip stage": "clip stage (finish, ins, files)",
              "ins": "ins: the calls into the library (launches, waits, columns read out)",
              "ext finish": "ins: the extension store's finish, between its events (device, with the host's waits between the launches)",
              "gather": "ins: `clip_ext_gather` (device)", "pairs": "ins: `clip_ins_count` x 2, `ks_carry_sum`, `clip_ins_pairs` (device, with the host's wait for the count)",
              "ins text": "ins: file text (host)"}


def main_ins(a):
    """--ins: the job with the switches off, with TIDDIT_CLIPS alone and with TIDDIT_CLIPS_INS beside it, interleaved in one process,
    medians of --reps; then every batch's push with and without the extension kernel, the stream idle"""
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, tiddit_clips
    ctx = _native.default_context()
    S, Q, L = tiddit_clips.parse_switch(a.switch)
    runs = {m: [] for m in INS_MODES}
    table = {}
    n_rows = 0
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up)
            for mode in INS_MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                rec = _one_job(cli, ctx, a.bam, a.ref, out, a.switch if mode != "off" else None, None, None, INS_KEYS, a.ins_switch if mode == "ins" else None)
                assert os.path.exists(out + ".clips.ins.tab") == (mode == "ins") and os.path.exists(out + ".clips.tab") == (mode != "off")
                if i:
                    runs[mode].append(rec)
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "ins" and i == a.reps:
                    lines = open(out + ".clips.ins.tab").read().split("\n")
                    table = {l.split("\t")[1]: int(l.split("\t")[2]) for l in lines if l.startswith("SN\t")}
                    n_rows = sum(1 for l in lines if l and not l.startswith(("#", "SN\t")))
    alone, both = keys_alone(a.bam, Q, L), keys_alone(a.bam, Q, L, ext=True)
    keys = ["wall"] + [short for short, _ in INS_KEYS]
    med = lambda mode, key: statistics.median([r[key] for r in runs[mode] if r.get(key) is not None] or [float("nan")])
    sp = lambda mode, key: (lambda v: (max(v) - min(v), min(v), max(v)))([r[key] for r in runs[mode]])
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "switch": a.switch, "ins": a.ins_switch, "SN": table, "rows": n_rows,
           "median_s": {m: {k: med(m, k) for k in keys if any(k in r for r in runs[m])} for m in runs}, "clips_alone_wall_spread_s": sp("clips", "wall")[0],
           "clips_alone_scan_spread_s": sp("clips", "scan")[0], "runs": runs, "clip_keys_alone": alone, "clip_keys_and_ext_keys": both}
    print(json.dumps(res))
    write_ins_record(res, a.out or os.path.join(REPO, "profiles", "clips_ins" + ("_%dmb.md" % a.mb if a.mb else ".md")))


def write_ins_record(res, path):
    """the record of --ins from its result line (also: --render FILE.json, which writes the record of a saved line again)"""
    runs, table, n_rows, alone, both = res["runs"], res["SN"], res["rows"], res["clip_keys_alone"], res["clip_keys_and_ext_keys"]
    keys = ["wall"] + [short for short, _ in INS_KEYS]
    med = lambda mode, key: statistics.median([r[key] for r in runs[mode] if r.get(key) is not None] or [float("nan")])
    sp = lambda mode, key: (lambda v: (max(v) - min(v), min(v), max(v)))([r[key] for r in runs[mode]])

    class a:
        bam, reps, switch, ins_switch = res["bam"], res["reps"], res["switch"], res["ins"]
    size = res["bam_MB"] * 1e6
    with open(path, "w") as f:
        f.write("# Insertion candidates from facing clip sites (`TIDDIT_CLIPS=%s TIDDIT_CLIPS_INS=%s`)\n\n" % (a.switch, a.ins_switch))
        f.write("File: `%s` (%.0f MB).  `tools/time_clips.py --ins`: one process, after one warm-up round %d rounds of { switches off, `TIDDIT_CLIPS` alone, "
                "`TIDDIT_CLIPS` + `TIDDIT_CLIPS_INS` }, interleaved.  Wall seconds unless a row says device.  The yardstick is the `TIDDIT_CLIPS`-alone job of the "
                "same process and the spread of its runs; no budget was fixed in advance, this is what was measured.\n\n" % (
                    os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), size / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in runs:
            for key in keys:
                if not any(key in r for r in runs[mode]):
                    continue
                f.write("| %s: %s | %s | %.5f |\n" % (mode, INS_LABELS[key], " | ".join("%.5f" % r.get(key, float("nan")) for r in runs[mode]), med(mode, key)))
        f.write("\nScan stage, ins against the `TIDDIT_CLIPS`-alone median: %+.4f s; the `TIDDIT_CLIPS`-alone runs' spread is %.4f s (min %.4f, max %.4f).  Whole job: "
                "%+.4f s; spread %.4f s (min %.4f, max %.4f).  The off runs' whole-job spread is %.4f s.\n" % (
                    (med("ins", "scan") - med("clips", "scan"),) + sp("clips", "scan") + (med("ins", "wall") - med("clips", "wall"),) + sp("clips", "wall") +
                    (sp("off", "wall")[0],)))
        f.write("\nThe expectation was that the push hides under the next span's inflate, as `clip_keys` does.  The scan stage's difference above against the "
                "spread beside it is the answer this file gives: a difference inside the spread confirms it for this file, one outside it refutes it.\n")
        cap = min(max(int(size) // 16, 1 << 16), 1 << 26)
        room = 8 * max(r["reads"] for r in both)
        f.write("\nThe pushes' stage timer (host side) is %.2f ms with `TIDDIT_CLIPS` alone and %.2f ms here.  It holds the waits of a reserve that has to ask "
                "the device: room for 8 keys per read is reserved before each launch, %d slots for the largest batch of this file, and the extension store is "
                "made for %d keys (file size / 16, at most 2^26), so %s.  An ask drains the stream, the batch's ingest included.  (Derived from the "
                "policy, not counted: the handle reports the first store's reserve only.)\n" % (
                    med("clips", "push") * 1e3, med("ins", "push") * 1e3, room, cap,
                    "a second batch's bound never fits behind the first's and the reserve asks the device for the real count before nearly every launch" if 2 * room > cap
                    else "the bounds of %d batches fit before the reserve asks the device for the real count" % (cap // room)))
        f.write("\nOn the device: the extension store's finish %.3f ms (%d keys; the figure is between two events round two sorts, the run-length and the site "
                "launches and holds the host's waits between them), `clip_ext_gather` %.3f ms over %d reported sites, the pair launches %.3f ms (%d pairs; "
                "the host's wait for the pair count lies inside).  The text of the file: %.3f ms on the host.\n" % (
                    med("ins", "ext finish") * 1e3, table.get("ext_keys", 0), med("ins", "gather") * 1e3,
                    table.get("left_sites", 0) + table.get("right_sites", 0), med("ins", "pairs") * 1e3, table.get("pairs", 0), med("ins", "ins text") * 1e3))
        f.write("\nThe table: %s; %d rows.\n" % (", ".join("%s %d" % kv for kv in table.items()), n_rows))
        f.write("\nThe push of one batch, the stream idle around it, best of 4, host clock around launch and sync (the launch latency is in it): `clip_keys` "
                "alone, and `clip_keys` + `clip_ext_keys` on a handle with the extension store.  The difference is what `clip_ext_keys` adds when nothing "
                "overlaps it; the `TIDDIT_CLIPS`-alone runs' scan-stage spread beside these figures is %.1f ms:\n\n| batch | reads | raw MB | clip_keys ms | both ms | "
                "difference ms |\n|---|---|---|---|---|---|\n" % (sp("clips", "scan")[0] * 1e3))
        for k, (r, q) in enumerate(zip(alone, both)):
            f.write("| %d | %d | %.1f | %.3f | %.3f | %+.3f |\n" % (k, r["reads"], r["raw_bytes"] / 1e6, r["ms"], q["ms"], q["ms"] - r["ms"]))
        f.write("\nThe synthetic file's reads are cut from the reference in one piece (`synth_bam.write_wgs_sv_bam` with `ref_seqs`), a clip included, so no "
                "insertion is planted and few pairs or none are expected: the figures are the cost of the stage, not a result.  Unmeasured until someone has "
                "real libraries: their clip density, sites with thousands of events, long reads (the cap of 140 columns).\n")


FAR_MODES = ("off", "clips", "far")
FAR_KEYS = (("scan", "signal extraction + coverage"), ("reference", "reference into HBM (TIDDIT_CLIPS_FAR)"), ("clip stage", "clip sites ({o}.clips.tab)"),
            ("far", "clip far (device: seed table, sort, one scan of the packed reference, rows)"), ("seeds", "clip far seeds + filter (device time)"),
            ("sort", "clip far sort (device time)"), ("far_scan", "clip far scan (device time)"), ("rows", "clip far rows (device time)"),
            ("far text", "clip far mates + table text (host)"), ("kernel", "clip align kernel (device time)"))
FAR_LABELS = {"wall": "whole job", "scan": "scan stage", "reference": "reference into HBM (read, upload, pack)", "clip stage": "clip stage (finish, far, files)",
              "far": "far: the calls into the library (launches, wait, six columns read out)", "seeds": "far: memsets + `far_seeds` (device)",
              "sort": "far: the sort's launches (device)", "far_scan": "far: `far_scan` (device)", "rows": "far: `far_rows` (device)",
              "far text": "far: mates and file text (host)", "kernel": "`clip_align_sites` at W = 2^20 (device)"}


def stream_read_rate(ctx, nbytes):
    """what a plain streaming read of ``nbytes`` of device memory reaches (tdt_calib_stream_read, bench.py's roofline.stream_read), GB/s"""
    import ctypes
    import torch
    from tiddit_amd import _native
    cal = torch.empty(max(nbytes // 8, 1 << 20), dtype=torch.int64, device="cuda")
    cal.random_(0, 1 << 40)
    torch.cuda.synchronize()
    rate = 0.0
    for wpc, blocked in ((2, 0), (8, 0), (8, 1)):
        cb, cm = ctypes.c_double(0), ctypes.c_double(0)
        _native.check(ctx.lib.tdt_calib_stream_read(ctx.handle, cal.data_ptr(), cal.numel() * 8, 10, wpc, blocked, ctypes.byref(cb), ctypes.byref(cm)))
        rate = max(rate, cal.numel() * 8 / (cm.value * 1e-3) / 1e9)
    return rate


def main_far(a):
    """--far: the job with the switches off, with TIDDIT_CLIPS alone and with TIDDIT_CLIPS_FAR beside it, interleaved in one process,
    medians of --reps; then TIDDIT_CLIPS_ALIGN at W = 2^20 on the same sites, the brute force the seeded scan replaces"""
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, bamio, tiddit_clip_align, tiddit_clip_far
    ctx = _native.default_context()
    K, M = tiddit_clip_far.parse_switch(a.far_switch)
    widest = "%d:%d:%d" % (tiddit_clip_align.MAX_WINDOW, K, M)
    rd = bamio.BamReader(a.bam, batch_bytes=1 << 20)
    lengths = [int(c["LN"]) for c in rd.header["SQ"]]
    rd.close()
    genome = sum(lengths)
    store = 16 + sum((n + 15) // 16 * 8 + 16 for n in lengths)          # the packed store's bytes (refseq.RefSeq.layout)
    runs = {m: [] for m in FAR_MODES + ("widest",)}
    table = wide = {}
    sn_of = lambda path: {l.split("\t")[1]: int(l.split("\t")[2]) for l in open(path).read().split("\n") if l.startswith("SN\t")}
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up)
            for mode in FAR_MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                rec = _one_job(cli, ctx, a.bam, a.ref, out, a.switch if mode != "off" else None, None, a.far_switch if mode == "far" else None, FAR_KEYS)
                assert os.path.exists(out + ".clips.far.tab") == (mode == "far") and os.path.exists(out + ".clips.tab") == (mode != "off")
                if i:
                    runs[mode].append(rec)
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "far" and i == a.reps:
                    table = sn_of(out + ".clips.far.tab")
                    types = {}
                    for l in open(out + ".clips.far.tab").read().split("\n"):
                        if l and not l.startswith(("#", "SN\t")):
                            types[l.split("\t")[10]] = types.get(l.split("\t")[10], 0) + 1
        for i in range(a.reps + 1):
            out = os.path.join(d, "w%d" % i)
            rec = _one_job(cli, ctx, a.bam, a.ref, out, a.switch, widest, None, FAR_KEYS)
            if i:
                runs["widest"].append(rec)
            if i == a.reps:
                wide = sn_of(out + ".clips.align.tab")
            print("widest %d: %.3f s, kernel %.3f ms" % (i, rec["wall"], rec.get("kernel", 0) * 1e3), file=sys.stderr, flush=True)
    rate = stream_read_rate(ctx, store)
    keys = ["wall"] + [short for short, _ in FAR_KEYS]
    med = lambda mode, key: statistics.median([r[key] for r in runs[mode] if r.get(key) is not None] or [float("nan")])
    base, offw = [r["wall"] for r in runs["clips"]], [r["wall"] for r in runs["off"]]
    scan_ms, brute_ms = med("far", "far_scan") * 1e3, med("widest", "kernel") * 1e3
    brute_scaled = brute_ms * genome / (2.0 * tiddit_clip_align.MAX_WINDOW + 1)
    stream_ms = store / (rate * 1e9) * 1e3
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "switch": a.switch, "far": a.far_switch, "SN": table, "TYPE": types,
           "SN_align_widest": wide, "genome_bases": genome, "store_bytes": store, "stream_read_GB_per_s": rate, "far_scan_ms": scan_ms,
           "clip_align_widest_ms": brute_ms, "clip_align_scaled_to_genome_ms": brute_scaled, "far_scan_frac_of_stream_read": stream_ms / scan_ms if scan_ms else None,
           "median_s": {m: {k: med(m, k) for k in keys if any(k in r for r in runs[m])} for m in runs}, "clips_alone_wall_spread_s": max(base) - min(base),
           "off_wall_spread_s": max(offw) - min(offw), "runs": runs}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "clips_far" + ("_%dmb.md" % a.mb if a.mb else ".md"))
    with open(path, "w") as f:
        f.write("# Clip-site consensus placed genome-wide by a seeded search (`TIDDIT_CLIPS=%s TIDDIT_CLIPS_FAR=%s`)\n\n" % (a.switch, a.far_switch))
        f.write("File: `%s` (%.0f MB), %d contigs, %d bases; the packed store is %d bytes.  `tools/time_clips.py --far`: one process, after one warm-up round "
                "%d rounds of { switches off, `TIDDIT_CLIPS` alone, `TIDDIT_CLIPS` + `TIDDIT_CLIPS_FAR` }, interleaved; then %d jobs with "
                "`TIDDIT_CLIPS_ALIGN=%s` on the same sites.  Wall seconds unless a row says device.  The yardstick is the `TIDDIT_CLIPS`-alone job of the "
                "same process and the spread of its runs; no threshold was fixed in advance, this is what was measured.\n\n" % (
                    os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, len(lengths), genome, store, a.reps, a.reps,
                    widest))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in runs:
            for key in keys:
                if not any(key in r for r in runs[mode]):
                    continue
                f.write("| %s: %s | %s | %.5f |\n" % (mode, FAR_LABELS[key], " | ".join("%.5f" % r.get(key, float("nan")) for r in runs[mode]), med(mode, key)))
        f.write("\nWhole job, far against the `TIDDIT_CLIPS`-alone median: %+.4f s; the `TIDDIT_CLIPS`-alone runs' spread is %.4f s (min %.4f, max %.4f), the off "
                "runs' %.4f s.  The reference going into HBM is %.4f s of it, which `TIDDIT_INDELS_NORM` / `TIDDIT_SNVS` / `TIDDIT_CLIPS_ALIGN` pay already when they "
                "are on.\n" % (med("far", "wall") - med("clips", "wall"), max(base) - min(base), min(base), max(base), max(offw) - min(offw), med("far", "reference")))
        f.write("\n`far_scan`: %.3f ms (device) for %d sites (%d searched: %d table entries) over %d bases.  The brute force it replaces, `clip_align_sites` at "
                "W = 2^20 on the same sites (%d searched there): %.3f ms for 2^21 + 1 starts per site, which scaled to the genome's length is %.1f ms — an "
                "extrapolation, not a measurement.  A plain streaming read of the store's %d bytes at `roofline.stream_read` (%.0f GB/s measured in this "
                "process) would take %.4f ms: `far_scan` runs at %.3f of it, so it is not bound by the memory: every base costs two funnel shifts, a multiply and "
                "one read of the filter in LDS, and which of these bounds it was not measured (no profiler run; with this few sites the filter passes almost "
                "nothing, so table lookups and atomics are not it).  The seed launch (two memsets and `far_seeds`) is %.3f ms, the sort's launches %.3f "
                "ms, `far_rows` %.3f ms; the stage's host side (the library calls with their wait, then mates and text) %.5f s + %.5f s.\n" % (
                    scan_ms, table.get("sites", 0), table.get("searched", 0), 2 * table.get("searched", 0), genome, wide.get("searched", 0), brute_ms, brute_scaled, store,
                    rate, stream_ms, stream_ms / scan_ms if scan_ms else float("nan"), med("far", "seeds") * 1e3, med("far", "sort") * 1e3, med("far", "rows") * 1e3,
                    med("far", "far"), med("far", "far text")))
        f.write("\nThe table: %s.  TYPE of the rows: %s.\n" % (", ".join("%s %d" % kv for kv in table.items()), ", ".join("%s %d" % kv for kv in sorted(types.items()))))
        f.write("\nThe synthetic file plants no junction sequence: the bases of a read, its clip included, are cut from the reference in one piece "
                "(`synth_bam.write_wgs_sv_bam` with `ref_seqs`), so every site is expected to place as `REF` beside its own breakpoint: the figures are the "
                "cost of the search, not a result.  Not measured by this record: real libraries, ten thousand sites and more (the filter's hit rate grows with "
                "the table: %d entries set at most that many of its 2^19 bits here), repeat-rich seeds (a seed with millions of occurrences pays an atomic "
                "pair per wave and tile), 3 Gb, the kernel under a profiler.\n" % (2 * table.get("searched", 0)))


def main_align(a):
    """--align: the job with the switches off, with TIDDIT_CLIPS alone and with TIDDIT_CLIPS_ALIGN beside it, interleaved in one process,
    medians of --reps; then the aligned job at the widest window (W = 2^20).  The yardstick is the TIDDIT_CLIPS-alone job and its spread."""
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, tiddit_clip_align
    ctx = _native.default_context()
    W, K, M = tiddit_clip_align.parse_switch(a.align_switch)
    widest = "%d:%d:%d" % (tiddit_clip_align.MAX_WINDOW, K, M)
    runs = {m: [] for m in ALIGN_MODES + ("widest",)}
    table = {}
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up)
            for mode in ALIGN_MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                rec = _one_job(cli, ctx, a.bam, a.ref, out, a.switch if mode != "off" else None, a.align_switch if mode == "align" else None)
                assert os.path.exists(out + ".clips.align.tab") == (mode == "align") and os.path.exists(out + ".clips.tab") == (mode != "off")
                if i:
                    runs[mode].append(rec)
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "align" and i == a.reps:
                    table = {l.split("\t")[1]: int(l.split("\t")[2]) for l in open(out + ".clips.align.tab").read().split("\n") if l.startswith("SN\t")}
        for i in range(a.reps + 1):
            out = os.path.join(d, "w%d" % i)
            rec = _one_job(cli, ctx, a.bam, a.ref, out, a.switch, widest)
            if i:
                runs["widest"].append(rec)
            if i == a.reps:
                wide = {l.split("\t")[1]: int(l.split("\t")[2]) for l in open(out + ".clips.align.tab").read().split("\n") if l.startswith("SN\t")}
            print("widest %d: %.3f s, kernel %.3f ms" % (i, rec["wall"], rec.get("kernel", 0) * 1e3), file=sys.stderr, flush=True)
    keys = ["wall"] + [short for short, _ in ALIGN_KEYS]
    med = lambda mode, key: statistics.median([r[key] for r in runs[mode] if r.get(key) is not None] or [float("nan")])
    base = [r["wall"] for r in runs["clips"]]
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "switch": a.switch, "align": a.align_switch, "SN": table, "SN_widest": wide,
           "median_s": {m: {k: med(m, k) for k in keys if any(k in r for r in runs[m])} for m in runs}, "clips_alone_wall_spread_s": max(base) - min(base),
           "runs": runs}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "clips_align" + ("_%dmb.md" % a.mb if a.mb else ".md"))
    with open(path, "w") as f:
        f.write("# Clip-site consensus realigned to the reference (`TIDDIT_CLIPS=%s TIDDIT_CLIPS_ALIGN=%s`)\n\n" % (a.switch, a.align_switch))
        f.write("File: `%s` (%.0f MB).  `tools/time_clips.py --align`: one process, after one warm-up round %d rounds of { switches off, `TIDDIT_CLIPS` alone, "
                "`TIDDIT_CLIPS` + `TIDDIT_CLIPS_ALIGN` }, interleaved; then %d jobs at the widest window, `TIDDIT_CLIPS_ALIGN=%s`.  Wall seconds unless a "
                "row says device.  The yardstick is the `TIDDIT_CLIPS`-alone job of the same process and the spread of its runs; no budget was fixed in "
                "advance, this is what was measured.\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6,
                                                             a.reps, a.reps, widest))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in runs:
            for key in keys:
                if not any(key in r for r in runs[mode]):
                    continue
                f.write("| %s: %s | %s | %.5f |\n" % (mode, ALIGN_LABELS[key], " | ".join("%.5f" % r.get(key, float("nan")) for r in runs[mode]), med(mode, key)))
        f.write("\nWhole job, aligned against the `TIDDIT_CLIPS`-alone median: %+.4f s; the `TIDDIT_CLIPS`-alone runs' spread is %.4f s (min %.4f, max %.4f).  Most of "
                "the difference is the reference going into HBM (%.4f s), which `TIDDIT_INDELS_NORM` / `TIDDIT_SNVS` pay already when they are on.\n" % (
                    med("align", "wall") - med("clips", "wall"), max(base) - min(base), min(base), max(base), med("align", "reference")))
        f.write("\nThe kernel: %.3f ms at W = %d for %d sites (%d searched), %.3f ms at W = 2^20 (%d searched; up to 2 x (2^21 + 1) candidates per site).\n" % (
            med("align", "kernel") * 1e3, W, table.get("sites", 0), table.get("searched", 0), med("widest", "kernel") * 1e3, wide.get("searched", 0)))
        f.write("\nThe table at W = %d: %s.  At W = 2^20: %s.\n" % (W, ", ".join("%s %d" % kv for kv in table.items()), ", ".join("%s %d" % kv for kv in wide.items())))
        f.write("\nThe synthetic file plants no junction sequence: the bases of a read, its clip included, are cut from the reference in one piece "
                "(`synth_bam.write_wgs_sv_bam` with `ref_seqs`), so what aligns here aligns as `REF` with `LEN` 0 (%d of %d searched sites) and no DEL / DUP / "
                "INV is expected: the figures are the cost of the search, not a result.  Not measured by this record: real libraries (sites by the ten "
                "thousand, repeats with many HITS), the kernel under a profiler (occupancy, the share of the loads), contigs far longer than the window's "
                "reach.\n" % (table.get("ref", 0), table.get("searched", 0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--switch", default="1")
    ap.add_argument("--align", action="store_true", help="measure TIDDIT_CLIPS_ALIGN against the TIDDIT_CLIPS-alone job instead")
    ap.add_argument("--align-switch", default="1")
    ap.add_argument("--far", action="store_true", help="measure TIDDIT_CLIPS_FAR against the TIDDIT_CLIPS-alone job instead")
    ap.add_argument("--far-switch", default="1")
    ap.add_argument("--ins", action="store_true", help="measure TIDDIT_CLIPS_INS against the TIDDIT_CLIPS-alone job instead")
    ap.add_argument("--ins-switch", default="1")
    ap.add_argument("--vcf", action="store_true", help="measure TIDDIT_CLIPS_VCF against the job with the four clip switches instead")
    ap.add_argument("--vcf-switch", default="1")
    ap.add_argument("--mei", action="store_true", help="measure TIDDIT_CLIPS_MEI against the job with the four clip switches instead")
    ap.add_argument("--render", help="write the --ins record of a saved result line (FILE.json) again; needs --out")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.render:
        return write_ins_record(json.loads(open(a.render).read().strip().split("\n")[-1]), a.out)
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    print("file: %s" % a.bam, file=sys.stderr, flush=True)
    if a.align:
        return main_align(a)
    if a.far:
        return main_far(a)
    if a.vcf:
        return main_vcf(a)
    if a.ins:
        return main_ins(a)
    if a.mei:
        return main_mei(a)
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, tiddit_clips
    S, Q, L = tiddit_clips.parse_switch(a.switch)
    ctx = _native.default_context()
    runs = {m: [] for m in MODES}
    notes = []
    table, n_rows = {}, 0
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                os.environ.pop("TIDDIT_CLIPS", None)
                if mode == "on":
                    os.environ["TIDDIT_CLIPS"] = a.switch
                buf = io.StringIO()
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(buf):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_CLIPS", None)
                Sx = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
                rec = {"wall": time.perf_counter() - t0}
                rec.update({short: Sx[key] for short, key in KEYS if key in Sx})
                assert os.path.exists(out + ".clips.tab") == (mode == "on")
                if i:
                    runs[mode].append(rec)
                    if mode == "on":
                        notes.append({k: cli.STAGE_NOTES.get(k) for k in NOTES})
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "on" and i == a.reps:
                    lines = open(out + ".clips.tab").read().split("\n")
                    table = {l.split("\t")[1]: int(l.split("\t")[2]) for l in lines if l.startswith("SN\t")}
                    n_rows = sum(1 for l in lines if l and not l.startswith(("#", "SN\t")))
    alone = keys_alone(a.bam, Q, L)

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None

    def spread(key):
        v = [r[key] for r in runs["off"] if r.get(key) is not None]
        return max(v) - min(v) if v else None
    keys = ["wall"] + [short for short, _ in KEYS]
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "switch": a.switch, "SN": table, "rows": n_rows,
           "median_s": {m: {k: med(m, k) for k in keys} for m in MODES}, "off_spread_s": {k: spread(k) for k in ("wall", "scan")}, "runs": runs,
           "reserve": notes, "clip_keys_alone": alone}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "clips" + ("_%dmb.md" % a.mb if a.mb else ".md"))
    with open(path, "w") as f:
        f.write("# The clipped-read breakpoint sites of `tiddit --sv` (`TIDDIT_CLIPS=%s`)\n\n" % a.switch)
        f.write("File: `%s` (%.0f MB).  `tools/time_clips.py`: one process, after one warm-up round %d rounds of { `--sv --skip_assembly` switch off, "
                "switch on }, interleaved.  Wall seconds unless a row says device; the yardstick is the off job of the same process; no budget was fixed "
                "in advance, this is what was measured.\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam),
                                                                 os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in MODES:
            for key in keys:
                if med(mode, key) is None:
                    continue
                f.write("| %s: %s | %s | %.4f |\n" % (mode, LABELS[key], " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        off, offw = [r["scan"] for r in runs["off"]], [r["wall"] for r in runs["off"]]
        f.write("\nScan stage, on against the off median: %+.4f s; the off runs' spread is %.4f s (min %.4f, max %.4f).  Whole job, on against the off "
                "median: %+.4f s; the off runs' spread is %.4f s (min %.4f, max %.4f).\n" % (
                    med("on", "scan") - med("off", "scan"), max(off) - min(off), min(off), max(off), med("on", "wall") - med("off", "wall"),
                    max(offw) - min(offw), min(offw), max(offw)))
        f.write("\nThe reserve (room for 2 keys per read before each launch), per on run: " +
                "; ".join("asked the device %s times, grew the store %s times, capacity %s keys, %s keys stored" % tuple(n[k] for k in NOTES) for n in notes) + ".\n")
        f.write("\nThe file: %d records, %d eligible (MAPQ >= %d); %d clipped reads with %d leading and %d trailing clips of %d bases or more, %d shorter "
                "clips, %d clips cut at a base that is not A C G T, %d records without sequence, %d without alignment, %d malformed; %d distinct sequences at "
                "%d sites, %d reported at a support of %d (%d rows in the file).\n" % (
                    table.get("records", 0), table.get("eligible", 0), Q, table.get("clipped_reads", 0), table.get("left_clips", 0), table.get("right_clips", 0), L,
                    table.get("short_clips", 0), table.get("cut_at_other_base", 0), table.get("no_sequence", 0), table.get("no_alignment", 0),
                    table.get("malformed", 0), table.get("distinct_sequences", 0), table.get("distinct_sites", 0), table.get("reported_sites", 0), S, n_rows))
        if med("on", "sort K2") is not None:
            dev = sum(med("on", k) for k in ("sort K2", "gather", "sort K1", "runs", "sites"))
            f.write("\nFinish on the device: %.3f ms for %d keys, of which the site launches (heads, vote, rows) are %.3f ms; the off runs' whole-job "
                    "spread beside it is %.1f ms.\n" % (dev * 1e3, table.get("left_clips", 0) + table.get("right_clips", 0), med("on", "sites") * 1e3,
                                                       (max(offw) - min(offw)) * 1e3))
        f.write("\n`clip_keys` alone (one batch, the stream idle around it, best of 4, host clock around launch and sync: the launch latency is in it); the "
                "off runs' scan-stage spread beside these figures is %.1f ms:\n\n| batch | reads | raw MB | ms | reads per us | raw GB/s (nominal: the launch reads the columns, and of the records only headers, CIGARs and clipped bases) |\n|---|---|---|---|---|---|\n"
                % ((max(off) - min(off)) * 1e3))
        for k, r in enumerate(alone):
            f.write("| %d | %d | %.1f | %.3f | %.0f | %.0f |\n" % (k, r["reads"], r["raw_bytes"] / 1e6, r["ms"], r["reads"] / (r["ms"] * 1e3),
                                                                  r["raw_bytes"] / (r["ms"] * 1e-3) / 1e9))
        f.write("\nNot measured by this record: real libraries (their clip density, sites of tens of thousands of distinct sequences, a finish over "
                "millions of keys), the kernels under a profiler (per-launch device times of `clip_keys` and of each site launch), long reads, N ranks "
                "(refused).\n")


if __name__ == "__main__":
    main()
