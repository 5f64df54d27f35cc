"""What the SNV candidates of `tiddit --sv` (TIDDIT_SNVS) cost the job: `tiddit --sv --skip_assembly` with the switch off and on,
interleaved, in one process — the whole job's wall and the scan stage off and on (with the spread of the off runs), the reference load,
the new stage timer (the pushes' host side: it also holds the waits of a reserve that has to ask the device), the finish stage split
into its two sorts, the gather and the run-length launches (HIP events round them inside tdt_snv_finish), the keys stored and how often
the reserve asked the device or grew the store.  The yardstick is the same job without the switch in the same process, never an
absolute number.  `snv_keys` is also timed alone (host clock around launch and sync, the stream idle, best of 4) on every batch of the
file, with its raw-bytes-per-second rate beside the 6.2 TB/s a plain streaming read reaches on the box (`roofline.stream_read`).  Writes
the record to profiles/snvs_<mb>mb.md (or --out) and prints one JSON line.

The synthetic file's reads are cut from the reference the job loads (bench.py's file: ``write_wgs_sv_bam(..., ref_seqs=...)``), so its
reads are not noisy; it holds no planted SNVs, so few keys are stored: what the record measures is the compare of every aligned base,
not a finish over millions of keys.

--profile: nothing is written: one warm-up and one run each way, for a `rocprofv3 --kernel-trace --output-format csv -- python
tools/time_snvs.py --mb 240 --profile` of its own; --kernels FILE: the *_kernel_trace.csv of such a run — `snv_keys` per batch and the
largest kernels go into the record.

usage: python tools/time_snvs.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--switch 1] [--profile] [--kernels FILE] [--out FILE.md]
(--mb: bench.py's synthetic file of that genome size, made at $TIDDIT_BENCH_TMP/tiddit_bench_sv_<mb>/ when it is not there)"""
import argparse
import contextlib
import csv
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

STREAM_READ_TBS = 6.2               # what a plain streaming read reaches on the box (README)
MODES = ("off", "on")
KEYS = (("scan", "signal extraction + coverage"), ("push", "snv keys (push)"), ("ingest wait", "ingest (inflate + decode, device)"),
        ("reference", "reference into HBM (TIDDIT_SNVS)"), ("ref read", "reference: file read (host)"),
        ("ref load", "reference: upload + ref_pack (returns when packed)"),
        ("finish", "snv candidates ({o}.snvs.tab)"), ("device", "snv sets (device: two sorts, gather, run lengths, rows)"),
        ("sort K2", "snv sort by K2 (device time)"), ("gather", "snv gather of K1 (device time)"), ("sort K1", "snv sort by K1 (device time)"),
        ("runs", "snv run lengths + rows (device time)"), ("text", "snv table text (host)"))
LABELS = {"wall": "whole job", "scan": "scan stage (the reference load runs inside it)", "push": "new stage timer (pushes, host side, reserve waits included)",
          "ingest wait": "scan: waited for the ingest", "reference": "reference into HBM (before the first batch)", "ref read": "reference: file read (host)",
          "ref load": "reference: upload + ref_pack (host clock, returns when packed)", "finish": "finish stage (sort, run lengths, rows, file)",
          "device": "finish: the calls into the library", "sort K2": "finish: sort by K2 (device)", "gather": "finish: gather of K1 (device)",
          "sort K1": "finish: sort by K1 (device)", "runs": "finish: gather of K2 + run-length and row launches (device)", "text": "finish: file text"}
NOTES = ("snv store: reserves that asked the device", "snv store: growths", "snv store: capacity (keys)", "snv store: keys")


def keys_alone(bam, fasta, min_mapq, min_bq):
    """every batch of the file through tdt_snv_push_device with the stream idle around it -> per batch (reads, raw bytes, ms of the launch)"""
    from tiddit_amd import bamio, refseq, tiddit_snvs
    from tiddit_amd.fasta import FastaFile
    rd = bamio.DeviceBamReader(bam)
    ref = refseq.load_for_bam(FastaFile(fasta), list(rd.references), list(rd.lengths), ctx=rd.ctx)[0]
    h = None
    rows = []
    try:
        for b in rd.batches():
            if h is None:                                # (room for the largest batch's bound: no reserve asks or grows inside the timing)
                h = tiddit_snvs.SnvCounter(len(rd.references), ref, min_mapq, min_bq, capacity=8 * len(b) + 4096, ctx=rd.ctx)
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
        ref.close()
        rd.close()
    return rows


def trace_rows(path, top=8):
    """a rocprofv3 *_kernel_trace.csv -> (every snv_keys dispatch's microseconds in order, [(kernel, calls, total us)] of the largest)"""
    snv, total = [], {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = (r.get("Kernel_Name") or "").split("(")[0][:60]
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
            if "snv_keys" in name:
                snv.append(us)
            c = total.setdefault(name, [0, 0.0])
            c[0] += 1
            c[1] += us
    big = sorted(total.items(), key=lambda kv: -kv[1][1])[:top]
    return snv, [(k, v[0], v[1]) for k, v in big]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--switch", default="1")
    ap.add_argument("--profile", action="store_true", help="one warm-up and one run each way, no record written (for rocprofv3)")
    ap.add_argument("--kernels", help="the *_kernel_trace.csv of a --profile run under rocprofv3: its rows go into the record")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    if a.profile:
        a.reps = 1
    print("file: %s" % a.bam, file=sys.stderr, flush=True)
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, tiddit_snvs
    S, Q, B = tiddit_snvs.parse_switch(a.switch)
    ctx = _native.default_context()
    runs = {m: [] for m in MODES}
    notes = []
    table, n_rows = {}, 0
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                os.environ.pop("TIDDIT_SNVS", None)
                if mode == "on":
                    os.environ["TIDDIT_SNVS"] = a.switch
                buf = io.StringIO()
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(buf):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_SNVS", None)
                Sx = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
                rec = {"wall": time.perf_counter() - t0}
                rec.update({short: Sx[key] for short, key in KEYS if key in Sx})
                assert os.path.exists(out + ".snvs.tab") == (mode == "on")
                if i:
                    runs[mode].append(rec)
                    if mode == "on":
                        notes.append({k: cli.STAGE_NOTES.get(k) for k in NOTES})
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "on" and i == a.reps:
                    lines = open(out + ".snvs.tab").read().split("\n")
                    table = {l.split("\t")[1]: int(l.split("\t")[2]) for l in lines if l.startswith("SN\t")}
                    n_rows = sum(1 for l in lines if l and not l.startswith(("#", "SN\t")))
    if a.profile:
        return
    alone = keys_alone(a.bam, a.ref, Q, B)

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = ["wall"] + [short for short, _ in KEYS]
    traced = trace_rows(a.kernels) if a.kernels else None
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "switch": a.switch, "SN": table, "rows": n_rows,
           "median_s": {m: {k: med(m, k) for k in keys} for m in MODES}, "runs": runs, "reserve": notes, "snv_keys_alone": alone,
           "snv_keys_traced_us": traced[0] if traced else None}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "snvs" + ("_%dmb.md" % a.mb if a.mb else ".md"))
    with open(path, "w") as f:
        f.write("# The SNV candidates of `tiddit --sv` (`TIDDIT_SNVS=%s`)\n\n" % a.switch)
        f.write("File: `%s` (%.0f MB), its reads cut from the reference the job loads.  `tools/time_snvs.py`: one process, after one warm-up round %d "
                "rounds of { `--sv --skip_assembly` switch off, switch on }, interleaved.  Wall seconds unless a row says device; the yardstick is the off "
                "job of the same process; no budget was fixed in advance, this is what was measured.\n\n" % (
                    os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in MODES:
            for key in keys:
                if med(mode, key) is None:
                    continue
                f.write("| %s: %s | %s | %.4f |\n" % (mode, LABELS[key], " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        off = [r["scan"] for r in runs["off"]]
        offw = [r["wall"] for r in runs["off"]]
        f.write("\nScan stage, off runs: spread %.4f s (min %.4f, max %.4f).  Scan stage, on against the off median: %+.4f s, of which the reference "
                "load is %.4f s.  Whole job, off runs: spread %.4f s.  Whole job, on against the off median: %+.4f s.\n" % (
                    max(off) - min(off), min(off), max(off), med("on", "scan") - med("off", "scan"), med("on", "reference") or 0.0, max(offw) - min(offw),
                    med("on", "wall") - med("off", "wall")))
        f.write("\nThe reserve (room for 8 keys per read before each launch), per on run: " +
                "; ".join("asked the device %s times, grew the store %s times, capacity %s keys, %s keys stored" % tuple(n[k] for k in NOTES) for n in notes) + ".\n")
        f.write("\nThe file: %d records, %d eligible (MAPQ >= %d); %d aligned bases compared; %d keys stored from %d reads, %d low-quality mismatches (below %d), "
                "%d noisy reads, %d off the reference, %d without sequence, %d malformed; %d distinct events, %d reported at a support of %d (%d rows in the "
                "file).\n" % (table.get("records", 0), table.get("eligible", 0), Q, table.get("aligned_bases", 0), table.get("mismatches", 0),
                              table.get("reads_with_events", 0), table.get("low_quality", 0), B, table.get("noisy_reads", 0), table.get("off_reference", 0),
                              table.get("no_sequence", 0), table.get("malformed", 0), table.get("distinct_events", 0), table.get("reported_events", 0), S, n_rows))
        if med("on", "sort K2") is not None:
            dev = sum(med("on", k) for k in ("sort K2", "gather", "sort K1", "runs"))
            f.write("\nFinish on the device: %.3f ms for %d keys.\n" % (dev * 1e3, table.get("mismatches", 0)))
        f.write("\n`snv_keys` alone (one batch, the stream idle around it, best of 4, host clock around launch and sync: the launch latency is in it), "
                "its raw record bytes per second beside the %.1f TB/s of a plain streaming read on the box:\n\n"
                "| batch | reads | raw MB | ms | reads per us | raw GB/s | of a streaming read |\n|---|---|---|---|---|---|---|\n" % STREAM_READ_TBS)
        for k, r in enumerate(alone):
            gbs = r["raw_bytes"] / (r["ms"] * 1e-3) / 1e9
            f.write("| %d | %d | %.1f | %.3f | %.0f | %.0f | %.3f |\n" % (k, r["reads"], r["raw_bytes"] / 1e6, r["ms"], r["reads"] / (r["ms"] * 1e3), gbs,
                                                                        gbs / (STREAM_READ_TBS * 1e3)))
        if traced:
            snv, big = traced
            f.write("\nKernels (`rocprofv3 --kernel-trace`, a run of its own: one warm-up and one run each of off / on).  `snv_keys`, every dispatch in order, "
                    "microseconds: %s.\n\n| kernel | calls | total us |\n|---|---|---|\n" % ", ".join("%.1f" % u for u in snv))
            for name, calls, us in big:
                f.write("| `%s` | %d | %.1f |\n" % (name, calls, us))
        f.write("\nNot measured by this record: real libraries (their mismatch density, base qualities and a finish over millions of keys), long reads, "
                "N ranks (refused).\n")


if __name__ == "__main__":
    main()
