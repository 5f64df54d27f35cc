"""What the read-level QC tables of `tiddit --sv` (TIDDIT_QC=1) cost the job: `tiddit --sv --skip_assembly` with the switch off and on,
interleaved, in one process — the whole job's wall, the scan stage, the new stage timer (the pushes' host side) and the read-out beside
them.  The yardstick is the same job without the switch in the same process, never an absolute number; for the base pass it is also the
bytes of raw records a batch holds against the device's streaming-read rate (tdt_calib_stream_read, what bench.py's roofline quotes as
`stream_read`).  The two kernels are also timed alone (host clock around launches and sync, the stream idle) on every batch of the file (`kernels alone`).  The tool reads from
the tables it has just made how many reads of the file carry qualities (`reads_no_qual`) and says so: the quality path is only timed
by a file whose reads have them.  Writes the record to profiles/qc_<mb>mb.md (or --out) and prints one JSON line.  With --profile
nothing is written: one warm-up and one run each way, for a `rocprofv3 --kernel-trace --stats -- python tools/time_qc.py ... --profile`
run of its own; --kernels FILE_kernel_stats.csv then puts that run's rows of the two kernels and of the scan's largest kernels into the
record.

usage: python tools/time_qc.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--profile] [--kernels FILE.csv] [--out FILE.md]
(--mb: bench.py's synthetic file of that genome size, made at $TIDDIT_BENCH_TMP/tiddit_bench_sv_<mb>/ when it is not there)"""
import argparse
import contextlib
import csv
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
KEYS = (("scan", "signal extraction + coverage"), ("push", "qc tables (push)"), ("ingest wait", "ingest (inflate + decode, device)"),
        ("file", "qc tables ({o}.qc.tab)"), ("read-out", "qc counters to the host"), ("text", "qc table text (host)"))


def kernel_rows(path, top=6):
    """the qc_* rows and the `top` largest rows of a rocprofv3 kernel_stats.csv -> [(name, calls, total ns, average ns)]"""
    with open(path) as f:
        rows = [(r.get("Name", ""), r.get("Calls"), r.get("TotalDurationNs"), r.get("AverageNs")) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: -int(r[2] or 0))
    keep = [r for i, r in enumerate(rows) if i < top or "qc_" in r[0]]
    return [(r[0].split("(")[0][:60],) + r[1:] for r in keep]


def kernels_alone(bam, ctx):
    """every batch of the file through tdt_qc_push_device with the stream idle around it -> per batch (reads, raw bytes, ms of the two
    launches together), and the streaming-read rate of the device over the largest batch's bytes"""
    import torch
    from tiddit_amd import _native, bamio, tiddit_qc
    rd = bamio.DeviceBamReader(bam)
    h = tiddit_qc.QcCounter(ctx=rd.ctx)
    rows = []
    try:
        for b in rd.batches():
            rd.ctx.sync()
            h.push_device_batch(b)                       # (warm: code objects, caches)
            rd.ctx.sync()
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                h.push_device_batch(b)
                rd.ctx.sync()
                dt = time.perf_counter() - t0
                best = dt if best is None or dt < best else best
            rows.append({"reads": len(b), "raw_bytes": int(b._raw_len), "ms": best * 1e3})
    finally:
        h.close()
        rd.close()
    big = max(r["raw_bytes"] for r in rows)
    cal = torch.empty(big // 8, dtype=torch.int64, device="cuda")
    cal.random_(0, 1 << 40)
    torch.cuda.synchronize()
    rate = 0.0
    for wpc, blocked in ((2, 0), (8, 0), (8, 1)):
        cb, cm = ctypes.c_double(0), ctypes.c_double(0)
        _native.check(ctx.lib.tdt_calib_stream_read(ctx.handle, cal.data_ptr(), cal.numel() * 8, 10, wpc, blocked, ctypes.byref(cb), ctypes.byref(cm)))
        rate = max(rate, cal.numel() * 8 / (cm.value * 1e-3) / 1e9)
    return rows, rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="one warm-up and one run each way, no record written (for rocprofv3)")
    ap.add_argument("--kernels", help="a rocprofv3 kernel_stats.csv of a --profile run: its rows go into the record")
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
    from tiddit_amd import _native
    ctx = _native.default_context()
    runs = {m: [] for m in MODES}
    table = {}
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                os.environ.pop("TIDDIT_QC", None)
                if mode == "on":
                    os.environ["TIDDIT_QC"] = "1"
                buf = io.StringIO()
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(buf):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_QC", None)
                S = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
                rec = {"wall": time.perf_counter() - t0}
                rec.update({short: S[key] for short, key in KEYS if key in S})
                assert os.path.exists(out + ".qc.tab") == (mode == "on")
                if i:
                    runs[mode].append(rec)
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "on" and i == a.reps:
                    table = {l.split("\t")[1]: int(l.split("\t")[2]) for l in open(out + ".qc.tab") if l.startswith("SN\t")}
    alone, rate = ([], None) if a.profile else kernels_alone(a.bam, ctx)

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = ["wall"] + [short for short, _ in KEYS]
    with_seq = table.get("primary", 0) - table.get("qc_fail", 0) - table.get("malformed", 0) - table.get("reads_no_seq", 0)
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "SN": table,
           "reads_with_qualities": (with_seq - table.get("reads_no_qual", 0)) / with_seq if with_seq > 0 else None,
           "median_s": {m: {k: med(m, k) for k in keys} for m in MODES}, "runs": runs, "kernels_alone": alone, "stream_read_GB_per_s": rate}
    print(json.dumps(res))
    if a.profile:
        return
    path = a.out or os.path.join(REPO, "profiles", "qc_%dmb.md" % a.mb if a.mb else "qc.md")
    with open(path, "w") as f:
        f.write("# The read-level QC tables of `tiddit --sv` (`TIDDIT_QC=1`)\n\n")
        f.write("File: `%s` (%.0f MB).  `tools/time_qc.py`: one process, after one warm-up round %d rounds of { `--sv --skip_assembly` switch off, "
                "switch on }, interleaved.  Wall seconds; the yardstick is the off job of the same process; no budget was fixed in advance, this is "
                "what was measured.\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        labels = {"wall": "whole job", "scan": "scan stage", "push": "new stage timer (pushes, host side)", "ingest wait": "scan: waited for the ingest",
                  "file": "counters off the device + file", "read-out": "counters to the host", "text": "file text"}
        for mode in MODES:
            for key in keys:
                if med(mode, key) is None:
                    continue
                f.write("| %s: %s | %s | %.4f |\n" % (mode, labels[key], " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        off = [r["scan"] for r in runs["off"]]
        f.write("\nScan stage, off runs: spread %.4f s (min %.4f, max %.4f).  Scan stage, on against the off median: %+.4f s.\n" % (
            max(off) - min(off), min(off), max(off), med("on", "scan") - med("off", "scan")))
        f.write("\nThe file: %d records, %d bases; %.1f %% of its reads with a sequence carry qualities (`reads_no_qual` %d), so the quality path "
                "(QUAL, qual_sum, q20 / q30) %s in the numbers above.\n" % (
                    table.get("records", 0), table.get("bases", 0), 100.0 * (res["reads_with_qualities"] or 0), table.get("reads_no_qual", 0),
                    "is" if (res["reads_with_qualities"] or 0) > 0.5 else "is NOT"))
        if alone:
            f.write("\nKernels alone (`qc_fields` + `qc_bases` of one batch, the stream idle around them, best of 3, host clock around launch and "
                    "sync); streaming-read rate of this device over %d MB: %.0f GB/s:\n\n| batch | reads | raw MB | ms | raw GB/s | of the streaming rate |\n"
                    "|---|---|---|---|---|---|\n" % (max(r["raw_bytes"] for r in alone) >> 20, rate))
            for k, r in enumerate(alone):
                gbs = r["raw_bytes"] / (r["ms"] * 1e-3) / 1e9
                f.write("| %d | %d | %.1f | %.3f | %.0f | %.2f |\n" % (k, r["reads"], r["raw_bytes"] / 1e6, r["ms"], gbs, gbs / rate))
        if a.kernels:
            f.write("\nKernels (`rocprofv3 --kernel-trace --stats`, a run of its own: one warm-up and one run each of off / on, so the two QC kernels "
                    "ran for two jobs' batches; the largest kernels of the four jobs beside them):\n\n"
                    "| kernel | calls | total ns | average ns |\n|---|---|---|---|\n")
            for row in kernel_rows(a.kernels):
                f.write("| `%s` | %s | %s | %s |\n" % row)


if __name__ == "__main__":
    main()
