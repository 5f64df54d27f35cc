"""What the duplicate metrics of `tiddit --sv` (TIDDIT_DUPS=1) cost the job: `tiddit --sv --skip_assembly` with the switch off and on,
interleaved, in one process — the whole job's wall, the scan stage, the new stage timer (the pushes' host side) and the finish stage
beside them, the finish split into its two sorts, the gather and the run-length launches (HIP events round them inside
tdt_dup_finish).  The yardstick is the same job without the switch in the same process, never an absolute number.  The key kernel is
also timed alone (host clock around launch and sync, the stream idle) on every batch of the file (`dup_keys alone`).  Writes the record
to profiles/dup_<mb>mb.md (or --out) and prints one JSON line.

usage: python tools/time_dup.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--out FILE.md]
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
KEYS = (("scan", "signal extraction + coverage"), ("push", "duplicates (push)"), ("ingest wait", "ingest (inflate + decode, device)"),
        ("finish", "duplicates ({o}.dup.tab)"), ("device", "duplicate sets (device: two sorts, gather, run lengths)"),
        ("sort K2", "sort by K2 (device time)"), ("gather", "gather of K1 (device time)"), ("sort K1", "sort by K1 (device time)"),
        ("runs", "run lengths + histogram (device time)"), ("text", "duplicate table text (host)"))
LABELS = {"wall": "whole job", "scan": "scan stage", "push": "new stage timer (pushes, host side)", "ingest wait": "scan: waited for the ingest",
          "finish": "finish stage (sort, run lengths, file)", "device": "finish: the call into the library", "sort K2": "finish: sort by K2 (device)",
          "gather": "finish: gather of K1 (device)", "sort K1": "finish: sort by K1 (device)", "runs": "finish: gather of K2 + run-length launches (device)",
          "text": "finish: file text"}


def keys_alone(bam):
    """every batch of the file through tdt_dup_push_device with the stream idle around it -> per batch (reads, raw bytes, ms of the launch)"""
    from tiddit_amd import bamio, tiddit_dup
    rd = bamio.DeviceBamReader(bam)
    h = tiddit_dup.DupCounter(len(rd.references), max(rd.lengths), capacity=os.path.getsize(bam) // 32, ctx=rd.ctx)
    rows = []
    try:
        for b in rd.batches():
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
        h.close()
        rd.close()
    return rows


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
    table = {}
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                os.environ.pop("TIDDIT_DUPS", None)
                if mode == "on":
                    os.environ["TIDDIT_DUPS"] = "1"
                buf = io.StringIO()
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(buf):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_DUPS", None)
                S = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
                rec = {"wall": time.perf_counter() - t0}
                rec.update({short: S[key] for short, key in KEYS if key in S})
                assert os.path.exists(out + ".dup.tab") == (mode == "on")
                if i:
                    runs[mode].append(rec)
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "on" and i == a.reps:
                    table = {l.split("\t")[1]: int(l.split("\t")[2]) for l in open(out + ".dup.tab") if l.startswith("SN\t")}
    alone = keys_alone(a.bam)

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = ["wall"] + [short for short, _ in KEYS]
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "SN": table,
           "median_s": {m: {k: med(m, k) for k in keys} for m in MODES}, "runs": runs, "dup_keys_alone": alone}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "dup_%dmb.md" % a.mb if a.mb else "dup.md")
    with open(path, "w") as f:
        f.write("# The duplicate metrics of `tiddit --sv` (`TIDDIT_DUPS=1`)\n\n")
        f.write("File: `%s` (%.0f MB).  `tools/time_dup.py`: one process, after one warm-up round %d rounds of { `--sv --skip_assembly` switch off, "
                "switch on }, interleaved.  Wall seconds unless a row says device; the yardstick is the off job of the same process; no budget was "
                "fixed in advance, this is what was measured.\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam),
                                                                     os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in MODES:
            for key in keys:
                if med(mode, key) is None:
                    continue
                f.write("| %s: %s | %s | %.4f |\n" % (mode, LABELS[key], " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        off = [r["scan"] for r in runs["off"]]
        f.write("\nScan stage, off runs: spread %.4f s (min %.4f, max %.4f).  Scan stage, on against the off median: %+.4f s.  Whole job, on against "
                "the off median: %+.4f s.\n" % (max(off) - min(off), min(off), max(off), med("on", "scan") - med("off", "scan"),
                                                med("on", "wall") - med("off", "wall")))
        stored = table.get("fragments", 0) + table.get("pairs", 0)
        f.write("\nThe file: %d records, %d eligible; %d keys stored (%d fragments, %d pairs, of which %d without a usable `MC`), %d mates without a "
                "key, %d malformed; %d pair sets, %d pair duplicates.\n" % tuple(table.get(k, 0) if k else stored for k in (
                    "records", "eligible", None, "fragments", "pairs", "pairs_no_mc", "pair_mates", "malformed", "pair_sets", "pair_duplicates")))
        if stored and med("on", "sort K2") is not None:
            dev = sum(med("on", k) for k in ("sort K2", "gather", "sort K1", "runs"))
            f.write("\nFinish on the device: %.2f ms for %d keys, %.2f ns per key.\n" % (dev * 1e3, stored, dev * 1e9 / stored))
        f.write("\n`dup_keys` alone (one batch, the stream idle around it, best of 4, host clock around launch and sync):\n\n"
                "| batch | reads | raw MB | ms | reads per us | raw GB/s |\n|---|---|---|---|---|---|\n")
        for k, r in enumerate(alone):
            f.write("| %d | %d | %.1f | %.3f | %.0f | %.0f |\n" % (k, r["reads"], r["raw_bytes"] / 1e6, r["ms"], r["reads"] / (r["ms"] * 1e3),
                                                                    r["raw_bytes"] / (r["ms"] * 1e-3) / 1e9))


if __name__ == "__main__":
    main()
