"""What the small-indel candidates of `tiddit --sv` (TIDDIT_INDELS) cost the job: `tiddit --sv --skip_assembly` with the switch off and
on, interleaved, in one process — the whole job's wall, the scan stage, the new stage timer (the pushes' host side: it also holds the
waits of a reserve that has to ask the device) and the finish stage beside them, the finish split into its two sorts, the gather and
the run-length launches (HIP events round them inside tdt_indel_finish), and how often the reserve asked the device for the real count
of keys.  The yardstick is the same job without the switch in the same process, never an absolute number.  The key kernel is also timed
alone (host clock around launch and sync, the stream idle) on every batch of the file (`indel_keys alone`).  Writes the record to
profiles/indels_<mb>mb.md (or --out) and prints one JSON line.

--norm: a third job per round, TIDDIT_INDELS_NORM=1 beside the switch (the yardstick of the normalised job is TIDDIT_INDELS alone in the same
process): the reference load (file read; upload + ref_pack), the three new counters, and `indel_keys<true>` alone beside `indel_keys<false>`
on every batch; the record goes to profiles/indels_norm_<mb>mb.md.

usage: python tools/time_indels.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--switch 1] [--norm] [--out FILE.md]
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
KEYS = (("scan", "signal extraction + coverage"), ("push", "indel keys (push)"), ("ingest wait", "ingest (inflate + decode, device)"),
        ("finish", "small indels ({o}.indels.tab)"), ("device", "indel sets (device: two sorts, gather, run lengths, rows)"),
        ("sort K2", "sort by K2 (device time)"), ("gather", "gather of K1 (device time)"), ("sort K1", "sort by K1 (device time)"),
        ("runs", "run lengths + rows (device time)"), ("text", "indel table text (host)"),
        ("reference", "reference into HBM (TIDDIT_INDELS_NORM)"), ("ref read", "reference: file read (host)"),
        ("ref load", "reference: upload + ref_pack (returns when packed)"))
LABELS = {"wall": "whole job", "scan": "scan stage", "push": "new stage timer (pushes, host side, reserve waits included)",
          "ingest wait": "scan: waited for the ingest", "finish": "finish stage (sort, run lengths, rows, file)", "device": "finish: the calls into the library",
          "sort K2": "finish: sort by K2 (device)", "gather": "finish: gather of K1 (device)", "sort K1": "finish: sort by K1 (device)",
          "runs": "finish: gather of K2 + run-length and row launches (device)", "text": "finish: file text",
          "reference": "reference into HBM (before the scan)", "ref read": "reference: file read (host)",
          "ref load": "reference: upload + ref_pack (host clock, returns when packed)"}
NORM_NOTE = ("The scan stage timer of a norm job INCLUDES the reference load (it runs inside that stage, in front of the first batch): without the load's "
             "%.4f s the scan stage is %+.4f s against the on median.  The load's second row is a host clock round upload, `ref_pack` and the wait for it; "
             "`ref_pack`'s device time alone is not in this record.")
NOTES = ("indel store: reserves that asked the device", "indel store: growths", "indel store: capacity (keys)")


def keys_alone(bam, min_mapq, fasta=None):
    """every batch of the file through tdt_indel_push_device with the stream idle around it -> per batch (reads, raw bytes, ms of the launch);
    fasta: with that reference attached (indel_keys<true>)"""
    from tiddit_amd import bamio, tiddit_indels
    rd = bamio.DeviceBamReader(bam)
    h = None
    ref = None
    if fasta is not None:
        from tiddit_amd import refseq
        from tiddit_amd.fasta import FastaFile
        ref = refseq.load_for_bam(FastaFile(fasta), list(rd.references), list(rd.lengths), ctx=rd.ctx)[0]
    rows = []
    try:
        for b in rd.batches():
            if h is None:                                # (room for the largest batch's bound: no reserve asks or grows inside the timing)
                h = tiddit_indels.IndelCounter(len(rd.references), min_mapq, capacity=4 * len(b) + 4096, ctx=rd.ctx)
                h.set_reference(ref)
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
        if ref is not None:
            ref.close()
        rd.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--switch", default="1")
    ap.add_argument("--norm", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    modes = MODES + ("norm",) if a.norm else MODES
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    print("file: %s" % a.bam, file=sys.stderr, flush=True)
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, tiddit_indels
    S, Q = tiddit_indels.parse_switch(a.switch)
    ctx = _native.default_context()
    runs = {m: [] for m in modes}
    notes = []
    table, n_rows = {}, 0
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in modes:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                os.environ.pop("TIDDIT_INDELS", None)
                os.environ.pop("TIDDIT_INDELS_NORM", None)
                if mode != "off":
                    os.environ["TIDDIT_INDELS"] = a.switch
                if mode == "norm":
                    os.environ["TIDDIT_INDELS_NORM"] = "1"
                buf = io.StringIO()
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(buf):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_INDELS", None)
                    os.environ.pop("TIDDIT_INDELS_NORM", None)
                Sx = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
                rec = {"wall": time.perf_counter() - t0}
                rec.update({short: Sx[key] for short, key in KEYS if key in Sx})
                assert os.path.exists(out + ".indels.tab") == (mode != "off")
                if i:
                    runs[mode].append(rec)
                    if mode == "on":
                        notes.append({k: cli.STAGE_NOTES.get(k) for k in NOTES})
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == modes[-1] and i == a.reps:
                    lines = open(out + ".indels.tab").read().split("\n")
                    table = {l.split("\t")[1]: int(l.split("\t")[2]) for l in lines if l.startswith("SN\t")}
                    n_rows = sum(1 for l in lines if l and not l.startswith(("#", "SN\t")))
    alone = keys_alone(a.bam, Q)
    alone_norm = keys_alone(a.bam, Q, a.ref) if a.norm else []

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = ["wall"] + [short for short, _ in KEYS]
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "switch": a.switch, "SN": table, "rows": n_rows,
           "median_s": {m: {k: med(m, k) for k in keys} for m in modes}, "runs": runs, "reserve": notes, "indel_keys_alone": alone,
           "indel_keys_norm_alone": alone_norm}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", ("indels_norm" if a.norm else "indels") + ("_%dmb.md" % a.mb if a.mb else ".md"))
    with open(path, "w") as f:
        f.write("# The small-indel candidates of `tiddit --sv` (`TIDDIT_INDELS=%s`)\n\n" % a.switch)
        f.write("File: `%s` (%.0f MB).  `tools/time_indels.py`: one process, after one warm-up round %d rounds of { `--sv --skip_assembly` switch off, "
                "switch on }, interleaved.  Wall seconds unless a row says device; the yardstick is the off job of the same process; no budget was "
                "fixed in advance, this is what was measured.\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam),
                                                                     os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in modes:
            for key in keys:
                if med(mode, key) is None:
                    continue
                f.write("| %s: %s | %s | %.4f |\n" % (mode, LABELS[key], " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        off = [r["scan"] for r in runs["off"]]
        offw = [r["wall"] for r in runs["off"]]
        f.write("\nScan stage, off runs: spread %.4f s (min %.4f, max %.4f).  Scan stage, on against the off median: %+.4f s.  Whole job, off runs: "
                "spread %.4f s.  Whole job, on against the off median: %+.4f s.\n" % (max(off) - min(off), min(off), max(off), med("on", "scan") - med("off", "scan"),
                                                                                       max(offw) - min(offw), med("on", "wall") - med("off", "wall")))
        f.write("\nThe reserve (room for 4 keys per read before each launch), per on run: " +
                "; ".join("asked the device %s times, grew the store %s times, capacity %s keys" % tuple(n[k] for k in NOTES) for n in notes) + ".\n")
        stored = table.get("insertions", 0) + table.get("deletions", 0)
        f.write("\nThe file: %d records, %d eligible (MAPQ >= %d); %d keys stored (%d insertions, %d deletions) from %d reads, %d unanchored and %d too long "
                "operations, %d noisy reads, %d malformed; %d distinct events, %d reported at a support of %d (%d rows in the file).\n" % (
                    table.get("records", 0), table.get("eligible", 0), Q, stored, table.get("insertions", 0), table.get("deletions", 0),
                    table.get("reads_with_events", 0), table.get("unanchored", 0), table.get("too_long", 0), table.get("noisy_reads", 0),
                    table.get("malformed", 0), table.get("distinct_events", 0), table.get("reported_events", 0), S, n_rows))
        if stored and med("on", "sort K2") is not None:
            dev = sum(med("on", k) for k in ("sort K2", "gather", "sort K1", "runs"))
            f.write("\nFinish on the device: %.3f ms for %d keys.\n" % (dev * 1e3, stored))
        f.write("\n`indel_keys` alone (one batch, the stream idle around it, best of 4, host clock around launch and sync):\n\n"
                "| batch | reads | raw MB | ms | reads per us | raw GB/s |\n|---|---|---|---|---|---|\n")
        for k, r in enumerate(alone):
            f.write("| %d | %d | %.1f | %.3f | %.0f | %.0f |\n" % (k, r["reads"], r["raw_bytes"] / 1e6, r["ms"], r["reads"] / (r["ms"] * 1e3),
                                                                    r["raw_bytes"] / (r["ms"] * 1e-3) / 1e9))
        if a.norm:
            onw, ons = [r["wall"] for r in runs["on"]], [r["scan"] for r in runs["on"]]
            f.write("\n## `TIDDIT_INDELS_NORM=1` against `TIDDIT_INDELS` alone (the same process)\n\nScan stage, norm against the on median: %+.4f s (on runs: "
                    "spread %.4f s).  Whole job: %+.4f s (on runs: spread %.4f s).  The new counters: %s.\n" % (
                        med("norm", "scan") - med("on", "scan"), max(ons) - min(ons), med("norm", "wall") - med("on", "wall"), max(onw) - min(onw),
                        ", ".join("%s %d" % (k, table.get(k, 0)) for k in ("shifted_events", "shift_capped", "off_reference"))))
            f.write("\n" + NORM_NOTE % (med("norm", "reference"), med("norm", "scan") - med("norm", "reference") - med("on", "scan")) + "\n")
            f.write("\nThe synthetic file's deletions are placed at random, so its shifts are short: long repeats, real libraries and the path that "
                    "stops at the cap are NOT measured by this record.\n\n`indel_keys<true>` alone beside `indel_keys<false>` (the table above), the same "
                    "batches, best of 4:\n\n| batch | reads | ms without a reference | ms with the reference |\n|---|---|---|---|\n")
            for k, (r0, r1) in enumerate(zip(alone, alone_norm)):
                f.write("| %d | %d | %.3f | %.3f |\n" % (k, r0["reads"], r0["ms"], r1["ms"]))


if __name__ == "__main__":
    main()
