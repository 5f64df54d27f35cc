"""What the clipped-read breakpoint sites of `tiddit --sv` (TIDDIT_CLIPS) cost the job: `tiddit --sv --skip_assembly` with the switch off
and on, interleaved, in one process — the whole job's wall and the scan stage off and on (with the spread of the off runs beside every
figure), the new stage timer (the pushes' host side: it also holds the waits of a reserve that has to ask the device), the finish stage
split into its two sorts, the gather, the run-length launches and the site launches (heads, vote, rows; HIP events round them inside
tdt_clip_finish), the keys stored and how often the reserve asked the device or grew the store.  The yardstick is the same job without
the switch in the same process, never an absolute number.  `clip_keys` is also timed alone (host clock around launch and sync, the
stream idle, best of 4) on every batch of the file.  Writes the record to profiles/clips_<mb>mb.md (or --out) and prints one JSON line.

usage: python tools/time_clips.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--switch 1] [--out FILE.md]
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


def keys_alone(bam, min_mapq, min_clip):
    """every batch of the file through tdt_clip_push_device with the stream idle around it -> per batch (reads, raw bytes, ms of the launch)"""
    from tiddit_amd import bamio, tiddit_clips
    rd = bamio.DeviceBamReader(bam)
    h = None
    rows = []
    try:
        for b in rd.batches():
            if h is None:                                # (room for the largest batch's bound: no reserve asks or grows inside the timing)
                h = tiddit_clips.ClipCounter(len(rd.references), min_mapq, min_clip, capacity=2 * len(b) + 4096, ctx=rd.ctx)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--switch", default="1")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    print("file: %s" % a.bam, file=sys.stderr, flush=True)
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
