"""What the tandem-repeat genotypes of `tiddit --sv` (TIDDIT_STR) cost the job: `tiddit --sv --skip_assembly` with the switch off and on,
interleaved, in one process — on at two generated catalogues, a locus per 3 kb (`sparse`) and a locus per 300 bp (`dense`) of every
contig — the whole job's wall, the scan stage, the new stage timer (the pushes' host side: it also holds the waits of a reserve that has
to ask the device) and the finish stage beside them, the finish split into its two sorts, the gather and the run-length launches (HIP
events round them inside tdt_str_finish).  The yardstick is the same job without the switch in the same process, never an absolute
number.  The key kernel is also timed alone (host clock around launch and sync, the stream idle) on every batch of the file at both
catalogues, with `indel_keys` on the same batches beside it.  The generated loci are 12 bases of a motif the file's reads do not carry
as planted repeats: the figures are the cost only.  Writes the record to profiles/str_<mb>mb.md (or --out) and prints one JSON line.

usage: python tools/time_str.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--cuts 5:5:20] [--out FILE.md]
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

MODES = ("off", "sparse", "dense")
STEP = {"sparse": 3000, "dense": 300}
KEYS = (("scan", "signal extraction + coverage"), ("push", "str keys (push)"), ("ingest wait", "ingest (inflate + decode, device)"),
        ("finish", "tandem repeats ({o}.str.tab)"), ("device", "str sets (device: two sorts, gather, run lengths, rows)"),
        ("sort K2", "sort by K2 (device time)"), ("gather", "gather of K1 (device time)"), ("sort K1", "sort by K1 (device time)"),
        ("runs", "run lengths + rows (device time)"), ("text", "str genotype rule + table text (host)"))
LABELS = {"wall": "whole job", "scan": "scan stage", "push": "new stage timer (pushes, host side, reserve waits included)",
          "ingest wait": "scan: waited for the ingest", "finish": "finish stage (sort, run lengths, rows, rule, file)",
          "device": "finish: the calls into the library", "sort K2": "finish: sort by K2 (device)", "gather": "finish: gather of K1 (device)",
          "sort K1": "finish: sort by K1 (device)", "runs": "finish: gather of K2 + run-length and row launches (device)",
          "text": "finish: genotype rule + file text"}
NOTES = ("str store: reserves that asked the device", "str store: growths", "str store: capacity (keys)")


def write_loci(path, names, lengths, step):
    """a locus of 12 bases (CAG) every `step` bases of every contig -> how many"""
    n = 0
    with open(path, "w") as f:
        for name, ln in zip(names, lengths):
            for s in range(step // 2, ln - 20, step):
                f.write("%s\t%d\t%d\tCAG\n" % (name, s, s + 12))
                n += 1
    return n


def keys_alone(bam, beds, cuts):
    """every batch of the file through tdt_str_push_device (per catalogue) and tdt_indel_push_device with the stream idle around it ->
    per batch (reads, raw bytes, ms per catalogue, ms of indel_keys)"""
    from tiddit_amd import bamio, tiddit_indels, tiddit_str
    rd = bamio.DeviceBamReader(bam)
    hs, hi = None, None
    rows = []

    def best_of(h, b):
        best = None
        for _ in range(4):                               # (the first one warms up)
            h.reset()
            rd.ctx.sync()
            t0 = time.perf_counter()
            h.push_device_batch(b)
            rd.ctx.sync()
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        return best * 1e3
    try:
        for b in rd.batches():
            if hs is None:                               # (room for the largest batch's bound: no reserve asks or grows inside the timing)
                loci = {m: tiddit_str.read_loci(p, list(rd.references), list(rd.lengths)) for m, p in beds.items()}
                hs = {m: tiddit_str.StrCounter(loci[m], cuts[0], cuts[2], capacity=4 * len(b) + 4096, ctx=rd.ctx) for m in beds}
                hi = tiddit_indels.IndelCounter(len(rd.references), cuts[2], capacity=4 * len(b) + 4096, ctx=rd.ctx)
            rd.ctx.sync()
            row = {"reads": len(b), "raw_bytes": int(b._raw_len), "indel_ms": best_of(hi, b)}
            for m in beds:
                row[m + "_ms"] = best_of(hs[m], b)
                row[m + "_in_reach"] = int(hs[m].finish()[2])
            rows.append(row)
    finally:
        for h in list((hs or {}).values()) + [hi]:
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
    ap.add_argument("--cuts", default="5:5:20")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    print("file: %s" % a.bam, file=sys.stderr, flush=True)
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, bamio, tiddit_str
    cuts = tiddit_str.parse_cuts(a.cuts)
    ctx = _native.default_context()
    runs = {m: [] for m in MODES}
    notes = {m: [] for m in MODES}
    tables, n_loci = {}, {}
    with tempfile.TemporaryDirectory() as d:
        rd = bamio.BamReader(a.bam, batch_bytes=1 << 20)
        names, lengths = list(rd.references), list(rd.lengths)
        rd.close()
        beds = {m: os.path.join(d, m + ".bed") for m in STEP}
        for m, p in beds.items():
            n_loci[m] = write_loci(p, names, lengths, STEP[m])
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                os.environ.pop("TIDDIT_STR", None)
                os.environ.pop("TIDDIT_STR_CUTS", None)
                if mode != "off":
                    os.environ["TIDDIT_STR"] = beds[mode]
                    os.environ["TIDDIT_STR_CUTS"] = a.cuts
                buf = io.StringIO()
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(buf):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_STR", None)
                    os.environ.pop("TIDDIT_STR_CUTS", None)
                Sx = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
                rec = {"wall": time.perf_counter() - t0}
                rec.update({short: Sx[key] for short, key in KEYS if key in Sx})
                rec["loci read"] = next((v for k, v in Sx.items() if k.startswith("str loci (")), None)
                assert os.path.exists(out + ".str.tab") == (mode != "off")
                if i:
                    runs[mode].append(rec)
                    if mode != "off":
                        notes[mode].append({k: cli.STAGE_NOTES.get(k) for k in NOTES})
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode != "off" and i == a.reps:
                    lines = open(out + ".str.tab").read().split("\n")
                    tables[mode] = {l.split("\t")[1]: int(l.split("\t")[2]) for l in lines if l.startswith("SN\t")}
        alone = keys_alone(a.bam, beds, cuts)

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = ["wall"] + [short for short, _ in KEYS] + ["loci read"]
    LABELS["loci read"] = "loci file read (host, before the scan)"
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "cuts": a.cuts, "loci": n_loci, "SN": tables,
           "median_s": {m: {k: med(m, k) for k in keys} for m in MODES}, "runs": runs, "reserve": notes, "keys_alone": alone}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "str" + ("_%dmb.md" % a.mb if a.mb else ".md"))
    with open(path, "w") as f:
        f.write("# The tandem-repeat genotypes of `tiddit --sv` (`TIDDIT_STR`, `TIDDIT_STR_CUTS=%s`)\n\n" % a.cuts)
        f.write("File: `%s` (%.0f MB).  `tools/time_str.py`: one process, after one warm-up round %d rounds of { `--sv --skip_assembly` switch off, "
                "on with a generated locus per 3 kb (`sparse`, %d loci), on with one per 300 bp (`dense`, %d loci) }, interleaved.  Wall seconds unless a "
                "row says device; the yardstick is the off job of the same process; no budget was fixed in advance, this is what was measured.  The "
                "file's reads carry no planted repeats: these figures are the cost only.\n\n" % (
                    os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, a.reps, n_loci["sparse"],
                    n_loci["dense"]))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in MODES:
            for key in keys:
                if med(mode, key) is None:
                    continue
                f.write("| %s: %s | %s | %.4f |\n" % (mode, LABELS[key], " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        off = [r["scan"] for r in runs["off"]]
        offw = [r["wall"] for r in runs["off"]]
        f.write("\nScan stage, off runs: spread %.4f s (min %.4f, max %.4f).  Whole job, off runs: spread %.4f s.\n" % (
            max(off) - min(off), min(off), max(off), max(offw) - min(offw)))
        for m in STEP:
            f.write("\n`%s`: scan stage against the off median %+.4f s, whole job %+.4f s.  The reserve (room for 4 keys per read before each launch), "
                    "per run: %s.\n" % (m, med(m, "scan") - med("off", "scan"), med(m, "wall") - med("off", "wall"),
                                        "; ".join("asked the device %s times, grew the store %s times, capacity %s keys" % tuple(n[k] for k in NOTES)
                                                  for n in notes[m])))
            t = tables.get(m, {})
            f.write("The file at `%s`: %d records, %d eligible (MAPQ >= %d), %d with a locus in reach; %d spanning, %d left and %d right keys, %d "
                    "unanchored, %d over the cap of four, %d malformed.\n" % (m, t.get("records", 0), t.get("eligible", 0), cuts[2], t.get("in_reach", 0),
                                                                             t.get("span_keys", 0), t.get("left_keys", 0), t.get("right_keys", 0),
                                                                             t.get("unanchored", 0), t.get("over_cap", 0), t.get("malformed", 0)))
            if med(m, "sort K2") is not None:
                f.write("Finish on the device: %.3f ms.\n" % (sum(med(m, k) for k in ("sort K2", "gather", "sort K1", "runs")) * 1e3))
        f.write("\n`str_keys` alone beside `indel_keys` on the same batches (one batch, the stream idle around it, best of 4, host clock around launch "
                "and sync):\n\n| batch | reads | raw MB | indel_keys ms | str_keys sparse ms | reads in reach | str_keys dense ms | reads in reach |\n"
                "|---|---|---|---|---|---|---|---|\n")
        for k, r in enumerate(alone):
            f.write("| %d | %d | %.1f | %.3f | %.3f | %d | %.3f | %d |\n" % (k, r["reads"], r["raw_bytes"] / 1e6, r["indel_ms"], r["sparse_ms"],
                                                                             r["sparse_in_reach"], r["dense_ms"], r["dense_in_reach"]))


if __name__ == "__main__":
    main()
