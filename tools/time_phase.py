"""What the read-backed phasing of `tiddit --sv` (TIDDIT_PHASE) costs the job: `tiddit --sv --skip_assembly` with TIDDIT_ALLELES alone and
with TIDDIT_PHASE=2 beside it, interleaved, in one process, medians of the rounds behind one warm-up round — the whole job's wall, the scan
stage, the allele push timer (which holds `phase_keys` too), the phase stage split into its launch groups (host clock, each group ends in
a synchronisation), the host het flags, the file text, and the observation store's reserve asks and growths.  The yardstick is the
TIDDIT_ALLELES-alone job of the same process, never an absolute number.  `phase_keys` is also timed per batch between device events on
the context's stream: the allele push with and without the store on the same batch, the stream idle around it.  The sites are generated: one
every `--every` bases of every contig, REF = the reference base.  The bench file's reads are cut from the reference in one piece, so it has
almost no hets: the figures are the cost of the stage, not a result.  Writes the record to profiles/phase_<mb>mb.md (or --out) and prints one
JSON line.

usage: python tools/time_phase.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--every 1000] [--profile] [--out FILE.md]
(--mb: bench.py's synthetic file of that genome size; --profile: the per-batch rows also go to stderr as they are measured)"""
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

MODES = ("alleles", "phase")
KEYS = (("scan", "signal extraction + coverage"), ("push", "allele counts (push)"), ("alleles", "allele counts ({o}.alleles.tab)"),
        ("phase", "phase sets ({o}.phase.tab, {o}.phase.blocks.tab)"), ("het", "phase het flags (host)"), ("finish", "phase finish (device)"),
        ("rows", "phase fragment rows"), ("link keys", "phase link keys"), ("link rows", "phase link rows"), ("forest", "phase forest, check, sites"),
        ("text", "phase tables text (host)"))
NOTES = ("phase store: reserves that asked the device", "phase store: growths", "phase store: capacity (keys)", "phase forest: rounds")


def write_sites(path, fasta, every):
    """a site every `every` bases of every contig of the FASTA, REF = its base there (N skipped), ALT = the next base of ACGT -> how many"""
    n = 0
    with open(path, "w") as out:
        out.write("##fileformat=VCFv4.2\n")
        name, seq = None, []

        def flush():
            nonlocal n
            if name is None:
                return
            s = "".join(seq).upper()
            for p in range(every // 2, len(s), every):
                if s[p] in "ACGT":
                    out.write("%s\t%d\t.\t%s\t%s\n" % (name, p + 1, s[p], "ACGT"[("ACGT".index(s[p]) + 1) % 4]))
                    n += 1
        for line in open(fasta):
            if line.startswith(">"):
                flush()
                name, seq = line[1:].split()[0], []
            else:
                seq.append(line.strip())
        flush()
    return n


def keys_alone(bam, vcf, profile):
    """every batch of the file through the allele push without and with the observation store, between two device events on the
    context's stream, best of 4 -> per batch (reads, raw bytes, ms without, ms with)"""
    import torch
    from tiddit_amd import bamio, tiddit_alleles, tiddit_phase
    rd = bamio.DeviceBamReader(bam)
    sites = tiddit_alleles.read_sites(vcf, list(rd.references), list(rd.lengths))
    codes = tiddit_phase.site_codes(sites)
    stream = torch.cuda.ExternalStream(rd.ctx.lib.tdt_ctx_stream(rd.ctx.handle))
    rows, hs = [], None

    def best_of(h, b):
        best = None
        for _ in range(4):                               # (the first one warms up)
            h.reset()
            rd.ctx.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h.push_device_batch(b)
            e1.record(stream)
            rd.ctx.sync()
            dt = e0.elapsed_time(e1)
            best = dt if best is None or dt < best else best
        return best
    try:
        for b in rd.batches():
            if hs is None:                               # (room for the largest batch's bound: no reserve asks or grows inside the timing)
                hs = (tiddit_alleles.AlleleCounter(sites.site_pos, sites.site_off, 5, 13, ctx=rd.ctx),
                      tiddit_alleles.AlleleCounter(sites.site_pos, sites.site_off, 5, 13, ctx=rd.ctx, phase=(codes, 8 * len(b) + 4096, 64)))
            rd.ctx.sync()
            row = {"reads": len(b), "raw_bytes": int(b._raw_len), "without_ms": best_of(hs[0], b), "with_ms": best_of(hs[1], b)}
            rows.append(row)
            if profile:
                print("batch %d: %r" % (len(rows) - 1, row), file=sys.stderr, flush=True)
    finally:
        for h in hs or ():
            h.close()
        rd.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--every", type=int, default=1000)
    ap.add_argument("--profile", action="store_true")
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
    sn, notes = {}, []
    with tempfile.TemporaryDirectory() as d:
        vcf = os.path.join(d, "sites.vcf")
        n_sites = write_sites(vcf, a.ref, a.every)
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in MODES:
                out = os.path.join(d, "r%d_%s" % (i, mode))
                os.environ["TIDDIT_ALLELES"] = vcf
                os.environ.pop("TIDDIT_PHASE", None)
                if mode == "phase":
                    os.environ["TIDDIT_PHASE"] = "2"
                buf = io.StringIO()
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(buf):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_ALLELES", None)
                    os.environ.pop("TIDDIT_PHASE", None)
                Sx = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
                rec = {"wall": time.perf_counter() - t0}
                rec.update({short: Sx[key] for short, key in KEYS if key in Sx})
                assert os.path.exists(out + ".phase.tab") == (mode == "phase")
                if i:
                    runs[mode].append(rec)
                    if mode == "phase":
                        notes.append({k: cli.STAGE_NOTES.get(k) for k in NOTES})
                print("round %d %s: %.3f s" % (i, mode, rec["wall"]), file=sys.stderr, flush=True)
                if mode == "phase" and i == a.reps:
                    lines = open(out + ".phase.tab").read().split("\n")
                    sn = {l.split("\t")[1]: int(l.split("\t")[2]) for l in lines if l.startswith("SN\t")}
        alone = keys_alone(a.bam, vcf, a.profile)

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = ["wall"] + [short for short, _ in KEYS]
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "sites": n_sites, "SN": sn,
           "median_s": {m: {k: med(m, k) for k in keys} for m in MODES}, "runs": runs, "reserve": notes, "keys_alone": alone}
    print(json.dumps(res))
    path = a.out or os.path.join(REPO, "profiles", "phase" + ("_%dmb.md" % a.mb if a.mb else ".md"))
    off = [r["scan"] for r in runs["alleles"]]
    diff = med("phase", "scan") - med("alleles", "scan")
    spread = max(off) - min(off)
    with open(path, "w") as f:
        f.write("# Read-backed phasing of `tiddit --sv` (`TIDDIT_PHASE=2` beside `TIDDIT_ALLELES`)\n\n")
        f.write("File: `%s` (%.0f MB), %d generated sites (one per %d bases, REF = the reference base).  `tools/time_phase.py`: one process, after one "
                "warm-up round %d rounds of { `--sv --skip_assembly` with `TIDDIT_ALLELES` alone, with `TIDDIT_PHASE=2` beside it }, interleaved.  Wall "
                "seconds; the yardstick is the `TIDDIT_ALLELES`-alone job of the same process; no time was fixed in advance, this is what was measured.  "
                "The file's reads are cut from the reference in one piece, so it has almost no hets: these figures are the COST of the stage, not a "
                "result.\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, n_sites, a.every, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode in MODES:
            for key in keys:
                if med(mode, key) is not None:
                    f.write("| %s: %s | %s | %.4f |\n" % (mode, key, " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        f.write("\nScan stage, `TIDDIT_ALLELES`-alone runs: spread %.4f s (min %.4f, max %.4f).  With `TIDDIT_PHASE`: %+.4f s against their median: %s.\n" % (
            spread, min(off), max(off), diff, "inside that spread" if abs(diff) <= spread else "NOT inside that spread"))
        f.write("\nThe observation store's reserve (room for 8 keys per read is asked before each launch; a reserve that does not fit asks the device "
                "for the real count, which synchronises the stream, and grows the store 1.5 x when that does not help either), per run: %s.\n" % "; ".join(
                    "asked the device %s times, grew the store %s times, capacity %s keys, %s forest rounds" % tuple(n[k] for k in NOTES) for n in notes))
        f.write("\nThe file as the phased job saw it: %s.\n" % ", ".join("%s %d" % kv for kv in sn.items()))
        f.write("\nThe allele push of one batch between two device events on the context's stream (the stream idle around it, best of 4): `al_count` alone, "
                "and `al_count` + `phase_keys` on a handle with the store (room for the batch's bound reserved before):\n\n"
                "| batch | reads | raw MB | al_count ms | al_count + phase_keys ms | difference ms |\n|---|---|---|---|---|---|\n")
        for k, r in enumerate(alone):
            f.write("| %d | %d | %.1f | %.3f | %.3f | %.3f |\n" % (k, r["reads"], r["raw_bytes"] / 1e6, r["without_ms"], r["with_ms"], r["with_ms"] - r["without_ms"]))
        f.write("\nNot measured: real libraries (their hets, their insert sizes), dense sites (dbSNP-scale catalogues), long reads (more than 8 "
                "observations per read are capped), a job with more than one GPU (refused); the host latency of the graph stage at a real het density (every round "
                "and every pointer-jumping launch ends in a synchronisation and an 8-byte copy: here the forest has next to nothing to join); the host text of "
                "the two tables at millions of het sites (one formatted line per het site, as the other tables of the job are written).\n")


if __name__ == "__main__":
    main()
