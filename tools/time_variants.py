"""Wall of `tiddit --sv --skip_assembly` with and without the native variant stage (TIDDIT_VARIANTS=1), in one process, runs
interleaved: the variant stage's own seconds (and its parts), the scan's time in the evidence store's pack launches, and the
scan stage with the switch on against off.  One JSON line.

--ranks N [--backend gloo|nccl]: the same job with the switch on as N ranks (fresh processes per run; gloo: the ranks share GPU 0;
nccl: N = 1 with TIDDIT_FORCE_DIST=1, every collective over RCCL).  Every rank reports its stage seconds, its scan's pack time and
its store size.

usage: python tools/time_variants.py --bam WGS.bam --ref ref.fa [--reps 3] [--ranks N --backend gloo|nccl]
(bench.py leaves its 240-Mb file at $TIDDIT_BENCH_TMP/tiddit_bench_sv_240/)"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _rank(rank, world, port, backend, argv, q):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      TIDDIT_VARIANTS="1")
    if backend == "gloo":
        os.environ.update(TIDDIT_DIST_BACKEND="gloo", TIDDIT_HIP_DEVICE="0")
    else:
        os.environ.pop("TIDDIT_DIST_BACKEND", None)
        os.environ["TIDDIT_FORCE_DIST"] = "1"
    try:
        from tiddit_amd import __main__ as cli
        from tiddit_amd import tiddit_region, tiddit_signal
        sizes = []
        real = tiddit_region.EvidenceStore.close

        def close(self):
            if getattr(self, "handle", None):
                sizes.append(self.n)
            real(self)
        tiddit_region.EvidenceStore.close = close
        cli.main(argv)
        rec = dict(cli.STAGE_SECONDS)
        rec["scan: evidence store (pack)"] = tiddit_signal.SCAN_SECONDS.get("evidence store (pack)")
        rec["store records"] = sizes[0] if sizes else None
        q.put((rank, rec))
    except BaseException:
        import traceback
        q.put((rank, traceback.format_exc()))


def ranks(a):
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    runs = []
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first run warms up the file cache)
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            q = ctx.Queue()
            argv = ["--sv", "--bam", a.bam, "--ref", a.ref, "-o", os.path.join(d, "r%d" % i), "--skip_assembly", "--force_overwrite"]
            procs = [ctx.Process(target=_rank, args=(r, a.ranks, port, a.backend, argv, q)) for r in range(a.ranks)]
            for p in procs:
                p.start()
            res = dict(q.get(timeout=1200) for _ in procs)
            for p in procs:
                p.join(120)
            bad = {r: v for r, v in res.items() if not isinstance(v, dict)}
            if bad:
                raise RuntimeError(json.dumps(bad))
            if i:
                runs.append([res[r] for r in range(a.ranks)])
        n_vcf = sum(1 for l in open(os.path.join(d, "r1.vcf")) if not l.startswith("#"))
    keys = sorted(set(k for run in runs for rec in run for k in rec))
    med = {r: {k: statistics.median([run[r][k] for run in runs if run[r].get(k) is not None]) for k in keys
               if any(run[r].get(k) is not None for run in runs)} for r in range(a.ranks)}
    print(json.dumps({"bam": a.bam, "reps": a.reps, "ranks": a.ranks, "backend": a.backend, "vcf_records": n_vcf, "median_s_per_rank": med,
                      "runs": runs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam", required=True)
    ap.add_argument("--ref", required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ranks", type=int, default=0)
    ap.add_argument("--backend", choices=("gloo", "nccl"), default="gloo")
    a = ap.parse_args()
    if a.ranks:
        return ranks(a)
    from tiddit_amd import __main__ as cli
    from tiddit_amd import tiddit_signal
    runs = {"off": [], "on": []}
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first pair warms up)
            for mode in ("off", "on"):
                if mode == "on":
                    os.environ["TIDDIT_VARIANTS"] = "1"
                else:
                    os.environ.pop("TIDDIT_VARIANTS", None)
                cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", os.path.join(d, "r%d%s" % (i, mode)), "--skip_assembly", "--force_overwrite"])
                rec = dict(cli.STAGE_SECONDS)
                rec["scan: evidence store (pack)"] = tiddit_signal.SCAN_SECONDS.get("evidence store (pack)")
                if i:
                    runs[mode].append(rec)
        os.environ.pop("TIDDIT_VARIANTS", None)
        n_vcf = sum(1 for l in open(os.path.join(d, "r1on.vcf")) if not l.startswith("#"))

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = sorted(set(k for r in runs["on"] for k in r))
    out = {"bam": a.bam, "reps": a.reps, "vcf_records": n_vcf,
           "scan_s_off": med("off", "signal extraction + coverage"), "scan_s_on": med("on", "signal extraction + coverage"),
           "on_median_s": {k: med("on", k) for k in keys}, "runs": runs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
