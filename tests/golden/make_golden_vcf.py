#!/usr/bin/env python3
"""Generate tests/golden/sv_vcf*.json — the VCF of `tiddit --sv --skip_assembly` — from the REAL reference.

Runs only in the build container (needs /root/reference, Cython and joblib).  For each of sv_e2e_small.json, sv_e2e.json and
sv_e2e_grch38.json the synthetic BAM + FASTA are regenerated from the fixture's seeds and taken through the chain of
make_golden.golden_sv_e2e (statistics, signal restatement, compiled GC / ploidy / clustering); the candidates must hash to the
committed ``candidates_sha256``.  Then tiddit_variant.pyx, compiled as it stands in a scratch dir under /tmp, runs its main() on
them, and the reference's tiddit_vcf_header.main() makes the header.

tiddit_variant.pyx cimports pysam.libcalignmentfile; a stub package built there with Cython serves the decoded records
(oracle.bam_walk) through ``AlignmentFile.fetch(chr, start, end)`` and ``AlignedSegment`` properties.  Its fetch restates htslib's
overlap rule — a record is returned when ``pos < end`` and ``endpos > start``, where a record that aligns no base ends at
``pos + 1`` — and that rule is the only piece of these fixtures not pinned by compiled reference code.

Each fixture holds the VCF — the header without its ##TIDDITcmd line as a checksum plus its lines other than ##contig, and the
records one per line — and, for tests/test_variant_cpu.py, what define_variant reads of every candidate it does not drop at its
first test (with the three coverage means), and every get_region call with its result.  The library dict keeps its global
entries and those of the contigs that carry candidates.  Only data is written here; nothing of the reference is copied.

usage: python tests/golden/make_golden_vcf.py [--only sv_e2e_small.json]
"""
import hashlib
import importlib
import json
import os
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
import make_golden  # noqa: E402
from make_golden import REF, _jsonable, build_reference, stat_reads  # noqa: E402

VBUILD = "/tmp/tiddit_ref_vcf_build"
VERSION = "3.9.5"          # what tiddit_amd.__main__ reports

_PXD = """
cdef class AlignedSegment:
    cdef public object is_unmapped, mate_is_unmapped, is_duplicate, reference_start, reference_end, next_reference_start
    cdef public object mapq, reference_name, next_reference_name, isize, _sa

cdef class AlignmentFile:
    cdef public object header
    cdef object _data
"""

_PYX = """
import numpy as np
DATA = {}      # bam path -> {"header": ..., "names": [...], per-contig column dict under "contigs"}

cdef class AlignedSegment:
    def has_tag(self, tag):
        return tag == "SA" and self._sa

cdef class AlignmentFile:
    def __init__(self, path, mode="r", reference_filename=None, index_filename=None):
        self._data = DATA[path]
        self.header = self._data["header"]

    def fetch(self, chrom, start, end):
        # htslib's overlap rule: pos < end and endpos > start (a record aligning no base ends at pos + 1)
        d = self._data
        c = d["contigs"].get(d["tid"][chrom])
        if c is None:
            return
        lo = int(np.searchsorted(c["pos_np"], start - c["span"], "left"))
        hi = int(np.searchsorted(c["pos_np"], end, "left"))
        names = d["names"]
        cdef AlignedSegment r
        for i in range(lo, hi):
            if not c["end"][i] > start:
                continue
            f = c["flag"][i]
            r = AlignedSegment()
            r.is_unmapped, r.mate_is_unmapped, r.is_duplicate = bool(f & 0x4), bool(f & 0x8), bool(f & 0x400)
            r.reference_start, r.next_reference_start, r.mapq, r.isize = c["pos"][i], c["mate_pos"][i], c["mapq"][i], c["tlen"][i]
            r.reference_end = None if f & 0x4 else c["end"][i]
            r.reference_name = names[c["tid"]]
            r.next_reference_name = names[c["mate_tid"][i]] if c["mate_tid"][i] >= 0 else None
            r._sa = bool(c["has_sa"][i])
            yield r

    def close(self):
        pass
"""


def build_variant():
    """tiddit_variant.pyx against the stub pysam.libcalignmentfile, both compiled under VBUILD -> the module"""
    pkg = os.path.join(VBUILD, "pysam")
    os.makedirs(pkg, exist_ok=True)
    for name, text in (("__init__.py", ""), ("__init__.pxd", ""), ("libcalignmentfile.pxd", _PXD), ("libcalignmentfile.pyx", _PYX)):
        p = os.path.join(pkg, name)
        if not os.path.exists(p) or open(p).read() != text:
            open(p, "w").write(text)
    inc = sysconfig.get_paths()["include"]
    ext = sysconfig.get_config_var("EXT_SUFFIX")

    def compile_(pyx, c, so):
        if os.path.exists(so) and os.path.getmtime(so) > os.path.getmtime(pyx):
            return
        subprocess.check_call(["cython", "-3", "-I", VBUILD, pyx, "-o", c])
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-w", "-I", inc, "-I", np.get_include(), c, "-o", so])
    compile_(os.path.join(pkg, "libcalignmentfile.pyx"), os.path.join(pkg, "libcalignmentfile.c"), os.path.join(pkg, "libcalignmentfile" + ext))
    compile_(os.path.join(REF, "tiddit_variant.pyx"), os.path.join(VBUILD, "tiddit_variant.c"), os.path.join(VBUILD, "tiddit_variant" + ext))
    # make_golden's pysam stand-in is a plain module: give it the stub package's path so that pysam.libcalignmentfile resolves
    pysam = sys.modules["pysam"]
    pysam.__path__ = [pkg]
    stub = importlib.import_module("pysam.libcalignmentfile")
    sys.path.insert(0, VBUILD)
    return importlib.import_module("tiddit_variant"), stub


def serve(stub, bam, sq, fields):
    names = [c["SN"] for c in sq]
    tid = fields["tid"]
    contigs = {}
    for t in np.unique(tid[tid >= 0]):
        m = tid == t
        c = {k: fields[k][m] for k in ("pos", "end", "flag", "mapq", "mate_pos", "mate_tid", "tlen", "has_sa")}
        c = {k: v.tolist() for k, v in c.items()}
        c["span"] = int((fields["end"][m].astype(np.int64) - fields["pos"][m]).max())
        c["tid"] = int(t)
        c["pos_np"] = np.asarray(c["pos"], dtype=np.int64)
        contigs[int(t)] = c
    stub.DATA[bam] = {"header": {"SQ": sq}, "names": names, "tid": {n: i for i, n in enumerate(names)}, "contigs": contigs}


def means_of(cand, cov, gc, lib):
    """the three coverage means define_variant forms per candidate (numpy.average, as the reference calls it)"""
    import math
    import warnings
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for a in cand:
            out[a] = {}
            for b in cand[a]:
                out[a][b] = {}
                for cid, c in cand[a][b].items():
                    posA, posB = c["posA"], c["posB"]
                    if a == b and posA > posB:
                        posA, posB = posB, posA
                    avg_a = np.average(cov[a][int(math.floor(c["startA"] / 50.0)):int(math.floor(c["endA"] / 50.0)) + 1])
                    avg_b = np.average(cov[b][int(math.floor(c["startB"] / 50.0)):int(math.floor(c["endB"] / 50.0)) + 1])
                    if a != b:
                        covM = 0
                    elif abs(posB - posA) < 1000:
                        covM = None
                    else:
                        s, e = int(math.floor(posA / 50.0)), int(math.floor(posB / 50.0)) + 1
                        between = cov[a][s:e][gc[a][s:e] > -1]
                        covM = float(np.average(between)) if len(between) > 4 else lib["avg_coverage_{}".format(a)]
                    out[a][b][str(cid)] = {"avg_a": float(avg_a), "avg_b": float(avg_b), "covM": covM}
    return out


# what define_variant reads of a candidate, one row each; the sample sets enter only through their sizes, and N_contigs is 0 with
# --skip_assembly (no contig names)
CANDIDATE_COLUMNS = ["chrA", "chrB", "cluster", "posA", "posB", "startA", "endA", "startB", "endB", "N_discordants", "N_splits", "N_contigs",
                     "orientation_discordants_A", "orientation_discordants_B", "orientation_splits_A", "orientation_splits_B",
                     "orientation_contigs_A", "orientation_contigs_B", "n_sample_splits", "n_sample_discordants", "avg_a", "avg_b", "covM"]


def candidate_rows(cand, means, args, sample="WGS"):
    """the candidates define_variant does not drop at its first test, in the reference's order, with their means"""
    rows = []
    for a in cand:
        for b in cand[a]:
            for cid, c in cand[a][b].items():
                if (c["N_discordants"] < args.p and c["N_splits"] < args.r) and not c["N_contigs"]:
                    continue
                assert not c["N_contigs"]
                m = means[a][b][str(cid)]
                pa, pb = c["positions_A"], c["positions_B"]
                rows.append(_jsonable([a, b, str(cid), c["posA"], c["posB"], c["startA"], c["endA"], c["startB"], c["endB"], c["N_discordants"],
                                       c["N_splits"], c["N_contigs"], pa["orientation_discordants"], pb["orientation_discordants"],
                                       pa["orientation_splits"], pb["orientation_splits"], pa["orientation_contigs"], pb["orientation_contigs"],
                                       len(c["sample_splits"][sample]), len(c["sample_discordants"][sample]), m["avg_a"], m["avg_b"], m["covM"]]))
    return rows


def write_rows(res, path):
    """one JSON document: one line per key, and one per element of the four lists (a readable diff; json.load reads it back)"""
    c = (",", ":")
    parts = []
    for k, v in res.items():
        if k in ("vcf_header_other_lines", "vcf_records", "candidates", "get_region_calls"):
            parts.append(json.dumps(k) + ":[\n" + ",\n".join(json.dumps(r, separators=c) for r in v) + "\n]")
        else:
            parts.append(json.dumps(k) + ":" + json.dumps(v, separators=c))
    open(path, "w").write("{\n" + ",\n".join(parts) + "\n}\n")


def golden_vcf(M, V, stub, fixture_name, out_name):
    import oracle
    from oracle import cluster_oracle, signal_oracle
    from tiddit_amd import synth_bam
    from tiddit_amd.__main__ import _sv_parser
    fx = json.load(open(os.path.join(HERE, fixture_name)))
    P = fx["params"]
    contigs = synth_bam.contigs_for(P)
    with tempfile.TemporaryDirectory() as td:
        fa, bam, prefix = os.path.join(td, "ref.fa"), os.path.join(td, "WGS.bam"), os.path.join(td, "out")
        seqs = synth_bam.write_fasta(fa, contigs, seed=P["fasta_seed"])
        info = synth_bam.write_wgs_sv_bam(bam, contigs, depth=P["depth"], read_len=P["read_len"], insert=P["insert"], insert_sd=P["insert_sd"],
                                          seed=P["seed"], sv_per_mb=P["sv_per_mb"], threads=8, ref_seqs=seqs)
        assert info["n_records"] == fx["n_records"]
        header, sq, raw = signal_oracle.inflate_bam(bam)
        fields = oracle.bam_walk(raw)
        names = [c["SN"] for c in sq]
        M["pysam"].READS = stat_reads(fields, names)
        library = M["tiddit_stats"].statistics(bam, fa, P["min_q"], 100000, P["n_reads_stats"])
        max_ins = library["percentile_insert_size"]
        cov, disc, split, clips, clip_each, n_rec = signal_oracle.signal_main_file(bam, P["min_q"], max_ins, "WGS", P["min_contig"],
                                                                                   P["min_anchor_len"], P["min_clip_len"])
        os.makedirs(prefix + "_tiddit")
        open(prefix + "_tiddit/discordants_WGS.tab", "w").write(disc)
        open(prefix + "_tiddit/splits_WGS.tab", "w").write(split)
        M["pysam"].SEQS = {n: seqs[n].tobytes().decode() for n, _ in contigs}
        gc = {n: M["tiddit_gc"].binned_gc(fa, n, 50, 0.5)[1] for n, _ in contigs}
        lib = M["tiddit_coverage_analysis"].determine_ploidy(cov, names, dict(library), P["ploidy"], prefix, None, fa, 50, header, gc)
        eps = int(library["avg_insert_size"] / 2.0) or 50
        contig_length = {c["SN"]: c["LN"] for c in sq}
        cand = M["tiddit_cluster"].main(prefix, names, contig_length, ["WGS"], library["mp"], eps, P["m"], max_ins, P["min_contig"], True, P["min_reads"])
        assert hashlib.sha256(cluster_oracle.canonical(cand).encode()).hexdigest() == fx["candidates_sha256"], "candidates differ from " + fixture_name
        used = set(a for a in cand for b in cand[a] if cand[a][b]) | set(b for a in cand for b in cand[a] if cand[a][b])
        lib_json = {k: v for k, v in _jsonable(dict(lib)).items()
                    if not k.startswith(("avg_coverage_", "contig_ploidy_")) or k.split("_", 2)[2] in used}
        # the variant stage of the reference, every get_region call recorded
        serve(stub, bam, sq, fields)
        calls = []
        real = V.get_region

        def get_region(samfile, chrom, start, end, bp, min_q, max_ins_, contig_number):
            r = real(samfile, chrom, start, end, bp, min_q, max_ins_, contig_number)
            calls.append([chrom, start, end, bp, min_q, max_ins_, list(r)])
            return r
        V.get_region = get_region
        args = _sv_parser().parse_args(["--sv", "--bam", bam, "--ref", fa, "-o", prefix, "--skip_assembly", "-s", str(P["n_reads_stats"])])
        contig_number = {n: i for i, n in enumerate(names)}
        rows = candidate_rows(cand, means_of(cand, cov, gc, lib), args)          # (before the variant stage, which reads them only)
        variants = V.main(bam, cand, args, lib, P["min_q"], ["WGS"], cov, contig_number, max_ins, gc)
        V.get_region = real
        sample_id = "WGS"
        vcf_header = importlib.import_module("tiddit.tiddit_vcf_header").main(header, lib, sample_id, VERSION)
        body = []
        for chrom in names:
            if chrom not in variants:
                continue
            for variant in sorted(variants[chrom], key=lambda x: x[0]):
                body.append("\t".join(variant[1]) + "\n")
        body = "".join(body)
    head = [l for l in vcf_header.split("\n") if not l.startswith("##TIDDITcmd=")]
    args_json = {k: v for k, v in vars(args).items() if k not in ("bam", "ref", "o")}
    meta = {"source_fixture": fixture_name, "params": P, "version": VERSION, "sample_id": sample_id, "max_ins_len": max_ins,
            "min_mapq": P["min_q"], "args": args_json, "library": lib_json, "n_records": body.count("\n"),
            "fetch_rule": "pos < end and endpos > start; a record aligning no base ends at pos + 1 (htslib's overlap rule, restated by the stub)",
            "candidate_columns": CANDIDATE_COLUMNS, "get_region_columns": ["chrom", "start", "end", "bp", "min_q", "max_ins", "result"]}
    res = {"meta": meta,
           # the header without its ##TIDDITcmd line: its checksum, and every line but the ##contig ones (those follow from the params)
           "vcf_header_sha256": hashlib.sha256("\n".join(head).encode()).hexdigest(),
           "vcf_header_other_lines": [l for l in head if not l.startswith("##contig=")],
           "vcf_body_sha256": hashlib.sha256(body.encode()).hexdigest(), "vcf_records": body.splitlines(),
           "candidates": rows, "get_region_calls": calls}
    write_rows(res, os.path.join(HERE, out_name))
    print(out_name, ":", meta["n_records"], "VCF records,", len(calls), "get_region calls,", len(rows), "candidates kept")
    return res


FIXTURES = (("sv_e2e_small.json", "sv_vcf_small.json"), ("sv_e2e.json", "sv_vcf.json"), ("sv_e2e_grch38.json", "sv_vcf_grch38.json"))


def main():
    M = build_reference()
    V, stub = build_variant()
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    for src, dst in FIXTURES:
        if only is None or only in (src, dst):
            golden_vcf(M, V, stub, src, dst)


if __name__ == "__main__":
    main()
