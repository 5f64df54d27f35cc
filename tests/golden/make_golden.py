#!/usr/bin/env python3
"""Generate the golden input/output vectors under tests/golden/ from the REAL reference.

Runs only in the build container (needs /root/reference and Cython).  The reference's pysam-free
modules (tiddit_coverage.pyx, tiddit_gc.pyx, tiddit_cluster.pyx, DBSCAN.py) are cythonized from
where they lie into a scratch dir under /tmp (never into this repo), imported, fed the inputs
below, and only DATA (inputs + the reference's outputs) is written here.  tiddit_gc.pyx imports
pysam for FastaFile only; a tiny in-memory stand-in (oracle-side tooling, lives in /tmp) serves
the sequences.  Nothing in tests/, bench.py or smoke() reads /root/reference at run time.

usage: python tests/golden/make_golden.py [--slow | --large | --grch38 | --only-y-labels | --only-edges | --only-coverage-edges]
  --slow adds the 1M-point DBSCAN run (~6 min); --large makes ONLY sv_e2e_large.json (the 240-Mb file of bench.py's sv_e2e section, ~12 min)
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
REF = "/root/reference/tiddit"
BUILD = "/tmp/tiddit_ref_build"
sys.path.insert(0, REPO)
from tiddit_amd import synth  # noqa: E402


def build_reference():
    pkg = os.path.join(BUILD, "tiddit")
    os.makedirs(pkg, exist_ok=True)
    with open(os.path.join(pkg, "__init__.py"), "w") as f:
        # pure-python modules (DBSCAN.py) are picked up from the reference tree itself
        f.write("__path__.append(%r)\n" % REF)
    with open(os.path.join(BUILD, "pysam.py"), "w") as f:
        f.write(
            "SEQS = {}\n"
            "class FastaFile:\n"
            "    def __init__(self, path): self.path = path\n"
            "    def get_reference_length(self, c): return len(SEQS[c])\n"
            "    def fetch(self, c, s, e): return SEQS[c][s:e]\n"
            "READS = lambda: iter(())\n"
            "class AlignmentFile:\n"
            "    def __init__(self, *a, **k): pass\n"
            "    def fetch(self, *a, **k): return READS()\n"
            "    def close(self): pass\n")
    inc = sysconfig.get_paths()["include"]
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    for mod in ("tiddit_coverage", "tiddit_gc", "tiddit_cluster", "tiddit_coverage_analysis"):
        so = os.path.join(pkg, mod + ext)
        if os.path.exists(so):
            continue
        c = os.path.join(BUILD, mod + ".c")
        subprocess.check_call(["cython", "-3", os.path.join(REF, mod + ".pyx"), "-o", c])
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-w", "-I", inc, "-I", np.get_include(),
                               c, "-o", so])
    sys.path.insert(0, BUILD)
    mods = {m: importlib.import_module("tiddit." + m)
            for m in ("tiddit_coverage", "tiddit_gc", "tiddit_cluster", "DBSCAN", "tiddit_coverage_analysis", "tiddit_stats")}
    mods["pysam"] = importlib.import_module("pysam")
    return mods


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# --------------------------------------------------------------------------------- coverage
def golden_coverage(M, out):
    cov = M["tiddit_coverage"]
    kat = []
    hdr = {"SQ": [{"SN": "c", "LN": 1137}]}
    for s, e in [(0, 150), (350, 500), (450, 600), (499, 501), (400, 1100), (900, 1100), (990, 1137),
                 (1000, 1137), (0, 1137), (500, 1000), (499, 1001), (1136, 1137), (0, 1), (999, 1000)]:
        arr, ebs = cov.create_coverage(hdr, 500, "c")
        r = cov.update_coverage(s, e, 500, arr, ebs)
        assert r is arr
        kat.append({"LN": 1137, "bin": 500, "s": s, "e": e, "bins": [float(x) for x in arr]})
    # create_coverage shapes
    shapes = []
    for LN, z in [(1137, 500), (1000, 500), (1, 500), (500, 500), (501, 500), (123457, 50), (999, 1000)]:
        d, eb = cov.create_coverage({"SQ": [{"SN": "a", "LN": LN}, {"SN": "b", "LN": 77}]}, z)
        shapes.append({"LN": LN, "bin": z, "nbins": int(len(d["a"])), "end_bin_size": int(eb["a"]),
                       "nbins_b": int(len(d["b"])), "end_bin_size_b": int(eb["b"])})
    # random property cases: many contig/bin shapes, reads of mixed span
    rng = np.random.default_rng(7)
    cases = {}
    for ci, (LN, z, n, maxspan) in enumerate([(1137, 500, 300, 400), (100000, 50, 5000, 400), (100000, 500, 5000, 400),
                                              (65536, 64, 4000, 1000), (12345, 7, 2000, 100), (250000, 1000, 3000, 30000),
                                              (5000, 5000, 200, 300), (5001, 5000, 200, 300), (99999, 333, 4000, 5000),
                                              (3000, 1, 500, 40)]):
        arr, ebs = cov.create_coverage({"SQ": [{"SN": "c", "LN": LN}]}, z, "c")
        s = np.sort(rng.integers(0, LN, n))
        e = np.minimum(s + rng.integers(1, maxspan, n), LN)
        for a, b in zip(s.tolist(), e.tolist()):
            arr = cov.update_coverage(a, b, z, arr, ebs)
        cases["c%d_meta" % ci] = np.array([LN, z], dtype=np.int64)
        cases["c%d_start" % ci] = s.astype(np.int64)
        cases["c%d_end" % ci] = e.astype(np.int64)
        cases["c%d_bins" % ci] = arr
    np.savez_compressed(os.path.join(out, "coverage_random.npz"), **cases)

    # config-1 stream (BASELINE configs[0]): gen_reads(1_000_000, 10), z 500 q 20, --cov filter
    L = 1_000_000
    start, end, mapq, flag = synth.gen_reads(L, 10)
    hdr = {"SQ": [{"SN": "chrS", "LN": L}]}
    res = {}
    for tag, z, q in (("cov", 500, 20), ("sv", 50, 5)):
        if tag == "cov":
            d, eb = cov.create_coverage(hdr, z)
            arr, ebs = d["chrS"], eb["chrS"]
        else:
            arr, ebs = cov.create_coverage(hdr, z, "chrS")
        kept = 0
        for s, e, mq, fl in zip(start.tolist(), end.tolist(), mapq.tolist(), flag.tolist()):
            if fl & 0x4 or fl & 0x400:
                continue
            if mq >= q:
                kept += 1
                arr = cov.update_coverage(s, e, z, arr, ebs)
        res[tag] = {"bin": z, "q": q, "n_reads": int(len(start)), "kept": kept, "nbins": int(len(arr)),
                    "sum": float(arr.sum()), "bins_sha256": sha(arr.astype("<f8"))}
        np.save(os.path.join(out, "config1_bins_%s.npy" % tag), arr)
        if tag == "cov":
            with tempfile.TemporaryDirectory() as td:
                for ft in ("bed", "wig"):
                    p = os.path.join(td, "o." + ft)
                    cov.print_coverage({"chrS": arr}, hdr, z, ft, p)
                    b = open(p, "rb").read()
                    res[tag][ft + "_sha256"] = hashlib.sha256(b).hexdigest()
                    res[tag][ft + "_head"] = b[:300].decode()
                    res[tag][ft + "_tail"] = b[-120:].decode()
    # print_coverage on a two-contig header (bed +1 quirk, last-bin end = LN)
    hdr2 = {"SQ": [{"SN": "a", "LN": 1137}, {"SN": "b", "LN": 1000}]}
    d, eb = cov.create_coverage(hdr2, 500)
    d["a"] = cov.update_coverage(400, 1100, 500, d["a"], eb["a"])
    d["b"] = cov.update_coverage(10, 160, 500, d["b"], eb["b"])
    with tempfile.TemporaryDirectory() as td:
        for ft in ("bed", "wig"):
            p = os.path.join(td, "o." + ft)
            cov.print_coverage(d, hdr2, 500, ft, p)
            res["print_" + ft] = open(p).read()
    json.dump({"kat": kat, "shapes": shapes, "config1": res}, open(os.path.join(out, "coverage.json"), "w"), indent=1)
    print("coverage:", res["cov"]["bins_sha256"], res["sv"]["bins_sha256"])


# --------------------------------------------------------------------------------------- gc
def golden_gc(M, out):
    gc = M["tiddit_gc"]
    seqs = M["pysam"].SEQS
    kat = []
    for seq, bs, cut in [("G" + "A" * 7, 50, 0.5), ("GGG" + "A" * 5, 50, 0.5), ("N" * 25 + "G" * 25, 50, 0.5),
                         ("N" * 26 + "G" * 24, 50, 0.5), ("n" * 26 + "G" * 24 + "N" * 30, 50, 0.5),
                         ("A" * 50 + "N" * 20, 50, 0.5), ("acgtRYSW" * 6 + "gc", 50, 0.5),
                         ("ACGT" * 30, 7, 0.5), ("GC" * 10 + "N" * 3 + "AT" * 10, 5, 0.2), ("G", 50, 0.5),
                         ("C" * 50, 50, 0.5), ("CG" * 100 + "N" * 101, 200, 0.5), ("N" * 10, 3, 0.0),
                         ("ANNA" * 10, 4, 0.5), ("ANNA" * 10, 4, 0.49)]:
        seqs["k"] = seq
        r = gc.binned_gc("mem.fa", "k", bs, cut)
        assert r[0] == "k" and r[1].dtype == np.int8
        kat.append({"seq": seq, "bin": bs, "n_cutoff": cut, "out": [int(x) for x in r[1]]})
    json.dump({"kat": kat}, open(os.path.join(out, "gc.json"), "w"), indent=1)
    cases = {}
    for ci, (L, bs, cut, seed) in enumerate([(200_003, 50, 0.5, 1), (50_000, 50, 0.1, 2), (30_011, 7, 0.5, 3),
                                             (120_000, 500, 0.5, 4), (70_001, 64, 0.25, 5), (40_000, 1, 0.5, 6),
                                             (100_000, 3000, 0.3, 7), (20_000, 20_000, 0.5, 8), (20_001, 20_000, 0.5, 9)]):
        s = synth.gen_sequence(L, seed=seed, n_frac=0.08)
        seqs["r"] = s.tobytes().decode()
        r = gc.binned_gc("mem.fa", "r", bs, cut)
        cases["c%d_meta" % ci] = np.array([L, bs, seed], dtype=np.int64)
        cases["c%d_cut" % ci] = np.array([cut])
        cases["c%d_out" % ci] = r[1]
    np.savez_compressed(os.path.join(out, "gc_random.npz"), **cases)
    seqs["x"] = "ACGT"
    seqs["y"] = "NNNN"
    d = gc.main("mem.fa", ["x", "y"], 1, 2, 0.5)
    assert sorted(d) == ["x", "y"]
    print("gc: %d kats, %d random cases" % (len(kat), len(cases) // 3))


# ----------------------------------------------------------------------------------- dbscan
def golden_dbscan(M, out, slow):
    D = M["DBSCAN"]
    kat = []

    def run(data, eps, m):
        data = np.array(data)
        xl, xid = D.x_coordinate_clustering(data, eps, m)
        xl = xl.copy()
        yl, yid = D.y_coordinate_clustering(data, eps, m, xid, xl.copy())
        full = D.main(data, eps, m)
        assert np.array_equal(full, yl)
        return xl, int(xid), yl, int(yid)

    for data, eps, m in [([[1, 2], [1, 2], [1, 2], [10, 11]], 0.1, 2),
                         ([[v, v] for v in [100, 110, 120, 130, 10000, 20000, 30000]], 500, 3),
                         ([[v, v] for v in [100, 110, 120, 10000, 20000, 30000, 40000]], 500, 3),
                         ([[v, v] for v in [100, 10000, 20000, 30000, 30010, 30020]], 500, 3),
                         ([[1, 1], [2, 2]], 500, 3),
                         ([[1, 1], [2, 2], [3, 3]], 500, 3),
                         ([[1, 1], [2, 5000], [3, 2], [4, 5001], [5, 3], [6, 5002], [7, 4], [8, 5003]], 500, 3),
                         ([[i, (i * 7919) % 1000] for i in range(40)], 30, 2),
                         ([[i * 100, 5] for i in range(30)], 500, 3),
                         ([[i * 100, i * 100] for i in range(30)], 100, 3),
                         ([[i * 100, i * 100] for i in range(30)], 101, 3),
                         ([[5, 5]] * 10, 1, 4)]:
        xl, xid, yl, yid = run(data, eps, m)
        kat.append({"data": data, "eps": eps, "m": m, "x": xl.tolist(), "x_id": xid, "y": yl.tolist(), "y_id": yid})
    json.dump({"kat": kat}, open(os.path.join(out, "dbscan.json"), "w"))
    # random cases (sorted by x, as tiddit_cluster hands them over), varied density / eps / m
    rng = np.random.default_rng(11)
    cases = {}
    nc = 0
    for rep in range(260):
        n = int(rng.choice([0, 1, 2, 3, 4, 5, 8, 17, 64, 65, 200, 700]))
        m = int(rng.choice([2, 3, 3, 3, 4, 5, 8]))
        eps = int(rng.choice([1, 5, 50, 500, 500, 5000]))
        span = int(rng.choice([50, 1000, 20000, 1000000]))
        x = np.sort(rng.integers(0, span, n))
        mode = rep % 3
        if mode == 0:
            y = rng.integers(0, span, n)
        elif mode == 1:
            y = x + rng.integers(0, 3 * eps, n)
        else:
            y = np.where(rng.random(n) < 0.5, x + rng.integers(0, eps, n), rng.integers(0, span, n))
        data = np.stack([x, y, np.arange(n)], 1).astype(np.int64).reshape(n, 3)
        if n == 0:
            continue  # reference indexes data[i,:] only inside loops; len 0 works but set() of empty is trivial
        xl, xid, yl, yid = run(data, eps, m)
        cases["r%d_data" % nc] = data
        cases["r%d_par" % nc] = np.array([eps, m, xid, yid], dtype=np.int64)
        cases["r%d_x" % nc] = xl
        cases["r%d_y" % nc] = yl
        nc += 1
    np.savez_compressed(os.path.join(out, "dbscan_random.npz"), **cases)
    # unsorted x (x_coordinate_clustering is also called on clip positions; abs() makes it order-agnostic)
    ucases = {}
    for rep in range(40):
        n = int(rng.choice([5, 17, 64, 300]))
        m = int(rng.choice([2, 3, 4]))
        eps = int(rng.choice([5, 50, 500]))
        x = rng.integers(0, 2000, n)
        data = np.stack([x, x], 1).astype(np.int64)
        xl, xid = D.x_coordinate_clustering(data, eps, m)
        ucases["u%d_data" % rep] = data
        ucases["u%d_par" % rep] = np.array([eps, m, xid], dtype=np.int64)
        ucases["u%d_x" % rep] = xl
    np.savez_compressed(os.path.join(out, "dbscan_unsorted_x.npz"), **ucases)
    # planted-cluster generator, 100k (and 1M with --slow)
    res = {}
    sizes = [100_000] + ([1_000_000] if slow else [])
    for n in sizes:
        pts = synth.gen_points(n)
        xl, xid = D.x_coordinate_clustering(pts, 500, 3)
        nx = int(xid) + 1
        lab, yid = D.y_coordinate_clustering(pts, 500, 3, xid, xl)
        res[str(n)] = {"eps": 500, "m": 3, "x_clusters": nx, "final_max_id": int(lab.max()),
                       "n_noise": int((lab == -1).sum()), "labels_sha256": sha(lab.astype("<f8"))}
        if n == 100_000:
            np.save(os.path.join(out, "dbscan_100k_labels_i32.npy"), lab.astype(np.int32))
        print("dbscan", n, res[str(n)])
    prev = {}
    p = os.path.join(out, "dbscan_gen.json")
    if os.path.exists(p):
        prev = json.load(open(p))
    prev.update(res)
    json.dump(prev, open(p, "w"), indent=1)


def golden_dbscan_y_labels(M, out):
    """DBSCAN.y_coordinate_clustering of the real reference on label arrays its own x pass would NOT produce: labels from another
    eps / m, clusters above 128 members, a value on several ranges, arbitrary (sparse, float, negative) values, a starting
    cluster_id below the largest label (the produced ids then collide with clusters not visited yet and get merged by the later
    `clusters == cluster` mask, DBSCAN.py:70-72,115).  -> dbscan_y_labels.npz"""
    D = M["DBSCAN"]
    rng = np.random.default_rng(23)
    cases, nc = {}, 0

    def add(data, eps, m, cid, lab, kind):
        nonlocal nc
        data = np.ascontiguousarray(data, dtype=np.int64)
        lab = np.ascontiguousarray(lab, dtype=np.float64)
        got, gid = D.y_coordinate_clustering(data, eps, m, cid, lab.copy())
        cases["c%d_data" % nc] = data
        cases["c%d_par" % nc] = np.array([eps, m, cid, int(gid)], dtype=np.int64)
        cases["c%d_in" % nc] = lab
        cases["c%d_out" % nc] = np.asarray(got, dtype=np.float64)
        cases["c%d_kind" % nc] = np.array(kind)
        nc += 1

    def points(n, span, eps, mode):
        x = np.sort(rng.integers(0, span, n))
        if mode == 0:
            y = rng.integers(0, span, n)
        elif mode == 1:
            y = x + rng.integers(0, 3 * eps, n)
        else:
            y = np.where(rng.random(n) < 0.5, x + rng.integers(0, eps, n), rng.integers(0, span, n))
        return np.stack([x, y], 1)

    for rep in range(120):
        n = int(rng.choice([3, 8, 40, 130, 300, 700]))
        m = int(rng.choice([2, 3, 3, 4, 6]))
        eps = int(rng.choice([5, 50, 500, 5000]))
        data = points(n, int(rng.choice([1000, 20000, 1000000])), eps, rep % 3)
        kind = rep % 6
        if kind == 0:        # the x pass of ANOTHER (eps, m): contiguous ascending ids, any cluster_id at or above the largest
            xl, xid = D.x_coordinate_clustering(data, eps * int(rng.choice([2, 10, 100])), int(rng.choice([2, 3, 5])))
            add(data, eps, m, int(xid) + int(rng.integers(0, 4)), xl, "other_eps")
        elif kind == 1:      # few large clusters (well above 128 members), contiguous
            k = int(rng.integers(1, 4))
            lab = np.sort(rng.integers(0, k, n)).astype(np.float64)
            lab[rng.random(n) < 0.1] = -1
            add(data, eps, m, k - 1 + int(rng.integers(0, 3)), lab, "large")
        elif kind == 2:      # the same value on several ranges (members selected by value, not by range)
            lab = rng.integers(-1, 6, n).astype(np.float64)
            add(data, eps, m, 5 + int(rng.integers(0, 3)), lab, "split_ranges")
        elif kind == 3:      # arbitrary values: sparse, large, non-integer, below -1; cluster_id above all of them
            vals = np.array([0.0, 7.0, 2.5, 1e6, -3.0, 12345.0, 64.0, 1023.0, -1.0, 8.0])
            lab = rng.choice(vals, n)
            add(data, eps, m, 2_000_000 + int(rng.integers(0, 3)), lab, "arbitrary")
        elif kind == 4:      # cluster_id BELOW the largest label: produced ids collide with unvisited clusters
            xl, xid = D.x_coordinate_clustering(data, eps * 20, 2)
            add(data, max(eps // 4, 1), m, int(rng.integers(-1, max(int(xid), 0) + 1)), xl, "collide")
        else:                # collisions on random dense labels
            lab = rng.integers(-1, 12, n).astype(np.float64)
            add(data, eps, m, int(rng.integers(-1, 8)), lab, "collide_random")
    # one case at a size where the visiting order of set() is far from trivial: 3000 distinct sparse values
    n = 6000
    data = points(n, 400000, 50, 1)
    lab = rng.choice(rng.integers(0, 10**7, 3000), n).astype(np.float64)
    add(data, 50, 3, 10**7, lab, "many_sparse")
    np.savez_compressed(os.path.join(out, "dbscan_y_labels.npz"), **cases)
    print("dbscan_y_labels:", nc, "cases")


def golden_dbscan_edges(M, out):
    """The real DBSCAN.py on the small aimed cases of tests/cluster_stage_cases.py (tile, route and bucket edges of the clustering
    kernels), bucket by bucket: x_coordinate_clustering for every case and main for the cases of mode 0.  Only the labels (int32), the
    ids per bucket and a hash of the inputs are stored; the inputs are regenerated from the case module.  -> dbscan_edges.npz"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import cluster_stage_cases as cc
    D = M["DBSCAN"]
    res, names, hashes, xids = {}, [], [], []
    for name in cc.case_names():
        c = cc.get(name)
        if not cc.in_golden(c):
            continue
        xl, ml = np.full(c["n"], -1, dtype=np.int32), np.full(c["n"], -1, dtype=np.int32)
        xid = np.full(c["nb"], -1, dtype=np.int64)
        for b in range(c["nb"]):
            lo, hi = int(c["off"][b]), int(c["off"][b + 1])
            if lo == hi:
                continue
            data = np.stack([c["x"][lo:hi], c["y"][lo:hi]], 1)
            lab, cid = D.x_coordinate_clustering(data, c["eps"], c["m"])
            xl[lo:hi], xid[b] = lab, cid
            if c["mode"] == 0:
                ml[lo:hi] = D.main(data, c["eps"], c["m"])
        k = len(names)
        names.append(name)
        res["c%d_x" % k] = xl
        if c["mode"] == 0:
            res["c%d_main" % k] = ml
        hashes.append(cc.input_hash(c))
        xids.append(xid)
    res["names"], res["hashes"], res["xid"] = np.array(names), np.array(hashes), np.concatenate(xids)      # (xid: nb values per case, in order)
    np.savez_compressed(os.path.join(out, "dbscan_edges.npz"), **res)
    print("dbscan_edges:", len(names), "cases,", os.path.getsize(os.path.join(out, "dbscan_edges.npz")), "bytes")


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def golden_coverage_edges(M, out):
    """The real update_coverage, read by read behind the filter of __main__.py:231-235, on the small aimed cases of
    tests/coverage_stage_cases.py (window, table and contig-end edges of the coverage kernels).  Stored sparse — the indices and values
    of the nonzero bins of every contig — with a hash of the inputs, which are regenerated from the case module.  -> coverage_edges.npz"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import coverage_stage_cases as cc
    cov = M["tiddit_coverage"]
    res, names, hashes = {}, [], []
    for name in cc.case_names():
        c = cc.get(name)
        if not cc.in_golden(c):
            continue
        k = len(names)
        for ci, ((sn, LN), (start, end, mapq, flag)) in enumerate(zip(c["contigs"], c["cols"])):
            arr = np.zeros(0)
            if LN:
                arr, ebs = cov.create_coverage({"SQ": [{"SN": sn, "LN": LN}]}, c["z"], sn)
            for s, e, q, f in zip(start.tolist(), end.tolist(), mapq.tolist(), flag.tolist()):
                if f & 0x4 or f & 0x400 or q < c["min_q"]:
                    continue
                arr = cov.update_coverage(s, e, c["z"], arr, ebs)
            nz = np.flatnonzero(arr)
            res["k%d_c%d_idx" % (k, ci)], res["k%d_c%d_val" % (k, ci)] = nz.astype(np.int32), arr[nz].astype("<f8")
        names.append(name)
        hashes.append(cc.input_hash(c))
    res["names"], res["hashes"] = np.array(names), np.array(hashes)
    write_npz(os.path.join(out, "coverage_edges.npz"), res)
    print("coverage_edges:", len(names), "cases,", os.path.getsize(os.path.join(out, "coverage_edges.npz")), "bytes")


def load_dbscan_only():
    """the reference's DBSCAN.py alone (pure Python: nothing to compile)"""
    pkg = os.path.join(BUILD, "tiddit")
    os.makedirs(pkg, exist_ok=True)
    with open(os.path.join(pkg, "__init__.py"), "w") as f:
        f.write("__path__.append(%r)\n" % REF)
    sys.path.insert(0, BUILD)
    return {"DBSCAN": importlib.import_module("tiddit.DBSCAN")}


# ---------------------------------------------------------------------------------- cluster
def _jsonable(c):
    if isinstance(c, dict):
        return {str(k): _jsonable(v) for k, v in c.items()}
    if isinstance(c, set):
        return {"__set__": sorted(_jsonable(x) for x in c)}
    if isinstance(c, (list, tuple)):
        return [_jsonable(x) for x in c]
    if isinstance(c, (np.integer,)):
        return int(c)
    if isinstance(c, (np.floating,)):
        return float(c)
    return c


def golden_cluster(M, out):
    cl = M["tiddit_cluster"]
    # find_discordant_pos truth table
    fdp = []
    frag = ["q", "1", "1", "100", "250", None, "900", "1050", None]
    for mp in (True, False):
        for a in ("True", "False"):
            for b in ("True", "False"):
                f = list(frag)
                f[5], f[8] = a, b
                fdp.append({"is_mp": mp, "revA": a, "revB": b, "out": list(cl.find_discordant_pos(f, mp))})
    rng = np.random.default_rng(5)
    cases = []
    for case in range(6):
        chroms = ["chr1", "chr2", "chrM"]
        lens = {"chr1": 200000, "chr2": 150000, "chrM": 9000}
        disc, splits = [], []
        qn = 0
        n_events = [4, 12, 30, 3, 20, 60][case]
        for ev in range(n_events):
            ca = chroms[int(rng.integers(0, 3))]
            cb = chroms[int(rng.integers(0, 3))]
            if cb < ca:
                ca, cb = cb, ca
            pa = int(rng.integers(500, lens[ca] - 100))
            pb = int(rng.integers(500, lens[cb] + 400)) if ca != cb else int(min(lens[cb] + 300, pa + rng.integers(300, 30000)))
            for _ in range(int(rng.integers(1, 9))):
                qn += 1
                sa = pa + int(rng.integers(-150, 150))
                sb = pb + int(rng.integers(-150, 150))
                ra, rb = rng.random() < 0.8, rng.random() < 0.2
                disc.append("q%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%s" % (qn, ca, cb, sa, sa + 150, ra, sb, sb + 150, rb))
            for _ in range(int(rng.integers(0, 6))):
                qn += 1
                spa = pa + int(rng.integers(0, 3))
                spb = pb + int(rng.integers(0, 3))
                splits.append("s%d\t%s\t%s\t%d\t%s\t%d\t%s\t%d\t%d\t%d\t%d" % (
                    qn, ca, cb, spa, rng.random() < 0.5, spb, rng.random() < 0.5, spa - 80, spa, spb, spb + 70))
        for _ in range(n_events * 2):  # background noise pairs
            qn += 1
            ca = cb = "chr1"
            sa = int(rng.integers(1, 190000))
            sb = int(rng.integers(sa, 199000))
            disc.append("n%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%s" % (qn, ca, cb, sa, sa + 150, False, sb, sb + 150, True))
        order = rng.permutation(len(disc))
        disc = [disc[i] for i in order]
        is_mp = case == 3
        eps, m, max_ins, min_contig, min_reads = [(175, 3, 600, 10000, 3), (175, 3, 600, 10000, 3), (250, 3, 600, 5000, 3),
                                                  (175, 2, 600, 10000, 2), (100, 4, 600, 10000, 3), (300, 3, 800, 10000, 3)][case]
        with tempfile.TemporaryDirectory() as td:
            os.mkdir(os.path.join(td, "p_tiddit"))
            open(os.path.join(td, "p_tiddit", "discordants_S.tab"), "w").write("".join(l + "\n" for l in disc))
            open(os.path.join(td, "p_tiddit", "splits_S.tab"), "w").write("".join(l + "\n" for l in splits))
            cand = cl.main(os.path.join(td, "p"), chroms, lens, ["S"], is_mp, eps, m, max_ins, min_contig, True, min_reads)
        cases.append({"chromosomes": chroms, "contig_length": lens, "is_mp": is_mp, "epsilon": eps, "m": m,
                      "max_ins_len": max_ins, "min_contig": min_contig, "min_reads": min_reads,
                      "discordants_tab": disc, "splits_tab": splits, "candidates": _jsonable(cand)})
        ncand = sum(len(cand[a][b]) for a in cand for b in cand[a])
        print("cluster case", case, "signals", len(disc) + len(splits), "candidates", ncand)
    json.dump({"find_discordant_pos": fdp, "cases": cases}, open(os.path.join(out, "cluster.json"), "w"))


# --------------------------------------------------------------------------------- `tiddit --sv --skip_assembly`, BASELINE configs[3]
E2E = {"total_mb": 24, "seed": 7, "depth": 30, "read_len": 150, "insert": 400, "insert_sd": 40, "sv_per_mb": 3.0, "fasta_seed": 100,
       "min_q": 5, "n_reads_stats": 25000000, "min_contig": 10000, "min_anchor_len": 60, "min_clip_len": 25, "m": 3, "min_reads": 3, "ploidy": 2}


class _StatRead:
    __slots__ = ("query_length", "mate_is_unmapped", "is_reverse", "mate_is_reverse", "next_reference_name", "reference_name",
                 "template_length", "next_reference_start", "reference_start", "is_supplementary", "is_secondary", "is_duplicate", "mapq")


def stat_reads(fields, names):
    """the attributes tiddit_stats.statistics reads (tiddit_stats.py:17-47), record by record, for `samfile.fetch()` —
    placed records only, in file order"""
    def gen():
        r = _StatRead()
        cols = [fields[k].tolist() for k in ("tid", "pos", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "l_seq")]
        for tid, pos, mapq, flag, mtid, mpos, tlen, lseq in zip(*cols):
            if tid < 0:
                continue
            r.query_length = lseq
            r.mate_is_unmapped, r.is_reverse, r.mate_is_reverse = bool(flag & 0x8), bool(flag & 0x10), bool(flag & 0x20)
            r.reference_name, r.next_reference_name = names[tid], (names[mtid] if mtid >= 0 else None)
            r.template_length, r.next_reference_start, r.reference_start = tlen, mpos, pos
            r.is_supplementary, r.is_secondary, r.is_duplicate, r.mapq = bool(flag & 0x800), bool(flag & 0x100), bool(flag & 0x400), mapq
            yield r
    return gen


def golden_sv_e2e(M, out, params=None, name="sv_e2e.json"):
    """The whole --sv --skip_assembly path on a WGS-shaped synthetic BAM (tiddit_amd.synth_bam.write_wgs_sv_bam, everything derived
    from a seed so the GPU box regenerates the identical file): library statistics by the reference's tiddit_stats.py (stub
    AlignmentFile serving the decoded records), signal extraction by the restatement (oracle/signal_oracle.py — tiddit_signal.pyx
    cannot be compiled here), GC by the compiled tiddit_gc, ploidies by the compiled tiddit_coverage_analysis, candidates by the
    compiled tiddit_cluster on the restatement's .tab files."""
    import oracle
    from oracle import signal_oracle
    from tiddit_amd import synth_bam
    P = dict(E2E)
    P.update(params or {})
    contigs = synth_bam.contigs_for(P)
    with tempfile.TemporaryDirectory() as td:
        fa, bam, prefix = os.path.join(td, "ref.fa"), os.path.join(td, "WGS.bam"), os.path.join(td, "out")
        seqs = synth_bam.write_fasta(fa, contigs, seed=P["fasta_seed"])
        info = synth_bam.write_wgs_sv_bam(bam, contigs, depth=P["depth"], read_len=P["read_len"], insert=P["insert"], insert_sd=P["insert_sd"],
                                          seed=P["seed"], sv_per_mb=P["sv_per_mb"], threads=8, ref_seqs=seqs)
        header, sq, raw = signal_oracle.inflate_bam(bam)
        fields = oracle.bam_walk(raw)
        names = [c["SN"] for c in sq]
        M["pysam"].READS = stat_reads(fields, names)
        library = M["tiddit_stats"].statistics(bam, fa, P["min_q"], 100000, P["n_reads_stats"])
        lib0 = {k: (float(v) if not isinstance(v, bool) else v) for k, v in library.items()}
        max_ins = library["percentile_insert_size"]
        cov, disc, split, clips, clip_each, n_rec = signal_oracle.signal_main_file(bam, P["min_q"], max_ins, "WGS", P["min_contig"],
                                                                                   P["min_anchor_len"], P["min_clip_len"])
        os.makedirs(prefix + "_tiddit")
        open(prefix + "_tiddit/discordants_WGS.tab", "w").write(disc)
        open(prefix + "_tiddit/splits_WGS.tab", "w").write(split)
        # GC (compiled tiddit_gc.binned_gc through the FastaFile stand-in) and ploidies (compiled determine_ploidy)
        M["pysam"].SEQS = {n: seqs[n].tobytes().decode() for n, _ in contigs}
        gc = {n: M["tiddit_gc"].binned_gc(fa, n, 50, 0.5)[1] for n, _ in contigs}
        lib = M["tiddit_coverage_analysis"].determine_ploidy(cov, names, dict(library), P["ploidy"], prefix, None, fa, 50, header, gc)
        ploidies = open(prefix + ".ploidies.tab").read()
        eps = int(library["avg_insert_size"] / 2.0) or 50
        contig_length = {c["SN"]: c["LN"] for c in sq}
        cand = M["tiddit_cluster"].main(prefix, names, contig_length, ["WGS"], library["mp"], eps, P["m"], max_ins, P["min_contig"], True, P["min_reads"])
    from oracle import cluster_oracle
    h = lambda t: hashlib.sha256(t.encode()).hexdigest()
    res = {"params": P, "n_records": int(n_rec), "n_events": len(info["events"]), "events": info["events"], "library": lib0,
           "epsilon": eps,
           "discordants_sha256": h(disc), "discordants_rows": disc.count("\n"), "splits_sha256": h(split), "splits_rows": split.count("\n"),
           "clips_sha256": h(clips), "clips_entries": clips.count(">"),
           "coverage_sha256": {n: sha(cov[n].astype("<f8")) for n in cov},
           # (a table of thousands of contigs: one checksum each for the contigs the job processes, ONE over all the others in header order)
           "gc_sha256": {n: sha(gc[n]) for n, ln in contigs if len(contigs) <= 100 or ln >= P["min_contig"]},
           "gc_sha256_rest": None if len(contigs) <= 100 else sha(np.concatenate([np.ascontiguousarray(gc[n]).view(np.uint8).ravel() for n, ln in contigs if ln < P["min_contig"]])),
           "ploidies_tab": ploidies, "library_after_ploidy": {k: float(v) for k, v in lib.items() if k.startswith(("avg_coverage", "contig_ploidy"))},
           "candidates_sha256": h(cluster_oracle.canonical(cand)), "candidates": cluster_oracle.summary(cand)}
    json.dump(res, open(os.path.join(out, name), "w"), indent=0)
    print("sv_e2e:", n_rec, "records,", res["discordants_rows"], "discordant rows,", res["splits_rows"], "split rows,", len(res["candidates"]), "candidates")
    return res


def main():
    slow = "--slow" in sys.argv
    if "--only-edges" in sys.argv:
        golden_dbscan_edges(load_dbscan_only(), HERE)
        return
    M = build_reference()
    if "--only-coverage-edges" in sys.argv:
        golden_coverage_edges(M, HERE)
        return
    if "--only-y-labels" in sys.argv:
        golden_dbscan_y_labels(M, HERE)
        return
    if "--grch38" in sys.argv:      # tests/golden/sv_e2e_grch38.json: a header shaped like the GRCh38 analysis set's (3 366 contigs), ~25 Mb
        golden_sv_e2e(M, HERE, params={"total_mb": 24, "contig_table": "grch38", "seed": 38, "n_reads_stats": 400000}, name="sv_e2e_grch38.json")
        return
    if "--large" in sys.argv:       # tests/golden/sv_e2e_large.json: the 240-Mb file bench.py's sv_e2e section times (48 M records; ~12 min here)
        golden_sv_e2e(M, HERE, params={"total_mb": 240}, name="sv_e2e_large.json")
        return
    golden_coverage(M, HERE)
    golden_gc(M, HERE)
    golden_dbscan(M, HERE, slow)
    golden_dbscan_y_labels(M, HERE)
    golden_dbscan_edges(M, HERE)
    golden_coverage_edges(M, HERE)
    golden_cluster(M, HERE)
    golden_sv_e2e(M, HERE)
    golden_sv_e2e(M, HERE, params={"total_mb": 3, "seed": 11, "sv_per_mb": 8.0, "n_reads_stats": 300000}, name="sv_e2e_small.json")


if __name__ == "__main__":
    main()
