"""Shared by the CPU and GPU tests of TIDDIT_GENOTYPE (tiddit_amd/tiddit_genotype.py, csrc/tdt_links.hip): the two reference
implementations of the link counts, the adversarial signal tables and sites they are compared on, and the golden VCF records turned
into the evidence the pure column function takes.

The link count of a site {bucket, startA, endA, startB, endB}: the signals of that bucket with startA <= posA <= endA and
startB <= posB <= endB, per kind (0 pair -> DV, 1 split -> RV, 2 contig -> neither); bucket -1 -> (0, 0).
``strict``: names of the comparisons ("startA", "endA", "startB", "endB") made strict (< for <=) — the mutants the cases must tell
from the definition."""
import numpy as np

BOUNDS = ("startA", "endA", "startB", "endB")


def link_counts_loop(posA, posB, kind, off, sites, strict=()):
    """the definition, as a plain double loop"""
    out = []
    for bucket, sA, eA, sB, eB in sites:
        dv = rv = 0
        if bucket >= 0:
            for i in range(int(off[bucket]), int(off[bucket + 1])):
                a, b = int(posA[i]), int(posB[i])
                okA0 = sA < a if "startA" in strict else sA <= a
                okA1 = a < eA if "endA" in strict else a <= eA
                okB0 = sB < b if "startB" in strict else sB <= b
                okB1 = b < eB if "endB" in strict else b <= eB
                if okA0 and okA1 and okB0 and okB1:
                    if kind[i] == 0:
                        dv += 1
                    elif kind[i] == 1:
                        rv += 1
        out.append((dv, rv))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def link_counts_numpy(posA, posB, kind, off, sites, strict=()):
    """the same through a sort of every bucket by posA and two binary searches per site (fast enough for 10^6 signals)"""
    posA, posB, kind = np.asarray(posA, dtype=np.int64), np.asarray(posB, dtype=np.int64), np.asarray(kind)
    by_bucket = {}
    out = np.zeros((len(sites), 2), dtype=np.int64)
    for q, (bucket, sA, eA, sB, eB) in enumerate(sites):
        if bucket < 0:
            continue
        if bucket not in by_bucket:
            lo, hi = int(off[bucket]), int(off[bucket + 1])
            order = np.argsort(posA[lo:hi], kind="stable")
            by_bucket[bucket] = (posA[lo:hi][order], posB[lo:hi][order], kind[lo:hi][order])
        a, b, k = by_bucket[bucket]
        lo = np.searchsorted(a, sA, "right" if "startA" in strict else "left")
        hi = np.searchsorted(a, eA, "left" if "endA" in strict else "right")
        if hi <= lo:
            continue
        bb, kk = b[lo:hi], k[lo:hi]
        m = (bb > sB if "startB" in strict else bb >= sB) & (bb < eB if "endB" in strict else bb <= eB)
        out[q] = (np.count_nonzero(m & (kk == 0)), np.count_nonzero(m & (kk == 1)))
    return out


def edge_sites(bucket, a, b):
    """sites whose four bounds sit exactly on, one below and one above the signal (a, b): every start <= end combination"""
    d = (-1, 0, 1)
    return [(bucket, a + s0, a + e0, b + s1, b + e1) for s0 in d for e0 in d if s0 <= e0 for s1 in d for e1 in d if s1 <= e1]


def _runs_bucket(rng, n, runs, span):
    """n signals with posA ascending in value but shuffled in row order, containing runs of equal posA of the given lengths"""
    a = np.sort(rng.integers(1000, span, n))
    at = 0
    marks = []
    for r in runs:
        r = min(r, n - at)
        if r <= 0:
            break
        start = at + int(rng.integers(0, 3))
        start = min(start, n - r)
        a[start:start + r] = a[start]
        marks.append((start, r))
        at = start + r + int(rng.integers(1, 50))
    a = np.sort(a)
    b = rng.integers(0, span, n)
    k = rng.choice([0, 1], n, p=[0.7, 0.3]).astype(np.uint8)
    p = rng.permutation(n)
    return a[p], b[p], k[p]


def small_table(seed=5):
    """buckets of 0, 1, 63, 64, 65 signals, one of pairs only, one of splits only, one with contig-kind rows, and one of 5 000 with
    runs of equal posA of 63 / 64 / 65 / 130 (the 64-lane stride, the last bracket of the search) -> (posA, posB, kind, off, sites)"""
    rng = np.random.default_rng(seed)
    cols, sizes = [], []
    for n in (0, 1, 63, 64, 65):
        cols.append((rng.integers(100, 400, n), rng.integers(100, 400, n), rng.choice([0, 1], n).astype(np.uint8)))
        sizes.append(n)
    n = 200
    cols.append((rng.integers(100, 300, n), rng.integers(100, 300, n), np.zeros(n, dtype=np.uint8)))
    cols.append((rng.integers(100, 300, n), rng.integers(100, 300, n), np.ones(n, dtype=np.uint8)))
    cols.append((rng.integers(100, 300, n), rng.integers(100, 300, n), rng.choice([0, 1, 2], n).astype(np.uint8)))
    sizes += [n, n, n]
    cols.append(_runs_bucket(rng, 5000, (63, 64, 65, 130), 40_000))
    sizes.append(5000)
    posA = np.concatenate([c[0] for c in cols]).astype(np.int32)
    posB = np.concatenate([c[1] for c in cols]).astype(np.int32)
    kind = np.concatenate([c[2] for c in cols]).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    sites = [(-1, 0, 10**6, 0, 10**6)]
    for bkt in range(len(sizes)):
        lo, hi = int(off[bkt]), int(off[bkt + 1])
        sites.append((bkt, 0, 10**6, 0, 10**6))                      # the whole bucket (an empty one too)
        sites.append((bkt, 250, 250, 0, 10**6))
        pick = rng.choice(np.arange(lo, hi), min(hi - lo, 6), replace=False) if hi > lo else []
        for i in pick:
            sites += edge_sites(bkt, int(posA[i]), int(posB[i]))
        if hi > lo:
            a = posA[lo:hi]
            vals, cnt = np.unique(a, return_counts=True)
            for v in vals[np.argsort(-cnt)[:4]]:                     # the longest runs of equal posA: bounds on, below and above them
                v = int(v)
                sites += [(bkt, v, v, 0, 10**6), (bkt, v - 1, v - 1, 0, 10**6), (bkt, v + 1, v + 1, 0, 10**6), (bkt, v - 1, v, 0, 10**6),
                          (bkt, v, v + 1, 0, 10**6), (bkt, 0, v - 1, 0, 10**6), (bkt, v + 1, 10**6, 0, 10**6)]
    return posA, posB, kind, off, sites


def large_table(seed=8, n_big=1_000_003):
    """a bucket of about 10^6 signals with runs of equal posA of 1, 63, 64, 65, 4 095, 4 096, 4 097 and 70 000 (every bracket size of
    the 64-ary search: 64, 64^2, 64^3 and the remainders), between two small buckets; 40 000 sites and more (more than the waves one
    grid holds at a time) -> (posA, posB, kind, off, sites)"""
    rng = np.random.default_rng(seed)
    small = (rng.integers(0, 5000, 65), rng.integers(0, 5000, 65), rng.choice([0, 1], 65).astype(np.uint8))
    big = _runs_bucket(rng, n_big, (1, 63, 64, 65, 4095, 4096, 4097, 70_000), 200_000_000)
    tail = (rng.integers(0, 5000, 1), rng.integers(0, 5000, 1), np.zeros(1, dtype=np.uint8))
    cols = [small, big, tail]
    sizes = [65, n_big, 1]
    posA = np.concatenate([c[0] for c in cols]).astype(np.int32)
    posB = np.concatenate([c[1] for c in cols]).astype(np.int32)
    kind = np.concatenate([c[2] for c in cols]).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    a = posA[65:65 + n_big]
    vals, cnt = np.unique(a, return_counts=True)
    W = 2**30 - 1
    sites = [(1, 0, W, 0, W), (0, 0, W, 0, W), (2, 0, W, 0, W), (-1, 0, W, 0, W)]
    for v in vals[np.argsort(-cnt)[:12]]:
        v = int(v)
        sites += [(1, v, v, 0, W), (1, v - 1, v - 1, 0, W), (1, v + 1, v + 1, 0, W), (1, v - 1, v, 0, W), (1, v, v + 1, 0, W),
                  (1, 0, v - 1, 0, W), (1, 0, v, 0, W), (1, v, W, 0, W), (1, v + 1, W, 0, W)]
    for i in rng.integers(0, n_big, 60):
        sites += edge_sites(1, int(a[i]), int(posB[65 + i]))
    centre = rng.integers(0, 200_000_000, 40_000)
    width = rng.integers(0, 5_000, 40_000)
    lo_b = rng.integers(0, 150_000_000, 40_000)
    for c, w, lb in zip(centre.tolist(), width.tolist(), lo_b.tolist()):
        sites.append((1, c, c + w, lb, lb + 60_000_000))
    return posA, posB, kind, off, sites


# ---- the golden VCFs as evidence ----------------------------------------------------------------------------------------------
def golden_evidence(fx):
    """a tests/golden/sv_vcf*.json fixture -> (contig_number, contig_length, [(line number, columns)] of its records, regions keyed
    (chrom, start, end, bp), cov_between keyed (chrA, chrB, startA, endA, startB, endB))"""
    from tiddit_amd import synth_bam
    contigs = synth_bam.contigs_for(fx["meta"]["params"])
    records = [(i + 1, l.split("\t")) for i, l in enumerate(fx["vcf_records"])]
    regions = {(c[0], c[1], c[2], c[3]): tuple(c[6]) for c in fx["get_region_calls"]}
    cols = fx["meta"]["candidate_columns"]
    between = {}
    for row in fx["candidates"]:
        r = dict(zip(cols, row))
        between[(r["chrA"], r["chrB"], r["startA"], r["endA"], r["startB"], r["endB"])] = r["covM"]
    return {n: i for i, (n, _) in enumerate(contigs)}, dict(contigs), records, regions, between
