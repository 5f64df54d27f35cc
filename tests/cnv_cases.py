"""Cases and references for the copy-number segments of ``tiddit --sv`` (``TIDDIT_CNV``, tiddit_amd/tiddit_cnv.py, csrc/tdt_cnv.hip).

Three references, none of which shares code with the product:
  * the literal definition of tiddit_cnv.py's docstring as plain Python loops over Python integers and floats (``ref_*``); its
    ``mutant`` argument switches ONE line to a plausible wrong reading, for tests/test_cnv_refs_cpu.py to show that the cases tell
    the readings apart;
  * an independent numpy restatement of the forward pass (``numpy_viterbi``: whole-vector steps, argmin / where);
  * for ``T <= 5`` the optimal cost by enumeration of all ``8**T`` paths (``brute_force_cost``).
Every case is built from literals or a seeded generator; a case's ``claims`` are checked on the CPU before the GPU tests rely on them."""
import functools
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r"^#define\s+CNV_CHUNK\s+(\d+)", open(os.path.join(REPO, "tiddit_amd", "csrc", "tdt_cnv.hip")).read(), re.M).group(1))
L = CHUNK
UNIT = 256
U = UNIT
STATES = 8
CAP = 4 * UNIT * UNIT
LAMBDA = 2 * UNIT * UNIT
MIN_CLASS = 100
HEADER = "#chrom\tstart\tend\ttype\tCN\tbins\tmeanCN\n"
MUTANTS = {"bp_lt": "tie", "argmin_high": "argmin", "no_end_penalty": "contig_end", "mask_le": "mask_threshold", "round_half_up": "rint_tie",
           "pairwise_sum": "sum_order"}


# ---- the literal definition ---------------------------------------------------------------------------------------------------
def _pairwise(values):
    if len(values) == 1:
        return values[0]
    h = len(values) // 2
    return _pairwise(values[:h]) + _pairwise(values[h:])


def ref_bins(cov, gc, K, P, E, unit=UNIT, mutant=None):
    """the CNV bins of ONE contig; E: the 101 expected depths of its classes -> list of x_t"""
    nb = len(cov)
    T = -(-nb // K)
    out = []
    for t in range(T):
        usable = [b for b in range(t * K, min((t + 1) * K, nb)) if int(gc[b]) != -1]
        n = len(usable)
        if (2 * n <= K) if mutant == "mask_le" else (2 * n < K):
            out.append(-1)
            continue
        if mutant == "pairwise_sum":
            obs = _pairwise([float(cov[b]) for b in usable])
            exp = _pairwise([float(E[int(gc[b])]) for b in usable])
        else:
            obs, exp = 0.0, 0.0
            for b in usable:
                obs = obs + float(cov[b])
            for b in usable:
                exp = exp + float(E[int(gc[b])])
        v = (obs / exp) * float(P * unit)
        r = int(np.floor(v + 0.5)) if mutant == "round_half_up" else int(np.rint(v))
        out.append(min(8 * unit, r))
    return out


def emission(x, k, unit=UNIT, cap=CAP):
    return 0 if x < 0 else min(cap, (int(x) - unit * k) ** 2)


def ref_viterbi(x, P, unit=UNIT, cap=CAP, lam=LAMBDA, mutant=None, details=None):
    """the states of ONE contig -> list of s_t.  details (a dict): 'cost' = the minimal end cost, 'ties' = the (t, k) with
    V_{t-1}(k) == m + lam exactly."""
    T = len(x)
    if T == 0:
        return []
    V = [emission(x[0], k, unit, cap) + (0 if k == P else lam) for k in range(STATES)]
    B = [None]
    ties = []
    for t in range(1, T):
        m = min(V)
        hits = [i for i in range(STATES) if V[i] == m]
        a = hits[-1] if mutant == "argmin_high" else hits[0]
        nV, b = [], []
        for k in range(STATES):
            if V[k] == m + lam:
                ties.append((t, k))
            stay = (V[k] < m + lam) if mutant == "bp_lt" else (V[k] <= m + lam)
            b.append(k if stay else a)
            nV.append(emission(x[t], k, unit, cap) + min(V[k], m + lam))
        V = nV
        B.append(b)
    end = [V[k] + (0 if (k == P or mutant == "no_end_penalty") else lam) for k in range(STATES)]
    best = min(end)
    hits = [k for k in range(STATES) if end[k] == best]
    s = [0] * T
    s[T - 1] = hits[-1] if mutant == "argmin_high" else hits[0]
    for t in range(T - 1, 0, -1):
        s[t - 1] = B[t][s[t]]
    if details is not None:
        details["cost"] = best
        details["ties"] = ties
    return s


def path_cost(x, P, s, unit=UNIT, cap=CAP, lam=LAMBDA):
    """what the model charges the path s"""
    c = 0 if s[0] == P else lam
    for t in range(len(x)):
        c += emission(x[t], s[t], unit, cap)
        if t and s[t] != s[t - 1]:
            c += lam
    return c + (0 if s[-1] == P else lam)


def ref_segments(s, x, P, W, length, chrom):
    T = len(s)
    out = []
    t = 0
    while t < T:
        e = t
        while e + 1 < T and s[e + 1] == s[t]:
            e += 1
        if s[t] != P:
            first, last = t, e
            while first <= last and x[first] < 0:
                first += 1
            while last >= first and x[last] < 0:
                last -= 1
            if first <= last:
                seen = [int(x[i]) for i in range(first, last + 1) if x[i] >= 0]
                out.append((chrom, first * W, min((last + 1) * W, length), "DEL" if s[t] < P else "DUP", s[t], len(seen),
                            "{:.3f}".format(sum(seen) / (len(seen) * UNIT))))
        t = e + 1
    return out


def ref_contig_median(cov, gc):
    v = [float(cov[b]) for b in range(len(cov)) if cov[b] > 0 and int(gc[b]) != -1]
    return float(np.median(v)) if v else float("nan")


def ref_expected(cov, gc, C):
    """E[101] of ONE contig"""
    E = []
    for g in range(101):
        v = [float(cov[b]) for b in range(len(cov)) if int(gc[b]) == g and cov[b] > 0]
        E.append(float(np.median(v)) if len(v) >= MIN_CLASS else C)
    return E


def ref_job(coverage_data, gc, library, contigs, contig_length, min_contig, W):
    """-> (the text of {o}.cnv.bed, the skipped contigs, {contig: (x, s)})"""
    K = W // 50
    lines, skipped, tracks = [], [], {}
    for c in contigs:
        P = library.get("contig_ploidy_%s" % c)
        ok = c in coverage_data and len(coverage_data[c]) >= 1 and contig_length[c] >= min_contig and P is not None and 1 <= P <= 6
        if ok:
            cov, g = coverage_data[c], gc[c][:len(coverage_data[c])]
            C = ref_contig_median(cov, g)
            ok = np.isfinite(C) and C > 0
        if not ok:
            skipped.append(c)
            continue
        x = ref_bins(cov, g, K, P, ref_expected(cov, g, C))
        s = ref_viterbi(x, P)
        tracks[c] = (x, s)
        lines += ref_segments(s, x, P, W, contig_length[c], c)
    return HEADER + "".join("\t".join(map(str, l)) + "\n" for l in lines), skipped, tracks


# ---- the forward pass again, with numpy ---------------------------------------------------------------------------------------
def numpy_viterbi(x, P, unit=UNIT, cap=CAP, lam=LAMBDA):
    """-> (int8 states, minimal end cost): whole-vector steps, the back-pointers as one [T][8] array"""
    x = np.asarray(x, dtype=np.int64)
    T = len(x)
    if T == 0:
        return np.zeros(0, dtype=np.int8), 0
    k = np.arange(STATES, dtype=np.int64)
    e = np.where(x[:, None] < 0, 0, np.minimum(cap, (x[:, None] - unit * k[None, :]) ** 2))
    pen = np.where(k == P, 0, lam)
    V = e[0] + pen
    B = np.zeros((T, STATES), dtype=np.int8)
    for t in range(1, T):
        a = int(np.argmin(V))                         # (the first of equal minima)
        jump = V[a] + lam
        B[t] = np.where(V <= jump, k, a)
        V = e[t] + np.minimum(V, jump)
    end = V + pen
    s = np.zeros(T, dtype=np.int8)
    s[-1] = int(np.argmin(end))
    for t in range(T - 1, 0, -1):
        s[t - 1] = B[t, s[t]]
    return s, int(end.min())


def brute_force_cost(x, P, unit=UNIT, cap=CAP, lam=LAMBDA):
    """T <= 5: the minimum of path_cost over all 8**T paths"""
    T = len(x)
    assert 1 <= T <= 5
    paths = np.stack(np.meshgrid(*[np.arange(STATES)] * T, indexing="ij"), axis=-1).reshape(-1, T).astype(np.int64)
    xs = np.asarray(x, dtype=np.int64)
    e = np.where(xs[None, :] < 0, 0, np.minimum(cap, (xs[None, :] - unit * paths) ** 2)).sum(axis=1)
    jumps = (paths[:, 1:] != paths[:, :-1]).sum(axis=1) + (paths[:, 0] != P) + (paths[:, -1] != P)
    return int((e + lam * jumps).min())


# ---- Viterbi cases ------------------------------------------------------------------------------------------------------------
def track(T, P, segs=(), noise=0, seed=0, masked=()):
    """x of T bins at P copies with (lo, hi, cn) intervals at cn copies, seeded uniform noise of +-noise, (lo, hi) intervals masked"""
    x = np.full(T, P * U, dtype=np.int64)
    for lo, hi, cn in segs:
        x[lo:hi] = cn * U
    if noise:
        x = x + np.random.default_rng(seed).integers(-noise, noise + 1, T)
    x = np.clip(x, 0, 8 * U)
    for lo, hi in masked:
        x[lo:hi] = -1
    return x.astype(np.int32)


def _v(name, family, contigs, **claims):
    return {"name": name, "family": family, "contigs": [(np.asarray(x, dtype=np.int32), int(P)) for x, P in contigs], "claims": claims}


def _viterbi_cases():
    cases = []
    rng = np.random.default_rng(20261018)
    for name, T in (("T=1", 1), ("T=2", 2), ("T=L-1", L - 1), ("T=L", L), ("T=L+1", L + 1), ("T=2L", 2 * L), ("T=2L+1", 2 * L + 1),
                    ("T=300L+1", 300 * L + 1)):
        segs = []
        for _ in range(max(1, T // 97)):
            lo = int(rng.integers(0, T))
            segs.append((lo, min(T, lo + int(rng.integers(1, 40))), int(rng.integers(0, 8))))
        cases.append(_v(name, "size", [(track(T, 2, segs, noise=90, seed=T), 2)], T=T))
    for p in (L - 2, L - 1, L, L + 1):
        cases.append(_v("into a deletion at %d" % p, "seam", [(track(2 * L, 2, [(p, p + 12, 1)]), 2)], change_at=p))
        cases.append(_v("out of a duplication at %d" % p, "seam", [(track(2 * L, 2, [(p - 12, p, 3)]), 2)], change_at=p))
        cases.append(_v("noisy step down at %d" % p, "seam", [(track(2 * L, 3, [(p, 2 * L - 30, 2)], noise=60, seed=p), 3)], change_at=p))
    cases.append(_v("one bin is not a segment", "length", [(track(40, 2, [(20, 21, 1)]), 2)], all_P=True))
    cases.append(_v("five bins are one", "length", [(track(40, 2, [(20, 25, 1)]), 2)], run=(20, 25, 1)))
    cases.append(_v("five bins across the seam", "length", [(track(2 * L, 2, [(L - 2, L + 3, 3)]), 2)], run=(L - 2, L + 3, 3)))
    # four bins cost 4 U^2 to sit out and 2 LAMBDA = 4 U^2 to call: at the bin behind them staying in 2 ties with jumping from 1
    cases.append(_v("stay ties with jump", "tie", [(track(6, 2, [(1, 5, 1)]), 2)], tie=(5, 2), all_P=True))
    cases.append(_v("stay ties with jump at the seam", "tie", [(track(2 * L, 2, [(L - 4, L, 1)]), 2)], tie=(L, 2), all_P=True))
    # states 1 and 2 are equally far from 1.5 copies: the run is called at the LOWEST of the equal minima
    cases.append(_v("midway between two states", "argmin", [(track(30, 4, [(5, 15, 1)]) + np.where((np.arange(30) >= 5) & (np.arange(30) < 15), U // 2, 0), 4)],
                    run=(5, 15, 1), midway=(5, 15)))
    cases.append(_v("midway, staying put", "argmin", [(np.full(50, U + U // 2, dtype=np.int32), 2)], all_P=True, midway=(0, 50)))
    # three low bins at the end: 3 U^2 to sit out, one jump AND the end penalty (4 U^2) to call
    cases.append(_v("three bins at the end", "contig_end", [(track(30, 2, [(27, 30, 1)]), 2)], all_P=True))
    cases.append(_v("three bins at the start", "contig_end", [(track(30, 2, [(0, 3, 3)]), 2)], all_P=True))
    cases.append(_v("five bins at the end", "contig_end", [(track(30, 2, [(25, 30, 1)]), 2)], run=(25, 30, 1)))
    cases.append(_v("five bins at the end of a chunk's last contig bin", "contig_end", [(track(L, 2, [(L - 5, L, 3)]), 2)], run=(L - 5, L, 3)))
    m = [(L - 5, L + 5)]
    cases.append(_v("masked run across the seam inside a deletion", "masked", [(track(2 * L, 2, [(L - 20, L + 20, 1)], masked=m), 2)],
                    run=(L - 20, L + 20, 1)))
    cases.append(_v("masked run across the seam", "masked", [(track(2 * L, 2, noise=50, seed=5, masked=m), 2)], all_P=True))
    cases.append(_v("a masked run keeps two halves together", "masked", [(track(60, 2, [(19, 22, 1), (32, 35, 1)], masked=[(22, 32)]), 2)],
                    run=(19, 35, 1)))
    cases.append(_v("masked at both ends", "masked", [(track(L + 9, 2, [(0, 12, 1), (L, L + 9, 3)], masked=[(0, 6), (L + 4, L + 9)]), 2)],
                    run=(0, 12, 1)))
    cases.append(_v("all masked", "masked", [(np.full(L + 3, -1, dtype=np.int32), 3)], all_P=True))
    cases.append(_v("all masked, one bin", "masked", [(np.full(1, -1, dtype=np.int32), 1)], all_P=True))
    # one bin at 8 copies: the cap makes it 4 U^2 to sit out, 4 U^2 + U^2 to visit state 7; uncapped it would be 36 U^2
    cases.append(_v("the cap lets an outlier pass", "cap", [(track(20, 2, [(10, 11, 8)]), 2)], all_P=True, capped_at=10))
    x = track(24, 2)
    x[8], x[12], x[16] = 2 * U + 2 * U - 1, 2 * U + 2 * U, 2 * U + 2 * U + 1
    cases.append(_v("the cap missed by one, reached, passed", "cap", [(x, 2)], all_P=True, cap_edges=(8, 12, 16)))
    x = track(40, 2, [(10, 30, 4)])
    x[10:30] -= 1
    cases.append(_v("a run one short of the cap away", "cap", [(x, 2)], run=(10, 30, 4)))
    cases.append(_v("70 000 bins at 8 copies", "int64", [(np.full(70000, 8 * U, dtype=np.int32), 2)], cost_above=2 ** 31, run=(0, 70000, 7)))
    six = [(track(0, 2), 2), (track(1, 1, [(0, 1, 0)]), 1), (track(L, 2, [(L - 6, L, 3)], noise=40, seed=1), 2),
           (track(L + 1, 3, [(L - 3, L + 1, 1)], noise=40, seed=2), 3), (track(3, 6, [(1, 2, 7)]), 6),
           (track(2 * L, 4, [(100, 140, 2), (L - 1, L + 6, 5)], noise=40, seed=3), 4)]
    cases.append(_v("six contigs", "multi", six))
    cases.append(_v("six contigs, another order", "multi", [six[i] for i in (5, 3, 0, 4, 2, 1)]))
    for P in range(0, 8):
        cases.append(_v("ploidy %d" % P, "ploidy", [(track(70, P, [(10, 20, (P + 1) % 8), (40, 52, (P + 7) % 8)], noise=30, seed=P), P)]))
    for i in range(6):
        T = int(rng.integers(1, 6))
        cases.append(_v("tiny %d" % i, "tiny", [(rng.integers(-1, 8 * U + 1, T).astype(np.int32), int(rng.integers(1, 7)))]))
    return cases


VITERBI_CASES = _viterbi_cases()


@functools.lru_cache(maxsize=None)
def _viterbi_reference(index):
    out = []
    for x, P in VITERBI_CASES[index]["contigs"]:
        d = {}
        s = ref_viterbi([int(v) for v in x], P, details=d) if len(x) else []
        out.append((np.asarray(s, dtype=np.int8), d.get("cost", 0), d.get("ties", [])))
    return out


def viterbi_reference(case):
    """[(int8 states, cost, ties)] per contig of the case: computed once, shared, read-only"""
    out = _viterbi_reference(next(i for i, c in enumerate(VITERBI_CASES) if c is case))
    for s, _, _ in out:
        s.setflags(write=False)
    return out


def viterbi_arrays(case):
    """-> (int32 x of all contigs, int64[nseg][3] {toff, T, P})"""
    xs = [x for x, _ in case["contigs"]]
    table, at = [], 0
    for x, P in case["contigs"]:
        table.append((at, len(x), P))
        at += len(x)
    return (np.concatenate(xs) if xs else np.zeros(0, dtype=np.int32)).astype(np.int32), np.array(table, dtype=np.int64).reshape(-1, 3)


# ---- bins cases ---------------------------------------------------------------------------------------------------------------
def _b(name, family, contigs, unit=UNIT):
    """contigs: (cov, gc, K, P, E[101])"""
    return {"name": name, "family": family, "unit": unit,
            "contigs": [(np.asarray(c, dtype=np.float64), np.asarray(g, dtype=np.int8), int(K), int(P), np.asarray(E, dtype=np.float64)) for c, g, K, P, E in contigs]}


def _random_contig(rng, nb, K, P, masked=0.2):
    E = rng.uniform(20, 40, 101)
    gc = rng.integers(0, 101, nb)
    gc[rng.random(nb) < masked] = -1
    cov = rng.uniform(0, 2, nb) * E[np.maximum(gc, 0)] * rng.choice([0.5, 1.0, 1.0, 1.5], nb)
    cov[rng.random(nb) < 0.05] = 0.0
    return cov, gc, K, P, E


def _bins_cases():
    rng = np.random.default_rng(5)
    cases = []
    for K, nb in ((1, 333), (2, 1001), (10, 2507), (64, 64 * 9 + 1), (64, 63), (7, 5)):
        cases.append(_b("K=%d nb=%d" % (K, nb), "size", [_random_contig(rng, nb, K, 2)]))
    cases.append(_b("P = 1 .. 6 in one call", "ploidy", [_random_contig(rng, 400 + 13 * P, 3 + P, P) for P in range(1, 7)]))
    one = np.ones(101)
    # exactly half of a bin usable (kept) and one fewer (masked), the masked bins at either end of the CNV bin
    for K in (1, 2, 10, 64):
        rows = []
        for n in sorted({K // 2 + 1, (K + 1) // 2, (K + 1) // 2 - 1, K, 0}):
            if n < 0:
                continue
            rows.append([0] * n + [-1] * (K - n))
            rows.append([-1] * (K - n) + [0] * n)
        gc = np.array(sum(rows, []))
        cases.append(_b("half usable, K=%d" % K, "mask_threshold", [(np.full(len(gc), 1.0), gc, K, 2, one)]))
    # the last CNV bin is short: its threshold is still K
    cases.append(_b("short last bin", "mask_threshold", [(np.full(25, 1.0), np.zeros(25), 10, 2, one), (np.full(24, 1.0), np.zeros(24), 10, 2, one),
                                                        (np.full(23, 1.0), np.array([0] * 18 + [-1, -1, 0, 0, 0]), 6, 2, one)]))
    # obs = (2^53 + 1) + 1 = 2^53 left to right, 2^53 + (1 + 1) pairwise; exp = 2^62 either way: the ratio times UNIT is 0.5 or just above
    E = np.ones(101)
    E[10], E[11], E[12] = 2.0 ** 61, 2.0 ** 60, 2.0 ** 60
    cases.append(_b("2^53, 1, 1", "sum_order", [(np.array([2.0 ** 53, 1.0, 1.0]), np.array([10, 11, 12]), 3, 1, E),
                                                (np.array([1.0, 1.0, 2.0 ** 53]), np.array([11, 12, 10]), 3, 1, E)]))
    # (n + 0.5) / UNIT / P is exact for P = 1, 2, 4: the product is the tie n + 0.5 itself
    for P in (1, 2, 4):
        n = np.arange(0, 40)
        cases.append(_b("rint ties, P=%d" % P, "rint_tie", [((n + 0.5) / U / P, np.zeros(len(n)), 1, P, one)]))
    cases.append(_b("the clamp at 8 UNIT", "clamp", [(np.array([8.0, 8.0 - 1.0 / U, 8.0 + 1.0 / U, 1e300, 7.998, 9.0, 0.0]) / 2, np.zeros(7), 1, 2, one)]))
    cases.append(_b("another unit", "unit", [_random_contig(rng, 300, 4, 3)], unit=1000))
    return cases


BINS_CASES = _bins_cases()


@functools.lru_cache(maxsize=None)
def _bins_reference(index):
    case = BINS_CASES[index]
    return tuple(np.asarray(ref_bins(cov, gc, K, P, E, unit=case["unit"]), dtype=np.int32) for cov, gc, K, P, E in case["contigs"])


def bins_reference(case):
    out = _bins_reference(next(i for i, c in enumerate(BINS_CASES) if c is case))
    for a in out:
        a.setflags(write=False)
    return out


def bins_arrays(case):
    """-> (cov, gc, int64[nseg][5] {off, nb, K, P, toff}, E[nseg][101])"""
    table, off, toff = [], 0, 0
    for cov, gc, K, P, E in case["contigs"]:
        table.append((off, len(cov), K, P, toff))
        off += len(cov)
        toff += -(-len(cov) // K)
    return (np.concatenate([c[0] for c in case["contigs"]]), np.concatenate([c[1] for c in case["contigs"]]),
            np.array(table, dtype=np.int64), np.stack([c[4] for c in case["contigs"]]))


# ---- a whole job on made-up bins ----------------------------------------------------------------------------------------------
PLANTED = {"seed": 7, "nb": 40000, "depth": 30.0, "W": 500, "del": (10000, 12000), "dup": (25000, 26500)}


@functools.lru_cache(maxsize=None)
def planted_job():
    """one contig 'chrA' of seeded Poisson depth with a half-depth and a 1.5x interval, beside contigs that exercise the class
    fallback on both sides of MIN_CLASS and every reason to skip a contig -> the arguments of tiddit_cnv.main (without prefix)"""
    p = PLANTED
    rng = np.random.default_rng(p["seed"])
    nb = p["nb"]
    gc = rng.integers(35, 56, nb).astype(np.int8)
    scale = np.ones(nb)
    scale[p["del"][0]:p["del"][1]] = 0.5
    scale[p["dup"][0]:p["dup"][1]] = 1.5
    bias = 1.0 + (gc - 45) * 0.01
    cov = rng.poisson(p["depth"] * 50 * scale * bias).astype(np.float64) / 50.0
    gc[3000:3100] = -1
    # chrC: classes 60 / 61 / 62 hold 101 / 100 / 99 covered bins at twice the depth, and uncovered ones that do not count: the first
    # two are their own yardstick (no segment), the 99 fall back to C and read as four copies
    nc = 3000
    gc_c = rng.integers(40, 50, nc).astype(np.int8)
    cov_c = rng.poisson(p["depth"] * 50, nc).astype(np.float64) / 50.0
    at = 500
    for g, n in ((60, 101), (61, 100), (62, 99)):
        gc_c[at:at + n] = g
        cov_c[at:at + n] = 2 * p["depth"] + rng.integers(0, 5, n)
        gc_c[at + n:at + n + 3] = g
        cov_c[at + n:at + n + 3] = 0.0
        at += 800
    coverage = {"chrA": cov, "chrC": cov_c, "chrB": rng.poisson(p["depth"], 900).astype(np.float64), "tiny": np.full(100, 30.0), "empty": np.zeros(600),
                "odd": np.full(500, 30.0), "none": np.zeros(0)}
    coverage["chrB"][400:480] = 0.0
    gcs = {"chrA": gc, "chrC": gc_c, "chrB": rng.integers(40, 50, 905).astype(np.int8), "tiny": np.full(100, 40, dtype=np.int8),
           "empty": np.full(600, 40, dtype=np.int8), "odd": np.full(500, 40, dtype=np.int8), "none": np.zeros(0, dtype=np.int8),
           "absent": np.zeros(10, dtype=np.int8)}
    contigs = ["chrA", "absent", "chrB", "chrC", "tiny", "empty", "odd", "none"]
    length = {"chrA": nb * 50 - 20, "chrC": nc * 50, "absent": 500000, "chrB": 900 * 50, "tiny": 5000, "empty": 30000, "odd": 25000, "none": 20000}
    library = {"contig_ploidy_chrA": 2, "contig_ploidy_chrC": 2, "contig_ploidy_chrB": 1, "contig_ploidy_tiny": 2, "contig_ploidy_empty": 2, "contig_ploidy_odd": 7,
               "contig_ploidy_none": 2}
    return coverage, gcs, library, contigs, length, 10000, p["W"]
