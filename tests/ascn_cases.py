"""Cases and references for the allele-specific copy number of ``tiddit --sv`` (``TIDDIT_ASCN``, tiddit_amd/tiddit_ascn.py,
csrc/tdt_ascn.hip).

References, none of which shares code with the product:
  * the literal definition of tiddit_ascn.py's docstring as plain Python loops over sites, bins and states (``ref_emissions``,
    ``ref_viterbi``, ``ref_segments``); their ``mutant`` argument switches ONE line to a plausible wrong reading, for
    tests/test_ascn_refs_cpu.py to show that the cases tell the readings apart;
  * a dense numpy restatement of the chain: every step a full 16 x 16 (min,+) product (``dense_viterbi``);
  * for ``T <= 4`` the optimal cost by enumeration of all ``16**T`` paths (``brute_force_cost``).
Every case is built from literals or a seeded generator."""
import functools
import os
import re

import numpy as np

import cnv_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r"^#define\s+H16_CHUNK\s+(\d+)", open(os.path.join(REPO, "tiddit_amd", "csrc", "tdt_ascn.hip")).read(), re.M).group(1))
L = CHUNK
UNIT = 256
CAP = 4 * UNIT * UNIT
LAMBDA = 2 * UNIT * UNIT
BU = 512
ACAP = 65536
HOM = 4096
MIN_N = 8
S = 16
CM = [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (4, 0), (4, 1), (4, 2), (5, 0), (5, 1), (5, 2), (6, 0), (6, 1), (6, 2), (6, 3)]
MU_OF = [0, 0, 0, 256, 0, 170, 0, 128, 256, 0, 102, 204, 0, 85, 170, 256]
HEADER = "#chrom\tstart\tend\ttype\tCN\tminorCN\tbins\tsites\tmeanCN\tmeanBAF\n"
BIG = 1 << 61
MUTANTS = {"bp_lt": "tie", "argmin_high": "argmin", "no_hom": "floor", "beta_round": "floor", "bin_edge": "edges", "min_n": "min_n"}


# ---- the literal definition ---------------------------------------------------------------------------------------------------
def ref_emissions(x, W, pos, ref_n, alt_n, mutant=None):
    """ONE contig -> (E [T][16], nsite [T], sum_beta [T]) as Python lists"""
    T = len(x)
    E, nsite, sum_beta = [], [0] * T, [0] * T
    for t in range(T):
        E.append([0 if x[t] < 0 else min(CAP, (int(x[t]) - UNIT * c) ** 2) for c, m in CM])
    for p, r, a in zip(pos, ref_n, alt_n):
        p, r, a = int(p), int(r), int(a)
        t = (p + 1) // W if mutant == "bin_edge" else p // W
        if t >= T:
            continue
        n = r + a
        if (n <= MIN_N) if mutant == "min_n" else (n < MIN_N):
            continue
        beta = (2 * min(r, a) * BU + n) // (2 * n) if mutant == "beta_round" else (min(r, a) * BU) // n
        h = min(ACAP, beta * beta)
        nsite[t] += 1
        sum_beta[t] += beta
        for k in range(S):
            if CM[k][1] == 0:
                g = h
            else:
                g = min(min(ACAP, (beta - MU_OF[k]) ** 2), h + (0 if mutant == "no_hom" else HOM))
            E[t][k] += g
    return E, nsite, sum_beta


def ref_viterbi(E, home, lam=LAMBDA, mutant=None, details=None):
    """the states of ONE contig -> list of s_t.  details (a dict): 'cost' = the minimal end cost, 'ties' = the (t, k) with
    V_{t-1}(k) == m + lam exactly, 'args' = the set of a that a jump on the path used."""
    T = len(E)
    if T == 0:
        return []
    V = [int(E[0][k]) + (0 if k == home else lam) for k in range(S)]
    B, A, ties = [None], [None], []
    for t in range(1, T):
        m = min(V)
        hits = [i for i in range(S) if V[i] == m]
        a = hits[-1] if mutant == "argmin_high" else hits[0]
        nV, b = [], []
        for k in range(S):
            if V[k] == m + lam:
                ties.append((t, k))
            stay = (V[k] < m + lam) if mutant == "bp_lt" else (V[k] <= m + lam)
            b.append(k if stay else a)
            nV.append(int(E[t][k]) + min(V[k], m + lam))
        V = nV
        B.append(b)
        A.append(a)
    end = [V[k] + (0 if k == home else lam) for k in range(S)]
    best = min(end)
    hits = [k for k in range(S) if end[k] == best]
    s = [0] * T
    s[T - 1] = hits[-1] if mutant == "argmin_high" else hits[0]
    used = set()
    for t in range(T - 1, 0, -1):
        s[t - 1] = B[t][s[t]]
        if s[t - 1] != s[t]:
            used.add(A[t])
    if details is not None:
        details.update(cost=best, ties=ties, args=used)
    return s


def path_cost(E, home, s, lam=LAMBDA):
    c = 0 if s[0] == home else lam
    for t in range(len(E)):
        c += int(E[t][s[t]])
        if t and s[t] != s[t - 1]:
            c += lam
    return c + (0 if s[-1] == home else lam)


def ref_segments(s, x, nsite, sum_beta, P, W, length, chrom):
    home = CM.index((P, P // 2))
    T, out, t = len(s), [], 0
    while t < T:
        e = t
        while e + 1 < T and s[e + 1] == s[t]:
            e += 1
        if s[t] != home:
            first, last = t, e
            while first <= last and x[first] < 0 and nsite[first] == 0:
                first += 1
            while last >= first and x[last] < 0 and nsite[last] == 0:
                last -= 1
            if first <= last:
                c, m = CM[s[t]]
                seen = [int(x[i]) for i in range(first, last + 1) if x[i] >= 0]
                ns, sb = sum(nsite[first:last + 1]), sum(sum_beta[first:last + 1])
                kind = "DEL" if c < P else "DUP" if c > P else "LOH" if m == 0 else "AI"
                out.append((chrom, first * W, min((last + 1) * W, length), kind, c, m, len(seen), ns,
                            "{:.3f}".format(sum(seen) / (len(seen) * UNIT)) if seen else ".", "{:.3f}".format(sb / (ns * BU)) if ns else "."))
        t = e + 1
    return out


def text_of(segments):
    return HEADER + "".join("\t".join(map(str, l)) + "\n" for l in segments)


# ---- the chain again: dense (min,+) products ----------------------------------------------------------------------------------
def dense_viterbi(E, home, lam=LAMBDA):
    """-> (int8 states, minimal end cost): V_t = min_i (V_{t-1}(i) + M[i][k]) + E_t(k) over the full 16 x 16 jump matrix, the
    back-pointer the diagonal where it attains the minimum, else the first argmin of the column"""
    E = np.asarray(E, dtype=np.int64).reshape(-1, S)
    T = len(E)
    if T == 0:
        return np.zeros(0, dtype=np.int8), 0
    M = np.where(np.eye(S, dtype=bool), 0, lam).astype(np.int64)
    pen = np.where(np.arange(S) == home, 0, lam)
    V = E[0] + pen
    B = np.zeros((T, S), dtype=np.int8)
    d = np.arange(S)
    for t in range(1, T):
        C = V[:, None] + M                            # C[i][k]: in i before, in k now
        best = C.min(axis=0)
        off = np.where(np.eye(S, dtype=bool), BIG, C)
        B[t] = np.where(C[d, d] == best, d, off.argmin(axis=0))
        V = E[t] + best
    end = V + pen
    s = np.zeros(T, dtype=np.int8)
    s[-1] = int(np.argmin(end))
    for t in range(T - 1, 0, -1):
        s[t - 1] = B[t, s[t]]
    return s, int(end.min())


def brute_force_cost(E, home, lam=LAMBDA):
    """T <= 4: the minimum of path_cost over all 16**T paths"""
    E = np.asarray(E, dtype=np.int64).reshape(-1, S)
    T = len(E)
    assert 1 <= T <= 4
    paths = np.stack(np.meshgrid(*[np.arange(S)] * T, indexing="ij"), axis=-1).reshape(-1, T)
    e = E[np.arange(T)[None, :], paths].sum(axis=1)
    jumps = (paths[:, 1:] != paths[:, :-1]).sum(axis=1) + (paths[:, 0] != home) + (paths[:, -1] != home)
    return int((e + lam * jumps).min())


# ---- Viterbi cases ------------------------------------------------------------------------------------------------------------
def chain(T, home, segs=(), seed=0, noise=60000, off=(20000, 120000)):
    """emissions of T bins whose cheapest state is home, or st inside the (lo, hi, st) intervals: seeded noise on every cell, a seeded
    surcharge on every state but the cheapest"""
    rng = np.random.default_rng(seed)
    truth = np.full(T, home)
    for lo, hi, st in segs:
        truth[lo:hi] = st
    E = rng.integers(0, noise + 1, (T, S)) + rng.integers(off[0], off[1] + 1, (T, S))
    E[np.arange(T), truth] = rng.integers(0, noise + 1, T)
    return E.astype(np.int32)


def _v(name, family, contigs, lam=LAMBDA, **claims):
    return {"name": name, "family": family, "lam": lam, "contigs": [(np.asarray(E, dtype=np.int32).reshape(-1, S), int(h)) for E, h in contigs],
            "claims": claims}


def _viterbi_cases():
    cases = []
    rng = np.random.default_rng(20261018)
    for T in (1, 2, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 65 * L + 1):
        segs = []
        for _ in range(max(1, T // 97)):
            lo = int(rng.integers(0, T))
            segs.append((lo, min(T, lo + int(rng.integers(1, 40))), int(rng.integers(0, S))))
        cases.append(_v("T=%d" % T, "size", [(chain(T, 3, segs, seed=T), 3)], T=T))
    nine = [(chain(int(T), int(h), [(int(T) // 3, int(T) // 3 + 9, (int(h) + 5) % S)], seed=100 + i), int(h))
            for i, (T, h) in enumerate(((0, 3), (1, 1), (L, 3), (1, 8), (L + 1, 5), (3, 15), (2 * L, 8), (1, 0), (40, 3)))]
    cases.append(_v("nine contigs", "multi", nine))
    cases.append(_v("nine contigs, another order", "multi", [nine[i] for i in (8, 3, 0, 6, 1, 7, 2, 5, 4)]))
    many = []
    for i in range(300):
        T = 1 if i % 3 else int(rng.integers(0, 70))
        if i == 150:
            T = L + 2
        h = int(rng.integers(0, S))
        many.append((chain(T, h, [(T // 2, T // 2 + 6, (h + 1) % S)], seed=1000 + i), h))
    cases.append(_v("300 contigs", "multi", many))
    cases.append(_v("every state as home", "home", [(chain(70, h, [(10, 20, (h + 1) % S), (40, 52, (h + 9) % S)], seed=h), h) for h in range(S)]))
    cases.append(_v("all-zero emissions", "tie", [(np.zeros((T, S)), h) for T, h in ((1, 0), (2, 3), (L + 5, 15), (40, 8))], all_home=True))
    # V_0(k) = LAMBDA = V_0(home) + LAMBDA for every k: at t = 1 staying in k ties with jumping from home, and from t = 1 on only k is free
    for k, h in ((0, 3), (15, 3), (3, 8)):
        E = np.full((12, S), 3 * LAMBDA)
        E[0] = 0
        E[1:, k] = 0
        cases.append(_v("stay ties with jump, state %d" % k, "tie", [(E, h)], tie=(1, k), path=[k] * 12))
    # ... the same tie at the first bin of a chunk: L bins in which every state costs the same, then only k is free
    E = np.zeros((L + 8, S))
    E[L:] = 3 * LAMBDA
    E[L:, 6] = 0
    cases.append(_v("stay ties with jump at the seam", "tie", [(E, 3)], tie=(L, 6), path=[6] * (L + 8)))
    # two states equally cheap, then a jump away from them to home: the back-pointer is the LOWEST of the equal minima
    for a in range(S):
        b, c = (a + 1) % S, (a + 7) % S
        E = np.full((2 * L + 20, S), 5 * LAMBDA)
        p = L - 1 if a % 2 else L                      # the jump on the last bin of a chunk, or on the first bin of the next
        E[:p, a] = 0
        E[:p, b] = 0
        E[p:, c] = 0
        cases.append(_v("argmin %d, jump at %d" % (a, p), "argmin", [(E, c)], jump_at=p, arg=min(a, b), path=[min(a, b)] * p + [c] * (2 * L + 20 - p)))
    cases.append(_v("lambda 0", "lambda", [(chain(2 * L + 3, 3, [(100, 130, 7)], seed=77), 3), (chain(5, 0, seed=78), 0)], lam=0))
    cases.append(_v("lambda 2^28", "lambda", [(chain(2 * L + 3, 3, [(100, 130, 7)], seed=79, noise=1 << 27, off=(1 << 26, 1 << 27)), 3),
                                              (chain(700, 8, [(L - 5, L + 300, 2)], seed=80, noise=1 << 27, off=(1 << 26, 1 << 27)), 8)], lam=1 << 28))
    E = np.full((4096, S), 1 << 28)
    E[np.arange(4096), np.where((np.arange(4096) // 700) % 2, 11, 3)] -= rng.integers(0, 1 << 20, 4096)
    cases.append(_v("emissions of 2^28 over 4096 bins", "int64", [(E, 3)], cost_above=1 << 39))
    for i in range(6):
        T = int(rng.integers(1, 5))
        cases.append(_v("tiny %d" % i, "tiny", [(rng.integers(0, 3 * LAMBDA, (T, S)), int(rng.integers(0, S)))]))
        cases.append(_v("tiny %d, small steps" % i, "tiny", [(rng.integers(0, 4, (T, S)) * (LAMBDA // 2), int(rng.integers(0, S)))]))
    return cases


VITERBI_CASES = _viterbi_cases()


@functools.lru_cache(maxsize=None)
def _viterbi_reference(index):
    case = VITERBI_CASES[index]
    out = []
    for E, home in case["contigs"]:
        d = {}
        s = ref_viterbi(E.tolist(), home, case["lam"], details=d) if len(E) else []
        out.append((np.asarray(s, dtype=np.int8), d.get("cost", 0), d.get("ties", []), d.get("args", set())))
    return out


def viterbi_reference(case):
    """[(int8 states, cost, ties, args)] per contig of the case: computed once, shared, read-only"""
    out = _viterbi_reference(next(i for i, c in enumerate(VITERBI_CASES) if c is case))
    for r in out:
        r[0].setflags(write=False)
    return out


def viterbi_arrays(case):
    """-> (int32 E[n][16] of all contigs, int64[nseg][3] {toff, T, home})"""
    table, at = [], 0
    for E, home in case["contigs"]:
        table.append((at, len(E), home))
        at += len(E)
    return np.ascontiguousarray(np.concatenate([E for E, _ in case["contigs"]]), dtype=np.int32), np.array(table, dtype=np.int64).reshape(-1, 3)


# ---- emissions cases ----------------------------------------------------------------------------------------------------------
def _contig(x, W, pos=(), ref_n=(), alt_n=(), cols=None, rest=None, processed=True, seed=0):
    """one contig of an emissions case: its sites' positions and REF / ALT counters; cols: the (REF, ALT) counter columns of every site
    (default 0, 1); the six other counters of a site's row are seeded noise"""
    n = len(pos)
    cols = np.tile([0, 1], (n, 1)) if cols is None else np.asarray(cols).reshape(n, 2)
    counts = np.random.default_rng(seed).integers(0, 1 << 32, (n, 8), dtype=np.uint64)
    counts[np.arange(n), cols[:, 0]] = np.asarray(ref_n, dtype=np.uint64)
    counts[np.arange(n), cols[:, 1]] = np.asarray(alt_n, dtype=np.uint64)
    return {"x": np.asarray(x, dtype=np.int32), "W": int(W), "pos": np.asarray(pos, dtype=np.int32), "ref_n": [int(v) for v in ref_n],
            "alt_n": [int(v) for v in alt_n], "cols": cols.astype(np.uint8), "counts": counts.astype(np.uint32), "processed": processed}


def _e(name, family, contigs):
    return {"name": name, "family": family, "contigs": contigs}


def _emissions_cases():
    rng = np.random.default_rng(11)
    cases = []
    # sites at tW - 1, tW, tW + 1 and on the last base of a contig whose last bin is short; every site tells its bin by its own counters
    W, length = 500, 1730
    pos = sorted({t * W + d for t in (1, 2, 3) for d in (-1, 0, 1)} | {0, length - 1})
    cases.append(_e("bin edges, short last bin", "edges", [_contig([300, 512, 200, 770], W, pos, [20 + 3 * i for i in range(len(pos))],
                                                                   [9 + 5 * i for i in range(len(pos))]),
                                                           _contig([256, 256], 50, [48, 49, 50, 51, 99], [9, 8, 30, 4, 11], [1, 8, 10, 40, 11])]))
    # no site, one site, and a site on every base of the largest bin, every one at the largest score of the states without a minor copy
    W = 3200
    pos = [W + 7] + list(range(2 * W, 3 * W))
    cases.append(_e("0, 1 and 3200 sites at the largest scores", "load", [_contig([8 * UNIT, 8 * UNIT, 8 * UNIT], W, pos, [50] * len(pos), [50] * len(pos))]))
    pairs = [(3, 4), (4, 3), (4, 4), (7, 0), (0, 7), (8, 0), (0, 8), (7, 1), (0, 0), (5, 3)]
    cases.append(_e("n = MIN_N - 1 and MIN_N", "min_n", [_contig([256] * 2, 500, [10 + 30 * i for i in range(len(pairs))], [p[0] for p in pairs],
                                                                 [p[1] for p in pairs])]))
    top = (1 << 32) - 1
    pairs = [(top, top), (top, 0), (0, top), (top, 1), (1, top), (top, top - 1), (top // 3, top), (top, top // 2), (12, 12), (30, 0)]
    cases.append(_e("ref_n == alt_n, alt_n == 0, counters of 2^32 - 1", "wide", [_contig([512] * 3, 100, [5 + 25 * i for i in range(len(pairs))],
                                                                                          [p[0] for p in pairs], [p[1] for p in pairs])]))
    # every (ref_n, alt_n) with n <= 64: beta on both sides of each floor step
    pairs = [(r, n - r) for n in range(0, 65) for r in range(n + 1)]
    cases.append(_e("every pair with n <= 64", "floor", [_contig(rng.integers(0, 7 * UNIT, -(-len(pairs) // 50)), 50, np.arange(len(pairs)),
                                                                 [p[0] for p in pairs], [p[1] for p in pairs])]))
    cols = [(r, a) for r in range(4) for a in range(4) if r != a]
    cases.append(_e("all 12 (REF, ALT) column pairs", "columns", [_contig([600, 100], 1000, [50 + 150 * i for i in range(12)],
                                                                          [10 + i for i in range(12)], [30 - 2 * i for i in range(12)], cols=cols)]))
    a = _contig([256, 300, 512], 500, [3, 700, 701, 1400], [10, 20, 5, 9], [12, 0, 5, 30], seed=1)
    b = _contig([256] * 4, 500, [1, 2, 600], [10, 10, 10], [10, 10, 10], processed=False, seed=2)
    c = _contig([100, 900], 500, seed=3)
    d = _contig([256], 3200, [0, 3199], [40, 22], [2, 21], seed=4)
    cases.append(_e("contigs without sites, sites of unprocessed contigs", "contigs", [a, b, c, d, dict(b), dict(c)]))
    cases.append(_e("nothing but unprocessed contigs in front", "contigs", [b, dict(b), d]))
    cases.append(_e("masked bins with and without sites", "masked", [_contig([-1, -1, 256, -1], 500, [10, 20, 1100, 1600], [9, 3, 10, 40], [9, 3, 12, 0])]))
    # a site past the last bin of its contig counts nowhere
    cases.append(_e("a site behind the last bin", "edges", [_contig([256, 256], 500, [999, 1000, 1200], [10, 11, 12], [10, 11, 12])]))
    nb = 700
    pos = np.sort(rng.choice(nb * 500, 900, replace=False))
    depth = rng.poisson(30, len(pos))
    alt = rng.binomial(depth, rng.choice([0.0, 0.5, 1.0, 0.33, 0.25], len(pos)))
    cases.append(_e("700 bins of seeded sites", "size", [_contig(rng.integers(-1, 8 * UNIT, nb), 500, pos, depth - alt, alt,
                                                                 cols=[cols[i] for i in rng.integers(0, 12, len(pos))])]))
    return cases


EMISSIONS_CASES = _emissions_cases()


def emissions_arrays(case):
    """-> (counts uint32[sites][8], site_pos, cols uint8[sites][2], x, int64[nseg][5] {site_lo, site_hi, toff, T, W}): the sites of every
    contig, the bins and the rows of the processed ones"""
    cs = case["contigs"]
    table, at, toff = [], 0, 0
    for c in cs:
        if c["processed"]:
            table.append((at, at + len(c["pos"]), toff, len(c["x"]), c["W"]))
            toff += len(c["x"])
        at += len(c["pos"])
    used = [c for c in cs if c["processed"]]
    return (np.concatenate([c["counts"] for c in cs]).reshape(-1, 8), np.concatenate([c["pos"] for c in cs]).astype(np.int32),
            np.concatenate([c["cols"] for c in cs]).reshape(-1, 2), np.concatenate([c["x"] for c in used]).astype(np.int32),
            np.array(table, dtype=np.int64).reshape(-1, 5))


@functools.lru_cache(maxsize=None)
def _emissions_reference(index, mutant=None):
    E, ns, sb = [], [], []
    for c in EMISSIONS_CASES[index]["contigs"]:
        if c["processed"]:
            e, n, b = ref_emissions(c["x"].tolist(), c["W"], c["pos"].tolist(), c["ref_n"], c["alt_n"], mutant=mutant)
            E += e
            ns += n
            sb += b
    return np.array(E, dtype=np.int64).reshape(-1, S), np.array(ns, dtype=np.int64), np.array(sb, dtype=np.int64)


def emissions_reference(case, mutant=None):
    """(E int64[total][16], nsite, sum_beta): computed once, shared, read-only"""
    out = _emissions_reference(next(i for i, c in enumerate(EMISSIONS_CASES) if c is case), mutant)
    for a in out:
        a.setflags(write=False)
    return out


# ---- a whole stage on made-up bins and counters -------------------------------------------------------------------------------
PLANTED = {"seed": 3, "nb": 20000, "depth": 30.0, "W": 500, "per_copy": 15, "het": 0.3, "site_every": 1000,
           "plants": (("LOH", 2, 0, 200, 700), ("DEL", 1, 0, 1000, 1060), ("DUP", 3, 1, 1400, 1500))}


class PlantedSites:
    """what tiddit_ascn.main reads of a tiddit_alleles.Sites"""

    def __init__(self, rows, site_pos, site_off):
        self.rows, self.site_pos, self.site_off = rows, site_pos, site_off

    def __len__(self):
        return len(self.site_pos)


@functools.lru_cache(maxsize=None)
def planted_job():
    """'chrA' at two copies with three planted intervals — a copy-neutral LOH, a one-copy deletion, a 2+1 duplication — in seeded
    Poisson depth (the bins of tests/cnv_cases.py's kind) and seeded allele counters at one site per kb, 30 % of them het; 'chrH' at
    one copy with sites, 'chrN' processed without a site, 'tiny' skipped with sites -> (the arguments of tiddit_cnv.bins_stage, the
    counter table, the sites, contig_number)"""
    p = PLANTED
    rng = np.random.default_rng(p["seed"])
    nb, W = p["nb"], p["W"]
    K = W // 50
    gc = rng.integers(35, 56, nb).astype(np.int8)
    copies, minor = np.full(nb // K, 2), np.full(nb // K, 1)
    for _, c, m, lo, hi in p["plants"]:
        copies[lo:hi], minor[lo:hi] = c, m
    bias = 1.0 + (gc - 45) * 0.01
    cov = rng.poisson(p["depth"] * 50 * np.repeat(copies, K) / 2.0 * bias).astype(np.float64) / 50.0
    gc[3000:3100] = -1
    nh = 4000
    coverage = {"chrA": cov, "chrH": rng.poisson(p["depth"] * 25, nh).astype(np.float64) / 50.0, "chrN": rng.poisson(p["depth"] * 50, 1200).astype(np.float64) / 50.0,
                "tiny": np.full(100, 30.0)}
    gcs = {"chrA": gc, "chrH": rng.integers(40, 50, nh).astype(np.int8), "chrN": rng.integers(40, 50, 1200).astype(np.int8), "tiny": np.full(100, 40, dtype=np.int8)}
    contigs = ["tiny", "chrA", "chrN", "chrH"]
    length = {"chrA": nb * 50 - 20, "chrH": nh * 50, "chrN": 1200 * 50, "tiny": 5000}
    library = {"contig_ploidy_chrA": 2, "contig_ploidy_chrH": 1, "contig_ploidy_chrN": 2, "contig_ploidy_tiny": 2}
    rows, site_pos, site_off, table = [], [], [0], []
    for name in contigs:
        n_here = 0
        if name != "chrN":
            for pos in range(p["site_every"] // 2, length[name], p["site_every"]):
                t = pos // W
                c, m = (int(copies[t]), int(minor[t])) if name == "chrA" else (1, 0) if name == "chrH" else (2, 1)
                depth = int(rng.poisson(p["per_copy"] * c))
                if m and rng.random() < p["het"]:
                    alt = int(rng.binomial(depth, (m if rng.random() < 0.5 else c - m) / c))
                else:
                    alt = 0 if rng.random() < 0.5 else depth
                ref, altb = [("A", "C"), ("G", "T"), ("T", "A"), ("C", "G")][len(site_pos) % 4]
                row = rng.integers(0, 3, 8)
                row["ACGT".index(ref)], row["ACGT".index(altb)] = depth - alt, alt
                rows.append((name, pos + 1, ref, altb, len(site_pos)))
                if len(site_pos) % 50 == 7:
                    rows.append((name, pos + 1, altb, ref, len(site_pos)))           # a second row at the site: the first one names REF / ALT
                site_pos.append(pos)
                table.append(row)
                n_here += 1
        site_off.append(site_off[-1] + n_here)
    sites = PlantedSites(rows, np.array(site_pos, dtype=np.int32), np.array(site_off, dtype=np.int64))
    return ((coverage, gcs, library, contigs, length, 10000, W), np.array(table, dtype=np.uint32).reshape(-1, 8), sites,
            {c: i for i, c in enumerate(contigs)})


def ref_stage(job, tracks, mutant=None):
    """the file of the planted stage from the literal references: tracks = {contig: (x, states of TIDDIT_CNV)} of cnv_cases.ref_job
    -> (text, {contig: (E, nsite, sum_beta, states)})"""
    (coverage, gcs, library, contigs, length, min_contig, W), table, sites, number = job
    col = {"A": 0, "C": 1, "G": 2, "T": 3}
    first = {}
    for _, _, ref, alt, k in sites.rows:
        first.setdefault(k, (col[ref], col[alt]))
    lines, detail = [], {}
    for c in contigs:
        if c not in tracks:
            continue
        x = [int(v) for v in tracks[c][0]]
        lo, hi = int(sites.site_off[number[c]]), int(sites.site_off[number[c] + 1])
        P = library["contig_ploidy_%s" % c]
        E, ns, sb = ref_emissions(x, W, sites.site_pos[lo:hi].tolist(), [int(table[k][first[k][0]]) for k in range(lo, hi)],
                                  [int(table[k][first[k][1]]) for k in range(lo, hi)], mutant=mutant)
        s = ref_viterbi(E, CM.index((P, P // 2)))
        detail[c] = (E, ns, sb, s)
        lines += ref_segments(s, x, ns, sb, P, W, length[c], c)
    return text_of(lines), detail


@functools.lru_cache(maxsize=None)
def planted_reference():
    job = planted_job()
    _, skipped, tracks = cnv_cases.ref_job(*job[0])
    text, detail = ref_stage(job, tracks)
    return text, skipped, tracks, detail
