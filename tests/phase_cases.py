"""Aimed cases for the read-backed phasing of the known SNV sites (tiddit_amd/tiddit_phase.py, csrc/tdt_phase.hip), each with the literal
claims it makes, the builders the CPU and the GPU tests share, and a second, independent reference: :func:`restate_keys` expands every
read's CIGAR into per-base arrays (no operation-by-operation walk), :func:`restate` is numpy over the sorted keys for rules 5 ... 8, a
plain union-find for the forest's edges and a BFS 2-colouring of that forest for rule 9.  The definition keeps parities inside its
union-find; the two share no code.

A read case is a dict: ``sites`` (per contig the rows ``(pos0, REF, ALT)`` of a sites file, a position may have two), ``reads`` (see
:func:`R`), the cuts ``S`` / ``H`` / ``min_bq`` / ``min_q`` / ``hash_bits``, ``cuts`` (where the reads are cut into batches) and its claims:
``keys`` = the observation keys as (name, site position, allele) in any order, ``links`` = the link rows ``(pos_j, pos_i, N, TRANS)``,
``gt`` = {site position: (GT, PS)} of every het site, ``sn`` = counters by name — whichever the case states, written down from the
case's own strings, never computed by either reference.

Mutants of the restatement (``mutant=``), each noticed inside the family named beside it in :data:`MUTANTS`.
"""
import collections
import os
import re
import struct
import tempfile

import numpy as np

from tiddit_amd import bamio, tiddit_alleles, tiddit_phase

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc")


def _define(path, name):
    m = re.search(r"^#define\s+%s\s+(\w+)" % name, open(path).read(), re.M)
    v = m.group(1)
    return int(v, 0) if v[0].isdigit() else _define(os.path.join(os.path.dirname(_CSRC), "..", "include", "tiddit_hip.h"), v)


KS_TILE = _define(os.path.join(_CSRC, "tdt_keystore.h"), "KS_TILE")
KS_BLOCK = _define(os.path.join(_CSRC, "tdt_keystore.h"), "KS_BLOCK")
MAX_OBS = _define(os.path.join(_CSRC, "tdt_phase.hip"), "PH_MAX_OBS")
PHL_TILE = _define(os.path.join(_CSRC, "tdt_phase.hip"), "PHL_TILE")
assert (KS_TILE, KS_BLOCK, MAX_OBS, PHL_TILE) == (4096, 256, 8, 256) and MAX_OBS == tiddit_phase.MAX_OBS

NAMES, LENGTHS = ["c0", "c1"], [3000, 2000]
PAD, PAD_BYTE = 64 << 10, 0x44
COLUMNS = ("tid", "pos", "end", "mapq", "flag", "rec_off")
MUTANTS = collections.OrderedDict([
    ("cap7", "cap"), ("cap9", "cap"), ("hash_nul", "names"), ("q_ff_refused", "qualities"), ("keep_discordant", "fragments"),
    ("link_nonhet", "fragments"), ("link_cross", "fragments"), ("lt_support", "thresholds"), ("lt_ratio", "thresholds"),
    ("tie_larger_row", "thresholds"), ("rebase_highest", "graphs"), ("parity_of_first", "graphs")])


def fnv(name):
    """FNV-1a, 64 bit, written out on its own (the literal values below come from the published test vectors, not from here)"""
    h = 14695981039346656037
    for b in name.encode() if isinstance(name, str) else name:
        h ^= b
        h = (h * 1099511628211) % (1 << 64)
    return h


# three names with their FNV-1a-64 values as published (draft-eastlake-fnv, the test suite of the reference implementation)
FNV_LITERALS = {"": 0xcbf29ce484222325, "a": 0xaf63dc4c8601ec8c, "foobar": 0x85944171f73967e8}


def R(tid, pos, cigar, seq, qual=30, mapq=60, flag=0, name=None, patch=(), pad=0):
    """one read.  seq: the query bases; qual: one value, a list, or None (absent: 0xff); name: the read name (default r<index>);
    patch: ((byte offset in the record, struct format, value), ...); pad: bytes of PAD_BYTE behind the record in the host entry's buffer"""
    cig = bamio.parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    if isinstance(qual, int):
        qual = [qual] * len(seq)
    return {"tid": tid, "pos": pos, "cigar": cig, "seq": seq, "qual": qual, "mapq": mapq, "flag": flag, "name": name, "patch": tuple(patch), "pad": pad}


def over(sites, tid, pos, length, choose=None, name=None, base="r", **kw):
    """a read of ``length`` M at pos whose base at every site in reach is chosen: ``choose`` = {site pos: 'r' REF, 'a' ALT, 'x' a third
    base, 'n' N}, every other site ``base``; the bases between the sites are N"""
    choose = choose or {}
    seq = ["N"] * length
    for p, ref, alt in sites[tid]:
        if pos <= p < pos + length:
            c = choose.get(p, base)
            seq[p - pos] = {"r": ref, "a": alt, "n": "N", "x": next(b for b in "ACGT" if b not in (ref, alt))}[c]
    return R(tid, pos, "%dM" % length, "".join(seq), name=name, **kw)


class Batch:
    def __init__(self, *cols_raw):
        self.tid, self.pos, self.end, self.mapq, self.flag, self.rec_off, self.raw = cols_raw

    def __len__(self):
        return len(self.tid)

    def cut(self, lo, hi):
        return Batch(self.tid[lo:hi], self.pos[lo:hi], self.end[lo:hi], self.mapq[lo:hi], self.flag[lo:hi], self.rec_off[lo:hi], self.raw)


def build_reads(reads, padding=True, truncate_last=False):
    parts, offs, o = [], [], 0
    for i, r in enumerate(reads):
        rec = bytearray(bamio.encode_record(r["name"] if r["name"] is not None else "r%d" % i, r["flag"], r["tid"], r["pos"], r["mapq"], r["cigar"], -1, -1, 0,
                                            seq=r["seq"], qual=None if r["qual"] is None else bytes(r["qual"])))
        for off, fmt, val in r["patch"]:
            struct.pack_into(fmt, rec, off, val)
        offs.append(o)
        parts.append(bytes(rec))
        o += len(rec)
        if padding and r["pad"]:
            parts.append(bytes([PAD_BYTE]) * r["pad"])
            o += r["pad"]
    pos = np.array([r["pos"] for r in reads], dtype=np.int32)
    rlen = np.array([sum(l for op, l in r["cigar"] if op in (0, 2, 3, 7, 8)) or 1 for r in reads], dtype=np.int32)
    b = Batch(np.array([r["tid"] for r in reads], dtype=np.int32), pos, (pos + rlen).astype(np.int32), np.array([r["mapq"] for r in reads], dtype=np.uint8),
              np.array([r["flag"] for r in reads], dtype=np.uint16), np.array(offs, dtype=np.uint64), np.frombuffer(b"".join(parts), dtype=np.uint8))
    if truncate_last:
        b.raw = b.raw[:offs[-1] + 20]
    return b


def build(case, padding=True):
    if ("built", padding) not in case:
        case[("built", padding)] = build_reads(case["reads"], padding, case.get("truncate_last", False))
    return case[("built", padding)]


def batches(case, padding=True):
    b = build(case, padding)
    cuts = [0] + list(case["cuts"]) + [len(b)]
    return [b.cut(lo, hi) for lo, hi in zip(cuts, cuts[1:]) if hi > lo]


def sites_text(rows_per_contig, names=NAMES):
    return "##fileformat=VCFv4.2\n" + "".join("%s\t%d\t.\t%s\t%s\n" % (names[t], p + 1, ref, alt) for t, rows in enumerate(rows_per_contig) for p, ref, alt in rows)


def sites_of(case):
    """the case's sites file through the product's own reader -> (Sites, codes)"""
    if "Sites" not in case:
        with tempfile.NamedTemporaryFile("w", suffix=".vcf", delete=False) as f:
            f.write(sites_text(case["sites"]))
        try:
            case["Sites"] = tiddit_alleles.read_sites(f.name, NAMES, case["lengths"])
        finally:
            os.unlink(f.name)
        case["codes"] = tiddit_phase.site_codes(case["Sites"])
    return case["Sites"], case["codes"]


def g_of(case, tid, pos):
    s, _ = sites_of(case)
    o0, o1 = int(s.site_off[tid]), int(s.site_off[tid + 1])
    return o0 + int(np.searchsorted(s.site_pos[o0:o1], pos))


# ------------------------------------------------------------------------------------------- the definition over a case
def definition(case, padding=True):
    """-> (keys [(K1, K2)], push counters, allele table, het flags, summarise's dict)"""
    s, codes = sites_of(case)
    keys, sn = [], tiddit_phase.new_counters()
    table, stats = np.zeros((len(s), 8), dtype=np.uint32), [0, 0]
    for b in batches(case, padding):
        tiddit_phase.keys_of_batch(keys, sn, codes, case["hash_bits"], s.site_pos, s.site_off, b, case["min_q"], case["min_bq"])
        tiddit_alleles.count_batch(table, stats, s.site_pos, s.site_off, b, case["min_q"], case["min_bq"])
    het, _, _ = tiddit_phase.het_flags(table, codes, case["H"])
    return keys, sn, table, het, tiddit_phase.summarise(keys, het, s.site_off, case["S"])


# ------------------------------------------------------------------------------------------- the restatement
def restate_keys(case, mutant=None, padding=True):
    """rules 2 - 4 restated: per read one array of (reference position, query index) per M/=/X base (np.repeat over the operations), the
    sites looked up in it -> (keys, push counters)"""
    s, codes = sites_of(case)
    cap = {"cap7": 7, "cap9": 9}.get(mutant, 8)
    keys, sn = [], dict(malformed=0, reads_used=0, observations=0, capped_reads=0)
    for b in batches(case, padding):
        raw = np.asarray(b.raw, dtype=np.uint8)
        for x in np.flatnonzero((b.tid >= 0) & (b.tid < len(s.site_off) - 1) & ((b.flag & 0xF04) == 0) & (b.mapq >= case["min_q"])):
            o0, o1 = int(s.site_off[b.tid[x]]), int(s.site_off[b.tid[x] + 1])
            k0, k1 = o0 + np.searchsorted(s.site_pos[o0:o1], b.pos[x]), o0 + np.searchsorted(s.site_pos[o0:o1], b.end[x])
            if k1 <= k0:
                continue
            ro = int(b.rec_off[x])
            if ro + 36 > len(raw):
                sn["malformed"] += 1
                continue
            bs, l_name, n_cig, l_seq = (int.from_bytes(raw[ro:ro + 4].tobytes(), "little"), int(raw[ro + 12]), int.from_bytes(raw[ro + 16:ro + 18].tobytes(), "little"),
                                        int.from_bytes(raw[ro + 20:ro + 24].tobytes(), "little", signed=True))
            if n_cig == 0 or l_seq < 1:
                continue
            c0 = ro + 36 + l_name
            if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs or ro + 4 + bs > len(raw):
                sn["malformed"] += 1
                continue
            words = np.frombuffer(raw[c0:c0 + 4 * n_cig].tobytes(), dtype="<u4").astype(np.int64)
            code, ln = words & 0xf, words >> 4
            if l_name < 1 or (code > 8).any():
                sn["malformed"] += 1
                continue
            on_ref, on_qry = np.isin(code, [0, 2, 3, 7, 8]), np.isin(code, [0, 1, 4, 7, 8])
            r0 = int(b.pos[x]) + np.cumsum(np.where(on_ref, ln, 0)) - np.where(on_ref, ln, 0)
            q0 = np.cumsum(np.where(on_qry, ln, 0)) - np.where(on_qry, ln, 0)
            m = np.isin(code, [0, 7, 8])
            within = np.concatenate([np.arange(l) for l in ln[m]] + [np.zeros(0, dtype=np.int64)])
            ref_at = np.repeat(r0[m], ln[m]) + within
            qry_at = np.repeat(q0[m], ln[m]) + within
            mine = np.arange(k0, k1)
            hit = np.isin(s.site_pos[mine], ref_at)
            qi = qry_at[np.searchsorted(ref_at, s.site_pos[mine][hit])]          # (ref_at ascends: M bases lie in reference order)
            if (qi >= l_seq).any():
                sn["malformed"] += 1
                continue
            sn["reads_used"] += 1
            seq = raw[c0 + 4 * n_cig:c0 + 4 * n_cig + (l_seq + 1) // 2]
            qual = raw[c0 + 4 * n_cig + (l_seq + 1) // 2:][:l_seq]
            nib = np.where(qi & 1, seq[qi >> 1] & 0xf, seq[qi >> 1] >> 4)
            ql = qual[qi].astype(np.int64)
            cd = codes[mine[hit]]
            fine = ((ql != 0xff) & (ql >= case["min_bq"])) if mutant == "q_ff_refused" else ((ql == 0xff) | (ql >= case["min_bq"]))
            allele = np.where(nib == 1 << (cd & 3), 0, np.where(nib == 1 << ((cd >> 2) & 3), 1, -1))
            ok = (cd != 0xff) & fine & (allele >= 0)
            obs = ((mine[hit][ok].astype(np.int64) << 1) | allele[ok]).tolist()
            if len(obs) > cap:
                sn["capped_reads"] += 1
            obs = obs[:cap]
            name = raw[ro + 36:ro + 36 + l_name - (0 if mutant == "hash_nul" else 1)].tobytes()
            keys.extend((fnv(name) & ((1 << case["hash_bits"]) - 1), o) for o in obs)
            sn["observations"] += len(obs)
    return keys, sn


def restate_forest(n_sites, j, i, n, trans, S, mutant=None):
    """rules 8 - 10 restated -> the dict of tiddit_phase.forest"""
    j, i, n, trans = (np.asarray(x, dtype=np.int64) for x in (j, i, n, trans))
    cis = n - trans
    hi, lo = np.maximum(cis, trans), np.minimum(cis, trans)
    elig = ((hi > S) if mutant == "lt_support" else (hi >= S)) & ((4 * lo < hi) if mutant == "lt_ratio" else (4 * lo <= hi))
    p = (trans > cis).astype(np.int64)
    w = np.minimum(hi - lo, (1 << 31) - 1)
    rows = np.flatnonzero(elig)
    rows = rows[np.lexsort(((-rows if mutant == "tie_larger_row" else rows), -w[rows]))]
    label = {}

    def top(v):
        while label.get(v, v) != v:
            v = label[v]
        return v
    used = np.zeros(len(j), dtype=np.uint8)
    adj = collections.defaultdict(list)
    for r in rows.tolist():
        a, b = top(int(i[r])), top(int(j[r]))
        label.setdefault(a, a), label.setdefault(b, b)
        if a != b:
            label[max(a, b)] = min(a, b)
            used[r] = 1
            adj[int(i[r])].append((int(j[r]), int(p[r])))
            adj[int(j[r])].append((int(i[r]), int(p[r])))
    root = np.full(n_sites, -1, dtype=np.int32)
    phase = np.zeros(n_sites, dtype=np.uint8)
    for v in (sorted(adj, reverse=True) if mutant == "rebase_highest" else sorted(adj)):
        if root[v] >= 0:
            continue
        comp, queue = [v], collections.deque([v])
        root[v], colour = v, {v: 0}
        while queue:
            u = queue.popleft()
            for t, par in adj[u]:
                if t not in colour:
                    colour[t] = colour[u] ^ (0 if mutant == "parity_of_first" and u != v else par)
                    root[t] = v
                    comp.append(t)
                    queue.append(t)
        for u in comp:
            root[u], phase[u] = min(comp), colour[u]
    agree, conflict = np.zeros(n_sites, dtype=np.uint32), np.zeros(n_sites, dtype=np.uint32)
    for r in rows.tolist():
        if not used[r]:
            (agree if int(phase[i[r]]) ^ int(phase[j[r]]) == p[r] else conflict)[root[i[r]]] += 1
    return {"root": root, "phase": phase, "edge_used": used, "agree": agree, "conflict": conflict,
            "sn": {"weak_links": int(len(j) - len(rows)), "forest_edges": int(used.sum()), "agree": int(agree.sum()), "conflict": int(conflict.sum()),
                   "phased_sites": int((root >= 0).sum()), "blocks": len(set(root[root >= 0].tolist()))}}


def restate(keys, het, site_off, S, mutant=None):
    """rules 5 - 10 restated: numpy over the sorted keys -> the dict of tiddit_phase.summarise"""
    k = np.array(keys, dtype=np.uint64).reshape(-1, 2)
    k = k[np.lexsort((k[:, 1], k[:, 0]))]
    g, a = (k[:, 1] >> np.uint64(1)).astype(np.int64), (k[:, 1] & np.uint64(1)).astype(np.int64)
    sn = {"fragment_rows": 0, "discordant_rows": 0, "cross_contig_pairs": 0}
    lj = li = par = np.zeros(0, dtype=np.int64)
    if len(k):
        head = np.r_[True, (k[1:, 0] != k[:-1, 0]) | (g[1:] != g[:-1])]
        at = np.flatnonzero(head)
        n, n_alt = np.diff(np.r_[at, len(k)]), np.add.reduceat(a, at)
        K1, G = k[at, 0], g[at]
        clean = (n_alt == 0) | (n_alt == n)
        sn["fragment_rows"], sn["discordant_rows"] = len(at), int((~clean).sum())
        if mutant == "keep_discordant":
            clean = np.ones(len(at), dtype=bool)
        good = clean & (np.ones(len(at), dtype=bool) if mutant == "link_nonhet" else np.asarray(het)[G] != 0)
        K1, G, A = K1[good], G[good], (n_alt[good] != 0).astype(np.int64)
        pair = K1[1:] == K1[:-1]
        contig = np.searchsorted(np.asarray(site_off), G, side="right")
        same = np.ones(len(pair), dtype=bool) if mutant == "link_cross" else contig[1:] == contig[:-1]
        sn["cross_contig_pairs"] = int((pair & ~same).sum())
        keep = pair & same
        li, lj, par = G[:-1][keep], G[1:][keep], (A[:-1] ^ A[1:])[keep]
    uniq, inv = np.unique((lj << 32) | li, return_inverse=True)
    N = np.bincount(inv, minlength=len(uniq)).astype(np.int64)
    T = np.bincount(inv, weights=par, minlength=len(uniq)).astype(np.int64)
    J, I = uniq >> 32, uniq & 0xffffffff
    f = restate_forest(len(het), J, I, N, T, S, mutant)
    u32 = lambda x: np.asarray(x).astype(np.uint32)
    return {"links": (u32(J), u32(I), u32(N), u32(T), f["edge_used"]), "root": f["root"], "phase": f["phase"],
            "blocks": tiddit_phase.blocks_of(f["root"], f["agree"], f["conflict"]), "sn": dict(sn, links=len(uniq), **f["sn"])}


def same_result(a, b):
    """two dicts of summarise / restate / device_finish: every array and every finish counter equal"""
    return (all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a["links"], b["links"])) and np.array_equal(a["root"], b["root"]) and
            np.array_equal(a["phase"], b["phase"]) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a["blocks"], b["blocks"])) and
            all(a["sn"][k] == b["sn"][k] for k in tiddit_phase.FINISH))


def same_forest(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("root", "phase", "edge_used", "agree", "conflict")) and a["sn"] == b["sn"]


def key_rows(keys):
    k = np.array(keys, dtype=np.uint64).reshape(-1, 2)
    return k[np.lexsort((k[:, 1], k[:, 0]))]


# ------------------------------------------------------------------------------------------- the read and fragment cases
CASES = []


def case(name, family, sites, reads, S=1, H=1, min_bq=13, min_q=20, hash_bits=64, cuts=(), reader_ok=True, lengths=None, capacity=None, **claims):
    CASES.append({"name": name, "family": family, "sites": sites, "reads": reads, "S": S, "H": H, "min_bq": min_bq, "min_q": min_q, "hash_bits": hash_bits,
                  "cuts": tuple(cuts), "reader_ok": reader_ok, "lengths": lengths or LENGTHS, "capacity": capacity, "claims": claims})


# ---- CIGAR edges: sites 100 (A>C) and 109 (G>T) on c0; the read shows ALT at the first and REF at the second
TWO = [[(100, "A", "C"), (109, "G", "T")], []]
for name, pos, cigar, seq, keys in (
        ("first and last base of an M", 100, "10M", "C" + "N" * 8 + "G", [(100, 1), (109, 0)]),
        ("in = and in X", 99, "2=8X1=", "NC" + "N" * 8 + "G", [(100, 1), (109, 0)]),
        ("behind I", 95, "5M3I10M", "N" * 8 + "C" + "N" * 8 + "G", [(100, 1), (109, 0)]),
        ("behind a leading S", 100, "4S10M", "TTTTC" + "N" * 8 + "G", [(100, 1), (109, 0)]),
        ("under D: no observation", 95, "5M1D9M", "N" * 5 + "N" * 8 + "G", [(109, 0)]),
        ("under N: no observation", 95, "5M3N7M", "N" * 11 + "G", [(109, 0)])):
    case("cigar " + name, "cigar", TWO, [R(0, pos, cigar, seq, name="q")], keys=[("q", p, a) for p, a in keys],
         sn={"observations": len(keys), "reads_used": 1, "malformed": 0, "fragment_rows": len(keys)})

# ---- bases: REF, ALT, a third base, N at four sites; a position with two rows is never observed
FIVE = [[(100, "A", "C"), (102, "C", "G"), (104, "G", "T"), (106, "T", "A"), (108, "A", "C"), (108, "A", "G")], []]
case("bases REF ALT third N and a position with two rows", "bases", FIVE, [R(0, 100, "9M", "ANGNCNNNA", name="q")], keys=[("q", 100, 0), ("q", 102, 1)],
     sn={"observations": 2})

# ---- qualities: min_bq - 1, min_bq, 0xff
Q3 = [[(100, "A", "C"), (101, "A", "C"), (102, "A", "C")], []]
case("qualities min_bq - 1, min_bq and 0xff", "qualities", Q3, [R(0, 100, "3M", "CCC", qual=[12, 13, 0xff], name="q")], keys=[("q", 101, 1), ("q", 102, 1)])
case("qualities absent", "qualities", Q3, [R(0, 100, "3M", "ACA", qual=None, name="q")], keys=[("q", 100, 0), ("q", 101, 1), ("q", 102, 0)])

# ---- the cap: a read over 8 and one over 9 sites
NINE = [[(100 + 2 * k, "A", "C") for k in range(9)], []]
case("cap the 8th and the 9th observation", "cap", NINE, [over(NINE, 0, 100, 16, name="eight", base="a"), over(NINE, 0, 100, 17, name="nine", base="a")],
     keys=[("eight", 100 + 2 * k, 1) for k in range(8)] + [("nine", 100 + 2 * k, 1) for k in range(8)], sn={"capped_reads": 1, "observations": 16})
case("cap a third base does not use a slot", "cap", NINE, [over(NINE, 0, 100, 17, {100: "x"}, name="q", base="a")],
     keys=[("q", 102 + 2 * k, 1) for k in range(8)], sn={"capped_reads": 0})

# ---- names: 1, 2 and 254 characters, an empty name, two names that differ in their last byte, mates with equal names
ONE2 = [[(100, "A", "C"), (150, "G", "T")], []]
_long = "L" * 253
_N = [over(ONE2, 0, 95, 10, name=nm, base="ra"[k > 1]) for k, nm in enumerate(("a", "ab", _long + "x", _long + "y", ""))] + [
    over(ONE2, 0, 96, 10, name="mate", base="a"), over(ONE2, 0, 145, 10, name="mate", base="r"), over(ONE2, 0, 146, 10, name="solo", base="a")]
case("names 1 2 254 characters, empty, last byte, mates", "names", ONE2, _N,
     keys=[("a", 100, 0), ("ab", 100, 0)] + [(nm, 100, 1) for nm in (_long + "x", _long + "y", "", "mate")] + [("mate", 150, 0), ("solo", 150, 1)],
     links=[(150, 100, 1, 1)], sn={"fragment_rows": 8, "links": 1}, H=1)

# ---- malformed: every shape the allele cases have, and l_read_name 0; a good read in front and behind
_G = lambda nm: over(ONE2, 0, 95, 10, name=nm, base="a")
for name, bad, n_bad, ok in (
        ("n_cigar_op runs past block_size", R(0, 95, "10M", "T" * 10, patch=((4 + 12, "<H", 2000),), pad=PAD), 1, False),
        ("the CIGAR asks for more than l_seq", R(0, 95, "80M", "C" * 10, pad=PAD), 1, False),
        ("l_seq 0", R(0, 95, "10M", "", pad=PAD), 0, True),
        ("op code 9", R(0, 95, [(0, 5), (9, 3), (0, 5)], "C" * 10, pad=PAD), 1, False),
        ("l_read_name 0", R(0, 95, "10M", "C" * 10, name="", patch=((4 + 8, "<B", 0),), pad=PAD), 1, False)):
    case("malformed " + name, "malformed", ONE2, [_G("g0"), bad, _G("g1")], keys=[("g0", 100, 1), ("g1", 100, 1)],
         sn={"malformed": n_bad, "reads_used": 2, "observations": 2}, reader_ok=ok)
case("malformed rec_off past the buffer", "malformed", ONE2, [_G("g0"), _G("g1"), R(0, 95, "10M", "C" * 10)], keys=[("g0", 100, 1), ("g1", 100, 1)],
     sn={"malformed": 1, "reads_used": 2}, reader_ok=False)
CASES[-1]["truncate_last"] = True

# ---- fragments.  Three het sites 100, 200, 300 and a hom site 250 between (only REF is ever seen there)
FR = [[(100, "A", "C"), (200, "C", "G"), (250, "G", "T"), (300, "T", "A")], [(100, "A", "C")]]
_pair = lambda nm, a0, a1, p0=95, p1=195: [over(FR, 0, p0, 10, name=nm, base=a0), over(FR, 0, p1, 10, name=nm, base=a1)]
_hets = [x for k in range(3) for x in _pair("h%d" % k, "r", "r")] + [x for k in range(3) for x in _pair("k%d" % k, "a", "a")]
case("fragments mates overlapping a site, agreeing and disagreeing", "fragments", FR,
     sorted(_hets + [over(FR, 0, 95, 10, name="ov", base="a"), over(FR, 0, 98, 10, name="ov", base="a"), over(FR, 0, 195, 10, name="ov", base="a"),
                     over(FR, 0, 95, 10, name="dis", base="a"), over(FR, 0, 98, 10, name="dis", base="r"), over(FR, 0, 195, 10, name="dis", base="a")],
            key=lambda r: r["pos"]),
     links=[(200, 100, 7, 0)], gt={100: ("0|1", 100 + 1), 200: ("0|1", 100 + 1)}, sn={"discordant_rows": 1, "fragment_rows": 16, "links": 1, "blocks": 1})
case("fragments a hom site between two hets", "fragments", FR,
     sorted(_hets + [over(FR, 0, 195, 10, name="w%d" % k, base="ra"[k % 2]) for k in range(4)] + [over(FR, 0, 245, 10, name="w%d" % k, base="r") for k in range(4)] +
            [over(FR, 0, 295, 10, name="w%d" % k, base="ra"[k % 2]) for k in range(4)], key=lambda r: r["pos"]),
     links=[(200, 100, 6, 0), (300, 200, 4, 0)], gt={100: ("0|1", 101), 200: ("0|1", 101), 300: ("0|1", 101)}, sn={"links": 2, "forest_edges": 2})
case("fragments mates on two contigs", "fragments", FR,
     [over(FR, 0, 95, 10, name="x%d" % k, base="ra"[k % 2]) for k in range(4)] + [over(FR, 1, 95, 10, name="x%d" % k, base="ra"[k % 2]) for k in range(4)],
     links=[], sn={"cross_contig_pairs": 4, "links": 0, "blocks": 0}, gt={100: ("0/1", None)})
# three and four records on one K1 through hash_bits = 4: the names are searched so that two fragments share the low four bits
_same4 = [nm for nm in ("n%d" % k for k in range(200)) if fnv(nm) & 15 == fnv("n0") & 15][:2]
_other4 = next(nm for nm in ("n%d" % k for k in range(200)) if fnv(nm) & 15 != fnv("n0") & 15)
case("fragments three and four records on one K1 (hash_bits 4)", "fragments", FR,
     sorted(_pair(_same4[0], "r", "r") + _pair(_same4[1], "r", "r") + _pair(_other4, "a", "a") + [over(FR, 0, 295, 10, name=_same4[0], base="r"),
                                                                                                   over(FR, 0, 295, 10, name=_other4, base="a")], key=lambda r: r["pos"]),
     hash_bits=4, links=[(200, 100, 2, 0), (300, 200, 2, 0)], sn={"fragment_rows": 6, "links": 2})
# a fragment of 16 rows: 16 het sites 20 apart, four reads of one name over four sites each, a second name with the other haplotype
SIX = [[(100 + 20 * k, "A", "C") for k in range(16)], []]
_sixteen = [over(SIX, 0, 95 + 80 * q, 70, name=nm, base=b) for nm, b in (("f", "r"), ("g", "a")) for q in range(4)]
case("fragments a fragment of 16 rows", "fragments", SIX, sorted(_sixteen, key=lambda r: r["pos"]),
     links=[(100 + 20 * (k + 1), 100 + 20 * k, 2, 0) for k in range(15)], sn={"fragment_rows": 32, "links": 15, "blocks": 1, "phased_sites": 16})


_POOL = sorted(("s%d" % k for k in range(4000)), key=fnv)     # names in the order their rows sort by K1


def _straddle(offset):
    """90 fragments of three rows each (sites 100, 200, 300) behind (PHL_TILE + offset) % 3 fragments of one row: the rows sort by K1, so
    a three-row fragment starts at row PHL_TILE + offset — at -2 and -1 its look-ahead crosses into the next tile, at 0 it starts the
    tile, at +1 and +2 the fragment in front of it is the one that crosses"""
    singles = (PHL_TILE + offset) % 3
    reads = [over(FR, 0, 95, 10, name=nm, base="ra"[k % 2]) for k, nm in enumerate(_POOL[:singles])]
    for k, nm in enumerate(_POOL[singles:singles + 90]):
        reads += _pair(nm, "ra"[k % 2], "ra"[k % 2]) + [over(FR, 0, 295, 10, name=nm, base="ra"[k % 2])]
    assert (PHL_TILE + offset - singles) % 3 == 0 and singles + 3 * 90 > PHL_TILE + 4
    return sorted(reads, key=lambda r: r["pos"]), singles


for _o in (-2, -1, 0, 1, 2):
    _reads, _s = _straddle(_o)
    case("fragments rows straddling a phase_links tile boundary at %+d" % _o, "tiles", FR, _reads, links=[(200, 100, 90, 0), (300, 200, 90, 0)],
         sn={"links": 2, "fragment_rows": 270 + _s, "forest_edges": 2})

# ---- thresholds.  n_cis pairs show (REF, REF) or (ALT, ALT), n_trans pairs (REF, ALT) or (ALT, REF), at the sites 100 and 200
def _links(n_cis, n_trans, tag=""):
    out = []
    for k in range(n_cis):
        out += _pair("%sc%d" % (tag, k), "ra"[k % 2], "ra"[k % 2])
    for k in range(n_trans):
        out += _pair("%st%d" % (tag, k), "ra"[k % 2], "ar"[k % 2])
    return out


for name, n_cis, n_trans, S, elig in (("max = S - 1", 2, 0, 3, False), ("max = S", 3, 0, 3, True), ("4 min = max", 8, 2, 2, True),
                                      ("4 min = max + 1: 4 x 3 > 11", 11, 3, 2, False), ("CIS = TRANS", 4, 4, 2, False), ("TRANS wins", 1, 6, 2, True)):
    case("thresholds " + name, "thresholds", FR, sorted(_links(n_cis, n_trans), key=lambda r: r["pos"]), S=S, links=[(200, 100, n_cis + n_trans, n_trans)],
         sn={"weak_links": 0 if elig else 1, "forest_edges": 1 if elig else 0},
         gt={100: ("0|1", 101), 200: ("1|0" if n_trans > n_cis else "0|1", 101)} if elig else {100: ("0/1", None), 200: ("0/1", None)})
# equal w decided by row: a triangle 100 - 200 - 300 whose three links all have w = 3; (300, 100) is TRANS and inconsistent with the other
# two; rows in (j, i) order: (200, 100) = 0, (300, 100) = 1, (300, 200) = 2, so row 2 stays out and is the CONFLICT
_tri = _links(3, 0, "a") + [x for k in range(3) for x in _pair("b%d" % k, "ra"[k % 2], "ar"[k % 2], 95, 295)] + \
    [x for k in range(3) for x in _pair("c%d" % k, "ra"[k % 2], "ra"[k % 2], 195, 295)]
case("thresholds equal w decided by row", "thresholds", FR, sorted(_tri, key=lambda r: r["pos"]), S=2,
     links=[(200, 100, 3, 0), (300, 100, 3, 3), (300, 200, 3, 0)], gt={100: ("0|1", 101), 200: ("0|1", 101), 300: ("1|0", 101)},
     sn={"forest_edges": 2, "conflict": 1, "agree": 0})

# ---- state: two pushes; the store grown from room for 64 keys
case("state two pushes, the store grown from 64 keys", "state", FR, sorted(_links(40, 3), key=lambda r: r["pos"]), S=2, cuts=(30,), capacity=64,
     links=[(200, 100, 43, 3)], sn={"observations": 86, "fragment_rows": 86})

# ---- the gate, which phase_keys takes from tdt_keystore.h and not from al_count: every read that must stay out carries ALT at site 100
_ALT10 = "NNNNNCNNNN"
case("gate each of the five flag bits alone stays out, every other bit comes in", "gate", ONE2,
     [R(0, 95, "10M", _ALT10, flag=bit, name="f%x" % bit) for bit in (0x4, 0x100, 0x200, 0x400, 0x800)] + [over(ONE2, 0, 95, 10, name="ok", base="r", flag=0xF0FB)],
     keys=[("ok", 100, 0)], sn={"reads_used": 1, "observations": 1, "malformed": 0})
case("gate mapq min_q - 1 stays out, min_q comes in", "gate", ONE2,
     [R(0, 95, "10M", _ALT10, mapq=19, name="lo"), over(ONE2, 0, 95, 10, name="hi", base="r", mapq=20)], min_q=20,
     keys=[("hi", 100, 0)], sn={"reads_used": 1, "observations": 1})
case("gate tid -1 and tid n_contigs stay out", "gate", ONE2,
     [R(-1, 95, "10M", _ALT10, name="none"), over(ONE2, 0, 95, 10, name="ok", base="r"), R(2, 95, "10M", _ALT10, name="beyond")],
     keys=[("ok", 100, 0)], sn={"reads_used": 1, "observations": 1}, reader_ok=False)

FAMILIES = sorted({c["family"] for c in CASES})
N_CASES = 39


def claim_problems(c, keys, sn, het, result):
    """the case's literal claims against one set of results -> a list of what does not hold"""
    s, _ = sites_of(c)
    bad, cl = [], c["claims"]
    at = lambda p, tid=0: g_of(c, tid, p)
    if "keys" in cl:
        want = sorted((fnv(nm) & ((1 << c["hash_bits"]) - 1), at(p) << 1 | a) for nm, p, a in cl["keys"])
        if sorted(keys) != want:
            bad.append(("keys", sorted(keys)[:4], want[:4]))
    if "links" in cl:
        got = list(zip(*[x.tolist() for x in result["links"][:4]]))
        want = sorted((at(pj), at(pi), n, t) for pj, pi, n, t in cl["links"])
        if got != want:
            bad.append(("links", got[:4], want[:4]))
    for p, (gt, ps) in cl.get("gt", {}).items():
        g = at(p)
        got = ("0/1", None) if result["root"][g] < 0 else ("1|0" if result["phase"][g] else "0|1", int(s.site_pos[result["root"][g]]) + 1)
        if not het[g] or got != (gt, ps):
            bad.append(("gt", p, bool(het[g]), got, (gt, ps)))
    allsn = dict(sn, **result["sn"])
    for k, v in cl.get("sn", {}).items():
        if allsn[k] != v:
            bad.append(("sn", k, allsn[k], v))
    return bad


# ------------------------------------------------------------------------------------------- the graph cases (tdt_phase_forest)
GRAPHS = []


def graph(name, n_sites, links, S=2, **claims):
    """links: [(j, i, N, TRANS)] in row order"""
    cols = [np.array([l[k] for l in links], dtype=dt) for k, dt in enumerate((np.int32, np.int32, np.uint32, np.uint32))]
    GRAPHS.append({"name": name, "n_sites": n_sites, "j": cols[0], "i": cols[1], "n": cols[2], "trans": cols[3], "S": S, "claims": claims})


for _n in (2, 3, 64, 65, 4097, 70000):                      # a chain with alternating parity: site k has phase k // 2 % 2
    graph("chain of %d" % _n, _n, [(k + 1, k, 5, 5 * (k % 2)) for k in range(_n - 1)], blocks=1, edges=_n - 1,
          phase=[(k // 2) % 2 for k in range(_n)] if _n <= 65 else None)
# a triangle whose edge (2, 0) says TRANS while the path 0 - 1 - 2 says CIS: all three have w = 5, (2, 0) is row 2 and stays out
graph("triangle with one inconsistent edge", 3, [(1, 0, 5, 0), (2, 1, 5, 0), (2, 0, 5, 5)], blocks=1, edges=2, out=[2], conflict=1, phase=[0, 0, 0])
# a square 0 - 1 - 2 - 3 - 0 whose edge (3, 0), the lightest (w = 2), is inconsistent: it stays out whatever its row
graph("square with one inconsistent edge", 4, [(3, 0, 2, 0), (1, 0, 5, 0), (2, 1, 5, 5), (3, 2, 5, 0)], blocks=1, edges=3, out=[0], conflict=1, phase=[0, 0, 1, 1])
graph("star of 1000", 1001, [(k, 0, 3 + k % 5, (3 + k % 5) * (k % 2)) for k in range(1, 1001)], blocks=1, edges=1000, phase=[0] + [k % 2 for k in range(1, 1001)])
# two components {0, 1} and {2, 3} that both pick the heavy edge (2, 1)
graph("two components that both pick the same edge", 4, [(1, 0, 3, 0), (3, 2, 3, 3), (2, 1, 9, 0)], blocks=1, edges=3, phase=[0, 0, 0, 1])
# the lowest site is a leaf that hangs TRANS on site 5, which every label points to: its phase before re-basing is 1
graph("a component whose lowest site is a leaf with phase 1 before re-basing", 6, [(5, 0, 4, 4), (5, 3, 9, 0), (5, 4, 9, 0)], blocks=1, edges=3,
      phase=[0, 0, 0, 1, 1, 1], root=[0, -1, -1, 0, 0, 0])
graph("isolated sites and weak links only", 5, [(1, 0, 1, 0), (3, 2, 4, 2)], blocks=0, edges=0, weak=2, root=[-1] * 5)
graph("no links", 7, [], blocks=0, edges=0)
graph("agreeing chord", 3, [(1, 0, 5, 5), (2, 1, 5, 5), (2, 0, 2, 0)], blocks=1, edges=2, agree=1, phase=[0, 1, 0])


def _random_graphs(seed, count, max_sites):
    """`count` random graphs of at most max_sites sites as ONE graph of disjoint parts (the row order runs over all of them)"""
    rng = np.random.default_rng(seed)
    links, base = [], 0
    for _ in range(count):
        n = int(rng.integers(2, max_sites + 1))
        pairs = {tuple(sorted(rng.choice(n, 2, replace=False).tolist())) for _ in range(int(rng.integers(0, 2 * n)))}
        for a, b in sorted(pairs):
            N = int(rng.integers(1, 7))
            links.append((base + b, base + a, N, int(rng.integers(0, N + 1))))
        base += n
    return base, [links[k] for k in rng.permutation(len(links))]


_ns, _l = _random_graphs(11, 1000, 12)
graph("1000 random graphs of at most 12 sites", _ns, _l)
_rng = np.random.default_rng(12)
_a, _b = _rng.integers(0, 50000, 200000), _rng.integers(0, 50000, 200000)
_keep = _a != _b
_N = _rng.integers(1, 9, 200000)
_pairs = {}
for a, b, N, t in zip(_a[_keep].tolist(), _b[_keep].tolist(), _N[_keep].tolist(), (_rng.integers(0, 9, 200000)[_keep] % (_N[_keep] + 1)).tolist()):
    _pairs.setdefault((max(a, b), min(a, b)), (N, t))
graph("one random graph of 50000 sites and 200000 links", 50000, [(j, i, N, t) for (j, i), (N, t) in _pairs.items()])
N_GRAPHS = 16


def graph_problems(c, f):
    """the graph case's literal claims against one forest dict"""
    bad, cl = [], c["claims"]
    if "phase" in cl and cl["phase"] is not None and f["phase"].tolist() != cl["phase"]:
        bad.append(("phase", f["phase"].tolist()[:8]))
    if "root" in cl and f["root"].tolist() != cl["root"]:
        bad.append(("root", f["root"].tolist()[:8]))
    if "out" in cl and np.flatnonzero(f["edge_used"] == 0).tolist() != cl["out"]:
        bad.append(("out", np.flatnonzero(f["edge_used"] == 0).tolist()[:8]))
    for k, name in (("blocks", "blocks"), ("edges", "forest_edges"), ("conflict", "conflict"), ("agree", "agree"), ("weak", "weak_links")):
        if k in cl and f["sn"][name] != cl[k]:
            bad.append((k, f["sn"][name], cl[k]))
    return bad
