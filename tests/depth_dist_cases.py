"""Aimed inputs and references for the depth-distribution kernel (csrc/tdt_depth_dist.hip, ``tdt_depth_dist``).

Everything is deterministic.  ``DD_TILE`` and ``DD_CAP`` are read from the `#define` lines of the source when this module is imported, so
the cases stay on their edges when a constant is retuned.  A case is a dict:

  name, family     "tile" boundaries, contig "ends", "records" and filter bits, depth "values", "multi" contig launches, call "state"
  lengths          the contigs' lengths, header order
  records          rows (tid, start, end, mapq, flag, mate_tid, mate_pos, tlen, sa) for ``tdt_evstore_append``, sorted by (tid, start)
  order            None, or the permutation of the contig table's rows the call is made with
  batches          the record counts at which the appends are cut (the store grows between them), capacity = the store's first size
  claims           what the case says about itself, checked on the CPU against the literal loop (tests/test_depth_dist_refs_cpu.py):
                   ("start" | "end", record index, value), ("depth", contig, base, value), ("max" | "min", contig, value),
                   ("bin", contig, depth bin, bases), ("tiles", contig, count), ("span_over_tile", contig)

Three statements of the same definition (tiddit_amd/tiddit_depth_dist.py): ``reference`` (numpy: difference array, cumsum, bincount of
the clipped depth — what the GPU test compares with), ``literal`` (a loop per read and per base) and ``restatement`` (tile by tile as the
kernel works, with one-line mutants that the cases must tell apart)."""
import os
import re

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc", "tdt_depth_dist.hip")


def parse_constants(text=None):
    text = open(_SRC).read() if text is None else text
    out = {}
    for name in ("DD_TILE", "DD_CAP"):
        m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+([0-9]+)[ \t]*(?://[^\n]*)?$" % name, text, re.M)
        if not m:
            raise KeyError("cannot parse #define %s" % name)
        out[name] = int(m.group(1))
    return out


K = parse_constants()
T, CAP = K["DD_TILE"], K["DD_CAP"]
MIN_Q, MAX_INS = 5, 1000
UNMAPPED, DUPLICATE = 0x4, 0x400
COLUMNS = ("tid", "pos", "end", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "sa_off")
TYPES = (np.int32, np.int32, np.int32, np.uint8, np.uint16, np.int32, np.int32, np.int32, np.int64)
MUTANTS = {"start_strict": "tile", "end_inclusive": "tile", "no_halo": "tile", "no_clip": "ends", "cap_off_by_one": "values",
           "drop_unmapped": "records", "drop_duplicate": "records", "drop_low_q": "records"}


def rec(tid, start, end, mapq=60, flag=0x3):
    return (tid, start, end, mapq, flag, tid, max(0, start + 300), 450, -1)


def kept(r, min_q=MIN_Q, drop=None):
    """the record filter: none of UNMAPPED, DUPLICATE, LOW_Q (drop: the bit a mutant forgets)"""
    bad = []
    if drop != "drop_unmapped":
        bad.append(bool(r[4] & UNMAPPED))
    if drop != "drop_duplicate":
        bad.append(bool(r[4] & DUPLICATE))
    if drop != "drop_low_q":
        bad.append(r[3] < min_q)
    return not any(bad)


def _row(depth, cap=CAP):
    depth = np.asarray(depth, dtype=np.int64)
    row = np.zeros(cap + 4, dtype=np.int64)
    if len(depth):
        row[:cap + 1] = np.bincount(np.minimum(depth, cap), minlength=cap + 1)
        row[cap + 1], row[cap + 2], row[cap + 3] = depth.sum(), depth.max(), depth.min()
    return row


def depths(lengths, records, min_q=MIN_Q):
    """per contig the depth of every base: difference array, then cumsum"""
    out = []
    for t, LN in enumerate(lengths):
        d = np.zeros(LN + 1, dtype=np.int64)
        for r in records:
            if r[0] == t and kept(r, min_q):
                s, e = max(r[1], 0), min(r[2], LN)
                if e > s:
                    d[s] += 1
                    d[e] -= 1
        out.append(np.cumsum(d[:LN]))
    return out


def reference(lengths, records, min_q=MIN_Q):
    """int64[n_contigs][CAP + 4], header order"""
    return np.stack([_row(d) for d in depths(lengths, records, min_q)]) if lengths else np.zeros((0, CAP + 4), dtype=np.int64)


def literal(lengths, records, min_q=MIN_Q):
    """the definition read aloud: for every kept read, every base it names that exists"""
    out = [[0] * LN for LN in lengths]
    for r in records:
        if (r[4] & UNMAPPED) or (r[4] & DUPLICATE) or r[3] < min_q:
            continue
        for b in range(r[1], r[2]):
            if 0 <= b < lengths[r[0]]:
                out[r[0]][b] += 1
    return out


def spans(lengths, records):
    """what tdt_evstore_spans gives: per contig max(end - start) over ALL its records, not below 0"""
    sp = [0] * len(lengths)
    for r in records:
        sp[r[0]] = max(sp[r[0]], r[2] - r[1])
    return sp


def restatement(lengths, records, mutant=None, tile=None, cap=None, min_q=MIN_Q):
    """the table tile by tile, as the kernel forms it: the records with start in [lo - span, hi) by a search on the sorted starts,
    +1 / -1 in a difference array of the tile, its running sum, the histogram of min(depth, cap)"""
    tile, cap = tile or T, cap or CAP
    sp = spans(lengths, records)
    out = np.zeros((len(lengths), cap + 4), dtype=np.int64)
    drop = mutant if mutant in ("drop_unmapped", "drop_duplicate", "drop_low_q") else None
    for t, LN in enumerate(lengths):
        mine = [r for r in records if r[0] == t]
        starts = np.array([r[1] for r in mine], dtype=np.int64)
        hist = np.zeros(cap + 1, dtype=np.int64)
        total, mx, mn = 0, 0, None
        for lo in range(0, LN, tile):
            hi = lo + tile if mutant == "no_clip" else min(lo + tile, LN)
            i0 = int(np.searchsorted(starts, lo if mutant == "no_halo" else lo - sp[t], side="left"))
            i1 = int(np.searchsorted(starts, hi, side="left"))
            diff = np.zeros(hi - lo + 1, dtype=np.int64)
            for r in mine[i0:i1]:
                if not kept(r, min_q, drop):
                    continue
                s = r[1] + 1 if mutant == "start_strict" else r[1]
                e = r[2] + 1 if mutant == "end_inclusive" else r[2]
                e = e if mutant == "no_clip" else min(e, LN)
                a, b = max(s, lo), min(e, hi)
                if a < b:
                    diff[a - lo] += 1
                    diff[b - lo] -= 1
            depth = np.cumsum(diff[:hi - lo])
            binned = np.where(depth < cap - 1, depth, cap) if mutant == "cap_off_by_one" else np.minimum(depth, cap)
            hist += np.bincount(binned, minlength=cap + 1)
            total += int(depth.sum())
            mx = max(mx, int(depth.max()))
            mn = int(depth.min()) if mn is None else min(mn, int(depth.min()))
        out[t, :cap + 1] = hist
        out[t, cap + 1], out[t, cap + 2], out[t, cap + 3] = total, mx, mn or 0
    return out


def columns(records):
    """the records as the columns of one host batch"""
    import types
    a = np.array(records, dtype=np.int64).reshape(-1, 9)
    return types.SimpleNamespace(**{k: np.ascontiguousarray(a[:, i].astype(dt)) for i, (k, dt) in enumerate(zip(COLUMNS, TYPES))})


def _case(name, family, lengths, records, claims, order=None, batches=(), capacity=0):
    records = sorted(records, key=lambda r: (r[0], r[1]))          # (stable: equal starts keep their order)
    return {"name": name, "family": family, "lengths": list(lengths), "records": records, "claims": claims, "order": order,
            "batches": tuple(batches), "capacity": capacity}


def _random_reads(rng, tid, LN, n, longest=150):
    pos = np.sort(rng.integers(0, max(1, LN - 20), n))
    end = pos + rng.integers(1, longest + 1, n)
    mapq = rng.choice([0, MIN_Q - 1, MIN_Q, 30, 60], n)
    flag = rng.choice([0x3, 0x1, 0x13, 0x403, 0x7, 0x103, 0x803], n, p=[.5, .1, .1, .08, .07, .08, .07])
    return [rec(tid, int(p), int(e), int(q), int(f)) for p, e, q, f in zip(pos, end, mapq, flag)]


def _index(records, r):
    return sorted(records, key=lambda x: (x[0], x[1])).index(r)


def cases():
    out = []
    rng = np.random.default_rng(11)
    LN = 4 * T + 3
    lo, hi = T, 2 * T
    # ---- tile boundaries
    edge_starts = [rec(0, s, s + 50) for s in (lo - 1, lo, lo + 1, hi - 1, hi)]
    edge_ends = [rec(0, e - 50, e) for e in (lo - 1, lo, lo + 1, hi - 1, hi)]
    recs = edge_starts + edge_ends
    claims = [("start", _index(recs, r), r[1]) for r in edge_starts] + [("end", _index(recs, r), r[2]) for r in edge_ends]
    claims += [("depth", 0, lo - 2, 3), ("depth", 0, lo - 1, 3), ("depth", 0, lo, 3), ("depth", 0, lo + 1, 3), ("depth", 0, lo + 49, 2),
               ("depth", 0, lo + 50, 1), ("depth", 0, hi - 2, 2), ("depth", 0, hi - 1, 2), ("depth", 0, hi, 2), ("depth", 0, hi + 48, 2),
               ("depth", 0, hi + 49, 1), ("depth", 0, hi + 50, 0), ("tiles", 0, 5)]
    out.append(_case("reads that start or end on lo-1, lo, lo+1, hi-1, hi", "tile", [LN], recs, claims))
    out.append(_case("a read covering exactly one tile", "tile", [LN], [rec(0, 2 * T, 3 * T)],
                     [("depth", 0, 2 * T - 1, 0), ("depth", 0, 2 * T, 1), ("depth", 0, 3 * T - 1, 1), ("depth", 0, 3 * T, 0), ("bin", 0, 1, T)]))
    out.append(_case("tile 0 to tile 3, tiles 1-2 through the halo alone", "tile", [LN], [rec(0, T - 100, 3 * T + 100)],
                     [("start", 0, T - 100), ("end", 0, 3 * T + 100), ("depth", 0, T, 1), ("depth", 0, 3 * T - 1, 1), ("bin", 0, 1, 2 * T + 200),
                      ("span_over_tile", 0)]))
    recs = _random_reads(rng, 0, LN, 1500) + [rec(0, T // 2, 2 * T + T // 2 + 7)]
    out.append(_case("one read longer than a tile among many short ones", "tile", [LN], recs, [("span_over_tile", 0), ("tiles", 0, 5)]))
    # ---- contig ends
    lengths = [1, T - 1, T, T + 1]
    recs = [rec(0, 0, 1), rec(0, 0, 2), rec(0, 0, T + 10)]
    for t, n in enumerate(lengths[1:], 1):
        recs += [rec(t, n - 40, n), rec(t, n - 30, n + 1), rec(t, n - 5, n + T + 50), rec(t, 0, 30)]
    claims = [("depth", 0, 0, 3), ("max", 0, 3), ("min", 0, 3), ("bin", 0, 3, 1)]
    for t, n in enumerate(lengths[1:], 1):
        claims += [("end", _index(recs, rec(t, n - 40, n)), n), ("end", _index(recs, rec(t, n - 30, n + 1)), n + 1),
                   ("end", _index(recs, rec(t, n - 5, n + T + 50)), n + T + 50), ("depth", t, n - 1, 3), ("depth", t, n - 41, 0),
                   ("tiles", t, 1 if n <= T else 2)]
    out.append(_case("contigs of 1, T-1, T, T+1 bases; reads ending on LN and overhanging it by 1 and by more than a tile", "ends",
                     lengths, recs, claims))
    # ---- records and filter bits
    lengths = [3000, 500, 2 * T + 11]
    recs = [rec(0, 100, 100), rec(0, 200, 190), rec(0, 300, 400)]
    filtered = [rec(0, 1000, 1100, 60, 0x3 | UNMAPPED), rec(0, 1200, 1300, 60, 0x3 | DUPLICATE), rec(0, 1400, 1500, MIN_Q - 1, 0x3),
                rec(0, 1600, 1700, 60, 0x3 | UNMAPPED | DUPLICATE), rec(0, 1800, 1900, 0, 0x3 | DUPLICATE), rec(0, 2000, 2100, 0, 0x3 | UNMAPPED),
                rec(0, 2200, 2300, 0, 0x3 | UNMAPPED | DUPLICATE)]
    recs += filtered + [rec(0, 2400, 2500, MIN_Q, 0x3), rec(0, 2600, 2700, 60, 0x3 | 0x100 | 0x800)]
    recs += [rec(2, T - 10, T + 10), rec(2, T, T + 5, MIN_Q - 1), rec(2, 2 * T, 2 * T + 11, 60, 0x3 | DUPLICATE)]
    claims = [("depth", 0, 100, 0), ("depth", 0, 195, 0), ("depth", 0, 350, 1), ("depth", 0, 2450, 1), ("depth", 0, 2650, 1), ("max", 0, 1),
              ("max", 1, 0), ("bin", 1, 0, 500), ("depth", 2, T, 1), ("depth", 2, 2 * T + 5, 0), ("bin", 0, 1, 300)]
    claims += [("depth", 0, r[1] + 50, 0) for r in filtered]
    out.append(_case("end == start, end < start, an empty contig between two, every filter bit alone and combined, mapq min_q-1 / min_q",
                     "records", lengths, recs, claims))
    # ---- depth values
    recs = [rec(0, 100, 110)] * (CAP + 1) + [rec(0, 110, 120)] * CAP + [rec(0, 120, 130)] * (CAP - 1) + [rec(0, 0, T + 7), rec(0, 0, T + 9)]
    claims = [("depth", 0, 105, CAP + 3), ("depth", 0, 115, CAP + 2), ("depth", 0, 125, CAP + 1), ("max", 0, CAP + 3), ("min", 0, 2),
              ("bin", 0, CAP, 30), ("bin", 0, 2, T + 7 - 30)]
    out.append(_case("stacked reads over the cap on a contig covered end to end", "values", [T + 7], recs, claims))
    recs = [rec(0, 100, 110)] * (CAP - 1) + [rec(0, 110, 120)] * (CAP - 2) + [rec(0, 120, 130)] * (CAP - 3) + [rec(0, 0, 500), rec(0, 90, 140)]
    claims = [("depth", 0, 105, CAP + 1), ("depth", 0, 115, CAP), ("depth", 0, 125, CAP - 1), ("bin", 0, CAP - 1, 10), ("bin", 0, CAP, 20),
              ("max", 0, CAP + 1), ("min", 0, 0)]
    out.append(_case("depth exactly CAP-1, CAP and CAP+1", "values", [600], recs, claims))
    # ---- several contigs in one launch
    lengths = [77, T + 1, 2 * T + 5, 3 * T + 9, 0, 4 * T]
    recs = []
    for t, n in enumerate(lengths):
        if n:
            recs += _random_reads(rng, t, n, 40 if t == 0 else 500)
    claims = [("tiles", 0, 1), ("tiles", 1, 2), ("tiles", 2, 3), ("tiles", 3, 4), ("tiles", 4, 0), ("tiles", 5, 4)]
    out.append(_case("contigs of 1, 2, 3, 4 tiles (and one of no bases), header order", "multi", lengths, recs, claims))
    out.append(_case("the same with the table's rows permuted", "multi", lengths, recs, claims, order=[3, 5, 0, 4, 2, 1]))
    # ---- call-to-call state
    out.append(_case("two calls on one store that grew on the device between appends", "state", lengths, recs, claims,
                     batches=(700, 1500), capacity=16))
    return out


CASES = cases()
