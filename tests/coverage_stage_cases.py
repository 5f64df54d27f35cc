"""Aimed inputs, references and claimed properties for the coverage kernels (csrc/tdt_coverage.hip, csrc/tdt_cov_record.h): the ten
flavours of cov_accumulate — bin size 1, 2..128 (difference pairs, MODE 1), 129..1023 (pair tables in LDS) and >= 1024 (tables in global
memory), each fed from four arrays, 8-byte packed records or 8-byte binned records, and the run-merged flavour forced onto the small
bins by TIDDIT_COV_MODE=0.

Everything is deterministic.  The window, tile and chunk constants are read from the `#define` lines of the two sources when this
module is imported, so the cases stay on their edges when a constant is retuned.  A case is a dict:

  name, family      "A" read geometry, "B" window geometry, "C" counts and alignment, "D" contig end, "E" filter and validity,
                    "F" accumulation, "G" multi-contig launches (family H, call-to-call state, is `state_sequence()`: a list of steps)
  contigs           [(name, LN)];  z, min_q
  cols              per contig the four columns (int32 start, int32 end, uint8 mapq, uint16 flag)
  items             the launch order of the multi-contig entries: [(contig index, lo, hi)] slices of the contigs' columns
  layouts           the entries that take it: "host" (CoverageHistogram.push), "arrays" (push_device), "arrays_multi"
                    (push_device_multi), "packed" (tdt_cov_pack_device + push_packed_device_multi), "binned" (pack_binned_device +
                    push_binned_device_multi)
  mode0             also run in a histogram created under TIDDIT_COV_MODE=0
  expect            "bins", or the error code `finish` must raise;  expect_by_layout: codes that one entry raises at the push
  misalign          every column starts one element into its allocation (CovItem.aligned == 0)
  null_end          the packed entry gets no `end` array (legal while no record carries the escape span)
  paths             the path classes the case is aimed at; claim: where the model below says it lands

The references: `reference(case)` is the C oracle (oracle.coverage_stream), `restatement(case)` a numpy restatement of
tiddit_coverage.pyx:50-72 with a sparse result; tests/golden/coverage_edges.npz holds what the real update_coverage gives on the
small cases.  They are pinned against each other, and the claims against what every family promises, by
test_coverage_stage_refs_cpu.py; test_gpu_coverage_stages.py compares the kernels.  Test infrastructure only."""
import hashlib
import itertools
import os
import re

import numpy as np

import oracle

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc")
_CONST_FILES = {"COV_THREADS": "tdt_coverage.hip", "COV_RPL": "tdt_coverage.hip", "COV_RPL1": "tdt_coverage.hip",
                "COV_READS_PER_BLOCK": "tdt_coverage.hip", "COV_WIN": "tdt_coverage.hip", "COV_WIN1": "tdt_coverage.hip",
                "COV_DQMAX": "tdt_coverage.hip", "COV_LUT_LDS_MAX": "tdt_coverage.hip", "COV_KEPT_SLOTS": "tdt_coverage.hip",
                "COV_PK_SPAN": "tdt_cov_record.h"}


def parse_constants(sources=None):
    """the `#define`s the cases are aimed at, evaluated from the text of the two sources (object-like macros of integers, other
    macros, + - * / << and brackets; the first definition, i.e. the one under #ifndef); KeyError when one can no longer be read.
    `sources`: file name -> text, for the test of this parser."""
    defs = {}
    for fn in sorted(set(_CONST_FILES.values())):
        text = sources[fn] if sources else open(os.path.join(_CSRC, fn)).read()
        for name, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+([A-Za-z_]\w*)[ \t]+([^\n]*?)[ \t]*(?://[^\n]*)?$", text, re.M):
            defs.setdefault((fn, name), body)
            defs.setdefault(name, body)

    def value(name, depth=0):
        if name not in defs or depth > 8:
            raise KeyError("cannot parse #define %s" % name)
        expr = re.sub(r"\b(0[xX][0-9a-fA-F]+|[0-9]+)[uUlL]*\b", lambda h: str(int(h.group(1), 0)), defs[name])
        expr = re.sub(r"[A-Za-z_]\w*", lambda h: str(value(h.group(0), depth + 1)), expr)
        if not re.fullmatch(r"[0-9()+\-*/< \t]+", expr) or "<" in expr.replace("<<", ""):
            raise KeyError("#define %s is not an integer expression: %r" % (name, defs[name]))
        return int(eval(expr.replace("/", "//")))

    out = {}
    for name, fn in _CONST_FILES.items():
        if (fn, name) not in defs:
            raise KeyError("cannot parse #define %s in %s" % (name, fn))
        out[name] = value(name)
    return out


CONSTANTS = parse_constants()
THREADS, RPL0, RPL1, RPB = (CONSTANTS[k] for k in ("COV_THREADS", "COV_RPL", "COV_RPL1", "COV_READS_PER_BLOCK"))
WIN0, WIN1, DQMAX, LUT_LDS_MAX = (CONSTANTS[k] for k in ("COV_WIN", "COV_WIN1", "COV_DQMAX", "COV_LUT_LDS_MAX"))
KEPT_SLOTS, PK_SPAN = CONSTANTS["COV_KEPT_SLOTS"], CONSTANTS["COV_PK_SPAN"]

TDT_E_RANGE, TDT_E_INEXACT, TDT_E_UNSUPPORTED = -3, -4, -6
GOLDEN_MAX = 2100                                   # cases up to this many reads also have the real update_coverage's bins in the fixture
CASE_MAX = 3 * RPB + 1                              # reads per contig (the kept-slot and 2^53 cases of family F alone are larger)
CLASSES = {1: (1,), 2: (2, 3, 50, 127, 128), 3: (129, 500, 1022, 1023), 4: (1024, 1025, 4096, 1 << 20, (1 << 20) + 1)}
ALL_Z = tuple(z for k in sorted(CLASSES) for z in CLASSES[k])
ALL_LAYOUTS = ("host", "arrays", "arrays_multi", "packed", "binned")
REC = {"host": 0, "arrays": 0, "arrays_multi": 0, "packed": 1, "binned": 2}
MUTANTS = ("no_one_short", "z_in_last_bin", "end_bin_size_for_single", "mapq_gt", "ignore_duplicate", "interior_short", "interior_long")


def z_class(z):
    return next(k for k, v in CLASSES.items() if z in v) if z in ALL_Z else (1 if z == 1 else 2 if z <= 128 else 3 if z < 1024 else 4)


def ceil_log2(z):
    return (z - 1).bit_length()


def dispatch(z, layout="arrays", forced_mode0=False):
    """The host's choice of kernel flavour, restated: tdt_cov_create (`small_bins`: bin_size >= 2 and S = 24 + ceil_log2 <= 31, unless
    TIDDIT_COV_MODE=0; xmax) and cov_launch_items (margin, lds_lut, the template arguments) in tdt_coverage.hip."""
    rec = REC[layout]
    if rec == 2 and not 2 <= z < LUT_LDS_MAX:
        raise ValueError("binned records exist for 2 <= bin_size < %d" % LUT_LDS_MAX)
    small = z >= 2 and 24 + ceil_log2(z) <= 31 and not forced_mode0
    lds_lut = z + 1 <= LUT_LDS_MAX
    rpl = RPL1 if small else RPL0
    kind = "mode1" if small else "z1" if z == 1 else "tabled" if lds_lut else "global"
    return {"mode": 1 if small else 0, "kind": kind, "rec": rec, "flavour": "%s/rec%d" % (kind, rec), "RPL": rpl, "TILE": THREADS * rpl,
            "WIN": WIN1 if small else WIN0, "margin": DQMAX + 8 if small else 640 // z + 4, "xmax": min(DQMAX * z, 32768),
            "safe_ko": (WIN1 - DQMAX - 2) if small else (WIN0 - 3), "safe_last": (DQMAX + 2) if small else 3}


def layouts_for(z, want=ALL_LAYOUTS):
    return [l for l in want if l != "binned" or 2 <= z < LUT_LDS_MAX]


# ================================================================================================================ references
class CoverageRangeError(IndexError):
    pass


def _f32q(num, den):
    return (np.asarray(num).astype(np.float32) / np.float32(den)).astype(np.float64)


def restate_contig(start, end, mapq, flag, LN, z, min_q, mutant=None):
    """tiddit_coverage.pyx:50-72 behind the read filter of __main__.py:231-235, over one contig's columns -> (indices of the nonzero
    bins, their float64 values, reads kept).  Every contribution is double(float32(bases) / float32(den)): a multiple of 2^-(24 +
    ceil_log2 z), so the float64 sums are exact in any order while a bin stays below 2^53 of these units and numpy may
    add them in its own order.  Raises CoverageRangeError where the reference raises IndexError (a kept read whose last bin lies beyond
    the contig) and for what the library also refuses (tdt_cov_finish: start < 0, end <= start).
    `mutant` names a one-line departure (MUTANTS) for the tests of the cases' aim."""
    assert mutant is None or mutant in MUTANTS, mutant
    s, e = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    mapq, flag = np.asarray(mapq, dtype=np.int64), np.asarray(flag, dtype=np.int64)
    nbins = -(-LN // z)
    ebs = LN - (nbins - 1) * z
    keep = (flag & 0x4) == 0
    if mutant != "ignore_duplicate":
        keep &= (flag & 0x400) == 0
    keep &= (mapq > min_q) if mutant == "mapq_gt" else (mapq >= min_q)
    s, e = s[keep], e[keep]
    kept = int(keep.sum())
    if not kept:
        return np.zeros(0, np.int64), np.zeros(0), 0
    fb, eb = s // z, (e - 1) // z                                                   # :50-51
    if (s < 0).any() or (e <= s).any() or (eb >= nbins).any():
        raise CoverageRangeError("a kept read leaves the contig's bins")
    one = fb == eb                                                                  # :55
    den1 = np.where(fb[one] == nbins - 1, ebs, z) if mutant == "end_bin_size_for_single" else np.full(int(one.sum()), z)
    idx = [fb[one]]
    val = [((e[one] - s[one]).astype(np.float32) / den1.astype(np.float32)).astype(np.float64)]      # :56-57, always by bin_size
    m = ~one
    sm, em, fm, lm = s[m], e[m], fb[m], eb[m]
    idx.append(fm)
    val.append(_f32q((fm + 1) * z - sm, z))                                         # :61-62
    bl = em - lm * z - (0 if mutant == "no_one_short" else 1)                       # :63, one short
    den = np.full(len(lm), z) if mutant == "z_in_last_bin" else np.where(lm < nbins - 1, z, ebs)      # :66-69
    idx.append(lm)
    val.append((bl.astype(np.float32) / den.astype(np.float32)).astype(np.float64))
    lo = fm + (2 if mutant == "interior_short" else 1)                              # :71
    hi = lm + (1 if mutant == "interior_long" else 0)
    ok = hi > lo
    if ok.any():                                                                    # +1.0 per interior bin, as a difference array
        pos = np.concatenate([lo[ok], hi[ok]])
        dlt = np.concatenate([np.ones(ok.sum(), np.int64), -np.ones(ok.sum(), np.int64)])
        u, inv = np.unique(pos, return_inverse=True)
        cnt = np.cumsum(np.bincount(inv, weights=dlt).astype(np.int64))[:-1]
        seg = np.flatnonzero(cnt > 0)
        length = (u[1:] - u[:-1])[seg]
        first = np.repeat(u[:-1][seg] - np.concatenate([[0], np.cumsum(length)[:-1]]), length)
        idx.append(first + np.arange(int(length.sum())))
        val.append(np.repeat(cnt[seg], length).astype(np.float64))
    idx, val = np.concatenate(idx), np.concatenate(val)
    if mutant == "interior_long" and len(idx) and idx.max() >= nbins:
        keep_i = idx < nbins
        idx, val = idx[keep_i], val[keep_i]
    u, inv = np.unique(idx, return_inverse=True)
    tot = np.bincount(inv, weights=val, minlength=len(u))
    nz = tot != 0
    return u[nz], tot[nz], kept


def restatement(case, mutant=None):
    """-> [(nonzero bin indices, values) per contig], reads kept in all; CoverageRangeError for a case that must be refused"""
    out, kept = [], 0
    for (_, LN), cols in zip(case["contigs"], case["cols"]):
        i, v, k = restate_contig(*cols, LN, case["z"], case["min_q"], mutant)
        out.append((i, v))
        kept += k
    return out, kept


def reference(case):
    """the C oracle on every contig -> [(nonzero bin indices, values) per contig], reads kept; IndexError where the reference raises"""
    out, kept = [], 0
    for (_, LN), cols in zip(case["contigs"], case["cols"]):
        if LN == 0:
            assert not len(cols[0])
            out.append((np.zeros(0, np.int64), np.zeros(0)))
            continue
        bins, k = oracle.coverage_stream(*cols, LN, case["z"], case["min_q"])
        nz = np.flatnonzero(bins)
        out.append((nz, bins[nz]))
        kept += k
    return out, kept


def dense(sparse, nbins):
    b = np.zeros(nbins)
    b[sparse[0]] = sparse[1]
    return b


def nbins_of(LN, z):
    return -(-LN // z)


def input_hash(case):
    h = hashlib.sha256(repr((case["z"], case["min_q"], case["contigs"])).encode())
    for cols in case["cols"]:
        for a in cols:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ================================================================================================================ the model
def _shape(s, e, nbins, z, mode1):
    """cov_bin_record's shape and clamped first bin (tdt_cov_record.h) -> shape (3 = invalid), first bin"""
    last = nbins - 1
    fb, eb = np.maximum(s, 0) // z, (e - 1) // z
    valid = (s >= 0) & (e > s) & (eb <= last)
    shape = np.where(eb == fb, 0, np.where((eb >= last) | (eb - fb > (255 if mode1 else 1)), 2, 1))
    return np.where(valid, shape, 3), np.minimum(fb, last)


def model_item(s, e, cand, nbins, z, d):
    """The lane and window bookkeeping of cov_accumulate for one item (one contig's slice of a launch), restated: chunks of
    COV_READS_PER_BLOCK reads, tiles of TILE, the lane key K (first bin of the lane's first read), the `safe` test, the register-path
    conditions of each flavour and the re-base rule `s_tbin[step] + margin >= base + WIN`.  -> dict with `bases` (per workgroup the
    sequence of window bases), `slack` (per re-base test: s_tbin[step] + margin - (base + WIN); >= 0 re-bases), `same_base` (re-base
    tests met with nb == base), per-read `path` (0 filtered, 1 register, 2 literal inside the window, 3 literal to global memory,
    4 refused) and `slot`.  It says where a case lands; no expected bin comes from it."""
    s, e, cand = np.asarray(s, np.int64), np.asarray(e, np.int64), np.asarray(cand, bool)
    n, rpl, tile, win, last = len(s), d["RPL"], d["TILE"], d["WIN"], nbins - 1
    fb, eb = np.maximum(s, 0) // z, (e - 1) // z
    valid = (s >= 0) & (e > s) & (eb <= last)
    shape, fbc = _shape(s, e, nbins, z, d["mode"] == 1)
    keybin = fbc if d["rec"] == 2 else fb                      # K of a lane / what the re-base looks at (clamped for the window base)
    i = np.arange(n)
    K = keybin[(i // rpl) * rpl]
    base = np.zeros(n, np.int64)
    out = {"bases": [], "slack": [], "same_base": 0}
    for r0 in range(0, n, RPB):
        r1 = min(n, r0 + RPB)
        b = int(min(keybin[r0], last))
        seq = [b]
        for step, t0 in enumerate(range(r0, r1, tile)):
            if step:
                tl = lambda k: int(min(keybin[min(r0 + (k + 1) * tile, r1) - 1], last))
                slack = tl(step) + d["margin"] - (b + win)
                out["slack"].append(slack)
                if slack >= 0:
                    if tl(step - 1) != b:
                        b = tl(step - 1)
                        seq.append(b)
                    else:
                        out["same_base"] += 1
            base[t0:min(t0 + tile, r1)] = b
        out["bases"].append(seq)
    ko = K - base
    rs, re1 = s - K * z, e - K * z
    ln = e - s
    if d["rec"] == 2:
        fast = cand & (ko >= 0) & (ko < d["safe_ko"]) & ((fbc - K == 0) | (fbc - K == 1)) & (shape <= 1)
    elif d["kind"] == "mode1":
        safe = (ko >= 0) & (ko < d["safe_ko"]) & (K + d["safe_last"] <= last)
        fast = cand & safe & (rs >= 0) & (rs < 2 * z) & (ln >= 1) & (ln <= d["xmax"]) & (re1 <= d["xmax"])
    else:
        dq, r = (re1 - 1) // z, (rs >= z).astype(np.int64)
        fast = cand & (rs >= 0) & (rs < 2 * z) & (ln >= 1) & (re1 <= 3 * z) & (dq >= r) & (dq - r <= 1)
        if d["kind"] == "tabled":
            fast &= (ko >= 0) & (ko < d["safe_ko"]) & (K + d["safe_last"] <= last)
        else:
            fast &= valid
    inwin = (fb >= base) & (eb < base + win)
    path = np.where(~cand, 0, np.where(~valid, 4, np.where(fast, 1, np.where(inwin, 2, 3))))
    out["path"], out["slot"] = path, i % rpl
    return out


def model(case, layout="arrays", forced_mode0=False):
    """the claim of a case under one entry: flavour, window bases per workgroup, reads per path class, (family A) slots per geometry"""
    z = case["z"]
    d = dispatch(z, layout, forced_mode0)
    claim = {"flavour": d["flavour"], "bases": [], "slack": [], "same_base": 0, "register": 0, "literal_window": 0, "literal_global": 0,
             "refused": 0, "behind": 0, "RPL": d["RPL"]}
    slots = {}
    for ci, lo, hi in case["items"]:
        st, en, mq, fl = (a[lo:hi] for a in case["cols"][ci])
        if hi == lo or nbins_of(case["contigs"][ci][1], z) == 0:
            continue
        cand = ((fl & 0x404) == 0) & ((np.minimum(mq, 63) if d["rec"] else mq).astype(np.int64) >= max(case["min_q"], 0 if d["rec"] else -1))
        m = model_item(st, en, cand, nbins_of(case["contigs"][ci][1], z), z, d)
        claim["bases"] += m["bases"]
        claim["slack"] += m["slack"]
        claim["same_base"] += m["same_base"]
        for k, code in (("register", 1), ("literal_window", 2), ("literal_global", 3), ("refused", 4)):
            claim[k] += int((m["path"] == code).sum())
        for g, at in case.get("geometry", {}).get(ci, {}).items():
            for a in at:
                if lo <= a < hi:
                    slots.setdefault(g, set()).add((int(m["slot"][a - lo]), int(m["path"][a - lo])))
    if slots:
        claim["slots"] = slots
    return claim


# ================================================================================================================ building blocks
def _cols(s, e, mapq=None, flag=None):
    s, e = np.asarray(s, dtype=np.int64), np.asarray(e, dtype=np.int64)
    assert len(s) == len(e) and (np.abs(s) < 2 ** 31).all() and (np.abs(e) < 2 ** 31).all()
    n = len(s)
    mapq = np.full(n, 60, np.uint8) if mapq is None else np.asarray(mapq).astype(np.uint8)
    flag = np.zeros(n, np.uint16) if flag is None else np.asarray(flag).astype(np.uint16)
    return s.astype(np.int32), e.astype(np.int32), mapq, flag


def lanes_to_reads(z, lanes):
    """The lane builder.  lanes: [(K, [(first bin - K, offset of the first base in its bin, last bin - K, offset of the last base in its
    bin), ...])], one entry per lane, every lane with the flavour's RPL reads -> start, end (exclusive).  The first read of a lane fixes
    the lane key: with first bin - K == 0 there, K is the key the kernel derives."""
    s, e = [], []
    for K, reads in lanes:
        for fr, so, lr, eo in reads:
            s.append((K + fr) * z + so)
            e.append((K + lr) * z + eo + 1)
    return np.array(s, np.int64), np.array(e, np.int64)


def offsets(z):
    return sorted({0, 1 % z, z - 1})


CASES, _ORDER = {}, []


def make_case(name, family, z, contigs, cols, layouts=ALL_LAYOUTS, mode0=None, min_q=0, expect="bins", paths=("register",), **extra):
    items = extra.pop("items", None) or [(i, 0, len(c[0])) for i, c in enumerate(cols)]
    c = {"name": name, "family": family, "z": z, "min_q": min_q, "contigs": list(contigs), "cols": list(cols), "items": items,
         "layouts": layouts_for(z, layouts), "mode0": (2 <= z <= 128) if mode0 is None else mode0, "expect": expect,
         "expect_by_layout": {}, "misalign": 0, "null_end": False, "paths": paths, "n": sum(len(k[0]) for k in cols)}
    c.update(extra)
    assert family in "FG" or max(len(k[0]) for k in cols) <= CASE_MAX, name
    return c


def _case(name, *a, **k):
    assert name not in CASES, name
    c = CASES[name] = make_case(name, *a, **k)
    _ORDER.append(name)
    return c


def case_names(family=None):
    return [n for n in _ORDER if family is None or CASES[n]["family"] == family]


def get(name):
    c = CASES[name]
    if "claim" not in c:
        c["claim"] = model(c, c["layouts"][min(1, len(c["layouts"]) - 1)])
    return c


def in_golden(c):
    return c["expect"] == "bins" and c["n"] <= GOLDEN_MAX and max(nbins_of(LN, c["z"]) for _, LN in c["contigs"]) <= 1 << 16


def n_pairs(c):
    """(layout, forced mode 0) runs of a case"""
    return len(c["layouts"]) * (2 if c["mode0"] else 1)


# ---------------------------------------------------------------------------------------------------------------- A: read geometry
def a_geometries(z, d):
    g = {}
    for so, eo, nb in itertools.product(offsets(z), offsets(z), (0, 1, 2, 3)):
        if nb or eo >= so:
            g["s%d_e%d_b%d" % (so, eo, nb)] = (so, nb, eo)
    if d["mode"] == 1:
        for nb in (DQMAX - 2, DQMAX - 1, DQMAX, DQMAX + 1):
            g["s0_e0_b%d" % nb] = (0, nb, 0)
            g["s%d_e%d_b%d" % (z - 1, z - 1, nb)] = (z - 1, nb, z - 1)
        x = d["xmax"]                                              # re1 == xmax and xmax + 1 from bin K: the last base is x - 1 / x past K z
        g["re1_xmax"] = (0, (x - 1) // z, (x - 1) % z)
        g["re1_xmax_plus1"] = (0, x // z, x % z)
    return g


def _family_a():
    for z in ALL_Z:
        d = dispatch(z)
        rpl, geo = d["RPL"], a_geometries(z, d)
        lanes, at, K = [], {}, 40
        for name, (so, nb, eo) in geo.items():
            for j in range(rpl):
                fr = 0 if j == 0 else (j - 1) % 3              # the geometry from bin K (as the lane's own first read), K, K + 1 or K + 2
                reads = [(k % 3, 0, k % 3, 0) for k in range(rpl)]     # its siblings: one base in K, K + 1, K + 2
                reads[0] = (0, 0, 0, 0)
                reads[j] = (fr, so, fr + nb, eo)
                at.setdefault(name, []).append(len(lanes) * rpl + j)
                lanes.append((K, reads))
                K += 1
        s, e = lanes_to_reads(z, lanes)
        LN = z * 1000 + (1 if z > 1 else 0)
        _case("a_geometry_z%d" % z, "A", z, [("c", LN)], [_cols(s, e)], geometry={0: at},
              paths=("register", "literal_window") if z > 1 else ("register",))
        lanes, K = [], 7
        for run in (1, 2, 63, 64, 65, 3):
            for k in range(run):
                o = offsets(z)
                lanes.append((K, [(j & 1, o[(j + k) % len(o)], (j & 1) + ((j >> 1) & 1), o[(j + k + 1) % len(o)] if (j >> 1) & 1 else z - 1)
                                  for j in range(rpl)]))
            K += 5
        s, e = lanes_to_reads(z, lanes)
        _case("a_runs_z%d" % z, "A", z, [("c", LN)], [_cols(s, e)])


# ---------------------------------------------------------------------------------------------------------------- B: window geometry
B_Z = (1, 50, 128, 500, 1023, 1024, 4096)


def _tile(d, fill_K, last_K, special=()):
    """256 lanes: `special` lanes first, lanes of one-base reads in bin fill_K, and the last lane (whose last read is the tile's last
    read: what the re-base test of the NEXT step looks at) in bin last_K"""
    lanes = list(special)
    lanes += [(fill_K, [(0, 0, 0, 0)] * d["RPL"])] * (THREADS - 1 - len(lanes))
    lanes.append((last_K, [(0, 0, 0, 0)] * d["RPL"]))
    assert len(lanes) == THREADS
    return lanes


def _family_b():
    for z in B_Z:
        d = dispatch(z)
        rpl, win, mg, lim = d["RPL"], d["WIN"], d["margin"], d["safe_ko"]
        B0 = 100
        two = lambda: [(0, z - 1, 1, 0)] * rpl                                     # two-bin reads: a register-path lane where it is safe
        sp0 = [(B0, [(0, 0, 0, 0)] * rpl)]                                          # the chunk's first read fixes base = B0
        sp0 += [(B0 + lim + k, two()) for k in (-1, 0, 1)]                          # ko one below, on and one above the `safe` limit
        sp0 += [(B0 + win - 3, [(0, 0, 2 + k, 0)] * rpl) for k in (0, 1, 6)]        # last bin base + WIN - 1, base + WIN and beyond
        sp0 += [(B0 - 3, two())]                                                    # in front of the window
        sp0 += [(B0, [(0, 0, 0, 0), (-3, 0, -2, 0)] + [(0, 0, 0, 0)] * (rpl - 2))]  # ... as a sibling of a lane inside it
        B1 = B0 + win - mg - 1
        t = [_tile(d, B0, B0, sp0),
             _tile(d, B0 + 5, B1, [(B0 + 7, two())]),                               # tile 1 ends 1 short of the re-base condition
             _tile(d, B1, B1 + 1, [(B0, two()), (B1 + 3, two())]),                  # tile 2 meets it by exactly 0: base moves to B1; reads behind
             _tile(d, B1 + 1, B1 + win - mg + 10, [(B1 + 9, two())]),               # tile 3: again, base moves to B1 + 1
             _tile(d, B1 + 1, B1 + 1, [(B1 + 30, two()), (B0, two())]),
             _tile(d, B1 + 1, B1 + win, [(B1 + 31, two())]),                        # tile 5 meets the condition with nb == base
             _tile(d, B1 + 2, B1 + 2)]
        s, e = lanes_to_reads(z, [l for tl in t for l in tl])
        assert len(s) <= RPB
        LN = z * (B1 + 2 * win + 50) + (z // 2)
        _case("b_window_z%d" % z, "B", z, [("c", LN)], [_cols(s, e)], paths=("register", "literal_window", "literal_global"))
        # the same edges against the contig end: K + safe_last one below, on and above last_bin
        nb = 300 + d["safe_last"]
        lanes = [(nb - 1 - d["safe_last"] + k, two()) for k in (-1, 0, 1)]
        s, e = lanes_to_reads(z, lanes)
        _case("b_last_bin_limit_z%d" % z, "B", z, [("c", z * nb)], [_cols(s, e)], paths=("register",))


# ---------------------------------------------------------------------------------------------------------------- C: counts, alignment
C_Z = (1, 50, 128, 500, 1023, 1024, 1 << 20)


def pattern_reads(n, z, nbins, seed):
    """n sorted reads of 1 .. 3 z bases inside a contig of nbins bins, a fixed arithmetic pattern (no generator state)"""
    i = np.arange(n, dtype=np.int64)
    room = nbins * z
    span = 1 + (i * 13 + seed * 7) % (3 * z if z > 1 else 5)
    s = (i * max(1, (room - 4 * z - 8) // max(n, 1)) + (i * 7 + seed) % z) % max(1, room - 4 * z - 8)
    s = np.sort(s)
    mapq = np.where((i + seed) % 11 == 0, 3, 60)
    flag = np.where((i + seed) % 13 == 0, 0x400, np.where((i + seed) % 17 == 0, 0x4, (i % 3) * 0x10))
    return _cols(s, s + span, mapq, flag)


def count_list():
    out = {1, 2 * RPB - 1, 2 * RPB, 2 * RPB + 1, RPB - 1, RPB, RPB + 1}
    for rpl in (RPL0, RPL1):
        out |= {rpl - 1, rpl, rpl + 1, THREADS * rpl - 1, THREADS * rpl, THREADS * rpl + 1}
    return sorted(out)


def _family_c():
    for z in C_Z:
        nb = 1500
        ns = count_list()
        contigs = [("n%d" % n, z * nb - (k % 3)) for k, n in enumerate(ns)]
        for mis in (0, 1):
            _case("c_counts_z%d%s" % (z, "_misaligned" if mis else ""), "C", z, contigs,
                  [pattern_reads(n, z, nb - 1, k) for k, n in enumerate(ns)], min_q=10, misalign=mis,
                  layouts=ALL_LAYOUTS if not mis else ("arrays", "arrays_multi", "packed", "binned"),
                  paths=("register", "literal_window") if z > 1 else ("register",))
        ns = [n for n in ns if n <= RPL0 + 1]                      # the vector-load tail alone: small enough for the fixture
        _case("c_lane_tail_z%d" % z, "C", z, [("n%d" % n, z * 40 - 1) for n in ns], [pattern_reads(n, z, 39, n) for n in ns], min_q=10,
              paths=())
        n = RPB + 3 * THREADS
        s = np.full(n, 77 * z + z // 2, np.int64)                  # one run of equal K across the chunk boundary
        _case("c_run_across_chunks_z%d" % z, "C", z, [("c", z * nb)], [_cols(s, s + (z + 1 if z <= 4096 else 1))])      # (depth below 2^(29 - L))


# ---------------------------------------------------------------------------------------------------------------- D: contig end
def overhang_fits(z, ebs):
    """an overhanging read's last-bin quotient (z - 1) / end_bin_size stays below 2^53 fixed-point units of 2^-(24 + ceil_log2 z): what
    the accumulators can hold (above it the library answers TDT_E_INEXACT: d_overhang_unrepresentable_*)"""
    return (z - 1) * (1 << (24 + ceil_log2(z))) < ebs << 53


def d_contig_reads(z, nb, ebs):
    LN = (nb - 1) * z + ebs
    last0 = (nb - 1) * z
    r = [(LN - 1, LN), (last0, LN), (0, LN), (0, 1)]                                # in the last bin (divided by z, :55-57); whole contig
    if ebs > 1:
        r += [(last0 + 1, LN), (last0, LN - 1)]
    if nb >= 2:
        r += [(last0 - 1, last0 + 1), (last0 - z, last0 + 1), (last0 - 1, LN), (last0 - z, LN)]       # one-short last-bin count 0; ends at LN
        r += [(b * z + o, LN) for b in range(max(0, nb - 5), nb - 1) for o in offsets(z)]
        if ebs < z and overhang_fits(z, ebs):                                       # overhang inside the last bin: quotient above 1
            r += [(last0 - 1, nb * z), (last0 - 1, LN + 1), (last0 - z, nb * z)]
    if ebs < z:
        r += [(last0, nb * z), (LN - 1, LN + 1)]                                    # single-bin reads overhanging: still divided by z
    if nb >= 3:
        r += [(0, last0), (z - 1, last0 + 1), (1 % z, last0 - 1)]
    r.sort()
    return np.array([a for a, _ in r]), np.array([b for _, b in r])


def _family_d():
    for z in ALL_Z:
        contigs, cols = [], []
        for nb in (1, 2, 3, 4, DQMAX + 1, DQMAX + 2, DQMAX + 3):
            for ebs in sorted({1, max(1, z - 1), z}):
                contigs.append(("b%d_e%d" % (nb, ebs), (nb - 1) * z + ebs))
                cols.append(_cols(*d_contig_reads(z, nb, ebs)))
        _case("d_contig_end_z%d" % z, "D", z, contigs, cols, paths=("literal_window",))
    for z in ALL_Z:
        if not overhang_fits(z, 1):                                                 # (z - 1) / 1 in one bin: more than an accumulator holds
            s, e = np.array([z - 1, z - 1, 5]), np.array([2 * z, z + 2, 9])
            _case("d_overhang_unrepresentable_z%d" % z, "D", z, [("c", z + 1)], [_cols(s, e)], expect=TDT_E_INEXACT, paths=("register",))
    for z in (128, 500, 1024, 1 << 20):
        LN = (1 << 31) - 1
        nb = nbins_of(LN, z)
        d = dispatch(z)
        ends = [(LN - 1, LN), (LN - 300, LN), (LN - 3 * z, LN), (LN - 3 * z - 1, LN - 1), ((nb - 1) * z, LN), ((nb - 1) * z - 1, LN),
                ((nb - 2) * z - 1, (nb - 1) * z + 1), (LN - (1 << 24), LN), (5, 5 + 2 * z), (LN // 2, LN // 2 + z)]
        lanes = [(nb - 1100 + 2 * k, [(j & 1, offsets(z)[j % 3 % len(offsets(z))], (j & 1) + (j >> 1 & 1), z - 1) for j in range(d["RPL"])])
                 for k in range(2 * THREADS)]
        s, e = lanes_to_reads(z, lanes)
        s, e = np.concatenate([s, [a for a, _ in ends]]), np.concatenate([e, [b for _, b in ends]])
        _case("d_contig_2g_z%d" % z, "D", z, [("big", LN)], [_cols(s, e)], paths=("register", "literal_global"), big=True)


# ---------------------------------------------------------------------------------------------------------------- E: filter, validity
E_Z = (1, 50, 128, 500, 1024)
INVALID = {"negative_start": lambda z, nb: (-1, z), "empty": lambda z, nb: (3 * z, 3 * z), "reversed": lambda z, nb: (3 * z + 1, 3 * z),
           "beyond": lambda z, nb: ((nb - 1) * z, nb * z + 1)}


def _family_e():
    for z in E_Z:
        nb = 400
        LN = z * nb
        base_s = np.arange(64, dtype=np.int64) * (z + 1)
        for q in (-1, 0, 1, 63, 64, 255):
            mq = np.array([max(q - 1, 0), min(max(q, 0), 255), 63, 64, 255, 0, 62, 254] * 8)
            c = _case("e_mapq_q%d_z%d" % (q, z), "E", z, [("c", LN)], [_cols(base_s, base_s + z + 2, mq)], min_q=q, paths=())
            if q > 63:
                c["expect_by_layout"] = {"packed": TDT_E_UNSUPPORTED, "binned": TDT_E_UNSUPPORTED}
        fl = np.array([0] + [1 << b for b in range(16)] + [0x404, 0xffff, 0xfbfb])
        s = np.arange(len(fl), dtype=np.int64) * 2 * z
        _case("e_flag_bits_z%d" % z, "E", z, [("c", LN)], [_cols(s, s + 2 * z + 1, None, fl)], paths=())
        rpl = dispatch(z)["RPL"]
        good = lambda k: (10 * z + k, 11 * z + k + 1)
        for kind, make in INVALID.items():
            bad = make(z, nb)
            # filtered: every slot holds the bad read once, behind the unmapped bit, the duplicate bit or a low mapq — no error
            s, e, mq, fl = [], [], [], []
            for j in range(rpl):
                for k in range(rpl):
                    a, b = bad if k == j else good(k)
                    s.append(a), e.append(b)
                    mq.append(3 if (k == j and j % 3 == 2) else 60)
                    fl.append((0x4, 0x400, 0)[j % 3] if k == j else 0)
            _case("e_%s_filtered_z%d" % (kind, z), "E", z, [("c", LN)], [_cols(s, e, mq, fl)], min_q=10, paths=())
            for j in range(rpl):
                reads = [bad if k == j else good(k) for k in range(2 * rpl)]      # two lanes: the bad read in slot j of the first
                _case("e_%s_slot%d_z%d" % (kind, j, z), "E", z, [("c", LN)], [_cols([a for a, _ in reads], [b for _, b in reads])],
                      expect=TDT_E_RANGE, paths=("refused",))
    for z in (50, 500, 1024):
        LN = PK_SPAN + 10 * z + 7
        s = np.array([z + 1, z + 2, z + 3, 5 * z, 9 * z])
        e = np.array([z + 1 + PK_SPAN - 1, z + 2 + PK_SPAN, z + 3 + PK_SPAN + 1, 5 * z + 3, LN])
        _case("e_packed_span_z%d" % z, "E", z, [("c", LN)], [_cols(s, e)], paths=("literal_global",))
        s = np.arange(3 * RPL0, dtype=np.int64) * 3
        _case("e_packed_null_end_z%d" % z, "E", z, [("c", LN)], [_cols(s, s + 2 * z)], null_end=True, layouts=("packed",))


# ---------------------------------------------------------------------------------------------------------------- F: accumulation
def _family_f():
    for z in ALL_Z:
        n = min(RPB, (1 << (29 - ceil_log2(z))) - 1)              # one workgroup of identical reads (fewer where 2^53 units are nearer)
        s = np.full(n, 20 * z + 1 % z, np.int64)                  # every add lands on the same bins
        _case("f_pileup_z%d" % z, "F", z, [("c", 400 * z + 1)], [_cols(s, s + 2 * z + z // 2)],
              paths=("register",) if z <= 128 else ("literal_window",))
    for z in (4096, 1 << 20):
        full = 1 << (29 - ceil_log2(z))                            # reads of depth 1.0 that bring one accumulator to 2^53 units
        for n, expect in ((full - 1, "bins"), (full, TDT_E_INEXACT)):
            s = np.full(n, 3 * z + 5, np.int64)
            _case("f_2p53_%s_z%d" % ("below" if expect == "bins" else "reached", z), "F", z, [("c", 40 * z)], [_cols(s, s + 2 * z)],
                  layouts=("host", "arrays", "packed"), expect=expect, paths=("literal_window",))
    n = KEPT_SLOTS * RPB // 4 + RPB + 1                            # more workgroups than kept-read counters: the slots wrap
    i = np.arange(n, dtype=np.int64)
    s = (i * 50 * 40000) // n + i % 7
    _case("f_kept_slots_wrap_z50", "F", 50, [("c", 50 * 40100)], [_cols(s, s + 1 + i % 120, np.where(i % 5 == 0, 3, 60))], min_q=10,
          layouts=("arrays", "packed"), mode0=False)


# ---------------------------------------------------------------------------------------------------------------- G: multi-contig launches
def _family_g():
    sizes = (0, 1, RPB, RPB + 1)
    for z in (1, 50, 500, 1024):
        perms = list(itertools.permutations(range(4))) if z in (50, 500) else [(0, 1, 2, 3), (1, 2, 3, 0), (2, 3, 0, 1), (3, 2, 1, 0)]
        for p in perms:
            contigs, cols = [], []
            for k, si in enumerate(p):
                nb = 2001 + 2 * k + (k & 1) * 0 + (1 if k != 2 else 0)          # odd and even bin counts: the padded accumulator offset
                contigs.append(("g%d" % k, z * nb - (k * (z // 4 + 1)) % z))       # a different end_bin_size on every contig
                cols.append(pattern_reads(sizes[si], z, nb - 1 - k, 3 * k + si))
                if k == 1:
                    contigs.append(("empty", 0))                                    # a contig of length 0 between real ones
                    cols.append(_cols([], []))
            _case("g_sizes_%s_z%d" % ("".join(map(str, p)), z), "G", z, contigs, cols, min_q=10, layouts=("arrays_multi", "packed", "binned"),
                  paths=("register",))
        for k_items in (1, 2, 3, 9):
            nb = 900
            contigs = [("m%d" % k, z * (nb + 3 * k) - (k * 3) % z) for k in range(min(k_items, 5))]
            cols = [pattern_reads(700 + 41 * k, z, nb - 2, k) for k in range(len(contigs))]
            items = [(k % len(contigs), (k // len(contigs)) * 350, min((k // len(contigs) + 1) * 350, 700 + 41 * (k % len(contigs))))
                     for k in range(k_items)] if k_items == 9 else None
            if items:                                                               # 9 items over 5 contigs: the first four come in two slices
                items = [(ci, lo, hi if (k + len(contigs)) < k_items else len(cols[ci][0])) for k, (ci, lo, hi) in enumerate(items)]
            _case("g_items%d_z%d" % (k_items, z), "G", z, contigs, cols, min_q=10, items=items, layouts=("arrays_multi", "packed", "binned"))


# ---------------------------------------------------------------------------------------------------------------- H: call-to-call state
def state_sequence():
    """steps on ONE histogram (z = 50, one contig): (what, case name, layout).  push, push, finish (twice: the same bins); reset, then
    another layout; a refused push, reset, a clean result"""
    return [("push", "h_state_a", "arrays"), ("push", "h_state_b", "packed"), ("finish", ("h_state_a", "h_state_b"), None),
            ("finish", ("h_state_a", "h_state_b"), None), ("reset", None, None), ("push", "h_state_b", "binned"), ("finish", ("h_state_b",), None),
            ("reset", None, None), ("push", "h_state_bad", "arrays_multi"), ("finish_error", TDT_E_RANGE, None), ("reset", None, None),
            ("push", "h_state_a", "host"), ("finish", ("h_state_a",), None)]


def _family_h():
    z, LN = 50, 50 * 3000 + 17
    _case("h_state_a", "H", z, [("c", LN)], [pattern_reads(2 * THREADS * RPL1 + 5, z, 2990, 1)], min_q=10)
    _case("h_state_b", "H", z, [("c", LN)], [pattern_reads(RPB + 9, z, 2990, 2)], min_q=10)
    s = np.array([10, 20, LN - 10, 30])
    _case("h_state_bad", "H", z, [("c", LN)], [_cols(s, s + 100)], min_q=10, expect=TDT_E_RANGE, paths=("refused",))


for _f in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f, _family_g, _family_h):
    _f()
N_CASES = len(_ORDER)
N_PAIRS = sum(n_pairs(CASES[n]) for n in _ORDER)
# the families each departure of the restatement must show up in (test_coverage_stage_refs_cpu.py)
MUTANT_FAMILIES = {"no_one_short": "ABCDFG", "z_in_last_bin": "D", "end_bin_size_for_single": "D", "mapq_gt": "E", "ignore_duplicate": "ECG",
                   "interior_short": "ABDF", "interior_long": "ABDF"}
