"""Aimed inputs, references and claimed properties for the clustering kernels (csrc/tdt_dbscan.hip and its two headers): the
tile-resident pass (route 1, csrc/tdt_dbscan_tile.h), the ballot-mask route it falls through to when an x-cluster has more than
DB_SMALL members (route 2, csrc/tdt_dbscan_fused.h) and the general multi-launch route for m > DBF_M_MAX (route 3).

Everything is deterministic.  The tile constants are read from the `#define` lines of the three sources when this module is imported,
so the cases stay on their edges when a constant is retuned.  A case is a dict:

  name, family            "A" tile geometry, "B" the 128 | 129 switch, "C" bucket boundaries, "D" values, "E" call-to-call state
  x, y                    int64 columns (each bucket in DBSCAN.main's input order), off = int64[nb + 1] bucket offsets
  eps, m, mode            mode 0: DBSCAN.main (x then y pass), mode 1: x_coordinate_clustering alone
  entries                 which entries take it: "device" (tdt_dbscan_device), "host" (tdt_dbscan, one bucket), "sort"
                          (tdt_sort_dbscan after a shuffle inside every bucket), "columns" (tdt_cluster_columns after the same
                          shuffle), "ylabels" (DBSCAN.y_coordinate_clustering on the reference's x labels)
  claim                   what the case is aimed at: largest x-cluster, indices where clusters start, the route, tiles and groups

The references: `reference(case, literal=True)` is the reference's run-labelling state machine in C (oracle/tiddit_oracle.c),
`literal=False` its closed form; tests/golden/dbscan_edges.npz holds what the real DBSCAN.py gives on the small cases.  They are pinned
against each other, and the claims against the literal labels, by test_cluster_stage_refs_cpu.py; test_gpu_cluster_stages.py compares
the kernels.  Test infrastructure only."""
import hashlib
import os
import re

import numpy as np

import oracle

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc")
_CONST_FILES = {"DT_NW": "tdt_dbscan_tile.h", "DT_T": "tdt_dbscan_tile.h", "DT_S": "tdt_dbscan_tile.h", "DT_GRP": "tdt_dbscan_tile.h",
                "DB_SMALL": "tdt_dbscan.hip", "DBF_M_MAX": "tdt_dbscan_fused.h", "DBF_TILE": "tdt_dbscan_fused.h",
                "DBM_INLINE_PREFIX_MAX": "tdt_dbscan_fused.h"}


def parse_constants(sources=None):
    """the `#define`s the cases are aimed at, evaluated from the text of the three sources (object-like macros of integers, other
    macros, + - * / and brackets); KeyError when one can no longer be read.  `sources`: file name -> text, for the test of this parser."""
    defs = {}
    for fn in sorted(set(_CONST_FILES.values())):
        text = sources[fn] if sources else open(os.path.join(_CSRC, fn)).read()
        for name, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+([A-Za-z_]\w*)[ \t]+([^\n]*?)[ \t]*(?://[^\n]*)?$", text, re.M):
            defs.setdefault((fn, name), body)                 # (the first definition: the one under #ifndef for a measurement macro)
            defs.setdefault(name, body)

    def value(name, depth=0):
        if name not in defs or depth > 8:
            raise KeyError("cannot parse #define %s" % name)
        expr = re.sub(r"[A-Za-z_]\w*", lambda h: str(value(h.group(0), depth + 1)), defs[name])
        if not re.fullmatch(r"[0-9()+\-*/ \t]+", expr):
            raise KeyError("#define %s is not an integer expression: %r" % (name, defs[name]))
        return int(eval(expr.replace("/", "//")))

    out = {}
    for name, fn in _CONST_FILES.items():
        if (fn, name) not in defs:
            raise KeyError("cannot parse #define %s in %s" % (name, fn))
        out[name] = value(name)
    if out["DT_S"] != out["DT_NW"] * 64 or out["DT_T"] != (out["DT_NW"] - 2) * 64:
        raise KeyError("the tile geometry no longer follows from DT_NW")
    return out


CONSTANTS = parse_constants()
DT_NW, DT_GRP, DB_SMALL, DBF_M_MAX = CONSTANTS["DT_NW"], CONSTANTS["DT_GRP"], CONSTANTS["DB_SMALL"], CONSTANTS["DBF_M_MAX"]
DBF_TILE, DBM_INLINE_PREFIX_MAX = CONSTANTS["DBF_TILE"], CONSTANTS["DBM_INLINE_PREFIX_MAX"]
DT_S, DT_T = CONSTANTS["DT_S"], CONSTANTS["DT_T"]

LITERAL_MAX = 300_000          # cases up to this many points are compared with the literal state machine
GOLDEN_MAX = 12_000            # cases up to this many points also have labels of the real DBSCAN.py in the fixture
EPS = 100                      # layouts: points of a stretch are 1 apart, stretches 10 * EPS apart; m <= 65 < EPS
GAP = 10 * EPS
TDT_E_UNSUPPORTED = -6


# ======================================================================================================= building blocks
# A layout is a list of items: ("c", k) a cluster of exactly k labelled members, ("g", g) g isolated points.  k + 1 points one apart
# give k members (the reference never labels the last point of a stretch) — except at the END of a bucket, where the slice of the last
# windows is cut short by the array end and the last point is labelled too: there a cluster of k members is k points (at_end).
Y_KINDS = ("equal", "two", "desc", "groups", "none", "one_plus", "scatter")


def _cluster_y(kind, npts, m, rng):
    """y of one stretch, chosen by what the y pass makes of it (eps = EPS): `equal` one sub-run of ties, `two` two alternating values
    EPS apart (two sub-runs if each has m members), `desc` descending by 1 (the stable order is the reverse index order), `groups`
    several groups 10 * EPS apart in shuffled order (many sub-runs, groups below m members none), `none` all 2 * EPS apart (no
    sub-run), `one_plus` one group and stragglers, `scatter` random within 3 * EPS"""
    i = np.arange(npts)
    if kind == "equal":
        return np.full(npts, 7)
    if kind == "two":
        return (i & 1) * EPS
    if kind == "desc":
        return npts - i
    if kind == "groups":
        g = rng.integers(0, max(2, npts // max(m, 2)), npts)
        return g * GAP + rng.integers(0, 3, npts)
    if kind == "none":
        return rng.permutation(npts) * 2 * EPS
    if kind == "one_plus":
        y = rng.integers(0, 5, npts)
        y[rng.random(npts) < 0.3] += 5 * EPS
        return y
    return rng.integers(0, 3 * EPS, npts)


def build_layout(items, m, seed=0, y_kind=None):
    """-> x, y (int64), starts (index of the first member of every cluster), sizes (members of every cluster)"""
    xs, ys, starts, sizes = [], [], [], []
    pos, idx = 0, 0
    for j, (what, k) in enumerate(items):
        rng = np.random.default_rng([seed, j])       # a stream per item: one more point in one cluster leaves the others as they were
        if what == "g":
            xs.append(pos + GAP * np.arange(k))
            ys.append(rng.integers(0, 50 * EPS, k))
            pos += GAP * k
            idx += k
            continue
        assert k >= m, (k, m)
        at_end = j == len(items) - 1
        npts = k if at_end else k + 1
        xs.append(pos + np.arange(npts))
        kind = y_kind or Y_KINDS[int(rng.integers(0, len(Y_KINDS)))]
        ys.append(_cluster_y(kind, npts, m, rng))
        starts.append(idx)
        sizes.append(k)
        pos += npts + GAP
        idx += npts
    cat = lambda v: np.concatenate(v).astype(np.int64) if v else np.zeros(0, np.int64)
    return cat(xs), cat(ys), starts, sizes


def filler(room, m, busy=True):
    """items filling exactly `room` points without a cluster above m + 1 members: small clusters between isolated points"""
    items, j = [], 0
    while room > 0:
        k = m + (j & 1)
        if busy and room >= k + 1 + 2 and j % 3 != 2:
            items.append(("c", k))
            room -= k + 1
        else:
            g = min(room, 1 + j % 5 if busy else room)
            items.append(("g", g))
            room -= g
        j += 1
    return items


def place(clusters, n, m, end_cluster=None):
    """a layout of n points with a cluster of k members starting on every (index, k) of `clusters` (ascending, not overlapping) and
    small filler in between; end_cluster = k: a cluster of k members ends on the last point of the array"""
    items, at = [], 0
    for index, k in clusters:
        assert index >= at, (index, at)
        items += filler(index - at, m)
        items.append(("c", k))
        at = index + k + 1
    tail = n - at - (end_cluster or 0)
    assert tail >= 0, (n, at)
    items += filler(tail, m)
    if end_cluster:
        if items and items[-1][0] == "c":            # two stretches need a gap: the filler ended on a cluster, turn it into points
            items[-1] = ("g", items[-1][1] + 1)
        items.append(("c", end_cluster))
    return items


def dense_starts(n):
    """a run start on every second position, the densest the x pass allows (the tile kernel sizes segA / segE by it): an UNSORTED x
    column — even positions 0, odd positions alternating +6 / -6 — with eps = 10, m = 2 gives the labels 0 0 1 1 2 2 ..."""
    i = np.arange(n)
    x = np.where(i & 1, np.where((i >> 1) & 1, -6, 6), 0).astype(np.int64)
    y = ((i * 7) % 23).astype(np.int64)
    return x, y


def route_of(m, largest):
    return 3 if m > DBF_M_MAX else (2 if largest > DB_SMALL else 1)


def _case(name, family, x, y, eps, m, off=None, mode=0, entries=None, starts=(), largest=None, route=None, note=""):
    x, y = np.ascontiguousarray(x, dtype=np.int64), np.ascontiguousarray(y, dtype=np.int64)
    n = len(x)
    off = np.array([0, n], dtype=np.int64) if off is None else np.ascontiguousarray(off, dtype=np.int64)
    nb = len(off) - 1
    sorted_x = all(bool((np.diff(x[off[b]:off[b + 1]]) >= 0).all()) for b in range(nb))
    if entries is None:
        entries = ["device"]
        if nb == 1:
            entries.append("host")
        if sorted_x and mode == 0 and float(eps) == int(eps):
            entries.append("sort")
            if n == 0 or (max(x.max(), y.max()) < (1 << 31) and min(x.min(), y.min()) >= -(1 << 31)):
                entries.append("columns")
        if family == "A" and nb == 1 and mode == 0:
            entries.append("ylabels")
    tiles = -(-n // DT_T)
    claim = {"largest": largest, "starts": sorted(int(s) for s in starts), "route": route, "tiles": tiles, "groups": -(-tiles // DT_GRP)}
    return {"name": name, "family": family, "x": x, "y": y, "off": off, "nb": nb, "n": n, "eps": eps, "m": int(m), "mode": int(mode),
            "entries": tuple(entries), "claim": claim, "sorted_x": sorted_x, "note": note}


# ============================================================================================================ references
def reference(case, literal=None, mode=None):
    """-> (labels float64[n], last_id int64[nb]) per bucket: ids restart per bucket, -1 for an empty bucket or one without a cluster.
    literal=None: the literal state machine up to LITERAL_MAX points, the closed form above."""
    literal = case["n"] <= LITERAL_MAX if literal is None else literal
    mode = case["mode"] if mode is None else mode
    return reference_columns(case["x"], case["y"], case["off"], case["eps"], case["m"], mode, literal)


def reference_columns(x, y, off, eps, m, mode, literal):
    lab, last = np.full(len(x), -1.0), np.full(len(off) - 1, -1, dtype=np.int64)
    for b in range(len(off) - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        if lo == hi:
            continue
        d = np.stack([x[lo:hi], y[lo:hi]], 1)
        xl, xid = oracle.x_coordinate_clustering(d, eps, m)
        if mode == 0:
            xl, xid = oracle.y_coordinate_clustering(d, eps, m, xid, xl, literal=literal)
        lab[lo:hi], last[b] = xl, xid
    return lab, last


def properties(case):
    """the claimed quantities computed from the literal x labels: largest x-cluster, the set of indices where a cluster starts"""
    xl, _ = reference(case, literal=True, mode=1)
    off, starts, largest = case["off"], set(), 0
    for b in range(case["nb"]):
        lo, hi = int(off[b]), int(off[b + 1])
        seg = xl[lo:hi]
        if not len(seg):
            continue
        first = np.flatnonzero((seg >= 0) & (np.concatenate([[-2.0], seg[:-1]]) != seg))
        starts.update((lo + first).tolist())
        if (seg >= 0).any():
            largest = max(largest, int(np.bincount(seg[seg >= 0].astype(np.int64)).max()))
    tiles = -(-case["n"] // DT_T)
    return {"largest": largest, "starts": starts, "route": route_of(case["m"], largest), "tiles": tiles, "groups": -(-tiles // DT_GRP)}


def window_distances(case):
    """the largest distance of every window of the two passes (what is compared with eps), as two sets — from the closed form's labels"""
    x, y, m, off = case["x"], case["y"], case["m"], case["off"]
    dx, dy = set(), set()
    xl, _ = reference(case, literal=False, mode=1)
    for b in range(case["nb"]):
        lo, hi = int(off[b]), int(off[b + 1])
        for i in range(lo, hi - m + 1):
            dx.add(int(np.abs(x[i + 1:min(i + m + 1, hi)] - x[i]).max()))
        seg = xl[lo:hi]
        for c in np.unique(seg[seg >= 0]):
            ys = np.sort(y[lo:hi][seg == c])
            if len(ys) >= m:
                dy.update((ys[m - 1:] - ys[:len(ys) - m + 1]).tolist())
    return dx, dy


def input_hash(case):
    h = hashlib.sha256()
    for a in (case["x"], case["y"], case["off"]):
        h.update(np.ascontiguousarray(a, dtype="<i8").tobytes())
    h.update(("%r %d %d" % (float(case["eps"]), case["m"], case["mode"])).encode())
    return h.hexdigest()[:16]


def in_golden(case):
    """the cases whose labels the real DBSCAN.py recorded in tests/golden/dbscan_edges.npz: every case of at most GOLDEN_MAX points,
    except that of the seam layouts — whose cross of member counts, m and tile offsets is large, while DBSCAN.py knows nothing of
    tiles — only the one-bucket layouts of offset -1 are recorded (every m, every member count).  This keeps the fixture below the
    largest one already in tests/golden."""
    name = case["name"]
    return case["n"] <= GOLDEN_MAX and (not name.startswith("a_seam_") or name.endswith("_o-1"))


def shuffled(case, seed=5):
    """the same points shuffled inside every bucket -> (x, y, want_perm): want_perm is the stable order by x per bucket, what
    tdt_sort_dbscan must return"""
    rng = np.random.default_rng(seed)
    x, y, off = case["x"].copy(), case["y"].copy(), case["off"]
    want = np.empty(case["n"], dtype=np.int64)
    for b in range(case["nb"]):
        lo, hi = int(off[b]), int(off[b + 1])
        p = rng.permutation(hi - lo)
        x[lo:hi], y[lo:hi] = x[lo:hi][p], y[lo:hi][p]
        want[lo:hi] = lo + np.argsort(x[lo:hi], kind="stable")
    return x, y, want


# ============================================================================================================== family A
A_MS = (2, 3, 4, 5, 63, 64)
A_SEAM_OFFSETS = (-65, -64, -2, -1, 0, 1)            # cluster starts on tile positions DT_T + o and 2 * DT_T + o
A_WORD_STARTS = (2 * 64 + 0, 6 * 64 + 1, 10 * 64 + 62, 14 * 64 + 63)       # word positions 0, 1, 62, 63 (tile 0, words 2, 6, 10, 14)


def a_member_counts(m):
    return sorted({k for k in (m, m + 1, 63, 64, 65, 127, 128) if k >= m})


def _a_seam(m, k, o, nb3):
    cl = [(s, k) for s in A_WORD_STARTS] + [(DT_T + o, k), (2 * DT_T + o, k)]
    n = 2 * DT_T + 1 + DB_SMALL + 1 + 40
    x, y, starts, sizes = build_layout(place(cl, n, m), m, seed=m * 1000 + k * 7 + o + 100)
    name = "a_seam_m%d_k%d_o%+d" % (m, k, o)
    if not nb3:
        return _case(name, "A", x, y, EPS, m, starts=[s for s, _ in cl], largest=max(k, m + 1), route=1)
    # the same points as the middle bucket of three: the first bucket is exactly one tile of points (ending on a cluster that ends on
    # the bucket's last point), the last one a short tail, so every claimed start keeps its tile position
    x0, y0, _, _ = build_layout(place([], DT_T, m, end_cluster=m + 2), m, seed=11)
    x2, y2, _, _ = build_layout(place([(3, m)], 100, m), m, seed=12)
    off = np.cumsum([0, DT_T, len(x), len(x2)])
    return _case(name + "_nb3", "A", np.concatenate([x0, x, x2]), np.concatenate([y0, y, y2]), EPS, m, off=off,
                 starts=[DT_T + s for s, _ in cl], largest=max(k, m + 2), route=1)


def _a_n(n, m=3):
    k = min(n, m + 4)
    x, y, _, _ = build_layout(place([], n, m, end_cluster=k if k >= m else None), m, seed=n)
    return _case("a_n%d_m%d" % (n, m), "A", x, y, EPS, m, starts=[n - k] if k >= m else [], largest=max(k, m + 1) if n > 2 * m + 4 else (k if k >= m else 0),
                 route=1, note="n on a tile / group edge; a cluster ends on the last point of the array")


def _a_tiny(n, m):
    x = np.arange(n)
    return _case("a_tiny_n%d_m%d" % (n, m), "A", x, np.zeros(n), EPS, m, starts=[0] if n >= m else [], largest=n if n >= m else 0, route=1,
                 note="n < m: nothing; n = m and n = m + 1: the cut-short last windows label every point")


def _a_tail_on_seam(m, k):
    x, y, _, _ = build_layout(place([(DT_T - k, k)], 2 * DT_T, m), m, seed=m + k)
    return _case("a_tail_on_seam_m%d_k%d" % (m, k), "A", x, y, EPS, m, starts=[DT_T - k], largest=max(k, m + 1), route=1,
                 note="the stretch's unlabelled last point is the first point of the next tile")


def _a_end_cluster(m, k):
    x, y, _, _ = build_layout(place([], DT_T + 10, m, end_cluster=k), m, seed=m * 3 + k)
    return _case("a_end_cluster_m%d_k%d" % (m, k), "A", x, y, EPS, m, starts=[DT_T + 10 - k], largest=max(k, m + 1), route=1,
                 note="a cluster that ends on the last point of the array, from the halo of tile 0 into tile 1")


def _a_dense(n):
    x, y = dense_starts(n)
    return _case("a_dense_starts_n%d" % n, "A", x, y, 10, 2, starts=list(range(0, n - 1, 2)), largest=2 + (n & 1), route=1,
                 note="a run start on every second position (unsorted x: no sorting entries; the cut-short last window labels an odd last point)")


A_NS = (DT_T - 1, DT_T, DT_T + 1, DT_S, DT_S + 1, DT_GRP * DT_T - 1, DT_GRP * DT_T, DT_GRP * DT_T + 1)


def _family_a():
    reg = {}
    for m in A_MS:
        for k in a_member_counts(m):
            for o in A_SEAM_OFFSETS:
                for nb3 in (False, True):
                    reg["a_seam_m%d_k%d_o%+d%s" % (m, k, o, "_nb3" if nb3 else "")] = (lambda m=m, k=k, o=o, nb3=nb3: _a_seam(m, k, o, nb3))
        for n in (m - 1, m, m + 1):
            reg["a_tiny_n%d_m%d" % (n, m)] = (lambda n=n, m=m: _a_tiny(n, m))
        for k in (m, DB_SMALL):
            reg["a_tail_on_seam_m%d_k%d" % (m, k)] = (lambda m=m, k=k: _a_tail_on_seam(m, k))
            reg["a_end_cluster_m%d_k%d" % (m, k)] = (lambda m=m, k=k: _a_end_cluster(m, k))
    for n in A_NS:
        reg["a_n%d_m3" % n] = (lambda n=n: _a_n(n))
    for n in (DT_T + 2, DT_S):
        reg["a_n%d_m64" % n] = (lambda n=n: _a_n(n, 64))
    for n in (3 * DT_T + 100, 3 * DT_T + 101, 4000):
        reg["a_dense_starts_n%d" % n] = (lambda n=n: _a_dense(n))
    return reg


# ============================================================================================================== family B
def _b_layout(big, where, m, n_other=3 * DT_T):
    """small clusters (at most DB_SMALL - 1 members) and ONE cluster of `big` members at the array's start, at its end or across the
    seam between tiles 0 and 1"""
    small = [(40 + 150 * j, DB_SMALL - 1 - j) for j in range(4)]
    if where == "start":
        cl = [(0, big)] + [(s + big + 10, k) for s, k in small]
        return place(cl, n_other + big + 1, m), 0
    if where == "end":
        return place(small, n_other + big, m, end_cluster=big), n_other
    at = DT_T - 60
    cl = [c for c in small if c[0] + c[1] + 1 < at] + [(at, big)] + [(at + big + 20 + s, k) for s, k in small]
    return place(cl, at + big + 1 + 20 + small[-1][0] + DB_SMALL + 1000, m), at


def _b_switch(where, big, m=3):
    items, at = _b_layout(big, where, m)
    x, y, _, _ = build_layout(items, m, seed=77)     # (the same seed: the 128 and the 129 variant differ by the one point)
    return _case("b_switch_%s_%d" % (where, big), "B", x, y, EPS, m, starts=[at], largest=big, route=route_of(m, big),
                 note="largest cluster %d members at the array's %s" % (big, where))


B_BIGS = (129, 4095, 4096, 4097, 30000)


def _b_mixed(big, m):
    lm = min(m, DBF_M_MAX)                         # m = 65 runs on the very points of m = 64
    items, at = _b_layout(big, "seam", lm)
    x, y, _, _ = build_layout(items, lm, seed=31)
    return _case("b_mixed_%d_m%d" % (big, m), "B", x, y, EPS, m, starts=[at], largest=big, route=route_of(m, big),
                 note="dby_rank and db_sort_large in one call (m = 65: route 3 on the same points)")


def _b_masks(m):
    items, at = _b_layout(DB_SMALL + 1, "seam", m, n_other=2 * DBF_TILE + 100)
    x, y, _, _ = build_layout(items, m, seed=m)
    return _case("b_masks_m%d" % m, "B", x, y, EPS, m, starts=[at], largest=DB_SMALL + 1, route=2,
                 note="one bucket: dbm_x_masks<%s>" % ("true" if m <= 4 else "false"))


def _b_tiles(ntiles, m=3):
    """more than `ntiles` tiles of route 2 with a cluster of DB_SMALL + 1 members in the middle of small ones"""
    n = ntiles * DBF_TILE + 321
    at = (n // 2 // DBF_TILE) * DBF_TILE - 50
    period = [("c", 100), ("g", 2), ("c", m), ("c", 57), ("g", 1)]
    plen = sum(k + 1 if w == "c" else k for w, k in period)
    items = period * (at // plen)
    items += [("g", at - plen * (at // plen))] if at % plen else []
    items.append(("c", DB_SMALL + 1))
    rest = n - at - DB_SMALL - 2
    items += period * (rest // plen)
    if rest % plen:
        items.append(("g", rest % plen))
    x, y, _, _ = build_layout(items, m, seed=ntiles)
    return _case("b_tiles%d" % ntiles, "B", x, y, EPS, m, starts=[at], largest=DB_SMALL + 1, route=2,
                 note="route 2 over %d tiles: %s" % (ntiles + 1, "tile_scan launches" if ntiles >= DBM_INLINE_PREFIX_MAX else "in-kernel prefixes"))


B_LARGE = "b_tiles%d" % DBM_INLINE_PREFIX_MAX         # the one case above LITERAL_MAX: closed form, its family pinned by b_tiles3 / b_tiles40


def _family_b():
    reg = {}
    for where in ("start", "end", "seam"):
        for big in (DB_SMALL, DB_SMALL + 1):
            reg["b_switch_%s_%d" % (where, big)] = (lambda where=where, big=big: _b_switch(where, big))
    for big in B_BIGS:
        for m in (3, DBF_M_MAX, DBF_M_MAX + 1):
            reg["b_mixed_%d_m%d" % (big, m)] = (lambda big=big, m=m: _b_mixed(big, m))
    for m in (2, 3, 4, 5):
        reg["b_masks_m%d" % m] = (lambda m=m: _b_masks(m))
    for nt in (3, 40, DBM_INLINE_PREFIX_MAX):
        reg["b_tiles%d" % nt] = (lambda nt=nt: _b_tiles(nt))
    return reg


# ============================================================================================================== family C
C_CUT_POSITIONS = (DT_T - 64, DT_T - 1, DT_T, DT_T + 1, DT_S - 1, DT_S)


def _stretch_y(total, m, seed):
    rng = np.random.default_rng(seed)
    return _cluster_y(Y_KINDS[seed % len(Y_KINDS)], total, m, rng)


def _c_cut(pos, m, mode):
    """ONE stretch of 2 * (m + 30) points that a bucket boundary on tile position `pos` cuts in two"""
    half = m + 30
    lo = pos - half
    x0, y0, _, _ = build_layout(filler(lo - 1, m), m, seed=pos)
    xs = x0.max() + GAP + np.arange(2 * half)
    x1, y1, _, _ = build_layout(filler(DT_T, m), m, seed=pos + 1)
    x = np.concatenate([x0, [x0.max() + 1], xs, xs.max() + GAP + x1])       # (one lone point so that the stretch starts on lo)
    y = np.concatenate([y0, [3], _stretch_y(2 * half, m, pos), y1])
    return _case("c_cut_p%d_m%d_mode%d" % (pos, m, mode), "C", x, y, EPS, m, off=[0, pos, len(x)], mode=mode, starts=[lo, pos], largest=half,
                 route=1, note="a bucket boundary on tile position %d inside one stretch" % pos)


def _c_tail(m, mode):
    """boundaries m - 1, m and m + 1 points before the end of a stretch and one ON a stretch's end: the window must stop at the
    bucket's end (and the cut-short last windows then label the bucket's last point)"""
    xs, ys, off, end = [], [], [0], 0
    for j, d in enumerate((m - 1, m, m + 1, 0, None)):           # (0: the bucket ends with the stretch and the next one begins far away)
        total = min(2 * m + 9, DB_SMALL - 4) + j
        xs.append(j * GAP + np.arange(total))
        ys.append(_stretch_y(total, m, j + m))
        end += total
        off.append(end - (d or 0))               # (the bucket that begins here runs on through the head of the next stretch)
    x, y = np.concatenate(xs), np.concatenate(ys)
    return _case("c_tail_m%d_mode%d" % (m, mode), "C", x, y, EPS, m, off=off, mode=mode, largest=None, route=1,
                 note="boundaries m - 1, m, m + 1 and 0 points before a stretch's end")


def _c_many(m, mode):
    """several hundred buckets of 0, 1, 2, m - 1, m, m + 1, m + 2 points packed into ONE tile of points one apart: every wave of 64
    positions holds many boundaries (the stepping branch of db_bucket_wave)"""
    sizes, tot, j = [], 0, 0
    cyc = (0, 1, 2, m - 1, m, m + 1, m + 2, 0, 0, m)
    while True:
        s = cyc[(j * 7 + j // 10) % len(cyc)]
        if tot + s > DT_T - 3:
            break
        sizes.append(s)
        tot += s
        j += 1
    x = np.arange(tot)
    y = (np.arange(tot) * 37) % 11 * (EPS // 4)
    return _case("c_many_m%d_mode%d" % (m, mode), "C", x, y, EPS, m, off=np.cumsum([0] + sizes), mode=mode, largest=m + 2, route=1,
                 note="%d buckets in one tile" % len(sizes))


def _c_empty(mode, m=3):
    """empty buckets first, last and several in a row on the seam; a bucket whose first point is a tile's first point and one whose
    first point is the tile's last owned position"""
    n = 3 * DT_T + 50
    x = np.arange(n) + (np.arange(n) // 37) * GAP            # stretches of 37 points
    y = (np.arange(n) * 13) % 7 * 40
    off = [0, 0, 0, 500, DT_T - 1, DT_T, DT_T, DT_T, DT_T, 2 * DT_T - 1, 2 * DT_T, 2 * DT_T + 1, n, n, n]
    return _case("c_empty_mode%d" % mode, "C", x, y, EPS, m, off=off, mode=mode, largest=36, route=1,
                 note="empty buckets first, last, four in a row on a seam; buckets starting on DT_T - 1, DT_T, 2 DT_T - 1, 2 DT_T")


def _c_route(m, mode):
    """bucket boundaries on routes 2 and 3: a stretch of 400 points cut on a fused-tile seam, empty buckets around"""
    n = 2 * DBF_TILE + 300
    x = np.arange(n) + (np.arange(n) // 400) * GAP
    y = (np.arange(n) * 29) % 17 * 30
    off = [0, 0, 100, DBF_TILE - 1, DBF_TILE, DBF_TILE, DBF_TILE + 1, n - 2, n, n]
    return _case("c_route_m%d_mode%d" % (m, mode), "C", x, y, EPS, m, off=off, mode=mode, largest=399, route=route_of(m, 399),
                 note="boundaries on a 4096-point seam on route %d" % route_of(m, 399))


def _family_c():
    reg = {}
    for mode in (0, 1):
        for pos in C_CUT_POSITIONS:
            for m in (3, DBF_M_MAX):
                reg["c_cut_p%d_m%d_mode%d" % (pos, m, mode)] = (lambda pos=pos, m=m, mode=mode: _c_cut(pos, m, mode))
        for m in (2, 3, 5, DBF_M_MAX):
            reg["c_tail_m%d_mode%d" % (m, mode)] = (lambda m=m, mode=mode: _c_tail(m, mode))
        for m in (2, 3, 5):
            reg["c_many_m%d_mode%d" % (m, mode)] = (lambda m=m, mode=mode: _c_many(m, mode))
        reg["c_empty_mode%d" % mode] = (lambda mode=mode: _c_empty(mode))
        for m in (3, DBF_M_MAX + 1):
            reg["c_route_m%d_mode%d" % (m, mode)] = (lambda m=m, mode=mode: _c_route(m, mode))
    return reg


# ============================================================================================================== family D
def _d_dist(m, E, eps, gaps, tag):
    """window distances of exactly E - 1, E and E + 1 in both passes: x steps of E // m + {-1, 0, 1}, y steps of E // (m - 1) +
    {-1, 0, 1} (assigned in shuffled order inside every stretch); the comparison with eps is strict"""
    rng = np.random.default_rng(E * 10 + m)
    n = 3000
    x = np.cumsum(E // m + rng.integers(-1, 2, n))
    y = np.cumsum(E // (m - 1) + rng.integers(-1, 2, n))
    x += (np.arange(n) // 50) * 100 * E
    if not gaps:                                     # one stretch of 200 points one apart sends the whole call to route 2
        x = np.concatenate([x, x.max() + 100 * E + np.arange(200)])
        y = np.concatenate([y, y.max() + (np.arange(200) * 7) % 50 * (E // 4)])
        n += 200
    for lo in range(0, 3000, 50):
        y[lo:lo + 50] = y[lo:lo + 50][rng.permutation(50)]
    ent = None if float(eps) == int(eps) else ["host", "sort", "columns"]
    return _case("d_dist_%s_m%d" % (tag, m), "D", x, y, eps, m, entries=ent, largest=None, route=None,
                 note="distances E - 1, E, E + 1 around eps = %r" % (eps,))


def _d_eps0():
    x, y, _, _ = build_layout(place([(100, 30)], 600, 3), 3, seed=1)
    return _case("d_eps0", "D", x, y, 0, 3, largest=0, route=1, note="nothing is < 0")


def _d_wide(n, eps):
    """coordinates spanning 0 .. 2^32 - 2 in both columns; eps = 2^32 - 1 is the largest 32-bit eps, anything above is the `wide` switch"""
    rng = np.random.default_rng(n)
    top = (1 << 32) - 2
    x = np.sort(np.concatenate([[0, top], rng.integers(0, top + 1, n - 2)]))
    y = np.concatenate([[top, 0], rng.integers(0, top + 1, n - 2)])
    return _case("d_wide_n%d_eps%d" % (n, eps), "D", x, y, eps, 3, entries=["device", "host", "sort"], largest=n, starts=[0], route=route_of(3, n),
                 note="every distance is below eps: one cluster of all points")


def _d_wide_below():
    top = (1 << 32) - 2
    return _case("d_wide_below", "D", [0, top // 2, top], [top, 0, 5], top, 2, entries=["device", "host", "sort"], largest=2, starts=[1], route=1,
                 note="eps = 2^32 - 2 = the span itself: the one distance equal to it, in the first window, does not qualify")


def _d_ties(kind, m):
    items = [("g", 3)]
    for j in range(40):
        items += [("c", m + (j * 5) % (DB_SMALL - m + 1)), ("g", j % 3)]
    x, y, _, _ = build_layout(items, m, seed=m, y_kind=kind)
    return _case("d_ties_%s_m%d" % (kind, m), "D", x, y, EPS, m, largest=None, route=1, note="y %s in every cluster" % kind)


def _d_straddle(m):
    """ties on the positions where a sub-run ends and the next begins: sorted y of a cluster is a, a, ..., then values that make the
    window fail, then ties again; members in an index order that differs from the y order"""
    rng = np.random.default_rng(m)
    items = [("g", 2)]
    for j in range(60):
        k = m + 2 + j % (3 * m + 5)
        items += [("c", k), ("g", 1 + j % 2)]
    x, y, starts, sizes = build_layout(items, m, seed=m)
    for s, k in zip(starts, sizes):
        v = np.repeat(np.arange(k // 2 + 2), 2)[:k + 1] * (EPS // max(m - 1, 1)) + np.repeat(rng.integers(0, 2, k // 2 + 2), 2)[:k + 1]
        y[s:s + k + 1] = v[rng.permutation(k + 1)]
    return _case("d_straddle_m%d" % m, "D", x, y, EPS, m, largest=None, route=1, note="pairs of equal y stepping by about eps / (m - 1)")


def _d_subruns(m):
    """clusters whose y pass yields 0, 1, 2 and many sub-runs, in that cycle: the extra ids of earlier clusters shift later ones"""
    items = []
    for j in range(80):
        items += [("c", min(DB_SMALL, (j % 4 + 1) * (m + 1) + j % 3)), ("g", 1)]
    x, y, starts, sizes = build_layout(items, m, seed=3)
    for j, (s, k) in enumerate(zip(starts, sizes)):
        want = j % 4                                   # sub-runs wanted
        if want == 0:
            y[s:s + k + 1] = np.arange(k + 1) * 2 * EPS
        else:
            groups = min(want if want < 3 else 99, (k + 1) // m)
            g = np.arange(k + 1) % groups
            y[s:s + k + 1] = g * GAP + (np.arange(k + 1) * 3) % 5
    return _case("d_subruns_m%d" % m, "D", x, y, EPS, m, largest=None, route=1, note="0, 1, 2, many sub-runs per cluster")


def _family_d():
    reg = {}
    for m in (2, 3):
        reg["d_dist_r1_m%d" % m] = (lambda m=m: _d_dist(m, 60, 60, True, "r1"))
        reg["d_dist_r2_m%d" % m] = (lambda m=m: _d_dist(m, 60, 60, False, "r2"))
        reg["d_dist_f395_m%d" % m] = (lambda m=m: _d_dist(m, 40, 39.5, True, "f395"))
        reg["d_dist_f400_m%d" % m] = (lambda m=m: _d_dist(m, 40, 40.0, True, "f400"))
    reg["d_eps0"] = _d_eps0
    for n in (100, 300):
        for eps in ((1 << 32) - 1, 1 << 32, 1 << 33):
            reg["d_wide_n%d_eps%d" % (n, eps)] = (lambda n=n, eps=eps: _d_wide(n, eps))
    reg["d_wide_below"] = _d_wide_below
    for m in (2, 3, 5):
        for kind in ("equal", "two", "desc"):
            reg["d_ties_%s_m%d" % (kind, m)] = (lambda kind=kind, m=m: _d_ties(kind, m))
        reg["d_straddle_m%d" % m] = (lambda m=m: _d_straddle(m))
        reg["d_subruns_m%d" % m] = (lambda m=m: _d_subruns(m))
    return reg


# ============================================================================================================== family E
def state_sequence():
    """the calls of the call-to-call state test, in order; every one is compared with the reference"""
    def generic(n, m=3, mode=0, seed=0):
        x, y, _, _ = build_layout(place([], n, m, end_cluster=m + 1), m, seed=seed + n)
        return _case("e_n%d_mode%d" % (n, mode), "E", x, y, EPS, m, mode=mode, entries=["device"], largest=m + 1, route=1)
    empty = _case("e_n0", "E", np.zeros(0), np.zeros(0), EPS, 3, entries=["device"], largest=0, route=1)
    return [generic(2 * DT_GRP * DT_T + 5000),                     # three groups of tiles
            generic(1000),                                         # one tile
            get("b_switch_seam_%d" % (DB_SMALL + 1)),              # falls through to route 2
            generic(1001),                                         # one tile again
            get("c_many_m3_mode0"),                                # several buckets
            empty,
            generic(DT_GRP * DT_T + 10),                           # two groups
            generic(3 * DT_T + 3, mode=1)]                         # x pass only


def state_prefix():
    x, y, _, _ = build_layout(place([], 5 * DT_T, 3), 3, seed=9)
    return _case("e_prefix", "E", x, y, EPS, 3, entries=["device"], largest=4, route=1)


# =============================================================================================================== registry
_REGISTRY = {"A": _family_a(), "B": _family_b(), "C": _family_c(), "D": _family_d()}
FAMILIES = tuple(_REGISTRY)
_CACHE = {}


def case_names(family=None):
    if family is None:
        return [n for f in FAMILIES for n in _REGISTRY[f]]
    return list(_REGISTRY[family])


def family_of(name):
    return next(f for f in FAMILIES if name in _REGISTRY[f])


def get(name):
    if name not in _CACHE:
        c = _REGISTRY[family_of(name)][name]()
        assert c["name"] == name, (name, c["name"])
        _CACHE[name] = c
    return _CACHE[name]


# What the GPU test must have run: cases, and (case, entry) pairs over families A - D (test_cluster_stage_refs_cpu.py holds the two
# numbers to the registry; the GPU test counts what it ran against them).
N_CASES = 602
N_PAIRS = 2360

# The one-line mutants of the restatement in test_cluster_stage_refs_cpu.py and the families in which each must be caught.
MUTANT_FAMILIES = {
    "x_le_eps": ("D",),                   # x pass: <= eps for < eps (only family D has distances equal to eps)
    "y_le_eps": ("D",),                   # y pass: <= eps for < eps
    "x_window_m_minus_1": ("A", "B", "C", "D"),
    "x_window_m_plus_1": ("A", "B", "C", "D"),
    "y_window_m_minus_2": ("A", "D"),
    "y_window_m": ("A", "D"),
    "x_stretch_longer": ("A", "B", "C"),  # a new run labels m + 1 points
    "x_stretch_shorter": ("A", "B", "C"),
    "y_stretch_longer": ("A", "D"),
    "y_stretch_shorter": ("A", "D"),
    "x_last_window_minus_1": ("A", "C"),  # range(n - m) for range(n - m + 1)
    "x_last_window_plus_1": ("A", "C"),
    "y_last_window_minus_1": ("A", "D"),
    "bucket_boundaries_ignored": ("C",),
    "ids_not_restarted": ("C",),
    "subrun1_renumbered": ("A", "D"),
    "extra_offset_dropped": ("A", "D"),
}
# `ties in y taken in reverse index order` is NOT in the table: it is an equivalent mutant.  The sorted y of a cluster is monotone,
# so if window i passes and y[i + 1] == y[i] then window i + 1 passes as well, and a run can neither start nor end between two equal
# values: the label of a sorted position is the same for all positions of equal y, whatever the order among them.  The CPU test asserts
# that equivalence on every small case (family D's tie cases included) instead of demanding a difference that cannot exist.
EQUIVALENT_MUTANTS = ("y_ties_reversed",)
