"""Pins the references and generators of tests/sv_stage_cases.py on the CPU, so that test_gpu_sv_stages.py compares the kernels
with something that has itself been checked: the vectorised statistics reference against its literal per-read loop and against the
host C loop (tdt_stats_scan, csrc/tdt_bam.hip — host code, the library loads without a GPU); select_host against a literal per-read
transcription of the action rules; and every case family against the property it claims, so that a later edit of the generators
cannot quietly remove an edge."""
import ctypes

import numpy as np
import pytest

import sigtab_common
import sv_stage_cases as sc


@pytest.fixture(scope="module")
def lib():
    from tiddit_amd import _native, build
    build.build()
    return _native.load()


SMALL = [c for c in sc.stats_cases(large=False) if sum(len(b["tid"]) for b in c["batches"]) <= 12_000]
ALL = sc.stats_cases(large=True)


def test_case_counts():
    assert len(sc.stats_value_cases()) == len(sc.TLEN_FAMILIES) * len(sc.INSERT_LENGTHS) == 70
    assert len(sc.stats_cutoff_cases()) == len(sc.CUT_TARGETS) == 13
    assert len(ALL) == 70 + 13 + 2 + 2 and len(SMALL) >= 60
    assert len({c["name"] for c in ALL}) == len(ALL)
    assert len(sc.median_cases()) == len(sc.MEDIAN_FAMILIES) == 7


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_vectorised_statistics_equal_the_literal_loop(case):
    a = (case["batches"], case["n_reads"], case["min_mapq"], case["max_ins_len"])
    cv, iv = sc.stats_reference(*a)
    cl, il = sc.stats_loop(*a)
    assert cv == cl and np.array_equal(iv, il) and iv.dtype == il.dtype == np.int32


def _host_scan(lib, case):
    """the sampling loop in C over the case's batches, state carried over as tiddit_stats._statistics does"""
    from tiddit_amd import _native
    state = np.zeros(6, dtype=np.int64)
    chunks, done = [], []
    for b in case["batches"]:
        cols = [np.ascontiguousarray(b[k], dtype=sc._DT[k]) for k in sc.COLS]
        n = len(cols[0])
        out = np.empty(max(n, 1), dtype=np.int32)
        k = ctypes.c_size_t(0)
        _native.check(lib.tdt_stats_scan(*[_native.ptr(c) for c in cols], n, case["n_reads"], case["min_mapq"], case["max_ins_len"],
                                         _native.ptr(state), _native.ptr(out), ctypes.byref(k)))
        chunks.append(out[:k.value].copy())
        done.append(bool(state[5]))
    ins = np.concatenate(chunks)
    counters = dict(zip(("sampled", "sum_len", "n_len", "innie", "outtie"), (int(x) for x in state[:5])), n_ins=len(ins),
                    sum_ins=int(ins.astype(np.int64).sum()))
    return counters, ins, done


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_vectorised_statistics_equal_the_host_c_loop(lib, case):
    cv, iv = sc.stats_reference(case["batches"], case["n_reads"], case["min_mapq"], case["max_ins_len"])
    ch, ih, done = _host_scan(lib, case)
    assert cv == ch and np.array_equal(iv, ih)
    assert done == sc.done_flags(case["batches"], case["n_reads"])
    if case["figures"] and len(iv):
        # inside +-2^30 numpy's int32 interpolation does not wrap: the figures of the int32 list are those of the reference's Python ints
        wide = np.array(iv.tolist(), dtype=np.int64)
        assert sc.stats_figures(iv) == sc.stats_figures(wide) == sc.stats_figures(iv.tolist())
        assert np.abs(wide).max() <= 1 << 30


# ------------------------------------------------------------------------------------------------ the families' own claims
def _key_bytes(v):
    """the four bytes of the radix select's keys (sign-biased, top byte first)"""
    k = (np.atleast_1d(np.asarray(v, dtype=np.int64)) + (1 << 31)).astype(np.uint32)
    return np.stack([(k >> s) & 255 for s in (24, 16, 8, 0)], axis=1)


def test_insert_size_families_have_their_properties():
    for n in sc.INSERT_LENGTHS:
        k0, k1 = sc.percentile_ranks(n)
        assert len(np.unique(sc.tlen_family("equal", n, 1))) == 1
        s = np.sort(sc.tlen_family("two", n, 1))
        assert len(s) == n and (n == 1 or (s[k0] < 0 < s[k1] and _key_bytes(s[k0])[0, 0] != _key_bytes(s[k1])[0, 0]))
        for k in (1, 2, 3):
            b = _key_bytes(sc.tlen_family("top%d" % k, n, 1))
            assert all(len(np.unique(b[:, j])) == 1 for j in range(k))                      # the k top bytes agree ...
            assert n == 1 or len(np.unique(b[:, k])) > 1                                    # ... and byte k is the first that differs
        assert np.abs(sc.tlen_family("uniform", n, 1).astype(np.int64)).max() <= 1 << 30
    assert sc.tlen_family("top2", 100, 1).max() < 0 < sc.tlen_family("top1", 100, 1).min()
    # uniform: the percentile's two order statistics differ in the TOP byte in most lists, and in sign for some seed
    top_differs = sign_differs = 0
    for seed in range(300):
        s = np.sort(sc.tlen_family("uniform", 3, seed))
        k0, k1 = sc.percentile_ranks(3)
        top_differs += _key_bytes(s[k0])[0, 0] != _key_bytes(s[k1])[0, 0]
        sign_differs += (s[k0] < 0) != (s[k1] < 0)
    assert top_differs > 200 and sign_differs >= 1
    # ... and in the cases as they are run: both order statistics distinct, in different top-byte buckets, for the lists of the value cases
    seen = 0
    for c in sc.stats_value_cases():
        if c["name"].startswith("uniform-"):
            _, ins = sc.stats_reference(c["batches"], c["n_reads"], c["min_mapq"], c["max_ins_len"])
            s = np.sort(ins)
            k0, k1 = sc.percentile_ranks(len(s))
            seen += int(k1 > k0 and _key_bytes(s[k0])[0, 0] != _key_bytes(s[k1])[0, 0])
    assert seen >= 3
    f = sc.tlen_family("fixture", 8192, 1)
    assert 380 < f.mean() < 1000 and f.min() > 0 and f.max() < 1 << 17
    e = sc.stats_extreme_case()
    _, ins = sc.stats_reference(e["batches"], e["n_reads"], e["min_mapq"], e["max_ins_len"])
    s = np.sort(ins)
    assert len(s) == 1000 and s[0] == sc.I32_MIN and s[sc.percentile_ranks(1000)[1]] == sc.I32_MAX and not e["figures"]


def test_value_cases_have_the_list_lengths_and_sit_on_the_filter_edges():
    for c in sc.stats_value_cases():
        fam, L = c["name"].rsplit("-", 1)
        cnt, ins = sc.stats_reference(c["batches"], c["n_reads"], c["min_mapq"], c["max_ins_len"])
        assert cnt["n_ins"] == int(L) and np.array_equal(ins, sc.tlen_family(fam, int(L), 1000 + 37 * sc.TLEN_FAMILIES.index(fam) +
                                                                             sc.INSERT_LENGTHS.index(int(L))))
        assert int(ins.max()) == c["max_ins_len"]                                           # tlen == max_ins_len passes
        cols = sc._concat(c["batches"])
        assert (cols["tlen"].astype(np.int64) == c["max_ins_len"] + 1).any()                # ... and one more does not
    large = sc.stats_large_cases()
    assert [c["large"] for c in large] == [True, True]
    for c in large:
        sizes = [len(b["tid"]) for b in c["batches"]]
        assert set(sc.BATCH_SIZES) <= set(sizes) and 300 in sizes and (c["batches"][4]["tid"] == -1).all()
        cnt, ins = sc.stats_reference(c["batches"], c["n_reads"], c["min_mapq"], c["max_ins_len"])
        assert cnt["n_ins"] == sc.LARGE_INSERTS > 1_100_000


def test_every_filter_flips_one_step_past_its_edge():
    """each kind of failing read fails its ONE filter: moved back onto the edge it joins the list; each edge kind of passing read
    leaves the list when moved one step on"""
    case, kind = sc.stats_filter_case()
    a = (10 ** 9, case["min_mapq"], case["max_ins_len"])
    cols = sc._concat(case["batches"])
    base = sc.stats_reference([cols], *a)[0]["n_ins"]
    assert base == 400 and set(kind) == set(sc.FAIL_KINDS) | set(sc.PASS_KINDS)

    def n_ins(edit):
        c = {k: v.copy() for k, v in cols.items()}
        edit(c)
        return sc.stats_reference([c], *a)[0]["n_ins"]

    def setter(col, m, fn):
        def edit(c):
            c[col][m] = fn(c, m)
        return edit
    undo = {"mapq": ("mapq", lambda c, m: c["mapq"][m] + 1), "tlen": ("tlen", lambda c, m: c["tlen"][m] - 1),
            "mate_pos": ("mate_pos", lambda c, m: c["mate_pos"][m] + 1), "f0x8": ("flag", lambda c, m: c["flag"][m] & ~np.uint16(0x8)),
            "both_rev": ("flag", lambda c, m: c["flag"][m] & ~np.uint16(0x10)), "both_fwd": ("flag", lambda c, m: c["flag"][m] | np.uint16(0x20)),
            "f0x100": ("flag", lambda c, m: c["flag"][m] & ~np.uint16(0x100)), "f0x400": ("flag", lambda c, m: c["flag"][m] & ~np.uint16(0x400)),
            "f0x800": ("flag", lambda c, m: c["flag"][m] & ~np.uint16(0x800)), "mate_tid": ("mate_tid", lambda c, m: c["tid"][m]),
            "unplaced": ("tid", lambda c, m: c["mate_tid"][m])}
    assert set(undo) == set(sc.FAIL_KINDS)
    for k, (col, fn) in undo.items():
        m = kind == k
        assert m.sum() >= 2 and n_ins(setter(col, m, fn)) == base + m.sum(), k
    step = {"mapq_edge": ("mapq", lambda c, m: c["mapq"][m] - 1), "mate_pos_edge": ("mate_pos", lambda c, m: c["mate_pos"][m] - 1)}
    for k, (col, fn) in step.items():
        m = kind == k
        assert m.sum() >= 100 and (cols[col][m] == (case["min_mapq"] if k == "mapq_edge" else cols["pos"][m])).all()
        assert n_ins(setter(col, m, fn)) == base - m.sum(), k
    m = cols["tlen"].astype(np.int64) == case["max_ins_len"]
    assert n_ins(setter("tlen", m, lambda c, m: c["tlen"][m] + 1)) < base


def test_cutoff_cases_put_the_cut_where_they_say():
    cases = sc.stats_cutoff_cases()
    want = {"lane0": (0, 0), "lane63": (63, 63), "lane64": (0, 64), "tile_last": (63, 255), "tile_first": (0, 0)}
    for c in cases:
        name = c["name"][4:]
        sizes = [len(b["tid"]) for b in c["batches"]]
        assert sizes[:8] == [1000] * 8 and (c["batches"][4]["tid"] == -1).all()
        if c["cut"] is None:
            continue
        b, o = c["cut"]
        placed = np.concatenate([x["tid"] for x in c["batches"]]) >= 0
        g = 1000 * b + o                                                                  # the n_reads-th placed read, as a global index
        assert placed[g] and int(placed[:g + 1].sum()) == c["n_reads"]
        if name in want:
            assert (o % 64, o % 256) == want[name]
        if name == "batch_last":
            assert o == sizes[b] - 1
        if name in ("next_batch_first", "after_unplaced_batch"):
            assert o == 0
        if name == "before_unplaced_batch":
            assert (b, o) == (3, 999)
        if name == "after_unplaced_batch":
            assert b == 5
        # the loop breaks at the NEXT placed read: in the same batch, or — cut on a batch's last read — not before a later batch
        done = sc.done_flags(c["batches"], c["n_reads"])
        assert done.index(True) == (b if placed[1000 * b + o + 1:1000 * (b + 1)].any() else (b + 2 if name == "before_unplaced_batch" else b + 1))
    by = {c["name"][4:]: c for c in cases}
    total = int((sc._concat(by["zero"]["batches"])["tid"] >= 0).sum())
    assert (by["zero"]["n_reads"], by["one"]["n_reads"], by["exact_total"]["n_reads"]) == (0, 1, total) and by["beyond"]["n_reads"] > total
    assert sc.done_flags(by["zero"]["batches"], 0)[0] and not any(sc.done_flags(by["exact_total"]["batches"], total))
    c0, i0 = sc.stats_reference(by["zero"]["batches"], 0, sc.MIN_MAPQ, by["zero"]["max_ins_len"])
    assert (c0["sampled"], c0["n_len"], c0["n_ins"], len(i0)) == (1, 1, 0, 0)              # the first read still leaves its length behind


# ------------------------------------------------------------------------------------------------ the signal scan
@pytest.fixture(scope="module")
def scan_file(lib, tmp_path_factory):
    records, spans = sc.scan_records()
    path = sc.scan_batch(records, tmp_path_factory.mktemp("scan") / "scan.bam")
    return records, spans, path


def _host_batches(path):
    from tiddit_amd import bamio
    r = bamio.BamReader(path)
    out = list(r.batches())
    r.close()
    return out, r.lengths


@pytest.mark.parametrize("pi", range(len(sc.SCAN_PARAMS)))
def test_select_host_selects_what_the_literal_rules_select(scan_file, pi):
    records, spans, path = scan_file
    P = sc.SCAN_PARAMS[pi]
    assert len(sc.SCAN_PARAMS) == 3 and len(records) >= 40_000
    batches, lengths = _host_batches(path)
    assert lengths == [l for _, l in sc.SCAN_CONTIGS] and sum(len(b) for b in batches) == len(records)
    want = np.array([sc.record_action(r, P) for r in records], dtype=np.uint8)
    big = [l >= P["min_contig"] for l in lengths]
    o = 0
    for b in batches:
        meta, raw_end, raw = sigtab_common.select_host(b, big, P["min_q"], P["max_ins"], P["min_anchor_len"], P["min_clip_len"])
        w = want[o:o + len(b)]
        assert np.array_equal(meta["idx"], np.flatnonzero(w)) and np.array_equal(meta["action"], w[w != 0])
        assert len(raw_end) == len(meta) and (len(raw) == raw_end[-1] if len(meta) else len(raw) == 0)
        o += len(b)
    assert {2, 4, 8, 12, 6} <= set(want.tolist())


def test_scan_records_have_their_edges_and_densities():
    records, spans = sc.scan_records()
    E = sc.SCAN_EDGE
    act = np.array([sc.record_action(r, E) for r in records])
    # layout: selected reads at 4095 / 4096 / 4097 and nowhere before; an empty stretch that holds two whole tiles; a full one
    assert np.flatnonzero(act[:4098]).tolist() == [4095, 4096, 4097]
    lo, hi = spans["empty"]
    assert hi - lo > 2 * 4096 and not act[lo:hi].any() and (-(-lo // 4096) + 1) * 4096 <= hi
    lo, hi = spans["full"]
    assert hi - lo >= 4097 and act[lo:hi].all()
    assert len(records) >= 40_000 and len(records) // 4096 >= 10
    lo, hi = spans["mix"]
    assert 0.01 < (act[lo:hi] != 0).mean() < 0.06 and {r["tid"] for r in records[lo:hi]} == {0, 1}
    for n in (1023, 1024, 1025):
        assert sum(sc.record_action(r, E) != 0 for r in sc.scan_count_records(n)) == n
    # record sizes: the smallest legal record and the largest
    by = {r["label"]: r for r in records}
    s, l = by["smallest_selected"], by["largest_selected"]
    assert (len(s["qname"]), s["cigar"], s["seq"], s["tags"]) == (1, "", "", ()) and sc.record_action(s, E)
    assert len(l["qname"]) == 250 and len(l["seq"]) == 10_000 and sc.record_action(l, E) and not sc.record_action(by["largest_quiet"], E)
    # every comparison on its edge, flipping one step past it
    e = {r["label"]: sc.record_action(r, E) for r in sc.scan_edge_records()}
    for sign in ("+1", "-1"):
        assert [e["tlen%s*(max_ins%+d)" % (sign, d)] for d in (-1, 0, 1)] == [2, 0, 8]      # isz < max_ins clips, isz > max_ins is discordant
    assert e["tlen=int32_min"] == 8
    for side in ("left", "right"):
        assert [e["%s_clip%d_anchor%d" % (side, c, a)] for c in (0, 1) for a in (0, 1)] == [0, 0, 0, 2]
    assert e["cigar:150M"] == e["cigar:150S"] == e["cigar:none"] == 0 and e["cigar:none+discordant"] == 8
    assert e["cigar:40S20M5D85M"] == 2 and all(e["cigar:" + c] == 0 for c in ("10H40S100M", "40S100M10H", "40S110=", "110=40S", "40S100M10I",
                                                                                "10I100M40S", "40I110M", "40H110M", "110M40H", "40S60M40S"))
    assert (e["mapq-1_discordant"], e["mapq+0_discordant"]) == (0, 8) and (e["mapq-1_clip"], e["mapq+0_clip"]) == (0, 2)
    assert (e["mapq-1_sa"], e["mapq+0_sa"]) == (0, 4)
    assert (e["flag_base_discordant"], e["flag_base_mate_elsewhere"]) == (8, 8)
    for what, on in (("discordant", 8), ("mate_elsewhere", 8), ("clip", 2), ("sa", 4)):
        for bit in (0x4, 0x100, 0x400, 0x800):
            assert e["flag^0x%x_%s" % (bit, what)] == 0
        for bit in (0x1, 0x8):                                                              # read only by the discordant test
            assert e["flag^0x%x_%s" % (bit, what)] == (0 if on == 8 else on)
    assert (e["mate_tid=-1,0x8_clear"], e["mate_tid=-1,0x8_clear,sa"], e["mate_tid=-1,0x8_set"]) == (0, 4, 0)
    assert e["sa_first"] == e["sa_last"] == e["sa_middle"] == 4 and e["sa_only_as_text"] == 0 and e["sa_and_clip_and_discordant"] == 12
    assert e["small_contig_discordant"] == e["small_contig_clip"] == e["small_contig_sa"] == e["unplaced_with_sa"] == 0
    assert e["mate_on_small_contig"] == 8
    # the generated lengths ARE the parameters of SCAN_EDGE
    cig = {r["label"]: r["cigar"] for r in sc.scan_edge_records()}
    assert cig["left_clip0_anchor0"] == "%dS%dM" % (E["min_clip_len"], E["min_anchor_len"])
    assert cig["right_clip1_anchor1"] == "%dM%dS" % (E["min_anchor_len"] + 1, E["min_clip_len"] + 1)


def test_scan_file_decodes_to_its_records(scan_file):
    """the host decode of the file gives back the generated fields, the missing-CIGAR sentinel and the SA offsets"""
    records, spans, path = scan_file
    batches, _ = _host_batches(path)
    for k in ("tid", "mapq", "flag", "mate_tid", "tlen"):
        assert np.array_equal(np.concatenate([getattr(b, k) for b in batches]).astype(np.int64), np.array([r[k] for r in records], dtype=np.int64)), k
    first = np.concatenate([b.cigar_first for b in batches])
    assert np.array_equal(first == 0xffffffff, np.array([r["cigar"] == "" for r in records]))
    has_sa = np.concatenate([b.sa_off for b in batches]) >= 0
    assert np.array_equal(has_sa, np.array([any(t[0] == "SA" for t in r["tags"]) for r in records]))


# ------------------------------------------------------------------------------------------------ the medians
def _pattern_bytes(v):
    p = np.asarray(v, dtype=np.float64).view(np.uint64)
    return np.stack([(p >> np.uint64(s)) & np.uint64(255) for s in range(56, -8, -8)], axis=1)


def test_median_cases_have_their_properties():
    cases = {name: (cov, gc, seg) for name, cov, gc, seg in sc.median_cases()}
    assert list(cases) == list(sc.MEDIAN_FAMILIES)
    for name, (cov, gc, seg) in cases.items():
        ln = (seg[:, 1] - seg[:, 0]).tolist()
        assert set(sc.MEDIAN_LENGTHS) <= set(ln) and tuple(seg[-1]) == (0, len(cov)) and (seg[:, 0] >= 0).all() and (seg[:, 1] <= len(cov)).all()
        assert all(lo % 2 == 1 for lo, hi in seg[:-1] if name not in ("wide", "two") and hi - lo not in (0, len(cov)))
        order = np.argsort(seg[:, 0], kind="stable")
        assert (seg[order][1:, 0] < np.maximum.accumulate(seg[order][:-1, 1])).any()       # segments overlap
        med, cnt = sc.median_reference(cov, gc, seg)
        assert len(med) == len(seg) and np.isnan(med[np.array(ln) == 0]).all()
    cov, gc, seg = cases["equal"]
    assert len(np.unique(cov[cov > 0])) == 1
    cov, gc, seg = cases["two"]
    assert tuple(seg[0]) == (0, 2) and sc.median_reference(cov, gc, seg)[0][0] == 2.5 and set(np.unique(cov)) == {2.0, 3.0}
    cov, gc, seg = cases["wide"]
    assert cov.min() > 0 and cov.max() < 1e301 and ((cov < np.finfo(np.float64).tiny) & (cov > 0)).sum() > 100
    for k in range(8):                                                                     # ladder k is decided in byte k
        lo, hi = seg[k]
        b = _pattern_bytes(cov[lo:hi])
        assert hi - lo == 9 and all(len(np.unique(b[:, j])) == 1 for j in range(k)) and len(np.unique(b[:, k])) == 7 and not b[:, k + 1:].any()
        assert sc.median_reference(cov, gc, seg)[1][k] == 9 and np.array_equal(cov[lo:hi], sc.byte_ladder(k))
    assert len({tuple(r) for r in _pattern_bytes(cov)[:, :1].tolist()}) > 60               # the top byte spreads widely
    cov, gc, seg = cases["low_byte"]
    b = _pattern_bytes(cov)
    assert all(len(np.unique(b[:, j])) == 1 for j in range(7)) and len(np.unique(b[:, 7])) == 256
    cov, gc, seg = cases["dropped"]
    assert np.isnan(cov).sum() > 500 and (np.signbit(cov) & (cov == 0)).sum() > 500 and (cov < 0).sum() > 2000 and (cov > 0).sum() > 2000
    assert (np.signbit(cov) & np.isnan(cov)).any() and ((cov < 0) & (cov > -np.finfo(np.float64).tiny)).any()
    med, cnt = sc.median_reference(cov, gc, seg)
    assert cnt[-1] == ((cov > 0) & (gc != -1)).sum() and med[-1] > 0
    cov, gc, seg = cases["masked_segment"]
    med, cnt = sc.median_reference(cov, gc, seg)
    lo, hi = seg[5]
    assert hi - lo == 2048 and (gc[lo:hi] == -1).all() and (cov[lo:hi] > 0).all() and cnt[5] == 0 and np.isnan(med[5])
    assert len(cases["many_segments"][2]) > 3000
    parts, pseg = sc.median_parts(cov, gc, (1, 2049, 2049, 6145))
    assert [len(p[0]) for p in parts] == [1, 2048, 0, 4096, len(cov) - 6145] and tuple(pseg[-1]) == (0, len(cov))
