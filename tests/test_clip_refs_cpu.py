"""The clipped-read breakpoint sites without a GPU: the definition (tiddit_amd/tiddit_clips.py), an independent numpy restatement that
unpacks every sequence into one nibble array and works the sites out from the SORTED keys, and the claims of tests/clip_cases.py agree
on every case; one-line departures of the restatement are each noticed by a claim of the family listed for them; on the generated file
of tests/scan_all_cases.py the clips planted there for the signal predicates are rows at their planted positions; the result does not
depend on where the batches are cut; and the switch, the file and the summary line.

Every test of this file fails on the parent commit: the module does not exist there."""
import collections

import numpy as np
import pytest

import clip_cases as D
import scan_all_cases as C
from tiddit_amd import tiddit_clips

REF_CONSUMING, QUERY_CONSUMING = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def restated_keys(b, Q, L, mutant=None):
    """one batch -> ([(K1, K2)], Counter of the push counters), a record at a time over numpy views of its bytes"""
    raw = np.frombuffer(bytes(b.raw), dtype=np.uint8)
    keys, sn = [], collections.Counter()
    word = lambda o, dt: int(raw[o:o + np.dtype(dt).itemsize].view(dt)[0])
    for flag, tid, pos, mapq, ro in zip(*(np.asarray(getattr(b, k)).tolist() for k in D.COLUMNS)):
        sn["records"] += 1
        if flag & (0x4 | 0x100 | 0x200 | 0x400 | 0x800) or tid < 0 or mapq < Q:
            continue
        sn["eligible"] += 1
        ok = tid < 2 ** 24 and pos >= 0 and ro + 36 <= len(raw)
        if ok:
            block, l_name, nc, l_seq = word(ro, "<u4"), int(raw[ro + 12]), word(ro + 16, "<u2"), word(ro + 20, "<i4")
            ok = l_seq >= 0 and 32 + l_name + 4 * nc + (l_seq + 1) // 2 + l_seq <= block and ro + 4 + block <= len(raw)
        if ok:
            cig = raw[ro + 36 + l_name:ro + 36 + l_name + 4 * nc].view("<u4").astype(np.int64)
            ops, lens = cig & 15, cig >> 4
            reflen, qlen = int(lens[np.isin(ops, REF_CONSUMING)].sum()), int(lens[np.isin(ops, QUERY_CONSUMING)].sum())
            ok = not (ops > 8).any() and pos + reflen <= 2 ** 31 - 1 and not (l_seq >= 1 and nc >= 1 and qlen != l_seq)
        if not ok:
            sn["malformed"] += 1
            continue
        if nc == 0 or l_seq == 0:
            sn["no_sequence"] += 1
            continue
        if reflen == 0:
            sn["no_alignment"] += 1
            continue
        seq = raw[ro + 36 + l_name + 4 * nc:ro + 36 + l_name + 4 * nc + (l_seq + 1) // 2]
        nib = np.stack([seq >> 4, seq & 15], axis=1).ravel()[:l_seq]                   # every base's 4-bit code, in read order
        first = 1 if nc >= 2 and ops[0] == 5 else 0
        last = nc - 2 if nc >= 2 and ops[-1] == 5 else nc - 1
        clips = []
        if ops[first] == 4:
            clips.append((0, int(lens[first]), nib[:int(lens[first])] if mutant == "l_not_reversed" else nib[:int(lens[first])][::-1],
                          pos if mutant == "p_left_off" else pos + 1))
        elif mutant == "h_is_clip" and ops[0] == 5:
            clips.append((0, int(lens[0]), nib[:int(lens[0])][::-1], pos + 1))
        if ops[last] == 4:
            clips.append((1, int(lens[last]), nib[l_seq - int(lens[last]):], pos + reflen - 1 if mutant == "p_right_off" else pos + reflen))
        got = 0
        for side, cliplen, outward, P in clips:
            if cliplen <= L if mutant == "short_le" else cliplen < L:
                sn["short_clips"] += 1
                continue
            cols = outward[:27 if mutant == "cap27" else 28]
            good = np.isin(cols, (1, 2, 4, 8))
            n = len(cols) if good.all() else int(np.argmin(good))
            packed = sum(int(v) << (2 * j) for j, v in enumerate(np.log2(cols[:n].astype(np.float64)).astype(np.int64).tolist()))
            sn["cut_at_other_base"] += n < min(cliplen, 28)
            sn["left_clips" if side == 0 else "right_clips"] += 1
            rev = 0 if mutant == "rev_ignored" else flag >> 4 & 1
            keys.append((tid << 32 | P, side << 63 | n << 58 | packed << 2 | rev))
            got += 1
        sn["clipped_reads"] += got > 0
    return keys, sn


def restated_sites(keys, S, mutant=None):
    """every key of the job -> (the three set counters, the nine row columns), from the keys SORTED by (K1, K2)"""
    empty = tuple(np.zeros(0, dtype=dt) for dt in D.ROW_DTYPES)
    if not keys:
        return (0, 0, 0), empty
    k = np.array(keys, dtype=np.uint64).reshape(-1, 2)
    k = k[np.lexsort((k[:, 1], k[:, 0]))]
    k1, k2 = k[:, 0], k[:, 1]
    side = (k2 >> np.uint64(63)).astype(np.int64)
    new_seq = np.r_[True, (k1[1:] != k1[:-1]) | ((k2[1:] >> np.uint64(1)) != (k2[:-1] >> np.uint64(1)))]
    new_site = np.r_[True, (k1[1:] != k1[:-1]) | (side[1:] != side[:-1])]
    site = np.cumsum(new_site) - 1
    ns = int(site[-1]) + 1
    support = np.bincount(site, minlength=ns)
    rev = np.bincount(site, weights=(k2 & np.uint64(1)).astype(np.float64), minlength=ns).astype(np.int64)
    seqs = np.bincount(site, weights=new_seq.astype(np.float64), minlength=ns).astype(np.int64)
    n = ((k2 >> np.uint64(58)) & np.uint64(31)).astype(np.int64)
    votes = np.zeros((ns, 28, 4), dtype=np.int64)
    for j in range(28):
        m = n > j
        np.add.at(votes, (site[m], j, ((k2[m] >> np.uint64(2 + 2 * j)) & np.uint64(3)).astype(np.int64)), 1)
    depth = votes.sum(axis=2)
    deep = depth > S if mutant == "depth_gt" else depth >= S
    clen = np.cumprod(deep, axis=1).sum(axis=1)
    winner = 3 - votes[:, :, ::-1].argmax(axis=2) if mutant == "tie_larger" else votes.argmax(axis=2)
    inside = np.arange(28)[None, :] < clen[:, None]
    agree = (np.take_along_axis(votes, winner[:, :, None], axis=2)[:, :, 0] * inside).sum(axis=1)
    total = (depth * inside).sum(axis=1)
    cons = [sum(int(w) << (2 * j) for j, w in enumerate(row[:c].tolist())) for row, c in zip(winner, clen.tolist())]
    keep = support >= S
    heads = np.flatnonzero(new_site)
    cols = (k1[heads], side[heads], support, rev, seqs, clen, np.array(cons, dtype=np.uint64), agree, total)
    return (int(new_seq.sum()), ns, int(keep.sum())), tuple(np.asarray(c)[keep].astype(dt) for c, dt in zip(cols, D.ROW_DTYPES))


def restatement(case, mutant=None):
    """-> what clip_cases.definition gives, from the restatement"""
    keys, sn = [], collections.Counter()
    for b in D.batches(case):
        ks, s = restated_keys(b, case["Q"], case["L"], mutant)
        keys += ks
        sn.update(s)
    out = {}
    for S in case["S"]:
        sets, cols = restated_sites(keys, S, mutant)
        c = D.push_counters(+sn)
        c[10:13] = sets
        out[S] = (c, cols)
    return D.key_rows(keys), out


@pytest.fixture(scope="module")
def defined():
    return {c["name"]: D.definition(c) for c in D.CASES}


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_stated_ones():
    assert D.N_CASES == len(D.CASES) == 35 and len({c["name"] for c in D.CASES}) == 35
    assert {c["family"] for c in D.CASES} == {"length", "phase", "other", "hard", "both", "nothing", "malformed", "filter", "strand", "site", "vote", "depth",
                                              "support", "store"}
    assert all(c["claims"] for c in D.CASES)


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_definition_restatement_and_claim_agree(case, defined):
    d = defined[case["name"]]
    assert D.agrees_with_claim(case, d) is None, D.agrees_with_claim(case, d)
    r = restatement(case)
    assert D.agrees_with_claim(case, r) is None, D.agrees_with_claim(case, r)
    assert D.same(d, r)
    for S in case["S"]:
        assert [x.dtype for x in d[1][S][1]] == list(D.ROW_DTYPES)


def test_every_stated_kind_is_the_definitions_kind():
    for c in D.CASES:
        kinds, keys, sn = [], [], {}
        for b in D.batches(c):
            tiddit_clips.keys_of_batch_by_read(b, keys, sn, c["Q"], c["L"], kinds=kinds)
        assert kinds == [r["kind"] for reads, _ in c["batches"] for r in reads], c["name"]


MUTANTS = [("tie_larger", ("vote",)), ("depth_gt", ("depth",)), ("l_not_reversed", ("phase",)), ("p_left_off", ("site",)), ("p_right_off", ("site",)),
           ("h_is_clip", ("hard",)), ("cap27", ("length",)), ("rev_ignored", ("strand",)), ("short_le", ("length",))]


@pytest.mark.parametrize("mutant,families", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_a_one_line_departure_is_noticed_inside_its_family(mutant, families):
    noticed = [c["name"] for c in D.CASES if c["family"] in families and D.agrees_with_claim(c, restatement(c, mutant)) is not None]
    assert noticed, mutant


def test_the_order_of_the_reads_does_not_matter():
    case = next(c for c in D.CASES if c["family"] == "store")
    reads = [r for rs, _ in case["batches"] for r in rs]
    turned = dict(case, batches=[(reads[::-1], 0)])
    turned.pop("built", None)
    assert D.same(D.definition(case), D.definition(turned))


# ---- the generated file of scan_all_cases ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scanned(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("clip_all"))
    info = C.generate(d)
    bam = C.paths(d)[0]
    return info, bam, C.host_batches(bam)


def _over(batches, Q=20, L=10):
    keys, sn = [], {}
    for b in batches:
        tiddit_clips.keys_of_batch_by_read(b, keys, sn, Q, L)
    return keys, sn


def test_the_planted_clips_are_rows_at_their_planted_positions(scanned):
    info, bam, batches = scanned
    keys, sn = _over(batches)
    counts, rows = tiddit_clips.summarise(keys, sn, 1)
    at = {(r[0], r[1]): r for r in rows}
    lefts = rights = 0
    for k, tid, g in C.grid_points():
        if k % 4 == 0:                                          # 30S70M at g + 380, the clip 30 x G: an L site at the first aligned base
            r = at[(tid << 32 | (g + 381), 0)]
            lefts += 1
            if r[2] == 1:
                assert r[5:] == (28, D.literal_rows([(0, 0, 0, 0, 0, 0, 0, "G" * 28, 0, 0)])[0][6], 28, 28) and r[3] == 0 and r[4] == 1
        elif k % 4 == 1:                                        # 60M40S at g + 420, the clip 40 x A: an R site at the last aligned base
            r = at[(tid << 32 | (g + 480), 1)]
            rights += 1
            if r[2] == 1:
                assert r[5:] == (28, 0, 28, 28) and tiddit_clips.consensus_text(1, r[5], r[6]) == "A" * 28
    assert lefts == info["clip_reads"] > 10 and rights == info["split_reads"] > 10
    v = lambda k: int(counts[tiddit_clips.SN_INDEX[k]])
    assert v("records") == info["n_records"] and v("short_clips") > 0 and v("malformed") == 0
    assert v("left_clips") >= lefts and v("right_clips") >= rights and v("left_clips") + v("right_clips") == len(keys)
    assert v("reported_sites") == v("distinct_sites") == len(rows)
    # the restatement on the same batches
    rk, rs = [], collections.Counter()
    for b in batches:
        ks, s = restated_keys(b, 20, 10)
        rk += ks
        rs.update(s)
    assert sorted(rk) == sorted(keys) and dict(+rs) == sn
    for S in (1, 2, 3):
        c, rows = tiddit_clips.summarise(keys, sn, S)
        sets, cols = restated_sites(keys, S)
        assert tuple(int(x) for x in c[10:13]) == sets
        assert all(np.array_equal(x, y) for x, y in zip(D.row_columns(rows), cols))


def test_the_result_does_not_depend_on_where_the_batches_are_cut(scanned):
    info, bam, batches = scanned
    small = C.host_batches(bam, 1 << 16)
    assert len(small) > len(batches) > 1
    keys, sn = _over(batches)
    keys2, sn2 = _over(small)
    assert sn == sn2 and sorted(keys) == sorted(keys2)
    one = C.merged_batch(batches)
    keys3, sn3 = _over([one])
    assert sn == sn3 and keys == keys3


# ---- the switch, the file, the summary line -------------------------------------------------------------------------------------
def test_parse_switch():
    P = tiddit_clips.parse_switch
    assert P(None) is None and P("") is None
    assert P("1") == (3, 20, 10) and P("2") == (2, 20, 10) and P("1:20") == (1, 20, 10) and P("4:0") == (4, 0, 10) and P("5:255:65535") == (5, 255, 65535)
    assert P("1000000:7:1") == (10 ** 6, 7, 1)
    form = "the switch is 1, S, S:Q or S:Q:L (minimum support 1 ... 10^6, minimum MAPQ 0 ... 255, minimum clip length 1 ... 65535)"
    for bad, text in (("yes", form), ("1:2:3:4", form), ("-1", form), ("2:", form), (":2", form), ("1.5", form), ("٣", form), ("1" * 10, form),
                      ("0", "the minimum support is 1 ... 10^6"), ("1000001", "the minimum support is 1 ... 10^6"), ("2:256", "the minimum MAPQ is 0 ... 255"),
                      ("2:20:0", "the minimum clip length is 1 ... 65535"), ("2:20:65536", "the minimum clip length is 1 ... 65535")):
        with pytest.raises(ValueError) as e:
            P(bad)
        assert str(e.value) == text, bad


def test_write_file_and_summary_line(tmp_path):
    case = next(c for c in D.CASES if c["name"].startswith("phase"))
    keys, sn = _over(D.batches(case), case["Q"], case["L"])
    counts, rows = tiddit_clips.summarise(keys, sn, 1)
    cover = {"c0": np.arange(10, dtype=np.float64) + 0.125}
    for form in (rows, D.row_columns(rows)):
        path = str(tmp_path / "x.clips.tab")
        tiddit_clips.write_file(path, counts, form, ["c0", "c1"], cover, 1, 20, 10)
        lines = open(path).read().split("\n")
        assert lines[0] == "# tiddit_amd clips v1 min_support=1 min_mapq=20 min_clip=10 cols=28"
        assert lines[1:14] == ["SN\t%s\t%d" % (k, int(counts[i])) for i, k in enumerate(tiddit_clips.SN)]
        assert lines[14] == "#CHROM\tPOS\tSIDE\tSUPPORT\tFWD\tREV\tSEQS\tCLEN\tCONSENSUS\tAGREE\tTOTAL\tCOV"
        # an L site's consensus is written in reference direction: the clip as the read holds it
        assert lines[15] == "c0\t101\tL\t1\t1\t0\t1\t12\tACGTTGCAACGT\t12\t12\t2.12"
        assert lines[17] == "c0\t220\tR\t1\t1\t0\t1\t12\tCATGGTACCATG\t12\t12\t4.12"
        assert lines[19] == "c0\t301\tL\t1\t0\t1\t1\t12\tTTGCAACGTTGC\t12\t12\t6.12"
        assert lines[20] == "c0\t321\tR\t1\t0\t1\t1\t12\tGGATCCAATTGG\t12\t12\t6.12" and lines[21:] == [""]
    # no bins for the contig, a bin beyond them, a contig beyond the names, no column deep enough
    tiddit_clips.write_file(path, counts, [(5 << 32 | 7, 1, 2, 1, 2, 0, 0, 0, 0), (0 << 32 | 501, 0, 2, 0, 1, 1, 2, 2, 2)], ["c0", "c1"], cover, 3, 20, 10)
    lines = open(path).read().split("\n")
    assert lines[15:] == ["5\t7\tR\t2\t1\t1\t2\t0\t.\t0\t0\t.", "c0\t501\tL\t2\t2\t0\t1\t1\tG\t2\t2\t.", ""]
    assert tiddit_clips.summary_line(counts) == ("clips: 5 records, 5 eligible, 5 clipped reads, 3 left and 3 right clips, 6 distinct sites, 6 reported, short clips 0, "
                                                 "malformed records 0")
