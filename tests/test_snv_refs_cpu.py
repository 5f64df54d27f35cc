"""The definition of ``TIDDIT_SNVS`` (tiddit_amd/tiddit_snvs.py) on the CPU: its per-read loop against an independent restatement in
numpy (a read's ``M = X`` operations expanded to index arrays, whole arrays compared; written from the specification, not from the
loop) on every aimed case of tests/snv_cases.py and on the generated file of tests/scan_all_cases.py; every case's claim; a list of
one-line departures of the restatement, each noticed inside the family named for it; the switch and the file; and an anchor that comes
from neither: ``tiddit_alleles.count_batch`` counts the alternative base at the rows the definition reports.

Every test of this file fails on the parent commit: the module does not exist there."""
import collections
import struct

import numpy as np
import pytest

import scan_all_cases as C
import snv_cases as D

MUTANTS = {"nibble_swap": "phase", "p_is_r": "phase", "le_B": "quality", "ff_low": "quality", "cap9": "cap", "end_ge": "ends", "x_skipped": "ops",
           "n_stays": "ops", "s_moves": "ops", "nostrand": "sets"}
_ACGT = np.full(16, -1, dtype=np.int64)
_ACGT[[1, 2, 4, 8]] = [0, 1, 2, 3]


def _among(codes):
    """op code -> is it one of ``codes`` (a lookup table: a CIGAR's op codes are 0 ... 15)"""
    t = np.zeros(16, dtype=bool)
    t[list(codes)] = True
    return t


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def restate_batch(b, ref, Q, B, keys, sn, mutant=None, kinds=None):
    """``ref``: {tid: uint8 codes}.  Appends (K1, K2) to keys, adds to the Counter sn"""
    raw = np.ascontiguousarray(b.raw, dtype=np.uint8)
    mem = raw.tobytes()
    match_ops = _among((0, 7) if mutant == "x_skipped" else (0, 7, 8))
    ref_ops = _among({"n_stays": (0, 2, 7, 8), "s_moves": (0, 2, 3, 4, 7, 8)}.get(mutant, (0, 2, 3, 7, 8)))
    spans_ref, spans_query, aligned_ops = _among((0, 2, 3, 7, 8)), _among((0, 1, 4, 7, 8)), _among((0, 7, 8))
    for i in range(len(b)):
        flag, tid, pos, mapq, ro = (int(getattr(b, k)[i]) for k in D.COLUMNS)
        sn["records"] += 1
        kind = None
        if flag & (0x4 | 0x100 | 0x200 | 0x400 | 0x800) or tid < 0 or mapq < Q:
            if kinds is not None:
                kinds.append(D.NOT_ELIGIBLE)
            continue
        sn["eligible"] += 1
        ok = tid < 2 ** 24 and pos >= 0 and len(mem) - ro >= 36
        if ok:
            bs, _, _, l_name, _, _, n_cig, _, l_seq, _, _, _ = struct.unpack_from("<IiiBBHHHiiii", mem, ro)
            ok = l_seq >= 0 and 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq <= bs and ro + 4 + bs <= len(mem)
        if ok:
            at = ro + 36 + l_name
            words = np.frombuffer(mem, dtype="<u4", count=n_cig, offset=at).astype(np.int64)
            ops, lens = words & 15, words >> 4
            on_ref, on_query = spans_ref[ops], spans_query[ops]
            ok = not (ops > 8).any() and pos + int(lens[on_ref].sum()) <= 2 ** 31 - 1
            ok = ok and not (l_seq >= 1 and n_cig >= 1 and int(lens[on_query].sum()) != l_seq)
        if not ok:
            kind = D.MALFORMED
            sn["malformed"] += 1
        elif n_cig == 0 or l_seq == 0:
            kind = D.NO_SEQUENCE
            sn["no_sequence"] += 1
        else:
            span = int(lens[on_ref].sum())
            contig = ref.get(tid)
            if contig is None or (pos + span >= len(contig) if mutant == "end_ge" else pos + span > len(contig)):
                kind = D.OFF_REFERENCE
                sn["off_reference"] += 1
        if kind is not None:
            if kinds is not None:
                kinds.append(kind)
            continue
        moves_r = ref_ops[ops]
        r0 = pos + np.concatenate([[0], np.cumsum(np.where(moves_r, lens, 0))[:-1]])
        q0 = np.concatenate([[0], np.cumsum(np.where(on_query, lens, 0))[:-1]])
        m = match_ops[ops]
        if not m.any():
            qi = ri = np.zeros(0, dtype=np.int64)
        else:
            within = np.concatenate([np.arange(n) for n in lens[m]])
            qi, ri = np.repeat(q0[m], lens[m]) + within, np.repeat(r0[m], lens[m]) + within
        seq = at + 4 * n_cig
        packed = raw[seq:seq + (l_seq + 1) // 2]
        pair = (packed & 15, packed >> 4) if mutant == "nibble_swap" else (packed >> 4, packed & 15)
        nib = np.stack(pair, axis=1).ravel()[:l_seq]
        qv = raw[seq + (l_seq + 1) // 2:seq + (l_seq + 1) // 2 + l_seq].astype(np.int64)
        inside = ri < len(contig)                                  # (only a mutant walks off the contig)
        qi, ri = qi[inside], ri[inside]
        c, g = nib[qi].astype(np.int64), contig[ri].astype(np.int64)
        mis = (_ACGT[c] >= 0) & (_ACGT[g] >= 0) & (c != g)
        q = qv[qi]
        low = mis & ((q == 255) | (q < B) if mutant == "ff_low" else (q != 255) & ((q <= B) if mutant == "le_B" else (q < B)))
        ev = mis & ~low
        sn["aligned_bases"] += int(lens[aligned_ops[ops]].sum())
        sn["low_quality"] += int(low.sum())
        n = int(ev.sum())
        if n > (9 if mutant == "cap9" else 8):
            sn["noisy_reads"] += 1
            if kinds is not None:
                kinds.append(D.NOISY)
            continue
        if kinds is not None:
            kinds.append(D.OK)
        if n:
            sn["reads_with_events"] += 1
            sn["mismatches"] += n
            P = ri[ev] + (0 if mutant == "p_is_r" else 1)
            rev = 0 if mutant == "nostrand" else (flag >> 4) & 1
            k2 = _ACGT[g[ev]] * 8 + _ACGT[c[ev]] * 2 + rev
            keys.extend(zip((tid * 2 ** 32 + P).tolist(), k2.tolist()))


def restatement(case, mutant=None):
    ref = {t: v for t, v in D.host_reference().contigs.items()}
    keys, sn = [], collections.Counter()
    for b in D.batches(case):
        restate_batch(b, ref, case["Q"], case["B"], keys, sn, mutant)
    sn = {k: v for k, v in sn.items() if v}
    out = {}
    for S in case["S"]:
        distinct, rows = D.sets_of(keys, S)
        out[S] = (D.counters_of(sn, distinct, len(rows)), D.row_columns(rows))
    return D.key_rows(keys), out


# ---- the aimed cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_claim_definition_and_restatement_agree(case):
    claim, loop, arrays = D.expected(case), D.definition(case), restatement(case)
    assert D.same(claim, loop), "the definition departs from the claim: " + case["claims"]
    assert D.same(claim, arrays), "the restatement departs from the claim: " + case["claims"]


def test_the_families_and_what_they_hold():
    assert len(D.CASES) == D.N_CASES == 26
    assert {c["family"] for c in D.CASES} == set(D.FAMILIES)
    every = [r for c in D.CASES for reads, _ in c["batches"] for r in reads]
    assert {r["kind"] for r in every} == {D.NOT_ELIGIBLE, D.MALFORMED, D.NO_SEQUENCE, D.OFF_REFERENCE, D.NOISY, D.OK}
    sizes = sorted({len(reads) for c in D.CASES if c["family"] == "workgroups" for reads, _ in c["batches"]})
    assert sizes == [D.SNV_BLOCK - 1, D.SNV_BLOCK, D.SNV_BLOCK + 1, 2 * D.SNV_BLOCK - 1, 2 * D.SNV_BLOCK, 2 * D.SNV_BLOCK + 1]
    runs = collections.Counter(k for k, _ in D.claimed(next(c for c in D.CASES if c["name"].startswith("sets: runs")))[0])
    assert sorted(runs.values()) == [D.KS_TILE - 1, D.KS_TILE, D.KS_TILE + 1]
    grown = next(c for c in D.CASES if c["family"] == "store")
    assert grown["capacity"] == 64 and len(D.claimed(grown)[0]) > 3 * 64
    src = open(D.__file__.replace("tests/snv_cases.py", "tiddit_amd/csrc/tdt_snv.hip")).read()
    assert "#define SNV_K_TILE %d " % D.SNV_BLOCK in src
    assert "#define KS_TILE %d " % D.KS_TILE in open(D.__file__.replace("tests/snv_cases.py", "tiddit_amd/csrc/tdt_keystore.h")).read()


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_departure_is_noticed_in_its_family(mutant):
    family = [c for c in D.CASES if c["family"] == MUTANTS[mutant]]
    assert family
    assert any(not D.same(D.expected(c), restatement(c, mutant)) for c in family), mutant


# ---- the generated file ---------------------------------------------------------------------------------------------------------
Q, B, S = 20, 20, 2


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    from tiddit_amd import tiddit_snvs
    d = str(tmp_path_factory.mktemp("snv_scan_all"))
    info = C.generate(d)
    batches = C.host_batches(C.paths(d)[0])
    ref = C.host_reference()
    keys, sn, kinds = [], {}, []
    for b in batches:
        tiddit_snvs.keys_of_batch_by_read(b, keys, sn, ref, Q, B, kinds)
    return d, info, batches, ref, keys, sn, kinds


def test_the_definition_equals_the_restatement_on_the_generated_file(made):
    d, info, batches, ref, keys, sn, kinds = made
    keys2, sn2, kinds2 = [], collections.Counter(), []
    for b in batches:
        restate_batch(b, ref.contigs, Q, B, keys2, sn2, kinds=kinds2)
    assert kinds == kinds2
    assert {k: v for k, v in sn2.items() if v} == sn
    assert np.array_equal(D.key_rows(keys), D.key_rows(keys2))
    assert sn["records"] == info["n_records"] and sn["mismatches"] == len(keys) > 1000 and sn.get("malformed", 0) == 0
    assert sn["aligned_bases"] > 50 * sn["eligible"]


def test_planted_heterozygous_sites_are_rows_with_the_support_the_allele_counter_counts(made, tmp_path):
    """the anchor on the generated file: at every planted heterozygous site whose alternative base ``tiddit_alleles.count_batch`` counts
    S times or more, the definition reports a row with exactly that SUPPORT — unless a read the definition calls noisy, malformed or
    off the reference lies over the site (the allele counter counts that read, the SNV definition drops it)"""
    from tiddit_amd import tiddit_alleles, tiddit_snvs
    d, info, batches, ref, keys, sn, kinds = made
    table_ = C.contigs()
    names, lengths = [n for n, _ in table_], [l for _, l in table_]
    counts, rows = tiddit_snvs.summarise(keys, sn, S)
    by_site = {(k1, k2): sup for k1, k2, sup, _ in rows}
    sites = tiddit_alleles.read_sites(C.paths(d)[2], names, lengths)
    table, stats = np.zeros((len(sites), 8), dtype=np.int64), [0, 0]
    dropped, at = [], 0
    for b in batches:
        tiddit_alleles.count_batch(table, stats, sites.site_pos, sites.site_off, b, Q, B)
        for i in range(len(b)):
            if kinds[at + i] in (D.NOISY, D.MALFORMED, D.OFF_REFERENCE):
                dropped.append((int(b.tid[i]), int(b.pos[i]), int(b.end[i])))
        at += len(b)
    checked = excluded = 0
    for (chrom, pos1, r, a, k), (tid, p0, _, _, het) in zip(sites.rows, info["sites"]):
        assert pos1 == p0 + 1
        n_alt = int(table[k][tiddit_alleles.COLUMNS.index(a)])
        if not het or n_alt < S:
            continue
        if any(t == tid and lo <= p0 < hi for t, lo, hi in dropped):
            excluded += 1
            continue
        checked += 1
        assert by_site.get((D.K1(tid, pos1), D.K2(r, a))) == n_alt, (chrom, pos1, r, a, n_alt)
    print("planted heterozygous sites checked: %d, excluded because a dropped read lies over them: %d" % (checked, excluded))
    assert checked > 0


# ---- the anchor on the aimed cases ----------------------------------------------------------------------------------------------
def test_the_written_rows_are_a_sites_file_and_the_allele_counter_counts_their_support(tmp_path):
    from tiddit_amd import tiddit_alleles, tiddit_snvs
    clean = [c for c in D.CASES if c["clean"]]
    assert len(clean) >= 15
    ref = D.host_reference()
    total = 0
    for n, case in enumerate(clean):
        keys, sn = [], {}
        for b in D.batches(case):
            tiddit_snvs.keys_of_batch_by_read(b, keys, sn, ref, case["Q"], case["B"])
        assert not any(sn.get(k) for k in ("malformed", "noisy_reads", "off_reference")), case["name"]
        counts, rows = tiddit_snvs.summarise(keys, sn, 1)
        path = str(tmp_path / ("case%d.snvs.tab" % n))
        tiddit_snvs.write_file(path, counts, rows, D.NAMES, None, 1, case["Q"], case["B"])
        sites = tiddit_alleles.read_sites(path, D.NAMES, D.LENGTHS)
        assert len(sites.rows) == len(rows) and sites.skipped == {"unknown contig": 0, "position outside the contig": 0, "not a biallelic SNV": 12}
        table, stats = np.zeros((len(sites), 8), dtype=np.int64), [0, 0]
        for b in D.batches(case):
            tiddit_alleles.count_batch(table, stats, sites.site_pos, sites.site_off, b, case["Q"], case["B"])
        assert stats[1] == 0
        for (chrom, pos1, r, a, k), (k1, k2, sup, rev) in zip(sites.rows, rows):
            assert (D.NAMES.index(chrom), pos1, r, a) == (k1 >> 32, k1 & 0xffffffff, "ACGT"[(k2 >> 3) & 3], "ACGT"[(k2 >> 1) & 3])
            assert int(table[k][tiddit_alleles.COLUMNS.index(a)]) == sup, (case["name"], chrom, pos1, r, a)
        total += len(rows)
    assert total > 400 and tiddit_alleles.FLAG_MASK == 0xF04


# ---- the switch and the file ----------------------------------------------------------------------------------------------------
def test_parse_switch():
    from tiddit_amd.tiddit_snvs import parse_switch
    assert parse_switch(None) is None and parse_switch("") is None
    assert parse_switch("1") == (3, 20, 20) and parse_switch("1:20") == (1, 20, 20) and parse_switch("2") == (2, 20, 20)
    assert parse_switch("5:0") == (5, 0, 20) and parse_switch("1000000:255:93") == (10 ** 6, 255, 93) and parse_switch("7:30:0") == (7, 30, 0)
    for bad, text in (("0", "the minimum support is 1 ... 10^6"), ("1000001", "the minimum support is 1 ... 10^6"), ("2:256", "the minimum MAPQ is 0 ... 255"),
                      ("2:20:94", "the minimum base quality is 0 ... 93")):
        with pytest.raises(ValueError, match="^" + text.replace(".", r"\.").replace("^", r"\^") + "$"):
            parse_switch(bad)
    for bad in ("yes", "2:", ":20", "2:20:20:20", "-1", "2:-1", " 2", "2 ", "1.5", "2:20:", "1234567890", "٢", "+2", "2;20"):
        with pytest.raises(ValueError, match="the switch is 1, S, S:Q or S:Q:B"):
            parse_switch(bad)


def test_write_file_and_summary_line(tmp_path):
    from tiddit_amd import tiddit_snvs
    counts = np.arange(101, 113, dtype=np.uint64)
    rows = [(D.K1(0, 7), D.K2("A", "G"), 5, 2), (D.K1(0, 7), D.K2("A", "T"), 3, 3), (D.K1(1, 51), D.K2("T", "C"), 4, 0), (D.K1(2, 1), D.K2("C", "A"), 3, 1),
            (D.K1(5, 9), D.K2("G", "C"), 3, 1)]
    cover = {"one": np.array([10.0, 12.345]), "two": np.array([7.5])}
    path = str(tmp_path / "x.snvs.tab")
    tiddit_snvs.write_file(path, counts, rows, ["one", "two", "three"], cover, 3, 20, 13)
    assert open(path).read() == (
        "# tiddit_amd snvs v1 min_support=3 min_mapq=20 min_bq=13\n"
        "SN\trecords\t101\nSN\teligible\t102\nSN\tmalformed\t103\nSN\tno_sequence\t104\nSN\toff_reference\t105\nSN\taligned_bases\t106\n"
        "SN\tlow_quality\t107\nSN\tnoisy_reads\t108\nSN\treads_with_events\t109\nSN\tmismatches\t110\nSN\tdistinct_events\t111\nSN\treported_events\t112\n"
        "#CHROM\tPOS\tID\tREF\tALT\tSUPPORT\tFWD\tREV\tCOV\n"
        "one\t7\t.\tA\tG\t5\t3\t2\t10.00\n"
        "one\t7\t.\tA\tT\t3\t0\t3\t10.00\n"
        "two\t51\t.\tT\tC\t4\t4\t0\t.\n"
        "three\t1\t.\tC\tA\t3\t2\t1\t.\n"
        "5\t9\t.\tG\tC\t3\t2\t1\t.\n")
    cols = D.row_columns(rows)
    tiddit_snvs.write_file(path + "2", counts, cols, ["one", "two", "three"], cover, 3, 20, 13)
    assert open(path + "2").read() == open(path).read()
    assert tiddit_snvs.summary_line(counts) == ("snvs: 101 records, 102 eligible, 106 aligned bases, 110 mismatches, 111 distinct events, 112 reported, "
                                                "noisy reads 108, malformed records 103")
    assert tiddit_snvs.SN == D.SN and tiddit_snvs.SIZE == D.SIZE == 12 and tiddit_snvs.SNV_MAX_PER_READ == 8
