"""The references of the small-indel candidates agree before any kernel is asked (no GPU): on every aimed case of tests/indel_cases.py the
case's written claim, the struct / regex / Counter restatement, the definition (``tiddit_indels.events_of_read`` / ``summarise``) and its
whole-column form (``keys_of_batch``) give the same sorted keys, the same counter array and the same row columns for every stated
minimum support; every edge is where its case says it is; each one-line departure of the restatement changes the expected output inside
the family listed for it; the switch parser accepts and refuses what it should; the file writer gives a literal text."""
import numpy as np
import pytest

import indel_cases as D
from tiddit_amd import tiddit_indels as T


@pytest.fixture(scope="module")
def refs():
    return {c["name"]: D.reference(c) for c in D.CASES}


def test_the_stated_number_of_cases_in_seven_families():
    assert len(D.CASES) == D.N_CASES == 53 and len({c["name"] for c in D.CASES}) == 53
    assert D.FAMILIES == ["cap", "filters", "malformed", "sequence", "sets", "shape", "walk"]
    assert sorted(set(D.MUTANTS.values())) == ["cap", "filters", "sequence", "sets", "walk"] and len(D.MUTANTS) == 8
    assert T.SN == D.SN and T.SIZE == D.SIZE == 11 and T.INDEL_MAX_PER_READ == 4


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_claim_restatement_definition_and_column_form_agree(case, refs):
    claim, ref = D.expected(case), refs[case["name"]]
    assert D.same(claim, ref), case["name"]
    assert D.same(D.definition(case), ref), case["name"]
    assert D.same(D.definition(case, numpy_form=True), ref), case["name"]
    if case["reader_ok"]:                                       # (back to back, as a BAM file holds them: the same answer)
        assert D.same(D.reference(case, padding=False), ref)


def _kinds(case):
    raw = memoryview(np.ascontiguousarray(D.build(case).raw))
    b = D.build(case)
    return [T.events_of_read(int(b.flag[i]), int(b.tid[i]), int(b.pos[i]), int(b.mapq[i]), int(b.rec_off[i]), raw, case["Q"]) for i in range(len(b))]


def _case(name):
    return next(c for c in D.CASES if c["name"] == name)


def test_every_edge_is_where_its_case_says_it_is():
    kind_of = lambda k2: (k2 >> 45) & 3
    ev = _kinds(_case("sequence 1 21 and 22 bases are packed, 23 are hashed"))
    assert [(e[0], e[1][0][1] >> 63, (e[1][0][1] >> 47) & 0xffff, kind_of(e[1][0][1])) for e in ev] == [("ok", 1, n, k) for n, k in ((1, 0), (21, 0), (22, 0), (23, 1))]
    ev = _kinds(_case("sequence 65535 bases are hashed, 65536 are too long"))
    assert [(e[0], len(e[1]), e[3]) for e in ev] == [("ok", 1, 0), ("ok", 0, 1), ("ok", 1, 0), ("ok", 0, 1)]
    assert kind_of(ev[0][1][0][1]) == 1 and (ev[0][1][0][1] >> 47) & 0xffff == 65535
    ev = _kinds(_case("sequence a span that ends one base behind the sequence, and one that ends on it"))
    assert [kind_of(e[1][0][1]) for e in ev] == [2, 0]
    ev = _kinds(_case("sequence an N or = base is hashed"))
    assert [kind_of(e[1][0][1]) for e in ev] == [1, 1, 1, 0]
    ev = _kinds(_case("cap 0 1 4 and 5 keyed events; unanchored and too long ones do not count towards the cap"))
    assert [(e[0], len(e[1]), e[2], e[3]) for e in ev] == [("ok", 0, 0, 0), ("ok", 1, 0, 0), ("ok", 4, 0, 0), ("noisy", 0, 1, 0), ("ok", 4, 1, 1)]
    ev = _kinds(_case("walk 65535 operations"))
    assert [(e[0], len(e[1])) for e in ev] == [("noisy", 0), ("ok", 4)]
    ev = _kinds(_case("malformed P 0 and 1, 2^31 - 1 and 2^31 through long N operations"))
    assert [e[0] for e in ev] == ["malformed", "ok", "ok", "malformed", "malformed"]
    assert [k1 & 0xffffffff for e in ev for k1, _ in e[1]] == [1, 2 ** 31 - 1]
    ev = _kinds(_case("malformed tid 2^24 - 1 and 2^24, pos -1"))
    assert [e[0] for e in ev] == ["ok", "malformed", "malformed"]
    for name in ("the fixed fields end behind the buffer", "the fields are longer than block_size", "block_size ends behind the buffer (the last record)",
                 "a negative l_seq", "op codes 9 and 15"):
        kinds = [e[0] for e in _kinds(_case("malformed " + name))]
        assert kinds.count("malformed") == (2 if "op codes" in name else 1) and kinds.count("ok") == 2, name
    for q, want in ((0, ["ok", "ok"]), (20, ["not_eligible", "ok", "ok"]), (255, ["not_eligible", "ok"])):
        assert [e[0] for e in _kinds(_case("filters mapq round a minimum of %d" % q))] == want
    assert [e[0] for e in _kinds(_case("filters each bit of 0xF04 alone, the other bits, tid -1"))] == ["not_eligible"] * 5 + ["ok"] * 7 + ["not_eligible"]
    # the shape cases sit on the push kernel's wave, round and tile; the set cases on the run-length tile and the sort's
    sizes = sorted(len(c["reads"]) for c in D.CASES if c["name"].startswith("shape a batch of"))
    assert sizes == sorted([1, 63, 64, 65, D.INDEL_BLOCK + 1, D.INDEL_K_TILE - 1, D.INDEL_K_TILE, D.INDEL_K_TILE + 1])
    full = _case("shape every read of a workgroup gives 4 events")
    assert len(full["reads"]) == D.INDEL_K_TILE + 1 and sum(n for _, n in full["keys"]) == 4 * (D.INDEL_K_TILE + 1)
    stores = sorted(sum(n for _, n in c["keys"]) for c in D.CASES if c["name"].startswith("sets a store of"))
    for t in {D.RS_TILE, D.INDEL_TILE}:
        assert all(stores.count(v) >= 1 for v in (t - 1, t, t + 1, t + 2, 2 * t + 1))
    big = _case("sets one event over more keys than two tiles hold, through repeated pushes")
    assert sum(n for _, n in big["keys"]) == 2 * D.INDEL_TILE + 1


@pytest.mark.parametrize("mutant", sorted(D.MUTANTS))
def test_a_one_line_departure_changes_the_output_inside_its_family(mutant, refs):
    family = D.MUTANTS[mutant]
    changed = [c["name"] for c in D.CASES if c["family"] == family and len(c["reads"]) * c["repeat"] <= 200 and not D.same(D.reference(c, mutant=mutant), refs[c["name"]])]
    assert changed, mutant


def test_nothing_depends_on_the_order_of_the_reads(refs):
    case = _case("sets forward only, reverse only and mixed; supports round 1 2 and 3")
    for order in (np.arange(12)[::-1], np.random.default_rng(3).permutation(12)):
        other = dict({k: v for k, v in case.items() if not isinstance(k, tuple)}, reads=[case["reads"][k] for k in order.tolist()])
        assert D.same(D.reference(other), refs[case["name"]]) and D.same(D.definition(other), refs[case["name"]])


def test_parse_switch():
    assert T.parse_switch(None) is None and T.parse_switch("") is None
    assert T.parse_switch("1") == (2, 20) and T.parse_switch("2") == (2, 20) and T.parse_switch("3") == (3, 20)
    assert T.parse_switch("1:20") == (1, 20) and T.parse_switch("5:0") == (5, 0) and T.parse_switch("1000000:255") == (10 ** 6, 255)
    for bad in ("0", "1000001", "1:256", "x", "-1", "1:", ":5", "1:2:3", "1.5", " 1", "2:-1", "0:20", "1" * 10):
        with pytest.raises(ValueError):
            T.parse_switch(bad)


def test_write_file_gives_a_literal_text(tmp_path):
    counts = np.array([100, 90, 1, 2, 0, 3, 8, 4, 5, 6, 5], dtype=np.uint64)
    rows = (np.array([D.K1(0, 105), D.K1(0, 105), D.K1(0, 160), D.K1(1, 51), D.K1(2, 7)], dtype=np.uint64),
            np.array([D.DEL(3), D.INS("GAT"), D.INSX(7), (D.INSH("ANA") >> 1) << 1, D.DEL(65535)], dtype=np.uint64),
            np.array([4, 2, 3, 2, 9], dtype=np.uint32), np.array([1, 2, 0, 1, 9], dtype=np.uint32))
    cov = {"c0": np.array([30.0, 31.256, 12.5, 7.125]), "c1": np.array([9.0])}
    path = str(tmp_path / "x.indels.tab")
    T.write_file(path, counts, rows, ["c0", "c1", "c2"], cov, 2, 20)
    h = (D.INSH("ANA") >> 1) & (2 ** 44 - 1)
    want = ("# tiddit_amd indels v1 min_support=2 min_mapq=20\n"
            "SN\trecords\t100\nSN\teligible\t90\nSN\tmalformed\t1\nSN\tunanchored\t2\nSN\ttoo_long\t0\nSN\tnoisy_reads\t3\nSN\treads_with_events\t8\n"
            "SN\tinsertions\t4\nSN\tdeletions\t5\nSN\tdistinct_events\t6\nSN\treported_events\t5\n"
            "#CHROM\tPOS\tTYPE\tLEN\tSEQ\tSUPPORT\tFWD\tREV\tCOV\n"
            "c0\t105\tDEL\t3\t.\t4\t3\t1\t12.50\n"
            "c0\t105\tINS\t3\tGAT\t2\t0\t2\t12.50\n"
            "c0\t160\tINS\t7\t*\t3\t3\t0\t7.12\n"
            "c1\t51\tINS\t3\t#%011x\t2\t1\t1\t.\n"
            "c2\t7\tDEL\t65535\t.\t9\t0\t9\t.\n" % h)
    assert open(path).read() == want
    assert T.summary_line(counts) == "indels: 100 records, 90 eligible, 4 insertions, 5 deletions, 6 distinct events, 5 reported, noisy reads 3, malformed records 1"
