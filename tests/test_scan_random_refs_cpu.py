"""The files of tests/scan_random_cases.py — random legal records for every consumer of the ``--sv`` scan — without a GPU: each seed's file is
the same bytes when made twice and is read back whole by the host reader; every consumer's definition over it is independent of where
the host batches are cut and changed by one batch left out or fed twice; the product definitions equal the independent restatements of
the case modules (``reference_batch`` of qc_cases, dup_cases, indel_cases, alleles_cases and str_cases) on every seed; every file holds
enough for every consumer (``scan_random_cases.FLOORS``: half of the smallest value the definitions give over the six seeds, so that
tests/test_gpu_scan_random.py never passes on an empty table); and over the seeds together every ``SN`` counter of every consumer is
raised, but for ``malformed``, which no legal record can raise."""
import collections
import os
import struct

import numpy as np
import pytest

import scan_all_cases as C
import scan_random_cases as RC

FLOORS, SPANS = RC.FLOORS, RC.SPANS
# the counters no legal record can raise: a malformed record is not a legal one
NEVER = {"indels": ("malformed",), "indels_norm": ("malformed",), "snvs": ("malformed",), "clips": ("malformed",), "dups": ("malformed",),
         "str": ("malformed",), "qc": ("malformed",), "alleles": ("malformed",), "clip_ext": ()}


class Seed:
    pass


@pytest.fixture(scope="module")
def seeds(tmp_path_factory):
    out = {}
    for seed in RC.SEEDS:
        s = Seed()
        s.dir = str(tmp_path_factory.mktemp("scan_random_%d" % seed))
        s.info = RC.generate(s.dir, seed)
        s.batches = C.host_batches(C.paths(s.dir)[0])
        s.sites, s.ref = C.sites_table(s.dir), C.host_reference()
        s.parts = [C.partial(b, s.sites, s.ref) for b in s.batches]
        s.E = C.combine(s.parts)
        out[seed] = s
    return out


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_the_file_is_the_same_bytes_when_made_twice_and_is_read_back_whole(seeds, tmp_path, seed):
    s = seeds[seed]
    info = RC.generate(str(tmp_path), seed)
    for a, b in zip(C.paths(s.dir) + (C.library_path(s.dir), C.str_path(s.dir)), C.paths(str(tmp_path)) + (C.library_path(str(tmp_path)), C.str_path(str(tmp_path)))):
        assert open(a, "rb").read() == open(b, "rb").read(), a
    assert info["n_records"] == s.info["n_records"] == sum(len(b) for b in s.batches) == s.E["records"] == RC.RECORDS
    assert info["hot"] >= 0.55 * RC.RECORDS and info["background"] >= 0.3 * RC.RECORDS and info["tail"] >= 10
    assert os.path.getsize(C.paths(s.dir)[0]) >= (1 << 20) + SPANS * 65536
    other = RC.generate(str(tmp_path), seed + 100)
    assert open(C.paths(s.dir)[0], "rb").read() != open(C.paths(str(tmp_path))[0], "rb").read() and other["n_records"] == RC.RECORDS


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_the_records_are_legal_sorted_and_of_every_shape(seeds, seed):
    s = seeds[seed]
    m = C.merged_batch(s.batches)
    table = C.contigs()
    n = len(m)
    tid, pos, flag, mapq = m.tid.astype(np.int64), m.pos.astype(np.int64), m.flag.astype(np.int64), m.mapq.astype(np.int64)
    placed = np.flatnonzero(tid >= 0)
    assert 0 < len(placed) < n and placed[-1] == len(placed) - 1                # a tail of unplaced reads, behind every placed one
    key = tid[placed] * (1 << 32) + pos[placed]
    assert np.all(np.diff(key) >= 0)                                           # coordinate-sorted
    raw = m.raw.tobytes()
    ops, names, lseq0, no_ref, one_m, noqual, longest_n = collections.Counter(), [], 0, 0, 0, 0, 0
    for i in range(n):
        o = int(m.rec_off[i])
        bs, t, p, l_name, mq, _, n_cig, fl, l_seq, mt, mp, tl = struct.unpack_from("<IiiBBHHHiiii", raw, o)
        assert -1 <= t < len(table) and -1 <= mt < len(table) and p >= -1 and mp >= -1 and 2 <= l_name <= 251
        name = raw[o + 36:o + 36 + l_name]
        assert name[-1] == 0 and all(33 <= c <= 126 for c in name[:-1])
        names.append(name)
        words = struct.unpack_from("<%dI" % n_cig, raw, o + 36 + l_name)
        assert n_cig <= 12 and all(w & 0xf <= 8 and w >> 4 >= 1 for w in words)
        codes = [w & 0xf for w in words]
        inner = [c for c in codes if c != 5]
        assert 5 not in codes[1:-1] and 4 not in inner[1:-1]                    # H outermost, S inside it
        q = sum(w >> 4 for w in words if w & 0xf in (0, 1, 4, 7, 8))
        assert l_seq in (0, q) or n_cig == 0                                    # the CIGAR's query length is l_seq wherever l_seq is not 0
        assert 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq <= bs
        ops.update(codes)
        longest_n = max([longest_n] + [w >> 4 for w in words if w & 0xf == 3])
        if n_cig:
            lseq0 += l_seq == 0
            no_ref += not any(c in (0, 2, 3, 7, 8) for c in codes)
            one_m += codes == [0]
        qual = raw[o + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2:][:l_seq]
        noqual += l_seq > 0 and qual == b"\xff" * l_seq
    assert set(ops) == set(range(9)) and 300 < longest_n <= C.FAR_SKIP + 10          # (the far member of a duplicate set skips 50 010)
    # the shares that are drawn per read — SA:Z on 10 %, an empty sequence on 5 % — are drawn for the ``drawn`` reads of the file (about
    # 2 950 of 4 000: the background and the hot-spot reads made here; the planter's duplicate sets, repeat-unit and clip-site reads, about
    # a quarter of the file, carry neither).  Binomial over 2 900 reads: 290 +- 16 and 145 +- 12; the bounds lie five deviations below
    drawn = s.info["drawn"]
    assert 0.7 * n <= drawn <= n and lseq0 >= 0.03 * drawn and int((m.sa_off >= 0).sum()) >= 0.07 * drawn
    assert no_ref >= 20 and one_m >= 100 and noqual >= 50
    assert all(int(((flag >> b) & 1).sum()) >= 10 for b in range(12))          # every one of the twelve flag bits
    assert int(((flag & 0xF04) == 0).sum()) >= 0.4 * n
    # MAPQ: uniform over MAPQS on the background, uniform over its values from 20 up on the hot-spot reads made here, 60 on the planter's
    assert set(np.unique(mapq).tolist()) == set(RC.MAPQS) and min(collections.Counter(mapq.tolist()).values()) >= 60       # (1 500 / 13 = 115 +- 10 each)
    shared = collections.Counter(names)
    assert sum(c for c in shared.values() if c in (2, 3)) >= 0.1 * n and len({len(x) - 1 for x in names}) >= 8 and max(len(x) for x in names) == 251
    assert int(((flag & 0x4) != 0)[placed].sum()) >= 10                         # unmapped reads with a placement, and without one (the tail)
    ln = np.array([l for _, l in table])
    end = m.end.astype(np.int64)
    assert int((pos[placed] == 0).sum()) >= 2 and int((end[placed] == ln[tid[placed]]).sum()) >= 2 and int((end[placed] > ln[tid[placed]]).sum()) >= 1
    assert int((ln[tid[placed]] < C.MIN_CONTIG).sum()) >= 3
    mt, tl = m.mate_tid.astype(np.int64), np.abs(m.tlen.astype(np.int64))
    assert int((mt[placed] == tid[placed]).sum()) >= 100 and int(((mt[placed] >= 0) & (mt[placed] != tid[placed])).sum()) >= 100 and int((mt[placed] < 0).sum()) >= 100
    assert int(((tl > 0) & (tl < C.MAX_INS)).sum()) >= 100 and int((tl > C.MAX_INS).sum()) >= 100 and int((tl == C.MAX_INS).sum()) >= 1
    assert raw.count(b"MCZ") >= 200


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_every_file_holds_enough_for_every_consumer(seeds, seed):
    s = seeds[seed]
    found = RC.measure(s.batches, s.E)
    assert set(found) == set(FLOORS)
    assert all(found[k] >= v >= 1 for k, v in FLOORS.items()), {k: (found[k], v) for k, v in FLOORS.items() if found[k] < v}
    assert found["allele_sites"] >= 100
    # key sets of support 2, 3 and 4 and more for every keyed consumer
    for name, sup in (("indels", s.E["indels"][1][1][1][2]), ("indels_norm", s.E["indels_norm"][1][1][1][2]), ("snvs", s.E["snvs"][1][C.SNV_SUPPORTS[0]][1][2]),
                      ("clips", s.E["clips"][1][C.CLIP_SUPPORTS[0]][1][2]), ("str", s.E["str"][2][2])):
        assert all(int((sup == k).sum()) >= 3 for k in (2, 3)) and int((sup >= 4).sum()) >= 3, name


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_every_definition_is_invariant_to_where_the_batches_are_cut_and_changed_by_a_batch_left_out_or_fed_twice(seeds, seed):
    s = seeds[seed]
    small = C.host_batches(C.paths(s.dir)[0], 1 << 16)
    assert len(small) > len(s.batches) >= 4
    assert C.differing(C.combine([C.partial(b, s.sites, s.ref) for b in small]), s.E) == []
    assert C.differing(C.combine([C.partial(C.merged_batch(s.batches), s.sites, s.ref)]), s.E) == []
    i = len(s.parts) // 2
    assert C.differing(C.combine(s.parts[:i] + s.parts[i + 1:]), s.E) == list(C.CONSUMERS)
    assert C.differing(C.combine(s.parts[:i + 1] + s.parts[i:]), s.E) == list(C.CONSUMERS)


def _nonzero(sn):
    return {k: v for k, v in sn.items() if v}


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_the_definitions_equal_the_restatements_of_the_case_modules(seeds, seed):
    """each ``reference_batch`` takes the host reader's batch as it is: the columns it reads are the batch's own"""
    import alleles_cases
    import dup_cases
    import indel_cases
    import qc_cases
    import str_cases
    s = seeds[seed]
    qc = np.zeros(len(s.E["qc"]), dtype=np.int64)
    indel_keys, indel_sn, dup_keys, dup_sn, str_keys, str_sn = [], collections.Counter(), [], collections.Counter(), [], collections.Counter()
    alleles, stats = np.zeros((len(s.sites), 8), dtype=np.int64), [0, 0]
    loci = [r[:4] for r in C.str_loci().rows]
    names, str_cases.NAMES = str_cases.NAMES, tuple(n for n, _ in C.contigs())
    try:
        for b in s.batches:
            qc_cases.reference_batch(qc, b)
            indel_cases.reference_batch(b, indel_keys, indel_sn, C.INDEL_Q)
            dup_cases.reference_batch(b, dup_keys, dup_sn)
            alleles_cases.reference_batch(alleles, stats, s.sites.site_pos, s.sites.site_off, b, C.MIN_Q, C.MIN_BQ)
            str_cases.reference_batch(b, loci, str_keys, str_sn, C.STR_F, C.STR_Q)
    finally:
        str_cases.NAMES = names
    assert np.array_equal(qc.astype(np.uint64), s.E["qc"]), "qc"
    assert np.array_equal(C.key_rows(indel_keys), s.E["indels"][0]) and len(indel_keys) >= 100, "indels: the keys"
    assert _nonzero(indel_sn) == _nonzero(C._sum_sn(s.parts, "indel_sn")), "indels: the counters"
    assert np.array_equal(C.key_rows(dup_keys), s.E["dups"][0]) and len(dup_keys) >= 100, "dups: the keys"
    assert _nonzero(dup_sn) == _nonzero(C._sum_sn(s.parts, "dup_sn")), "dups: the counters"
    assert np.array_equal(alleles.astype(np.uint32), s.E["alleles"][0]) and tuple(stats) == s.E["alleles"][1:], "alleles"
    assert C._eq(C.str_result(str_keys, _nonzero(str_sn)), s.E["str"]) and len(str_keys) >= 100, "str"


def test_over_the_seeds_every_counter_of_every_consumer_is_raised(seeds):
    from tiddit_amd import tiddit_clip_ins, tiddit_clips, tiddit_dup, tiddit_indels, tiddit_qc, tiddit_snvs, tiddit_str
    total = collections.Counter()
    for s in seeds.values():
        E = s.E
        v = {"indels": dict(zip(tiddit_indels.SN, E["indels"][1][1][0].tolist())),
             "indels_norm": dict(zip(tiddit_indels.SN + tiddit_indels.NORM_SN, E["indels_norm"][1][1][0].tolist() + list(E["indels_norm"][2]))),
             "snvs": dict(zip(tiddit_snvs.SN, E["snvs"][1][C.SNV_SUPPORTS[0]][0].tolist())),
             "clips": dict(zip(tiddit_clips.SN, E["clips"][1][C.CLIP_SUPPORTS[0]][0].tolist())),
             "dups": dict(zip(tiddit_dup.SN, E["dups"][1][:len(tiddit_dup.SN)].tolist())),
             "str": dict(zip(tiddit_str.SN, E["str"][1].tolist())),
             "qc": dict(zip(tiddit_qc.SN, E["qc"][tiddit_qc.LAYOUT["SN"][0]:][:len(tiddit_qc.SN)].tolist())),
             "alleles": {"reads_used": E["alleles"][1], "malformed": E["alleles"][2]},
             "clip_ext": dict(zip(tiddit_clip_ins.SN, E["clip_chain"]["ins"][0].tolist() if hasattr(E["clip_chain"]["ins"][0], "tolist") else E["clip_chain"]["ins"][0]))}
        for name, d in v.items():
            for k, n in d.items():
                total[(name, k)] += int(n)
    assert set(NEVER) == {name for name, _ in total}
    zero = sorted(k for k, n in total.items() if n == 0)
    assert zero == sorted((name, k) for name, ks in NEVER.items() for k in ks), zero
    # the list holds nothing but the counters of records that are not legal
    assert {k for ks in NEVER.values() for k in ks} == {"malformed"}
    assert total[("indels_norm", "shift_capped")] == len(seeds)                 # (the planted tandem duplication of 1 100 bases, once per file)
