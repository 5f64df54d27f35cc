"""The definition of the exact per-base depth (tiddit_amd/tiddit_pileup.py) on the CPU: it equals every literal claim of
tests/pileup_cases.py; an independent numpy restatement (the CIGAR as arrays, the spans by a cumulative sum, ``np.add.at`` on a
difference array with a guard slot per contig, ``cumsum``) equals it on the cases and on 500 random legal records drawn by the generator
of tests/scan_random_cases.py; eight departures from the definition are each noticed by a named family of cases; and, as an outside
anchor, every depth equals ``A + C + G + T + N + LOWBQ`` of ``tiddit_alleles.count_batch`` with a site at every base.

Every test of this file fails on the parent commit: the module does not exist there."""
import struct

import numpy as np
import pytest

import pileup_cases as D

CLAIMS = {}


def _claim(c):
    if c["name"] not in CLAIMS:
        CLAIMS[c["name"]] = D.expected(c)
    return CLAIMS[c["name"]]


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_the_definition_equals_the_claim(case):
    want, got = _claim(case), D.definition(case)
    assert np.array_equal(got[1], want[1]), (got[1].tolist(), want[1].tolist())
    assert D.same(got, want)


def test_the_families_and_the_counts_are_what_the_module_states():
    from tiddit_amd import tiddit_pileup
    assert D.N_CASES == 18 and tiddit_pileup.SN == D.SN and tiddit_pileup.SIZE == D.SIZE == 7
    total = sum(_claim(c)[1] for c in D.CASES)
    assert all(total[i] > 0 for i in range(D.SIZE)), total.tolist()               # every counter is moved by some case
    assert max(int(d.max()) for c in D.CASES for d in _claim(c)[0]) == 3007


def test_spans_of_read_gives_the_kind_and_the_stated_spans_of_every_read():
    from tiddit_amd import tiddit_pileup
    from tiddit_amd.bamio import _raw_of
    n = 0
    for c in D.CASES:
        for (reads, _), b in zip(c["batches"], D.batches(c)):
            raw = _raw_of(b)
            for i, r in enumerate(reads):
                kind, spans = tiddit_pileup.spans_of_read(int(b.flag[i]), int(b.tid[i]), int(b.pos[i]), int(b.mapq[i]), int(b.rec_off[i]), raw, c["lengths"], c["Q"])
                assert (kind, spans) == (r["kind"], r["spans"]), (c["name"], i, kind, spans, r["kind"], r["spans"])
                n += 1
    assert n > 5000


# ---- the restatement ------------------------------------------------------------------------------------------------------------
DEPARTURES = ("D counted", "I splits a span", "no clamp", "the -1 one slot early", "no guard slot", "MAPQ > for >=")


def restated(batches, lengths, Q, departure=None):
    """spans -> np.add.at on a difference array -> cumsum, written independently of the definition (arrays, not a walk with a list);
    ``departure``: one of DEPARTURES, built in on purpose"""
    guard = 0 if departure == "no guard slot" else 1
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64) + guard)])
    # (room behind the end for the departure that runs over it; WITHOUT guard slots a global sum still comes out right wherever another
    #  contig follows — the -1 lands on its first slot — and what is lost is the slot of the LAST contig's -1: no room, an IndexError)
    diff = np.zeros(int(off[-1]) + (2 ** 16 if departure == "no clamp" else 0), dtype=np.int64)
    c = np.zeros(D.SIZE, dtype=np.int64)
    for b in batches:
        raw = np.ascontiguousarray(b.raw, dtype=np.uint8)
        n = len(raw)
        for flag, tid, pos, mapq, ro in zip(b.flag.tolist(), b.tid.tolist(), b.pos.tolist(), b.mapq.tolist(), b.rec_off.tolist()):
            c[0] += 1
            if flag & 0xF04 or tid < 0 or (mapq <= Q if departure == "MAPQ > for >=" else mapq < Q):
                continue
            c[1] += 1
            fields = None
            if ro + 36 <= n:
                block_size, _, _, l_name, _, _, n_cig, _, l_seq = struct.unpack_from("<IiiBBHHHi", raw, ro)
                if l_seq >= 0 and 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq <= block_size and ro + 4 + block_size <= n:
                    fields = np.frombuffer(raw[ro + 36 + l_name:ro + 36 + l_name + 4 * n_cig].tobytes(), dtype="<u4").astype(np.int64)
            if fields is None or tid >= len(lengths) or tid >= 1 << 24 or pos < 0:
                c[2] += 1
                continue
            op, ln = fields & 15, fields >> 4
            on_ref, on_query, covers = np.isin(op, (0, 2, 3, 7, 8)), np.isin(op, (0, 1, 4, 7, 8)), np.isin(op, (0, 7, 8))
            if departure == "D counted":
                covers = covers | (op == 2)
            if (op > 8).any() or pos + int(ln[on_ref].sum()) > 2 ** 31 - 1 or (l_seq >= 1 and n_cig >= 1 and int(ln[on_query].sum()) != l_seq):
                c[2] += 1
                continue
            if n_cig == 0:
                c[3] += 1
                continue
            start = pos + np.cumsum(ln * on_ref) - ln * on_ref
            keep = covers & (ln > 0)
            s, e = start[keep], (start + ln)[keep]
            if departure == "I splits a span":
                group = np.cumsum(np.concatenate([[0], np.diff(np.flatnonzero(keep)) > 1])) if len(s) else np.zeros(0, dtype=np.int64)
                fresh = np.concatenate([[True], (s[1:] != e[:-1]) | (group[1:] != group[:-1])]) if len(s) else np.zeros(0, dtype=bool)
            else:
                fresh = np.concatenate([[True], s[1:] != e[:-1]]) if len(s) else np.zeros(0, dtype=bool)
            first, last = np.flatnonzero(fresh), np.flatnonzero(np.concatenate([fresh[1:], [True]])) if len(s) else np.zeros(0, dtype=np.int64)
            s, e = s[first], e[last]
            L = lengths[tid]
            if departure != "no clamp":
                cs, ce = np.minimum(s, L), np.minimum(e, L)
                c[6] += int(((cs != s) | (ce != e)).sum())
                s, e = cs[cs < ce], ce[cs < ce]
            c[4] += len(s)
            c[5] += int((e - s).sum())
            np.add.at(diff, off[tid] + s, 1)
            np.add.at(diff, off[tid] + e - (1 if departure == "the -1 one slot early" else 0), -1)
    depth = np.cumsum(diff)
    return [depth[int(off[t]):int(off[t]) + int(lengths[t])].astype(np.uint32) for t in range(len(lengths))], c.astype(np.uint64)


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_the_restatement_equals_the_definition_on_the_cases(case):
    got, want = restated(D.batches(case), case["lengths"], case["Q"]), D.definition(case)
    assert np.array_equal(got[1], want[1]), (got[1].tolist(), want[1].tolist())
    assert D.same(got, want)


class _Batch:
    def __len__(self):
        return len(self.tid)


def random_batch(seed, records=500):
    """``records`` random legal records of scan_random_cases' generator (its background reads: CIGARs of 1 ... 12 operations over all nine
    codes, reads from base 0, over a contig's end and on the small contigs, every flag bit and MAPQ), as one batch in the order drawn"""
    import scan_all_cases as C
    import scan_random_cases as R
    table = C.contigs()
    seqs, sites = R._reference()
    G = R._Gen(table, seqs, sites, seed)
    G.background(records)
    recs = [r[2] for r in G.recs[:records]]
    b = _Batch()
    b.raw = np.frombuffer(b"".join(recs), dtype=np.uint8)
    b.rec_off = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint64)
    f = lambda fmt, at, dt: np.array([struct.unpack_from(fmt, r, at)[0] for r in recs], dtype=dt)
    b.tid, b.pos, b.mapq, b.flag = f("<i", 4, np.int32), f("<i", 8, np.int32), f("<B", 13, np.uint8), f("<H", 18, np.uint16)
    return b, [l for _, l in table]


def test_the_restatement_equals_the_definition_on_500_random_legal_records():
    from tiddit_amd import tiddit_pileup
    b, lengths = random_batch(11)
    assert len(b) == 500
    for Q in (0, 20):
        spans, sn = [], {}
        tiddit_pileup.spans_of_batch(b, spans, sn, lengths, Q)
        want = (tiddit_pileup.depth_of(spans, lengths), tiddit_pileup.counters_of(sn))
        got = restated([b], lengths, Q)
        assert np.array_equal(got[1], want[1]), (Q, got[1].tolist(), want[1].tolist())
        assert D.same(got, want), Q
        c = dict(zip(D.SN, want[1].tolist()))
        assert c["records"] == 500 and c["eligible"] > 100 and c["spans"] > 100 and c["malformed"] == 0 and c["clamped_spans"] >= 1, c


# ---- the departures -------------------------------------------------------------------------------------------------------------
NOTICED_BY = {"D counted": "cigar", "I splits a span": "cigar", "no clamp": "edges", "the -1 one slot early": "merge", "no guard slot": "edges",
              "MAPQ > for >=": "gate"}


@pytest.mark.parametrize("departure", DEPARTURES)
def test_a_departure_is_noticed_by_its_family(departure):
    """(the two departures of the genotype rule — ties to the larger index, GQ uncapped — are in tests/test_small_vcf_refs_cpu.py)"""
    family = [c for c in D.CASES if c["family"] == NOTICED_BY[departure]]
    assert family
    def differs_on(c):
        try:
            return not D.same(restated(D.batches(c), c["lengths"], c["Q"], departure), _claim(c))
        except IndexError:                                                      # (a -1 with no slot to go to)
            return True
    differs = [c["name"] for c in family if differs_on(c)]
    assert differs, departure


# ---- the outside anchor ---------------------------------------------------------------------------------------------------------
def test_every_depth_equals_the_allele_counters_bases_with_a_site_at_every_base():
    """tiddit_alleles.count_batch is another walk of the same records, written for another purpose: with a site at every base of every
    contig, ``A + C + G + T + N + LOWBQ`` of a site is the number of reads with an aligned base there.  Restricted to reads eligible
    under BOTH gates — the allele counter leaves out records without a sequence (``l_seq < 1``; the depth counts one with a CIGAR) and
    calls a read whose CIGAR asks for more query bases than ``l_seq`` malformed only where a site lies there.  The designed case holds no
    such record: nothing is left out, which the test asserts."""
    from tiddit_amd import tiddit_alleles, tiddit_pileup
    lengths = (300, 64)
    rd = D.rd
    reads = [rd(tid=0, pos=0, cigar="50M"), rd(tid=0, pos=10, cigar="20M5D20M"), rd(tid=0, pos=30, cigar="10M40N10M2I10M"),
             rd(tid=0, pos=100, cigar="5S20M5S"), rd(tid=0, pos=100, cigar="3H20=5X"), rd(tid=0, pos=250, cigar="50M"), rd(tid=0, pos=299, cigar="1M"),
             rd(tid=0, pos=120, cigar="10M0D10M1P5M", flag=0x10), rd(tid=0, pos=130, cigar="30M", mapq=19), rd(tid=0, pos=130, cigar="30M", mapq=20),
             rd(tid=0, pos=130, cigar="30M", flag=0x400), rd(tid=1, pos=0, cigar="64M"), rd(tid=1, pos=60, cigar="4M"), rd(tid=1, pos=5, cigar="10M3D10M3N10M")]
    reads += [rd(tid=0, pos=200 + k % 3, cigar="25M") for k in range(70)]
    b = D.build_batch(reads)
    assert all(len(r["seq"]) >= 1 and r["cigar"] and r["pos"] + sum(n for op, n in r["cigar"] if op in (0, 2, 3, 7, 8)) <= lengths[r["tid"]] for r in reads)
    spans, sn = [], {}
    tiddit_pileup.spans_of_batch(b, spans, sn, lengths, 20)
    depth = tiddit_pileup.depth_of(spans, lengths)
    site_pos = np.concatenate([np.arange(n) for n in lengths])
    site_off = [0, lengths[0], lengths[0] + lengths[1]]
    table, stats = np.zeros((len(site_pos), 8), dtype=np.int64), [0, 0]
    tiddit_alleles.count_batch(table, stats, site_pos, site_off, b, 20, 13)
    assert stats == [sn["eligible"], 0] and sn["eligible"] == len(reads) - 2 and sn.get("malformed", 0) == 0        # no record is left out by either side
    bases = table[:, [tiddit_alleles.A, tiddit_alleles.C, tiddit_alleles.G, tiddit_alleles.T, tiddit_alleles.N, tiddit_alleles.LOWBQ]].sum(axis=1)
    assert np.array_equal(bases[:300], depth[0]) and np.array_equal(bases[300:], depth[1])
    assert int(depth[0].max()) >= 70 and table[:, tiddit_alleles.DEL].sum() == 8 and table[:, tiddit_alleles.SKIP].sum() == 43
