"""CPU pin of tests/ingest_cases.py: the struct-walk reference against the independent parser (oracle/signal_oracle.parse_record) and
the host decoder (bamio.BamReader -> tdt_bam_decode) on every case; every stream is valid BGZF and every aimed placement is where its
case says; every decoy is a well-formed record at its own offset; the restated finder contract gives the chases the cases state; and
every listed departure of the reference changes the expected output inside its family.  No GPU.

Cases per family: A 34, B 10, C 16, D 8, E 7, F 7, G 4, H 4, I 4 (94)."""
import struct
import zlib

import numpy as np
import pytest

import ingest_cases as ic
from oracle import signal_oracle
from tiddit_amd import bamio

SEG = ic.SEG


def test_the_case_set_is_the_one_the_files_state():
    fam = {f: len(ic.by_family(f)) for f in ic.FAMILIES}
    assert fam == {"A": 34, "B": 10, "C": 16, "D": 8, "E": 7, "F": 7, "G": 4, "H": 4, "I": 4} == ic.FAMILY_COUNTS, fam
    assert len(ic.cases()) == 94
    routes = {}
    for _, r in ic.ledger():
        routes[r] = routes.get(r, 0) + 1
    assert routes == {"wave": 90, "serial": 75, "second_binned": 8, "second_generic": 8, "ahead": 2, "sharded": 4}, routes
    for c in ic.cases():
        assert c.aim and len(c.stream) <= (400 << 10), c.name


def test_constants_are_read_from_the_source():
    assert ic.K == {"ING_SEG": 16384, "ING_EDGES": 8191, "ING_MAXREC": (16384 + 35) // 36}
    text = "#ifndef ING_SEG\n#define ING_SEG 4096\n#endif\n#define ING_EDGES 15   // runs\n#define ING_MAXREC ((ING_SEG + 35) / 36)\n"
    assert ic.parse_constants(text) == {"ING_SEG": 4096, "ING_EDGES": 15, "ING_MAXREC": 114}
    with pytest.raises(KeyError):
        ic.parse_constants(text.replace("ING_EDGES 15", "ING_EDGES sizeof(x)"))
    with pytest.raises(KeyError):
        ic.parse_constants(text.replace("#define ING_MAXREC", "#define ING_MAXRECORDS"))


def _oracle_record(c, raw, o, sq):
    """parse_record at o; where it cannot read the aux area (types it does not know, stray bytes: only in the cases that say so) the
    same record with the aux area cut off"""
    try:
        return signal_oracle.parse_record(raw, o, sq)[0], True
    except (ValueError, KeyError, struct.error, UnicodeDecodeError):
        assert c.loose_aux, c.name
    bs, l_name, n_cig, l_seq = struct.unpack_from("<I", raw, o)[0], raw[o + 12], struct.unpack_from("<H", raw, o + 16)[0], struct.unpack_from("<i", raw, o + 20)[0]
    var = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    cut = struct.pack("<I", var) + raw[o + 4:o + 4 + var]
    return signal_oracle.parse_record(cut, 0, sq)[0], False


@pytest.mark.parametrize("family", ["A", "B", "C", "D", "E", "I", "G"])
def test_reference_equals_independent_parser_and_host_decoder(family, tmp_path):
    sq = [{"SN": n, "LN": l} for n, l in ic.REFS] + [{"SN": "beyond%d" % k, "LN": 1} for k in range(8)]
    checked_sa = 0
    for c in ic.by_family(family):
        R = c.reference()
        raw = c.stream
        for i, o in enumerate(R["rec_off"].tolist()):
            r, whole = _oracle_record(c, raw, o, sq)
            got = (r.reference_id, r.reference_start, r.reference_end, r.mapq, r.flag, r.next_reference_id, r.mate_pos, r.isize, len(r.query_sequence))
            want = tuple(int(R[k][i]) for k in ("tid", "pos", "end", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "l_seq"))
            assert got == want, (c.name, i)
            cig = r.cigartuples
            assert int(R["cigar_first"][i]) == ((cig[0][1] << 4 | cig[0][0]) if cig else ic.NONE), (c.name, i)
            assert int(R["cigar_last"][i]) == ((cig[-1][1] << 4 | cig[-1][0]) if cig else ic.NONE), (c.name, i)
            if whole and c.sa_by_oracle:
                s = int(R["sa_off"][i])
                assert (s >= 0) == ("SA" in r.tags), (c.name, i)
                if s >= 0:
                    assert raw[s:raw.index(b"\x00", s)].decode() == r.tags["SA"], (c.name, i)
                    checked_sa += 1
        if not c.host:
            continue
        path = str(tmp_path / (c.name + ".bam"))
        open(path, "wb").write(c.file_bytes())
        rd = bamio.BamReader(path)
        assert rd.header_bytes == c.skip and len(rd.references) == c.n_ref
        H = {k: [] for k in ic.COLUMNS}
        for b in rd.batches():
            for k in ic.COLUMNS:
                H[k].append(getattr(b, k))
        rd.close()
        H = {k: np.concatenate(v) if v else np.zeros(0, t) for (k, t), v in zip(zip(ic.COLUMNS, ic.TYPES), H.values())}
        for k in ic.COLUMNS[:11]:
            assert np.array_equal(H[k], R[k]), (c.name, k)
        has = R["sa_off"] >= 0
        assert np.array_equal(H["sa_off"] >= 0, has), c.name
        assert np.array_equal((H["sa_off"] - H["rec_off"].astype(np.int64))[has], (R["sa_off"] - R["rec_off"].astype(np.int64))[has]), c.name
    assert checked_sa or family not in "ACDE"


def _blocks_inflate(data):
    out, o, sizes = b"", 0, []
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04" and data[o + 12:o + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        piece = zlib.decompress(data[o + 18:o + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", data, o + bsize - 8)
        assert crc == zlib.crc32(piece) & 0xffffffff and isize == len(piece) <= 0xff00
        out += piece
        sizes.append(len(piece))
        o += bsize
    assert o == len(data)
    return out, sizes


def test_every_stream_is_valid_bgzf_cut_where_the_case_says():
    for c in ic.cases():
        if c.shard:
            blocks, j, own = c.shard_blocks()
            data, sizes = _blocks_inflate(b"".join(blocks))
            assert data == c.stream and sizes == c.shard[0] and sum(sizes[:j]) == own and 0 < j < len(sizes), c.name
            continue
        o = 0
        for k, (comp, n) in enumerate(zip(c.comp_pushes(), c.pushes)):
            data, sizes = _blocks_inflate(comp)
            assert data == c.stream[o:o + n] and all(z <= c.block for z in sizes), (c.name, k)
            o += n
        assert o == len(c.stream) and c.comp_pushes()[-1].endswith(bamio._BGZF_EOF), c.name
        assert c.stream[:4] == b"BAM\x01" or c.name == "C_empty_file"


def _starts_per_segment(B):
    return np.bincount((B["rec_off"] // np.uint64(SEG)).astype(np.int64), minlength=1) if B["n"] else np.zeros(1, np.int64)


def test_every_aimed_placement_is_where_the_case_says():
    kinds = set()
    for c in ic.cases():
        if c.shard:
            continue
        Bs, R = c.batches(model=False), c.reference()
        assert sum(B["n"] for B in Bs) == len(R["tid"]) and Bs[-1]["carry"] == 0, c.name
        for a in c.aims:
            kinds.add(a["kind"])
            B = Bs[a["batch"]] if "batch" in a else None
            if a["kind"] == "start":
                assert int(R["rec_off"][a["rec"]]) - B["base"] == a["at"] and B["lo"] <= a["rec"] < B["hi"], (c.name, a)
            elif a["kind"] == "end":
                assert int(R["rec_end"][a["rec"]]) - B["base"] == a["at"] and B["lo"] <= a["rec"] < B["hi"], (c.name, a)
            elif a["kind"] == "size":
                assert int(R["rec_end"][a["rec"]] - R["rec_off"][a["rec"]]) == a["size"], (c.name, a)
            elif a["kind"] == "covers":
                lo, hi = int(R["rec_off"][a["rec"]]) - B["base"], int(R["rec_end"][a["rec"]]) - B["base"]
                per = _starts_per_segment(B)
                for g in a["segments"]:
                    assert lo <= g * SEG and (g + 1) * SEG <= hi and per[g] == 0, (c.name, a)
            elif a["kind"] == "per_segment":
                assert _starts_per_segment(B)[a["segment"]] == a["starts"], (c.name, a, _starts_per_segment(B))
            elif a["kind"] == "tail":
                assert B["carry"] == a["left"], (c.name, a, B["carry"])
                nxt = B["hi"]
                if a["left"]:
                    assert len(B["raw"]) - a["left"] == int(R["rec_off"][nxt]) - B["base"], (c.name, a)
            elif a["kind"] == "zero":
                assert B["n"] == 0, (c.name, a)
            elif a["kind"] == "count":
                assert B["n"] == a["n"], (c.name, a)
            elif a["kind"] == "first_behind":
                g = a["segment"]
                off = B["rec_off"].astype(np.int64)
                assert int(off[off >= g * SEG][0]) == int(R["rec_off"][a["rec"]]) - B["base"] and off[a["rec"] - B["lo"] - 1] < g * SEG, (c.name, a)
            elif a["kind"] == "runs":
                assert (B["edges"] is None) if a["n"] is None else (len(B["edges"]) == a["n"] == len(B["edge_tids"])), (c.name, a)
            elif a["kind"] == "edges":
                assert B["edges"].tolist() == a["edges"] and a["edges"][-1] == B["n"] - 1, (c.name, a)
            else:
                raise AssertionError(a)
    assert kinds == {"start", "end", "size", "covers", "per_segment", "tail", "zero", "count", "first_behind", "runs", "edges"}
    # the aimed values themselves
    names = {c.name for c in ic.cases()}
    for d in ic.START_D:
        for pre in ("A_start_", "A2_start_"):
            c = ic.get(pre + (("m%d" % -d) if d < 0 else "p%d" % d))
            assert [a["at"] for a in c.aims if a["kind"] == "start"] == [SEG + d]
    for d in ic.END_D:
        for pre in ("A_end_", "A2_end_"):
            c = ic.get(pre + (("m%d" % -d) if d < 0 else "p%d" % d))
            assert [a["at"] for a in c.aims if a["kind"] == "end"] == [SEG + d]
    for n in (63, 64, 65, 128, 129):
        assert {a["starts"] for a in ic.get("B_%d" % n).aims} == {n}
    assert ic.get("B_min38").aims[0]["starts"] == -(-SEG // 38) == ic.get("B2_min38").aims[0]["starts"] > 6 * 64
    assert -(-SEG // 38) <= ic.MAXREC
    for t in ic.TAILS:
        assert ic.get("C_tail_%d" % t).aims[0]["left"] == t
    assert {"C_tail_name", "C_first_incomplete", "C_remainder_only", "C_inside_record", "C_empty_file", "C_header_only"} <= names
    # every record of the dense cases differs from its neighbours in its fields
    for c in ic.by_family("B"):
        R = c.reference()
        for k in ("pos", "mapq", "mate_pos", "tlen", "flag"):
            assert np.all(R[k][1:] != R[k][:-1]), (c.name, k)


def test_every_decoy_is_a_well_formed_record_in_front_of_the_entry_point():
    sq = [{"SN": n, "LN": l} for n, l in ic.REFS]
    n = 0
    for c in ic.cases():
        R = c.reference()
        true_starts = set(R["rec_off"].tolist())
        for d in c.decoys:
            n += 1
            o = d["off"]
            assert o not in true_starts
            host = int(np.searchsorted(R["rec_off"], o, side="right")) - 1               # the true record the decoy lies in
            assert int(R["rec_off"][host]) < o < int(R["rec_end"][host])
            if not c.shard:                                          # (on the grid of the batch that decodes the straddling record)
                base = next(B["base"] for B in c.batches(model=False) if B["lo"] <= host < B["hi"])
                assert (int(R["rec_off"][host]) - base) // SEG < (o - base) // SEG, "the straddling record starts in the segment before the decoy's"
            if d["kind"] == "weak":
                assert struct.unpack_from("<I", c.stream, o)[0] + o + 4 > len(c.stream)
                body = c.stream[o + 4:o + d["len"]]
                r, end = signal_oracle.parse_record(struct.pack("<I", len(body)) + body, 0, sq)
            else:
                r, end = signal_oracle.parse_record(c.stream, o, sq)
                if d["kind"] == "complete":
                    assert end == int(R["rec_end"][host]) and end in true_starts, (c.name, d)           # ... ends on the next true record start
                else:
                    assert end < int(R["rec_end"][host]) and c.stream[end:end + 4] == bytes(4), (c.name, d)
            assert r.query_name == "dcy" and 0 <= r.reference_id < c.n_ref and 0 <= r.next_reference_id < c.n_ref and not r.cigartuples
            assert r.query_sequence == "" and ic.plausible(c.stream, o, len(c.stream), c.n_ref, True)[0] in (0, 1)
    assert n == 9


def test_the_finder_contract_gives_the_chases_the_cases_state():
    for c in ic.cases():
        if c.shard:
            continue
        Bs = c.batches()
        assert [b for b, B in enumerate(Bs) if B["chased"]] == c.chased, c.name
        if c.family not in "FG":
            assert c.chased == [], c.name
        for B in Bs:
            if B["searched"] and not B["chased"]:                   # a confirmed chain is the sequential decode
                m = ic.guess_and_confirm(B["raw"], B["s0"], c.n_ref)
                assert m["n"] == B["n"] and len(B["raw"]) - m["cur"] == B["carry"], c.name
    assert sum(len(c.chased) for c in ic.by_family("F")) == 5 and sum(len(c.chased) for c in ic.by_family("G")) == 4
    # what the host decoder accepts, the device check refuses: each G case has exactly one record that fails the deep check
    for c in ic.by_family("G"):
        R = c.reference()
        bad = [i for i, o in enumerate(R["rec_off"].tolist()) if ic.plausible(c.stream, o, len(c.stream), c.n_ref, True)[0] == 2]
        assert len(bad) == 1, c.name
        shallow = ic.plausible(c.stream, int(R["rec_off"][bad[0]]), len(c.stream), c.n_ref, False)[0]
        assert shallow == (2 if c.name.startswith("G_tid_beyond") else 0), c.name


def test_sharded_seams():
    for c in ic.by_family("H"):
        e = ic.shard_expectation(c)
        R = c.reference()
        assert e["model0"]["confirmed"] and e["model0"]["n"] == e["n0"] and e["model0"]["cur"] - e["own"] == e["next_off"], c.name
        assert e["model1"]["confirmed"], c.name
        if c.decoys:
            assert e["model1"]["start"] == c.decoys[0]["off"] - e["own"] != e["next_off"]
            assert e["model1"]["n"] == len(R["tid"]) - e["n0"] + 1
        else:
            assert e["model1"]["start"] == e["next_off"] and e["model1"]["n"] == len(R["tid"]) - e["n0"], c.name
    starts = ic.get("H_on_record_start").reference()["rec_off"].tolist()
    assert ic.shard_expectation(ic.get("H_on_record_start"))["own"] in starts and ic.shard_expectation(ic.get("H_on_record_start"))["next_off"] == 0
    assert ic.shard_expectation(ic.get("H_one_behind_start"))["own"] - 1 in ic.get("H_one_behind_start").reference()["rec_off"].tolist()


def _expected(c, mutant):
    if c.shard:
        e = ic.shard_expectation(c, mutant)
        return [e["model0"], e["model1"]]
    out = []
    for B in c.batches(mutant):
        out.append((B["n"], B["chased"], B["packed"].tobytes()) + tuple(B[k].tobytes() for k in ic.COLUMNS))
    return out


@pytest.mark.parametrize("mutant", sorted(ic.MUTANTS))
def test_every_departure_of_the_reference_is_noticed_in_its_family(mutant):
    family = ic.MUTANTS[mutant]
    changed = [c.name for c in ic.by_family(family) if _expected(c, mutant) != _expected(c, None)]
    assert changed, mutant
    want = {"end_ignores_N": "D_cigar_ops", "end_no_fallback": "D_reference_length_0", "unmapped_keeps_span": "D_unmapped_with_cigar",
            "span_saturates_early": "D_spans", "sa_byte_scan": "E_lookalikes", "sa_any_type": "E_sa_not_Z", "first_plausible_offset": "F_broken_chain"}
    assert want[mutant] in changed, (mutant, changed)


def test_packed_record_restates_the_layout():
    assert ic.pack_record(5, 5 + 0xfffffe, 70, 0x404) == ((0xfffffe | 63 << 24 | 1 << 30 | 1 << 31) << 32) | 5
    assert ic.pack_record(5, 5 + 0xffffff, 0, 0) >> 32 == 0xffffff == ic.pack_record(5, 5 + 0x1000000, 0, 0) >> 32
    assert ic.pack_record(-1, 0, 1, 0) == ((1 | 1 << 24) << 32) | 0xffffffff
