"""The insertion candidates from facing clip sites without a GPU: the definition (tiddit_amd/tiddit_clip_ins.py), an independent numpy
restatement that works the extended consensus out from the SORTED keys of the two stores chunk by chunk (as the device does) and the
pairs and closures from arrays, and the claims of tests/clip_ins_cases.py agree on every case; one-line departures of the restatement
are each noticed by a claim of the family listed for them; the first 28 columns are ``tiddit_clips``' own; every insertion length from
O to 268 closes at its own length; the generated job's reads meet the generator's condition and give the planted rows; and the switch,
the file and the summary line.

Every test of this file fails on the parent commit: the module does not exist there."""
import collections

import numpy as np
import pytest

import clip_cases as D
import clip_ins_cases as X
from tiddit_amd import tiddit_clip_ins as I, tiddit_clips

REF_CONSUMING, QUERY_CONSUMING = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)
CODE = np.full(16, -1, dtype=np.int64)
CODE[[1, 2, 4, 8]] = [0, 1, 2, 3]


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def restated_keys(b, Q, L, mutant=None):
    """one batch -> (base keys, extension keys, Counter of the four push counters), a record at a time over numpy views of its bytes"""
    raw = np.frombuffer(bytes(b.raw), dtype=np.uint8)
    base, ext, sn = [], [], collections.Counter()
    word = lambda o, dt: int(raw[o:o + np.dtype(dt).itemsize].view(dt)[0])
    cap = 141 if mutant == "ext_cols_141" else 140
    for flag, tid, pos, mapq, ro in zip(*(np.asarray(getattr(b, k)).tolist() for k in D.COLUMNS)):
        if flag & (0x4 | 0x100 | 0x200 | 0x400 | 0x800) or tid < 0 or mapq < Q:
            continue
        ok = tid < 2 ** 24 and pos >= 0 and ro + 36 <= len(raw)
        if ok:
            block, l_name, nc, l_seq = word(ro, "<u4"), int(raw[ro + 12]), word(ro + 16, "<u2"), word(ro + 20, "<i4")
            ok = l_seq >= 0 and 32 + l_name + 4 * nc + (l_seq + 1) // 2 + l_seq <= block and ro + 4 + block <= len(raw)
        if ok:
            cig = raw[ro + 36 + l_name:ro + 36 + l_name + 4 * nc].view("<u4").astype(np.int64)
            ops, lens = cig & 15, cig >> 4
            reflen, qlen = int(lens[np.isin(ops, REF_CONSUMING)].sum()), int(lens[np.isin(ops, QUERY_CONSUMING)].sum())
            ok = not (ops > 8).any() and pos + reflen <= 2 ** 31 - 1 and not (l_seq >= 1 and nc >= 1 and qlen != l_seq)
        if not ok or nc == 0 or l_seq == 0 or reflen == 0:
            continue
        seq = raw[ro + 36 + l_name + 4 * nc:ro + 36 + l_name + 4 * nc + (l_seq + 1) // 2]
        nib = np.stack([seq >> 4, seq & 15], axis=1).ravel()[:l_seq]                   # every base's 4-bit code, in read order
        first = 1 if nc >= 2 and ops[0] == 5 else 0
        last = nc - 2 if nc >= 2 and ops[-1] == 5 else nc - 1
        clips = []
        if ops[first] == 4:
            n = int(lens[first])
            clips.append((0, n, nib[:n] if mutant == "l_not_reversed" else nib[:n][::-1], pos + 1))
        if ops[last] == 4:
            n = int(lens[last])
            clips.append((1, n, nib[l_seq - n:], pos + reflen))
        rev = 0 if mutant == "rev_dropped" else (flag >> 4) & 1
        for side, n, out, P in clips:
            if n < L:
                continue
            c = CODE[out[:cap]]
            stop = np.flatnonzero(c < 0)
            kept = c[:int(stop[0])] if len(stop) else c
            k = len(kept)
            sn["cut_beyond_28"] += (k < min(n, cap)) if mutant == "cut_counts_front" else (28 <= k < min(n, cap))
            pack = lambda v: int(sum(int(x) << (2 * j) for j, x in enumerate(v)))
            base.append((tid << 32 | P, side << 63 | min(k, 28) << 58 | pack(kept[:28]) << 2 | rev))
            if k > 28:
                sn["ext_right_events" if side else "ext_left_events"] += 1
            for ch in range(1, (k + 27) // 28):
                part = kept[28 * ch:28 * ch + 28]
                ext.append((ch << 56 | tid << 32 | P, side << 63 | len(part) << 58 | pack(part) << 2 | rev))
    sn["ext_keys"] += len(ext)
    return base, ext, +sn


def _chunk_vote(k2, S, mutant):
    """the K2 of one (chunk, site) -> (CLEN, winners): the vote of tdt_clip over the keys' 28 columns"""
    k2 = np.asarray(k2, dtype=np.uint64)
    n = ((k2 >> np.uint64(58)) & np.uint64(31)).astype(np.int64)
    cols = ((k2[:, None] >> (np.uint64(2) + np.uint64(2) * np.arange(28, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)
    live = np.arange(28)[None, :] < n[:, None]
    votes = np.stack([(live & (cols == c)).sum(axis=0) for c in range(4)], axis=1)     # [28][4]
    depth = votes.sum(axis=1)
    deep = depth > S if mutant == "depth_gt" else depth >= S
    clen = int(np.argmin(deep)) if not deep.all() else 28
    win = 3 - np.argmax(votes[:, ::-1], axis=1) if mutant == "tie_larger" else np.argmax(votes, axis=1)
    return clen, win[:clen].tolist()


def restated_sites(base, ext, S, mutant=None):
    """the sorted keys of the two stores -> [(K1, side, SUPPORT, ECLEN, codes)]: per reported site chunk 0's vote, then the further
    chunks' while the one in front had all 28 columns and the chunk has S keys"""
    groups = collections.defaultdict(list)
    for k1, k2 in sorted(base) + sorted(ext):
        groups[(k1, k2 >> 63)].append(k2)
    out = []
    for (k1, side), k2 in sorted(groups.items()):
        if k1 >> 56 or len(k2) < S:
            continue
        total, cons, c = 0, [], 0
        while c < 5:
            g = groups.get((c << 56 | k1, side)) if c else k2
            if g is None or len(g) < S:
                break
            clen, win = _chunk_vote(g, S, mutant)
            total, cons = total + clen, cons + win
            if clen < 28:
                break
            c += 1
        out.append((k1, side, len(k2), total, cons))
    return out


def restated_pairs(sites, K, O, M, mutant=None):
    """site rows -> rows as pairs_of_sites gives them, from arrays: the L rows found by a search over their keys, the closure by one
    comparison of two slices per candidate length"""
    k1 = np.array([s[0] for s in sites], dtype=np.int64) if sites else np.zeros(0, dtype=np.int64)      # (tid < 2^24: below 2^63)
    side = np.array([s[1] for s in sites], dtype=np.int64)
    eclen = np.array([s[3] for s in sites], dtype=np.int64)
    kmin = K - 1 if mutant == "k_minus_1" else K
    Ls = np.flatnonzero((side == 0) & (eclen >= kmin))
    lk = k1[Ls]
    far = {"tsd_31": 31, "tsd_33": 33}.get(mutant, 32)
    rows = []
    for i in np.flatnonzero((side == 1) & (eclen >= kmin)).tolist():
        tid, P = int(k1[i]) >> 32, int(k1[i]) & 0xffffffff
        hi = P + (2 if mutant == "l_right_2" else 1)
        for j in Ls[np.searchsorted(lk, (tid << 32) + P + 1 - far):].tolist():
            tj, Pj = int(k1[j]) >> 32, int(k1[j]) & 0xffffffff
            if mutant == "ignore_tid":
                if not P + 1 - far <= Pj <= hi:
                    continue
            elif tj != tid or Pj > hi or Pj < P + 1 - far:
                break
            x, yr = np.array(sites[i][4], dtype=np.int64), np.array(sites[j][4], dtype=np.int64)[::-1]
            a, b = len(x), len(yr)
            omin = O - 1 if mutant == "o_minus_1" else O
            found = []
            for l in range(omin, a + b - omin + 1):
                lo, top = max(0, l - b), min(a, l)
                if top - lo < omin:
                    continue
                mm = int(np.count_nonzero(x[lo:top] != yr[lo + b - l:top + b - l]))
                if (mm < M) if mutant == "mm_lt" else (mm <= M):
                    found.append((mm, -l if mutant == "best_largest" else l))
            if not found:
                rows.append((i, j, P + 1 - Pj, 0, 0, 0, 0, []))
                continue
            mm, l = min(found)
            l = abs(l)
            top = min(a, l)
            cut = max(0, l - b) if mutant == "seq_from_y" else top
            seq = x[:cut].tolist() + yr[cut + b - l:].tolist()
            rows.append((i, j, P + 1 - Pj, 1, l, mm, len(found), seq))
    return sorted(rows, key=lambda r: (r[0], int(k1[r[1]])))


def restated_key_case(case, mutant=None):
    base, ext, sn = [], [], collections.Counter()
    for b in D.batches(case):
        x, y, z = restated_keys(b, case["Q"], case["L"], mutant)
        base, ext = base + x, ext + y
        sn.update(z)
    return base, ext, +sn


# ---- keys ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.KEY_CASES, ids=[c["name"] for c in X.KEY_CASES])
def test_key_cases_definition_restatement_and_claim_agree(case):
    rows, sn, events = X.key_definition(case)
    assert X.key_agrees_with_claim(case, rows, sn) is None
    base, ext, rsn = restated_key_case(case)
    assert X.key_agrees_with_claim(case, D.key_rows(ext), rsn) is None
    # the first 28 columns are the event tiddit_clips keys
    want, _ = D.definition(case)
    assert np.array_equal(D.key_rows(base), want)
    got = [(k1, side << 63 | min(len(kept), 28) << 58 | sum(c << (2 * j) for j, c in enumerate(kept[:28])) << 2 | rev) for k1, side, rev, kept in events]
    assert np.array_equal(D.key_rows(got), want)
    assert all(len(e[3]) <= 140 for e in events)


def test_the_stated_key_cases_and_their_largest_read():
    assert len(X.KEY_CASES) == X.N_KEY_CASES == 11
    per_read = collections.Counter()
    case = next(c for c in X.KEY_CASES if c["name"].startswith("both:"))
    keys, sn = X.claimed_keys(case)
    assert len(keys) == 8 + 4 + 1 and X.MAX_PER_READ == I.CLIP_EXT_MAX_PER_READ == 8
    full = next(c for c in X.KEY_CASES if c["name"].startswith("store: every read"))
    assert len(X.claimed_keys(full)[0]) == 8 * X.K_TILE == full["capacity"]


MUTANTS = {"ext_cols_141": "length", "l_not_reversed": "phase", "rev_dropped": "length", "cut_counts_front": "other"}


@pytest.mark.parametrize("mutant,family", sorted(MUTANTS.items()))
def test_a_departure_of_the_key_restatement_is_noticed_in_its_family(mutant, family):
    noticed = []
    for case in X.KEY_CASES:
        if case["family"] == family:
            _, ext, sn = restated_key_case(case, mutant)
            noticed.append(X.key_agrees_with_claim(case, D.key_rows(ext), sn) is not None)
    assert any(noticed), mutant


# ---- consensus -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CONS_CASES, ids=[c["name"] for c in X.CONS_CASES])
def test_consensus_cases_definition_restatement_and_claim_agree(case):
    S = case["min_support"]
    want = X.literal_sites(case)
    assert X.cons_definition(case) == want
    base, ext, _ = restated_key_case(case)
    assert restated_sites(base, ext, S) == want
    # columns 0 ... 27 equal CLEN / CONSENSUS of the clip table's row
    _, rows = tiddit_clips.summarise(base, None, S)
    assert [(r[0], r[1], r[2]) for r in rows] == [(s[0], s[1], s[2]) for s in want]
    for r, s in zip(rows, want):
        assert r[5] == min(s[3], 28) and r[6] == sum(c << (2 * j) for j, c in enumerate(s[4][:28]))


def test_the_key_cases_sites_agree_too():
    for case in X.KEY_CASES:
        base, ext, _ = restated_key_case(case)
        events = X.key_definition(case)[2]
        for S in (1, 2, 3):
            assert restated_sites(base, ext, S) == I.extended_sites(events, S), (case["name"], S)


@pytest.mark.parametrize("mutant", ["tie_larger", "depth_gt"])
def test_a_departure_of_the_consensus_restatement_is_noticed(mutant):
    noticed = []
    for case in X.CONS_CASES:
        base, ext, _ = restated_key_case(case)
        noticed.append(restated_sites(base, ext, case["min_support"], mutant) != X.literal_sites(case))
    assert any(noticed), mutant


# ---- pairs and closures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.PAIR_CASES, ids=[c["name"] for c in X.PAIR_CASES])
def test_pair_cases_definition_restatement_and_claim_agree(case):
    counts, rows = X.pair_definition(case)
    assert X.pair_agrees_with_claim(case, counts, rows) is None
    assert [tuple(r) for r in restated_pairs(X.sites_of(case), case["K"], case["O"], case["M"])] == X.literal_rows(case)


def test_the_stated_pair_cases():
    assert len(X.PAIR_CASES) == X.N_PAIR_CASES == 33
    fams = collections.Counter(c["family"] for c in X.PAIR_CASES)
    assert fams == {"pairs": 9, "closure": 24}


PAIR_MUTANTS = {"tsd_31": "pairs", "tsd_33": "pairs", "l_right_2": "pairs", "ignore_tid": "pairs", "k_minus_1": "pairs", "o_minus_1": "closure", "mm_lt": "closure",
                "best_largest": "closure", "seq_from_y": "closure"}


@pytest.mark.parametrize("mutant,family", sorted(PAIR_MUTANTS.items()))
def test_a_departure_of_the_pair_restatement_is_noticed_in_its_family(mutant, family):
    noticed = [[tuple(r) for r in restated_pairs(X.sites_of(c), c["K"], c["O"], c["M"], mutant)] != X.literal_rows(c) for c in X.PAIR_CASES if c["family"] == family]
    assert any(noticed), mutant


def test_every_length_from_O_to_268_closes_at_its_own_length():
    case = X.every_length_case()
    assert len(case["rows"]) == 268 - 12 + 1 and {r[4] for r in case["rows"]} == set(range(12, 269))
    counts, rows = X.pair_definition(case)
    assert X.pair_agrees_with_claim(case, counts, rows) is None
    assert [tuple(r) for r in restated_pairs(X.sites_of(case), case["K"], case["O"], case["M"])] == X.literal_rows(case)
    # every phase of the shift between the two strings: b - l runs over every residue of 32 on both signs
    assert {(140 - r[4]) % 32 for r in case["rows"] if r[4] < 140} == set(range(32)) == {(r[4] - 140) % 32 for r in case["rows"] if r[4] > 140}


def test_packing_round_trips():
    codes = X.codes(X.seeded(140, 5))
    assert I.unpack_words(I.pack_words(codes, 5), 140) == codes and all(w < 1 << 56 for w in I.pack_words(codes, 5))
    long = X.codes(X.seeded(272, 6))
    assert I.unpack_words(I.pack_words(long, I.SEQ_WORDS), 272) == long


# ---- the job's reads -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def job():
    g, ins = X.job_genome()
    reads = X.job_reads(g, ins)
    b = D.build_batch(reads)
    events, keys, sn = [], [], {}
    I.events_of_batch_by_read(b, events, keys, sn, X.JOB_Q, X.JOB_L)
    return g, ins, reads, b, events, keys, sn


def test_the_generator_meets_its_condition(job):
    """every junction is covered by at least S reads per side whose clips reach K columns; the reference has about 20 kb in two contigs"""
    g, ins, reads, b, events, keys, sn = job
    assert len(g) == 2 and len(g[0].b) + len(g[1].b) == 20000
    assert sorted({n for _, _, _, n in X.PLANTED}) == [60, 130, 250, 600] and {tsd for _, _, tsd, _ in X.PLANTED} == {0, 15}
    for t, P, tsd, n in X.PLANTED:
        for k1, side in ((t << 32 | P, 1), (t << 32 | (P + 1 - tsd), 0)):
            reach = [e for e in events if e[0] == k1 and e[1] == side and len(e[3]) >= X.JOB_K]
            assert len(reach) >= X.JOB_S, (t, P, side, len(reach))


def test_the_definition_finds_the_planted_insertions(job, tmp_path):
    g, ins, reads, b, events, keys, sn = job
    path = str(tmp_path / "want.clips.ins.tab")
    counts = I.definition_file(path, events, sn, ["chrA", "chrB"], X.JOB_S, X.JOB_K, X.JOB_O, X.JOB_M)
    text = open(path).read()
    assert text.startswith("# tiddit_amd clips_ins v1 cols=140 max_tsd=32 min_cols=20 min_overlap=12 max_mismatch=1\nSN\text_left_events\t")
    lines = text.split("\n")
    assert [l.split("\t")[1] for l in lines[1:12]] == list(I.SN) and lines[12] + "\n" == I.COLUMNS
    table = [l.split("\t") for l in lines[13:] if l]
    # CHROM POS END TSD R_SUPPORT L_SUPPORT R_COLS L_COLS STATUS LEN MISMATCH CLOSURES SEQ LEFT_SEQ RIGHT_SEQ
    assert [[r[0], r[1], r[2], r[3], r[8], r[9], r[12]] for r in table] == X.job_expected_rows(ins)
    assert all(r[4:8] == ["7", "7", "140", "140"] for r in table) and all(r[10] == "0" for r in table if r[8] == "CLOSED")
    big = table[-1]
    assert big[8] == "OPEN" and big[9:13] == [".", ".", "0", "."] and big[13] == ins[-1][:140] and big[14] == ins[-1][-140:]
    v = lambda k: int(counts[I.SN_INDEX[k]])
    assert (v("pairs"), v("closed"), v("open"), v("left_sites"), v("right_sites"), v("sites_extended")) == (7, 6, 1, 7, 7, 14)
    assert v("ext_keys") == len(keys) == 14 * (1 + 2 + 3 + 4 + 3 * 4) and v("ext_left_events") == v("ext_right_events") == 7 * 7 and v("cut_beyond_28") == 0
    assert I.summary_line(counts) == ("clips ins: 308 extension keys, 14 sites extended, 7 left and 7 right sites, 7 pairs, 6 closed (0 with several closures), "
                                      "1 open")


def test_the_result_does_not_depend_on_the_order_of_the_reads(job):
    g, ins, reads, b, events, keys, sn = job
    a = I.summarise(events, sn, X.JOB_S, X.JOB_K, X.JOB_O, X.JOB_M)
    r = I.summarise(events[::-1], sn, X.JOB_S, X.JOB_K, X.JOB_O, X.JOB_M)
    assert np.array_equal(a[0], r[0]) and a[1] == r[1] and a[2] == r[2]


# ---- the switch ------------------------------------------------------------------------------------------------------------------
def test_the_switch():
    assert I.parse_switch(None) is None and I.parse_switch("") is None and I.parse_switch(None, clips=False) is None
    assert I.parse_switch("1") == (20, 12, 1) and I.parse_switch("10") == (10, 12, 1) and I.parse_switch("140:140:8") == (140, 140, 8)
    assert I.parse_switch("25:8") == (25, 8, 1) and I.parse_switch("25:8:0") == (25, 8, 0)
    for value, text in (("9", "the minimum extended-consensus columns are 10 ... 140"), ("141", "the minimum extended-consensus columns are 10 ... 140"),
                        ("20:7", "the minimum overlap is 8 ... 140"), ("20:141", "the minimum overlap is 8 ... 140"), ("20:12:9", "the maximum mismatches are 0 ... 8"),
                        ("yes", None), ("20:12:1:1", None), ("-20", None), ("20:", None), ("0", "the minimum extended-consensus columns are 10 ... 140")):
        with pytest.raises(ValueError) as e:
            I.parse_switch(value)
        assert str(e.value) == (text or "the switch is 1, K, K:O or K:O:M (minimum extended-consensus columns 10 ... 140, minimum overlap 8 ... 140, maximum "
                                        "mismatches 0 ... 8)")
    with pytest.raises(ValueError) as e:
        I.parse_switch("1", clips=False)
    assert str(e.value) == "the switch pairs the sites of TIDDIT_CLIPS, which is not set"
