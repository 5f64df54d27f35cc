"""The file of tests/scan_all_cases.py holds what it says it holds — so that tests/test_gpu_scan_all.py can never pass on an empty table —
is the same bytes when made twice, and every consumer's definition over it is what the GPU tests need it to be: independent of where the
host batches are cut, and changed by any one batch left out or fed twice."""
import os

import numpy as np
import pytest

import scan_all_cases as C


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("scan_all"))
    info = C.generate(d)
    batches = C.host_batches(C.paths(d)[0])
    parts = C.partials(d)
    assert len(parts) == len(batches)
    return d, info, batches, parts, C.combine(parts)


def test_size_contigs_and_the_unplaced_tail(made):
    d, info, batches, parts, E = made
    table = C.contigs()
    assert 30000 <= info["n_records"] == E["records"] <= 80000
    assert os.path.getsize(C.paths(d)[0]) >= 24 * 65536
    assert sum(L >= C.MIN_CONTIG for _, L in table) >= 3 and sum(L < C.MIN_CONTIG for _, L in table) >= 1
    tid = np.concatenate([b.tid for b in batches])
    placed = np.flatnonzero(tid >= 0)
    assert 0 < len(placed) < len(tid) and placed[-1] == len(placed) - 1          # a tail of unplaced reads, behind every placed one
    assert np.all(np.diff(tid[placed]) >= 0)
    small = [t for t, (_, L) in enumerate(table) if L < C.MIN_CONTIG]
    assert np.isin(tid, small).sum() >= 3                                      # reads on a contig below --min_contig


def test_indels(made):
    from tiddit_amd import tiddit_indels as T
    d, info, batches, parts, E = made
    keys, by_support = E["indels"]
    nkeys, nby, norm = E["indels_norm"]
    v = lambda c, k: int(c[T.SN_INDEX[k]])
    c1, rows1 = by_support[1]
    assert v(c1, "distinct_events") >= 200 and v(c1, "insertions") > 0 and v(c1, "deletions") > 0 and v(c1, "malformed") == 0
    k1, k2, sup, rev = by_support[3][1]
    assert int(((rev > 0) & (sup > rev)).sum()) >= 50                          # support >= 3, carried on both strands
    ins, ln, kind = k2 >> np.uint64(63), (k2 >> np.uint64(47)) & np.uint64(0xffff), (k2 >> np.uint64(45)) & np.uint64(3)
    assert int(((ins == 1) & (ln > T.PACK_MAX) & (kind == 1)).sum()) >= 1 and info["long_insertions"] >= 1       # the hashed payload
    assert int(((ins == 1) & (kind == 0)).sum()) >= 1 and int((ins == 0).sum()) >= 1
    assert v(c1, "noisy_reads") >= 1 and v(c1, "unanchored") >= 1
    # the events inside repeats: one row each with the reference attached, one per placement without it
    assert info["repeat_events"] >= 20
    assert len(nby[1][1][0]) + 20 <= len(rows1[0]) and norm[0] > 0              # strictly fewer rows, by at least the 20 events
    assert len(nkeys) == len(keys) and not np.array_equal(nkeys, keys)
    assert len(nby[3][1][0]) >= len(by_support[3][1][0]) + 20                  # (placements of support 1 became events of support 3 and 4)


def test_duplicates(made):
    from tiddit_amd import tiddit_dup as T
    d, info, batches, parts, E = made
    rows, c = E["dups"]
    v = lambda k: int(c[T.SN_INDEX[k]])
    assert v("pairs") > 0 and v("pairs") - v("pairs_no_mc") >= 1000 and v("pairs_no_mc") > 0 and v("malformed") == 0       # pairs with and without MC
    hist = c[T.OFF_HIST:].reshape(-1, 2)                                       # [size - 1][pair sets, fragment sets]
    assert all(hist[s - 1][0] > 0 and hist[s - 1][1] > 0 for s in range(2, 7))
    assert int(hist[1:6].sum()) >= 300 and int(hist[1:6, 0].sum()) >= 100 and int(hist[1:6, 1].sum()) >= 100
    # sets whose members lie far apart in the compressed file: more than two 64-KiB spans between them
    m = C.merged_batch(batches)
    at = C.compressed_offsets(C.paths(d)[0])
    assert len(at) == len(m)
    raw = memoryview(m.raw)
    sets = {}
    for i in np.flatnonzero((m.flag & 0x1) == 0).tolist():
        kind, k1, k2, _, _ = T.key_of_read(int(m.flag[i]), int(m.tid[i]), int(m.pos[i]), int(m.end[i]), int(m.mate_tid[i]), int(m.mate_pos[i]),
                                           int(m.rec_off[i]), raw)
        if kind == T.FRAGMENT:
            sets.setdefault((k1, k2), []).append(int(at[i]))
    far = [max(s) - min(s) for s in sets.values() if len(s) >= 2 and max(s) - min(s) > 2 * 65536]
    assert len(far) >= 3 and info["far_sets"] >= 3, (len(far), info["far_sets"])


def test_alleles(made):
    d, info, batches, parts, E = made
    table, used, bad = E["alleles"]
    sites = C.sites_table(d)
    assert len(sites) == len(table) >= 500 and not any(sites.skipped.values()) and len(sites.rows) == len(info["sites"])
    assert int((np.diff(sites.site_off) > 0).sum()) >= 3
    het = np.array([s[4] for s in info["sites"]])
    assert abs(het.mean() - 1 / 3) < 0.02
    col = {"A": 0, "C": 1, "G": 2, "T": 3}
    ref_n = sum(int(table[k][col[r]]) for (_, _, r, a, k), h in zip(sites.rows, het) if h)
    alt_n = sum(int(table[k][col[a]]) for (_, _, r, a, k), h in zip(sites.rows, het) if h)
    assert 0.4 < alt_n / (ref_n + alt_n) < 0.6, (ref_n, alt_n)                 # about half of the reads over a heterozygous site
    assert int(table[:, 7].sum()) > 0 and int(table[:, :4].sum()) > 0          # base qualities on both sides of min_bq
    assert used > 0 and bad == 0
    assert int(((table[:, :4] > 0).sum(axis=1) >= 2).sum()) >= 300


def test_signals(made):
    import oracle
    from oracle import signal_oracle
    d, info, batches, parts, E = made
    header, sq, raw = signal_oracle.inflate_bam(C.paths(d)[0])
    f = oracle.bam_walk(raw)
    chromosomes = [c["SN"] for c in sq if c["LN"] >= C.MIN_CONTIG]
    res, clips = signal_oracle._workers_over_fields(sq, raw, f, chromosomes, C.MIN_Q, C.MAX_INS, C.MIN_ANCHOR, C.MIN_CLIP)
    assert sum(len(r[1]) for r in res) >= 100 and sum(len(r[2]) for r in res) >= 100 and sum(t.count(">") for t in clips.values()) >= 100
    assert sum(int(C.signal_selected(b).sum()) for b in batches) >= 300


def test_every_batch_holds_something_for_every_consumer(made):
    d, info, batches, parts, E = made
    assert len(batches) >= 24
    rows = E["dups"][0]
    uniq, count = np.unique(rows[:, :2], axis=0, return_counts=True)
    in_set = {tuple(r) for r in uniq[count >= 2].tolist()}
    bare = []
    for i, (b, p) in enumerate(zip(batches, parts)):
        has = (len(p["indel_keys"]) > 0, any((k1, k2) in in_set for k1, k2, _ in p["dup_keys"]), p["allele_stats"][0] > 0, bool(C.signal_selected(b).any()))
        if not all(has):
            bare.append((i, has))
    assert len(bare) <= 2, bare


def test_the_file_is_the_same_bytes_when_made_twice(made, tmp_path):
    d = made[0]
    C.generate(str(tmp_path), threads=2)
    for a, b in zip(C.paths(d), C.paths(str(tmp_path))):
        assert open(a, "rb").read() == open(b, "rb").read(), os.path.basename(a)


def test_every_definition_is_invariant_to_where_the_batches_are_cut(made):
    d, info, batches, parts, E = made
    sites, ref = C.sites_table(d), C.host_reference()
    small = C.host_batches(C.paths(d)[0], 1 << 16)
    assert 2 * len(small) > 3 * len(batches)                                   # (pieces of at most 128 KiB against 256 KiB)
    assert C.differing(C.combine([C.partial(b, sites, ref) for b in small]), E) == []
    assert C.differing(C.combine([C.partial(C.merged_batch(batches), sites, ref)]), E) == []


@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_one_batch_left_out_or_fed_twice_changes_every_result(made, which):
    d, info, batches, parts, E = made
    i = {"first": 0, "middle": len(parts) // 2, "last": len(parts) - 1}[which]
    assert C.differing(C.combine(parts[:i] + parts[i + 1:]), E) == list(C.CONSUMERS)
    assert C.differing(C.combine(parts[:i + 1] + parts[i:]), E) == list(C.CONSUMERS)
