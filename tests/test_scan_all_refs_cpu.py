"""The file of tests/scan_all_cases.py holds what it says it holds — so that tests/test_gpu_scan_all.py can never pass on an empty table —
is the same bytes when made twice, and every consumer's definition over it is what the GPU tests need it to be: independent of where the
host batches are cut, and changed by any one batch left out or fed twice.  The comparison helper of the GPU module names the part in
which a result departs from its definition, and the GPU module's tables name every consumer global the scan of tiddit_signal reads and
every switch any docstring of the package's ``__main__`` names."""
import ast
import collections
import copy
import os
import re

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
    """(67 936 records with the clip events planted, 1 250 of them theirs: the bound of 80 000 stands)"""
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


def test_str(made):
    """(on the file as it stands: 496 loci, 4 210 keys — 2 881 span, 724 left, 605 right —, 48 unanchored, 252 over the cap of four, 4 222
    reads in reach, 446 loci genotyped, 186 of them heterozygous, 18 flagged LONGER; every floor is half of that)"""
    from tiddit_amd import tiddit_str as T
    d, info, batches, parts, E = made
    table = C.contigs()
    loci = T.read_loci(C.str_path(d), [n for n, _ in table], [l for _, l in table])
    assert loci.rows == C.str_loci().rows and len(loci) == len(C.grid_points()) >= 248 and not any(loci.skipped.values())
    seqs = C.reference()[0]
    for chrom, s, e, unit, _ in loci.rows:                                     # the catalogue's motif is in phase with the reference at start
        assert seqs[chrom][s:e].tobytes().decode() == (unit * 16)[:e - s]
    keys, counts, cols, tab = E["str"]
    v = lambda k: int(counts[T.SN_INDEX[k]])
    assert len(keys) == v("span_keys") + v("left_keys") + v("right_keys") >= 2105
    assert v("span_keys") >= 1440 and v("left_keys") >= 362 and v("right_keys") >= 302 and v("unanchored") >= 24 and v("over_cap") >= 126
    assert all(v(k) > 0 for k in ("span_keys", "left_keys", "right_keys", "unanchored", "over_cap"))
    assert v("in_reach") >= 2111 and v("malformed") == 0 and v("records") == E["records"]
    assert len(cols) == 4 and len(cols[0]) > 0 and int(cols[2].sum()) == len(keys) and int((cols[3] > 0).sum()) > 0
    called = [t[2] for t in tab if t[2] is not None]
    assert len(tab) == len(loci) and len(called) >= 223 and sum(1 for g in called if g[0] != g[2]) >= 93
    assert sum(t[5] for t in tab) >= 9                                         # LONGER
    assert sum(1 for p in parts if p["str_keys"]) >= len(parts) - 2            # (keys in nearly every batch)


def test_str_equals_the_restatement_of_its_case_module(made):
    """``str_cases.reference_batch`` over the same batches (it looks contigs up in its module's ``NAMES``: set to this file's for the call)"""
    import str_cases as D
    from tiddit_amd import tiddit_str as T
    d, info, batches, parts, E = made
    loci = [r[:4] for r in C.str_loci().rows]
    keys, sn = [], collections.Counter()
    names, D.NAMES = D.NAMES, tuple(n for n, _ in C.contigs())
    try:
        for b in batches:
            D.reference_batch(b, loci, keys, sn, C.STR_F, C.STR_Q)
    finally:
        D.NAMES = names
    assert len(keys) >= 2105
    assert C._eq(C.str_result(keys, {k: n for k, n in sn.items() if n}), E["str"])


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


def test_every_batch_yields_an_snv_key_and_a_clip_key(made):
    d, info, batches, parts, E = made
    assert len(parts) >= 24
    for i, p in enumerate(parts):
        assert len(p["snv_keys"]) >= 1 and len(p["clip_keys"]) >= 1, i
    assert len(E["clip_ext"]) > 0 and sum(len(p["ext_keys"]) for p in parts) == len(E["clip_ext"])
    assert sum(1 for p in parts if p["ext_keys"]) >= len(parts) - 2           # (clips of more than 28 columns nearly everywhere)
    # both supports report rows, and the smaller support more of them
    for name, supports in (("snvs", C.SNV_SUPPORTS), ("clips", C.CLIP_SUPPORTS)):
        n = [len(E[name][1][s][1][0]) for s in supports]
        assert n[0] > n[1] >= 100, (name, n)
    k1, side, sup, rev = E["clips"][1][C.CLIP_S][1][:4]
    assert int(((sup >= 4) & (rev >= 1) & (sup > rev)).sum()) >= 200           # the planted sites: support >= 4 on both strands


def test_the_clip_chain_holds_every_class_of_event(made):
    from tiddit_amd import tiddit_clip_ins as I, tiddit_clip_mei as M
    d, info, batches, parts, E = made
    chain = E["clip_chain"]
    align, far, ins, mei = (chain[k][1] for k in ("align", "far", "ins", "mei"))
    # mated DEL junctions from align, some of them with a microhomology
    dels = [r for r in align if r[2] == 1 and r[9] == "DEL" and r[11] is not None]
    assert len(dels) >= 3 and sum(1 for r in dels if r[12] > 0) >= 3 and sum(1 for r in dels if r[12] == 0) >= 3
    assert info["clip_deletions"] >= 3 and info["clip_hom_deletions"] >= 3
    # placements that only far finds: on another contig, where align has nothing
    unaligned = {r[:3] for r in align if r[9] is None}
    only_far = [r for r in far if r[10] is not None and r[:3] in unaligned]
    assert len(only_far) >= 3 and sum(1 for r in only_far if r[10] == "BND" and r[13] is not None) >= 3 and info["clip_translocations"] >= 3
    # closed and open pairs
    assert sum(1 for r in ins if r[8] == I.CLOSED) >= 3 and sum(1 for r in ins if r[8] == I.OPEN) >= 3
    assert sum(1 for r in ins if r[3] > 0) >= 3 and sum(1 for r in ins if r[3] == 0) >= 3               # with and without a target-site duplication
    # named pairs
    calls = M.calls_for_vcf(mei, C.MEI_MIN, [n for n, _ in C.library()])
    assert len(calls) >= 3 and sum(1 for c in calls.values() if c[1] == "-") >= 1 and len({c[0] for c in calls.values()}) >= 2
    assert info["clip_minus"] >= 1
    # the VCF
    counts, lines = chain["vcf"]
    kinds = [dict(kv.split("=", 1) for kv in l.split("\t")[7].split(";")) for l in lines]
    assert sum(1 for k in kinds if k["SVTYPE"] == "DEL") >= 1 and sum(1 for k in kinds if k["SVTYPE"] == "BND") >= 2
    assert sum(1 for l, k in zip(lines, kinds) if k["SVTYPE"] == "INS" and "MEI" in k and "\t<INS>\t" in l) >= 1
    assert counts["records"] == len(lines) and counts["junctions"] >= 6 and counts["ins_rows"] >= 6


def test_the_definitions_files_are_written_and_hold_the_chains_rows(made, tmp_path):
    d, info, batches, parts, E = made
    prefix = str(tmp_path / "want")
    C.write_definition_files(prefix, parts, E, C.library_path(d))
    for ext in C.STAGE_FILES + (C.STR_FILE,):
        assert os.path.getsize(prefix + ext) > 500, ext
    body = [l.split("\t") for l in open(prefix + C.STR_FILE).read().split("\n") if l and not l.startswith(("#", "SN\t"))]
    assert len(body) == len(E["str"][3]) and sum(1 for f in body if f[11] != ".") == sum(1 for t in E["str"][3] if t[2] is not None)
    body = [l for l in open(prefix + ".clips.vcf").read().split("\n") if l and not l.startswith("#")]
    assert body == E["clip_chain"]["vcf"][1]
    for ext, stage in ((".clips.align.tab", "align"), (".clips.far.tab", "far"), (".clips.ins.tab", "ins"), (".clips.mei.tab", "mei")):
        rows = [l for l in open(prefix + ext).read().split("\n") if l and not l.startswith(("#", "SN\t"))]
        assert len(rows) == len(E["clip_chain"][stage][1]), ext


def test_the_file_is_the_same_bytes_when_made_twice(made, tmp_path):
    d = made[0]
    C.generate(str(tmp_path), threads=2)
    for a, b in zip(C.paths(d) + (C.library_path(d), C.str_path(d)), C.paths(str(tmp_path)) + (C.library_path(str(tmp_path)), C.str_path(str(tmp_path)))):
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


# ---- the GPU module's comparison helper and tables ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def right(made, tmp_path_factory):
    """what an all-on run that is right leaves behind, from the definitions alone"""
    import test_gpu_scan_all as G
    d, info, batches, parts, E = made
    prefix = os.path.join(str(tmp_path_factory.mktemp("scan_all_files")), "want")
    C.write_definition_files(prefix, parts, E, C.library_path(d))
    files = {ext: G._content(prefix + ext) for ext in C.STAGE_FILES + (C.STR_FILE,)}
    return G, E, files


def _one_snv_key_dropped(R):
    R["snvs"] = (R["snvs"][0][1:], R["snvs"][1])


def _one_snv_row_support_off(R):
    R["snvs"][1][C.SNV_SUPPORTS[1]][1][2][0] += 1


def _one_clip_consensus_changed(R):
    R["clips"][1][C.CLIP_S][1][6][5] ^= 1


def _one_extension_key_changed(R):
    R["clips"][2][0, 1] ^= 4


def _one_align_partner_moved(R):
    rows = R["chain"]["rows"]["align"]
    i = next(i for i, r in enumerate(rows) if r[5] is not None)
    rows[i] = rows[i][:5] + (rows[i][5] + 1,) + rows[i][6:]


def _one_mei_family_changed(R):
    rows = R["chain"]["rows"]["mei"]
    rows[0] = rows[0][:6] + ((rows[0][6] + 1) % 3,) + rows[0][7:]


def _one_boundary_support_off_by_one(R):
    lines = R["chain"]["files"][".clips.vcf"].split(b"\n")
    i = next(i for i, l in enumerate(lines) if l and not l.startswith(b"#"))
    f = lines[i].split(b"\t")
    sample = f[9].split(b":")                                                   # GT:RV:RR:LQ:DPF
    a, b = sample[2].split(b",")
    sample[2] = b"%d,%s" % (int(a) + 1, b)
    f[9] = b":".join(sample)
    lines[i] = b"\t".join(f)
    R["chain"]["files"][".clips.vcf"] = b"\n".join(lines)


def _one_str_key_dropped(R):
    R["str"] = (R["str"][0][1:],) + R["str"][1:]


def _one_str_row_support_off(R):
    R["str"][2][2][0] += 1


def _one_str_file_line_changed(R):
    lines = R["str"][4].split(b"\n")
    i = next(i for i, l in enumerate(lines) if l and not l.startswith((b"#", b"SN\t")) and l.split(b"\t")[11] == b"0/1")
    f = lines[i].split(b"\t")
    f[11] = b"1/1"
    lines[i] = b"\t".join(f)
    R["str"] = R["str"][:4] + (b"\n".join(lines),)


DEPARTURES = ((_one_snv_key_dropped, "snvs: the keys"), (_one_snv_row_support_off, "snvs: row column 2"), (_one_clip_consensus_changed, "clips: row column 6"),
              (_one_extension_key_changed, "clips: the extension keys"), (_one_align_partner_moved, "chain: column 5 of the align rows"),
              (_one_mei_family_changed, "chain: column 6 of the mei rows"), (_one_boundary_support_off_by_one, "chain: the file .clips.vcf"),
              (_one_str_key_dropped, "str: the keys"), (_one_str_row_support_off, "str: row column 2"), (_one_str_file_line_changed, "str: the file .str.tab"))


def test_the_comparison_passes_on_the_definitions_and_names_each_departure(right):
    G, E, files = right
    G._equals_definitions(G._as_run(E, files), E, files)
    noticed = 0
    for depart, named in DEPARTURES:
        R = copy.deepcopy(G._as_run(E, files))
        depart(R)
        with pytest.raises(AssertionError) as e:
            G._equals_definitions(R, E, files)
        assert str(e.value).startswith(named), (depart.__name__, str(e.value)[:200])
        assert G._differing(R, G._as_run(E, files), ("snvs", "clips", "chain", "str")) == [named.split(":")[0]]
        noticed += 1
    assert noticed == len(DEPARTURES) == 10                                    # departures, each noticed and named


# the all-capitals globals of tiddit_signal that __main__ sets or the scan reads and that attach nothing: timings, seams, the track's result
NOT_CONSUMERS = ("AFTER_SCAN", "BACKGROUND_WRITES", "COV_TRACK_BINS", "STAGE_SECONDS", "WRITE_SECONDS", "LAST_SEAM", "READER_SECONDS", "SCAN_SECONDS")


def scan_globals(source):
    """the module-level all-capitals names of tiddit_signal's source that ``_scan`` or a module function it calls (at any depth) reads or
    sets: what a scan can be steered by or leave behind, however ``__main__`` or anybody else attaches it"""
    tree = ast.parse(source)
    top = {t.id for n in tree.body if isinstance(n, (ast.Assign, ast.AnnAssign)) for t in (n.targets if isinstance(n, ast.Assign) else [n.target])
           if isinstance(t, ast.Name) and re.fullmatch(r"[A-Z][A-Z0-9_]*", t.id)}
    functions = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    seen, todo, names = set(), ["_scan"], set()
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for n in ast.walk(functions[f]):
            if isinstance(n, ast.Name):
                names |= {n.id} & top
                todo += [n.id] if n.id in functions else []
            elif isinstance(n, ast.Global):
                names |= set(n.names) & top
    return names


def test_every_consumer_switch_and_counter_of_the_scan_is_driven_by_the_attachable_table():
    import test_gpu_scan_all as G
    from tiddit_amd import tiddit_signal as S
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(repo, "tiddit_amd", "__main__.py")).read()
    counters = {n for n in vars(S) if n.endswith("_COUNTER")}
    # from tiddit_signal itself — a consumer counts however it is attached (tiddit_str.attach sets STR from its own module) — and, as
    # before, what __main__ names
    in_scan = scan_globals(open(os.path.join(repo, "tiddit_amd", "tiddit_signal.py")).read())
    assert counters <= in_scan <= set(vars(S))
    switches = (in_scan | set(re.findall(r"tiddit_signal\.([A-Z][A-Z_]*)\b", source))) - set(NOT_CONSUMERS) - counters
    assert counters >= {"ALLELE_COUNTER", "QC_COUNTER", "DUP_COUNTER", "INDEL_COUNTER", "SNV_COUNTER", "CLIP_COUNTER"}
    assert switches >= {"COV_TRACK", "KEEP_EVIDENCE", "ALLELES", "QC", "DUPS", "INDELS", "SNVS", "CLIPS", "CLIPS_INS"}
    driven = [n for names in G.DRIVES.values() for n in names]
    assert len(driven) == len(set(driven)) and tuple(G.DRIVES) == G.ATTACHABLE
    assert counters | switches == set(driven), sorted((counters | switches) ^ set(driven))
    assert all(hasattr(S, n) for n in driven) and set(driven) <= in_scan         # (whatever the table drives, the scan itself reads or sets)
    assert all(getattr(S, n) is G.OFF.get(n) for n in driven)                  # (and every one of them is off as the module is imported)


def test_every_switch_the_package_names_is_stripped_from_the_jobs_environment():
    import test_gpu_scan_all as G
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tree = ast.parse(open(os.path.join(repo, "tiddit_amd", "__main__.py")).read())
    # every docstring of the file, not the module's alone: a switch documented at the function that reads it counts as much
    docs = [ast.get_docstring(n) for n in ast.walk(tree) if isinstance(n, (ast.Module, ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef))]
    named = set(re.findall(r"TIDDIT_[A-Z0-9_]*[A-Z0-9]", "\n".join(d for d in docs if d)))
    assert len(docs) >= 2 and {"TIDDIT_STR", "TIDDIT_STR_CUTS"} <= named
    assert len(named) >= 19 and {"TIDDIT_SNVS", "TIDDIT_CLIPS", "TIDDIT_CLIPS_ALIGN", "TIDDIT_CLIPS_FAR", "TIDDIT_CLIPS_INS", "TIDDIT_CLIPS_VCF", "TIDDIT_CLIPS_MEI"} <= named
    assert len(G.NOT_SCAN_SWITCHES) <= 4 and not set(G.NOT_SCAN_SWITCHES) & set(G.ALL_SWITCHES)
    left = named - set(G.ALL_SWITCHES) - set(G.NOT_SCAN_SWITCHES)
    assert not left, sorted(left)
    assert len(set(G.ALL_SWITCHES)) == len(G.ALL_SWITCHES)
