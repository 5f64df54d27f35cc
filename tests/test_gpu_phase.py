"""`TIDDIT_PHASE` on the GPU: the kernels of csrc/tdt_phase.hip on every aimed case of tests/phase_cases.py through both push entries of
the allele handle — ``tdt_alleles_push`` on host columns, ``tdt_alleles_push_device`` on the batches a ``DeviceBamReader`` decodes from a
small BAM written from the case's records — the store, the link rows, per-site (root, phase), the blocks and every counter against the
definition, exactly; every graph case through ``tdt_phase_forest`` and ``tdt_phase_forest_device`` on poisoned and padded outputs; the
handle's state and its refusals; and the switch end to end on a generated 20-kb, two-contig reference with two planted haplotypes, every
job a fresh child process under its own time limit (the first job that fails ends the fixture: nothing more is started behind a crash, a
time-out or a GPU error).

Every test of this file fails on the parent commit: the module, the symbols and the switch do not exist there."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import phase_cases as D
from clip_align_cases import fasta_raw, other, seeded

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = []
READER_OK = [c for c in D.CASES if c["reader_ok"]]
PAD = 16


def _counter(case, ctx=None, capacity=None, phase=True):
    from tiddit_amd import tiddit_alleles
    s, codes = D.sites_of(case)
    return tiddit_alleles.AlleleCounter(s.site_pos, s.site_off, case["min_q"], case["min_bq"], ctx=ctx,
                                        phase=(codes, capacity or case["capacity"] or 1 << 12, case["hash_bits"], case["S"], case["H"]) if phase else None)


@pytest.fixture(scope="module")
def wanted():
    return {c["name"]: D.definition(c) for c in D.CASES}


def _same(h, case, want, what):
    from tiddit_amd import tiddit_phase
    keys, sn, table, het, result = want
    k1, k2 = tiddit_phase.device_keys(h)
    assert k1.dtype == k2.dtype == np.uint64
    got = D.key_rows(list(zip(k1.tolist(), k2.tolist())))
    assert np.array_equal(got, D.key_rows(keys)), (what, got[:6].tolist(), D.key_rows(keys)[:6].tolist())
    counts, used, bad = h.counts()
    assert np.array_equal(counts, table), what
    dhet, _, _ = tiddit_phase.het_flags(counts, D.sites_of(case)[1], case["H"])
    assert np.array_equal(dhet, het)
    dev = tiddit_phase.device_finish(h, dhet, case["S"])
    assert {k: dev["sn"][k] for k in tiddit_phase.PUSH} == sn, (what, dev["sn"], sn)
    assert D.same_result(dev, result), (what, dev["sn"], result["sn"], [x.tolist()[:6] for x in dev["links"]], [x.tolist()[:6] for x in result["links"]])
    assert not D.claim_problems(case, list(zip(k1.tolist(), k2.tolist())), sn, dhet, dev), what
    return dev


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_push_equals_the_definition(case, wanted):
    h = _counter(case)
    try:
        for b in D.batches(case):
            h.push_host_batch(b)
        _same(h, case, wanted[case["name"]], case["name"])
        if case["capacity"] == 64:                                  # (the store grew where the case says it does)
            from tiddit_amd import tiddit_phase
            asks, grows, cap = tiddit_phase.device_timing(h)[1]
            assert asks >= 1 and grows >= 1 and cap > 64
    finally:
        h.close()
    PAIRS.append((case["name"], "push"))


@pytest.mark.parametrize("case", READER_OK, ids=[c["name"] for c in READER_OK])
def test_push_device_from_a_small_bam_equals_the_definition(case, wanted, tmp_path):
    from tiddit_amd import bamio
    path = str(tmp_path / "case.bam")
    w = bamio.BamWriter(path, list(zip(D.NAMES, case["lengths"])))
    w._buf += D.build(case, padding=False).raw.tobytes()          # the case's records as they are
    w.close()
    rd = bamio.DeviceBamReader(path)
    h = None
    try:
        h = _counter(case, ctx=rd.ctx)
        n = 0
        for b in rd.batches():
            h.push_device_batch(b)
            n += len(b)
        assert n == len(case["reads"])
        _same(h, case, wanted[case["name"]], case["name"])
    finally:
        if h is not None:
            h.close()
        rd.close()
    PAIRS.append((case["name"], "push_device"))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert len(D.CASES) == D.N_CASES == 39 and len(READER_OK) == 33
    assert len(set(PAIRS)) == 39 + 33, len(set(PAIRS))


# ---- the graph stage ----------------------------------------------------------------------------------------------------------
def _forest_host(g):
    from tiddit_amd import _native
    ctx, P = _native.default_context(), _native.ptr
    ns, nl = g["n_sites"], len(g["j"])
    outs = [np.full(ns + 2 * PAD, -7, dtype=np.int32), np.full(ns + 2 * PAD, 0x5a, dtype=np.uint8), np.full(nl + 2 * PAD, 0x5a, dtype=np.uint8),
            np.full(ns + 2 * PAD, 0x5a5a5a5a, dtype=np.uint32), np.full(ns + 2 * PAD, 0x5a5a5a5a, dtype=np.uint32)]
    inner = [o[PAD:] for o in outs]
    _native.check(ctx.lib.tdt_phase_forest(ctx.handle, P(g["j"]), P(g["i"]), P(g["n"]), P(g["trans"]), nl, ns, g["S"], *[P(o) for o in inner]))
    for o, n in zip(outs, (ns, ns, nl, ns, ns)):
        assert (o[:PAD] == o[0]).all() and (o[PAD + n:] == o[0]).all() and o[0] in (-7, 0x5a, 0x5a5a5a5a)
    return [o[PAD:PAD + n].copy() for o, n in zip(outs, (ns, ns, nl, ns, ns))]


def _forest_device(g):
    import torch
    from tiddit_amd import _native
    ctx = _native.default_context()
    ns, nl = g["n_sites"], len(g["j"])
    ins = [torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda() for a in (g["j"], g["i"], g["n"], g["trans"])]
    outs = [torch.full((n + 2 * PAD,), p, dtype=dt, device="cuda") for n, p, dt in ((ns, -7, torch.int32), (ns, 0x5a, torch.uint8), (nl, 0x5a, torch.uint8),
                                                                                    (ns, -7, torch.int32), (ns, -7, torch.int32))]
    torch.cuda.synchronize()
    _native.check(ctx.lib.tdt_phase_forest_device(ctx.handle, *[t.data_ptr() for t in ins], nl, ns, g["S"], *[o.data_ptr() + PAD * o.element_size() for o in outs]))
    got = []
    for o, n in zip(outs, (ns, ns, nl, ns, ns)):
        h = o.cpu().numpy()
        assert (h[:PAD] == h[0]).all() and (h[PAD + n:] == h[0]).all() and h[0] in (-7, 0x5a)
        got.append(h[PAD:PAD + n].copy())
    return got[:3] + [got[3].view(np.uint32), got[4].view(np.uint32)]


@pytest.fixture(scope="module")
def forests():
    from tiddit_amd import tiddit_phase
    return {g["name"]: tiddit_phase.forest(g["n_sites"], g["j"], g["i"], g["n"], g["trans"], g["S"]) for g in D.GRAPHS}


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("graph", D.GRAPHS, ids=[g["name"] for g in D.GRAPHS])
def test_forest_entries_equal_the_definition(graph, entry, forests):
    want = forests[graph["name"]]
    got = (_forest_host if entry == "host" else _forest_device)(graph)
    for name, x in zip(("root", "phase", "edge_used", "agree", "conflict"), got):
        assert x.dtype == want[name].dtype and np.array_equal(x, want[name]), (graph["name"], name, x[:12].tolist(), want[name][:12].tolist())
    assert int(got[3].sum()) == want["sn"]["agree"] and int(got[4].sum()) == want["sn"]["conflict"]
    assert not D.graph_problems(graph, dict(want, root=got[0], phase=got[1], edge_used=got[2]))


def test_forest_refusals_leave_the_outputs_untouched():
    from tiddit_amd import _native
    ctx, P = _native.default_context(), _native.ptr
    j, i = np.array([1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    n, t = np.array([3, 3], dtype=np.uint32), np.array([0, 3], dtype=np.uint32)
    outs = [np.full(3, -7, dtype=np.int32), np.full(3, 7, dtype=np.uint8), np.full(2, 7, dtype=np.uint8), np.full(3, 7, dtype=np.uint32), np.full(3, 7, dtype=np.uint32)]

    def call(j_=j, i_=i, n_=n, t_=t, nl=2, ns=3, S=2, ctx_=ctx.handle, outs_=outs):
        return ctx.lib.tdt_phase_forest(ctx_, P(j_), P(i_), P(n_), P(t_), nl, ns, S, *[P(o) if o is not None else None for o in outs_])
    assert call(ctx_=None) == -1 and call(j_=None) == -1 and call(outs_=[None] + outs[1:]) == -1
    assert call(S=0) == -3 and call(S=1 << 31) == -3 and call(ns=1 << 31) == -3 and call(nl=1 << 31) == -3
    assert call(j_=np.array([1, 3], dtype=np.int32)) == -1                       # an end outside [0, 3)
    assert call(j_=np.array([1, -1], dtype=np.int32)) == -1
    assert call(j_=np.array([0, 2], dtype=np.int32)) == -1                       # two equal ends
    assert call(t_=np.array([0, 4], dtype=np.uint32)) == -1                      # TRANS > N
    assert all((o == o[0]).all() and o[0] in (-7, 7) for o in outs)
    assert call() == 0 and outs[0].tolist() == [0, 0, 0] and outs[1].tolist() == [0, 0, 1] and outs[2].tolist() == [1, 1]
    assert call(nl=0, ns=0) == 0


# ---- the handle ---------------------------------------------------------------------------------------------------------------
def _case(name):
    return next(c for c in D.CASES if c["name"] == name)


def test_refusals_of_the_phase_entries():
    from tiddit_amd import _native, tiddit_phase
    case = _case("thresholds equal w decided by row")
    s, codes = D.sites_of(case)
    plain = _counter(case, phase=False)
    lib, P = plain.ctx.lib, _native.ptr
    try:
        got = np.full(len(tiddit_phase.PUSH) + len(tiddit_phase.FINISH) + 1, 7, dtype=np.uint64)
        het = np.ones(len(codes), dtype=np.uint8)
        n = ctypes.c_size_t(77)
        assert lib.tdt_alleles_phase_finish(plain.handle, P(het), 2, P(got)) == -1 and (got == 7).all()          # finish without enable
        assert lib.tdt_alleles_phase_keys(plain.handle, None, None, ctypes.byref(n)) == -1 and n.value == 77
        assert lib.tdt_alleles_phase_sites(plain.handle, None, None, 0) == -1
        assert lib.tdt_alleles_phase_enable(None, P(codes), len(codes), 64, 64) == -1
        assert lib.tdt_alleles_phase_enable(plain.handle, P(codes), len(codes), 64, 0) == -3                      # hash_bits 0 and 65
        assert lib.tdt_alleles_phase_enable(plain.handle, P(codes), len(codes), 64, 65) == -3
        assert lib.tdt_alleles_phase_enable(plain.handle, P(codes), len(codes) + 1, 64, 64) == -1                 # n_sites mismatch
        assert lib.tdt_alleles_phase_enable(plain.handle, P(codes), len(codes) - 1, 64, 64) == -1
        assert lib.tdt_alleles_phase_enable(plain.handle, None, len(codes), 64, 64) == -1
        bad = codes.copy()
        bad[0] = 0                                                                                                # REF == ALT
        assert lib.tdt_alleles_phase_enable(plain.handle, P(bad), len(codes), 64, 64) == -1
        assert lib.tdt_alleles_phase_enable(plain.handle, P(codes), len(codes), 64, 64) == 0
        assert lib.tdt_alleles_phase_enable(plain.handle, P(codes), len(codes), 64, 64) == -1                     # enable twice
        assert lib.tdt_alleles_phase_finish(plain.handle, None, 2, P(got)) == -1 and lib.tdt_alleles_phase_finish(plain.handle, P(het), 2, None) == -1
        assert lib.tdt_alleles_phase_finish(plain.handle, P(het), 0, P(got)) == -3 and (got == 7).all()
        root, phase = np.full(len(codes), -7, dtype=np.int32), np.full(len(codes), 7, dtype=np.uint8)
        assert lib.tdt_alleles_phase_sites(plain.handle, P(root), P(phase), len(codes)) == -1 and (root == -7).all()      # no finish yet
        assert lib.tdt_alleles_phase_finish(plain.handle, P(het), 2, P(got)) == 0 and not got.any()
        assert lib.tdt_alleles_phase_sites(plain.handle, P(root), P(phase), len(codes) - 1) == -1
        assert lib.tdt_alleles_phase_sites(plain.handle, P(root), P(phase), len(codes)) == 0 and (root == -1).all() and not phase.any()
        assert lib.tdt_alleles_phase_timing(plain.handle, None) == -1 and lib.tdt_alleles_phase_reserve_stats(plain.handle, None) == -1
    finally:
        plain.close()
    pushed = _counter(case, phase=False)
    try:
        pushed.push_host_batch(D.build(case))
        assert lib.tdt_alleles_phase_enable(pushed.handle, P(codes), len(codes), 64, 64) == -1                    # enable behind a push
        pushed.reset()
        assert lib.tdt_alleles_phase_enable(pushed.handle, P(codes), len(codes), 64, 64) == 0
    finally:
        pushed.close()


def test_reset_and_a_second_job_on_one_handle_and_small_room(wanted):
    from tiddit_amd import _native, tiddit_phase
    case, second = _case("thresholds equal w decided by row"), _case("thresholds TRANS wins")
    h = _counter(case)
    lib, P = h.ctx.lib, _native.ptr
    try:
        h.push_host_batch(D.build(case))
        dev = _same(h, case, wanted[case["name"]], "the first job")
        assert D.same_result(dev, _same(h, case, wanted[case["name"]], "the finish again"))
        n = ctypes.c_size_t(2)                                      # room for 2 of the 3 links: refused, nothing written
        cols = [np.full(4, 7, dtype=np.uint32) for _ in range(4)] + [np.full(4, 7, dtype=np.uint8)]
        assert lib.tdt_alleles_phase_links(h.handle, *[P(c) for c in cols], ctypes.byref(n)) == -3 and n.value == 2 and all((c == 7).all() for c in cols)
        n = ctypes.c_size_t(0)
        b = [np.full(2, 7, dtype=np.int32) for _ in range(2)] + [np.full(2, 7, dtype=np.uint32) for _ in range(4)]
        assert lib.tdt_alleles_phase_blocks(h.handle, *[P(c) for c in b], ctypes.byref(n)) == -3 and all((c == 7).all() for c in b)
        h.push_host_batch(D.build(second))                          # a push since the finish: the read-outs are refused
        assert lib.tdt_alleles_phase_links(h.handle, None, None, None, None, None, ctypes.byref(n)) == -1
        h.reset()
        counts, used, bad = h.counts()
        assert not counts.any() and used == 0 and len(tiddit_phase.device_keys(h)[0]) == 0
        h.phase = h.phase[:3] + (second["S"], second["H"])
        h.push_host_batch(D.build(second))
        _same(h, second, wanted[second["name"]], "the second job")
    finally:
        h.close()


def test_a_counter_without_phase_gives_the_counters_it_gives_today(wanted):
    for name in ("fragments a fragment of 16 rows", "malformed op code 9", "state two pushes, the store grown from 64 keys"):
        case = _case(name)
        with_, without = _counter(case), _counter(case, phase=False)
        try:
            for b in D.batches(case):
                with_.push_host_batch(b)
                without.push_host_batch(b)
            a, b = with_.counts(), without.counts()
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and np.array_equal(b[0], wanted[name][2])
        finally:
            with_.close()
            without.close()


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------
CONTIGS = (("chrA", 14000), ("chrB", 6000))
READ, INSERT, STEP = 60, 250, 6
GAP = (5000, 5600)                              # no het site in [5000, 5600) of chrA: longer than any fragment
OVERLAP = (1000, 1600)                          # chrB: further fragments of 100 bases start here, their mates overlap by 20
HOM_ALT, THIRD = ("chrA", 8003), ("chrB", 4003)


def _sample():
    """-> (genomes, sites rows [(contig, pos0, ref, alt, planted allele of haplotype 0 or None)], reads)"""
    rng = np.random.RandomState(77)
    genomes, rows, reads = {}, [], []
    for c, (name, ln) in enumerate(CONTIGS):
        g = seeded(ln, 100 + c)
        genomes[name] = g
        pos = 200
        while pos < ln - 200:
            if not (c == 0 and GAP[0] - 1 <= pos < GAP[1]):
                rows.append((name, pos, g[pos], other(g[pos]), int(rng.randint(0, 2))))
            pos += 70 + int(rng.randint(0, 21))
        for special in (HOM_ALT, THIRD):
            if special[0] == name:
                rows.append((name, special[1], g[special[1]], other(g[special[1]]), None))
    rows.sort(key=lambda r: (r[0], r[1]))
    n = 0
    for c, (name, ln) in enumerate(CONTIGS):
        mine = [r for r in rows if r[0] == name]
        haps = []
        for hap in (0, 1):
            s = list(genomes[name])
            for _, p, ref, alt, planted in mine:
                if planted is not None:
                    s[p] = alt if planted ^ hap else ref             # haplotype 0 carries allele `planted`, haplotype 1 the other
                elif (name, p) == HOM_ALT:
                    s[p] = alt
                elif hap:
                    s[p] = other(alt) if other(alt) != ref else other(other(alt))      # a third base on one haplotype
            haps.append("".join(s))
        for start in range(0, ln - INSERT, STEP):
            hap = (start // STEP) % 2
            for ins in (INSERT, 100) if c == 1 and OVERLAP[0] <= start < OVERLAP[1] else (INSERT,):
                for k, p in enumerate((start, start + ins - READ)):
                    reads.append(D.R(c, p, "%dM" % READ, haps[hap][p:p + READ], name="p%d" % n, flag=0x1 | (0x40 if k == 0 else 0x80)))
                n += 1
    reads.sort(key=lambda r: (r["tid"], r["pos"]))
    return genomes, rows, reads


def write_sample(d):
    from tiddit_amd import bamio
    genomes, rows, reads = _sample()
    fa, bam, vcf = os.path.join(d, "ref.fa"), os.path.join(d, "sample.bam"), os.path.join(d, "sites.vcf")
    open(fa, "wb").write(b"".join(b">" + n.encode() + b"\n" + fasta_raw(genomes[n]) + b"\n" for n, _ in CONTIGS))
    w = bamio.BamWriter(bam, list(CONTIGS))
    w._buf += D.build_reads(reads, padding=False).raw.tobytes()
    w.close()
    open(vcf, "w").write("##fileformat=VCFv4.2\n" + "".join("%s\t%d\t.\t%s\t%s\n" % (c, p + 1, ref, alt) for c, p, ref, alt, _ in rows))
    return bam, fa, vcf, rows


def _job(bam, fa, out, timeout=300, **env):
    e = {k: v for k, v in os.environ.items() if not (k.startswith("TIDDIT_") and k != "TIDDIT_HIP_LIB") and k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env)
    argv = [sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly"]
    return subprocess.run(argv, cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)


def _ok(r):
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


def _files(prefix):
    d, base = os.path.split(prefix)
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            rel = os.path.relpath(p, d)
            if rel.startswith(base + ".") or rel.startswith(base + "_tiddit"):
                data = open(p, "rb").read()
                if p.endswith(".vcf"):                                        # (its ##TIDDITcmd= line names the job's own prefix)
                    data = b"\n".join(l for l in data.split(b"\n") if not l.startswith(b"##TIDDITcmd="))
                out[rel[len(base):]] = hashlib.sha256(data).hexdigest()
    return out


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """(each job is checked before the next one is started: a crash, a time-out or a GPU error ends the fixture there)"""
    d = str(tmp_path_factory.mktemp("phase"))
    bam, fa, vcf, rows = write_sample(d)
    paths = {n: os.path.join(d, n) for n in ("off", "on", "host", "ranks", "bad", "alone")}
    _ok(_job(bam, fa, paths["off"], TIDDIT_ALLELES=vcf))
    r = _ok(_job(bam, fa, paths["on"], TIDDIT_ALLELES=vcf, TIDDIT_PHASE="2"))
    _ok(_job(bam, fa, paths["host"], TIDDIT_ALLELES=vcf, TIDDIT_PHASE="2", TIDDIT_HOST_INGEST="1"))
    return bam, fa, vcf, rows, paths, r


def definitions_files(bam, vcf, min_link=2, min_allele=3, min_q=5, min_bq=13):
    """the definition over the host reader's batches, through the module's own text writer -> (phase.tab, blocks.tab, sn, result, sites, het)"""
    from tiddit_amd import bamio, tiddit_alleles, tiddit_phase
    rd = bamio.BamReader(bam)
    names = list(rd.references)
    sites = tiddit_alleles.read_sites(vcf, names, list(rd.lengths))
    codes = tiddit_phase.site_codes(sites)
    keys, push = [], tiddit_phase.new_counters()
    table, stats = np.zeros((len(sites), 8), dtype=np.uint32), [0, 0]
    for b in rd.batches():
        tiddit_phase.keys_of_batch(keys, push, codes, 64, sites.site_pos, sites.site_off, b, min_q, min_bq)
        tiddit_alleles.count_batch(table, stats, sites.site_pos, sites.site_off, b, min_q, min_bq)
    rd.close()
    het, ref_n, alt_n = tiddit_phase.het_flags(table, codes, min_allele)
    result = tiddit_phase.summarise(keys, het, sites.site_off, min_link)
    text, blocks, sn = tiddit_phase.file_text(sites, codes, het, ref_n, alt_n, result, push, names, min_link, min_allele, min_bq)
    return text, blocks, sn, result, sites, het


def test_the_files_equal_the_definitions_and_the_phases_are_the_planted_haplotypes(jobs):
    from tiddit_amd import tiddit_phase
    bam, fa, vcf, rows, paths, r = jobs
    text, blocks, sn, result, sites, het = definitions_files(bam, vcf)
    got, got_blocks = open(paths["on"] + ".phase.tab").read(), open(paths["on"] + ".phase.blocks.tab").read()
    assert len(got) > 2000 and got == text and got_blocks == blocks
    assert got.startswith("# tiddit_amd phase v1 min_link=2 min_allele=3 min_bq=13 hash=fnv1a64\nSN\tmalformed\t0\n")
    assert [l for l in r.stdout.split("\n") if l.startswith("phase:")] == [tiddit_phase.summary_line(sn)]
    planted = {(c, p + 1): a for c, p, _, _, a in rows}
    lines = [l.split("\t") for l in got.split("\n") if l and not l.startswith(("#", "SN"))]
    n_het = sum(a is not None for a in planted.values())
    assert len(lines) == n_het == sn["het_sites"] and sn["phaseable_sites"] == len(rows)         # the hom-alt and the third-allele site are no hets
    assert not any((l[0], int(l[1])) in ((HOM_ALT[0], HOM_ALT[1] + 1), (THIRD[0], THIRD[1] + 1)) for l in lines)
    by_ps = {}
    for l in lines:
        assert l[6] in ("0|1", "1|0") and l[7] != "."                                             # every het is phased: fragments reach the next het
        by_ps.setdefault((l[0], l[7]), []).append(int(l[6] == "1|0") ^ planted[(l[0], int(l[1]))])
    assert all(len(set(v)) == 1 and len(v) >= 2 for v in by_ps.values())                          # each block: the planted haplotype or its complement
    # the het-free stretch splits chrA into two blocks; chrB is one
    b = [l.split("\t") for l in got_blocks.split("\n")[1:] if l]
    assert [x[0] for x in b] == ["chrA", "chrA", "chrB"] and int(b[0][2]) <= GAP[0] and int(b[1][1]) > GAP[1]
    assert sum(int(x[3]) for x in b) == n_het and sn["conflict"] == 0 and sn["blocks"] == 3 and sn["discordant_rows"] == 0
    assert sn["fragment_rows"] < sn["observations"]                                               # the overlapping mates agree: one row, two observations


def test_host_ingest_writes_the_same_bytes(jobs):
    bam, fa, vcf, rows, paths, r = jobs
    for ext in (".phase.tab", ".phase.blocks.tab"):
        assert open(paths["host"] + ext, "rb").read() == open(paths["on"] + ext, "rb").read()


def test_every_other_output_is_what_the_alleles_job_writes(jobs):
    bam, fa, vcf, rows, paths, r = jobs
    off, on, host = (_files(paths[k]) for k in ("off", "on", "host"))
    assert set(on) - set(off) == {".phase.tab", ".phase.blocks.tab"} and set(off) <= set(on) and len(off) >= 5 and ".alleles.tab" in off
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert set(host) == set(on)


def test_the_three_refusals_of_the_switch(jobs):
    bam, fa, vcf, rows, paths, r = jobs
    alone = _job(bam, fa, paths["alone"], timeout=120, TIDDIT_PHASE="2")
    assert alone.returncode == 1
    assert [l for l in alone.stdout.split("\n") if l.startswith("error")] == ["error, TIDDIT_PHASE=2: the sites are those of TIDDIT_ALLELES=sites.vcf: TIDDIT_ALLELES not set"]
    bad = _job(bam, fa, paths["bad"], timeout=120, TIDDIT_ALLELES=vcf, TIDDIT_PHASE="2:0")
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == ["error, TIDDIT_PHASE=2:0: the minimum number of reads per allele is an integer 1 ... 10^6"]
    res = _job(bam, fa, paths["ranks"], timeout=120, TIDDIT_ALLELES=vcf, TIDDIT_PHASE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29548",
               TIDDIT_DIST_BACKEND="gloo", TIDDIT_FORCE_DIST="1")
    assert res.returncode == 1, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_PHASE is a one-process switch")
    for k in ("alone", "bad", "ranks"):
        assert not os.path.exists(paths[k] + "_tiddit") and not os.path.exists(paths[k] + ".phase.tab")
