"""GPU tests of the GC kernels (csrc/tdt_gc.hip: gc_small_bins, gc_fasta_bins, gc_large_bins) on the aimed cases of
tests/gc_stage_cases.py, against its references (pinned on the CPU by test_gc_stage_refs_cpu.py).  Every one of the 822 cases goes
through the host entry (tdt_gc_bins by way of tiddit_gc.binned_gc_array, or tdt_gc_bins_fasta) AND through the device entry
(tdt_gc_bins_device / tdt_gc_bins_fasta_device) on torch-owned memory with a poisoned, padded output; then the contigs of every layout
in one tdt_gc_bins_fasta_many call and through tiddit_gc.binned_gc / gc_of_contigs from a file, the argument refusals, and the grid
strides of gc_large_bins and gc_small_bins (the latter needs 4.3 GB of sequence, built and checked on the device; the same loop of
gc_fasta_bins is NOT reached by any test: 256 tiles per compute unit are more bases than the entry's 2^31 limit on this device).  Every comparison is np.array_equal on int8.
Run on the MI355X box: python -m pytest tests/test_gpu_gc_stages.py -m gpu"""
import time

import numpy as np
import pytest

import gc_stage_cases as gc

pytestmark = pytest.mark.gpu

RAN = set()
POISON, PAD = 0x55, 64


@pytest.fixture(scope="module")
def nat():
    from tiddit_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def ctx(nat):
    return nat.default_context(0)


@pytest.fixture(scope="module")
def gcmod(ctx):
    from tiddit_amd import tiddit_gc
    return tiddit_gc


@pytest.fixture(scope="module")
def num_cu(ctx):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def on_device(a):
    """a host uint8 array in torch-owned device memory of exactly its size, 16-byte aligned"""
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.uint8)).to("cuda:0") if len(a) else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def poisoned(nbins):
    import torch
    return torch.full((nbins + PAD,), POISON, dtype=torch.int8, device="cuda:0")


def device_result(ctx, out, nbins, where):
    """after a device entry: wait, the bins, and the pad behind them untouched"""
    ctx.sync()
    host = out.cpu().numpy()
    assert host.dtype == np.int8
    assert (host[nbins:] == POISON).all(), (where, "wrote past nbins")
    return host[:nbins]


def same(got, want, where):
    assert got.dtype == np.int8 and want.dtype == np.int8 and len(got) == len(want), where
    bad = np.flatnonzero(got != want)
    assert not len(bad), (where, "first differing bin %d: got %d, want %d; %d differ" % (bad[0], got[bad[0]], want[bad[0]], len(bad)))
    assert np.array_equal(got, want), where


def run_host(nat, ctx, gcmod, c):
    if c["kind"] == "seq":
        return gcmod.binned_gc_array(c["seq"], c["bin"], c["cut"], ctx)
    out = np.full(-(-c["len"] // c["bin"]), POISON, dtype=np.int8)
    nat.check(ctx.lib.tdt_gc_bins_fasta(ctx.handle, nat.ptr(c["raw"]), c["nbytes"], c["len"], c["lb"], c["lw"], c["bin"], c["cut"], nat.ptr(out)))
    return out


def run_device(nat, ctx, c):
    import torch
    nbins = -(-c["len"] // c["bin"])
    d_in, out = on_device(c["seq"] if c["kind"] == "seq" else c["raw"]), poisoned(nbins)
    torch.cuda.synchronize()
    if c["kind"] == "seq":
        nat.check(ctx.lib.tdt_gc_bins_device(ctx.handle, d_in.data_ptr(), c["len"], c["bin"], c["cut"], out.data_ptr()))
    else:
        nat.check(ctx.lib.tdt_gc_bins_fasta_device(ctx.handle, d_in.data_ptr(), c["nbytes"], c["len"], c["lb"], c["lw"], c["bin"], c["cut"],
                                                   out.data_ptr()))
    return device_result(ctx, out, nbins, c["name"])


@pytest.mark.parametrize("name", gc.case_names())
def test_case_through_host_and_device_entries(nat, ctx, gcmod, num_cu, name):
    c = gc.get(name, num_cu)
    want = gc.expected(c)
    if name == "large_grid_stride":
        assert len(want) == gc.LARGE_BINS_PER_CU * num_cu + 37
    same(run_host(nat, ctx, gcmod, c), want, (name, "host"))
    same(run_device(nat, ctx, c), want, (name, "device"))
    if c["family"] == "trail":                                     # the bytes behind the contig change nothing
        short = dict(c, raw=c["raw"][:c["nbytes"] - len(gc.TRAILING)].copy(), nbytes=c["nbytes"] - len(gc.TRAILING))
        same(run_host(nat, ctx, gcmod, short), want, (name, "host, without the trailing bytes"))
        same(run_device(nat, ctx, short), want, (name, "device, without the trailing bytes"))
    RAN.add(name)


def test_every_case_was_run():
    """(after the parametrised test above, in file order) nothing was skipped or deselected: the count is a condition"""
    assert len(RAN) == gc.N_CASES == 822, len(RAN)


def test_alphabet_against_the_table_itself(ctx, gcmod):
    """the three byte-table cases against what each byte must give by definition, without any reference in between"""
    for name in ("alpha_each_byte", "alpha_every_position", "alpha_pairs"):
        c = gc.get(name)
        same(gcmod.binned_gc_array(c["seq"], 1, 0.5, ctx), gc.alphabet_expected(c["seq"]), name)


# ================================================================================================== many contigs, and from a file
@pytest.mark.parametrize("bin_size", [7, 50, 64, 2048])
def test_many_contigs_in_one_call(nat, ctx, bin_size):
    g = gc.many_group(bin_size)
    out = np.full(g["out_bytes"] + PAD, POISON, dtype=np.int8)
    nat.check(ctx.lib.tdt_gc_bins_fasta_many(ctx.handle, nat.ptr(g["raw"]), len(g["raw"]), len(g["contigs"]), nat.ptr(g["raw_off"]),
                                             nat.ptr(g["raw_len"]), nat.ptr(g["len"]), nat.ptr(g["lb"]), nat.ptr(g["lw"]), bin_size, 0.5,
                                             nat.ptr(out), nat.ptr(g["out_off"]), g["out_bytes"]))
    assert (out[g["out_bytes"]:] == POISON).all()
    for i, c in enumerate(g["contigs"]):                           # packed: contig i's bins start where contig i-1's end
        want = gc.gc_literal(c["seq"], bin_size, 0.5)
        same(out[g["out_off"][i]:g["out_off"][i] + len(want)], want, (bin_size, i, c["lb"], c["lw"], c["len"]))


def test_contigs_of_every_layout_from_a_file(ctx, gcmod, tmp_path, monkeypatch):
    """tiddit_gc.binned_gc and gc_of_contigs (tiddit_gc.pyx:6-42) on a file whose contigs are wrapped at every line length of the table"""
    from tiddit_amd.fasta import FastaFile
    g = gc.many_group(50)
    path = str(tmp_path / "layouts.fa")
    with open(path, "wb") as f:
        for i, c in enumerate(g["contigs"]):
            eol = b"\r\n" if c["lw"] == c["lb"] + 2 else b"\n"
            f.write(b">c%d some text" % i + eol + c["raw"].tobytes() + (eol if c["len"] else b""))
    fa = FastaFile(path)
    names = ["c%d" % i for i in range(len(g["contigs"]))]
    want = {n: gc.gc_literal(c["seq"], 50, 0.5) for n, c in zip(names, g["contigs"])}
    for n in names[::5]:
        r = gcmod.binned_gc(fa, n, 50, 0.5, ctx=ctx)
        assert r[0] == n
        same(r[1], want[n], ("binned_gc", n))
    monkeypatch.setattr(gcmod, "_MANY_MAX_BATCH", 200_000)         # several groups, and the tile-crossing contigs on their own
    monkeypatch.setattr(gcmod, "_MANY_MAX_CONTIG", 60_000)
    got = gcmod.gc_of_contigs(fa, names[::-1], 50, 0.5, ctx=ctx)
    assert list(got) == names[::-1]
    for n in names:
        same(got[n], want[n], ("gc_of_contigs", n))


# ================================================================================================== refusals
def test_argument_refusals_launch_nothing(nat, ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    c = gc.get("fasta_line60_lf_bin50_len179")
    d_raw, d_seq = on_device(c["raw"]), on_device(gc.stripped(c))
    nbins = -(-c["len"] // 50)
    out = poisoned(nbins)
    torch.cuda.synchronize()
    P, R, O = d_seq.data_ptr(), d_raw.data_ptr(), out.data_ptr()

    def refused(rc, code, function):
        assert rc == code, (function, rc)
        assert lib.tdt_last_error().decode().startswith(function + ":"), lib.tdt_last_error()

    refused(lib.tdt_gc_bins_device(h, P + 1, c["len"] - 1, 50, 0.5, O), gc.TDT_E_ARG, "tdt_gc_bins_device")
    fasta = lambda raw, nbytes, ln, lb, lw, z: lib.tdt_gc_bins_fasta_device(h, raw, nbytes, ln, lb, lw, z, 0.5, O)
    refused(fasta(R + 1, c["nbytes"] - 1, c["len"] - 1, 60, 61, 50), gc.TDT_E_UNSUPPORTED, "tdt_gc_bins_fasta_device")
    refused(fasta(R, c["nbytes"], c["len"], 60, 61, 2049), gc.TDT_E_UNSUPPORTED, "tdt_gc_bins_fasta_device")
    refused(fasta(R, c["nbytes"], c["len"], 60, 63, 50), gc.TDT_E_UNSUPPORTED, "tdt_gc_bins_fasta_device")
    refused(fasta(R, c["nbytes"], 1 << 31, 60, 61, 50), gc.TDT_E_UNSUPPORTED, "tdt_gc_bins_fasta_device")
    refused(fasta(R, c["nbytes"] - 1, c["len"], 60, 61, 50), gc.TDT_E_ARG, "tdt_gc_bins_fasta_device")
    ctx.sync()
    assert (out.cpu().numpy() == POISON).all()                     # none of them wrote a bin

    g = gc.many_group(50)
    host_out = np.full(g["out_bytes"] + PAD, POISON, dtype=np.int8)

    def many(raw_off, out_off, out_bytes):
        return lib.tdt_gc_bins_fasta_many(h, nat.ptr(g["raw"]), len(g["raw"]), len(g["contigs"]), nat.ptr(raw_off), nat.ptr(g["raw_len"]),
                                          nat.ptr(g["len"]), nat.ptr(g["lb"]), nat.ptr(g["lw"]), 50, 0.5, nat.ptr(host_out), nat.ptr(out_off), out_bytes)
    off = g["raw_off"].copy()
    off[5] += 8
    refused(many(off, g["out_off"], g["out_bytes"]), gc.TDT_E_ARG, "tdt_gc_bins_fasta_many")
    refused(many(g["raw_off"], g["out_off"], g["out_bytes"] - 1), gc.TDT_E_ARG, "tdt_gc_bins_fasta_many")
    over = g["out_off"].copy()
    over[-1] += 1
    refused(many(g["raw_off"], over, g["out_bytes"]), gc.TDT_E_ARG, "tdt_gc_bins_fasta_many")
    assert (host_out == POISON).all()
    assert many(g["raw_off"], g["out_off"], g["out_bytes"]) == 0   # and the same arrays unaltered are taken


# ================================================================================================== the small-bin grid stride
def test_small_bin_grid_stride_on_a_sequence_built_on_the_device(nat, ctx, num_cu):
    """gc_small_bins walks more than one tile per workgroup only past 256 tiles per compute unit, 4.3 GB of sequence at 256 compute units:
    (256 * num_cu + 3) tiles of 64 KB and 17 bases, bin size 64.  Sequence, expected bins and comparison stay on the device."""
    import torch
    free = torch.cuda.mem_get_info(0)[0]
    if free < 16 << 30:
        pytest.skip("the small-bin grid stride needs 16 GB of free device memory; %.1f GB are free" % (free / 2 ** 30))
    z, cut = 64, 0.5
    assert gc.tile_bases(z) == 65536
    L = (gc.SMALL_TILES_PER_CU * num_cu + 3) * gc.tile_bases(z) + 17
    nbins = -(-L // z)
    t0 = time.time()
    lut = torch.tensor(list(b"ACGTacgtNnKkOo\xff\xe3\xc7\xee\x00AGgCc"), dtype=torch.uint8, device="cuda:0")
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(20240917)
    seq = torch.empty(L, dtype=torch.uint8, device="cuda:0")
    step = 1 << 26
    for a in range(0, L, step):
        n = min(step, L - a)
        seq[a:a + n] = lut[torch.randint(0, len(lut), (n,), generator=gen, device="cuda:0")]
        seq[a + 777:a + 777 + 4099] = 0x4e                         # a run of N across tile and bin edges: masked bins, and bins half in it
    seq[-17:] = torch.tensor(list(b"GGGGGGGGGGGGGGGGN"), dtype=torch.uint8, device="cuda:0")     # the last bin: 16 of 17 -> 94
    out = poisoned(nbins)
    assert seq.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    t1 = time.time()
    nat.check(ctx.lib.tdt_gc_bins_device(ctx.handle, seq.data_ptr(), L, z, cut, out.data_ptr()))
    ctx.sync()
    t2 = time.time()
    assert bool((out[nbins:] == POISON).all()), "wrote past nbins"
    step = 1 << 28                                                 # a multiple of the bin size: slices of whole bins
    seen = torch.zeros(102, dtype=torch.int64, device="cuda:0")
    for a in range(0, L, step):
        want = gc.gc_counts_torch(seq[a:a + step], z, cut)
        got = out[a // z:a // z + len(want)]
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want)[:, 0]
            raise AssertionError("bin %d: got %d, want %d; %d differ in this slice" % (a // z + int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), len(bad)))
        seen += torch.bincount((want.to(torch.int64) + 1), minlength=102)
        del want, got
    assert int(out[nbins - 1]) == 94
    seen = seen.cpu().numpy()
    assert seen.sum() == nbins and np.count_nonzero(seen) > 30 and seen[0] >= 64 * (L >> 26)      # a spread of values, and the masked bins of every run of N
    print("small-bin grid stride: %d bases, %d bins; build %.2f s, kernel %.3f s, check %.2f s" % (L, nbins, t1 - t0, t2 - t1, time.time() - t2))
