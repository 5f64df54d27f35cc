"""CPU pin of tests/gc_stage_cases.py: the literal loop, the numpy counts, the torch restatement and the C oracle against each other on
every case; the FASTA helpers; that the tie cases are ties and round to the even neighbour; that the threshold cases flip where they
say; the tile rule; the reciprocal that maps a base to its FASTA line.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import gc_stage_cases as gc
import oracle


def test_the_case_set_is_the_one_the_gpu_file_states():
    fam = {f: len(gc.case_names(f)) for f in ("alpha", "sat", "tie", "thr", "word", "len", "large", "fasta", "trail")}
    assert fam == {"alpha": 17, "sat": 6, "tie": 125, "thr": 144, "word": 24, "len": 253, "large": 19, "fasta": 208, "trail": 26}, fam
    assert gc.N_CASES == sum(fam.values()) == 822


@pytest.mark.parametrize("family", ["alpha", "sat", "tie", "thr", "word", "len", "large", "fasta", "trail"])
def test_literal_equals_counts_equals_oracle(family):
    literal = 0
    for name in gc.case_names(family):
        c = gc.get(name)
        s = gc.stripped(c)
        assert len(s) == c["len"], name
        want = gc.gc_counts(s, c["bin"], c["cut"])
        assert want.dtype == np.int8 and len(want) == -(-c["len"] // c["bin"]), name
        assert np.array_equal(want, oracle.binned_gc(s, c["bin"], c["cut"])), name
        if c["ref"] == "literal":
            assert np.array_equal(gc.gc_literal(s, c["bin"], c["cut"]), want), name
            literal += 1
        else:
            assert c["len"] > gc.LITERAL_MAX, name
    assert literal >= 1 and (literal == len(gc.case_names(family)) or family == "large"), family


def test_torch_restatement_equals_counts():
    import torch
    for name in ("alpha_pairs", "tie_full_bin64", "tie_full_bin4096", "thr_bin64_cut_k_over_bin_below_short_at", "thr_bin50_cut_nan_short_at",
                 "thr_bin2_cut_0.5_short_at", "len_bin64_len65537", "len_bin50_len64017", "large_bin4099_len8225", "sat_bin16"):
        c = gc.get(name)
        got = gc.gc_counts_torch(torch.from_numpy(c["seq"]), c["bin"], c["cut"])
        assert got.dtype == torch.int8 and np.array_equal(got.numpy(), gc.gc_counts(c["seq"], c["bin"], c["cut"])), name
    s = gc.hostile(64 * 3000 + 17, 5)                              # in slices, as the device test takes it
    parts = [gc.gc_counts_torch(torch.from_numpy(s[a:a + 64 * 1024]), 64, 0.5) for a in range(0, len(s), 64 * 1024)]
    assert np.array_equal(torch.cat(parts).numpy(), gc.gc_counts(s, 64, 0.5))


def test_alphabet_is_exact_by_construction():
    each = gc.get("alpha_each_byte")
    want = gc.alphabet_expected(each["seq"])
    assert sorted(np.flatnonzero(want == 100)) == sorted(gc.GC_BYTES) and sorted(np.flatnonzero(want == -1)) == sorted(gc.N_BYTES)
    assert np.count_nonzero(want) == 6 and np.array_equal(gc.expected(each), want)
    pos = gc.get("alpha_every_position")
    seen = set(zip(pos["seq"].tolist(), (np.arange(len(pos["seq"])) % 16).tolist()))
    assert len(seen) == 256 * 16                                   # every byte value at every position of a 16-byte chunk
    assert np.array_equal(gc.expected(pos), gc.alphabet_expected(pos["seq"]))
    pairs = gc.get("alpha_pairs")
    s = pairs["seq"]
    for need in (0x03, 0x07, 0x0e, 0x23, 0x27, 0x2e, 0x4b, 0x6b, 0x4f, 0x6f, 0xc3, 0xe3, 0xc7, 0xe7, 0xce, 0xee, 0xff, 0x00, 0x7f, 0x80):
        assert need in gc.PAIR_SET, hex(need)
    at = {}
    for i in range(len(s) - 1):
        if i % 16 != 15:
            at.setdefault((int(s[i]), int(s[i + 1])), set()).add(i % 16)
    for a in gc.PAIR_SET:                                          # every ordered pair, at every one of the fifteen adjacencies of a chunk
        for b in gc.PAIR_SET:
            assert at[(a, b)] == set(range(15)), (a, b)
    assert np.array_equal(gc.expected(pairs), gc.alphabet_expected(s))
    for filler, out in (("A", 6), ("ff", 6), ("G", 100), ("N", -1)):   # one byte in sixteen: 1/16 -> 6, 15/16 -> 94, 16/16 -> 100
        c = gc.get("alpha_one_in_sixteen_%s_bin16" % filler)
        got = gc.expected(c).reshape(16, 256)
        assert (got[:, 0x41] == {"A": 0, "ff": 0, "G": 94, "N": -1}[filler]).all()
        assert (got[:, 0x47] == {"A": 6, "ff": 6, "G": 100, "N": -1}[filler]).all() and (got[:, 0x6e] == -1).all(), filler


def test_saturation_is_exact_by_construction():
    c = gc.get("sat_bin16")
    want = np.array([{0x47: 100, 0x4e: -1, 0xff: 0}[int(v)] for v in c["seq"][::16]], dtype=np.int8)
    assert len(want) == 3 + 81 and np.array_equal(gc.expected(c), want)


def test_ties_are_ties_and_go_to_the_even_neighbour():
    assert gc.tie_counts(50) == [] and gc.tie_counts(300) == []    # the reference's own bin size never ties on a full bin
    for chars in gc.TIE_SHORT + gc.TIE_FULL:
        assert gc.tie_counts(chars), chars
    seen, parities = set(), {}
    for name in gc.case_names("tie"):
        c = gc.get(name)
        want = gc.expected(c)
        for at, g, chars in c["meta"]["ties"]:
            lo, hi = at * c["bin"], min((at + 1) * c["bin"], c["len"])
            assert hi - lo == chars and np.isin(c["seq"][lo:hi], gc.GC_BYTES).sum() == g and not np.isin(c["seq"][lo:hi], gc.N_BYTES).any(), name
            exact = Fraction(100 * g, chars)
            assert exact.denominator == 2, (name, exact)
            even = [v for v in (math.floor(exact), math.ceil(exact)) if v % 2 == 0]
            assert len(even) == 1 and want[at] == even[0], (name, at, want[at])
            parities.setdefault((c["bin"], chars), set()).add(math.floor(exact) & 1)
            seen.add((c["bin"], chars))
            if c["name"].startswith("tie_full"):                   # the neighbours: one count either side is no tie
                for d in (-1, 1):
                    assert Fraction(100 * (g + d), chars).denominator != 2
                    assert want[at + d] == round(Fraction(100 * (g + d), chars)), (name, at, d)
    assert seen == {(50, c) for c in gc.TIE_SHORT} | {(c, c) for c in gc.TIE_FULL} | {(4096, 4096), (4099, 2048)}
    assert all(p == {0, 1} for p in parities.values()), parities   # a tie that stays and a tie that goes up, for every width


def test_threshold_cases_flip_between_n_min_minus_one_and_n_min():
    flips = 0
    for name in gc.case_names("thr"):
        c = gc.get(name)
        want, n_min, z = gc.expected(c), c["meta"]["n_min"], c["bin"]
        assert all(not (n / z > c["cut"]) for n in range(min(n_min, z + 1))) and (n_min > z or n_min / z > c["cut"]), name
        for at, n in c["meta"]["bins"]:
            lo, hi = at * z, min((at + 1) * z, c["len"])
            assert np.isin(c["seq"][lo:hi], gc.N_BYTES).sum() == n, (name, at)
            assert (want[at] == -1) == (n >= n_min), (name, at, n, n_min)
        counts = {n for _, n in c["meta"]["bins"]}
        flips += n_min - 1 in counts and n_min in counts
    assert flips >= 60
    for z in gc.THR_BINS:                                          # the kinds of cut-off: never, always, and one ulp to either side of k / bin
        mins = {cn: gc.n_min_of(z, cut) for cn, cut in gc.thr_cutoffs(z)}
        assert mins["inf"] == mins["nan"] == mins["1.5"] == mins["1"] == z + 1 and mins["neginf"] == mins["neg"] == 0 and mins["0"] == 1, (z, mins)
        k = max(1, z // 3)
        assert (mins["k_over_bin_below"], mins["k_over_bin"], mins["k_over_bin_above"]) == (k, k + 1, k + 1), (z, mins)
    short = gc.get("thr_bin2_cut_0.5_short_at")                    # one N alone in the last bin of a 2-base binning: 1/2 is not above 0.5
    assert short["len"] % 2 == 1 and short["seq"][-1] in gc.N_BYTES and gc.expected(short)[-1] == 0


def test_tile_rule_and_the_lengths_around_it():
    assert [gc.tile_bins(z) for z in (1, 50, 64, 255, 256, 257, 300, 2047, 2048)] == [65536, 1280, 1024, 256, 256, 240, 208, 32, 32]
    assert gc.tile_bins(4096) == 16 and gc.tile_bins(70000) == 16  # the floor (no bin size the small-bin kernel takes reaches it)
    odd = [z for z in gc.LEN_BINS if (gc.tile_bases(z) >> 4) & 1]  # tiles of an odd number of 16-byte chunks: the upper half of the last
    assert odd == [257], odd                                       # LDS word is zeroed there (reached; the bit ranges never read it)
    for z in gc.LEN_BINS:
        T = gc.tile_bases(z)
        assert T % 16 == 0 and T <= gc.TILE_TARGET
        assert {T + d for d in gc.AROUND} | {2 * T + d for d in gc.AROUND} | {1, z, z + 1} <= set(gc.len_lengths(z)), z
    for z in gc.LARGE_BINS:
        assert {L % 16 for L in gc.large_lengths(z)} >= {0, 1, 15} and {z - 1, z, z + 1} <= set(gc.large_lengths(z))
    c = gc.get("large_grid_stride", num_cu=8)
    assert -(-c["len"] // 2049) == 16 * 8 + 37


def test_fasta_helpers_round_trip():
    for lb, eol in gc.LAYOUTS:
        for L in (1, 2, 63, 64, 65, 127, 128, 129, 4097):
            n = {"len": L, "len+5": L + 5}.get(lb, lb)
            s = gc.hostile(L, L + 3)
            for trailing in (b"", gc.TRAILING):
                raw, ln, b, w = gc.wrap_fasta(s, n, eol, trailing)
                assert (ln, b, w) == (L, n, n + len(eol))
                assert gc.strip_fasta(raw, ln, b, w) == s.tobytes(), (lb, eol, L)
                body = raw.tobytes()[:len(raw) - len(trailing)]
                assert body.replace(b"\r", b"").replace(b"\n", b"") == s.tobytes() and not body.endswith(b"\n")
                nfull, tail = divmod(L, n)                          # the byte count the .fai arithmetic gives
                assert len(body) == nfull * w + tail - ((w - n) if tail == 0 else 0)
    g = gc.many_group(50)
    assert (g["raw_off"] % 16 == 0).all() and g["len"][3] == 0 and g["raw_len"][3] == 0
    assert (np.diff(g["raw_off"]) >= g["raw_len"][:-1]).all() and (np.diff(g["raw_off"]) > g["raw_len"][:-1]).sum() >= 20
    assert np.array_equal(np.diff(np.append(g["out_off"], g["out_bytes"])), -(-g["len"] // 50))
    for i, c in enumerate(g["contigs"]):
        o = g["raw_off"][i]
        assert gc.strip_fasta(g["raw"][o:o + g["raw_len"][i]], c["len"], c["lb"], c["lw"]) == c["seq"].tobytes()


def test_trailing_bytes_do_not_change_the_reference():
    for name in gc.case_names("trail"):
        c = gc.get(name)
        assert c["raw"].tobytes().endswith(gc.TRAILING) and np.array_equal(gc.stripped(c), c["meta"]["seq"])
        last = c["nbytes"] - len(gc.TRAILING)
        assert np.isin(c["raw"][last:(last + 15) // 16 * 16 + 16], gc.GC_BYTES + gc.N_BYTES).any(), name   # counted bytes right behind the contig


def test_line_of_a_base_by_reciprocal():
    """floor(b / linebases) == mulhi(b, magic) >> shift for every line length used, at line starts and ends up to 2^31 - 1"""
    used = {lb for lb, _ in gc.LAYOUTS if not isinstance(lb, str)}
    for z in gc.FASTA_BINS:
        for L in gc.fasta_lengths("len", z):
            used |= {L, L + 5}
    used |= {3, 5, 59, 63, 66, 70, 80, 127, 128, 129, 1 << 20, (1 << 20) + 1, (1 << 31) - 1}
    top = (1 << 31) - 1
    for lb in sorted(used):
        magic, shift = gc.fb_reciprocal(lb)
        assert 0 <= magic <= 0xffffffff and (shift >= 0 or lb == 1)
        ks = {1, 2, 3, 7, 255, 256, 65535, 65536, 1 << 20, top // lb - 1, top // lb}
        for b in {0, 1, top} | {k * lb - 1 for k in ks} | {k * lb for k in ks}:
            if 0 <= b <= top:
                assert gc.fb_line(b, lb) == b // lb, (lb, b)
