"""Aimed inputs and references for the GC kernels (csrc/tdt_gc.hip: gc_small_bins, gc_fasta_bins, gc_large_bins).  No GPU and no native
library here: tests/test_gc_stage_refs_cpu.py pins the references against each other and against the C oracle, and
tests/test_gpu_gc_stages.py runs every case through the entry points.

The operation (tiddit_gc.pyx:14-31) is exact: per bin, n = #{N,n}, gc = #{C,c,G,g}, chars = bytes in the bin;
out = -1 if n/bin_size > n_cutoff else round(100*gc/chars).  Two references that share no code:
  gc_literal   the reference's loop, line for line, over bytes (true division, Python's round): the reference of record, slow
  gc_counts    numpy: counts from cumulative sums, the same double division for the mask, half-even rounding in integers
and gc_counts_torch, the arithmetic of gc_counts on a torch tensor (for the one case that never leaves the device).

Families (case names start with the family):
  alpha   every byte value, at every position of a 16-byte chunk, beside every neighbour that could carry into it
  sat     chunks of sixteen G / N / 0xff: the extremes of the bit gather's sums
  tie     100*gc/chars exactly on a half, in both parities, with the gc-1 / gc+1 neighbours; full bins and short last bins
  thr     bins with n_min-1, n_min and bin_size N's for every kind of cut-off; the short last bin still divides by bin_size
  word    bases counted only on bit 0 and bit 31 of a 32-base word, and everywhere else
  len     every bin size class at lengths around one and two tile boundaries (the `whole` fast path against the last tile)
  large   bins above 2048: one workgroup per bin, unaligned bin starts and ends, the last chunk cut by len, its grid stride
  fasta   the FASTA layouts: line lengths around powers of two, CRLF, one base per line, a single line, tile crossings
  trail   the same with the next record's header ('>chrG_NNNN...') inside nbytes: masked by the bit range alone
"""
import math
from collections import OrderedDict

import numpy as np

GC_BYTES = (0x43, 0x63, 0x47, 0x67)       # C c G g
N_BYTES = (0x4e, 0x6e)                    # N n
LITERAL_MAX = 300_000                     # bases: above this the literal loop is too slow and gc_counts is the reference
TDT_E_ARG, TDT_E_UNSUPPORTED = -1, -6

# The tile rule of the small-bin and FASTA kernels as the library documents it (about 64 KB of sequence per workgroup of 256 lanes: whole
# multiples of 256 bins where 256 fit, otherwise a multiple of 16 bins, never fewer than 16), restated here as a constant of the tests.
THREADS = 256
SMALL_MAX = 2048
TILE_TARGET = 65536
LARGE_BINS_PER_CU = 16                    # gc_large_bins strides over the bins beyond 16 workgroups per compute unit ...
SMALL_TILES_PER_CU = 256                  # ... gc_small_bins over the tiles beyond 256 per compute unit


def tile_bins(bin_size):
    t = TILE_TARGET // bin_size
    t = t // THREADS * THREADS if t >= THREADS else t & ~15
    return max(t, 16)


def tile_bases(bin_size):
    return tile_bins(bin_size) * bin_size


# ================================================================================================== references
def gc_literal(seq, bin_size, n_cutoff):
    """tiddit_gc.pyx:14-31 over bytes"""
    seq = bytes(seq)
    contig_length = len(seq)
    number_of_bins = int(math.ceil(contig_length / bin_size))
    contig_gc = np.zeros(number_of_bins, dtype=np.int8)
    next_start = 0
    for bin in range(0, number_of_bins):
        slice = seq[next_start:next_start + bin_size]
        n = 0
        gc = 0
        number_of_chars = 0
        for character in slice:
            number_of_chars += 1
            if character == 0x4e or character == 0x6e:
                n += 1
            elif character == 0x43 or character == 0x63 or character == 0x47 or character == 0x67:
                gc += 1
        if n / bin_size > n_cutoff:
            contig_gc[bin] = -1
        else:
            contig_gc[bin] = round(100 * gc / number_of_chars)
        next_start += bin_size
    return contig_gc


def gc_counts(seq, bin_size, n_cutoff):
    s = np.frombuffer(bytes(seq), dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)
    nbins = -(-len(s) // bin_size)
    if nbins == 0:
        return np.zeros(0, dtype=np.int8)
    edges = np.minimum(np.arange(nbins + 1, dtype=np.int64) * bin_size, len(s))
    per_bin = []
    for members in (GC_BYTES, N_BYTES):
        cum = np.concatenate([[0], np.cumsum(np.isin(s, members), dtype=np.int64)])
        per_bin.append(cum[edges[1:]] - cum[edges[:-1]])
    g, n = per_bin
    chars = np.diff(edges)
    masked = n.astype(np.float64) / np.float64(bin_size) > np.float64(n_cutoff)
    num, den = 200 * g + chars, 2 * chars                          # round half up ...
    q = num // den
    q -= ((num % den == 0) & (q & 1 == 1)).astype(np.int64)        # ... and a tie that went up to an odd number goes back to the even one
    return np.where(masked, -1, q).astype(np.int8)


def gc_counts_torch(t, bin_size, n_cutoff):
    """gc_counts' arithmetic on a 1-D uint8 torch tensor (any device) -> int8 tensor on the same device"""
    import torch
    outs = []
    full = len(t) // bin_size
    for x, chars in ((t[:full * bin_size].view(full, bin_size), bin_size), (t[full * bin_size:].view(1, -1), len(t) - full * bin_size)):
        if x.numel() == 0:
            continue
        g = ((x == 0x43) | (x == 0x63) | (x == 0x47) | (x == 0x67)).sum(1, dtype=torch.int64)
        n = ((x == 0x4e) | (x == 0x6e)).sum(1, dtype=torch.int64)
        masked = n.to(torch.float64) / float(bin_size) > float(n_cutoff)
        num, den = 200 * g + chars, 2 * chars
        q = torch.div(num, den, rounding_mode="floor")
        q = q - ((num - q * den == 0) & (q % 2 == 1)).to(torch.int64)
        outs.append(torch.where(masked, torch.full_like(q, -1), q).to(torch.int8))
    return torch.cat(outs) if outs else torch.zeros(0, dtype=torch.int8, device=t.device)


def n_min_of(bin_size, n_cutoff):
    """the smallest N count that masks a bin; bin_size + 1 if none does"""
    for n in range(bin_size + 1):
        if n / bin_size > n_cutoff:
            return n
    return bin_size + 1


# ================================================================================================== FASTA layouts
def wrap_fasta(seq, linebases, eol, trailing=b""):
    """-> (raw uint8[], len, linebases, linewidth): `seq` in lines of `linebases` bases ended by `eol`; the contig's last line has no line
    end (its bytes stop at its last base, as the .fai arithmetic has it), `trailing` follows at once"""
    s = np.frombuffer(bytes(seq), dtype=np.uint8)
    lw = linebases + len(eol)
    nlines = -(-len(s) // linebases)
    grid = np.zeros((max(nlines, 1), lw), dtype=np.uint8)
    if len(eol):
        grid[:, linebases:] = np.frombuffer(eol, dtype=np.uint8)
    flat = grid.reshape(-1)
    b = np.arange(len(s), dtype=np.int64)
    flat[b // linebases * lw + b % linebases] = s
    need = (nlines - 1) * lw + (len(s) - (nlines - 1) * linebases) if len(s) else 0
    raw = np.concatenate([flat[:need], np.frombuffer(trailing, dtype=np.uint8)])
    return raw, len(s), linebases, lw


def strip_fasta(raw, length, linebases, linewidth):
    """the `length` bases of a contig laid out as wrap_fasta does, line by line"""
    raw = bytes(raw)
    lines = []
    got = at = 0
    while got < length:
        take = min(linebases, length - got)
        lines.append(raw[at:at + take])
        got += take
        at += linewidth
    return b"".join(lines)


def fb_reciprocal(linebases):
    """(magic, shift) with floor(b / linebases) == mulhi32(b, magic) >> shift for 0 <= b < 2^31; shift -1: linebases is 1 and the line is b.
    The round-up reciprocal the FASTA kernel is handed (tdt_gc.hip, tdt_gc_bins_fasta_device)."""
    if linebases <= 1:
        return 0, -1
    l = 0
    while (1 << l) < linebases:
        l += 1
    m = ((1 << (31 + l)) + linebases - 1) // linebases
    if m > 0xffffffff:
        raise OverflowError(linebases)
    return m, l - 1


def fb_line(b, linebases):
    magic, shift = fb_reciprocal(linebases)
    return b if shift < 0 else ((b * magic) >> 32) >> shift


# ================================================================================================== generators
_COUNTED = bytes(GC_BYTES + N_BYTES)
NEIGHBOURS = sorted({c ^ (1 << k) for c in _COUNTED for k in range(8)} - set(_COUNTED))
PAIR_SET = sorted(set(_COUNTED) | set(NEIGHBOURS) | {0x00, 0x7f, 0x80, 0xff})
_FILL = np.frombuffer(b"ATatKkOoJjFfSs\x03\x07\x0e\x23\x27\x2e\xc3\xe3\xc7\xe7\xce\xee\xff\x00\x7f\x80", dtype=np.uint8)
_HOSTILE = np.concatenate([np.frombuffer(b"ACGTacgt" * 6 + b"NnNn", dtype=np.uint8), _FILL])


def hostile(L, seed):
    """random bytes: mostly bases of both cases, the bit-neighbours of the counted bytes, bytes with bit 7 set, and runs of N"""
    rng = np.random.default_rng(seed)
    s = _HOSTILE[rng.integers(0, len(_HOSTILE), L)]
    for at, ln in zip(rng.integers(0, max(L, 1), max(1, L // 700)), rng.integers(1, 120, max(1, L // 700))):
        s[at:at + ln] = np.frombuffer(b"Nn", dtype=np.uint8)[rng.integers(0, 2, len(s[at:at + ln]))]
    return s


def one_bin(chars, gc, n, rng):
    """`chars` bytes with exactly `gc` of C c G g and `n` of N n, the rest bytes that count as neither, shuffled"""
    assert 0 <= gc and 0 <= n and gc + n <= chars, (chars, gc, n)
    b = np.empty(chars, dtype=np.uint8)
    b[:gc] = np.frombuffer(b"CcGg", dtype=np.uint8)[np.arange(gc) % 4]
    b[gc:gc + n] = np.frombuffer(b"Nn", dtype=np.uint8)[np.arange(n) % 2]
    b[gc + n:] = _FILL[rng.integers(0, len(_FILL), chars - gc - n)]
    rng.shuffle(b)
    return b


def tie_counts(chars):
    """every gc with 100*gc/chars exactly on a half"""
    return [g for g in range(chars + 1) if (200 * g) % chars == 0 and (200 * g // chars) & 1]


# ================================================================================================== the case table
CASES = OrderedDict()


def _add(name, kind, build, **meta):
    assert name not in CASES, name
    CASES[name] = dict(name=name, family=name.split("_")[0], kind=kind, build=build, **meta)


def get(name, num_cu=256):
    """the built case: kind 'seq' -> seq, bin, cut; kind 'fasta' -> raw, nbytes, len, lb, lw, bin, cut; both: ref ('literal' | 'counts'), meta"""
    c = dict(CASES[name])
    built = c.pop("build")(num_cu)
    if c["kind"] == "seq":
        seq, c["bin"], c["cut"] = built[:3]
        c["seq"] = np.ascontiguousarray(seq, dtype=np.uint8)
        c["len"] = len(c["seq"])
    else:
        (raw, c["len"], c["lb"], c["lw"]), c["bin"], c["cut"] = built[:3]
        c["raw"] = np.ascontiguousarray(raw, dtype=np.uint8)
        c["nbytes"] = len(c["raw"])
    c["meta"] = built[3] if len(built) > 3 else {}
    c["ref"] = "literal" if c["len"] <= LITERAL_MAX else "counts"
    return c


def stripped(c):
    return c["seq"] if c["kind"] == "seq" else np.frombuffer(strip_fasta(c["raw"], c["len"], c["lb"], c["lw"]), dtype=np.uint8)


def expected(c):
    return (gc_literal if c["ref"] == "literal" else gc_counts)(stripped(c), c["bin"], c["cut"])


def case_names(family=None):
    return [n for n, c in CASES.items() if family is None or c["family"] == family]


# -------------------------------------------------------------------------------------------------- alpha
def alphabet_expected(seq):
    """bin size 1, cut-off 0.5: what every single byte must give"""
    return np.where(np.isin(seq, GC_BYTES), 100, np.where(np.isin(seq, N_BYTES), -1, 0)).astype(np.int8)


def _alpha_positions():
    i = np.arange(16 * 256)
    return ((i + i // 256) % 256).astype(np.uint8)                 # row r holds value v at offset (v - r) % 256: all 16 chunk positions


def _alpha_in_filler(filler):
    chunks = np.full((16, 256, 16), filler, dtype=np.uint8)        # chunk (p, v): byte v at position p, the filler in the other fifteen
    for p in range(16):
        chunks[p, :, p] = np.arange(256)
    return chunks.reshape(-1)


def _alpha_pairs():
    stream = np.array([x for a in PAIR_SET for b in PAIR_SET for x in (a, b)], dtype=np.uint8)
    blocks = []
    for s in range(16):                                            # pair k sits at chunk positions (s + 2k) % 16 and the next: all sixteen
        blocks.append(np.concatenate([np.full(s, 0x41, np.uint8), stream, np.full(-(s + len(stream)) % 16, 0x41, np.uint8)]))
    return np.concatenate(blocks)


_add("alpha_each_byte", "seq", lambda cu: (np.arange(256, dtype=np.uint8), 1, 0.5))
_add("alpha_every_position", "seq", lambda cu: (_alpha_positions(), 1, 0.5))
_add("alpha_pairs", "seq", lambda cu: (_alpha_pairs(), 1, 0.5))
_add("alpha_pairs_bin2", "seq", lambda cu: (_alpha_pairs()[1:], 2, 0.5))
for _f, _fn in ((0x41, "A"), (0xff, "ff"), (0x47, "G"), (0x4e, "N")):
    for _z, _cut in ((16, 0.0), (1, 0.5), (50, 0.5)):
        _add("alpha_one_in_sixteen_%s_bin%d" % (_fn, _z), "seq", lambda cu, f=_f, z=_z, cut=_cut: (_alpha_in_filler(f), z, cut))
_add("alpha_every_position_large_bin", "seq", lambda cu: (np.tile(_alpha_positions(), 3)[:3 * 2049 + 7], 2049, 0.5))

# -------------------------------------------------------------------------------------------------- sat
def _saturation(reps=1):
    sym = (0x47, 0x4e, 0xff)
    chunks = [np.full(16, s, np.uint8) for s in sym]
    chunks += [np.full(16, x, np.uint8) for a in sym for b in sym for c in sym for x in (a, b, c)]
    return np.tile(np.concatenate(chunks), reps)


for _z in (1, 16, 32, 50, 64):
    _add("sat_bin%d" % _z, "seq", lambda cu, z=_z: (_saturation(), z, 0.5))
_add("sat_bin2049", "seq", lambda cu: (_saturation(5), 2049, 0.5))

# -------------------------------------------------------------------------------------------------- tie
TIE_FULL = (64, 200, 256, 2048)
TIE_SHORT = (8, 16, 24, 40, 48)


def _tie_full(chars, scale=1, seed=7):
    rng = np.random.default_rng(seed + chars * scale)
    ties = tie_counts(chars)
    assert {100 * g // chars & 1 for g in ties} == {0, 1}, chars   # a tie that stays and one that goes up
    bins, where = [], []
    for g in ties:
        for d in (-1, 0, 1):
            if d == 0:
                where.append((len(bins), scale * g, scale * chars))
            bins.append(one_bin(scale * chars, scale * g + d, 0, rng))
    return np.concatenate(bins), scale * chars, 0.5, {"ties": where}


def _tie_short(bin_size, chars, g, d, seed=11):
    rng = np.random.default_rng(seed + 1000 * chars + 10 * g + d)
    assert chars < bin_size and g in tie_counts(chars)
    seq = np.concatenate([hostile(2 * bin_size, seed + chars), one_bin(chars, g + d, 0, rng)])
    return seq, bin_size, 0.5, {"ties": [(2, g, chars)] if d == 0 else []}


for _c in TIE_FULL:
    _add("tie_full_bin%d" % _c, "seq", lambda cu, c=_c: _tie_full(c))
_add("tie_full_bin4096", "seq", lambda cu: _tie_full(2048, 2))
for _c in TIE_SHORT:
    assert {100 * g // _c & 1 for g in tie_counts(_c)} == {0, 1}, _c
    for _g in tie_counts(_c):
        for _d in (-1, 0, 1):
            _add("tie_short_chars%d_gc%d%+d" % (_c, _g, _d), "seq", lambda cu, c=_c, g=_g, d=_d: _tie_short(50, c, g, d))
for _g in tie_counts(2048):                                        # the 64-bit rounding on chars != bin_size
    for _d in (-1, 0, 1):
        _add("tie_short_large_bin4099_gc%d%+d" % (_g, _d), "seq", lambda cu, g=_g, d=_d: _tie_short(4099, 2048, g, d))

# -------------------------------------------------------------------------------------------------- thr
THR_BINS = (1, 2, 50, 64, 2048, 4099)


def thr_cutoffs(bin_size):
    k = max(1, bin_size // 3)
    exact = k / bin_size
    return [("0", 0.0), ("0.1", 0.1), ("0.5", 0.5), ("1", 1.0), ("1.5", 1.5), ("neg", -0.1), ("inf", math.inf), ("neginf", -math.inf),
            ("nan", math.nan), ("k_over_bin", exact), ("k_over_bin_below", math.nextafter(exact, -math.inf)),
            ("k_over_bin_above", math.nextafter(exact, math.inf))]


def _thr(bin_size, cut, short_at_n_min, seed=13):
    rng = np.random.default_rng(seed + bin_size)
    n_min = n_min_of(bin_size, cut)
    counts = sorted({0, bin_size} | {n for n in (n_min - 1, n_min) if 0 <= n <= bin_size})
    bins = [one_bin(bin_size, (bin_size - n) // 2, n, rng) for n in counts]
    where = [(i, n) for i, n in enumerate(counts)]
    if bin_size > 1:                                               # the short last bin: one base short, and still n / bin_size
        chars = bin_size - 1
        n = min(max(n_min if short_at_n_min else n_min - 1, 0), chars)
        where.append((len(bins), n))
        bins.append(one_bin(chars, (chars - n) // 2, n, rng))
    return np.concatenate(bins), bin_size, cut, {"n_min": n_min, "bins": where}


for _z in THR_BINS:
    for _cn, _cut in thr_cutoffs(_z):
        for _s in (True, False):
            _add("thr_bin%d_cut_%s_%s" % (_z, _cn, "short_at" if _s else "short_below"), "seq", lambda cu, z=_z, cut=_cut, s=_s: _thr(z, cut, s))

# -------------------------------------------------------------------------------------------------- word
def _word(bin_size, inverse):
    i = np.arange(4096 + 37)
    on = np.isin(i % 32, (0, 31)) != inverse
    return np.where(on, np.where(i % 3 == 0, 0x4e, 0x67), 0x41).astype(np.uint8), bin_size, 0.3


for _z in (1, 15, 16, 17, 31, 32, 33, 50, 64, 65, 96, 97):
    for _inv in (False, True):
        _add("word_bin%d_%s" % (_z, "all_but_edges" if _inv else "edges_only"), "seq", lambda cu, z=_z, inv=_inv: _word(z, inv))

# -------------------------------------------------------------------------------------------------- len
LEN_BINS = (1, 2, 15, 16, 17, 31, 32, 33, 50, 64, 255, 256, 257, 300, 2047, 2048)
AROUND = (-1, 0, 1, 15, 16, 17)


def len_lengths(bin_size):
    T = tile_bases(bin_size)
    return sorted({L for L in [1, bin_size - 1, bin_size, bin_size + 1] + [k * T + d for k in (1, 2) for d in AROUND] if L > 0})


for _z in LEN_BINS:
    for _L in len_lengths(_z):
        _add("len_bin%d_len%d" % (_z, _L), "seq", lambda cu, z=_z, L=_L: (hostile(L, 1000 * z + L % 997), z, 0.5))

# -------------------------------------------------------------------------------------------------- large
LARGE_BINS = (2049, 4099, 100_003)


def large_lengths(bin_size):
    base = (2 * bin_size + 40) // 16 * 16
    return sorted({bin_size - 1, bin_size, bin_size + 1, base + 1, base + 15, base + 16})


for _z in LARGE_BINS:
    for _L in large_lengths(_z):
        _add("large_bin%d_len%d" % (_z, _L), "seq", lambda cu, z=_z, L=_L: (hostile(L, 77 * z + L % 991), z, 0.5))
_add("large_grid_stride", "seq", lambda cu: (hostile((LARGE_BINS_PER_CU * cu + 37) * 2049 - 5, 4242), 2049, 0.5))

# -------------------------------------------------------------------------------------------------- fasta, trail
LF, CRLF, NONE = b"\n", b"\r\n", b""
LAYOUTS = [(1, CRLF), (1, LF), (2, LF), (7, LF), (31, LF), (32, LF), (33, CRLF), (60, LF), (61, LF), (64, LF), (65, LF), (2048, LF),
           ("len", NONE), ("len+5", LF)]
FASTA_BINS = (7, 50, 64, 2048)
TRAILING = b"\n>chrG_NNNNCCGG nnn\nGGGGNNNN"
_EOL_NAME = {LF: "lf", CRLF: "crlf", NONE: "none"}


def fasta_lengths(lb, bin_size):
    """lengths ending on a line end, one base before it and one after it, and one that crosses a tile boundary"""
    if isinstance(lb, str):
        return [3 * bin_size + 5, tile_bases(bin_size) + 37]
    k = max(2, -(-(3 * bin_size + bin_size // 2) // lb))
    return [k * lb - 1, k * lb, k * lb + 1, tile_bases(bin_size) + 37]


def _fasta(lb, eol, bin_size, L, trailing=b""):
    lb = {"len": L, "len+5": L + 5}.get(lb, lb)
    seq = hostile(L, 31 * lb + 7 * bin_size + L % 983)
    seq[np.isin(seq, (0x0a, 0x0d))] = 0x41                         # (the alphabet has neither; a base is never a line end)
    return wrap_fasta(seq, lb, eol, trailing), bin_size, 0.5, {"seq": seq}


for _lb, _eol in LAYOUTS:
    for _z in FASTA_BINS:
        for _L in fasta_lengths(_lb, _z):
            _add("fasta_line%s_%s_bin%d_len%d" % (_lb, _EOL_NAME[_eol], _z, _L), "fasta",
                 lambda cu, lb=_lb, eol=_eol, z=_z, L=_L: _fasta(lb, eol, z, L))
    for _L in fasta_lengths(_lb, 50)[1:3] if not isinstance(_lb, str) else fasta_lengths(_lb, 50)[:1]:
        _add("trail_line%s_%s_len%d" % (_lb, _EOL_NAME[_eol], _L), "fasta",
             lambda cu, lb=_lb, eol=_eol, L=_L: _fasta(lb, eol, 50, L, TRAILING))

N_CASES = len(CASES)


# ================================================================================================== many contigs in one call
PADDING = b"GGNNCCggnncc\xffGCN"                                    # what lies between two contigs' bytes: all of it would count


def many_group(bin_size):
    """the FASTA contigs of one bin size (the short lengths of every layout, with and without trailing bytes excluded) and one empty
    contig, each at a multiple of 16 with hostile bytes between: -> dict of the arrays tdt_gc_bins_fasta_many takes, and the contigs"""
    contigs = []
    for lb, eol in LAYOUTS:
        for L in fasta_lengths(lb, bin_size)[:3]:
            (raw, ln, b, w), _, _, meta = _fasta(lb, eol, bin_size, L)
            contigs.append(dict(raw=raw, len=ln, lb=b, lw=w, seq=meta["seq"]))
    contigs.insert(3, dict(raw=np.zeros(0, np.uint8), len=0, lb=60, lw=61, seq=np.zeros(0, np.uint8)))
    parts, raw_off, out_off, at, ob = [], [], [], 0, 0
    for i, c in enumerate(contigs):
        raw_off.append(at)
        out_off.append(ob)
        pad = -len(c["raw"]) % 16 + 16 * (i % 2)                   # up to the next multiple of 16, and every other time 16 bytes more
        parts += [c["raw"], np.frombuffer((PADDING * 2)[:pad], dtype=np.uint8)]
        at += len(c["raw"]) + pad
        ob += -(-c["len"] // bin_size)
    return dict(contigs=contigs, raw=np.concatenate(parts), raw_off=np.array(raw_off, np.int64), out_off=np.array(out_off, np.int64),
                raw_len=np.array([len(c["raw"]) for c in contigs], np.int64), len=np.array([c["len"] for c in contigs], np.int64),
                lb=np.array([c["lb"] for c in contigs], np.int32), lw=np.array([c["lw"] for c in contigs], np.int32), out_bytes=ob)
