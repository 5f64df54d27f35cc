"""The references of tests/depth_cases.py hold the definitions of tiddit_amd/tiddit_depth.py, and the host side of the feature —
windows_of, the column and header text — needs no GPU."""
import os
import re

import numpy as np

import depth_cases as DC
from tiddit_amd import tiddit_depth as D
from tiddit_amd import tiddit_genotype as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_restatements_agree():
    for sites, cov, gc in (DC.told_apart_case(), DC.small_contigs()):
        a = [DC.site_values(s[1], s[3], cov[s[0]], gc[s[0]]) for s in sites if s[0] == s[2]]
        b = [DC.site_values_sorted(s[1], s[3], cov[s[0]], gc[s[0]]) for s in sites if s[0] == s[2]]
        assert len(a) > 6
        assert np.array_equal(np.array(a).view(np.uint64), np.array(b).view(np.uint64))                  # bit for bit, nan included
        assert DC.depth_reference(sites, cov, gc) == DC.depth_reference(sites, cov, gc, values=DC.site_values_sorted)


def test_every_departure_is_told_apart():
    sites, cov, gc = DC.told_apart_case()
    want = DC.depth_reference(sites, cov, gc)
    assert want[-1] == (".", ".", ".")
    numeric = [w for w in want if all(re.fullmatch(r"[0-9]+\.[0-9]{3}", x) for x in w)]
    assert len(numeric) == len(sites) - 1                      # the reference yields all three values on every one-contig site
    for name, kw in DC.DEPARTURES.items():
        assert DC.depth_reference(sites, cov, gc, **kw) != want, name


def test_zero_coverage_is_usable_and_empty_denominators_give_dots():
    cov = np.array([3.0] * 30 + [0.0] * 10 + [3.0] * 30)
    gc = np.full(70, 40, dtype=np.int8)
    assert DC.depth_reference([DC.site("c", 1500, "c", 2000)], {"c": cov}, {"c": gc}) == [("0.000", "0.000", "0.000")]      # a homozygous deletion
    gc2 = gc.copy()
    gc2[30:40] = -1
    assert DC.depth_reference([DC.site("c", 1500, "c", 2000)], {"c": cov}, {"c": gc2}) == [(".", ".", ".")]                  # I has no usable bin
    gc3 = gc.copy()
    gc3[10:30] = gc3[40:60] = -1
    assert DC.depth_reference([DC.site("c", 1500, "c", 2000)], {"c": cov}, {"c": gc3}) == [("0.000", "0.000", ".")]          # F has none
    assert DC.depth_reference([DC.site("c", 1500, "c", 2000)], {"c": np.zeros(70)}, {"c": gc}) == [(".", ".", ".")]          # C, G: no bin; F is 0


def _loop_windows(sites, contig_bins):
    """windows_of's rows by the literal definition"""
    rows = []
    order = list(contig_bins)
    for s in sites:
        if s[0] != s[2] or s[0] not in contig_bins or contig_bins[s[0]][1] < 1:
            rows += [[0, -1, -1, -1, -1, -1]] * 3
            continue
        off, nb = contig_bins[s[0]]
        lo, hi = min(s[1], s[3]), max(s[1], s[3])
        inside = [b for b in range(lo // 50, (lo if lo == hi else hi - 1) // 50 + 1)]
        inside = sorted({min(max(b, 0), nb - 1) for b in inside})
        first, last = inside[0], inside[-1]
        below = [b for b in range(first - 20, first) if 0 <= b < nb]
        above = [b for b in range(last + 1, last + 21) if 0 <= b < nb]
        fl = [below[0], below[-1]] if below else [-1, -1]
        fl += [above[0], above[-1]] if above else [-1, -1]
        rows += [[off, first, last, -1, -1, -1], [off] + fl + [-1], [off, first, last, -1, -1, order.index(s[0])]]
    return np.array(rows, dtype=np.int64).reshape(-1, 6)


def test_windows_of_clips_as_defined():
    for sites, cov, gc in (DC.told_apart_case(), DC.small_contigs()):
        bins, o = {}, 0
        for c in cov:
            bins[c] = (o, len(cov[c]))
            o += len(cov[c])
        t = D.windows_of(sites, bins)
        assert t.dtype == np.int64 and t.shape == (3 * len(sites), 6)
        assert np.array_equal(t, _loop_windows(sites, bins))
    one = {"c": (7, 1)}                                        # one bin: it is the inside, and there is no flank
    assert D.windows_of([DC.site("c", 0, "c", 50), DC.site("c", 900, "c", 10)], one).tolist() == \
        [[7, 0, 0, -1, -1, -1], [7, -1, -1, -1, -1, -1], [7, 0, 0, -1, -1, 0]] * 2
    far = D.windows_of([DC.site("c", 5000, "c", 9000)], {"c": (0, 41)})                 # both breakpoints behind the contig's end
    assert far.tolist() == [[0, 40, 40, -1, -1, -1], [0, 20, 39, -1, -1, -1], [0, 40, 40, -1, -1, 0]]
    assert D.windows_of([DC.site("c", 1, "c", 2)], {"c": (0, 0)}).tolist() == [[0, -1, -1, -1, -1, -1]] * 3
    assert D.windows_of([], {"c": (0, 5)}).shape == (0, 6)


def test_medians_of_is_numpy_median():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 4, 101, 1000):
        v = rng.random(n) * 1e3
        s = np.sort(v)
        m = D.medians_of([s[(n - 1) // 2]], [s[n // 2]], [n])
        assert m[0].tobytes() == np.float64(np.median(v)).tobytes()
    assert np.isnan(D.medians_of([0.0], [0.0], [0])[0])


def test_field_strings():
    nan = float("nan")
    assert D.fields_of(10.0, 20.0, 30.0, 8.0) == ("0.500", "0.333", "1.250")
    assert D.fields_of(0.0, 20.0, 30.0, 8.0) == ("0.000", "0.000", "0.000")
    assert D.fields_of(nan, 20.0, 30.0, 8.0) == (".", ".", ".")
    assert D.fields_of(10.0, 0.0, nan, 0.0) == (".", ".", ".")
    assert D.fields_of(10.0, nan, 4.0, 0.0) == (".", "2.500", ".")
    assert D.fields_of(1.0, 3.0, 3.0, 3.0) == DC.strings_of(1.0, 3.0, 3.0, 3.0) == ("0.333",) * 3


def test_column_and_header_text(monkeypatch):
    from tiddit_amd import tiddit_variant
    monkeypatch.setattr(G, "sample_column", lambda s, *a: "0/1:2:1,2,3:4:5:0,0:6,7:8,9")
    sites = [DC.site("c", 1, "c", 2), DC.site("c", 1, "d", 2)]
    plain = G.sample_columns(sites, {}, [0, 0], [(4, 5), (4, 5)], None, None)
    assert plain == ["0/1:2:1,2,3:4:5:0,0:6,7:8,9"] * 2
    cols = G.sample_columns(sites, {}, [0, 0], [(4, 5), (4, 5)], None, None, depth=[("0.512", "0.498", "0.503"), (".", ".", ".")])
    assert cols == [plain[0] + ":0.512:0.498:0.503", plain[1] + ":.:.:."]
    assert G.format_col() == tiddit_variant.FORMAT_COL == "GT:CN:COV:DV:RV:LQ:RR:DR"
    assert G.format_col(True) == "GT:CN:COV:DV:RV:LQ:RR:DR:DHFC:DHBFC:DHFFC"
    base = "##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"
    meta = ['##INFO=<ID=XX,Number=1,Type=Integer,Description="x">']
    off = G.header(base, meta, "sites.vcf", 500).split("\n")
    on = G.header(base, meta, "sites.vcf", 500, depth=True).split("\n")
    assert [l for l in on if l not in off] == on[-5:-2] == list(D.FORMAT_LINES)
    assert [l for l in on if l in off] == off and on[-2].startswith("##TIDDITgenotype=") and on[-1].startswith("#CHROM")
    for line, name in zip(D.FORMAT_LINES, ("DHFC", "DHBFC", "DHFFC")):
        assert line.startswith("##FORMAT=<ID={},Number=1,Type=Float,Description=\"".format(name)) and line.endswith("\">")


def test_write_vcf_format_column(tmp_path):
    rec = [(1, ["c", "5", "id", "N", "<DEL>", ".", "PASS", "SVTYPE=DEL;END=900", "GT", "./."])]
    for depth, fmt in ((False, "GT:CN:COV:DV:RV:LQ:RR:DR"), (True, "GT:CN:COV:DV:RV:LQ:RR:DR:DHFC:DHBFC:DHFFC")):
        p = str(tmp_path / ("o%d.vcf" % depth))
        G.write_vcf(p, "#CHROM", rec, ["col"], **({"depth": True} if depth else {}))
        assert open(p).read() == "#CHROM\n" + "\t".join(rec[0][1][:8] + [fmt, "col"]) + "\n"


def test_the_limit_is_a_define_of_the_source():
    src = open(os.path.join(REPO, "tiddit_amd", "csrc", "tdt_depth.hip")).read()
    m = re.search(r"^#define DP_WINDOW_LIMIT (\d+)\b", src, flags=re.M)
    assert m and int(m.group(1)) >= 64
