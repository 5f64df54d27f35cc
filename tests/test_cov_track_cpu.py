"""`TIDDIT_COV_TRACK=Z[:Q[:bed|wig]]` without a GPU: the switch's parser, the refusal of a malformed value before anything is created
or any device is touched, and the switch-off path of `run_sv` (nothing new is asked of the statistics pass or the scan)."""
import os

import pytest


def test_parser_accepts_the_documented_forms_with_the_defaults_of_cov():
    from tiddit_amd.__main__ import _cov_parser, parse_cov_track
    d = _cov_parser().parse_args(["--cov", "--bam", "x.bam"])
    assert parse_cov_track("500") == (500, d.q, "bed") == (500, 20, "bed") and d.z == 500 and not d.w
    assert parse_cov_track("100:0:wig") == (100, 0, "wig")
    assert parse_cov_track("2000:20") == (2000, 20, "bed")
    assert parse_cov_track("50:5") == (50, 5, "bed")
    assert parse_cov_track("1") == (1, 20, "bed")
    assert parse_cov_track("1024:60:bed") == (1024, 60, "bed")
    assert parse_cov_track(None) is None and parse_cov_track("") is None


@pytest.mark.parametrize("value", ["0", "-5", "0:20", "abc", "5.5", "1e3", "500:x", "500:2.5", "500:20:bam", "500:20:BED", "500:20:bed:1", ":", "500:",
                                   "500::wig", " 500", "5_0", "500:20:"])
def test_parser_rejects_malformed_values(value):
    from tiddit_amd.__main__ import parse_cov_track
    with pytest.raises(ValueError):
        parse_cov_track(value)


@pytest.mark.parametrize("value", ["0", "abc", "500:20:bam", "1:2:bed:4"])
def test_a_rejected_value_quits_before_the_output_folder_and_the_device(value, tmp_path, monkeypatch, capsys):
    """one error line, then quit(): `{o}_tiddit` is not made, no reference index is written, and nothing reached the device (on a box
    without one any touch raises TdtError instead of SystemExit)"""
    from tiddit_amd import __main__ as cli
    monkeypatch.setenv("TIDDIT_COV_TRACK", value)
    out = str(tmp_path / "out")
    ref = str(tmp_path / "ref.fa")
    open(ref, "w").write(">c\nACGT\n")
    with pytest.raises(SystemExit):
        cli.main(["--sv", "--bam", str(tmp_path / "none.bam"), "--ref", ref, "-o", out, "--skip_assembly"])
    text = capsys.readouterr().out
    lines = [l for l in text.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("error, TIDDIT_COV_TRACK=" + value)
    assert not os.path.exists(out + "_tiddit") and sorted(os.listdir(str(tmp_path))) == ["ref.fa"]


class _Stop(Exception):
    pass


def _tiny_job(tmp_path):
    from tiddit_amd import bamio
    bam, ref = str(tmp_path / "t.bam"), str(tmp_path / "ref.fa")
    w = bamio.BamWriter(bam, [("c1", 2000)])
    w.write("r1", 0, 0, 100, 60, "50M", -1, -1, 0, "A" * 50)
    w.close()
    open(ref, "w").write(">c1\n" + "ACGT" * 500 + "\n")
    return bam, ref


@pytest.mark.parametrize("value,want", [(None, None), ("", None), ("500", (500, 20)), ("100:0:wig", (100, 0))])
def test_run_sv_hands_the_request_on_only_when_the_switch_is_set(value, want, tmp_path, monkeypatch):
    """switch unset: the statistics pass is called as before (no track_bin_size) and the scan's module attribute is at its default when
    tiddit_signal.main runs; set: both receive the request, and the attribute is back at its default when the stage is left"""
    from tiddit_amd import __main__ as cli, tiddit_signal, tiddit_stats
    bam, ref = _tiny_job(tmp_path)
    if value is None:
        monkeypatch.delenv("TIDDIT_COV_TRACK", raising=False)
    else:
        monkeypatch.setenv("TIDDIT_COV_TRACK", value)
    monkeypatch.setenv("TIDDIT_GC_OVERLAP", "0")                  # (no helper thread: this test never reaches a device)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TIDDIT_FORCE_DIST", raising=False)
    seen = {}

    def statistics(*a, **k):
        seen["statistics"] = k
        return {"avg_read_length": 50.0, "avg_insert_size": 300, "std_insert_size": 30, "percentile_insert_size": 500, "mp": False}

    def signal_main(*a, **k):
        seen["COV_TRACK"] = tiddit_signal.COV_TRACK
        raise _Stop()
    monkeypatch.setattr(tiddit_stats, "statistics", statistics)
    monkeypatch.setattr(tiddit_signal, "main", signal_main)
    assert tiddit_signal.COV_TRACK is None
    with pytest.raises(_Stop):
        cli.main(["--sv", "--bam", bam, "--ref", ref, "-o", str(tmp_path / "o"), "--skip_assembly"])
    assert seen["COV_TRACK"] == want and tiddit_signal.COV_TRACK is None
    if want is None:
        assert seen["statistics"] == {"carry": True}
    else:
        assert seen["statistics"] == {"carry": True, "track_bin_size": want[0]}
    assert not os.path.exists(str(tmp_path / "o.bed")) and not os.path.exists(str(tmp_path / "o.wig"))


def test_bins_by_contig_finds_contigs_by_name():
    """the helper `--cov` and the track share: a contig's bins are cut out of the one array at the offset of its NAME, whatever the
    order of the names it is asked for"""
    import numpy as np
    from tiddit_amd import tiddit_coverage

    class Hist:
        names = ["c%d" % i for i in range(70)]

        def total_bins(self):
            return sum(range(1, 71))

        def offset(self, n):
            i = self.names.index(n)
            return sum(range(1, i + 1))

        def nbins(self, n):
            return self.names.index(n) + 1, 0

        def finish_all(self):
            return np.arange(self.total_bins(), dtype=np.float64)

    h = Hist()
    order = list(reversed(h.names))
    got = tiddit_coverage.bins_by_contig(h, order)
    assert list(got) == order
    for n in h.names:
        i = h.names.index(n)
        assert np.array_equal(got[n], np.arange(h.offset(n), h.offset(n) + i + 1, dtype=np.float64))
    with pytest.raises(ValueError):
        tiddit_coverage.bins_by_contig(h, order, np.zeros(3))
