"""The ``--sv`` scan with every consumer on one pass over RANDOM LEGAL records: the files of tests/scan_random_cases.py, six seeds, through
``tiddit_signal._scan`` exactly as tests/test_gpu_scan_all.py drives it (its ``_scan``, ``_collect`` and comparison, by import) — every
consumer attached at 64-KiB spans with the left-normalisation on, the clip chain and the STR stage behind the scan on the live objects,
every part against the definitions over the host reader's batches, piece by piece (a failure names the consumer) and as a whole.  The
signal rows, clip entries and 50-bp bins, which have no definition of their own there, against a host-ingest scan with nothing attached
(the literal Python rows).  One seed also at the default chunk, with host ingest for the four keyed consumers together, and with all six
stores made for 64 items; each equals that seed's all-on run.  Every comparison is exact.

What the files hold is pinned without a GPU by tests/test_scan_random_refs_cpu.py (the floors of scan_random_cases stand in for the non-emptiness asserts
test_gpu_scan_all.py ties to the designed file)."""
import pytest

import scan_all_cases as C
import scan_random_cases as RC
import test_gpu_scan_all as G

pytestmark = pytest.mark.gpu

ALSO = RC.SEEDS[0]                     # the seed that also runs at the default chunk, through host ingest and with the small stores


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """seed -> the file with everything ``test_gpu_scan_all.make`` gives, made when first asked for; the resident references are closed
    behind the module"""
    made = {}

    def of(seed):
        if seed not in made:
            made[seed] = G.make(str(tmp_path_factory.mktemp("scan_random_%d" % seed)), lambda d: RC.generate(d, seed))
        return made[seed]
    yield of
    for m in made.values():
        m.reference.close()


@pytest.fixture(scope="module")
def all_on(files):
    """seed -> that file's all-on run at 64-KiB spans (kept: the other runs of the seed are compared with it)"""
    runs = {}

    def of(seed):
        if seed not in runs:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("TIDDIT_INGEST_CHUNK", G.SPAN)
                mp.delenv("TIDDIT_HOST_INGEST", raising=False)
                runs[seed] = G._scan(files(seed), G.ATTACHABLE)
        return runs[seed]
    return of


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_all_on_at_64k_spans_every_consumer_equals_its_definition_on_random_records(files, all_on, monkeypatch, seed):
    m, R = files(seed), all_on(seed)
    assert R["batches"] >= RC.SPANS and R["records"] == m.info["n_records"] == m.E["records"] and list(R["track"]) == m.names
    batches = C.host_batches(m.bam)
    found = RC.measure(batches, m.E)
    assert all(found[k] >= v for k, v in RC.FLOORS.items()), {k: (found[k], v) for k, v in RC.FLOORS.items() if found[k] < v}
    G._equals_definitions(R, m.E, m.files)
    assert G._differing(R, G._as_run(m.E, m.files), [k for k in G.PARTS if k != "signals"]) == []
    # the signal tables: against the literal Python rows of a host-ingest scan with nothing attached
    monkeypatch.setenv("TIDDIT_HOST_INGEST", "1")
    H = G._scan(m, ())
    assert H["batches"] == 0
    data, splits, text = H["signals"]
    assert sum(len(v) for v in data.values()) > 0 and sum(len(v) for v in splits.values()) > 0 and sum(t.count(b">") for t in text.values()) > 0
    assert G._differing(R, H, ("cov", "signals")) == []


def test_the_default_chunk_equals_the_small_spans(files, all_on, monkeypatch):
    monkeypatch.delenv("TIDDIT_INGEST_CHUNK", raising=False)
    R = G._scan(files(ALSO), G.ATTACHABLE)
    assert 1 <= R["batches"] < all_on(ALSO)["batches"] and R["records"] == all_on(ALSO)["records"]
    assert G._differing(R, all_on(ALSO)) == []


def test_host_ingest_with_the_four_keyed_consumers_equals_the_all_on_run(files, all_on, monkeypatch):
    monkeypatch.setenv("TIDDIT_HOST_INGEST", "1")
    H = G._scan(files(ALSO), G.KEYED)
    assert H["batches"] == 0 and [k for k in G.PARTS if k in H] == ["cov", "signals"] + list(G.KEYED)
    assert G._differing(H, all_on(ALSO), ("cov", "signals") + G.KEYED) == []


def test_the_six_stores_grown_from_room_for_64_items_equal_the_all_on_run(files, all_on, monkeypatch):
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", G.SPAN)
    G._tiny(monkeypatch)
    R = G._scan(files(ALSO), G.ATTACHABLE)
    assert R["batches"] == all_on(ALSO)["batches"] and G._differing(R, all_on(ALSO)) == []
    G._grown(R)
