"""The N-rank protocol of the variant stage (tiddit_variant.evidence_sharded) over gloo on the CPU, with stand-in stores: rank 0's
queries reach every rank, the per-rank counts are summed exactly on rank 0, and a failure on any rank ends every rank with an
error instead of a hang."""
import os
import socket
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHROMS = ["chr1", "chr2", "chr3"]
QUERIES = [("chr1", 100, 900, 500), ("chr2", 5, 5, 5), ("chr1", 100, 900, 500), ("chr3", 7000, 9000, 7100), ("chr2", 40, 4000, 3000)]


class FakeStore:
    """counts that depend on the rank and the query, and a record of what was asked"""

    def __init__(self, rank, fail=False):
        self.rank, self.fail, self.closed, self.seen = rank, fail, False, None
        self.tid = {c: i for i, c in enumerate(CHROMS)}

    def region_counts(self, queries, min_q, max_ins):
        self.seen = np.array(queries, dtype=np.int64).copy()
        if self.fail:
            raise RuntimeError("counts failed on rank %d" % self.rank)
        return counts_of(self.rank, self.seen, min_q, max_ins)

    def close(self):
        self.closed = True


def counts_of(rank, rows, min_q, max_ins):
    rows = np.asarray(rows, dtype=np.int64)
    k = np.arange(7, dtype=np.int64)
    return (rank + 1) * (rows[:, 1:2] * 7 + rows[:, 2:3] + rows[:, 3:4] * 3 + rows[:, 0:1] * 1000 + k) + min_q + max_ins


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q, mode):
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tiddit_amd import tiddit_variant
        store = FakeStore(rank, fail=(mode == "rank1_fails" and rank == 1))
        queries = None
        if rank == 0:
            queries = list(QUERIES) + ([("chrX", 1, 2, 1)] if mode == "rank0_fails" else [])     # (no such contig: rank 0 fails)
        try:
            got = tiddit_variant.evidence_sharded(store, queries, 20, 600)
        except Exception as e:
            q.put((rank, ("raised", repr(e), store.closed)))
            return
        q.put((rank, ("ok", got, None if store.seen is None else store.seen.tolist())))
    except BaseException:  # pragma: no cover
        import traceback
        q.put((rank, ("crash", traceback.format_exc(), None)))
    finally:
        dist.destroy_process_group()


def _run(world, mode):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q, mode)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=120) for _ in procs)          # (a hang ends the test here)
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_evidence_sharded_sums_exactly(world):
    from tiddit_amd import tiddit_variant
    res = _run(world, "ok")
    assert all(v[0] == "ok" for v in res.values()), res
    keys = list(dict.fromkeys(QUERIES))
    rows = np.array([(CHROMS.index(c), s, e, bp) for c, s, e, bp in keys], dtype=np.int64)
    for r in range(world):
        assert res[r][2] == rows.tolist(), r                  # every rank answered the same deduplicated rows
    assert res[1][1] is None and (world < 3 or res[2][1] is None)
    total = sum(counts_of(r, rows, 20, 600) for r in range(world))
    want = {k: tiddit_variant.region_tuple(total[i], k[1], k[2]) for i, k in enumerate(keys)}
    assert res[0][1] == want


@pytest.mark.parametrize("world", [2, 3])
def test_rank0_failure_before_the_broadcast_ends_every_rank(world):
    res = _run(world, "rank0_fails")
    assert sorted(res) == list(range(world))
    assert res[0][0] == "raised" and "chrX" in res[0][1]
    for r in range(1, world):
        assert res[r][0] == "raised" and "rank 0 failed" in res[r][1] and res[r][2], (r, res[r])     # raised, store closed


@pytest.mark.parametrize("world", [2, 3])
def test_counts_failure_on_another_rank_ends_every_rank(world):
    res = _run(world, "rank1_fails")
    assert sorted(res) == list(range(world))
    assert res[1][0] == "raised" and "counts failed on rank 1" in res[1][1]
    assert res[0][0] == "raised" and "1 other rank" in res[0][1]
    for r in range(2, world):
        assert res[r][0] == "ok" and res[r][1] is None
