"""The N>1 benchmark path on CPU: world_size 2 over gloo (127.0.0.1).

bench.py shards pages by rank with no data-path collective; the process group
only provides the barrier and the max/sum reductions of the timing.  This
checks that those pieces behave across real processes, and the single-process
`--gpus N` plan (one runner thread per device, lib/batch_worker.c peer).
"""
import os
import socket
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, pages, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import bench
    d = bench.Dist()
    devices, firsts, n_gpus = bench.shard_plan(d.world, d.rank, d.local_rank, 1, 8, pages)
    assert devices == [rank] and n_gpus == world
    first, n = firsts[0], pages
    d.barrier()
    mx = d.max(float(rank + 1))
    tot = d.sum(float(n))
    bad = d.sum(0.0)
    d.barrier()
    d.close()
    q.put((rank, first, n, mx, tot + bad))


@pytest.mark.parametrize("world", [2])
def test_gloo_sharding_and_reductions(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    pages = 1000
    procs = [ctx.Process(target=_worker, args=(r, world, port, pages, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # shards are disjoint, consecutive and cover world * pages pages
    spans = [(first, first + n) for _, first, n, _, _ in res]
    assert spans[0][0] == 0
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 == b0
    assert spans[-1][1] == world * pages
    # max over ranks and the whole-job page count are the same on every rank
    assert all(mx == float(world) for _, _, _, mx, _ in res)
    assert all(tot == float(world * pages) for _, _, _, _, tot in res)


def test_single_process_device_fanout_plan():
    sys.path.insert(0, ROOT)
    import bench
    devices, firsts, n = bench.shard_plan(1, 0, 0, 4, 8, 1000)
    assert devices == [0, 1, 2, 3] and firsts == [0, 1000, 2000, 3000] and n == 4
    with pytest.raises(Exception, match="only 2 HIP devices"):
        bench.shard_plan(1, 0, 0, 4, 2, 1000)


def test_diag_guard():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.diag_guard("unpaper-hip 0.2 (gfx950)", {}, False) is True
    with pytest.raises(SystemExit):
        bench.diag_guard("unpaper-hip 0.2 (gfx950, diag)", {}, False)
    with pytest.raises(SystemExit):
        bench.diag_guard("unpaper-hip 0.2 (gfx950)", {"UPHIP_DIAG_SKIP": "1"}, False)
    assert bench.diag_guard("unpaper-hip 0.2 (gfx950, diag)", {}, True) is False


def test_product_library_has_no_diagnostics():
    """`make lib` builds without UPHIP_DIAG: the version string says so, and
    the library reads no diagnostics or debug variable at all (UPHIP_DIAG_*,
    UPHIP_DEBUG_*): no hidden sync or host print in the product path."""
    sys.path.insert(0, os.path.join(ROOT, "unpaper-gpu_amd", "python"))
    from unpaper_hip.device import LIB_PATH, load_library
    L = load_library()
    assert "diag" not in L.uphip_version().decode()
    with open(LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"UPHIP_DIAG" not in blob
    assert b"UPHIP_DEBUG" not in blob


def test_dump_outputs_is_a_fixed_sample_of_the_last_chunk(tmp_path):
    """--dump-outputs: of the batch that holds the shard's last chunk (72
    pages in 64-sheet batches: pages 64..71) a seeded choice of rows of every
    sheet, float32, within the 64 MB the option may write, the same from run
    to run."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    h, w = 3508, 2480

    def sheet(page):
        return np.random.default_rng(page).integers(0, 256, (h, w), dtype=np.uint8)

    class Image:
        def __init__(self, a):
            self.a = a

        def payload(self):
            return self.a

    class FakeBatch:
        def __init__(self, first):
            self.first = first

        def output(self, s):
            return Image(sheet(self.first + s))

    class FakeRunner:
        streams = 3
        chunks = [(0, 64), (64, 8), None]

        def slot_chunk(self, i, k):
            return self.chunks[k]

        def batch(self, i, k):
            return FakeBatch(self.chunks[k][0])

    info = bench.dump_outputs(str(tmp_path / "a"), FakeRunner(), [0], 0, 1, 72, 64)
    assert info["files"] == ["sheets_gpu0.npy"] and info["pages"] == [[64, 72]]
    got = np.load(tmp_path / "a" / "sheets_gpu0.npy")
    assert got.dtype == np.float32 and got.shape == (8, info["rows"], w)
    assert 1 < info["rows"] <= h and got.nbytes <= 64e6
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(h, info["rows"], replace=False))
    for s in range(8):
        assert np.array_equal(got[s], sheet(64 + s)[rows].astype(np.float32)), s
    bench.dump_outputs(str(tmp_path / "b"), FakeRunner(), [0], 0, 1, 72, 64)
    assert np.array_equal(got, np.load(tmp_path / "b" / "sheets_gpu0.npy"))
    # all GPUs of a job share the budget; pages are numbered over the whole job
    info2 = bench.dump_outputs(str(tmp_path / "c"), FakeRunner(), [72], 1, 2, 72, 64)
    assert info2["files"] == ["sheets_gpu1.npy"] and info2["pages"] == [[136, 144]]
    assert info2["rows"] <= info["rows"] // 2 + 1
