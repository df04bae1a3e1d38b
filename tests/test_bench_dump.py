"""bench.py --dump-outputs (dump_outputs) without a GPU: the decode leg's device buffers are stood
in for by the oracle's outputs of the same seeded blocks, and the files written are checked for
names, dtypes, the byte budget and their content; --full is off unless asked for."""
import os
import sys
import types

import numpy as np

import bench
from tools import workload as wl

N = 300


class _Buf:
    """DevBuf.download over a host array."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)

    def download(self, nbytes=None, off=0, dtype=np.uint8):
        n = self.a.size - off if nbytes is None else nbytes
        return self.a[off:off + n].copy().view(dtype)


def test_dump_outputs_files(oracle, tmp_path):
    import slatecodec as sc
    blob, off = wl.block_set(sc.SNAPPY, 0, 1, N, seed=bench.SEED, threads=2)
    out, oo, meta, rows, rb = oracle.block_decode_batch(oracle.SNAPPY, blob[:int(off[-1])], off)
    assert (meta["status"] == 0).all()
    leg = types.SimpleNamespace(n=N, d_meta=_Buf(meta), d_out_off=_Buf(oo), d_row_base=_Buf(rb), d_out=_Buf(out),
                                d_rows=_Buf(rows))
    d = str(tmp_path / "dump")
    bench.dump_outputs(d, sc, leg)
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert sorted(got) == ["block_index", "blocks_all", "decoded", "meta", "out_off", "row_base", "rows"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= bench.DUMP_BUDGET
    # N is below the sample size: every block is in the sample, in order
    assert np.array_equal(got["block_index"], np.arange(N))
    dl = meta["data_len"].astype(np.int64) + 2 * meta["n_rows"] + 2
    want = np.concatenate([out[int(oo[k]):int(oo[k]) + int(dl[k])] for k in range(N)])
    assert np.array_equal(got["decoded"], want.astype(np.float32))
    want_rows = np.concatenate([rows[int(rb[k]):int(rb[k]) + int(meta["n_rows"][k])] for k in range(N)])
    for j, f in enumerate(sc.ROW_DTYPE.names):
        assert np.array_equal(got["rows"][:, j], want_rows[f].astype(np.float32)), f
    for j, f in enumerate(sc.META_DTYPE.names):
        assert np.array_equal(got["meta"][:, j], meta[f].astype(np.float64)), f
    assert np.array_equal(got["out_off"], oo.astype(np.float64))
    assert np.array_equal(got["row_base"], rb.astype(np.float64))
    assert np.array_equal(got["blocks_all"][:, 1], meta["data_len"].astype(np.float32))


def test_dump_sample_is_fixed_and_within_budget(monkeypatch):
    """More blocks than the sample holds: the same seeded blocks every time, sized to the budget."""
    import slatecodec as sc
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BLOCKS", 64)
    n = 4 * bench.DUMP_SAMPLE_BLOCKS
    meta = np.zeros(n, sc.META_DTYPE)
    meta["data_len"], meta["n_rows"] = 3920, 38
    slot = 4016
    leg = types.SimpleNamespace(n=n, d_meta=_Buf(meta), d_out_off=_Buf(np.arange(n + 1, dtype=np.uint64) * slot),
                                d_row_base=_Buf(np.arange(n + 1, dtype=np.uint64) * 38),
                                d_out=_Buf(np.arange(n * slot, dtype=np.uint32).astype(np.uint8)),
                                d_rows=_Buf(np.zeros(n * 38, sc.ROW_DTYPE)))
    saved = []
    monkeypatch.setattr(np, "save", lambda path, a: saved.append((os.path.basename(path), a)))
    monkeypatch.setattr(os, "makedirs", lambda *a, **k: None)
    bench.dump_outputs("unused", sc, leg)
    first = dict(saved)
    del saved[:]
    bench.dump_outputs("unused", sc, leg)
    idx = first["block_index.npy"]
    assert len(idx) == bench.DUMP_SAMPLE_BLOCKS and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert all(np.array_equal(first[k], a) for k, a in saved)
    assert sum(a.nbytes for a in first.values()) <= bench.DUMP_BUDGET
    k = int(idx[5])
    assert np.array_equal(first["decoded.npy"][5 * 3998:6 * 3998],
                          (np.arange(k * slot, k * slot + 3998) % 256).astype(np.float32))


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.dump_outputs == "" and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
