"""The promises of the generators behind tests/test_get_shapes_gpu.py (value lengths, rows with
timestamps, long keys, many blocks, the 2 048 / 2 049 row counts, the query list that is longer
than the fused kernel's grid), and the point-read reference on blocks that compress better than
24:1 and against a plain dict lookup on every new SST (CPU only)."""
import random

import pytest

from oracle import binding as ob
from tests import getgen, getref, sstgen


def dict_lookup(kvs, keys, ref):
    """The reference's answers are those of a dict over the SST's KVs (None: a tombstone)."""
    kvd = dict(kvs)
    rs, val_off, vals = ref[:3]
    assert int(val_off[-1]) == len(vals)
    for i, (k, r) in enumerate(zip(keys, rs)):
        got = vals[int(val_off[i]):int(val_off[i + 1])]
        if k not in kvd:
            assert r["outcome"] == getref.MISS and r["sst"] == 1 and got == b"", k
        elif kvd[k] is None:
            assert r["outcome"] == getref.TOMBSTONE and r["sst"] == 0 and got == b"", k
        else:
            assert r["outcome"] == getref.VALUE and r["sst"] == 0 and got == kvd[k], k
            assert r["value_len"] == len(kvd[k])
        assert r["err"] == 0, k


@pytest.mark.parametrize("codec", getgen.CODECS)
def test_reference_decodes_a_block_that_compresses_past_24_to_1(codec):
    none = sstgen.none_sst([(b"a", b"x"), (b"key", b"\x07" * 70000), (b"z", b"y")], 4096, 0, 10)
    sst = none if codec == ob.NONE else sstgen.recode(none, codec, random.Random(codec))
    s = getref.RefSst(sst)
    assert s.open_status == 0 and len(s.metas) == 3
    if codec in (ob.ZLIB, ob.LZ4, ob.ZSTD):  # (Snappy's copies reach 21:1)
        start, end = s.metas[1][0], s.metas[2][0]
        assert 24 * (end - start) < 70000  # the default capacity would not hold it
    r = getref.get_one([s], b"key")
    assert (r["outcome"], r["value_len"], r["err"], r["block"]) == (getref.VALUE, 70000, 0, 1)
    assert r["value"] == b"\x07" * 70000
    st, data, offs = s.block(1)
    assert st == 0 and len(data) == 70000 + 17 + 3 and offs == [0]


def test_value_edges_contain_what_they_claim():
    kvs = getgen.kvs_value_edges()
    assert 70 <= len(kvs) <= 90 and list(kvs) == sorted(kvs)
    lens = [len(v) for _, v in kvs if v is not None]
    assert set(lens) == set(getgen.VALUE_LENGTHS) and all(lens.count(n) == 3 for n in getgen.VALUE_LENGTHS)
    assert getgen.VALUE_LENGTHS == (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 143, 144, 145, 255, 256, 257, 1024,
                                    4097, 65521, 70000)
    assert sum(1 for _, v in kvs if v is None) >= 3 and sum(1 for _, v in kvs if v == b"") == 3
    # neighbours in key order differ in length, so a copy past its end lands in another value
    assert all(len(a or b"") != len(b or b"") for (_, a), (_, b) in zip(kvs, kvs[1:]) if a and b)
    s = getref.RefSst(getgen.value_edges_sst(ob.NONE))
    kvd = dict(kvs)
    wraps = over = 0
    for b, fk in enumerate(s.first_keys):
        st, data, offs = s.block(b)
        assert st == 0
        if len(kvd[fk] or b"") >= 4097:
            assert len(offs) == 1  # alone in its block
        if len(kvd[fk] or b"") == 65521:
            assert len(data) > 65536 and len(data) % 65536 < 16  # uint16(len(Data)) wraps to a few bytes
            wraps += 1
        if len(kvd[fk] or b"") == 70000:
            assert len(data) > 65536
            over += 1
    assert wraps == 3 and over == 3
    q = list(getgen.value_edges_queries())
    assert all(q.count(k) == 3 for k, _ in kvs) and sum(1 for k in q if k not in kvd) >= len(kvs)


@pytest.mark.parametrize("codec", getgen.CODECS)
def test_value_edges_reference_is_a_dict_lookup(codec):
    q = list(getgen.value_edges_queries())
    ref = getgen.ref_of([getgen.value_edges_sst(codec)], q)
    dict_lookup(getgen.kvs_value_edges(), q, ref)
    empty = [r for k, r in zip(q, ref[0]) if dict(getgen.kvs_value_edges()).get(k) == b""]
    assert len(empty) == 9 and all(r["outcome"] == getref.VALUE and r["value_len"] == 0 for r in empty)


@pytest.mark.parametrize("codec", getgen.CODECS)
def test_timestamped_rows(codec):
    sst, kinds = getgen.timestamped_sst(codec)
    q = list(getgen.query_set("random", 512))
    kvd = dict(getgen.kv_set("random"))
    for kind in getgen.TS_KINDS:
        assert sum(1 for k in q if kinds.get(k) == kind) >= 100, kind
        assert sum(1 for k in q if kinds.get(k) == kind and kvd[k] is None) >= 3, kind  # tombstones too
    ref = getgen.ref_of([sst], q)
    dict_lookup(getgen.kv_set("random"), q, ref)
    if codec == ob.NONE:  # the rows carry what the kinds say
        s = getref.RefSst(sst)
        seen = {kind: 0 for kind in getgen.TS_KINDS}
        for b in range(len(s.metas)):
            st, data, offs = s.block(b)
            first = ob.v0_decode(data[offs[0]:], None).key_suffix
            for o in offs:
                row = ob.v0_decode(data[o:], len(first))
                assert row.status == 0
                kind = kinds.get(first[:row.key_prefix_len] + row.key_suffix, "none")
                assert (row.expire_ms is not None, row.create_ms is not None) == (kind in ("expire", "both"),
                                                                                 kind in ("create", "both"))
                seen[kind] += 1
        assert min(seen.values()) >= 100


@pytest.mark.parametrize("codec", getgen.CODECS)
def test_mixed_keys(codec):
    kvs = getgen.kvs_mixed()
    q = list(getgen.mixed_queries())
    s = getref.RefSst(getgen.mixed_sst(codec))
    assert s.open_status == 0 and s.filter is not None and len(s.metas) == 200
    ref = getgen.ref_of([s], q)
    dict_lookup(kvs, q, ref)
    if codec == ob.NONE:
        kvd = dict(kvs)
        ks = [k for k, _ in kvs]
        assert min(len(k) for k in ks) == 8 and max(len(k) for k in ks) >= 250
        assert all(k in q for k in ks) and b"" in q
        assert sorted(len(k) for k in q)[-2:] == [1000, 65535]
        absent = [k for k in q if k not in kvd]
        assert sum(1 for k in absent if any(p.startswith(k) for p in ks)) >= 100  # strict prefixes
        assert sum(1 for k in absent if k[-1:] == b"\x00" and k[:-1] in kvd) >= 100
        assert sum(1 for k in absent if len(k) >= 1000 and any(k.startswith(p) for p in ks)) == 2
        # the two long keys pass range and are looked for in a block
        assert all(r["stage"] >= getref.AT_FILTER for k, r in zip(q, ref[0]) if len(k) >= 1000)
        assert sum(1 for r in ref[0] if r["stage"] == getref.AT_ROW and r["outcome"] == getref.MISS) >= 100


def test_many_blocks():
    s = getref.RefSst(getgen.many_blocks_sst(ob.NONE))
    nb = len(s.metas)
    assert nb > 2048 and nb % 1024 != 0 and (nb + 1023) // 1024 == 3
    assert len(getgen.query_set("random", 64)) == getgen.N_QUERIES
    rs, _, _, consulted = getgen.reference("random", 64, ob.NONE)
    blocks = {b for _, b in consulted}
    # blocks read on both sides of each 1 024-block boundary, and gaps between them
    assert 200 <= len(blocks) < nb and {0, nb - 1} <= blocks
    for lo in (0, 1024, 2048):
        assert any(lo <= b < lo + 1024 for b in blocks)


@pytest.mark.parametrize("codec", [ob.SNAPPY, ob.ZSTD])
def test_many_blocks_reference_is_a_dict_lookup(codec):
    dict_lookup(getgen.kv_set("random"), list(getgen.query_set("random", 64)), getgen.reference("random", 64, codec))


def test_row_counts_at_the_fused_kernels_limit():
    a = getgen.block_rows(getref.RefSst(getgen.rows_2048_sst()))
    b = getgen.block_rows(getref.RefSst(getgen.rows_2049_sst()))
    assert a == [2048, 2046, 2047, 2048, 209] and max(a) == 2048
    assert b == [2049, 2047, 2047, 2048, 207] and max(b) == 2049 and [i for i, n in enumerate(b) if n > 2048] == [0]
    q = list(getgen.row_boundary_queries())
    kvs = [(k, None) for k in getgen.kvs_tombstones()]
    for sst in (getgen.rows_2048_sst(), getgen.rows_2049_sst()):
        s = getref.RefSst(sst)
        ref = getgen.ref_of([s], q)
        dict_lookup(kvs, q, ref)
        lasts = getgen.block_last_keys(s)
        assert all(k in q for k in s.first_keys) and all(k in q and k + b"\x00" in q for k in lasts)
        # no lookup walks into block 0, and those that start there read no other block
        seek0 = [k for k in q if s.may_include(k) is None and ob.index_seek(s.first_keys, k) == 0]
        assert len(seek0) >= 20
        assert all(r["block"] == 0 and r["stage"] == getref.AT_ROW for r in getgen.ref_of([s], seek0)[0])
        assert getgen.ref_of([s], seek0)[3] == {(0, 0)}
        assert sum(1 for r in ref[0] if r["outcome"] == getref.TOMBSTONE and r["block"] == 0) >= 20
    assert sum(1 for k in q if len(k) in (2, 3)) >= 2000


@pytest.mark.parametrize("waves", [16 * 32, 16 * 256, 16 * 304])
def test_stride_queries_outnumber_the_grid(waves):
    """The located count is computed from the grid's wave count, whatever the device's is."""
    q, located = getgen.stride_queries(waves)
    s = getref.RefSst(getgen.stride_sst(ob.NONE))
    assert s.filter is None and s.info["filter_len"] == 0
    ref = getgen.ref_of([s], q)
    by_ref = sum(1 for r in ref[0] if r["stage"] >= getref.AT_END)
    assert by_ref == located and located > 2 * waves and located % waves not in (0, waves - 1)
    rs = ref[0]
    assert sum(1 for r in rs if r["err"] == 2 and r["stage"] == getref.AT_ERROR) >= 20  # stale CRC
    assert sum(1 for r in rs if r["stage"] == getref.AT_END) >= 5  # past the last key
    assert sum(1 for r in rs if r["outcome"] == getref.TOMBSTONE) >= 20
    assert sum(1 for r in rs if r["outcome"] == getref.VALUE) >= 100
    assert sum(1 for k, r in zip(q, rs) if r["stage"] == getref.AT_ROW and
               r["block"] == ob.index_seek(s.first_keys, k) + 1) >= 20  # walked to block + 1
    assert sum(1 for r in rs if r["stage"] == getref.AT_RANGE) >= 1


@pytest.mark.parametrize("where", ["encoded", "decoded"])
@pytest.mark.parametrize("codec", getgen.CODECS)
def test_mutated_ssts_hold_errors(codec, where):
    q = list(getgen.query_set("random", 512))
    ref = getgen.ref_of([getgen.mutated_sst(codec, where)], q)
    assert sum(1 for r in ref[0] if r["err"]) >= 20
    if where == "decoded":
        # the frame is sound: no error is a decompressor's (10-18 Snappy / LZ4, 50-61 Zlib / Zstd),
        # all are block.Decode's (1-8), a row's (20-29) or the seek's (62-64)
        errs = {r["err"] for r in ref[0]} - {0}
        assert all(e <= 8 or 20 <= e <= 29 or 62 <= e <= 64 for e in errs), errs
        assert len(errs) >= 2
