"""The point-read reference (tests/getref.py) against a plain dict lookup on clean SSTs of every
codec, and the promises of the query sets the GPU tests use (CPU only)."""
import pytest

from oracle import binding as ob
from tests import getgen, getref

SETS = [("random", 512), ("random", 4096), ("synthetic", 4096)]


@pytest.mark.parametrize("codec", getgen.CODECS)
@pytest.mark.parametrize("name,block_size", SETS[:2])
def test_getref_is_a_dict_lookup_on_clean_ssts(name, block_size, codec):
    kvd = dict(getgen.kv_set(name))
    keys = list(getgen.query_set(name, block_size))
    rs, val_off, vals, _ = getgen.reference(name, block_size, codec)
    assert int(val_off[-1]) == len(vals)
    for i, (k, r) in enumerate(zip(keys, rs)):
        got = vals[int(val_off[i]):int(val_off[i + 1])]
        if k not in kvd:
            assert r["outcome"] == getref.MISS and r["sst"] == 1 and got == b"", k
        elif kvd[k] is None:
            assert r["outcome"] == getref.TOMBSTONE and r["sst"] == 0 and got == b"", k
        else:
            assert r["outcome"] == getref.VALUE and r["sst"] == 0 and got == kvd[k], k
        assert r["err"] == 0


@pytest.mark.parametrize("name,block_size", SETS)
def test_query_sets_contain_what_they_claim(name, block_size):
    kvs = getgen.kv_set(name)
    keys = list(getgen.query_set(name, block_size))
    s = getref.RefSst(getgen.clean_sst(name, block_size, ob.NONE))
    assert s.open_status == 0 and s.filter is not None
    assert 15 <= len(s.metas) <= 400
    c = getgen.classify(s, kvs, keys)
    assert len(keys) == getgen.N_QUERIES
    for kind in ("filter_fp", "between", "past_last", "below_first", "block_first", "tombstone"):
        assert c[kind] >= 20, (kind, c)
    assert c["empty"] >= 1
    assert len(set(keys)) < len(keys)  # duplicates
    # 64 queries (or more) land on one block
    per_block = {}
    for k in keys:
        if s.may_include(k) is None:
            b = ob.index_seek(s.first_keys, k)
            per_block[b] = per_block.get(b, 0) + 1
    assert max(per_block.values()) >= 64
    # and the reference's stages cover every way a lookup ends on a clean SST
    rs, _, _, _ = getgen.reference(name, block_size, ob.NONE)
    stages = {r["stage"] for r in rs}
    assert {getref.AT_RANGE, getref.AT_FILTER, getref.AT_END, getref.AT_ROW} <= stages


def test_precedence_and_tombstones_over_handles():
    a = [(b"k1", b"a1"), (b"k2", None), (b"k5", b"a5")]
    b = [(b"k2", b"b2"), (b"k3", b"b3"), (b"k5", b"b5")]
    from tests import sstgen
    ssts = [getref.RefSst(sstgen.none_sst(x, 4096, 1 << 30)) for x in (a, b)]
    rs, val_off, vals = getref.get_batch(ssts, [b"k1", b"k2", b"k3", b"k4", b"k5"])
    assert [(r["outcome"], r["sst"]) for r in rs] == [(1, 0), (2, 0), (1, 1), (0, 2), (1, 0)]
    assert vals == b"a1b3a5" and list(val_off) == [0, 2, 2, 4, 4, 6]
