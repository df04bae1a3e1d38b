"""GPU parity of the batched point reads with the reference (tests/getref.py) at the shapes
tests/test_get_gpu.py's inputs leave out: values longer than one step of the copy kernel and the
empty value, rows that carry timestamps, batches that are no multiple of a wave or a scan tile,
more located queries than the fused kernel's grid has waves, blocks of exactly 2 048 and 2 049
rows, SSTs of more than 2 048 blocks, long keys with shared prefixes, and handle lists (none, a
handle twice, a handle without blocks, five codecs, eight ranges).  Every test compares every
field of every result, the value offsets and the value bytes (getgen.check); the generators'
promises are asserted in tests/test_get_shapes_oracle.py."""
import pytest

from oracle import binding as ob
from tests import getgen, getref

pytestmark = pytest.mark.gpu

check = getgen.check


@pytest.fixture(scope="module")
def ctx():
    import slatecodec as sc
    return sc.Context(0)


def located(ref) -> int:
    return sum(1 for r in ref[0] if r["stage"] >= getref.AT_END)


@pytest.mark.parametrize("codec", getgen.CODECS)
def test_value_lengths(ctx, codec):
    """get_copy_kernel: eight lanes per value, 16 bytes per lane, steps of 128 -- lengths around
    every multiple of 16 up to 144, around 256, 1 024, 4 097 and two past 64 KiB (one giant row
    whose Data length wraps in 16 bits), next to each other in the output."""
    keys = list(getgen.value_edges_queries())
    ref = getgen.ref_of([getgen.value_edges_sst(codec)], keys)
    kvd = dict(getgen.kvs_value_edges())
    empty = [r for k, r in zip(keys, ref[0]) if kvd.get(k) == b""]
    assert len(empty) == 9 and all(r["outcome"] == getref.VALUE and r["value_len"] == 0 for r in empty)
    assert {r["value_len"] for r in ref[0] if r["outcome"] == getref.VALUE} == set(getgen.VALUE_LENGTHS)
    h = ctx.open_sst(getgen.value_edges_sst(codec))
    res = check(ctx, [h], keys, ref)
    got_empty = [g for k, g in zip(keys, res) if kvd.get(k) == b""]
    assert all(g["outcome"] == getref.VALUE and g["value_len"] == 0 for g in got_empty)
    h.close()


@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4097, 6145])
@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY])
def test_batch_sizes(ctx, codec, n):
    """The tails of the value scan (tiles of 2 048), of wave_append (a partial last wave) and of
    the copy kernel's eight lanes per value."""
    base = list(getgen.query_set("random", 4096))
    rs = getgen.reference("random", 4096, codec)[0]
    keys = [base[i % len(base)] for i in range(n)]
    ref = getgen.expand([rs[i % len(base)] for i in range(n)])
    h = ctx.open_sst(getgen.clean_sst("random", 4096, codec))
    check(ctx, [h], keys, ref)
    h.close()


def test_fused_kernel_takes_several_queries_per_wave(ctx):
    """get_fused_kernel's stride loop: more located queries than 2.5 times the grid's waves, so
    every wave takes a second and a third query with the LDS the one before left (after a value,
    a tombstone, a miss, the end of the SST or a checksum error), and `done` adds up."""
    import torch
    waves = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    keys, _ = getgen.stride_queries(waves)
    for codec in (ob.NONE, ob.SNAPPY):
        sst = getgen.stride_sst(codec)
        ref = getgen.ref_of([sst], keys)
        n_loc = located(ref)
        assert n_loc >= 2 * waves + waves // 2 + 37 and n_loc > 2 * waves
        assert sum(1 for r in ref[0] if r["err"] == 2 and r["stage"] == getref.AT_ERROR) >= 20
        h = ctx.open_sst(sst)
        assert h.info()["filter_present"] == 0
        ctx.get_counters(reset=True)
        check(ctx, [h], keys, ref, one_call=True)
        c = ctx.get_counters(reset=True)
        if codec == ob.NONE:
            assert c["n_fused"] == n_loc and c["n_general"] == 0
        else:
            assert c["n_fused"] == 0 and c["n_general"] == n_loc
        h.close()


def test_row_count_boundary(ctx):
    """cnt16 > kSeekWaveRows: a block of 2 048 rows is the fused kernel's, one of 2 049 is handed
    to the general path -- block 0 only, and only the queries whose index seek gives block 0."""
    keys = list(getgen.row_boundary_queries())
    for sst, big in ((getgen.rows_2048_sst(), False), (getgen.rows_2049_sst(), True)):
        s = getref.RefSst(sst)
        ref = getgen.ref_of([s], keys)
        h = ctx.open_sst(sst)
        ctx.get_counters(reset=True)
        check(ctx, [h], keys, ref, one_call=True)
        c = ctx.get_counters(reset=True)
        if not big:
            assert c["n_general"] == 0 and c["n_blocks_decoded"] == 0 and c["n_fused"] == located(ref)
        else:
            in0 = sum(1 for k in keys if s.may_include(k) is None and ob.index_seek(s.first_keys, k) == 0)
            assert in0 >= 20
            assert c["n_general"] == in0 and c["n_blocks_decoded"] == 1
            assert c["n_fused"] == located(ref) - in0
        h.close()


@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY, ob.ZSTD])
def test_many_blocks(ctx, codec):
    """2 051 blocks: get_locate_kernel's search over that many first keys, get_compact_kernel with
    three blocks per thread, its clamps and its idle threads; then five blocks far apart."""
    sst = getgen.many_blocks_sst(codec)
    s = getref.RefSst(sst)
    nb = len(s.metas)
    keys = list(getgen.query_set("random", 64))
    ref = getgen.reference("random", 64, codec)
    h = ctx.open_sst(sst)
    assert h.info()["n_blocks"] == nb
    ctx.get_counters(reset=True)
    check(ctx, [h], keys, ref, one_call=True)
    c = ctx.get_counters(reset=True)
    if codec != ob.NONE:
        assert c["n_blocks_decoded"] == len(ref[3])  # every block a lookup read, once, and no other
    sparse = [s.first_keys[b] for b in (0, 1, 1024, 2049, nb - 1)]
    ref5 = getgen.ref_of([s], sparse)
    assert [r["block"] for r in ref5[0]] == [0, 1, 1024, 2049, nb - 1]
    assert all(r["outcome"] != getref.MISS for r in ref5[0])
    check(ctx, [h], sparse, ref5, one_call=True)
    c = ctx.get_counters(reset=True)
    if codec != ob.NONE:
        assert c["n_blocks_decoded"] == 5 == len(ref5[3])
    h.close()


@pytest.mark.parametrize("codec", getgen.CODECS)
def test_rows_with_timestamps(ctx, codec):
    """get_row's value address suf + sl + meta_len: 13 bytes of seq, flags and value length in a
    plain row, 8 or 16 more with an expire and / or a create timestamp."""
    sst, kinds = getgen.timestamped_sst(codec)
    keys = list(getgen.query_set("random", 512))
    ref = getgen.ref_of([sst], keys)
    for kind in getgen.TS_KINDS[1:]:
        assert sum(1 for k, r in zip(keys, ref[0]) if kinds.get(k) == kind and r["outcome"] == getref.VALUE) >= 80
    h = ctx.open_sst(sst)
    check(ctx, [h], keys, ref)
    h.close()


@pytest.mark.parametrize("codec", getgen.CODECS)
def test_long_keys_shared_prefixes(ctx, codec):
    """Keys of 8-256 bytes with long shared prefixes: the compares' length tie-break (strict
    prefixes, key + 0x00), a 1 000-byte and a 65 535-byte query."""
    keys = list(getgen.mixed_queries())
    ref = getgen.ref_of([getgen.mixed_sst(codec)], keys)
    assert sum(1 for r in ref[0] if r["outcome"] == getref.VALUE) >= 600
    h = ctx.open_sst(getgen.mixed_sst(codec))
    check(ctx, [h], keys, ref)
    h.close()


def test_handle_lists(ctx):
    keys = list(getgen.query_set("random", 4096))
    clean = getgen.clean_sst("random", 4096, ob.NONE)
    # no handle at all
    ref = getgen.ref_of([], keys)
    assert all(r == getref.get_one([], k) for k, r in zip(keys[:50], ref[0]))
    check(ctx, [], keys, ref)
    # the same handle twice: what the first does not answer the second does not either
    h = ctx.open_sst(clean)
    ref = getgen.ref_of([clean, clean], keys)
    assert {r["sst"] for r in ref[0]} == {0, 2}
    check(ctx, [h, h], keys, ref)
    # a handle with a first key and no block: AT_END, alone and in front of a normal handle
    zero = getgen.zero_block_sst()
    hz = ctx.open_sst(zero)
    assert hz.info()["n_blocks"] == 0
    ref = getgen.ref_of([zero], keys)
    assert sum(1 for r in ref[0] if r["stage"] == getref.AT_END) >= 1000
    assert all(r["outcome"] == getref.MISS for r in ref[0])
    check(ctx, [hz], keys, ref)
    ref = getgen.ref_of([zero, clean], keys)
    assert sum(1 for r in ref[0] if r["outcome"] == getref.VALUE and r["sst"] == 1) >= 1000
    check(ctx, [hz, h], keys, ref)
    hz.close()
    h.close()


def test_five_codecs_in_precedence_order(ctx):
    ssts, parts = getgen.five_codec_ssts()
    keys = list(getgen.query_set("random", 4096))
    ref = getgen.ref_of(list(ssts), keys)
    rs = ref[0]
    d = [dict(p) for p in parts]
    for j in range(5):
        assert sum(1 for r in rs if r["outcome"] != getref.MISS and r["sst"] == j) >= 20
        assert sum(1 for r in rs if r["outcome"] == getref.VALUE and r["sst"] == j) >= 20
    for j in range(2):  # a tombstone hides the value a later handle holds
        assert sum(1 for k, r in zip(keys, rs) if r["outcome"] == getref.TOMBSTONE and r["sst"] == j and
                   any(d[i].get(k) is not None for i in range(j + 1, 5))) >= 20
    assert sum(1 for r in rs if r["outcome"] == getref.MISS and r["sst"] == 5) >= 20
    hs = [ctx.open_sst(s) for s in ssts]
    assert [h.info()["codec"] for h in hs] == list(getgen.CODECS)
    check(ctx, hs, keys, ref)
    for h in hs:
        h.close()


def test_eight_handles_with_disjoint_ranges(ctx):
    ssts = getgen.eight_range_ssts()
    order = [3, 7, 0, 5, 1, 6, 2, 4]
    keys = list(getgen.query_set("random", 4096))
    ref = getgen.ref_of([ssts[j] for j in order], keys)
    rs = ref[0]
    for j in range(8):
        assert sum(1 for r in rs if r["outcome"] != getref.MISS and r["sst"] == j) >= 20
    # a query leaves most handles at the range check or the filter
    per_handle = [getgen.ref_of([ssts[j]], keys)[0] for j in order]
    for prs in per_handle:
        assert sum(1 for r in prs if r["stage"] <= getref.AT_FILTER) >= len(keys) // 2
    assert sum(1 for prs in per_handle for r in prs if r["stage"] == getref.AT_RANGE) >= 1000
    assert sum(1 for prs in per_handle for r in prs if r["stage"] == getref.AT_FILTER) >= 1000
    hs = [ctx.open_sst(ssts[j]) for j in order]
    check(ctx, hs, keys, ref)
    for h in hs:
        h.close()
