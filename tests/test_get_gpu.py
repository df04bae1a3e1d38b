"""GPU parity of the batched point reads (slate_sst_open / slate_sst_get_batch) with the
reference composed from the oracle (tests/getref.py): every field of every result, the value
offsets and the value bytes, on clean SSTs of the five codecs and on SSTs with a missing or
corrupt filter, a corrupt index, corrupt blocks (every codec) and rows, an inverted block range,
a block with more rows than the fused kernel takes, several handles in precedence order, and the
capacity protocol; the counters as conditions on the paths taken."""
import random
import struct

import numpy as np
import pytest

from oracle import binding as ob
from tests import getgen, getref, sstgen

pytestmark = pytest.mark.gpu

E_BLOCK_CHECKSUM, E_ROW_VALUE, E_FILTER_CHECKSUM, E_INDEX_CHECKSUM, E_BLOB_RANGE = 2, 26, 31, 41, 45


@pytest.fixture(scope="module")
def ctx():
    import slatecodec as sc
    return sc.Context(0)


check = getgen.check  # (shared with tests/test_get_shapes_gpu.py)


ref_of = getgen.ref_of


@pytest.mark.parametrize("codec", getgen.CODECS)
@pytest.mark.parametrize("name,block_size", [("random", 512), ("random", 4096)])
def test_clean_sst(ctx, name, block_size, codec):
    sst = getgen.clean_sst(name, block_size, codec)
    keys = list(getgen.query_set(name, block_size))
    ref = getgen.reference(name, block_size, codec)
    h = ctx.open_sst(sst)
    inf = h.info()
    assert inf["codec"] == codec and inf["filter_present"] == 1 and inf["filter_status"] == 0
    assert inf["n_blocks"] == len(getgen.blocks_of(sst)[1]) and 15 <= inf["n_blocks"] <= 400
    assert inf["first_key"] == getgen.kv_set(name)[0][0]
    assert inf["device_bytes"] >= sum(len(b) for b in getgen.blocks_of(sst)[2])
    check(ctx, [h], keys, ref)
    # n == 0 and n == 1
    res, vals, val_off = ctx.get([h], [])
    assert len(res) == 0 and list(val_off) == [0] and vals.size == 0
    present = next(i for i, r in enumerate(ref[0]) if r["outcome"] == getref.VALUE)
    one = ([ref[0][present]], np.array([0, ref[0][present]["value_len"]], np.uint64), ref[0][present]["value"])
    check(ctx, [h], [keys[present]], one)
    h.close()


@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY])
def test_counters_on_clean_ssts(ctx, codec):
    """Conditions, not measurements: the clean CodecNone SST stays on the fused kernel, and the
    general path decodes no block twice."""
    sst = getgen.clean_sst("synthetic", 4096, codec)
    keys = list(getgen.query_set("synthetic", 4096))
    ref = getgen.reference("synthetic", 4096, codec)
    h = ctx.open_sst(sst)
    ctx.get_counters(reset=True)
    check(ctx, [h], keys, ref, one_call=True)
    c = ctx.get_counters(reset=True)
    located = sum(1 for r in ref[0] if r["stage"] >= getref.AT_END)
    if codec == ob.NONE:
        assert c["n_general"] == 0 and c["n_blocks_decoded"] == 0 and 1 <= c["n_rounds"] <= 2
        assert c["n_fused"] == located
    else:
        assert c["n_fused"] == 0 and c["n_general"] == located
        assert 1 <= c["n_blocks_decoded"] <= len(ref[3])
        assert 1 <= c["n_rounds"] <= 2
    h.close()


@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY])
def test_sst_without_filter(ctx, codec):
    n = len(getgen.kv_set("random"))
    sst = getgen.clean_sst("random", 4096, codec, 10, n + 1)
    keys = list(getgen.query_set("random", 4096))
    h = ctx.open_sst(sst)
    inf = h.info()
    assert inf["filter_present"] == 0 and inf["filter_status"] == 0 and inf["filter_len"] == 0
    ref = ref_of([sst], keys)
    assert not any(r["stage"] == getref.AT_FILTER for r in ref[0])
    check(ctx, [h], keys, ref)
    h.close()


@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY])
def test_filter_with_stale_crc_means_may_include(ctx, codec):
    clean = getgen.clean_sst("random", 4096, codec)
    sst = getgen.rebuild(clean, filt=getgen.stale_crc(getgen.blocks_of(clean)[3]))
    keys = list(getgen.query_set("random", 4096))
    h = ctx.open_sst(sst)
    inf = h.info()
    assert inf["filter_present"] == 0 and inf["filter_status"] == E_FILTER_CHECKSUM
    ref = ref_of([sst], keys)
    assert not any(r["stage"] == getref.AT_FILTER for r in ref[0])
    check(ctx, [h], keys, ref)
    h.close()


def test_index_with_stale_crc_fails_open(ctx):
    import slatecodec as sc
    clean = getgen.clean_sst("random", 4096, ob.NONE)
    info = getgen.blocks_of(clean)[0]
    index = clean[info["index_offset"]:info["index_offset"] + info["index_len"]]
    sst = getgen.rebuild(clean, index_bytes=getgen.stale_crc(index))
    assert getref.RefSst(sst).open_status == E_INDEX_CHECKSUM
    with pytest.raises(sc.SlateError) as e:
        ctx.open_sst(sst)
    assert e.value.status == E_INDEX_CHECKSUM


@pytest.mark.parametrize("codec", getgen.CODECS)
def test_stale_block_crc_is_a_miss(ctx, codec):
    clean = getgen.clean_sst("random", 4096, codec)
    blocks = list(getgen.blocks_of(clean)[2])
    for b in range(3, len(blocks), 7):
        blocks[b] = getgen.stale_crc(blocks[b])
    sst = getgen.rebuild(clean, blocks=blocks)
    keys = list(getgen.query_set("random", 4096))
    ref = ref_of([sst], keys)
    hit = [r for r in ref[0] if r["err"] == E_BLOCK_CHECKSUM]
    assert len(hit) >= 20 and all(r["outcome"] == getref.MISS and r["stage"] == getref.AT_ERROR for r in hit)
    h = ctx.open_sst(sst)
    check(ctx, [h], keys, ref)
    h.close()


@pytest.mark.parametrize("codec", getgen.CODECS)
def test_mutated_blocks(ctx, codec):
    """bg.mutate with the CRC fixed in a tenth of the blocks: flipped bits, truncation, planted
    BE16 values, trailing bytes -- block.Decode errors, seek errors, row errors and panics.  The
    encoded bytes are mutated: under a compressing codec mostly the decompressor's errors."""
    sst = getgen.mutated_sst(codec, "encoded")
    keys = list(getgen.query_set("random", 512))
    ref = ref_of([sst], keys)
    assert sum(1 for r in ref[0] if r["err"]) >= 20
    h = ctx.open_sst(sst)
    check(ctx, [h], keys, ref)
    h.close()


@pytest.mark.parametrize("codec", getgen.CODECS[1:])
def test_mutated_blocks_under_a_valid_frame(ctx, codec):
    """The same mutations made to the decoded block, which is then compressed and sealed with its
    CRC: the decompressor succeeds, and block.Decode, the seek and the row decode meet the damage
    on every codec's general path."""
    sst = getgen.mutated_sst(codec, "decoded")
    keys = list(getgen.query_set("random", 512))
    ref = ref_of([sst], keys)
    assert sum(1 for r in ref[0] if r["err"]) >= 20
    h = ctx.open_sst(sst)
    check(ctx, [h], keys, ref)
    h.close()


def _break_value_len(data: bytes, offs: list[int], row: int, first_len: int) -> bytes:
    """The row's value length set to 0xFFFFFFFF: v0RowCodec.Decode fails with "too short for value"."""
    r = ob.v0_decode(data[offs[row]:], first_len)
    assert r.status == 0 and not r.tombstone and r.expire_ms is None and r.create_ms is None
    at = offs[row] + 4 + len(r.key_suffix) + 9
    return data[:at] + b"\xff\xff\xff\xff" + data[at + 4:]


@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY])
def test_two_consecutive_corrupt_rows_chain_two_spills(ctx, codec):
    clean = getgen.clean_sst("random", 512, codec)
    s = getref.RefSst(clean)
    blocks = list(getgen.blocks_of(clean)[2])
    probes = []
    done = 0
    b = 2
    while done < 6 and b + 2 < len(blocks):
        _, d0, o0 = s.block(b)
        _, d1, o1 = s.block(b + 1)
        fk0 = ob.v0_decode(d0[o0[0]:], None)
        last = ob.v0_decode(d0[o0[-1]:], len(fk0.key_suffix))
        first1 = ob.v0_decode(d1[o1[0]:], None)
        if last.tombstone or first1.tombstone or len(o0) < 2:
            b += 1
            continue
        # the last row of block b and row 0 of block b + 1: a query for block b's last key reads
        # block b (row fails), block b + 1 (its row 0 fails) and ends on block b + 2's row 0
        blocks[b] = ob.block_encode(_break_value_len(d0, o0, len(o0) - 1, len(fk0.key_suffix)), o0, codec)[1]
        blocks[b + 1] = ob.block_encode(_break_value_len(d1, o1, 0, 0), o1, codec)[1]
        probes.append((fk0.key_suffix[:last.key_prefix_len] + last.key_suffix, b + 2))
        done += 1
        b += 4
    assert done >= 4
    sst = getgen.rebuild(clean, blocks=blocks)
    keys = list(getgen.query_set("random", 512))[: getgen.N_QUERIES - 64] + [probes[i % len(probes)][0] for i in range(64)]
    ref = ref_of([sst], keys)
    for k, r in zip(keys[-len(probes):], ref[0][-len(probes):]):
        want = dict(probes)[k]
        assert (r["outcome"], r["stage"], r["err"], r["block"], r["row"]) == (getref.MISS, getref.AT_ROW, E_ROW_VALUE,
                                                                               want, 0), (k, r)
    h = ctx.open_sst(sst)
    ctx.get_counters(reset=True)
    check(ctx, [h], keys, ref, one_call=True)
    assert ctx.get_counters()["n_rounds"] >= (1 if codec == ob.NONE else 3)
    h.close()


@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY])
def test_inverted_block_range(ctx, codec):
    clean = getgen.clean_sst("random", 4096, codec)

    def swap(offs):
        offs = list(offs)
        for k in (4, 11):
            offs[k], offs[k + 1] = offs[k + 1], offs[k]
        return offs

    sst = getgen.rebuild(clean, offsets=swap)
    keys = list(getgen.query_set("random", 4096))
    ref = ref_of([sst], keys)
    hit = [r for r in ref[0] if r["err"] == E_BLOB_RANGE]
    assert len(hit) >= 20 and all(r["outcome"] == getref.MISS and r["stage"] == getref.AT_ERROR for r in hit)
    h = ctx.open_sst(sst)
    check(ctx, [h], keys, ref)
    h.close()


def test_block_with_more_rows_than_the_fused_kernel_takes(ctx):
    """Tombstones under 2-byte keys: 15-byte rows, ~3 500 of them in a block -- past the 2 048
    rows the fused kernel's seek holds, so those queries take the general path."""
    rng = random.Random(5)
    ks = sorted({bytes([rng.randrange(256), rng.randrange(256)]) for _ in range(9000)})
    sst = sstgen.none_sst([(k, None) for k in ks], 60000, 0, 10)
    s = getref.RefSst(sst)
    assert max(len(s.block(b)[2]) for b in range(len(s.metas))) > 2048
    keys = [bytes([rng.randrange(256), rng.randrange(256)]) for _ in range(3000)]
    keys += [rng.choice(ks) + bytes([rng.randrange(256)]) for _ in range(getgen.N_QUERIES - len(keys))]
    ref = ref_of([sst], keys)
    assert sum(1 for r in ref[0] if r["outcome"] == getref.TOMBSTONE) >= 200
    h = ctx.open_sst(sst)
    ctx.get_counters(reset=True)
    check(ctx, [h], keys, ref, one_call=True)
    c = ctx.get_counters(reset=True)
    big = {b for b in range(len(s.metas)) if len(s.block(b)[2]) > 2048}
    assert big and c["n_general"] >= 1 and 1 <= c["n_blocks_decoded"] <= len(s.metas)
    assert c["n_fused"] + c["n_general"] >= sum(1 for r in ref[0] if r["stage"] >= getref.AT_END)
    h.close()


def test_three_handles_in_precedence_order(ctx):
    kvs = list(getgen.kv_set("random"))
    rng = random.Random(77)
    parts = [[], [], []]
    for i, (k, v) in enumerate(kvs):
        for j in range(3):
            if rng.random() < 0.5:
                # handle j's own version of the key; handle 0 deletes some keys the others hold
                val = None if (j == 0 and rng.random() < 0.3) else bytes([j]) + (v or b"x")
                parts[j].append((k, val))
    ssts = [sstgen.none_sst(p, 4096, 0, 10) for p in parts]
    ssts[1] = sstgen.recode(ssts[1], ob.SNAPPY, random.Random(1))
    # a stale block CRC in handle 0: its keys are a miss there (err_sst 0) and go on to handle 1
    blocks = list(getgen.blocks_of(ssts[0])[2])
    blocks[2] = getgen.stale_crc(blocks[2])
    ssts[0] = getgen.rebuild(ssts[0], blocks=blocks)
    keys = list(getgen.query_set("random", 4096))
    ref = ref_of(ssts, keys)
    rs = ref[0]
    d = [dict(p) for p in parts]
    assert sum(1 for k, r in zip(keys, rs) if r["outcome"] == getref.TOMBSTONE and r["sst"] == 0 and
               d[1].get(k) is not None) >= 20
    for j in range(3):
        assert sum(1 for r in rs if r["outcome"] == getref.VALUE and r["sst"] == j) >= 20
    assert sum(1 for r in rs if r["err"] == E_BLOCK_CHECKSUM and r["err_sst"] == 0 and r["sst"] in (1, 2)) >= 1
    assert sum(1 for r in rs if r["outcome"] == getref.MISS and r["sst"] == 3) >= 20
    hs = [ctx.open_sst(s) for s in ssts]
    check(ctx, hs, keys, ref)
    for h in hs:
        h.close()


def test_capacity_protocol(ctx):
    import slatecodec as sc
    sst = getgen.clean_sst("random", 4096, ob.NONE)
    keys = list(getgen.query_set("random", 4096))
    rs, ref_off, ref_vals, _ = getgen.reference("random", 4096, ob.NONE)
    h = ctx.open_sst(sst)
    total = int(ref_off[-1])
    for cap in (0, None, total - 1):
        st, res, vals, val_off = ctx.get_into([h], keys, cap)
        assert st == sc.E_CAPACITY
        assert np.array_equal(val_off, ref_off)
        assert np.array_equal(res["value_len"], np.array([r["value_len"] for r in rs]))
        assert not vals.any()
    st, res, vals, val_off = ctx.get_into([h], keys, total)
    assert st == sc.OK and vals.tobytes() == ref_vals and np.array_equal(val_off, ref_off)
    h.close()
