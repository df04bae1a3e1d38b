"""GPU parity of the batched point reads over sorted runs (slate_sorted_run_create /
slate_sst_get_batch_runs) with the reference composed from the oracle (tests/srref.py): every
field of every result, the run positions, the value offsets and the value bytes, on the runs of
tests/srgen.py; the equivalence with slate_sst_get_batch when there is no run; the ABI's
conditions; and the constant-launch claim as conditions on the counters."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as ob
from tests import getgen, getref, srgen, srref

pytestmark = pytest.mark.gpu

E_INVALID_ARG, E_CAPACITY = 102, 103


@pytest.fixture(scope="module")
def ctx():
    import slatecodec as sc
    return sc.Context(0)


def open_run(ctx, run):
    return ctx.open_run([ctx.open_sst(s) for s in run])


def compare(res, pos, vals, val_off, ref, keys):
    rs, ref_off, ref_vals = ref[:3]
    assert len(res) == len(keys) == len(pos)
    for f in srref.FIELDS:
        want = np.array([r[f] for r in rs], dtype=np.int64)
        got = (pos if f in ("run_sst", "err_run_sst") else res)[f].astype(np.int64)
        bad = np.nonzero(want != got)[0]
        assert bad.size == 0, (f, int(bad[0]), keys[int(bad[0])], rs[int(bad[0])], res[int(bad[0])], pos[int(bad[0])])
    assert np.array_equal(val_off, ref_off)
    assert vals.tobytes() == ref_vals


def check(ctx, l0, runs, keys, one_call=False):
    """One get over the encoded L0 SSTs and runs equals srref on every field."""
    ref = srgen.reference(tuple(l0), tuple(runs), tuple(keys))
    hs = [ctx.open_sst(s) for s in l0]
    rr = [open_run(ctx, r) for r in runs]
    if one_call:
        st, res, pos, vals, val_off = ctx.get_runs_into(hs, rr, list(keys), len(ref[2]))
        assert st == 0
    else:
        res, pos, vals, val_off = ctx.get_runs(hs, rr, list(keys))
    compare(res, pos, vals, val_off, ref, keys)
    return ref


@pytest.mark.parametrize("codec", srgen.CODECS)
def test_clean_run(ctx, codec):
    run = srgen.clean_run(codec)
    r = open_run(ctx, run)
    inf = r.info()
    assert inf["n_sst"] == 8 and inf["n_blocks"] == sum(len(getgen.blocks_of(s)[1]) for s in run)
    assert inf["device_bytes"] >= 4 * inf["n_blocks"]
    check(ctx, (), (run,), srgen.clean_queries())


def test_forged_run(ctx):
    check(ctx, (), (srgen.forged_run(),), srgen.forged_queries())


@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY])
@pytest.mark.parametrize("variant", srgen.DAMAGED_VARIANTS)
def test_damaged_run(ctx, codec, variant):
    check(ctx, (), (srgen.damaged_run(codec, variant),), srgen.damaged_queries())


def test_empty_first_key_run(ctx):
    check(ctx, (), (srgen.empty_first_key_run(),), srgen.empty_first_key_queries())


def test_mixed_codec_run(ctx):
    check(ctx, (), (srgen.mixed_codec_run(),), srgen.mixed_codec_queries())


def test_precedence(ctx):
    l0, runs, keys = srgen.precedence_set()
    check(ctx, l0, runs, keys)


def test_rows_2049_member_hands_over_inside_a_run(ctx):
    """A CodecNone run whose middle SST has a 2 049-row block: the fused kernel hands those queries
    to the general path, which finishes them (and walks on where the SST ends)."""
    big = getgen.rows_2049_sst()
    s = getref.RefSst(big)
    lo = [(b"\x00" + bytes([i]), b"lo%d" % i) for i in range(40)]
    hi = [(b"\xff\xff" + bytes([i]), b"hi%d" % i) for i in range(40)]
    from tests import sstgen
    run = (sstgen.none_sst(lo, 256, 0, 10), big, sstgen.none_sst(hi, 256, 0, 10))
    keys = list(getgen.row_boundary_queries())[:1500] + [k for k, _ in lo[::3]] + [k for k, _ in hi[::3]]
    keys += [getgen.block_last_keys(s)[-1] + b"\x00"]
    ctx.get_counters(reset=True)
    ref = check(ctx, (), (run,), keys, one_call=True)
    c = ctx.get_counters(reset=True)
    assert c["n_general"] >= 1 and c["n_fused"] >= 1 and c["n_blocks_decoded"] >= 1
    assert any(r["run_sst"] == 1 and r["block"] == 0 and r["stage"] == getref.AT_ROW for r in ref[0])


def test_empty_run_and_run_of_one(ctx):
    one = (getgen.clean_sst("random", 512, ob.NONE),)
    keys = list(getgen.query_set("random", 512))[:500]
    ref = check(ctx, (), ((), one), keys)
    assert sum(r["outcome"] == getref.VALUE and r["sst"] == 1 for r in ref[0]) >= 100
    ref = check(ctx, (), ((),), keys[:70])
    assert all(r["outcome"] == getref.MISS and r["sst"] == 1 and r["stage"] == getref.AT_RANGE for r in ref[0])
    check(ctx, (), (one,), [])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(ctx, n):
    for run in (srgen.clean_run(ob.NONE), srgen.mixed_codec_run()):
        check(ctx, (), (run,), srgen.mixed_codec_queries()[:n])


def test_batch_of_the_grid_stride(ctx):
    """More located queries than 2.5 fused grids: every wave takes a third query."""
    import torch
    waves = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    need = 2 * waves + waves // 2 + 37
    pool = srgen.present_queries()  # (each passes its SST's filter: every one is located)
    keys = [pool[i % len(pool)] for i in range(need)] + list(srgen.clean_queries()[:64])
    ctx.get_counters(reset=True)
    ref = check(ctx, (), (srgen.clean_run(ob.NONE),), keys, one_call=True)
    c = ctx.get_counters(reset=True)
    assert c["n_fused"] == sum(r["stage"] >= getref.AT_END for r in ref[0]) >= need
    assert c["n_general"] == 0


def test_no_run_equals_get_batch(ctx):
    """n_run = 0: res, val_off and vals byte for byte those of slate_sst_get_batch."""
    ssts, _ = getgen.five_codec_ssts()
    hs = [ctx.open_sst(s) for s in ssts]
    keys = list(getgen.query_set("random", 4096))
    st, res, vals, val_off = ctx.get_into(hs, keys, 1 << 20)
    assert st == 0
    st, res2, pos, vals2, val_off2 = ctx.get_runs_into(hs, [], keys, 1 << 20)
    assert st == 0
    total = int(val_off[len(keys)])
    assert total > 0 and res.tobytes() == res2.tobytes() and val_off.tobytes() == val_off2.tobytes()
    assert vals[:total].tobytes() == vals2[:total].tobytes()
    assert not pos["run_sst"].any() and not pos["err_run_sst"].any()
    compare(res2, pos, vals2[:total], val_off2, srgen.reference(tuple(ssts), (), tuple(keys)), keys)


def test_abi_conditions(ctx):
    run = srgen.clean_run(ob.SNAPPY)
    keys = list(srgen.clean_queries())
    ref = srgen.reference((), (run,), tuple(keys))
    r = open_run(ctx, run)
    total = len(ref[2])
    # pos = NULL
    st, res, pos, vals, val_off = ctx.get_runs_into([], [r], keys, total, want_pos=False)
    assert st == 0 and pos is None and vals.tobytes() == ref[2]
    for f in getref.FIELDS:
        assert np.array_equal(res[f].astype(np.int64), np.array([x[f] for x in ref[0]], dtype=np.int64)), f
    # the capacity protocol
    for cap in (total - 1, 0, None):
        st, res, pos, vals, val_off = ctx.get_runs_into([], [r], keys, cap)
        assert st == E_CAPACITY and int(val_off[len(keys)]) == total and np.array_equal(val_off, ref[1])
    st, res, pos, vals, val_off = ctx.get_runs_into([], [r], keys, int(val_off[len(keys)]))
    assert st == 0
    compare(res, pos, vals, val_off, ref, keys)
    # a NULL run pointer
    st = ctx.get_runs_into([], [r, None], keys, total)[0]
    assert st == E_INVALID_ARG
    import slatecodec as sc
    assert sc.status_string(65) == "Assertion Failed: sst must have first key"


def test_constant_launches_fused(ctx):
    """64 CodecNone SSTs, present keys: one fused round for the whole run, every query in it."""
    run = srgen.many_sst_run(ob.NONE)
    keys = srgen.present_queries()
    ctx.get_counters(reset=True)
    check(ctx, (), (run,), keys, one_call=True)
    c = ctx.get_counters(reset=True)
    assert c["n_rounds"] == 1 and c["n_fused"] == len(keys)
    assert c["n_general"] == 0 and c["n_blocks_decoded"] == 0


def test_constant_launches_general(ctx):
    """64 Snappy SSTs, present keys: one decode round for the whole run, each consulted block once."""
    run = srgen.many_sst_run(ob.SNAPPY)
    keys = srgen.present_queries()
    ctx.get_counters(reset=True)
    ref = check(ctx, (), (run,), keys, one_call=True)
    c = ctx.get_counters(reset=True)
    assert c["n_rounds"] == 1 and c["n_blocks_decoded"] == len(ref[3]) > 64
    assert c["n_fused"] == 0 and c["n_general"] == len(keys)
