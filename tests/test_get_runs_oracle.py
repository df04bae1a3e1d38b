"""The sorted-run reference (tests/srref.py) against the pieces it is composed from, and the
promises of the generators in tests/srgen.py, counted on the CPU: what the GPU tests compare with
is only worth something if these sets really hold the cases they name."""
import bisect
import random

import pytest

from oracle import binding as ob
from tests import getgen, getref, srgen, srref
from tests.getref import AT_END, AT_ERROR, AT_FILTER, AT_RANGE, AT_ROW, MISS, PANIC, TOMBSTONE, VALUE


def test_no_runs_equals_getref():
    ssts, _ = getgen.five_codec_ssts()
    refs = [getref.RefSst(s) for s in ssts]
    keys = list(getgen.query_set("random", 4096))[:600]
    for k in keys:
        want = getref.get_one(refs, k)
        got = srref.get_one(refs, [], k)
        assert got["run_sst"] == 0 and got["err_run_sst"] == 0
        for f in getref.FIELDS + ("value",):
            assert got[f] == want[f], (f, k)


def test_run_firstkey_panic_status():
    """Status 65 of the ABI: its string, and that the oracle (which restates no sorted run) has none."""
    import slatecodec as sc
    assert sc.E_RUN_FIRSTKEY_PANIC == srref.E_RUN_FIRSTKEY_PANIC == 65
    assert sc.status_string(65) == "Assertion Failed: sst must have first key"
    assert ob.status_string(65) == "unknown status"


def test_search_equals_bisect_right():
    rng = random.Random(3)
    for n in (0, 1, 2, 3, 5, 8, 64, 65):
        fks = sorted({bytes(rng.randrange(256) for _ in range(rng.randint(1, 4))) for _ in range(n)})
        for key in [b"", b"\xff" * 5] + fks + [k + b"\x00" for k in fks] + [k[:-1] for k in fks]:
            assert srref.search_first_keys(fks, key) == (bisect.bisect_right(fks, key), None)


def test_search_probe_set_with_empty_first_key():
    """Over five SSTs only a key below SST 1's first key probes index 0."""
    fks = [b"", b"b", b"d", b"f", b"h"]
    for key, panics in ((b"a", True), (b"", True), (b"b", False), (b"c", False), (b"e", False), (b"z", False)):
        probes = []
        idx, bad = srref.search_first_keys(fks, key, probes)
        assert (0 in probes) == panics and (idx is None) == panics
        if panics:
            assert bad == 0


@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY])
def test_clean_run_equals_one_sst(codec):
    """A present key's result over the run equals its result over one SST of all the KVs."""
    run = srgen.clean_run(codec)
    keys = srgen.clean_queries()
    rs = srgen.reference((), (run,), keys)[0]
    one = getref.RefSst(getgen.clean_sst("random", 256, codec))
    kvd = dict(getgen.kv_set("random"))
    n = 0
    for k, r in zip(keys, rs):
        if k in kvd:
            w = getref.get_one([one], k)
            assert (r["outcome"], r["value"]) == (w["outcome"], w["value"]), k
            assert r["outcome"] == (TOMBSTONE if kvd[k] is None else VALUE)
            n += 1
    assert n >= 400


def test_clean_queries_hold_what_they_promise():
    run = srgen.clean_run(ob.NONE)
    keys = srgen.clean_queries()
    assert 900 <= len(keys) <= 1100 and len(run) == 8
    rs, _, _, consulted, trace = srgen.reference((), (run,), keys)
    refs = srgen.refs(run)
    assert all(2 <= len(s.metas) for s in refs)
    firsts = [s.info["first_key"] for s in refs]
    lasts = [srgen.last_key(s) for s in run]
    kvd = dict(getgen.kv_set("random"))
    assert b"" in keys and set(firsts) <= set(keys) and set(lasts) <= set(keys)
    assert sum(k < firsts[0] for k in keys) >= 3 and sum(k > lasts[-1] for k in keys) >= 8
    assert len(set(keys)) < len(keys)
    assert sum(r["outcome"] == TOMBSTONE for r in rs) >= 30
    assert sum(r["stage"] == AT_RANGE for r in rs) >= 3
    assert sum(r["stage"] == AT_FILTER for r in rs) >= 50
    # absent keys the 2-bit filter let through
    assert sum(k not in kvd and r["stage"] == AT_ROW for k, r in zip(keys, rs)) >= 50
    # keys between two SSTs that walked off SST p into SST p + 1's row 0
    walked = [r for k, r in zip(keys, rs)
              if any(lo < k < hi for lo, hi in zip(lasts[:-1], firsts[1:])) and r["stage"] == AT_ROW]
    assert len(walked) >= 5 and all(r["block"] == 0 and r["row"] == 0 and r["run_sst"] >= 1 for r in walked)
    assert trace["walk_on"] >= 5 and trace["from_start_row0"] >= 5
    # past the run's last key: the run ends first
    assert sum(r["stage"] == AT_END and r["run_sst"] == 7 for r in rs) >= 1
    # every SST's first key is found in that SST
    for p, fk in enumerate(firsts):
        r = rs[keys.index(fk)]
        assert r["run_sst"] == p and r["stage"] == AT_ROW and r["outcome"] in (VALUE, TOMBSTONE)


def test_forged_run_returns_row0_from_start():
    run = srgen.forged_run()
    keys = srgen.forged_queries()
    rs, _, _, _, trace = srgen.reference((), (run,), keys)
    b = getref.RefSst(run[1])
    b0 = b.first_keys[0]
    in_b = [(k, r) for k, r in zip(keys, rs) if k >= b0]
    assert len(in_b) >= 500
    # an implementation that seeks in B would find these keys; Go returns B's row 0 and misses
    for k, r in in_b:
        assert (r["stage"], r["run_sst"], r["block"], r["row"]) == (AT_ROW, 1, 0, 0), k
        assert r["outcome"] == (VALUE if k == b0 else MISS)
    assert sum(k == b0 for k, _ in in_b) == 1
    assert sum(getref.get_one([b], k)["outcome"] != MISS for k, _ in in_b if k != b0) == 0  # (forged: out of range)
    assert trace["from_start_row0"] >= 500
    assert sum(r["outcome"] in (VALUE, TOMBSTONE) and r["run_sst"] == 0 for r in rs) >= 50


@pytest.mark.parametrize("codec", [ob.NONE, ob.SNAPPY])
@pytest.mark.parametrize("variant", srgen.DAMAGED_VARIANTS)
def test_damaged_run_holds_what_it_promises(codec, variant):
    run = srgen.damaged_run(codec, variant)
    keys = srgen.damaged_queries()
    rs, _, _, consulted, trace = srgen.reference((), (run,), keys)
    refs = srgen.refs(run)
    # (a): keys of SST 1's last block meet its CRC and walk on
    a = [r for r in rs if r["err"] == srgen.E_BLOCK_CHECKSUM and r["err_run_sst"] == 1]
    assert len(a) >= 5
    # (c): the walk passes SST 3's block 0 (row 0 rejected) and takes block 1's row 0
    c = [r for r in a if (r["stage"], r["run_sst"], r["block"], r["row"]) == (AT_ROW, 3, 1, 0)]
    assert len(c) >= 5
    assert (3, 0) in {(p, b) for _, p, b in consulted} and refs[3].block(0)[0] == 0
    if variant in (0, 2):  # (b)
        assert sum(r["err"] == srgen.E_BLOCK_CHECKSUM and r["err_run_sst"] == 2 for r in rs) >= 5
    if variant == 1:  # (d): SST 2 has no block, its keys walk on to SST 3
        assert len(refs[2].metas) == 0
        assert sum(r["err"] == srref.E_ROW_PREFIX and r["err_run_sst"] == 3 and r["run_sst"] == 3 for r in rs) >= 50
    if variant == 2:  # (e)
        assert sum(r["stage"] == AT_ERROR and r["run_sst"] == 4 for r in rs) >= 2  # (the last block is short)
    else:
        assert sum(r["stage"] == AT_END and r["run_sst"] == 4 for r in rs) >= 1
    assert not any(r["outcome"] == PANIC for r in rs)
    assert trace["walk_on"] >= 10


def test_empty_first_key_run_panics_only_below_a():
    run = srgen.empty_first_key_run()
    keys = srgen.empty_first_key_queries()
    rs = srgen.reference((), (run,), keys)[0]
    a_first = getref.RefSst(run[1]).info["first_key"]
    assert getref.RefSst(run[0]).info["first_key"] == b""
    pan = [(k, r) for k, r in zip(keys, rs) if r["outcome"] == PANIC]
    rest = [(k, r) for k, r in zip(keys, rs) if r["outcome"] != PANIC]
    assert len(pan) >= 50 and len(rest) >= 300
    for k, r in pan:
        assert k < a_first and (r["err"], r["stage"], r["sst"], r["err_sst"], r["err_run_sst"]) == (65, AT_RANGE, 0, 0, 0)
    assert all(k >= a_first for k, _ in rest)
    assert sum(r["outcome"] == VALUE for _, r in rest) >= 200


def test_mixed_codec_run_walks_from_none_into_snappy():
    run = srgen.mixed_codec_run()
    assert [getref.RefSst(s).codec for s in run] == list(srgen.CODECS)
    keys = srgen.mixed_codec_queries()
    rs = srgen.reference((), (run,), keys)[0]
    for p in range(4):
        assert sum(r["err_run_sst"] == p and r["err"] == srgen.E_BLOCK_CHECKSUM and r["run_sst"] == p + 1
                   and r["stage"] == AT_ROW for r in rs) >= 3, p
    assert sum(r["outcome"] == VALUE for r in rs) >= 500


def test_many_sst_run_shape():
    for codec in (ob.NONE, ob.SNAPPY):
        run = srgen.many_sst_run(codec)
        assert len(run) == 64
    keys = srgen.present_queries()
    rs, _, _, consulted, _ = srgen.reference((), (srgen.many_sst_run(ob.SNAPPY),), keys)
    assert all(r["outcome"] in (VALUE, TOMBSTONE) for r in rs)
    assert len({p for _, p, _ in consulted}) == 64 and len(consulted) > 64


def test_precedence_set_holds_what_it_promises():
    l0, runs, keys = srgen.precedence_set()
    rs = srgen.reference(l0, runs, keys)[0]
    r1 = srgen.reference((), (runs[1],), keys)[0]
    r0 = srgen.reference((), (runs[0],), keys)[0]
    # an L0 tombstone hides a run's value
    assert sum(a["outcome"] == TOMBSTONE and a["sst"] == 0 and b["outcome"] == VALUE for a, b in zip(rs, r1)) >= 100
    # a tombstone in run 0 hides a value in run 1
    assert sum(a["outcome"] == TOMBSTONE and a["sst"] == 2 and b["outcome"] == VALUE for a, b in zip(rs, r1)) >= 100
    # present only in run 1
    assert sum(a["outcome"] == VALUE and a["sst"] == 3 and a["value"][:2] == b"r1" and c["outcome"] == MISS
               for a, c in zip(rs, r0)) >= 300
    assert sum(a["outcome"] == VALUE and a["sst"] == 1 for a in rs) >= 100
    assert sum(a["outcome"] == VALUE and a["sst"] == 2 for a in rs) >= 100
    assert sum(a["outcome"] == MISS and a["sst"] == 4 for a in rs) >= 2
