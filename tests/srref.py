"""Reference for the batched point reads over sorted runs (test infrastructure): DB.GetWithOptions'
SST part (slatedb/db.go:237-265) for one key -- the L0 SSTs as tests/getref.py has them, then the
runs of Core.Compacted in list order, composed from the oracle's pieces as Go composes them:

  srMayIncludeKey (db.go:303-315)        SortedRun.SstWithKey: sort.Search over Info.FirstKey
                                         (compacted/sortedrun.go:24-41; assert.True panics on an
                                         empty first key it probes), then only that SST's filter;
                                         no RangeCoversKey
  NewSortedRunIteratorFromKey (:69-77)   sstable.NewIteratorAtKey in that SST: the index seek, then
                                         per block read, block.Decode, block.NewIteratorAtKey,
                                         blockIter.Next
  SortedRunIterator.Next (:113-145)      when an SST's iterator ends without a row (out of blocks,
                                         or a block error ended it) the next SST is iterated with
                                         sstable.NewIterator: from block 0, block.NewIterator (no
                                         seek, firstKey nil), no filter
  db.go:258-262                          the first row ends the run's part; an equal key ends the
                                         search

The result of one key is a dict with getref.FIELDS plus "run_sst", "err_run_sst" and "value";
`consulted` collects (source, sst in run, block) of the blocks the run lookups decoded (L0 blocks
as getref collects them: (sst, block)).
"""
from __future__ import annotations

import numpy as np

from oracle import binding as ob
from tests import getref
from tests.getref import AT_END, AT_ERROR, AT_FILTER, AT_RANGE, AT_ROW, E_BLOB_RANGE, MISS, PANIC, PANICS, TOMBSTONE, VALUE

E_RUN_FIRSTKEY_PANIC = 65
E_ROW_PREFIX = 21
FIELDS = getref.FIELDS + ("run_sst", "err_run_sst")


def search_first_keys(first_keys: list[bytes], key: bytes, probes: list | None = None):
    """sort.Search(len, FirstKey[i] > key) with Go's probe sequence -> (index, None), or
    (None, h) when probe h met an empty first key (the assert's panic)."""
    i, j = 0, len(first_keys)
    while i < j:
        h = (i + j) >> 1
        if probes is not None:
            probes.append(h)
        if len(first_keys[h]) == 0:
            return None, h
        if not first_keys[h] > key:
            i = h + 1
        else:
            j = h
    return i, None


def get_one(l0: list[getref.RefSst], runs: list[list[getref.RefSst]], key: bytes, consulted: set | None = None,
            trace: dict | None = None) -> dict:
    """trace (optional) counts what the lookup did: walk_on (SSTs entered from the start),
    from_start_row0 (rows returned by a from-start iterator)."""
    r = getref.get_one(l0, key, consulted)
    r.update(run_sst=0, err_run_sst=0)
    if r["outcome"] != MISS:
        return r
    r["sst"] = len(l0) + len(runs)

    for ri, run in enumerate(runs):
        src = len(l0) + ri

        def note(st, p):
            if r["err"] == 0:
                r.update(err=st, err_sst=src, err_run_sst=p)

        def panic(st, p):
            r.update(outcome=PANIC, err=st, err_sst=src, sst=src, err_run_sst=p)

        r.update(block=0, row=0, run_sst=0)
        idx, bad = search_first_keys([s.info["first_key"] for s in run], key)
        if idx is None:
            r["stage"] = AT_RANGE
            panic(E_RUN_FIRSTKEY_PANIC, bad)
            break
        if idx == 0:
            r["stage"] = AT_RANGE
            continue
        p = idx - 1
        s = run[p]
        r["run_sst"] = p
        if s.filter is not None and not ob.bloom_has_key(s.filter[0], s.filter[1], key):
            r["stage"] = AT_FILTER
            continue
        b = ob.index_seek(s.first_keys, key) if s.first_keys else 0
        from_start = False
        while True:  # SortedRunIterator.Next: one sstable.Iterator after the other
            s = run[p]
            got = False
            while True:  # iter.Next
                if b >= len(s.metas):
                    r["stage"] = AT_END
                    break
                st, data, offs = s.block(b)
                if consulted is not None and st != E_BLOB_RANGE:
                    consulted.add((src, p, b))
                start, first_idx, first_len = 0, 0, None  # block.NewIterator
                if st == 0 and not from_start:
                    (st, start, first_idx, first_len, _), _ = ob.block_seek_warnings(data, offs, key)
                if st:
                    r["stage"] = AT_ERROR
                    if st in PANICS:
                        panic(st, p)
                        got = True
                    else:
                        note(st, p)
                    break
                if start >= len(offs):
                    b += 1
                    continue
                if offs[start] > len(data):  # data[offset:] panics
                    r.update(stage=AT_ROW, block=b, row=start)
                    panic(27, p)
                    got = True
                    break
                row = ob.v0_decode(data[offs[start]:], first_len)
                if row.status == 27:
                    r.update(stage=AT_ROW, block=b, row=start)
                    panic(27, p)
                    got = True
                    break
                if row.status:
                    note(row.status, p)
                    b += 1
                    continue
                fo = offs[first_idx] + 4
                full = data[fo:fo + (first_len or 0)][:row.key_prefix_len] + row.key_suffix
                r.update(stage=AT_ROW, block=b, row=start)
                if trace is not None and from_start:
                    trace["from_start_row0"] = trace.get("from_start_row0", 0) + 1
                if full == key:
                    r["sst"] = src
                    if row.tombstone:
                        r["outcome"] = TOMBSTONE
                    else:
                        r.update(outcome=VALUE, value_len=len(row.value), value=row.value)
                got = True
                break
            r["run_sst"] = p
            if got or p + 1 >= len(run):
                break
            p, b, from_start = p + 1, 0, True
            if trace is not None:
                trace["walk_on"] = trace.get("walk_on", 0) + 1
        if r["outcome"] != MISS:
            break
    return r


def get_batch(l0, runs, keys: list[bytes], consulted: set | None = None, trace: dict | None = None):
    """-> (list of result dicts, val_off u64[n + 1], the values concatenated in query order);
    get_one is called once per distinct key."""
    memo = {}
    for k in keys:
        if k not in memo:
            memo[k] = get_one(l0, runs, k, consulted, trace)
    rs = [memo[k] for k in keys]
    val_off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        val_off[1:] = np.cumsum([r["value_len"] for r in rs], dtype=np.uint64)
    return rs, val_off, b"".join(r["value"] for r in rs)
