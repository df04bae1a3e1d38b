"""Reference for the batched point reads (test infrastructure): DB.GetWithOptions' SST part
(slatedb/db.go:237-250) for one key over encoded SSTs in precedence order, composed from the
oracle's pieces exactly as Go composes them:

  sstMayIncludeKey (db.go:291-301)     RangeCoversKey (table.go:89-94), ReadFilter (decode.go:50-71)
                                       + Filter.HasKey; an absent or undecodable filter = may include
  NewIteratorAtKey (iterator.go:43-57) ReadIndex, firstBlockIncludingOrAfterKey
  iter.Next (iterator.go:59-89)        per block: the range read (decode.go:93-103, blob.go:23-26),
                                       block.Decode, block.NewIteratorAtKey, blockIter.Next
                                       (block/iterator.go:84-107) -- a block error ends the iteration,
                                       a row past the end or a row that fails to decode goes on to
                                       the next block
  db.go:245-248                        a row with the key ends the search (value or tombstone)

The result of one key is a dict with slate_get_result's fields plus "value"; `consulted` collects
the (sst, block) pairs whose decode the lookups needed.
"""
from __future__ import annotations

import struct

import numpy as np

from oracle import binding as ob

MISS, VALUE, TOMBSTONE, PANIC = 0, 1, 2, 3
AT_RANGE, AT_FILTER, AT_END, AT_ERROR, AT_ROW = 0, 1, 2, 3, 4
E_BLOB_RANGE = 45
PANICS = (7, 27, 64)
FIELDS = ("outcome", "stage", "err", "sst", "err_sst", "block", "row", "value_len")


MAX_DECODE_CAP = 1 << 24


def decode_cap(enc: bytes, codec: int) -> int:
    """Room for block.Decode's output, sized from the block itself as the decode plan sizes it (the
    frame's own length: Snappy's prefix, the LZ4 / Zstd frame walk, Zlib's stream length), never
    less than ob.block_decode's default of 24 x the encoded length -- so a block that compresses
    better than 24:1 decodes instead of failing for room (Go's decoders grow their output).  A
    corrupt block may claim any length; past MAX_DECODE_CAP the claim is not followed."""
    cap = max(len(enc) * 24, 64)
    if len(enc) >= 6:
        h, p = ob._buf(enc)
        dl = ob.C.c_uint64(0)
        ob.lib().or_decompress_len(codec, p, len(enc) - 4, ob.C.byref(dl))
        if cap < dl.value + 16 <= MAX_DECODE_CAP:
            cap = dl.value + 16
    return cap


class RefSst:
    """What slate_sst_open reads of one encoded SST (open_status != 0: no handle is made)."""

    def __init__(self, sst: bytes):
        self.sst = sst
        self.blocks = {}
        self.open_status, self.info = ob.sst_read_info(sst)
        if self.open_status:
            return
        i = self.info
        self.codec = i["codec"]
        if i["index_offset"] > len(sst) or i["index_offset"] + i["index_len"] > len(sst):
            self.open_status = E_BLOB_RANGE
            return
        self.open_status, self.metas = ob.decode_index(sst[i["index_offset"]:i["index_offset"] + i["index_len"]],
                                                       self.codec)
        if self.open_status:
            return
        self.first_keys = [fk for _, fk in self.metas]
        self.filter = None
        self.filter_status = 0
        if i["filter_len"] >= 1:
            if i["filter_offset"] > len(sst) or i["filter_offset"] + i["filter_len"] > len(sst):
                self.filter_status = E_BLOB_RANGE
            else:
                st, num_probes, bits = ob.bloom_decode(sst[i["filter_offset"]:i["filter_offset"] + i["filter_len"]],
                                                       self.codec)
                self.filter_status = st
                if st == 0:
                    self.filter = (num_probes, bits)

    def may_include(self, key: bytes) -> int | None:
        """None: may include; else the stage that said no."""
        fk = self.info["first_key"]
        if len(fk) == 0 or key < fk:
            return AT_RANGE
        if self.filter is not None and not ob.bloom_has_key(self.filter[0], self.filter[1], key):
            return AT_FILTER
        return None

    def block(self, b: int):
        """(status, Data, Offsets) of block b as iter.Next reads and decodes it."""
        if b not in self.blocks:
            start = self.metas[b][0]
            end = self.metas[b + 1][0] if b + 1 < len(self.metas) else self.info["filter_offset"]
            if start > len(self.sst) or end > len(self.sst) or start > end:
                self.blocks[b] = (E_BLOB_RANGE, b"", [])
            else:
                enc = self.sst[start:end]
                m, out, _ = ob.block_decode(enc, self.codec, decode_cap(enc, self.codec))
                if m["status"]:
                    self.blocks[b] = (m["status"], b"", [])
                else:
                    dl, nr = m["data_len"], m["n_rows"]
                    offs = list(struct.unpack(">%dH" % nr, out[dl:dl + 2 * nr]))
                    self.blocks[b] = (0, out[:dl], offs)
        return self.blocks[b]


def get_one(ssts: list[RefSst], key: bytes, consulted: set | None = None) -> dict:
    r = dict(outcome=MISS, stage=AT_RANGE, err=0, sst=len(ssts), err_sst=0, block=0, row=0, value_len=0, value=b"")

    def note(st, j):
        if r["err"] == 0:
            r["err"], r["err_sst"] = st, j

    def panic(st, j):
        r.update(outcome=PANIC, err=st, err_sst=j, sst=j)

    for j, s in enumerate(ssts):
        r["block"] = r["row"] = 0
        no = s.may_include(key)
        if no is not None:
            r["stage"] = no
            continue
        b = ob.index_seek(s.first_keys, key) if s.first_keys else 0
        while True:
            if b >= len(s.metas):
                r["stage"] = AT_END
                break
            st, data, offs = s.block(b)
            if consulted is not None and st != E_BLOB_RANGE:
                consulted.add((j, b))
            if st == 0:
                (st, start, first_idx, first_len, _), _ = ob.block_seek_warnings(data, offs, key)
            if st:
                r["stage"] = AT_ERROR
                if st in PANICS:
                    panic(st, j)
                else:
                    note(st, j)
                break
            if start >= len(offs):
                b += 1
                continue
            if offs[start] > len(data):  # data[offset:] panics
                r.update(stage=AT_ROW, block=b, row=start)
                panic(27, j)
                break
            row = ob.v0_decode(data[offs[start]:], first_len)
            if row.status == 27:
                r.update(stage=AT_ROW, block=b, row=start)
                panic(27, j)
                break
            if row.status:
                note(row.status, j)
                b += 1
                continue
            fo = offs[first_idx] + 4
            full = data[fo:fo + first_len][:row.key_prefix_len] + row.key_suffix
            r.update(stage=AT_ROW, block=b, row=start)
            if full == key:
                r["sst"] = j
                if row.tombstone:
                    r["outcome"] = TOMBSTONE
                else:
                    r.update(outcome=VALUE, value_len=len(row.value), value=row.value)
            break
        if r["outcome"] != MISS:
            break
    return r


def get_batch(ssts: list[RefSst], keys: list[bytes], consulted: set | None = None):
    """-> (list of result dicts, val_off u64[n + 1], the values concatenated in query order)."""
    rs = [get_one(ssts, k, consulted) for k in keys]
    val_off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        val_off[1:] = np.cumsum([r["value_len"] for r in rs], dtype=np.uint64)
    return rs, val_off, b"".join(r["value"] for r in rs)


def between_keys(s: RefSst):
    """For every b: (last key of block b, first key of block b + 1) of a clean SST."""
    out = []
    for b in range(len(s.metas) - 1):
        st, data, offs = s.block(b)
        assert st == 0
        fl = ob.v0_decode(data[offs[0]:], None)
        last = ob.v0_decode(data[offs[-1]:], len(fl.key_suffix))
        out.append((fl.key_suffix[:last.key_prefix_len] + last.key_suffix, s.first_keys[b + 1]))
    return out
