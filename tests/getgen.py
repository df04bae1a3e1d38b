"""SSTs and query sets for the batched point-read tests (test infrastructure), shared by
tests/test_get_oracle.py (which asserts the sets contain what they claim) and
tests/test_get_gpu.py.  Everything is cached: an SST, its query set and its reference results are
built once per process."""
from __future__ import annotations

import functools
import random
import struct
import zlib

from oracle import binding as ob
from tests import blockgen as bg
from tests import getref, sstgen

N_QUERIES = 4096
CODECS = (ob.NONE, ob.SNAPPY, ob.ZLIB, ob.LZ4, ob.ZSTD)


@functools.lru_cache(maxsize=None)
def kvs_random(seed: int = 11, n: int = 2200):
    """~2 000 random KVs, a tenth tombstones (value None); no key starts below 0x10, so keys
    below the SST's first key are easy to make."""
    rng = random.Random(seed)
    kvs = bg.random_kvs(rng, n, klen=(2, 24), vlen=(1, 120), tomb_p=0.1)
    return tuple((k, None if v == b"" else v) for k, v in kvs if k[0] >= 0x10)


@functools.lru_cache(maxsize=None)
def kvs_synthetic(n: int = 2000):
    return tuple((k, None if v == b"" else v) for k, v in bg.kv_synthetic(n, tomb_every=9))


def kv_set(name: str):
    return kvs_random() if name == "random" else kvs_synthetic()


@functools.lru_cache(maxsize=None)
def clean_sst(name: str, block_size: int, codec: int, bits_per_key: int = 2, min_filter_keys: int = 0) -> bytes:
    """random KVs / synthetic KVs as an SST; bits_per_key 2 makes the filter pass many absent keys."""
    none = sstgen.none_sst(list(kv_set(name)), block_size, min_filter_keys, bits_per_key)
    return none if codec == ob.NONE else sstgen.recode(none, codec, random.Random(codec))


def blocks_of(sst: bytes):
    """(info, index metas, encoded blocks, filter bytes) of a well-formed SST."""
    st, info = ob.sst_read_info(sst)
    assert st == 0
    io, il, fo, fl = info["index_offset"], info["index_len"], info["filter_offset"], info["filter_len"]
    st, metas = ob.decode_index(sst[io:io + il], info["codec"])
    assert st == 0
    blocks = [sst[off:(metas[i + 1][0] if i + 1 < len(metas) else fo)] for i, (off, _) in enumerate(metas)]
    return info, metas, blocks, sst[fo:fo + fl]


def rebuild(sst: bytes, blocks: list[bytes] | None = None, filt: bytes | None = None, offsets=None,
            index_bytes=None) -> bytes:
    """The SST with some of its pieces replaced: data blocks (any lengths), the encoded filter, the
    index's block offsets (a function of the true offsets), or the encoded index itself."""
    info, metas, old_blocks, old_filt = blocks_of(sst)
    blocks = old_blocks if blocks is None else blocks
    filt = old_filt if filt is None else filt
    out = bytearray()
    offs = []
    for b in blocks:
        offs.append(len(out))
        out += b
    f_off = len(out)
    out += filt
    if offsets is not None:
        offs = offsets(offs)
    if index_bytes is None:
        index_bytes = ob.encode_index([(o, fk) for o, (_, fk) in zip(offs, metas)], info["codec"])
    i_off = len(out)
    out += index_bytes
    info_b = ob.encode_info(info["first_key"] if info["first_key_len"] else None, i_off, len(index_bytes), f_off,
                            len(filt), info["codec"])
    info_off = len(out)
    out += info_b + struct.pack(">I", info_off)
    return bytes(out)


def stale_crc(piece: bytes) -> bytes:
    return piece[:-4] + struct.pack(">I", (zlib.crc32(piece[:-4]) ^ 0x5A5A5A5A) & 0xFFFFFFFF)


def classify(s: getref.RefSst, kvs, keys: list[bytes]) -> dict:
    """How many of `keys` are of each kind the query sets promise."""
    kvd = dict(kvs)
    first, last = kvs[0][0], kvs[-1][0]
    firsts = set(s.first_keys)
    gaps = getref.between_keys(s)
    c = dict(filter_fp=0, between=0, past_last=0, below_first=0, block_first=0, tombstone=0, present=0, empty=0)
    for k in keys:
        c["empty"] += k == b""
        c["below_first"] += k < first
        c["past_last"] += k > last
        c["block_first"] += k in firsts
        if k in kvd:
            c["present"] += 1
            c["tombstone"] += kvd[k] is None
        elif first <= k and s.filter is not None and ob.bloom_has_key(s.filter[0], s.filter[1], k):
            c["filter_fp"] += 1
        if k not in kvd and any(lo < k < hi for lo, hi in gaps):
            c["between"] += 1
    return c


@functools.lru_cache(maxsize=None)
def query_set(name: str, block_size: int) -> tuple:
    """4 096 queries over clean_sst(name, block_size, *): present keys and tombstones, absent keys
    (many pass the 2-bit filter), keys between two blocks, past the last key, below the first key,
    block first keys, the empty key, duplicates, and 64 queries that land on one block."""
    kvs = kv_set(name)
    rng = random.Random(block_size * 7 + len(name))
    s = getref.RefSst(clean_sst(name, block_size, ob.NONE))
    kvd = dict(kvs)
    keys_sorted = [k for k, _ in kvs]
    q = [b""]
    gaps = getref.between_keys(s)
    q += [lo + b"\x00" for lo, hi in gaps if lo + b"\x00" < hi][:48]
    q += [keys_sorted[-1] + bytes([i]) for i in range(24)]
    q += [bytes([rng.randrange(0x10)]) + bytes(rng.randrange(256) for _ in range(rng.randint(0, 6))) for _ in range(24)]
    q += list(s.first_keys)[:64]
    q += [k for k, v in kvs if v is None][:64]
    # 64 queries on one block: keys of a middle block
    mid = len(s.first_keys) // 2
    lo = s.first_keys[mid]
    hi = s.first_keys[mid + 1] if mid + 1 < len(s.first_keys) else None
    inside = [k for k in keys_sorted if k >= lo and (hi is None or k < hi)]
    q += [rng.choice(inside) for _ in range(64)]  # (present keys: the filter lets every one through)
    # absent keys shaped like the present ones (filter false positives among them)
    while len(q) < 1800:
        k = rng.choice(keys_sorted)
        m = bytearray(k)
        m[rng.randrange(len(m))] ^= 1 << rng.randrange(8)
        m = bytes(m) if rng.random() < 0.7 else k + b"!"
        if m not in kvd:
            q.append(m)
    q += [rng.choice(keys_sorted) for _ in range(N_QUERIES - 128 - len(q))]
    q += [rng.choice(q) for _ in range(128)]  # duplicates
    assert len(q) == N_QUERIES
    rng.shuffle(q)
    return tuple(q)


@functools.lru_cache(maxsize=None)
def reference(name: str, block_size: int, codec: int):
    """getref over clean_sst(name, block_size, codec) and query_set(name, block_size):
    (results, val_off, values, consulted blocks)."""
    consulted = set()
    rs, vo, vals = getref.get_batch([getref.RefSst(clean_sst(name, block_size, codec))],
                                    list(query_set(name, block_size)), consulted)
    return rs, vo, vals, consulted
