"""SSTs and query sets for the batched point-read tests (test infrastructure), shared by
tests/test_get_oracle.py and tests/test_get_shapes_oracle.py (which assert the sets contain what
they claim), tests/test_get_gpu.py and tests/test_get_shapes_gpu.py.  Everything is cached: an
SST, its query set and its reference results are built once per process."""
from __future__ import annotations

import functools
import random
import struct
import zlib

import numpy as np

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


def encode_index(metas, codec: int) -> bytes:
    """ob.encode_index for every codec (the oracle compresses None and Snappy; the others as
    sstgen.recode does it)."""
    if codec in (ob.NONE, ob.SNAPPY):
        return ob.encode_index(metas, codec)
    return sstgen.crc(sstgen.compress(codec, ob.encode_index(metas, ob.NONE)[:-4], random.Random(codec)))


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
        index_bytes = encode_index([(o, fk) for o, (_, fk) in zip(offs, metas)], info["codec"])
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


# ------------------------------------------------------------------ shapes the first mould leaves out
def check(ctx, handles, keys, ref, one_call=False):
    """One get over `handles` equals the reference: res field by field, val_off, the value bytes.
    one_call: a single slate_sst_get_batch call with room for the values (for the counters;
    Context.get asks for the size first and looks the keys up twice)."""
    rs, ref_off, ref_vals = ref[:3]
    if one_call:
        st, res, vals, val_off = ctx.get_into(handles, keys, len(ref_vals))
        assert st == 0
    else:
        res, vals, val_off = ctx.get(handles, keys)
    assert len(res) == len(keys)
    for f in getref.FIELDS:
        want = np.array([r[f] for r in rs], dtype=np.int64)
        got = res[f].astype(np.int64)
        bad = np.nonzero(want != got)[0]
        assert bad.size == 0, (f, int(bad[0]), keys[int(bad[0])], rs[int(bad[0])], res[int(bad[0])])
    assert np.array_equal(val_off, ref_off)
    assert vals.tobytes() == ref_vals
    return res


def expand(rs: list[dict]):
    """(results, val_off, values concatenated) of a list of result dicts, as getref.get_batch."""
    val_off = np.zeros(len(rs) + 1, np.uint64)
    if rs:
        val_off[1:] = np.cumsum([r["value_len"] for r in rs], dtype=np.uint64)
    return rs, val_off, b"".join(r["value"] for r in rs)


def ref_of(ssts, keys):
    """getref over encoded SSTs (or RefSsts) in precedence order, getref.get_one called once per
    distinct key: (results, val_off, values, consulted blocks)."""
    refs = [s if isinstance(s, getref.RefSst) else getref.RefSst(s) for s in ssts]
    consulted = set()
    memo = {}
    for k in keys:
        if k not in memo:
            memo[k] = getref.get_one(refs, k, consulted)
    return expand([memo[k] for k in keys]) + (consulted,)


VALUE_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 143, 144, 145, 255, 256, 257, 1024, 4097, 65521, 70000)


@functools.lru_cache(maxsize=None)
def kvs_value_edges():
    """~80 KVs under 4-byte keys b"k%03d" (even numbers; the odd ones are absent neighbours): every
    length of VALUE_LENGTHS three times, lengths mixed so that a short value follows a long one,
    random (incompressible) bytes, the empty one an empty *value* (b""), and a tombstone (None)
    after every eighth key.  A 65521-byte value under a 4-byte key is a row of 65542 bytes: alone
    in its block, uint16(len(Data)) wraps to 6."""
    rng = random.Random(2025)
    lens = [VALUE_LENGTHS[(8 * i) % len(VALUE_LENGTHS)] for i in range(3 * len(VALUE_LENGTHS))]
    vals = []
    for i, n in enumerate(lens):
        vals.append(rng.randbytes(n))
        if i % 8 == 7:
            vals.append(None)
    return tuple((b"k%03d" % (2 * i), v) for i, v in enumerate(vals))


@functools.lru_cache(maxsize=None)
def value_edges_sst(codec: int) -> bytes:
    none = sstgen.none_sst(list(kvs_value_edges()), 4096, 0, 2)
    return none if codec == ob.NONE else sstgen.recode(none, codec, random.Random(100 + codec))


@functools.lru_cache(maxsize=None)
def value_edges_queries() -> tuple:
    """Every key three times and the absent neighbours (the odd numbers, key + 0x00, the 3-byte
    prefix), shuffled: values of different lengths lie next to each other in the output."""
    ks = [k for k, _ in kvs_value_edges()]
    q = ks * 3 + [b"k%03d" % (2 * i + 1) for i in range(len(ks))] + [k + b"\x00" for k in ks[::5]]
    q += [ks[9][:3], b"", b"l"]
    random.Random(6).shuffle(q)
    return tuple(q)


TS_KINDS = ("none", "expire", "create", "both")


@functools.lru_cache(maxsize=None)
def timestamped_sst(codec: int):
    """clean_sst("random", 512, *) with the rows of every third block re-encoded with an expire
    and / or a create timestamp (8 or 16 bytes between the row's flags and its value), cycling
    through TS_KINDS, tombstones included -> (sst, {key: kind} of the re-encoded rows)."""
    none = clean_sst("random", 512, ob.NONE)
    s = getref.RefSst(none)
    blocks = list(blocks_of(none)[2])
    kinds = {}
    n = 0
    for b in range(0, len(blocks), 3):
        st, data, offs = s.block(b)
        assert st == 0
        out, new_offs, first = bytearray(), [], None
        for o in offs:
            row = ob.v0_decode(data[o:], None if first is None else len(first))
            assert row.status == 0 and row.expire_ms is None and row.create_ms is None
            if first is None:
                first = row.key_suffix
            kind = TS_KINDS[n % 4]
            n += 1
            kinds[first[:row.key_prefix_len] + row.key_suffix] = kind
            new_offs.append(len(out))
            out += ob.v0_encode(row.key_prefix_len, row.key_suffix, None if row.tombstone else row.value, row.seq,
                                1_700_000_000_000 + n if kind in ("expire", "both") else None,
                                1_600_000_000_000 + 3 * n if kind in ("create", "both") else None)
        st, enc = ob.block_encode(bytes(out), new_offs, ob.NONE)
        assert st == 0
        blocks[b] = enc
    sst = rebuild(none, blocks=blocks)
    return (sst if codec == ob.NONE else sstgen.recode(sst, codec, random.Random(200 + codec))), kinds


@functools.lru_cache(maxsize=None)
def kvs_mixed():
    return tuple(bg.kv_mixed(600))


@functools.lru_cache(maxsize=None)
def mixed_sst(codec: int) -> bytes:
    """bg.kv_mixed(600): keys of 8-256 bytes with long shared prefixes, 1 KiB values, 200 blocks."""
    none = sstgen.none_sst(list(kvs_mixed()), 4096, 0, 2)
    return none if codec == ob.NONE else sstgen.recode(none, codec, random.Random(300 + codec))


@functools.lru_cache(maxsize=None)
def mixed_queries() -> tuple:
    """Every key, every key with its last byte changed, strict prefixes (the compare's length
    tie-break), key + 0x00, a 1 000-byte and a 65 535-byte key that extend a present key, the
    empty key."""
    ks = [k for k, _ in kvs_mixed()]
    rng = random.Random(8)
    q = list(ks)
    q += [k[:-1] + bytes([k[-1] ^ (1 << rng.randrange(8))]) for k in ks]
    q += [k[:rng.randrange(1, len(k))] for k in ks[::2]]
    q += [k[:-1] for k in ks[1::4]]
    q += [k + b"\x00" for k in ks[::3]]
    q += [ks[300] + b"z" * (1000 - len(ks[300])), ks[17] + b"\x01" * (65535 - len(ks[17])), b""]
    rng.shuffle(q)
    return tuple(q)


def many_blocks_sst(codec: int) -> bytes:
    """kv_set("random") at block size 64: one row per block, 2 051 blocks -- three blocks per thread
    in the general path's block compaction, and idle threads after the last block."""
    return clean_sst("random", 64, codec)


@functools.lru_cache(maxsize=None)
def kvs_tombstones():
    """8 398 tombstones under 2-byte keys: 15-byte rows (17 with the row's offset)."""
    rng = random.Random(5)
    return tuple(sorted({bytes([rng.randrange(256), rng.randrange(256)]) for _ in range(9000)}))


@functools.lru_cache(maxsize=None)
def rows_2048_sst() -> bytes:
    """Rows per block [2048, 2046, 2047, 2048, 209]: the most the fused kernel's seek takes."""
    return sstgen.none_sst([(k, None) for k in kvs_tombstones()], 34790, 0, 10)


@functools.lru_cache(maxsize=None)
def rows_2049_sst() -> bytes:
    """Rows per block [2049, 2047, 2047, 2048, 207]: block 0 is the first size handed over."""
    return sstgen.none_sst([(k, None) for k in kvs_tombstones()], 34798, 0, 10)


def block_rows(s: getref.RefSst) -> list[int]:
    return [len(s.block(b)[2]) for b in range(len(s.metas))]


def block_last_keys(s: getref.RefSst) -> list[bytes]:
    out = []
    for b in range(len(s.metas)):
        st, data, offs = s.block(b)
        assert st == 0
        fl = ob.v0_decode(data[offs[0]:], None)
        last = ob.v0_decode(data[offs[-1]:], len(fl.key_suffix))
        out.append(fl.key_suffix[:last.key_prefix_len] + last.key_suffix)
    return out


@functools.lru_cache(maxsize=None)
def row_boundary_queries() -> tuple:
    """For both row-count SSTs (same keys, other block cuts): the first and last key of every
    block, a key just past each last key, 2 000 random 2- and 3-byte keys."""
    rng = random.Random(9)
    q = []
    for sst in (rows_2048_sst(), rows_2049_sst()):
        s = getref.RefSst(sst)
        lasts = block_last_keys(s)
        q += list(s.first_keys) + lasts + [k + b"\x00" for k in lasts]
    q += [bytes(rng.randrange(256) for _ in range(rng.choice([2, 3]))) for _ in range(2000)]
    rng.shuffle(q)
    return tuple(q)


STRIDE_STALE = (3, 20, 41, 77, 130)


@functools.lru_cache(maxsize=None)
def stride_sst(codec: int) -> bytes:
    """clean_sst("random", 512, *) without a filter (every in-range query is located) and with a
    stale CRC on five blocks."""
    clean = clean_sst("random", 512, codec, 10, len(kv_set("random")) + 1)
    blocks = list(blocks_of(clean)[2])
    for b in STRIDE_STALE:
        blocks[b] = stale_crc(blocks[b])
    return rebuild(clean, blocks=blocks)



def stride_queries(waves: int):
    """-> (queries, number the reference locates) for a fused grid of `waves` waves: more located
    queries than 2.5 grids, so that every wave takes a third query and some take only two; drawn
    from present keys and tombstones, keys between two blocks, keys past the last key, keys in the
    stale-CRC blocks, and a few below the first key (not located)."""
    need = 2 * waves + waves // 2 + 37
    s = getref.RefSst(stride_sst(ob.NONE))
    rng = random.Random(waves)
    ks = [k for k, _ in kv_set("random")]
    gaps = [lo + b"\x00" for lo, hi in getref.between_keys(getref.RefSst(clean_sst("random", 512, ob.NONE)))
            if lo + b"\x00" < hi]
    past = [ks[-1] + bytes([i]) for i in range(16)]
    stale = [k for k in ks if ob.index_seek(s.first_keys, k) in STRIDE_STALE]
    pool = ks + gaps * 3 + past + stale * 4
    q = [rng.choice(pool) for _ in range(need)] + [b"", b"\x01", b"\x0f\xff"]
    located = sum(1 for k in q if s.may_include(k) is None)
    assert located == need
    rng.shuffle(q)
    return q, located


@functools.lru_cache(maxsize=None)
def mutated_sst(codec: int, where: str) -> bytes:
    """clean_sst("random", 512, codec) with bg.mutate applied to a tenth of its blocks and the CRC
    made right again.  where = "encoded": the block's encoded bytes are mutated (the frame of a
    compressing codec is damaged); "decoded": the block's payload is mutated and then compressed
    (the frame is sound, the block in it is not)."""
    clean = clean_sst("random", 512, codec)
    rng = random.Random(40 + codec)
    blocks = list(blocks_of(clean)[2])
    plain = blocks_of(clean_sst("random", 512, ob.NONE))[2]
    for b in rng.sample(range(len(blocks)), len(blocks) // 10):
        if where == "encoded":
            blocks[b] = bg.mutate(rng, blocks[b], fix_crc=True)
        else:
            blocks[b] = sstgen.crc(sstgen.compress(codec, bg.mutate(rng, plain[b], fix_crc=True)[:-4], rng))
    return rebuild(clean, blocks=blocks)


@functools.lru_cache(maxsize=None)
def zero_block_sst() -> bytes:
    """clean_sst("random", 4096, None) with its first key and filter and an index of no blocks:
    a key in range that passes the filter finds no block to read."""
    clean = clean_sst("random", 4096, ob.NONE)
    return rebuild(clean, blocks=[], index_bytes=ob.encode_index([], ob.NONE))


@functools.lru_cache(maxsize=None)
def five_codec_ssts():
    """-> (five SSTs, one per codec, in precedence order; their KV lists): each holds a random half
    of kv_set("random") under its own values, and the first two delete some keys the later hold."""
    rng = random.Random(78)
    parts = [[] for _ in CODECS]
    for k, v in kv_set("random"):
        for j in range(len(CODECS)):
            if rng.random() < 0.5:
                parts[j].append((k, None if (j < 2 and rng.random() < 0.3) else bytes([j]) + (v or b"x")))
    ssts = [sstgen.none_sst(p, 4096, 0, 10) for p in parts]
    return tuple(s if c == ob.NONE else sstgen.recode(s, c, random.Random(c)) for s, c in zip(ssts, CODECS)), parts


@functools.lru_cache(maxsize=None)
def eight_range_ssts():
    """Eight SSTs over disjoint, ascending eighths of kv_set("random"), codecs in turn: a query is
    out of range or filtered in most of them."""
    kvs = list(kv_set("random"))
    step = -(-len(kvs) // 8)
    out = []
    for j in range(8):
        s = sstgen.none_sst(kvs[j * step:(j + 1) * step], 512, 0, 10)
        c = CODECS[j % len(CODECS)]
        out.append(s if c == ob.NONE else sstgen.recode(s, c, random.Random(j)))
    return tuple(out)
