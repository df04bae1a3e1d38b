"""Sorted runs and query sets for the batched point reads over runs (test infrastructure), shared
by tests/test_get_runs_oracle.py (which asserts that the sets contain what they promise) and
tests/test_get_runs_gpu.py.  A run is a tuple of encoded SSTs in SSTList order.  Everything is
cached: a run, its query set and its reference results are built once per process."""
from __future__ import annotations

import functools
import random
import struct

from oracle import binding as ob
from tests import getgen, getref, srref, sstgen

CODECS = getgen.CODECS


def _enc(none: bytes, codec: int, seed: int) -> bytes:
    return none if codec == ob.NONE else sstgen.recode(none, codec, random.Random(seed))


def _parts(kvs, n: int):
    step = -(-len(kvs) // n)
    return [kvs[j * step:(j + 1) * step] for j in range(n)]


def with_first_key(sst: bytes, first_key: bytes | None) -> bytes:
    """The SST with Info.FirstKey replaced (None: no first key); nothing else moves."""
    st, info = ob.sst_read_info(sst)
    assert st == 0
    info_off = struct.unpack(">I", sst[-4:])[0]
    info_b = ob.encode_info(first_key, info["index_offset"], info["index_len"], info["filter_offset"],
                            info["filter_len"], info["codec"])
    return sst[:info_off] + info_b + struct.pack(">I", info_off)


def last_key(sst: bytes) -> bytes:
    return getgen.block_last_keys(getref.RefSst(sst))[-1]


def refs(run) -> list[getref.RefSst]:
    return [getref.RefSst(s) for s in run]


@functools.lru_cache(maxsize=None)
def reference(l0: tuple, runs: tuple, keys: tuple):
    """srref over encoded SSTs: (results, val_off, values, consulted run blocks, trace)."""
    consulted, trace = set(), {}
    out = srref.get_batch(refs(l0), [refs(r) for r in runs], list(keys), consulted, trace)
    return out + (consulted, trace)


# ------------------------------------------------------------------ a clean run
@functools.lru_cache(maxsize=None)
def clean_run(codec: int, n_sst: int = 8, block_size: int = 256) -> tuple:
    """kv_set("random") as n_sst SSTs over contiguous parts, several blocks each, 2-bit filters."""
    return tuple(_enc(sstgen.none_sst(p, block_size, 0, 2), codec, 500 + j)
                 for j, p in enumerate(_parts(list(getgen.kv_set("random")), n_sst)))


@functools.lru_cache(maxsize=None)
def clean_queries(n_sst: int = 8, block_size: int = 256) -> tuple:
    """~1 000 queries over clean_run(*, n_sst, block_size): present keys and tombstones, absent
    keys (many pass the 2-bit filter), the empty key, keys below the run's first key, every SST's
    first key and last key, keys between SST p's last key and SST p + 1's first key (those the
    filter lets through walk off p into p + 1's row 0), keys past the run's last key, duplicates."""
    kvs = getgen.kv_set("random")
    kvd = dict(kvs)
    ks = [k for k, _ in kvs]
    rng = random.Random(91 + n_sst)
    run = clean_run(ob.NONE, n_sst, block_size)
    q = [b"", b"\x01", b"\x0f\xff", ks[0][:1]]
    firsts = [getref.RefSst(s).info["first_key"] for s in run]
    lasts = [last_key(s) for s in run]
    q += firsts + lasts
    for lo, hi in zip(lasts[:-1], firsts[1:]):
        q += [k for k in (lo + bytes([i]) for i in range(12)) if k < hi]
    q += [ks[-1] + bytes([i]) for i in range(12)]
    q += [k for k, v in kvs if v is None][:60]
    while len(q) < 500:  # absent keys shaped like the present ones
        k = rng.choice(ks)
        m = bytearray(k)
        m[rng.randrange(len(m))] ^= 1 << rng.randrange(8)
        m = bytes(m) if rng.random() < 0.7 else k + b"!"
        if m not in kvd:
            q.append(m)
    q += [rng.choice(ks) for _ in range(440)]
    q += [rng.choice(q) for _ in range(60)]  # duplicates
    rng.shuffle(q)
    return tuple(q)


# ------------------------------------------------------------------ a forged first key
@functools.lru_cache(maxsize=None)
def forged_run() -> tuple:
    """[A, B]: the halves of kv_set("random"), A without a filter, B's Info.FirstKey forged above
    every query -- sort.Search always picks A, and B is only ever entered from its start."""
    kvs = list(getgen.kv_set("random"))
    half = next(i for i in range(len(kvs) // 2, len(kvs)) if kvs[i][1] is not None)  # B's row 0 is a value
    a = sstgen.none_sst(kvs[:half], 256, len(kvs) + 1, 2)
    b = with_first_key(sstgen.none_sst(kvs[half:], 256, 0, 2), b"\xff" * 40)
    return (a, b)


@functools.lru_cache(maxsize=None)
def forged_queries() -> tuple:
    """Keys of A, every key of B (each past A's last row: the lookup returns B's row 0, which only
    B's first key equals), keys past B."""
    kvs = list(getgen.kv_set("random"))
    b0 = getref.RefSst(forged_run()[1]).first_keys[0]
    at = [k for k, _ in kvs].index(b0)
    q = [k for k, _ in kvs[:at:7]] + [k for k, _ in kvs[at:]] + [kvs[-1][0] + b"\x00", b""]
    random.Random(17).shuffle(q)
    return tuple(q)


# ------------------------------------------------------------------ damaged runs
E_BLOCK_CHECKSUM = 2


def _prefixed_row0(none: bytes) -> bytes:
    """The CodecNone SST with block 0's row 0 re-encoded under prefix length 1 (the CRC right):
    v0RowCodec.Decode against a nil firstKey rejects it."""
    s = getref.RefSst(none)
    st, data, offs = s.block(0)
    assert st == 0
    out, new_offs, first = bytearray(), [], None
    for i, o in enumerate(offs):
        row = ob.v0_decode(data[o:], None if first is None else len(first))
        assert row.status == 0
        if first is None:
            first = row.key_suffix
        pl, suf = (1, row.key_suffix[1:]) if i == 0 else (row.key_prefix_len, row.key_suffix)
        new_offs.append(len(out))
        out += ob.v0_encode(pl, suf, None if row.tombstone else row.value, row.seq, row.expire_ms, row.create_ms)
    st, enc = ob.block_encode(bytes(out), new_offs, ob.NONE)
    assert st == 0
    blocks = list(getgen.blocks_of(none)[2])
    blocks[0] = enc
    return getgen.rebuild(none, blocks=blocks)


def _stale(sst: bytes, b: int) -> bytes:
    blocks = list(getgen.blocks_of(sst)[2])
    blocks[b] = getgen.stale_crc(blocks[b])
    return getgen.rebuild(sst, blocks=blocks)


DAMAGED_VARIANTS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def damaged_run(codec: int, variant: int = 0) -> tuple:
    """Five SSTs over the fifths of kv_set("random"), block size 256.  Every variant: (a) a stale
    CRC on SST 1's last block, (c) SST 3's block 0 with row 0 under prefix length 1 (CRC right: a
    walk moves on to its block 1).  Variant 0 and 2: (b) a stale CRC on SST 2's block 0.
    Variant 1: (d) SST 2 has no blocks (its first key and filter stay).  Variant 2: (e) a stale
    CRC on the last SST's last block, which ends the run AT_ERROR."""
    nones = [sstgen.none_sst(p, 256, 0, 2) for p in _parts(list(getgen.kv_set("random")), 5)]
    nones[3] = _prefixed_row0(nones[3])
    run = [_enc(s, codec, 600 + j) for j, s in enumerate(nones)]
    run[1] = _stale(run[1], -1)
    if variant in (0, 2):
        run[2] = _stale(run[2], 0)
    if variant == 1:
        run[2] = getgen.rebuild(run[2], blocks=[], index_bytes=getgen.encode_index([], codec))
    if variant == 2:
        run[4] = _stale(run[4], -1)
    return tuple(run)


@functools.lru_cache(maxsize=None)
def damaged_queries() -> tuple:
    """Every third key, every key of the damaged blocks and of SST 2, keys between and past SSTs."""
    kvs = list(getgen.kv_set("random"))
    parts = _parts(kvs, 5)
    q = [k for k, _ in kvs[::3]] + [k for k, _ in parts[2]]
    for j in (1, 3, 4):
        s = getref.RefSst(sstgen.none_sst(parts[j], 256, 0, 2))
        lo_first, lo_last = s.first_keys[0], s.first_keys[-1]
        q += [k for k, _ in parts[j] if k >= lo_last or (j == 3 and k < s.first_keys[1])]
        q += [lo_first]
    q += [parts[j][-1][0] + bytes([i]) for j in range(5) for i in range(8)] + [b""]
    random.Random(23).shuffle(q)
    return tuple(q)


# ------------------------------------------------------------------ an empty first key
@functools.lru_cache(maxsize=None)
def empty_first_key_run() -> tuple:
    """[Z, A, B, C, D]: Z (the first 5 % of kv_set("random")) has no Info.FirstKey; A..D are the
    quarters of the rest.  sort.Search over five probes 2, then 1 or 3 or 4, and index 0 only for
    keys below A's first key: those panic, every other key never sees Z."""
    kvs = list(getgen.kv_set("random"))
    cut = len(kvs) // 20
    z = with_first_key(sstgen.none_sst(kvs[:cut], 256, 0, 2), None)
    return (z,) + tuple(sstgen.none_sst(p, 256, 0, 2) for p in _parts(kvs[cut:], 4))


@functools.lru_cache(maxsize=None)
def empty_first_key_queries() -> tuple:
    kvs = list(getgen.kv_set("random"))
    cut = len(kvs) // 20
    q = [k for k, _ in kvs[:cut]] + [k for k, _ in kvs[cut::4]] + [b"", kvs[cut][0], kvs[cut][0][:-1], kvs[-1][0] + b"z"]
    random.Random(29).shuffle(q)
    return tuple(q)


# ------------------------------------------------------------------ mixed codecs
@functools.lru_cache(maxsize=None)
def mixed_codec_run() -> tuple:
    """Five SSTs over the fifths of kv_set("random"), one per codec in CODECS order (SST 0
    CodecNone, SST 1 Snappy, ...); the last block of each of the first four has a stale CRC, so its
    keys walk on into the next SST -- from the fused kernel's SST 0 into Snappy's SST 1 among them."""
    run = [_enc(sstgen.none_sst(p, 256, 0, 2), c, 700 + j)
           for j, (p, c) in enumerate(zip(_parts(list(getgen.kv_set("random")), 5), CODECS))]
    for j in range(4):
        run[j] = _stale(run[j], -1)
    return tuple(run)


@functools.lru_cache(maxsize=None)
def mixed_codec_queries() -> tuple:
    kvs = list(getgen.kv_set("random"))
    parts = _parts(kvs, 5)
    q = [k for k, _ in kvs[::2]]
    for p in parts:
        q += [k for k, _ in p[-12:]] + [p[-1][0] + bytes([i]) for i in range(8)]
    random.Random(31).shuffle(q)
    return tuple(q)


# ------------------------------------------------------------------ many SSTs
@functools.lru_cache(maxsize=None)
def many_sst_run(codec: int, n_sst: int = 64) -> tuple:
    """kv_set("random") as n_sst SSTs of about 32 KVs each, block size 256."""
    return tuple(_enc(sstgen.none_sst(p, 256, 0, 10), codec, 800 + j)
                 for j, p in enumerate(_parts(list(getgen.kv_set("random")), n_sst)) if p)


@functools.lru_cache(maxsize=None)
def present_queries() -> tuple:
    q = [k for k, _ in getgen.kv_set("random")]
    random.Random(37).shuffle(q)
    return tuple(q)


# ------------------------------------------------------------------ precedence
@functools.lru_cache(maxsize=None)
def precedence_set():
    """-> (two L0 SSTs, two runs of two SSTs each, queries).  Run 1 holds every key under a
    value; run 0 holds every third key, half of them as tombstones; L0[1] every fifth key under
    its own value; L0[0] every seventh key as a tombstone.  So an L0 tombstone hides a run's value,
    a tombstone in run 0 hides a value in run 1, and most keys are present only in run 1."""
    kvs = [(k, (v or b"v")) for k, v in getgen.kv_set("random")]
    run1 = tuple(_enc(sstgen.none_sst(p, 512, 0, 10), c, 900 + j)
                 for j, (p, c) in enumerate(zip(_parts([(k, b"r1" + v) for k, v in kvs], 2), (ob.NONE, ob.SNAPPY))))
    r0 = [(k, None if i % 2 else b"r0" + v) for i, (k, v) in enumerate(kvs[::3])]
    run0 = tuple(_enc(sstgen.none_sst(p, 512, 0, 10), c, 910 + j)
                 for j, (p, c) in enumerate(zip(_parts(r0, 2), (ob.ZSTD, ob.NONE))))
    l1 = sstgen.none_sst([(k, b"l1" + v) for k, v in kvs[::5]], 512, 0, 10)
    l0 = _enc(sstgen.none_sst([(k, None) for k, _ in kvs[::7]], 512, 0, 10), ob.LZ4, 920)
    q = [k for k, _ in kvs] + [kvs[9][0] + b"?", b""]
    random.Random(41).shuffle(q)
    return (l0, l1), (run0, run1), tuple(q)
