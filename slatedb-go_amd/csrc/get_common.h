// Device code shared by the batched point-read kernels over handles (get.hip) and over sorted
// runs (get_runs.hip): the result bookkeeping, one SST's filter probe and index seek, blockIter.Next
// on the row a seek stands on, and one block of iter.Next by one wave (the CodecNone fused body).
#pragma once
#include "bloom_probes.h"
#include "common.h"
#include "kernels.h"
#include "rows.h"
#include "seek_common.h"
#include "wave_crc.h"

namespace slate {

typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));  // 16 bytes at any alignment

// Position in a list for every lane with pred set: one atomic per wave.  Called by whole waves.
__device__ inline uint32_t wave_append(uint32_t* cnt, bool pred) {
  const uint64_t m = __ballot(pred);
  if (!m) return 0;
  const uint32_t lane = threadIdx.x & 63;
  const int leader = __builtin_ctzll(m);
  uint32_t base = 0;
  if (int(lane) == leader) base = atomicAdd(cnt, uint32_t(__popcll(m)));
  base = __shfl(base, leader, 64);
  return base + uint32_t(__popcll(m & ((uint64_t(1) << lane) - 1)));
}

__device__ inline void note_err(slate_get_result& r, int st, uint32_t sst) {
  if (r.err == SLATE_OK) {
    r.err = int16_t(st);
    r.err_sst = sst;
  }
}

__device__ inline void set_panic(slate_get_result& r, int st, uint32_t sst) {
  r.outcome = SLATE_GET_PANIC;
  r.err = int16_t(st);
  r.err_sst = sst;
  r.sst = sst;
}

// A status that ended the iteration in this block (a read, block.Decode or NewIteratorAtKey error)
__device__ inline void end_error(slate_get_result& r, int st, uint32_t sst) {
  r.stage = SLATE_GET_AT_ERROR;
  if (st == SLATE_E_BLOCK_FIRSTKEY_PANIC || st == SLATE_E_SEEK_PANIC) set_panic(r, st, sst);
  else note_err(r, st, sst);
}

// Filter.HasKey (bloom.go:19-49) of s's decoded filter, as bloom_check_kernel (s.has_filter)
__device__ inline bool sst_filter_has_key(const GetSst& s, const uint8_t* key, uint32_t kl) {
  const uint64_t m = (s.fbits_len * 8) & 0xFFFFFFFFull;
  if (m == 0) return false;
  uint64_t h64 = 0xcbf29ce484222325ull;  // FNV-1 64
  for (uint32_t b = 0; b < kl; b++) {
    h64 *= 0x100000001b3ull;
    h64 ^= key[b];
  }
  BloomProbes pr(h64, uint32_t(m));
  bool may = true;
  for (uint32_t k = 0; k < s.num_probes && may; k++) {
    const uint32_t p = pr.next();
    may = (s.fbits[p >> 3] & (1u << (p & 7))) != 0;
  }
  return may;
}

// firstBlockIncludingOrAfterKey (iterator.go:123-153) over s's index (s.nb > 0)
__device__ inline uint32_t sst_first_block(const GetSst& s, const uint8_t* key, uint32_t kl) {
  int64_t low = 0, high = int64_t(s.nb) - 1, found = 0;
  while (low <= high) {
    const int64_t mid = low + (high - low) / 2;
    const int c = cmp_bytes(s.ikeys + s.ikey_off[mid], uint32_t(s.ikey_off[mid + 1] - s.ikey_off[mid]), key, kl);
    if (c < 0) {
      low = mid + 1;
      found = mid;
    } else if (c > 0) {
      if (mid > 0) high = mid - 1;
      else break;
    } else {
      found = mid;
      break;
    }
  }
  return uint32_t(found);
}

// blockIter.Next (block/iterator.go:84-107) on the row the seek stands on, then db.go:246-248.
// d: Block.Data (dlen bytes, the BE16 offsets after it), cnt = len(Offsets).  false: the block
// gave no row (offsetIndex past the end, or the row failed v0RowCodec.Decode: row.go:191-261
// against the iterator's firstKey, sk.first_len bytes) and the iteration goes on with block + 1.
__device__ inline bool get_row(const uint8_t* d, uint32_t dlen, uint32_t cnt, const slate_seek& sk, const uint8_t* key,
                               uint32_t kl, uint32_t sst, uint32_t b, slate_get_result& r, uint64_t* vsrc) {
  if (sk.start >= cnt) return false;
  const uint8_t* offs = d + dlen;
  const uint32_t o = ld_be16(offs + 2 * sk.start);
  if (o > dlen) {  // data[offset:] panics (block.Decode's uint16 bound rules it out; kept for memory safety)
    r.stage = SLATE_GET_AT_ROW;
    r.block = b;
    r.row = sk.start;
    set_panic(r, SLATE_E_ROW_PANIC, sst);
    return true;
  }
  slate_row row;
  uint32_t sl;
  decode_row(d, dlen, o, int(sk.first_len), row, &sl);
  if (row.status == SLATE_E_ROW_PANIC) {
    r.stage = SLATE_GET_AT_ROW;
    r.block = b;
    r.row = sk.start;
    set_panic(r, SLATE_E_ROW_PANIC, sst);
    return true;
  }
  if (row.status != SLATE_OK) {
    note_err(r, row.status, sst);
    return false;
  }
  // Key = firstKey[:prefixLen] || suffix (row.go:72-79)
  const uint32_t pl = row.key_prefix_len;
  const uint8_t* fk = d + ld_be16(offs + 2 * uint32_t(sk.first_idx)) + 4;
  const uint8_t* suf = d + o + 4;
  bool eq = pl + sl == kl;
  for (uint32_t i = 0; eq && i < kl; i++) eq = (i < pl ? fk[i] : suf[i - pl]) == key[i];
  r.stage = SLATE_GET_AT_ROW;
  r.block = b;
  r.row = sk.start;
  if (eq) {
    r.sst = sst;
    if (row.flags & 1) {
      r.outcome = SLATE_GET_TOMBSTONE;
    } else {
      r.outcome = SLATE_GET_VALUE;
      r.value_len = row.value_len;
      *vsrc = uint64_t(reinterpret_cast<uintptr_t>(suf + sl + row.meta_len));
    }
  }
  return true;
}

// ---------------------------------------------------------------- fused CodecNone body
constexpr int kFusedThreads = 256;
constexpr uint32_t kFusedWaves = kFusedThreads / 64;
constexpr uint32_t kFusedWaveWords = kSeekWaveRows + 16;  // the seek's outcome per row, then its staged arguments

// what one block gave the iteration
enum {
  kBlkRow = 0,   // a row (or a panic decoding it): r is final for this SST
  kBlkNext = 1,  // no row: on to block + 1
  kBlkEnd = 2,   // an error (or panic) ended the SST's iteration: r.stage = AT_ERROR
  kBlkHand = 3,  // more rows than the wave's outcome array holds: the general path's
};

// One block of iter.Next (iterator.go:59-89) by one wave, every value wave-uniform: block b
// (< s.nb) of CodecNone SST s -- the range check, the CRC over the encoded bytes in place,
// block.Decode's checks (block.go:78-134; CodecNone aliases the input), then either
// block.NewIteratorAtKey (seek_one_wave) or, from_start, block.NewIterator (offsetIndex 0,
// firstKey nil), and blockIter.Next with the key compare.  tab: the CRC tables in LDS; wl: the
// wave's kFusedWaveWords words of LDS.  sst: the source index written to r.
__device__ inline int fused_block(const GetSst& s, uint32_t b, bool from_start, const uint32_t* tab, uint32_t* wl,
                                  uint32_t lane, const GetQ& q, uint32_t qi, const uint8_t* key, uint32_t kl,
                                  uint32_t sst, slate_get_result& r, uint64_t* vsrc) {
  uint32_t* outcome = wl;
  // seek_one_wave reads its block, offset and query through pointers: one block's worth in LDS
  slate_block_meta* lmeta = reinterpret_cast<slate_block_meta*>(outcome + kSeekWaveRows);
  uint64_t* loff = reinterpret_cast<uint64_t*>(outcome + kSeekWaveRows + 4);
  uint32_t* lqb = outcome + kSeekWaveRows + 6;
  slate_seek* lres = reinterpret_cast<slate_seek*>(outcome + kSeekWaveRows + 8);
  if (s.bbad[b]) {
    end_error(r, SLATE_E_BLOB_RANGE, sst);
    return kBlkEnd;
  }
  const uint64_t off = s.bstart[b], len = s.bend[b] - off;
  if (len < 6) {
    end_error(r, SLATE_E_BLOCK_TOO_SMALL, sst);
    return kBlkEnd;
  }
  const uint8_t* blk = s.region + off;
  const uint32_t cnt16 = len <= (1u << 30) ? ld_be16(blk + len - 6) : 0xFFFFFFFFu;
  if (cnt16 > kSeekWaveRows) return kBlkHand;
  const uint32_t n = uint32_t(len - 4);
  // block.go:85-88: the CRC over the encoded bytes where they lie (4-byte aligned base + msg)
  const uint32_t crc = wave_crc32(tab, s.region + (off & ~uint64_t(3)), int32_t(off & 3), n, int(lane));
  if (__builtin_amdgcn_readfirstlane(crc) != ld_be32(blk + n)) {
    end_error(r, SLATE_E_BLOCK_CHECKSUM, sst);
    return kBlkEnd;
  }
  // block.go:95-131 (rows.h block_finish)
  const int64_t osi = int64_t(n) - 2 - 2 * int64_t(cnt16);
  if (osi <= 0) {
    end_error(r, SLATE_E_BLOCK_INDEX_OFFSET, sst);
    return kBlkEnd;
  }
  const uint16_t osi16 = uint16_t(osi);
  bool bad = false;
  for (uint32_t i0 = 0; i0 < cnt16 && !bad; i0 += 64) {
    const uint32_t i = i0 + lane;
    bad = __ballot(i < cnt16 && ld_be16(blk + osi + 2 * i) > osi16) != 0;
  }
  if (bad) {
    end_error(r, SLATE_E_BLOCK_OFFSET_BOUNDS, sst);
    return kBlkEnd;
  }
  if (cnt16 == 0) {
    end_error(r, SLATE_E_BLOCK_NO_OFFSETS, sst);
    return kBlkEnd;
  }
  uint16_t fk16 = 0;
  {
    const uint32_t off0 = ld_be16(blk + osi);
    bool pan = uint64_t(osi) - off0 < 2;
    if (!pan) {
      fk16 = ld_be16(blk + off0);
      const uint16_t lo = uint16_t(off0 + 2), hi = uint16_t(off0 + 2 + fk16);
      pan = lo > hi || hi > n;
    }
    if (pan) {
      end_error(r, SLATE_E_BLOCK_FIRSTKEY_PANIC, sst);
      return kBlkEnd;
    }
  }
  slate_seek sk{};  // block.NewIterator: offsetIndex 0, firstKey nil
  if (!from_start) {
    __builtin_amdgcn_wave_barrier();  // (the lanes' reads of the previous block's seek result are done)
    if (lane == 0) {
      slate_block_meta m{};
      m.data_len = uint32_t(osi);
      m.n_rows = uint16_t(cnt16);
      m.aux = fk16;
      *lmeta = m;
      *loff = 0;
      *lqb = 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    seek_one_wave(blk, loff, lmeta, lqb, q.keys, q.key_off + qi, lres, nullptr, 0, lane, outcome);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    sk = *lres;
    if (sk.status != SLATE_OK) {
      end_error(r, sk.status, sst);
      return kBlkEnd;
    }
  }
  return get_row(blk, uint32_t(osi), cnt16, sk, key, kl, sst, b, r, vsrc) ? kBlkRow : kBlkNext;
}

}  // namespace slate
