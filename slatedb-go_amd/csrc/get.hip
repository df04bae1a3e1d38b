// Batched point reads (slate_sst_get_batch): DB.GetWithOptions' SST part (slatedb/db.go:237-250)
// for n keys at once over SSTs held in HBM (slate_sst_handle).
//   get_locate_kernel  sstMayIncludeKey (db.go:291-301: RangeCoversKey, the bloom probes of
//                      bloom.go:19-49) and firstBlockIncludingOrAfterKey (iterator.go:123-153),
//                      one thread per query;
//   get_fused_kernel   CodecNone: one wave per query walks iter.Next (iterator.go:59-89) itself --
//                      the block's CRC over the encoded bytes in place, block.Decode's checks
//                      (block.go:78-134; CodecNone aliases the input, nothing is copied), the
//                      wave-cooperative block.NewIteratorAtKey, blockIter.Next's row decode, the
//                      key compare of db.go:246, and on to block + 1 while the query is pending;
//   general path       every codec: mark the blocks the pending queries read, compact them in
//                      block order, gather their encoded bytes back to back, decode them as one
//                      batch (the block decode kernels), publish each block's decoded address and
//                      meta, then one thread per query seeks (seek_one) and fetches; a query that
//                      stands past its block's last row, or on a row that fails to decode, is
//                      appended to the next round's list with block + 1;
//   get_val_* / get_copy_kernel  the value offsets (a scan of the value lengths) and the copy of
//                      the values into one buffer in query order, eight lanes per value.
// What is expected to bound them (from the code and the timings in DESIGN.md; no counter
// profile yet): locate and fetch are dependent chains of scattered loads (a binary search over
// first keys or rows) -- latency, hidden by the batch; the fused kernel reads each block it visits
// once per query for the CRC (4 KiB, L2 hits for queries that share a block) and spends its time in
// the CRC's LDS table lookups; gather and copy are streaming copies.
// The result bookkeeping, get_row and the fused kernel's per-block body live in get_common.h,
// shared with the sorted-run kernels (get_runs.hip).
#include "get_common.h"

namespace slate {

namespace {

__global__ void get_init_kernel(GetQ q, uint32_t n_sst) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= q.n) return;
  slate_get_result r{};
  r.sst = n_sst;
  q.res[i] = r;
  q.vsrc[i] = 0;
  q.qblk[i] = kGetDone;
}

__global__ __launch_bounds__(256) void get_locate_kernel(GetSst s, GetQ q, const uint32_t* act, uint64_t na,
                                                         uint32_t* pend, uint32_t* cnt) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool want = false;
  uint32_t qi = 0;
  if (i < na) {
    qi = act ? act[i] : uint32_t(i);
    const uint8_t* key = q.keys + q.key_off[qi];
    const uint32_t kl = uint32_t(q.key_off[qi + 1] - q.key_off[qi]);
    uint32_t stage;
    if (s.first_key_len == 0 || cmp_bytes(key, kl, s.first_key, s.first_key_len) < 0) {
      stage = SLATE_GET_AT_RANGE;  // table.go:89-94
    } else {
      bool may = true;
      if (s.has_filter) may = sst_filter_has_key(s, key, kl);
      if (!may) {
        stage = SLATE_GET_AT_FILTER;
      } else if (s.nb == 0) {
        stage = SLATE_GET_AT_END;  // nextBlockIter: no block to read
      } else {
        q.qblk[qi] = sst_first_block(s, key, kl);
        stage = SLATE_GET_AT_END;  // (overwritten when the iteration ends)
        want = true;
      }
    }
    slate_get_result r = q.res[qi];
    r.stage = uint8_t(stage);
    r.block = 0;
    r.row = 0;
    q.res[qi] = r;
  }
  const uint32_t pos = wave_append(cnt + kGcPend, want);
  if (want) pend[pos] = qi;
}

// ---------------------------------------------------------------- fused CodecNone path
__global__ __launch_bounds__(kFusedThreads) void get_fused_kernel(GetSst s, GetQ q, const uint32_t* pend, uint32_t np,
                                                                  uint32_t* gen, uint32_t* cnt) {
  __shared__ uint32_t tab[1024];
  __shared__ __attribute__((aligned(16))) uint32_t wls[kFusedWaves][kFusedWaveWords];
  load_crc_tables(tab);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t waves_total = gridDim.x * kFusedWaves;
  uint32_t done = 0;
  for (uint32_t k = blockIdx.x * kFusedWaves + wave; k < np; k += waves_total) {
    const uint32_t qi = pend[k];
    const uint8_t* key = q.keys + q.key_off[qi];
    const uint32_t kl = uint32_t(q.key_off[qi + 1] - q.key_off[qi]);
    slate_get_result r = q.res[qi];
    uint64_t vsrc = 0;
    uint32_t b = q.qblk[qi];
    bool handed = false;
    for (;;) {  // iter.Next (iterator.go:59-89); every value below is wave-uniform
      if (b >= s.nb) {
        r.stage = SLATE_GET_AT_END;
        break;
      }
      const int w = fused_block(s, b, false, tab, wls[wave], lane, q, qi, key, kl, s.sst, r, &vsrc);
      if (w == kBlkHand) handed = true;
      if (w != kBlkNext) break;
      b++;
    }
    if (lane == 0) {
      if (handed) {
        q.res[qi] = r;  // (an err noted on the way here stays)
        q.qblk[qi] = b;
        gen[atomicAdd(cnt + kGcGen, 1u)] = qi;
      } else {
        q.res[qi] = r;
        q.vsrc[qi] = vsrc;
        q.qblk[qi] = kGetDone;
        done++;
      }
    }
  }
  if (lane == 0 && done) atomicAdd(cnt + kGcFused, done);
}

// ---------------------------------------------------------------- general path
__global__ void get_mark_kernel(GetSst s, GetQ q, const uint32_t* pend, uint32_t np, uint32_t* bflag) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= np) return;
  const uint32_t qi = pend[k];
  const uint32_t b = q.qblk[qi];
  if (b == kGetDone) return;
  if (b >= s.nb || s.bbad[b]) {
    slate_get_result r = q.res[qi];
    if (b >= s.nb) r.stage = SLATE_GET_AT_END;
    else end_error(r, SLATE_E_BLOB_RANGE, s.sst);
    q.res[qi] = r;
    q.qblk[qi] = kGetDone;
    return;
  }
  if (bflag[b] == 0) bflag[b] = 1;  // (every writer stores the same value)
}

constexpr int kCompactThreads = 1024;
__global__ __launch_bounds__(kCompactThreads) void get_compact_kernel(GetSst s, const uint32_t* bflag, uint32_t* list,
                                                                      uint64_t* in_off, uint32_t* cnt) {
  __shared__ uint32_t sc[kCompactThreads];
  __shared__ uint64_t sl[kCompactThreads];
  const uint32_t t = threadIdx.x;
  const uint32_t chunk = (s.nb + kCompactThreads - 1) / kCompactThreads;
  const uint32_t lo = min(s.nb, t * chunk), hi = min(s.nb, lo + chunk);
  uint32_t c = 0;
  uint64_t l = 0;
  for (uint32_t b = lo; b < hi; b++)
    if (bflag[b] == 1) {
      c++;
      l += s.bend[b] - s.bstart[b];
    }
  sc[t] = c;
  sl[t] = l;
  __syncthreads();
  for (uint32_t d = 1; d < kCompactThreads; d <<= 1) {  // inclusive scans
    const uint32_t pc = t >= d ? sc[t - d] : 0u;
    const uint64_t pl = t >= d ? sl[t - d] : 0ull;
    __syncthreads();
    sc[t] += pc;
    sl[t] += pl;
    __syncthreads();
  }
  uint32_t pos = sc[t] - c;
  uint64_t lp = sl[t] - l;
  for (uint32_t b = lo; b < hi; b++)
    if (bflag[b] == 1) {
      list[pos] = b;
      in_off[pos] = lp;
      pos++;
      lp += s.bend[b] - s.bstart[b];
    }
  if (t == kCompactThreads - 1) {
    in_off[sc[t]] = sl[t];
    cnt[kGcBlocks] = sc[t];
    cnt[kGcBytesLo] = uint32_t(sl[t]);
    cnt[kGcBytesHi] = uint32_t(sl[t] >> 32);
  }
}

// block list[i]'s encoded bytes to gin + in_off[i]: one workgroup per block, 16 bytes per lane
__global__ __launch_bounds__(256) void get_gather_kernel(GetSst s, const uint32_t* list, const uint64_t* in_off,
                                                         uint8_t* gin) {
  const uint32_t i = blockIdx.x;
  const uint32_t b = list[i];
  const uint8_t* src = s.region + s.bstart[b];
  uint8_t* dst = gin + in_off[i];
  const uint64_t len = s.bend[b] - s.bstart[b];
  const uint64_t chunks = len / 16;
  for (uint64_t c = threadIdx.x; c < chunks; c += blockDim.x)
    *reinterpret_cast<u32x4_u*>(dst + 16 * c) = *reinterpret_cast<const u32x4_u*>(src + 16 * c);
  for (uint64_t x = 16 * chunks + threadIdx.x; x < len; x += blockDim.x) dst[x] = src[x];
}

__global__ void get_publish_kernel(const uint32_t* list, uint32_t nc, const uint8_t* out, const uint64_t* out_off,
                                   const slate_block_meta* meta, uint32_t* bflag, uint64_t* bdata,
                                   slate_block_meta* bmeta) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  const uint32_t b = list[i];
  bmeta[b] = meta[i];
  bdata[b] = uint64_t(reinterpret_cast<uintptr_t>(out + out_off[i]));
  bflag[b] = 2;
}

__global__ __launch_bounds__(256) void get_fetch_kernel(GetSst s, GetQ q, const uint32_t* pend, uint32_t np,
                                                        const uint64_t* bdata, const slate_block_meta* bmeta,
                                                        slate_seek* seek, uint32_t* pend_next, uint32_t* cnt) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  bool want = false;
  uint32_t qi = 0;
  if (k < np) {
    qi = pend[k];
    const uint32_t b = q.qblk[qi];
    if (b != kGetDone) {
      // bdata holds addresses: block b's Data = (uint8_t*)0 + bdata[b]
      seek_one(qi, nullptr, bdata, bmeta, q.qblk, q.keys, q.key_off, seek, nullptr, 0);
      const slate_seek sk = seek[qi];
      slate_get_result r = q.res[qi];
      uint64_t vsrc = 0;
      bool fin = true;
      if (sk.status != SLATE_OK) {  // the block's decode status, or the seek's
        end_error(r, sk.status, s.sst);
      } else {
        const slate_block_meta m = bmeta[b];
        const uint8_t* key = q.keys + q.key_off[qi];
        const uint32_t kl = uint32_t(q.key_off[qi + 1] - q.key_off[qi]);
        fin = get_row(reinterpret_cast<const uint8_t*>(uintptr_t(bdata[b])), m.data_len, m.n_rows, sk, key, kl, s.sst,
                      b, r, &vsrc);
      }
      q.res[qi] = r;
      if (fin) {
        q.vsrc[qi] = vsrc;
        q.qblk[qi] = kGetDone;
      } else {
        q.qblk[qi] = b + 1;
        want = true;
      }
    }
  }
  const uint32_t pos = wave_append(cnt + kGcPend, want);
  if (want) pend_next[pos] = qi;
}

__global__ __launch_bounds__(256) void get_active_kernel(GetQ q, const uint32_t* act, uint64_t na, uint32_t* act_next,
                                                         uint32_t* cnt) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool want = false;
  uint32_t qi = 0;
  if (i < na) {
    qi = act ? act[i] : uint32_t(i);
    want = q.res[qi].outcome == SLATE_GET_MISS;
  }
  const uint32_t pos = wave_append(cnt + kGcAct, want);
  if (want) act_next[pos] = qi;
}

// ---------------------------------------------------------------- values
constexpr uint32_t kScanThreads = 256, kScanPer = 8, kScanTile = kScanThreads * kScanPer;

__global__ __launch_bounds__(kScanThreads) void get_vsum_kernel(GetQ q, uint64_t* part) {
  __shared__ uint64_t sh[kScanThreads];
  const uint64_t i0 = (uint64_t(blockIdx.x) * kScanThreads + threadIdx.x) * kScanPer;
  uint64_t v = 0;
  for (uint32_t u = 0; u < kScanPer; u++)
    if (i0 + u < q.n) v += q.res[i0 + u].value_len;
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t d = kScanThreads / 2; d; d >>= 1) {
    if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// part[0..np) -> exclusive scan in place; the total to val_off[n]
__global__ __launch_bounds__(1024) void get_vparts_kernel(uint64_t* part, uint32_t np, uint64_t* total) {
  __shared__ uint64_t sh[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t chunk = (np + 1023) / 1024;
  const uint32_t lo = min(np, t * chunk), hi = min(np, lo + chunk);
  uint64_t v = 0;
  for (uint32_t i = lo; i < hi; i++) v += part[i];
  sh[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint64_t p = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += p;
    __syncthreads();
  }
  uint64_t run = sh[t] - v;
  for (uint32_t i = lo; i < hi; i++) {
    const uint64_t x = part[i];
    part[i] = run;
    run += x;
  }
  if (t == 1023) *total = sh[t];
}

__global__ __launch_bounds__(kScanThreads) void get_vwrite_kernel(GetQ q, const uint64_t* part, uint64_t* val_off) {
  __shared__ uint64_t sh[kScanThreads];
  const uint32_t t = threadIdx.x;
  const uint64_t i0 = (uint64_t(blockIdx.x) * kScanThreads + t) * kScanPer;
  uint32_t vl[kScanPer];
  uint64_t v = 0;
  for (uint32_t u = 0; u < kScanPer; u++) {
    vl[u] = i0 + u < q.n ? q.res[i0 + u].value_len : 0u;
    v += vl[u];
  }
  sh[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
    const uint64_t p = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += p;
    __syncthreads();
  }
  uint64_t run = part[blockIdx.x] + sh[t] - v;
  for (uint32_t u = 0; u < kScanPer; u++) {
    if (i0 + u < q.n) val_off[i0 + u] = run;
    run += vl[u];
  }
}

// value i to vals + val_off[i]: eight lanes per value, 16 bytes per lane and step
__global__ __launch_bounds__(256) void get_copy_kernel(GetQ q, const uint64_t* val_off, uint8_t* vals) {
  const uint64_t i = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) / 8;
  const uint32_t sub = threadIdx.x & 7;
  if (i >= q.n) return;
  const uint32_t vl = q.res[i].value_len;
  if (vl == 0) return;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(uintptr_t(q.vsrc[i]));
  uint8_t* dst = vals + val_off[i];
  for (uint32_t o = sub * 16; o < vl; o += 128) {
    if (o + 16 <= vl) {
      *reinterpret_cast<u32x4_u*>(dst + o) = *reinterpret_cast<const u32x4_u*>(src + o);
    } else {
      for (uint32_t x = o; x < vl; x++) dst[x] = src[x];
    }
  }
}

}  // namespace

hipError_t launch_get_init(hipStream_t st, const GetQ& q, uint32_t n_sst) {
  if (q.n == 0) return hipSuccess;
  get_init_kernel<<<uint32_t((q.n + 255) / 256), 256, 0, st>>>(q, n_sst);
  return hipGetLastError();
}

hipError_t launch_get_locate(hipStream_t st, const GetSst& s, const GetQ& q, const uint32_t* act, uint64_t na,
                             uint32_t* pend, uint32_t* cnt) {
  if (na == 0) return hipSuccess;
  get_locate_kernel<<<uint32_t((na + 255) / 256), 256, 0, st>>>(s, q, act, na, pend, cnt);
  return hipGetLastError();
}

hipError_t launch_get_fused(hipStream_t st, const GetSst& s, const GetQ& q, const uint32_t* pend, uint32_t np,
                            uint32_t* gen, uint32_t* cnt, int num_cus) {
  if (np == 0) return hipSuccess;
  // four workgroups per CU fit LDS (36.3 KiB each of 160 KiB); queries beyond the grid are taken by stride
  const uint32_t grid = min((np + kFusedWaves - 1) / kFusedWaves, uint32_t(max(num_cus, 1)) * 4u);
  get_fused_kernel<<<grid, kFusedThreads, 0, st>>>(s, q, pend, np, gen, cnt);
  return hipGetLastError();
}

hipError_t launch_get_mark(hipStream_t st, const GetSst& s, const GetQ& q, const uint32_t* pend, uint32_t np,
                           uint32_t* bflag) {
  if (np == 0) return hipSuccess;
  get_mark_kernel<<<(np + 255) / 256, 256, 0, st>>>(s, q, pend, np, bflag);
  return hipGetLastError();
}

hipError_t launch_get_compact(hipStream_t st, const GetSst& s, const uint32_t* bflag, uint32_t* list, uint64_t* in_off,
                              uint32_t* cnt) {
  get_compact_kernel<<<1, kCompactThreads, 0, st>>>(s, bflag, list, in_off, cnt);
  return hipGetLastError();
}

hipError_t launch_get_gather(hipStream_t st, const GetSst& s, const uint32_t* list, const uint64_t* in_off, uint32_t nc,
                             uint8_t* gin) {
  if (nc == 0) return hipSuccess;
  get_gather_kernel<<<nc, 256, 0, st>>>(s, list, in_off, gin);
  return hipGetLastError();
}

hipError_t launch_get_publish(hipStream_t st, const uint32_t* list, uint32_t nc, const uint8_t* out,
                              const uint64_t* out_off, const slate_block_meta* meta, uint32_t* bflag, uint64_t* bdata,
                              slate_block_meta* bmeta) {
  if (nc == 0) return hipSuccess;
  get_publish_kernel<<<(nc + 255) / 256, 256, 0, st>>>(list, nc, out, out_off, meta, bflag, bdata, bmeta);
  return hipGetLastError();
}

hipError_t launch_get_fetch(hipStream_t st, const GetSst& s, const GetQ& q, const uint32_t* pend, uint32_t np,
                            const uint64_t* bdata, const slate_block_meta* bmeta, slate_seek* seek, uint32_t* pend_next,
                            uint32_t* cnt) {
  if (np == 0) return hipSuccess;
  get_fetch_kernel<<<(np + 255) / 256, 256, 0, st>>>(s, q, pend, np, bdata, bmeta, seek, pend_next, cnt);
  return hipGetLastError();
}

hipError_t launch_get_active(hipStream_t st, const GetQ& q, const uint32_t* act, uint64_t na, uint32_t* act_next,
                             uint32_t* cnt) {
  if (na == 0) return hipSuccess;
  get_active_kernel<<<uint32_t((na + 255) / 256), 256, 0, st>>>(q, act, na, act_next, cnt);
  return hipGetLastError();
}

size_t get_scan_parts(uint64_t n) { return size_t((n + kScanTile - 1) / kScanTile) + 1; }

hipError_t launch_get_val_scan(hipStream_t st, const GetQ& q, uint64_t* val_off, uint64_t* part) {
  if (q.n == 0) return hipMemsetAsync(val_off, 0, 8, st);
  const uint32_t tiles = uint32_t((q.n + kScanTile - 1) / kScanTile);
  get_vsum_kernel<<<tiles, kScanThreads, 0, st>>>(q, part);
  get_vparts_kernel<<<1, 1024, 0, st>>>(part, tiles, val_off + q.n);
  get_vwrite_kernel<<<tiles, kScanThreads, 0, st>>>(q, part, val_off);
  return hipGetLastError();
}

hipError_t launch_get_copy(hipStream_t st, const GetQ& q, const uint64_t* val_off, uint8_t* vals) {
  if (q.n == 0) return hipSuccess;
  get_copy_kernel<<<uint32_t((q.n * 8 + 255) / 256), 256, 0, st>>>(q, val_off, vals);
  return hipGetLastError();
}

}  // namespace slate
