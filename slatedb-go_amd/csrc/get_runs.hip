// Batched point reads over sorted runs (slate_sst_get_batch_runs): DB.GetWithOptions' walk through
// snapshot.Core.Compacted (slatedb/db.go:252-265) for n keys at once.  A run is one sorted key
// space; its blocks are numbered across its SSTs (global block = blk_base[p] + b) and every step
// below is one launch per run, whatever the number of SSTs in it.
//   get_run_locate_kernel  srMayIncludeKey (db.go:303-315): sort.Search over the SSTs' first keys
//                      with Go's probe sequence (compacted/sortedrun.go:24-41; a probed empty first
//                      key is the assert's panic), the chosen SST's filter, and
//                      firstBlockIncludingOrAfterKey in it; one thread per query;
//   get_run_fused_kernel   CodecNone SSTs: one wave per query walks SortedRunIterator.Next
//                      (sortedrun.go:113-145) -- the per-block body of get_fused_kernel
//                      (get_common.h fused_block), and when an SST's iterator ends without a row,
//                      the next SST from block 0 with block.NewIterator (no seek, firstKey nil);
//                      a block over 2 048 rows or an SST of another codec hands the query over;
//   general path       get_run_mark_kernel steps each pending query over SSTs that have ended
//                      (out of blocks, a rejected range), finishes those past the run's last SST
//                      and marks the global block the others read; get_run_compact_kernel lists
//                      the marked blocks of one codec (the host loops over the run's codec set);
//                      get_run_gather_kernel copies them back to back; the block decode kernels
//                      and get_publish_kernel are those of get.hip; get_run_fetch_kernel seeks
//                      (seek_one) or, from-start, takes row 0, fetches, and appends a query that
//                      got no row to the next round with block + 1, or SST + 1 and block 0.
// What is expected to bound them -- UNMEASURED: no counter profile of these kernels exists yet,
// this is read from the code.  locate is a dependent chain of scattered loads (two binary searches
// and the filter's probes per query): latency, hidden by the batch.  The fused kernel is bound as
// get_fused_kernel is, by the CRC's LDS table lookups over each visited block (4 KiB read once per
// query, L2 hits for queries that share a block); a walk-on adds one more block per query.  mark
// and fetch are scattered loads per query; compact is one workgroup's scan over the run's block
// count; gather is a streaming copy.
#include "get_common.h"

namespace slate {

namespace {

// An error noted or a panic raised in SST p of the run since `had` was taken
__device__ inline void note_run_pos(const slate_get_result& r, bool had, uint32_t p, slate_get_run_pos& pos) {
  if (r.outcome == SLATE_GET_PANIC || (!had && r.err != SLATE_OK)) pos.err_run_sst = p;
}

__global__ __launch_bounds__(256) void get_run_locate_kernel(GetRun run, GetQ q, GetRunQ rq, const uint32_t* act,
                                                             uint64_t na, uint32_t* pend, uint32_t* cnt) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool want = false;
  uint32_t qi = 0;
  if (i < na) {
    qi = act ? act[i] : uint32_t(i);
    const uint8_t* key = q.keys + q.key_off[qi];
    const uint32_t kl = uint32_t(q.key_off[qi + 1] - q.key_off[qi]);
    slate_get_result r = q.res[qi];
    slate_get_run_pos pos = rq.pos[qi];
    r.block = 0;
    r.row = 0;
    pos.run_sst = 0;
    // sort.Search(len(SSTList), FirstKey[i] > key) (sortedrun.go:24-28)
    uint32_t lo = 0, hi = run.n_sst;
    bool panic = false;
    while (lo < hi) {
      const uint32_t h = (lo + hi) >> 1;
      const uint32_t fl = uint32_t(run.fk_off[h + 1] - run.fk_off[h]);
      if (fl == 0) {  // assert.True(len(FirstKey) != 0, "sst must have first key")
        panic = true;
        r.stage = SLATE_GET_AT_RANGE;
        set_panic(r, SLATE_E_RUN_FIRSTKEY_PANIC, run.src);
        pos.err_run_sst = h;
        break;
      }
      if (!(cmp_bytes(run.fkeys + run.fk_off[h], fl, key, kl) > 0)) lo = h + 1;
      else hi = h;
    }
    if (panic) {
    } else if (lo == 0) {
      r.stage = SLATE_GET_AT_RANGE;
    } else {
      const uint32_t p = lo - 1;
      const GetSst& s = run.views[p];
      pos.run_sst = p;
      if (s.has_filter && !sst_filter_has_key(s, key, kl)) {
        r.stage = SLATE_GET_AT_FILTER;
      } else {
        // (an SST without blocks ends at once and the walk goes on: the fused / mark kernels see it)
        q.qblk[qi] = s.nb ? sst_first_block(s, key, kl) : 0u;
        rq.qsst[qi] = p;
        r.stage = SLATE_GET_AT_END;  // (overwritten when the iteration ends)
        want = true;
      }
    }
    q.res[qi] = r;
    rq.pos[qi] = pos;
  }
  const uint32_t at = wave_append(cnt + kGcPend, want);
  if (want) pend[at] = qi;
}

__global__ __launch_bounds__(kFusedThreads) void get_run_fused_kernel(GetRun run, GetQ q, GetRunQ rq,
                                                                      const uint32_t* pend, uint32_t np, uint32_t* gen,
                                                                      uint32_t* cnt) {
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
    slate_get_run_pos pos = rq.pos[qi];
    uint64_t vsrc = 0;
    uint32_t b = q.qblk[qi];
    uint32_t p = rq.qsst[qi] & ~kRunFromStart;
    bool from_start = (rq.qsst[qi] & kRunFromStart) != 0;
    bool handed = false;
    for (;;) {  // SortedRunIterator.Next (sortedrun.go:113-145); every value below is wave-uniform
      if (p >= run.n_sst) {  // the run ended: the stage is what the last SST's iterator left
        pos.run_sst = run.n_sst - 1;
        break;
      }
      if (run.codec[p] != SLATE_CODEC_NONE) {
        handed = true;
        break;
      }
      const GetSst& s = run.views[p];
      int w = kBlkEnd;
      if (b >= s.nb) {
        r.stage = SLATE_GET_AT_END;
      } else {
        const bool had = r.err != SLATE_OK;
        w = fused_block(s, b, from_start, tab, wls[wave], lane, q, qi, key, kl, run.src, r, &vsrc);
        note_run_pos(r, had, p, pos);
      }
      if (w == kBlkHand) {
        handed = true;
        break;
      }
      if (w == kBlkRow || r.outcome == SLATE_GET_PANIC) {
        pos.run_sst = p;
        break;
      }
      if (w == kBlkNext) {
        b++;
      } else {  // this SST's iterator ended without a row: sstable.NewIterator on the next one
        p++;
        b = 0;
        from_start = true;
      }
    }
    if (lane == 0) {
      q.res[qi] = r;  // (handed: an err noted on the way here stays)
      rq.pos[qi] = pos;
      if (handed) {
        q.qblk[qi] = b;
        rq.qsst[qi] = p | (from_start ? kRunFromStart : 0u);
        gen[atomicAdd(cnt + kGcGen, 1u)] = qi;
      } else {
        q.vsrc[qi] = vsrc;
        q.qblk[qi] = kGetDone;
        done++;
      }
    }
  }
  if (lane == 0 && done) atomicAdd(cnt + kGcFused, done);
}

// ---------------------------------------------------------------- general path
__global__ void get_run_mark_kernel(GetRun run, GetQ q, GetRunQ rq, const uint32_t* pend, uint32_t np,
                                    uint32_t* bflag) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= np) return;
  const uint32_t qi = pend[k];
  uint32_t b = q.qblk[qi];
  if (b == kGetDone) return;
  uint32_t p = rq.qsst[qi] & ~kRunFromStart;
  bool from_start = (rq.qsst[qi] & kRunFromStart) != 0;
  bool stepped = false;
  slate_get_result r = q.res[qi];
  slate_get_run_pos pos = rq.pos[qi];
  while (p < run.n_sst) {
    const GetSst& s = run.views[p];
    if (b >= s.nb) {
      r.stage = SLATE_GET_AT_END;
    } else if (s.bbad[b]) {
      const bool had = r.err != SLATE_OK;
      end_error(r, SLATE_E_BLOB_RANGE, run.src);
      note_run_pos(r, had, p, pos);
    } else {
      break;
    }
    stepped = true;
    p++;
    b = 0;
    from_start = true;
  }
  if (stepped) {
    q.res[qi] = r;
    rq.pos[qi] = pos;
  }
  if (p >= run.n_sst) {
    rq.pos[qi].run_sst = run.n_sst - 1;
    q.qblk[qi] = kGetDone;
    return;
  }
  if (stepped) {
    q.qblk[qi] = b;
    rq.qsst[qi] = p | (from_start ? kRunFromStart : 0u);
  }
  const uint32_t gb = run.blk_base[p] + b;
  rq.qgb[qi] = gb;
  if (bflag[gb] == 0) bflag[gb] = 1;  // (every writer stores the same value)
}

__device__ inline uint64_t run_block_len(const GetRun& run, uint32_t gb) {
  const uint32_t p = run.bsst[gb];
  const uint32_t b = gb - run.blk_base[p];
  return run.views[p].bend[b] - run.views[p].bstart[b];
}

constexpr int kCompactThreads = 1024;
__global__ __launch_bounds__(kCompactThreads) void get_run_compact_kernel(GetRun run, uint32_t codec,
                                                                          const uint32_t* bflag, uint32_t* list,
                                                                          uint64_t* in_off, uint32_t* cnt) {
  __shared__ uint32_t sc[kCompactThreads];
  __shared__ uint64_t sl[kCompactThreads];
  const uint32_t t = threadIdx.x;
  const uint32_t chunk = (run.nblk + kCompactThreads - 1) / kCompactThreads;
  // (64-bit products: nblk may be close to 2^32)
  const uint64_t lo64 = uint64_t(t) * chunk < run.nblk ? uint64_t(t) * chunk : run.nblk;
  const uint32_t lo = uint32_t(lo64), hi = uint32_t(lo64 + chunk < run.nblk ? lo64 + chunk : run.nblk);
  uint32_t c = 0;
  uint64_t l = 0;
  for (uint32_t b = lo; b < hi; b++)
    if (bflag[b] == 1 && run.codec[run.bsst[b]] == codec) {
      c++;
      l += run_block_len(run, b);
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
    if (bflag[b] == 1 && run.codec[run.bsst[b]] == codec) {
      list[pos] = b;
      in_off[pos] = lp;
      pos++;
      lp += run_block_len(run, b);
    }
  if (t == kCompactThreads - 1) {
    in_off[sc[t]] = sl[t];
    cnt[kGcBlocks] = sc[t];
    cnt[kGcBytesLo] = uint32_t(sl[t]);
    cnt[kGcBytesHi] = uint32_t(sl[t] >> 32);
  }
}

// global block list[i]'s encoded bytes to gin + in_off[i]: one workgroup per block, 16 bytes per lane
__global__ __launch_bounds__(256) void get_run_gather_kernel(GetRun run, const uint32_t* list, const uint64_t* in_off,
                                                             uint8_t* gin) {
  const uint32_t i = blockIdx.x;
  const uint32_t gb = list[i];
  const uint32_t p = run.bsst[gb];
  const uint32_t b = gb - run.blk_base[p];
  const GetSst& s = run.views[p];
  const uint8_t* src = s.region + s.bstart[b];
  uint8_t* dst = gin + in_off[i];
  const uint64_t len = s.bend[b] - s.bstart[b];
  const uint64_t chunks = len / 16;
  for (uint64_t c = threadIdx.x; c < chunks; c += blockDim.x)
    *reinterpret_cast<u32x4_u*>(dst + 16 * c) = *reinterpret_cast<const u32x4_u*>(src + 16 * c);
  for (uint64_t x = 16 * chunks + threadIdx.x; x < len; x += blockDim.x) dst[x] = src[x];
}

__global__ __launch_bounds__(256) void get_run_fetch_kernel(GetRun run, GetQ q, GetRunQ rq, const uint32_t* pend,
                                                            uint32_t np, const uint64_t* bdata,
                                                            const slate_block_meta* bmeta, slate_seek* seek,
                                                            uint32_t* pend_next, uint32_t* cnt) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  bool want = false;
  uint32_t qi = 0;
  if (k < np) {
    qi = pend[k];
    const uint32_t b = q.qblk[qi];
    if (b != kGetDone) {
      const uint32_t p = rq.qsst[qi] & ~kRunFromStart;
      const bool from_start = (rq.qsst[qi] & kRunFromStart) != 0;
      const uint32_t gb = rq.qgb[qi];
      const slate_block_meta m = bmeta[gb];
      slate_seek sk{};  // from-start: block.NewIterator -- offsetIndex 0, firstKey nil
      if (from_start) {
        sk.status = m.status;
      } else {
        // bdata holds addresses: global block gb's Data = (uint8_t*)0 + bdata[gb]
        seek_one(qi, nullptr, bdata, bmeta, rq.qgb, q.keys, q.key_off, seek, nullptr, 0);
        sk = seek[qi];
      }
      slate_get_result r = q.res[qi];
      slate_get_run_pos pos = rq.pos[qi];
      uint64_t vsrc = 0;
      const bool had = r.err != SLATE_OK;
      bool fin, ended = false;
      if (sk.status != SLATE_OK) {  // the block's decode status, or the seek's: this SST's iterator ends
        end_error(r, sk.status, run.src);
        fin = r.outcome == SLATE_GET_PANIC;
        ended = true;
      } else {
        const uint8_t* key = q.keys + q.key_off[qi];
        const uint32_t kl = uint32_t(q.key_off[qi + 1] - q.key_off[qi]);
        fin = get_row(reinterpret_cast<const uint8_t*>(uintptr_t(bdata[gb])), m.data_len, m.n_rows, sk, key, kl,
                      run.src, b, r, &vsrc);
      }
      note_run_pos(r, had, p, pos);
      if (fin) {
        pos.run_sst = p;
        q.vsrc[qi] = vsrc;
        q.qblk[qi] = kGetDone;
      } else if (ended) {
        q.qblk[qi] = 0;
        rq.qsst[qi] = (p + 1) | kRunFromStart;
        want = true;
      } else {
        q.qblk[qi] = b + 1;
        want = true;
      }
      q.res[qi] = r;
      rq.pos[qi] = pos;
    }
  }
  const uint32_t at = wave_append(cnt + kGcPend, want);
  if (want) pend_next[at] = qi;
}

}  // namespace

hipError_t launch_get_run_locate(hipStream_t st, const GetRun& run, const GetQ& q, const GetRunQ& rq,
                                 const uint32_t* act, uint64_t na, uint32_t* pend, uint32_t* cnt) {
  if (na == 0) return hipSuccess;
  get_run_locate_kernel<<<uint32_t((na + 255) / 256), 256, 0, st>>>(run, q, rq, act, na, pend, cnt);
  return hipGetLastError();
}

hipError_t launch_get_run_fused(hipStream_t st, const GetRun& run, const GetQ& q, const GetRunQ& rq,
                                const uint32_t* pend, uint32_t np, uint32_t* gen, uint32_t* cnt, int num_cus) {
  if (np == 0) return hipSuccess;
  // the grid of launch_get_fused: four workgroups per CU fit LDS, queries beyond it are taken by stride
  const uint32_t grid = min((np + kFusedWaves - 1) / kFusedWaves, uint32_t(max(num_cus, 1)) * 4u);
  get_run_fused_kernel<<<grid, kFusedThreads, 0, st>>>(run, q, rq, pend, np, gen, cnt);
  return hipGetLastError();
}

hipError_t launch_get_run_mark(hipStream_t st, const GetRun& run, const GetQ& q, const GetRunQ& rq,
                               const uint32_t* pend, uint32_t np, uint32_t* bflag) {
  if (np == 0) return hipSuccess;
  get_run_mark_kernel<<<(np + 255) / 256, 256, 0, st>>>(run, q, rq, pend, np, bflag);
  return hipGetLastError();
}

hipError_t launch_get_run_compact(hipStream_t st, const GetRun& run, uint32_t codec, const uint32_t* bflag,
                                  uint32_t* list, uint64_t* in_off, uint32_t* cnt) {
  get_run_compact_kernel<<<1, kCompactThreads, 0, st>>>(run, codec, bflag, list, in_off, cnt);
  return hipGetLastError();
}

hipError_t launch_get_run_gather(hipStream_t st, const GetRun& run, const uint32_t* list, const uint64_t* in_off,
                                 uint32_t nc, uint8_t* gin) {
  if (nc == 0) return hipSuccess;
  get_run_gather_kernel<<<nc, 256, 0, st>>>(run, list, in_off, gin);
  return hipGetLastError();
}

hipError_t launch_get_run_fetch(hipStream_t st, const GetRun& run, const GetQ& q, const GetRunQ& rq,
                                const uint32_t* pend, uint32_t np, const uint64_t* bdata, const slate_block_meta* bmeta,
                                slate_seek* seek, uint32_t* pend_next, uint32_t* cnt) {
  if (np == 0) return hipSuccess;
  get_run_fetch_kernel<<<(np + 255) / 256, 256, 0, st>>>(run, q, rq, pend, np, bdata, bmeta, seek, pend_next, cnt);
  return hipGetLastError();
}

}  // namespace slate
