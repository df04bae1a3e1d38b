// C-ABI: batched point reads (slatedb/db.go:237-250 over SSTs held in HBM): slate_sst_open /
// slate_sst_close / slate_sst_handle_info, slate_sst_get_batch, slate_sst_get_counters; and the
// sorted runs of db.go:252-265: slate_sorted_run_create / _free / _info and
// slate_sst_get_batch_runs, of which slate_sst_get_batch is the call without runs.
//
// A handle keeps, in HBM of its context's GPU (the footprint slate_sst_handle_info reports):
//   region   the object's bytes from the lowest valid block start to the highest valid block end
//            (a well-formed SST: its data blocks, once), 64 bytes of slack after them;
//   aux      per block its range ends in the region (2 x u64) and a flag for a range
//            bytesBlob.ReadRange rejects (1 byte), the index's first keys and their offsets
//            (8 bytes per block + 8), the decoded filter bits, the info's first key -- each array
//            rounded up to 256 bytes.
// Everything between the upload of the keys and the download of the results runs on the
// context's stream; the host waits only to read a round's counters (the pending count, and on the
// general path the number and size of the blocks to decode and the plan's totals, which size the
// round's buffers).
#include <algorithm>
#include <cstring>
#include <vector>

#include "host_ctx.h"

using namespace slate;

static_assert(SLATE_E_RUN_FIRSTKEY_PANIC == 65, "the ABI's value of SLATE_E_RUN_FIRSTKEY_PANIC");

struct slate_sst_handle {
  int device = 0;
  slate_sst_info info{};
  std::vector<uint8_t> first_key;
  uint64_t nb = 0;
  int filter_present = 0, filter_status = SLATE_OK;
  uint64_t device_bytes = 0;
  void* region_base = nullptr;  // hipMalloc: kDevGuard bytes, the region, 64 bytes of slack
  void* aux_base = nullptr;
  GetSst view{};
};

namespace {

// One block's byte range in the object (getBlockRange, decode.go:93-103, for [i, i + 1)) and
// whether bytesBlob.ReadRange accepts it (blob.go:23-26).
struct BlockRange {
  uint64_t start, end;
  bool ok;
};
BlockRange block_range(const std::vector<uint64_t>& offs, size_t i, uint64_t filter_offset, uint64_t sst_len) {
  BlockRange r;
  r.start = offs[i];
  r.end = i + 1 < offs.size() ? offs[i + 1] : filter_offset;
  r.ok = r.start <= sst_len && r.end <= sst_len && r.start <= r.end;
  return r;
}

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

// reads the call's counter words back (the host's only wait inside a call)
int read_cnt(slate_ctx* ctx, hipStream_t st, uint32_t* h) {
  SLATE_HIP(hipMemcpyAsync(h, ctx->get.cnt.p, kGcWords * 4, hipMemcpyDeviceToHost, st));
  SLATE_HIP(hipStreamSynchronize(st));
  return SLATE_OK;
}

// The nc blocks listed in g.list, gathered back to back in g.gin (in_bytes, offsets g.in_off):
// decode them as one batch into a buffer of their own (g.outs, kept until the values are copied)
// and publish each block's decoded address and meta (bflag 2, bdata, bmeta).
int decode_gathered(slate_ctx* ctx, hipStream_t st, int codec, uint32_t nc, uint64_t in_bytes, size_t* round_buf) {
  auto& g = ctx->get;
  SLATE_HIP(g.out_off.ensure((size_t(nc) + 1) * 8));
  SLATE_HIP(g.row_base.ensure((size_t(nc) + 1) * 8));
  SLATE_HIP(g.scr.ensure(decode_scratch_bytes_codec(nc, codec) + 64));
  SLATE_HIP(g.meta.ensure(size_t(nc) * sizeof(slate_block_meta)));
  SLATE_HIP(hipMemsetAsync(g.gin.as<uint8_t>() + in_bytes, 0, 64, st));
  SLATE_HIP(launch_decode_plan(st, codec, g.gin.as<uint8_t>(), g.in_off.as<uint64_t>(), nc, g.out_off.as<uint64_t>(),
                               g.row_base.as<uint64_t>(), g.scr.p));
  uint64_t tot[2] = {0, 0};
  SLATE_HIP(hipMemcpyAsync(&tot[0], g.out_off.as<uint64_t>() + nc, 8, hipMemcpyDeviceToHost, st));
  SLATE_HIP(hipMemcpyAsync(&tot[1], g.row_base.as<uint64_t>() + nc, 8, hipMemcpyDeviceToHost, st));
  SLATE_HIP(hipStreamSynchronize(st));
  if (*round_buf == g.outs.size()) g.outs.emplace_back();
  DevBuf& out = g.outs[(*round_buf)++];
  SLATE_HIP(out.ensure(tot[0] + 64));
  SLATE_HIP(g.rows.ensure((tot[1] + 1) * sizeof(slate_row)));
  DecodeArgs a{codec, g.gin.as<uint8_t>(), g.in_off.as<uint64_t>(), nc, out.as<uint8_t>(),
               g.out_off.as<uint64_t>(), g.meta.as<slate_block_meta>(), g.rows.as<slate_row>(),
               g.row_base.as<uint64_t>(), nullptr, nullptr, 0};
  a.side = &ctx->side;
  a.handbacks = ctx_handbacks(ctx);
  SLATE_HIP(launch_decode(st, a, g.scr.p, ctx->num_cus));
  SLATE_HIP(launch_get_publish(st, g.list.as<uint32_t>(), nc, out.as<uint8_t>(), g.out_off.as<uint64_t>(),
                               g.meta.as<slate_block_meta>(), g.bflag.as<uint32_t>(), g.bdata.as<uint64_t>(),
                               g.bmeta.as<slate_block_meta>()));
  g.n_blocks_decoded += nc;
  return SLATE_OK;
}

}  // namespace

// compacted.SortedRun over borrowed handles: the device arrays of GetRun in one allocation
struct slate_sorted_run {
  int device = 0;
  uint32_t n_sst = 0;
  uint64_t nblk = 0;
  uint64_t device_bytes = 0;
  void* base = nullptr;
  std::vector<int> codecs;  // the distinct codecs of its SSTs, ascending
  GetRun view{};
};

extern "C" {

int slate_sorted_run_create(slate_ctx* ctx, slate_sst_handle* const* ssts, uint32_t n_sst, slate_sorted_run** out) {
  if (!ctx || !out || (n_sst && !ssts)) return SLATE_E_INVALID_ARG;
  *out = nullptr;
  if (n_sst >= 0x80000000u) return SLATE_E_LIMIT;  // (bit 31 of a query's SST is its from-start flag)
  uint64_t nblk = 0, fkb = 0;
  for (uint32_t p = 0; p < n_sst; p++) {
    if (!ssts[p] || ssts[p]->device != ctx->device) return SLATE_E_INVALID_ARG;
    nblk += ssts[p]->nb;
    fkb += ssts[p]->first_key.size();
  }
  if (nblk >= 0x100000000ull) return SLATE_E_LIMIT;
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off += up256(bytes ? bytes : 1);
    return o;
  };
  const size_t o_v = carve(size_t(n_sst) * sizeof(GetSst)), o_fk = carve(fkb + 16), o_fo = carve((size_t(n_sst) + 1) * 8),
               o_bb = carve((size_t(n_sst) + 1) * 4), o_bs = carve(size_t(nblk) * 4), o_c = carve(n_sst);
  std::vector<uint8_t> img(off, 0);
  GetSst* views = reinterpret_cast<GetSst*>(img.data() + o_v);
  uint64_t* fo = reinterpret_cast<uint64_t*>(img.data() + o_fo);
  uint32_t* bb = reinterpret_cast<uint32_t*>(img.data() + o_bb);
  uint32_t* bs = reinterpret_cast<uint32_t*>(img.data() + o_bs);
  slate_sorted_run* r = new slate_sorted_run();
  uint64_t k = 0, g = 0;
  for (uint32_t p = 0; p < n_sst; p++) {
    const slate_sst_handle* h = ssts[p];
    views[p] = h->view;
    if (!h->first_key.empty()) memcpy(img.data() + o_fk + k, h->first_key.data(), h->first_key.size());
    fo[p] = k;
    k += h->first_key.size();
    bb[p] = uint32_t(g);
    for (uint64_t b = 0; b < h->nb; b++) bs[g + b] = p;
    g += h->nb;
    img[o_c + p] = uint8_t(h->info.codec);
    if (std::find(r->codecs.begin(), r->codecs.end(), int(h->info.codec)) == r->codecs.end())
      r->codecs.push_back(int(h->info.codec));
  }
  fo[n_sst] = k;
  bb[n_sst] = uint32_t(g);
  std::sort(r->codecs.begin(), r->codecs.end());
  r->device = ctx->device;
  r->n_sst = n_sst;
  r->nblk = nblk;
  hipError_t e = ctx_bind(ctx);
  if (e == hipSuccess) e = hipMalloc(&r->base, img.size());
  if (e != hipSuccess) {
    (void)hipGetLastError();
    delete r;
    return hip_status(e);
  }
  uint8_t* a = static_cast<uint8_t*>(r->base);
  int st = ctx_h2d(ctx, a, img.data(), img.size(), ctx->stream);
  if (!st && hipStreamSynchronize(ctx->stream) != hipSuccess) st = SLATE_E_HIP;
  if (st) {
    slate_sorted_run_free(r);
    return st;
  }
  r->device_bytes = img.size();
  GetRun& v = r->view;
  v.views = reinterpret_cast<const GetSst*>(a + o_v);
  v.fkeys = a + o_fk;
  v.fk_off = reinterpret_cast<const uint64_t*>(a + o_fo);
  v.blk_base = reinterpret_cast<const uint32_t*>(a + o_bb);
  v.bsst = reinterpret_cast<const uint32_t*>(a + o_bs);
  v.codec = a + o_c;
  v.n_sst = n_sst;
  v.nblk = uint32_t(nblk);
  v.src = 0;
  *out = r;
  return SLATE_OK;
}

void slate_sorted_run_free(slate_sorted_run* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  // hipFree synchronises the device: no kernel still reads the run afterwards
  if (r->base) (void)hipFree(r->base);
  delete r;
}

int slate_sorted_run_info(const slate_sorted_run* r, uint32_t* n_sst, uint64_t* n_blocks, uint64_t* device_bytes) {
  if (!r) return SLATE_E_INVALID_ARG;
  if (n_sst) *n_sst = r->n_sst;
  if (n_blocks) *n_blocks = r->nblk;
  if (device_bytes) *device_bytes = r->device_bytes;
  return SLATE_OK;
}

int slate_sst_open(slate_ctx* ctx, const uint8_t* sst, size_t sst_len, slate_sst_handle** out) {
  if (!ctx || !out || (sst_len && !sst)) return SLATE_E_INVALID_ARG;
  *out = nullptr;
  slate_sst_info info{};
  std::vector<uint8_t> fk;
  int st = slate_sst_read_info(sst, sst_len, &info, nullptr, 0);
  if (st == SLATE_E_CAPACITY) {
    fk.resize(info.first_key_len);
    st = slate_sst_read_info(sst, sst_len, &info, fk.data(), fk.size());
  }
  if (st) return st;
  // ReadIndex (decode.go:73-83): the range read, then DecodeIndex
  if (info.index_offset > sst_len || info.index_len > sst_len - info.index_offset) return SLATE_E_BLOB_RANGE;
  slate_index* index = nullptr;
  st = slate_decode_index(ctx, sst + info.index_offset, size_t(info.index_len), info.codec, &index);
  if (st) return st;
  const size_t nb = slate_index_num_blocks(index);
  std::vector<uint64_t> offs(nb);
  std::vector<uint8_t> ikeys;
  std::vector<uint64_t> ikey_off(nb + 1, 0);
  if (nb) (void)slate_index_block_offsets(index, offs.data(), nb);
  for (size_t i = 0; i < nb; i++) {
    const uint8_t* k = nullptr;
    size_t kl = 0;
    (void)slate_index_block_meta(index, i, nullptr, &k, &kl);
    ikeys.insert(ikeys.end(), k, k + kl);
    ikey_off[i + 1] = ikeys.size();
  }
  slate_index_free(index);
  if (nb >= 0xFFFFFFFFull) return SLATE_E_LIMIT;
  // ReadFilter (decode.go:50-71): absent, or present and decoded; an error means "may include"
  int filter_present = 0, filter_status = SLATE_OK;
  uint16_t num_probes = 0;
  std::vector<uint8_t> bits;
  if (info.filter_len >= 1) {
    if (info.filter_offset > sst_len || info.filter_len > sst_len - info.filter_offset) {
      filter_status = SLATE_E_BLOB_RANGE;
    } else {
      const uint8_t* fb = sst + info.filter_offset;
      size_t bl = 0;
      st = slate_bloom_decode(ctx, fb, size_t(info.filter_len), info.codec, &num_probes, nullptr, 0, &bl);
      if (st == SLATE_E_CAPACITY) {
        bits.resize(bl);
        st = slate_bloom_decode(ctx, fb, size_t(info.filter_len), info.codec, &num_probes, bits.data(), bl, &bl);
      }
      if (st >= SLATE_E_NO_DEVICE) return st;  // a runtime condition, not a verdict on the filter
      filter_status = st;
      filter_present = st == SLATE_OK;
      if (!filter_present) bits.clear();
    }
  }
  // the blocks' ranges and the region that holds the valid ones
  std::vector<uint64_t> bstart(nb, 0), bend(nb, 0);
  std::vector<uint8_t> bbad(nb, 0);
  uint64_t lo = UINT64_MAX, hi = 0;
  for (size_t i = 0; i < nb; i++) {
    const BlockRange r = block_range(offs, i, info.filter_offset, sst_len);
    if (!r.ok) {
      bbad[i] = 1;
      continue;
    }
    lo = std::min(lo, r.start);
    hi = std::max(hi, r.end);
  }
  if (lo > hi) lo = hi = 0;
  for (size_t i = 0; i < nb; i++) {
    if (bbad[i]) continue;
    const BlockRange r = block_range(offs, i, info.filter_offset, sst_len);
    bstart[i] = r.start - lo;
    bend[i] = r.end - lo;
  }
  const uint64_t region_len = hi - lo;
  // aux layout
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off += up256(bytes ? bytes : 1);
    return o;
  };
  const size_t o_bs = carve(nb * 8), o_be = carve(nb * 8), o_bad = carve(nb), o_ik = carve(ikeys.size() + 16),
               o_iko = carve((nb + 1) * 8), o_fb = carve(bits.size() + 16), o_fk = carve(fk.size() + 16);
  std::vector<uint8_t> aux(off, 0);
  if (nb) {
    memcpy(aux.data() + o_bs, bstart.data(), nb * 8);
    memcpy(aux.data() + o_be, bend.data(), nb * 8);
    memcpy(aux.data() + o_bad, bbad.data(), nb);
  }
  if (!ikeys.empty()) memcpy(aux.data() + o_ik, ikeys.data(), ikeys.size());
  memcpy(aux.data() + o_iko, ikey_off.data(), (nb + 1) * 8);
  if (!bits.empty()) memcpy(aux.data() + o_fb, bits.data(), bits.size());
  if (!fk.empty()) memcpy(aux.data() + o_fk, fk.data(), fk.size());

  SLATE_HIP(ctx_bind(ctx));
  slate_sst_handle* h = new slate_sst_handle();
  h->device = ctx->device;
  h->info = info;
  h->first_key = fk;
  h->nb = nb;
  h->filter_present = filter_present;
  h->filter_status = filter_status;
  hipError_t e = hipMalloc(&h->region_base, kDevGuard + region_len + 64);
  if (e == hipSuccess) e = hipMalloc(&h->aux_base, aux.size());
  if (e != hipSuccess) {
    (void)hipGetLastError();
    slate_sst_close(h);
    return hip_status(e);
  }
  uint8_t* region = static_cast<uint8_t*>(h->region_base) + kDevGuard;
  uint8_t* a = static_cast<uint8_t*>(h->aux_base);
  hipStream_t s = ctx->stream;
  st = region_len ? ctx_h2d(ctx, region, sst + lo, size_t(region_len), s) : SLATE_OK;
  if (!st) st = ctx_h2d(ctx, a, aux.data(), aux.size(), s);
  if (!st && hipMemsetAsync(region + region_len, 0, 64, s) != hipSuccess) st = SLATE_E_HIP;
  if (!st && hipStreamSynchronize(s) != hipSuccess) st = SLATE_E_HIP;
  if (st) {
    slate_sst_close(h);
    return st;
  }
  h->device_bytes = up256(size_t(region_len)) + aux.size();
  GetSst& v = h->view;
  v.region = region;
  v.bstart = reinterpret_cast<const uint64_t*>(a + o_bs);
  v.bend = reinterpret_cast<const uint64_t*>(a + o_be);
  v.bbad = a + o_bad;
  v.ikeys = a + o_ik;
  v.ikey_off = reinterpret_cast<const uint64_t*>(a + o_iko);
  v.fbits = a + o_fb;
  v.first_key = a + o_fk;
  v.fbits_len = bits.size();
  v.nb = uint32_t(nb);
  v.num_probes = num_probes;
  v.has_filter = filter_present ? 1u : 0u;
  v.first_key_len = uint32_t(fk.size());
  v.sst = 0;
  *out = h;
  return SLATE_OK;
}

void slate_sst_close(slate_sst_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  // hipFree synchronises the device: no kernel still reads the handle afterwards
  if (h->region_base) (void)hipFree(h->region_base);
  if (h->aux_base) (void)hipFree(h->aux_base);
  delete h;
}

int slate_sst_handle_info(const slate_sst_handle* h, slate_sst_info* info, uint8_t* first_key, size_t first_key_cap,
                          uint64_t* n_blocks, int* filter_present, int* filter_status, uint64_t* device_bytes) {
  if (!h) return SLATE_E_INVALID_ARG;
  if (info) *info = h->info;
  if (n_blocks) *n_blocks = h->nb;
  if (filter_present) *filter_present = h->filter_present;
  if (filter_status) *filter_status = h->filter_status;
  if (device_bytes) *device_bytes = h->device_bytes;
  if (first_key) {
    if (h->first_key.size() > first_key_cap) return SLATE_E_CAPACITY;
    if (!h->first_key.empty()) memcpy(first_key, h->first_key.data(), h->first_key.size());
  }
  return SLATE_OK;
}

int slate_sst_get_counters(slate_ctx* ctx, uint64_t* n_fused, uint64_t* n_general, uint64_t* n_rounds,
                           uint64_t* n_blocks_decoded, int reset) {
  if (!ctx) return SLATE_E_INVALID_ARG;
  auto& g = ctx->get;
  if (n_fused) *n_fused = g.n_fused;
  if (n_general) *n_general = g.n_general;
  if (n_rounds) *n_rounds = g.n_rounds;
  if (n_blocks_decoded) *n_blocks_decoded = g.n_blocks_decoded;
  if (reset) g.n_fused = g.n_general = g.n_rounds = g.n_blocks_decoded = 0;
  return SLATE_OK;
}

int slate_sst_get_batch(slate_ctx* ctx, slate_sst_handle* const* ssts, uint32_t n_sst, const uint8_t* keys,
                        const uint64_t* key_off, uint64_t n, slate_get_result* res, uint8_t* vals, uint64_t vals_cap,
                        uint64_t* val_off) {
  return slate_sst_get_batch_runs(ctx, ssts, n_sst, nullptr, 0, keys, key_off, n, res, nullptr, vals, vals_cap, val_off);
}

int slate_sst_get_batch_runs(slate_ctx* ctx, slate_sst_handle* const* ssts, uint32_t n_sst,
                             slate_sorted_run* const* runs, uint32_t n_run, const uint8_t* keys,
                             const uint64_t* key_off, uint64_t n, slate_get_result* res, slate_get_run_pos* pos,
                             uint8_t* vals, uint64_t vals_cap, uint64_t* val_off) {
  if (!ctx || (n_sst && !ssts) || (n_run && !runs)) return SLATE_E_INVALID_ARG;
  if (n == 0) {
    if (val_off) val_off[0] = 0;
    return SLATE_OK;
  }
  if (!key_off || !res || !val_off) return SLATE_E_INVALID_ARG;
  const uint64_t kb = key_off[n] - key_off[0];
  if (kb && !keys) return SLATE_E_INVALID_ARG;
  if (n >= 0xFFFFFFFFull) return SLATE_E_LIMIT;
  for (uint32_t j = 0; j < n_sst; j++)
    if (!ssts[j] || ssts[j]->device != ctx->device) return SLATE_E_INVALID_ARG;
  for (uint32_t r = 0; r < n_run; r++)
    if (!runs[r] || runs[r]->device != ctx->device) return SLATE_E_INVALID_ARG;
  const uint64_t n_src = uint64_t(n_sst) + n_run;
  if (n_src >= 0xFFFFFFFFull) return SLATE_E_LIMIT;
  SLATE_HIP(ctx_bind(ctx));
  hipStream_t st = ctx->stream;
  auto& g = ctx->get;
  SLATE_HIP(g.keys.ensure(kb + 16));
  SLATE_HIP(g.koff.ensure((n + 1) * 8));
  SLATE_HIP(g.res.ensure(n * sizeof(slate_get_result)));
  SLATE_HIP(g.vsrc.ensure(n * 8));
  SLATE_HIP(g.qblk.ensure(n * 4));
  SLATE_HIP(g.act0.ensure(n * 4));
  SLATE_HIP(g.act1.ensure(n * 4));
  SLATE_HIP(g.pend0.ensure(n * 4));
  SLATE_HIP(g.pend1.ensure(n * 4));
  SLATE_HIP(g.gen.ensure(n * 4));
  SLATE_HIP(g.seek.ensure(n * sizeof(slate_seek)));
  SLATE_HIP(g.cnt.ensure(kGcWords * 4));
  SLATE_HIP(g.voff.ensure((n + 1) * 8));
  SLATE_HIP(g.part.ensure(get_scan_parts(n) * 8));
  SLATE_HIP(g.h_cnt.ensure(kGcWords * 4));
  if (n_run) {
    SLATE_HIP(g.qsst.ensure(n * 4));
    SLATE_HIP(g.qgb.ensure(n * 4));
    SLATE_HIP(g.pos.ensure(n * sizeof(slate_get_run_pos)));
  }
  uint32_t* hc = g.h_cnt.as<uint32_t>();
  {
    std::vector<uint64_t> rel(n + 1);
    for (uint64_t i = 0; i <= n; i++) rel[i] = key_off[i] - key_off[0];
    int s = kb ? ctx_h2d(ctx, g.keys.p, keys + key_off[0], kb, st) : SLATE_OK;
    if (!s) s = ctx_h2d(ctx, g.koff.p, rel.data(), (n + 1) * 8, st);  // (synchronous: rel may go)
    if (s) return s;
  }
  GpuSpan span(ctx, st);  // device time of the lookups (slate_ctx_set_timing), the waits included
  GetQ q{g.keys.as<uint8_t>(), g.koff.as<uint64_t>(), n, g.res.as<slate_get_result>(), g.vsrc.as<uint64_t>(),
         g.qblk.as<uint32_t>()};
  uint32_t* cnt = g.cnt.as<uint32_t>();
  SLATE_HIP(launch_get_init(st, q, uint32_t(n_src)));
  if (n_run) SLATE_HIP(hipMemsetAsync(g.pos.p, 0, n * sizeof(slate_get_run_pos), st));
  const uint32_t* act = nullptr;  // nullptr: every query
  uint64_t na = n;
  uint32_t* act_next = g.act0.as<uint32_t>();
  size_t round_buf = 0;  // g.outs entries this call has used
  for (uint32_t j = 0; j < n_sst && na; j++) {
    GetSst s = ssts[j]->view;
    s.sst = j;
    const int codec = ssts[j]->info.codec;
    SLATE_HIP(hipMemsetAsync(cnt, 0, kGcWords * 4, st));
    uint32_t* cur = g.pend0.as<uint32_t>();
    uint32_t* other = g.pend1.as<uint32_t>();
    SLATE_HIP(launch_get_locate(st, s, q, act, na, cur, cnt));
    int rs = read_cnt(ctx, st, hc);
    if (rs) return rs;
    uint32_t np = hc[kGcPend];
    if (np && codec == SLATE_CODEC_NONE) {
      SLATE_HIP(launch_get_fused(st, s, q, cur, np, g.gen.as<uint32_t>(), cnt, ctx->num_cus));
      if ((rs = read_cnt(ctx, st, hc))) return rs;
      g.n_rounds++;
      g.n_fused += hc[kGcFused];
      np = hc[kGcGen];
      cur = g.gen.as<uint32_t>();  // the blocks the fused kernel refused; pend0 / pend1 alternate after it
      other = g.pend0.as<uint32_t>();
    }
    if (np) {
      g.n_general += np;
      const size_t nb = s.nb;
      SLATE_HIP(g.bflag.ensure(nb * 4));
      SLATE_HIP(g.bdata.ensure(nb * 8));
      SLATE_HIP(g.bmeta.ensure(nb * sizeof(slate_block_meta)));
      SLATE_HIP(g.list.ensure(nb * 4));
      SLATE_HIP(g.in_off.ensure((nb + 1) * 8));
      SLATE_HIP(hipMemsetAsync(g.bflag.p, 0, nb * 4, st));
    }
    while (np) {
      // one round: every pending query reads one block
      SLATE_HIP(launch_get_mark(st, s, q, cur, np, g.bflag.as<uint32_t>()));
      SLATE_HIP(launch_get_compact(st, s, g.bflag.as<uint32_t>(), g.list.as<uint32_t>(), g.in_off.as<uint64_t>(), cnt));
      if ((rs = read_cnt(ctx, st, hc))) return rs;
      const uint32_t nc = hc[kGcBlocks];
      if (nc) {
        const uint64_t in_bytes = uint64_t(hc[kGcBytesLo]) | (uint64_t(hc[kGcBytesHi]) << 32);
        SLATE_HIP(g.gin.ensure(in_bytes + 64));
        SLATE_HIP(launch_get_gather(st, s, g.list.as<uint32_t>(), g.in_off.as<uint64_t>(), nc, g.gin.as<uint8_t>()));
        if ((rs = decode_gathered(ctx, st, codec, nc, in_bytes, &round_buf))) return rs;
      }
      g.n_rounds++;
      SLATE_HIP(hipMemsetAsync(cnt + kGcPend, 0, 4, st));
      SLATE_HIP(launch_get_fetch(st, s, q, cur, np, g.bdata.as<uint64_t>(), g.bmeta.as<slate_block_meta>(),
                                 g.seek.as<slate_seek>(), other, cnt));
      if ((rs = read_cnt(ctx, st, hc))) return rs;
      np = hc[kGcPend];
      if (cur == g.gen.as<uint32_t>()) cur = g.pend1.as<uint32_t>();
      std::swap(cur, other);
    }
    if (j + 1 < n_src) {  // the queries no handle has answered yet go on to the next one
      SLATE_HIP(hipMemsetAsync(cnt + kGcAct, 0, 4, st));
      SLATE_HIP(launch_get_active(st, q, act, na, act_next, cnt));
      if ((rs = read_cnt(ctx, st, hc))) return rs;
      na = hc[kGcAct];
      act = act_next;
      act_next = act_next == g.act0.as<uint32_t>() ? g.act1.as<uint32_t>() : g.act0.as<uint32_t>();
    }
  }
  // the sorted runs (db.go:252-265): per run one locate, one fused pass, and rounds whose launch
  // count depends on the run's codec set, not on its SST count
  GetRunQ rq{g.qsst.as<uint32_t>(), g.qgb.as<uint32_t>(), g.pos.as<slate_get_run_pos>()};
  for (uint32_t ri = 0; ri < n_run && na; ri++) {
    const slate_sorted_run* sr = runs[ri];
    GetRun run = sr->view;
    run.src = n_sst + ri;
    SLATE_HIP(hipMemsetAsync(cnt, 0, kGcWords * 4, st));
    uint32_t* cur = g.pend0.as<uint32_t>();
    uint32_t* other = g.pend1.as<uint32_t>();
    SLATE_HIP(launch_get_run_locate(st, run, q, rq, act, na, cur, cnt));
    int rs = read_cnt(ctx, st, hc);
    if (rs) return rs;
    uint32_t np = hc[kGcPend];
    if (np && std::find(sr->codecs.begin(), sr->codecs.end(), int(SLATE_CODEC_NONE)) != sr->codecs.end()) {
      SLATE_HIP(launch_get_run_fused(st, run, q, rq, cur, np, g.gen.as<uint32_t>(), cnt, ctx->num_cus));
      if ((rs = read_cnt(ctx, st, hc))) return rs;
      g.n_rounds++;
      g.n_fused += hc[kGcFused];
      np = hc[kGcGen];
      cur = g.gen.as<uint32_t>();
      other = g.pend0.as<uint32_t>();
    }
    if (np) {
      g.n_general += np;
      const size_t nb = std::max<size_t>(run.nblk, 1);
      SLATE_HIP(g.bflag.ensure(nb * 4));
      SLATE_HIP(g.bdata.ensure(nb * 8));
      SLATE_HIP(g.bmeta.ensure(nb * sizeof(slate_block_meta)));
      SLATE_HIP(g.list.ensure(nb * 4));
      SLATE_HIP(g.in_off.ensure((nb + 1) * 8));
      SLATE_HIP(hipMemsetAsync(g.bflag.p, 0, nb * 4, st));
    }
    while (np) {
      // one round: every pending query reads one block; the touched blocks are decoded once per codec
      SLATE_HIP(launch_get_run_mark(st, run, q, rq, cur, np, g.bflag.as<uint32_t>()));
      bool decoded = false;
      for (int codec : sr->codecs) {
        SLATE_HIP(launch_get_run_compact(st, run, uint32_t(codec), g.bflag.as<uint32_t>(), g.list.as<uint32_t>(),
                                         g.in_off.as<uint64_t>(), cnt));
        if ((rs = read_cnt(ctx, st, hc))) return rs;
        const uint32_t nc = hc[kGcBlocks];
        if (!nc) continue;
        const uint64_t in_bytes = uint64_t(hc[kGcBytesLo]) | (uint64_t(hc[kGcBytesHi]) << 32);
        SLATE_HIP(g.gin.ensure(in_bytes + 64));
        SLATE_HIP(launch_get_run_gather(st, run, g.list.as<uint32_t>(), g.in_off.as<uint64_t>(), nc,
                                        g.gin.as<uint8_t>()));
        if ((rs = decode_gathered(ctx, st, codec, nc, in_bytes, &round_buf))) return rs;
        decoded = true;
      }
      if (decoded) g.n_rounds++;  // (a round that only steps queries over ended SSTs decodes nothing)
      SLATE_HIP(hipMemsetAsync(cnt + kGcPend, 0, 4, st));
      SLATE_HIP(launch_get_run_fetch(st, run, q, rq, cur, np, g.bdata.as<uint64_t>(), g.bmeta.as<slate_block_meta>(),
                                     g.seek.as<slate_seek>(), other, cnt));
      if ((rs = read_cnt(ctx, st, hc))) return rs;
      np = hc[kGcPend];
      if (cur == g.gen.as<uint32_t>()) cur = g.pend1.as<uint32_t>();
      std::swap(cur, other);
    }
    if (ri + 1 < n_run) {  // the queries no source has answered yet go on to the next run
      SLATE_HIP(hipMemsetAsync(cnt + kGcAct, 0, 4, st));
      SLATE_HIP(launch_get_active(st, q, act, na, act_next, cnt));
      if ((rs = read_cnt(ctx, st, hc))) return rs;
      na = hc[kGcAct];
      act = act_next;
      act_next = act_next == g.act0.as<uint32_t>() ? g.act1.as<uint32_t>() : g.act0.as<uint32_t>();
    }
  }
  SLATE_HIP(launch_get_val_scan(st, q, g.voff.as<uint64_t>(), g.part.as<uint64_t>()));
  span.stop();
  if (pos) {
    if (n_run) {
      const int ps = ctx_d2h(ctx, pos, g.pos.p, n * sizeof(slate_get_run_pos), st);
      if (ps) return ps;
    } else {
      memset(pos, 0, n * sizeof(slate_get_run_pos));
    }
  }
  int s = ctx_d2h(ctx, res, g.res.p, n * sizeof(slate_get_result), st);
  if (!s) s = ctx_d2h(ctx, val_off, g.voff.p, (n + 1) * 8, st);
  if (s) return s;
  const uint64_t total = val_off[n];
  if (total > vals_cap || (!vals && total)) return SLATE_E_CAPACITY;
  if (total) {
    SLATE_HIP(g.vals.ensure(total + 16));
    {
      GpuSpan cs(ctx, st);
      SLATE_HIP(launch_get_copy(st, q, g.voff.as<uint64_t>(), g.vals.as<uint8_t>()));
    }
    if ((s = ctx_d2h(ctx, vals, g.vals.p, total, st))) return s;
  }
  return SLATE_OK;
}

}  // extern "C"
