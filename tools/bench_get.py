"""Batched point-read measurement (tooling): slate_sst_get_batch over one SST opened into HBM
(slate_sst_open), against what a caller could compose before it existed and against the oracle.
Workload: an SST of --kvs KVs (16 B keys b"k%015d" over the even ids, 84 B values, 4 KiB blocks)
in CodecNone and in Snappy; --queries uniformly drawn ids, half of them present (even) and half
absent (odd), so absent keys fall between present ones all over the key range.
Per codec, three JSON lines from the same run on the same box:
  get_batch    queries/s over the wall time of the call (key upload, lookups, result download),
               device-busy ms (slate_ctx_set_timing spans), the counters, and the useful bytes
               (unique blocks touched x their size + value bytes) over the wall time as a fraction
               of the HBM peak bench.py uses;
  composed     slate_bloom_has_keys + slate_index_seek + slate_read_blocks over the touched block
               range + slate_block_seek, all from host buffers as those entry points take them
               (it stops at the seek: the row fetch and key compare are left to the caller);
  oracle       tests/getref.py on one thread over a sample (Python composing the C oracle).
--check compares 10 000 sampled queries of the get_batch run with tests/getref.py.
--runs measures sorted runs instead: the same KVs as one run of S SSTs (S = 1, 64, 512, or --run-ssts),
per codec and S one JSON line with, each as the median of the steps after warm-up with min and max:
  (a) runs      slate_sst_get_batch_runs over the run (and again with pos = NULL, which saves the
                download of 8 bytes per query);
  (b) per_sst   what a caller could do without it: a host bisect over the SSTs' first keys, the keys
                grouped per SST, one slate_sst_get_batch per SST (no walk-on; the grouping is timed,
                scattering the results back is not);
  (c) one_sst   slate_sst_get_batch over the same KVs as one SST, the floor;
and with --check 10 000 sampled queries of (a) against tests/srref.py.
usage: python tools/bench_get.py [--kvs 1000000] [--queries 1000000] [--steps 5] [--check] [--out FILE]
       python tools/bench_get.py --runs [--run-ssts 1,64,512] [--check] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "slatedb-go_amd")]

HBM_PEAK_GBPS = 8000.0  # as bench.py


def key_array(ids: np.ndarray) -> np.ndarray:
    """b"k%015d" % id for every id, as an (n, 16) byte array."""
    out = np.empty((len(ids), 16), np.uint8)
    out[:, 0] = ord("k")
    x = ids.astype(np.uint64).copy()
    for d in range(15, 0, -1):
        out[:, d] = (x % 10).astype(np.uint8) + ord("0")
        x //= 10
    return out


_WORKLOAD = {}


def build_sst(ob, n: int, codec: int, seed: int = 7, lo: int = 0, hi: int | None = None) -> bytes:
    """The workload's KVs [lo, hi) (default: all n) as one SST."""
    hi = n if hi is None else hi
    if (n, seed) not in _WORKLOAD:  # (one workload per process: the --runs leg cuts it many times)
        _WORKLOAD.clear()
        _WORKLOAD[(n, seed)] = (key_array(np.arange(n, dtype=np.uint64) * 2),
                                np.random.default_rng(seed).integers(0, 256, (n, 84), dtype=np.uint8))
    keys, vals = (x[lo:hi] for x in _WORKLOAD[(n, seed)])
    m = hi - lo
    b = ob.SstBuilder(4096, 0, 10, codec)
    ko = np.arange(m + 1, dtype=np.uint64) * 16
    vo = np.arange(m + 1, dtype=np.uint64) * 84
    assert b.add_batch(np.ascontiguousarray(keys).reshape(-1), ko, np.ascontiguousarray(vals).reshape(-1), vo) == 0
    assert b.build() == 0
    return b.encode_table()


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def stats(ts):
    return {"ms": round(median(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


def runs_leg(args, ctx, sc, ob, qk, qo, ids):
    """The --runs measurement (see the module's docstring) -> (lines, ok)."""
    from tests import getref, srref
    L = sc.lib()
    n, nq = args.kvs, args.queries
    lines, ok = [], True
    res = np.zeros(nq, sc.GET_DTYPE)
    pos = np.zeros(nq, sc.GET_POS_DTYPE)
    val_off = np.zeros(nq + 1, np.uint64)
    vals = np.zeros(84 * nq + 16, np.uint8)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    for codec, cname in ((sc.NONE, "none"), (sc.SNAPPY, "snappy")):
        one = ctx.open_sst(build_sst(ob, n, codec))
        h1 = (C.c_void_p * 1)(one.handle)

        def floor():
            st = L.slate_sst_get_batch(ctx.handle, h1, 1, sc._ptr(qk), sc._ptr(qo), nq, sc._ptr(res), sc._ptr(vals),
                                       vals.size, sc._ptr(val_off))
            assert st == sc.OK, st

        for S in args.run_ssts:
            step = -(-n // S)
            cuts = [(p * step, min(n, (p + 1) * step)) for p in range(S) if p * step < n]
            ssts = [build_sst(ob, n, codec, lo=lo, hi=hi) for lo, hi in cuts]
            hs = [ctx.open_sst(s) for s in ssts]
            run = ctx.open_run(hs)
            rp = (C.c_void_p * 1)(run.handle)
            first_ids = np.array([2 * lo for lo, _ in cuts], dtype=np.uint64)

            def runs(with_pos=True):
                st = L.slate_sst_get_batch_runs(ctx.handle, None, 0, rp, 1, sc._ptr(qk), sc._ptr(qo), nq, sc._ptr(res),
                                                sc._ptr(pos) if with_pos else None, sc._ptr(vals), vals.size,
                                                sc._ptr(val_off))
                assert st == sc.OK, st

            def per_sst():
                # the keys are b"k%015d" % id: a bisect over the first keys is one over their ids
                which = np.searchsorted(first_ids, ids, side="right").astype(np.int64) - 1
                order = np.argsort(which, kind="stable")
                sk = np.ascontiguousarray(qk.reshape(-1, 16)[order])
                bounds = np.searchsorted(which[order], np.arange(len(cuts) + 1))
                vo = 0
                for p in range(len(cuts)):
                    a, b = int(bounds[p]), int(bounds[p + 1])
                    if a == b:
                        continue
                    hp = (C.c_void_p * 1)(hs[p].handle)
                    st = L.slate_sst_get_batch(ctx.handle, hp, 1, sc._ptr(sk[a:b]), sc._ptr(qo), b - a,
                                               sc._ptr(res[a:b]), sc._ptr(vals[vo:]), vals.size - vo, sc._ptr(val_off[a:]))
                    assert st == sc.OK, st
                    vo += int(val_off[a + b - a])

            ctx.get_counters(reset=True)
            ta = timed(runs)
            cnt = {k: v // (args.steps + args.warmup) for k, v in ctx.get_counters(reset=True).items()}
            found = int((res["outcome"] == sc.GET_VALUE).sum())
            line = {"metric": f"batched point reads over one sorted run of {len(cuts)} SSTs, codec {cname}",
                    "config": {"kvs": n, "queries": nq, "ssts": len(cuts), "blocks": run.info()["n_blocks"],
                               "run_device_bytes": run.info()["device_bytes"], "steps": args.steps},
                    "runs": stats(ta), "counters": cnt, "found": found}
            if args.check:
                refs = [getref.RefSst(s) for s in ssts]
                pick = np.random.default_rng(2).choice(nq, min(10_000, nq), replace=False)
                bad = 0
                for i in pick:
                    r = srref.get_one([], [refs], qk[16 * i:16 * i + 16].tobytes())
                    got = vals[int(val_off[i]):int(val_off[i + 1])].tobytes()
                    bad += (any(int(res[f][i]) != r[f] for f in getref.FIELDS) or got != r["value"]
                            or int(pos["run_sst"][i]) != r["run_sst"] or int(pos["err_run_sst"][i]) != r["err_run_sst"])
                line["check"] = {"sampled": int(len(pick)), "mismatches": int(bad)}
                ok = ok and bad == 0
            tb = timed(per_sst)
            tc = timed(floor)
            line.update(runs_pos_null=stats(timed(lambda: runs(False))), per_sst=stats(tb), one_sst=stats(tc),
                        runs_over_per_sst=round(median(ta) / median(tb), 3),
                        runs_over_one_sst=round(median(ta) / median(tc), 3),
                        ranges_overlap_runs_per_sst=bool(min(ta) <= max(tb) and min(tb) <= max(ta)),
                        value=round(nq / median(ta)), unit="queries/s")
            lines.append(line)
            print(json.dumps(line), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    for ln in lines:
                        f.write(json.dumps(ln) + "\n")
            run.close()
            for h in hs:
                h.close()
        one.close()
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", action="store_true", help="measure sorted runs (slate_sst_get_batch_runs)")
    ap.add_argument("--run-ssts", type=lambda s: [int(x) for x in s.split(",")], default=[1, 64, 512])
    ap.add_argument("--kvs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-sample", type=int, default=20_000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import slatecodec as sc
    from oracle import binding as ob
    from tests import getref

    torch.cuda.set_device(0)  # torch's HIP runtime first, then the library's context (as bench.py)
    ctx = sc.Context(0)
    L = sc.lib()
    n, nq = args.kvs, args.queries
    rng = np.random.default_rng(1)
    ids = rng.integers(0, n, nq, dtype=np.uint64) * 2 + (rng.random(nq) < 0.5)
    qk = np.ascontiguousarray(key_array(ids).reshape(-1))
    qo = np.arange(nq + 1, dtype=np.uint64) * 16
    lines = []
    ok = True
    if args.runs:
        lines, ok = runs_leg(args, ctx, sc, ob, qk, qo, ids)
        sys.exit(0 if ok else 1)
    for codec, cname in ((sc.NONE, "none"), (sc.SNAPPY, "snappy")):
        sst = build_sst(ob, n, codec)
        a = np.frombuffer(sst, dtype=np.uint8)
        t0 = time.perf_counter()
        h = ctx.open_sst(sst)
        open_s = time.perf_counter() - t0
        inf = h.info()
        hs = (C.c_void_p * 1)(h.handle)
        res = np.zeros(nq, sc.GET_DTYPE)
        val_off = np.zeros(nq + 1, np.uint64)
        vals = np.zeros(84 * nq + 16, np.uint8)

        def get():
            st = L.slate_sst_get_batch(ctx.handle, hs, 1, sc._ptr(qk), sc._ptr(qo), nq, sc._ptr(res), sc._ptr(vals),
                                       vals.size, sc._ptr(val_off))
            assert st == sc.OK, st

        for _ in range(args.warmup):
            get()
        ctx.set_timing(True)
        ctx.get_counters(reset=True)
        wall, busy = [], []
        for _ in range(args.steps):
            ctx.gpu_busy_ms(reset=True)
            t0 = time.perf_counter()
            get()
            wall.append(time.perf_counter() - t0)
            busy.append(ctx.gpu_busy_ms(reset=True)[0])
        ctx.set_timing(False)
        cnt = {k: v // args.steps for k, v in ctx.get_counters(reset=True).items()}
        w = median(wall)
        at_row = res["stage"] >= sc.GET_AT_END
        touched = int(np.unique(res["block"][res["stage"] == sc.GET_AT_ROW]).size)
        block_bytes = (inf["filter_offset"] / max(inf["n_blocks"], 1))
        useful = touched * block_bytes + int(val_off[nq])
        lines.append({
            "metric": f"batched point reads (slate_sst_get_batch), codec {cname}", "value": round(nq / w),
            "unit": "queries/s", "wall_ms": round(w * 1e3, 3), "wall_ms_min": round(min(wall) * 1e3, 3),
            "device_busy_ms": round(median(busy), 3), "counters": cnt,
            "config": {"kvs": n, "queries": nq, "blocks": inf["n_blocks"], "block_size": 4096,
                       "handle_device_bytes": inf["device_bytes"], "open_ms": round(open_s * 1e3, 1)},
            "found": int((res["outcome"] == sc.GET_VALUE).sum()), "reached_a_block": int(at_row.sum()),
            "unique_blocks_touched": touched, "useful_bytes": int(useful),
            "useful_GBps": round(useful / w / 1e9, 2), "hbm_peak_GBps": HBM_PEAK_GBPS,
            "hbm_frac": round(useful / w / 1e9 / HBM_PEAK_GBPS, 5),
        })
        if args.check:
            ref = getref.RefSst(sst)
            pick = np.random.default_rng(2).choice(nq, min(10_000, nq), replace=False)
            bad = 0
            for i in pick:
                k = qk[16 * i:16 * i + 16].tobytes()
                r = getref.get_one([ref], k)
                got = vals[int(val_off[i]):int(val_off[i + 1])].tobytes()
                bad += any(int(res[f][i]) != r[f] for f in getref.FIELDS) or got != r["value"]
            lines[-1]["check"] = {"sampled": int(len(pick)), "mismatches": int(bad)}
            ok = ok and bad == 0

        # what a caller could compose before: four synchronous entry points from host buffers
        st, info, _ = sc.read_info(sst)
        st, index = ctx.decode_index(sst[info.index_offset:info.index_offset + info.index_len], codec)
        st, num_probes, bits = ctx.bloom_decode(sst[info.filter_offset:info.filter_offset + info.filter_len], codec)
        fb = np.frombuffer(bits, dtype=np.uint8)
        nb = inf["n_blocks"]
        data = a[: info.filter_offset]
        # decoded blocks start on 16-byte boundaries; one more row slot per block than the bytes need
        out = np.zeros(int(info.filter_offset) * (1 if codec == sc.NONE else 3) + 16 * nb + 65536, np.uint8)
        out_off = np.zeros(nb + 1, np.uint64)
        row_base = np.zeros(nb + 1, np.uint64)
        meta = np.zeros(nb, sc.META_DTYPE)
        rows = np.zeros(out.size // 15 + nb + 8, sc.ROW_DTYPE)

        def composed():
            may = np.zeros(nq, np.uint8)
            assert L.slate_bloom_has_keys(ctx.handle, num_probes, sc._ptr(fb), fb.size, sc._ptr(qk), sc._ptr(qo), nq,
                                          sc._ptr(may)) == sc.OK
            sel = np.nonzero(may)[0]
            sk = np.ascontiguousarray(qk.reshape(-1, 16)[sel].reshape(-1))
            so = np.arange(len(sel) + 1, dtype=np.uint64) * 16
            blk = np.zeros(len(sel), np.uint64)
            assert L.slate_index_seek(ctx.handle, index.handle, sc._ptr(sk), sc._ptr(so), len(sel), sc._ptr(blk)) == sc.OK
            b0, b1 = int(blk.min()), int(blk.max()) + 1
            rs, re_ = C.c_uint64(), C.c_uint64()
            assert L.slate_read_blocks_range(C.byref(info), index.handle, b0, b1, C.byref(rs), C.byref(re_)) == sc.OK
            failed = C.c_uint64()
            piece = data[rs.value:re_.value]
            st = L.slate_read_blocks(ctx.handle, C.byref(info), index.handle, b0, b1, sc._ptr(piece), piece.size,
                                     sc._ptr(out), out.size, sc._ptr(out_off), sc._ptr(meta), sc._ptr(rows), rows.size,
                                     sc._ptr(row_base), C.byref(failed))
            assert st == sc.OK, (st, int(out_off[b1 - b0]), out.size, int(row_base[b1 - b0]), rows.size)
            qb = (blk - b0).astype(np.uint32)
            seek = np.zeros(len(sel), sc.SEEK_DTYPE)
            assert L.slate_block_seek(ctx.handle, sc._ptr(out), sc._ptr(out_off), sc._ptr(meta), b1 - b0, sc._ptr(qb),
                                      sc._ptr(sk), sc._ptr(so), len(sel), sc._ptr(seek)) == sc.OK
            return len(sel)

        composed()
        cw = []
        for _ in range(max(args.steps // 2, 2)):
            t0 = time.perf_counter()
            nsel = composed()
            cw.append(time.perf_counter() - t0)
        lines.append({
            "metric": f"composed from the earlier entry points (bloom_has_keys + index_seek + read_blocks + "
                      f"block_seek; stops at the seek), codec {cname}",
            "value": round(nq / median(cw)), "unit": "queries/s", "wall_ms": round(median(cw) * 1e3, 3),
            "config": {"kvs": n, "queries": nq, "queries_past_the_filter": int(nsel), "blocks_decoded": nb},
        })
        ns = min(args.oracle_sample, nq)
        ref = getref.RefSst(sst)
        ref_keys = [qk[16 * i:16 * i + 16].tobytes() for i in range(ns)]
        for b in range(len(ref.metas)):  # decode every block outside the timed part, as the handle holds them
            ref.block(b)
        t0 = time.perf_counter()
        for k in ref_keys:
            getref.get_one([ref], k)
        os_ = time.perf_counter() - t0
        lines.append({
            "metric": f"oracle, one thread (tests/getref.py: Python composing the C oracle, blocks decoded "
                      f"beforehand), codec {cname}",
            "value": round(ns / os_), "unit": "queries/s", "config": {"sample": ns},
        })
        h.close()
        for ln in lines[-3:]:
            print(json.dumps(ln), flush=True)
        if args.out:  # rewritten after every codec, so a later failure keeps the earlier lines
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
