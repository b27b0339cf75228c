#!/usr/bin/env python3
"""End-to-end product throughput: CompressionBatch (CompressionBatch.java:41-148)
over a file list on local disk -> output files, one MI355X.  JPEG files are
read and header-parsed on host threads, decoded on the GPU straight into HBM,
compressed there (compressJpgWithTargetSize, -t 1 MiB), and written back.
Inputs: synthetic 4K q95 JPEGs (half smooth, half noise), and with --png N
as many 3840x2160 PNGs (BASELINE configs[4]'s mix: the PNG half is fitted
into the 1920 x 1920 box on the device, icx_png_fit_batch, and re-written on
host threads), written to a scratch directory first (not timed).  Runs the
batch twice with the same cache DB: run 1 learns (full search), run 2 is the
warm-cache run (C5's timing rule).  Before them an untimed warm-up run
(its own cache DB) takes the process's first-use costs - allocator slabs,
pinned pools, contexts' lazy setup, the inputs' page cache - out of the
timed runs, and a "search" run with a cache that never hits times the
cache-cold steady state (every file binary-searched: configs[2]'s first
pass).  Per run: wall time, and the device time
of each kernel family (HIP events) - the rest is host work (file reads,
header parses, PNG decode and deflate, file writes) not hidden behind it -
and the thread-seconds of every pipeline stage (pipeline.StageTimes).
--procs N runs N processes at once on the same GPU(s), each over its share of
the list (warm cache), to tell a per-process bound from the box's own.
Prints one JSON line."""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-compression_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--group", type=int, default=64)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--png", type=int, default=0, help="4K PNG files added to the list (configs[4] mix)")
    ap.add_argument("--devices", default="0,0",
                    help="GPU of each worker (one libicx context each); default: the CLI's, two workers on GPU 0")
    ap.add_argument("--group-max", type=int, default=0, help="files a worker takes at once when more wait (0: --group)")
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--reps", type=int, default=3, help="timed repetitions of each run (median reported)")
    ap.add_argument("--procs", type=int, default=1, help="processes sharing the list (warm-cache run only)")
    ap.add_argument("--decode-threads", type=int, default=0, help="host reader threads (0: every usable core)")
    ap.add_argument("--write-threads", type=int, default=4, help="JPEG output writer threads (the CLI default)")
    ap.add_argument("--png-filter", choices=("device", "host"), default="device",
                    help="where the PNG rows are filtered (the CLI's --png-filter)")
    a = ap.parse_args()
    from PIL import Image

    import icx
    from icx import pipeline
    from icx.core import CompressionParams
    from tests.oracle_ffi import noise, smooth
    work = a.dir or tempfile.mkdtemp(prefix="icx_pipe_")
    src = os.path.join(work, "src")
    os.makedirs(src, exist_ok=True)
    blobs = []
    for i in range(a.distinct):
        img = (smooth if i % 2 == 0 else noise)(2160, 3840, 70 + i)
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(b, "JPEG", quality=95, subsampling=2)
        blobs.append(b.getvalue())
    paths = []
    for i in range(a.files):
        p = os.path.join(src, f"f{i:05d}.jpg")
        with open(p, "wb") as f:
            f.write(blobs[i % a.distinct])
        paths.append(p)
    png_blobs = []
    if a.png:
        from icx.pngio import encode_png
        for i in range(min(a.distinct, a.png)):
            img = (smooth if i % 2 == 0 else noise)(2160, 3840, 170 + i)
            png_blobs.append(encode_png(img, level=1))
        for i in range(a.png):
            p = os.path.join(src, f"p{i:05d}.png")
            with open(p, "wb") as f:
                f.write(png_blobs[i % len(png_blobs)])
            paths.insert(2 * i + 1 if 2 * i + 1 <= len(paths) else len(paths), p)  # interleaved
    lst = os.path.join(work, "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(paths))
    # the inputs' dirty pages written back now, not under the timed runs
    # (their writeback beside a run moved the warm-cache rate by +-15 %)
    os.sync()
    params = CompressionParams(0.25, 1 << 20, 1920, 1920, 1 << 20)  # Execute.java defaults
    if a.procs > 1:
        multi_process(a, work, lst, params, blobs, png_blobs)
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
        return
    codecs = [icx.Codec(int(d)) for d in a.devices.split(",")]
    kernels = ("dec_unstuff", "dec_init", "dec_sync", "dec_sync_r1", "dec_sync_r2", "dec_sync_r3", "dec_write",
               "dec_dc", "dec_idct", "dec_color", "fdct", "huff", "scan", "ffscan", "stuff", "resize", "pngfilter")
    from icx.cache import LockedDict

    class NoHits(LockedDict):  # a learned cache that never hits: every file searches
        def get(self, k, default=None):
            return default

    def batch(out, cache_db):
        return pipeline.CompressionBatch(lst, out, params, 1, cache_db, codecs=codecs, group_size=a.group,
                                         decode_threads=a.decode_threads or None, stage_times=True,
                                         group_max=a.group_max, write_threads=a.write_threads,
                                         png_filter=a.png_filter)
    if not a.no_warmup:  # untimed: the process's first-use costs (its own cache DB)
        batch(os.path.join(work, "out_w"), os.path.join(work, "cache_w")).execute()
        shutil.rmtree(os.path.join(work, "out_w"), ignore_errors=True)
        os.sync()
    runs = []
    order = [("search", k) for k in range(a.reps)]
    for k in range(a.reps):  # each learn run starts from an empty cache DB; the warm runs reuse the last one's
        order.append(("learn", k))
    order += [("warm cache", k) for k in range(a.reps)]
    for r, (name, rep_k) in enumerate(order):
        if name == "learn":
            for f in os.listdir(work):
                if f.startswith("cache"):
                    os.remove(os.path.join(work, f))
        out = os.path.join(work, f"out{r}")
        for c in codecs:
            c.profile(True)
            c.profile_reset()
        t0 = time.perf_counter()
        b = batch(out, os.path.join(work, "cache"))
        rep = b.execute(cache=NoHits(), save_cache=False) if name == "search" else b.execute()
        dt = time.perf_counter() - t0
        os.sync()  # this run's output files written back before the next run starts (untimed)
        dev, host = {}, {}
        for c in codecs:
            c.profile(False)
            for k in kernels:
                ms = c.profile_query(k)["ms"]
                if ms:
                    dev[k] = round(dev.get(k, 0.0) + ms, 2)
            for k in ("host.call_decode", "host.call_fit", "host.dec_headers", "host.dec_setup", "host.sync",
                      "host.results"):
                q = c.profile_query(k)
                if q["launches"]:
                    host[k] = {"ms": round(host.get(k, {}).get("ms", 0.0) + q["ms"], 2),
                               "calls": host.get(k, {}).get("calls", 0) + q["launches"]}
        shutil.rmtree(out, ignore_errors=True)
        runs.append({"run": name, "rep": rep_k, "seconds": round(dt, 3),
                     "images_per_s": round(rep.total / dt, 1), "mp_per_s": round(rep.megapixels / dt, 1),
                     "success": rep.success, "failed": rep.failed, "skipped": rep.skipped,
                     "in_bytes": rep.original_size, "out_bytes": rep.compressed_size,
                     "device_ms": dev, "device_ms_total": round(sum(dev.values()), 1),
                     # kernel time / wall (an upper bound on the busy fraction where
                     # launches of two streams or contexts overlap)
                     "device_busy_frac": round(sum(dev.values()) / (dt * 1e3), 3), "library_host_spans": host,
                     "host_threads": a.decode_threads or pipeline.host_cores()[0], "stages": rep.stages,
                     "file_read_GBps": round(rep.original_size / dt / 1e9, 2)})
    for c in codecs:
        c.close()
    summary = {}
    for name in ("search", "learn", "warm cache"):
        rs = sorted((r for r in runs if r["run"] == name), key=lambda r: r["images_per_s"])
        med = rs[len(rs) // 2]
        summary[name] = {"images_per_s_median": med["images_per_s"], "mp_per_s_median": med["mp_per_s"],
                         "device_busy_frac_median": med["device_busy_frac"],
                         "images_per_s_all": [r["images_per_s"] for r in rs]}
    print(json.dumps({"metric": "CompressionBatch end-to-end (files -> files), 4K q95 JPEG" +
                                (" + 4K PNG (configs[4] mix)" if a.png else "") + ", -t 1MiB, devices " + a.devices,
                      "files": a.files, "png_files": a.png, "group_size": a.group, "group_max": a.group_max,
                      "write_threads": a.write_threads, "png_filter": a.png_filter,
                      "mean_src_bytes": int(np.mean([len(b) for b in blobs])),
                      "mean_png_src_bytes": int(np.mean([len(b) for b in png_blobs])) if png_blobs else 0,
                      "summary": summary, "runs": runs}))
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)


def _proc(k, n, lst, work, params, group, devices, threads, barrier, q):
    """One process of --procs: its share of the list, learning run untimed,
    the warm-cache run started with the others (barrier)."""
    import icx
    from icx import pipeline
    lines = open(lst).read().split("\n")
    mine = os.path.join(work, f"list{k}.txt")
    with open(mine, "w") as f:
        f.write("\n".join(lines[k::n]))
    codecs = [icx.Codec(int(d)) for d in devices.split(",")]
    cache = os.path.join(work, f"cache{k}")
    pipeline.CompressionBatch(mine, os.path.join(work, f"o{k}a"), params, 1, cache, codecs=codecs,
                              group_size=group, decode_threads=threads).execute()
    barrier.wait()
    t0 = time.perf_counter()
    rep = pipeline.CompressionBatch(mine, os.path.join(work, f"o{k}b"), params, 1, cache, codecs=codecs,
                                    group_size=group, decode_threads=threads, stage_times=True).execute()
    dt = time.perf_counter() - t0
    for c in codecs:
        c.close()
    q.put({"proc": k, "files": rep.total, "success": rep.success, "seconds": round(dt, 3),
           "in_bytes": rep.original_size, "stages": rep.stages})


def multi_process(a, work, lst, params, blobs, png_blobs):
    import multiprocessing as mp
    from icx import pipeline
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    barrier = ctx.Barrier(a.procs)
    threads = a.decode_threads or max(1, pipeline.host_cores()[0] // a.procs)
    ps = [ctx.Process(target=_proc, args=(k, a.procs, lst, work, params, a.group, a.devices, threads, barrier, q))
          for k in range(a.procs)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=900) for _ in ps), key=lambda r: r["proc"])
    for p in ps:
        p.join(60)
    wall = max(r["seconds"] for r in res)
    files = sum(r["files"] for r in res)
    print(json.dumps({"metric": f"CompressionBatch end-to-end, {a.procs} processes on devices {a.devices} "
                                "(warm cache), 4K q95 JPEG" + (" + 4K PNG" if a.png else ""),
                      "files": files, "procs": a.procs, "threads_per_proc": threads, "group_size": a.group,
                      "seconds": wall, "images_per_s": round(files / wall, 1),
                      "file_read_GBps": round(sum(r["in_bytes"] for r in res) / wall / 1e9, 2),
                      "mean_src_bytes": int(np.mean([len(b) for b in blobs])), "per_proc": res}))


if __name__ == "__main__":
    main()
