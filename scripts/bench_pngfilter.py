#!/usr/bin/env python3
"""The PNG row filter kernel on its own: a group of 4K RGB frames fitted into
the 1920 x 1920 box and filtered in one fused call (icx_png_fit_filter_batch),
the "pngfilter" and "resize" launches timed by the library's HIP events
(icx_profile_query).  The kernel reads each resized frame once (the row above
comes from L2) and writes the filtered stream, so its HBM traffic is taken as
2 x stream bytes.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-compression_amd"))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12  # measured copy rate of one MI355X (float4 copy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import icx
    from icx.core import CompressionParams
    from tests.oracle_ffi import noise, smooth
    frames = [(smooth if i % 2 == 0 else noise)(2160, 3840, 170 + i) for i in range(4)]
    imgs = [frames[i % 4] for i in range(a.images)]
    params = CompressionParams(0.25, 1 << 20, 1920, 1920, 1 << 20)
    codec = icx.Codec(0)
    codec.png_fit_filter_batch(imgs, params)  # warm-up: workspace, first launch
    runs = []
    for _ in range(a.reps):
        codec.profile(True)
        codec.profile_reset()
        res = codec.png_fit_filter_batch(imgs, params)
        q, r = codec.profile_query("pngfilter"), codec.profile_query("resize")
        codec.profile(False)
        runs.append({"pngfilter_ms": round(q["ms"], 4), "launches": q["launches"], "stream_bytes": q["units"],
                     "resize_ms": round(r["ms"], 4),
                     "GBps_on_2x_stream": round(2 * q["units"] / (q["ms"] * 1e-3) / 1e9, 1)})
    codec.close()
    med = sorted(runs, key=lambda x: x["pngfilter_ms"])[len(runs) // 2]
    print(json.dumps({"metric": f"pngfilter kernel, {a.images} x 3840x2160 RGB -> {res[0].width}x{res[0].height}, "
                                "one fused fit + filter call",
                      "median": med, "hbm_frac_on_2x_stream": round(med["GBps_on_2x_stream"] * 1e9 / HBM_BYTES_PER_S, 3),
                      "runs": runs}))


if __name__ == "__main__":
    main()
