"""bench.py's reporting helpers on the CPU: the roofline's `traffic` comes
from the committed PMC summary (profiles/pmc_summary.json), and the CPU
baseline runs on every host core the process may use."""
import json
import os

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_pmc_summary_gives_traffic_for_the_encode_kernels():
    summary = json.load(open(os.path.join(ROOT, "profiles", "pmc_summary.json")))
    assert "bytes_per_unit" in summary, "commit the file scripts/pmc_summary.py writes, not its stdout"
    for kernel, units in (("huff", 56_700_000), ("fdct", 333 * 3840 * 2160)):
        t = bench.pmc_traffic(kernel, units)
        assert t is not None and t > 0, kernel
    # k_huff: measured HBM bytes within 1.0x-1.5x of its ~74 algorithmic B per block-trial
    assert 74 <= summary["bytes_per_unit"]["huff"] <= 111
    # k_fdct_color: 3 B/px pixel reads + candidate lists
    assert 3.0 <= summary["bytes_per_unit"]["fdct"] <= 6.0


def test_pmc_bytes_per_unit_reads_both_summary_forms():
    file_form = {"bytes_per_unit": {"huff": 82.5}}
    kernel_form = {"icx::k_huff": {"hbm_bytes_per_unit": 82.5}, "icx::k_fdct_color<true>": {"hbm_bytes_per_unit": 4.27},
                   "icx::k_other": {"hbm_bytes_per_unit": 1.0}}
    assert bench.pmc_bytes_per_unit(file_form) == {"huff": 82.5}
    assert bench.pmc_bytes_per_unit(kernel_form) == {"huff": 82.5, "fdct": 4.27}


def test_dump_outputs_writes_results_checksums_and_a_byte_sample(tmp_path):
    """--dump-outputs: float32 / float64 .npy files only; the per-image
    columns cover every image, the checksums cover outs[i][:out_len] alone,
    and the sample holds whole JPEGs of the listed images in index order."""
    import numpy as np
    import torch

    import icx
    n, cap = 20, 5000
    outs = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (n, cap), dtype=np.uint8))
    res = [{"status": 0, "success": True, "cache_hit": i % 2 == 0, "out_len": 1000 + 100 * i, "encodes": 1 + i % 3,
            "learned": icx.LearnedParams(0.25, 1.0)} for i in range(n)]
    bench.dump_outputs(str(tmp_path / "d"), res, outs)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert all(p.suffix == ".npy" for p in (tmp_path / "d").iterdir())
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert got["out_len"].tolist() == [1000 + 100 * i for i in range(n)]
    assert got["encodes"].tolist() == [1 + i % 3 for i in range(n)]
    assert got["learned_quality"].tolist() == [0.25] * n and got["learned_scale"].tolist() == [1.0] * n
    o = outs.numpy().astype(np.int64)
    for i in range(n):
        b = o[i, :1000 + 100 * i]
        assert got["jpeg_byte_sum"][i] == b.sum()
        assert got["jpeg_weighted_sum"][i] == (b * (np.arange(len(b)) % 251 + 1)).sum()
    idx = got["jpeg_sample_index"].astype(int)
    assert len(idx) == bench.DUMP_SAMPLE_IMAGES and list(idx) == sorted(set(idx))
    want = np.concatenate([o[i, :1000 + 100 * i] for i in idx])
    assert np.array_equal(got["jpeg_sample_bytes"], want.astype(np.float32))
    # the same sample on every run
    bench.dump_outputs(str(tmp_path / "e"), res, outs)
    assert np.array_equal(np.load(tmp_path / "e" / "jpeg_sample_index.npy"), got["jpeg_sample_index"])


def test_host_cores_is_the_usable_core_count():
    n, how = bench.host_cores()
    assert 1 <= n <= len(os.sched_getaffinity(0))
    assert how in ("sched_getaffinity", "cgroup cpu.max quota")
