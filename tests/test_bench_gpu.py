"""bench.py's plain run on the device: the record's headline keys, no side
leg without --full, and --dump-outputs holding the keys the timed path
returned, checked against the C restatement on the same tours."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"rows_layout", "rows_vs_words_identical", "quality", "quality_x1000",
             "quality_tdvrp200", "quality_tdvrp200_het", "islands", "cpu_baseline",
             "other_configs", "search", "cfg1_main_py", "quality_summary"}


@pytest.mark.gpu
def test_plain_run_record_and_dumped_keys(ctx, coracle, tmp_path):
    import torch

    from vrpms_amd import synth
    C = 5000                    # three 2048-tour workgroups, the last one partly filled
    out = tmp_path / "dump"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--steps", "2", "--warmup", "1", "--candidates", str(C),
                          "--dump-outputs", str(out)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.strip().splitlines() if ln.startswith("{")]
    rec = json.loads(lines[-1])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "evals/s" and rec["higher_is_better"] is True and rec["dtype"] == "int32"
    assert rec["ms_per_step"] > 0
    # one GPU: value = C x steps / wall and ms_per_step = wall / steps
    assert rec["value"] == pytest.approx(C / (rec["ms_per_step"] * 1e-3), rel=1e-4)
    assert rec["roofline"]["kernel"] == "eval_cvrp_words2" and rec["roofline"]["peak"] is None
    legs = {json.loads(ln)["bench_detail"] for ln in lines[:-1]}
    assert not legs & FULL_ONLY and not set(rec) & FULL_ONLY

    # the same tours (bench.make_batch: seed 0, stream 0xBE7C) through the C restatement
    inst = synth.cvrp(100, 8, seed=0)
    P = ctx.random_tours(C, inst.n, 0, stream_id=0xBE7C, dtype=torch.uint8).cpu().numpy()
    ref = coracle.eval_batch(inst.durations, P, inst.demand, inst.capacities, inst.start_times)[0]
    f = {n: np.load(out / f"keys_{n}.npy") for n in ("unvisited", "primary", "secondary")}
    assert all(a.dtype == np.float64 and a.shape == (C,) for a in f.values())
    got = (f["unvisited"].astype(np.uint64) << np.uint64(56)) \
        | (f["primary"].astype(np.uint64) << np.uint64(28)) | f["secondary"].astype(np.uint64)
    assert (got == ref).all()
