"""The multi-GPU bench path (`bench.py --gpus N`, what the driver's scaling run launches) rehearsed on the test box's
one GPU: STGCN_BENCH_REHEARSE=1 puts both ranks on GPU 0 over gloo.  `bench.py --gpus 2` must spawn its ranks, run
DDP, meet at the barriers and have rank 0 print exactly one JSON line with the whole-job fields (the numbers of two
ranks timesharing one GPU are not a measurement)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra", [[], ["--config", "4"], ["--sync-bn"]])
def test_bench_two_ranks_rehearsal(extra):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    env = dict(os.environ, STGCN_BENCH_REHEARSE="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--no-cpu-baseline", "--no-layer-roofline", "--kernel-steps", "0"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["parallelism"].startswith("dp2") and "REHEARSAL" in d["config"]["parallelism"]
    assert d["config"]["bn_stats"] == ("sync (all ranks)" if "--sync-bn" in extra else "per-replica")


def test_bench_plain_run_dumps_outputs(tmp_path, pkg):
    """A plain `bench.py --gpus 1` run times exactly --steps steps, leaves the secondary measurements (--full) out
    and, with --dump-outputs, writes the last timed step's logits, loss terms, gradients and updated parameters as
    float32 .npy files of at most 64 MB in all."""
    import numpy as np

    import bench
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["full"] is False
    assert abs(d["value"] - 64 * 300 / (d["ms_per_step"] / 1e3)) / d["value"] < 0.01
    for k in ("roofline", "roofline_tcn_fwd", "kernels", "layer_roofline", "layer_roofline_ln", "cpu_baseline"):
        assert d[k] is None, k
    files = {f[:-4]: np.load(out / f, allow_pickle=False) for f in os.listdir(out)}
    assert files["logits"].shape[:2] == (64, 52) and files["loss_ce"].size == 1 and files["loss_mse"].size == 1
    params = {k[6:] for k in files if k.startswith("param.")}
    grads = {k[5:] for k in files if k.startswith("grad.")}
    model = pkg.MODELS["st-gcn"](rank=None, **dict(bench.ARCH, graph=pkg.PKU_MMD))  # the bench's model, on the host
    want = {k: tuple(p.shape) for k, p in model.named_parameters() if p.requires_grad}
    assert params == set(want) and grads and grads <= params
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert all(files["grad." + k].shape == files["param." + k].shape == want[k] for k in grads)
    assert any(np.abs(files["grad." + k]).max() > 0 for k in grads)
    # the dumped loss terms belong to the dumped logits: torch's loss (bench.loss_fn, fp32 on the host) of those
    # logits with the bench's own labels and class weights.  Tolerance: both sides sum 64 x 52 fp32 terms of O(1)
    # (log-softmax, weighted mean), rounding ~1e-6 relative; 1e-4 leaves two orders for the summation orders
    dev = torch.device("cuda", 0)
    cd = bench.class_dist(dev).cpu()
    _, labels = bench.config2_batch(dev, 0)
    ref = bench.loss_fn(torch.from_numpy(files["logits"]), labels.cpu(), 1 - cd / cd.sum()).item()
    got = files["loss_ce"].item() + files["loss_mse"].item()
    assert abs(got - ref) <= 1e-4 * abs(ref), (got, ref)
    # the parameters are the updated ones: Adam has moved every parameter whose gradient is not zero away from the
    # bench's seeded initial value
    torch.manual_seed(1538574472)
    init = pkg.MODELS["st-gcn"](rank=None, **dict(bench.ARCH, graph=pkg.PKU_MMD)).state_dict()
    stuck = [k for k in grads if np.any(files["grad." + k]) and np.array_equal(files["param." + k], init[k].numpy())]
    assert not stuck, stuck[:5]
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
