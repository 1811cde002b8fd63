"""bench.py host-side contract pieces that need no GPU: the metric string is BASELINE.json's verbatim, the committed
HBM-traffic measurement resolves for the dominant kernel families, every workload names its shape, and the CLI keeps
the driver's flags."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench():
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench
    finally:
        sys.argv = argv
    return bench


def test_metric_is_baseline_json_verbatim():
    b = _bench()
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        assert b.baseline_metric() == json.load(f)["metric"]


def test_traffic_file_covers_the_profiled_kernel_families():
    b = _bench()
    for cfg in ("h768", "cfg1"):
        for kind in b.KIND_TO_FAMILY:
            t = b.hbm_traffic(cfg, kind)
            assert t is None or t > 0
    assert b.hbm_traffic("cfg1", "gemm_tn") and b.hbm_traffic("cfg1", "gemm_tn") > 5e7      # committed PMC measurement present
    if os.path.exists(os.path.join(ROOT, "profiles", b.TRAFFIC_FILES["h768"])):
        assert b.hbm_traffic("h768", "gemm_dma_tn") > 5e7 and b.hbm_traffic("h768", "gemm_dma_nt") > 5e7


def test_default_workload_is_the_metric_configuration():
    """BASELINE.json's metric is quoted on hidden 768, 3-modal unaligned: that is what `value` must describe."""
    b = _bench()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert "default: h768" in out.stdout.replace("(default", "default").replace("'", "") or "h768" in out.stdout
    c = b.CONFIGS["h768"]
    assert c["hidden_sz"] == 768 and c["model"] == "mmtrvat" and (c["L"], c["V"], c["A"]) == (20, 500, 400)
    import inspect
    assert 'default="h768"' in inspect.getsource(b.main)


def test_workloads_and_cli():
    b = _bench()
    assert {"cfg1", "cfg3", "cfg4", "cfg5", "h768", "k768"} <= set(b.CONFIGS)      # every BASELINE.json config has a line
    for c in b.CONFIGS.values():
        assert c["desc"] and c["batch"] >= 1 and len(c["nv"]) == 3
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup"):
        assert flag in out.stdout


def test_full_and_dump_outputs_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--full", "--dump-outputs"):
        assert flag in out.stdout


def test_dump_outputs_is_deterministic_and_bounded(tmp_path):
    """dump_outputs on a small CPU model: float32 / float64 files, the same sample positions on every call, the sample
    and the norms are the gradients', a parameter without a gradient reads as zeros, and the default sample of a large
    gradient stays far below 64 MB."""
    import numpy as np
    import torch
    b = _bench()
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(64, 300), torch.nn.ReLU(), torch.nn.Linear(300, 6), torch.nn.Linear(6, 6))
    x = torch.randn(5, 64)
    logits = m[2](m[1](m[0](x)))                   # the last Linear gets no gradient
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, (torch.rand(5, 6) > 0.5).float())
    loss.backward()
    names = b.dump_outputs(str(tmp_path / "a"), m, logits, loss, n_sample=1000)
    b.dump_outputs(str(tmp_path / "b"), m, logits, loss, n_sample=1000)
    assert names == ["grad_norms", "grad_sample", "logits", "loss"]
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    for n in names:
        assert got[n].dtype in (np.float32, np.float64)
        assert np.array_equal(got[n], np.load(tmp_path / "b" / (n + ".npy")))
    assert got["logits"].shape == (5, 6) and got["loss"].shape == (1,)
    assert np.allclose(got["logits"], logits.detach().numpy()) and np.isclose(got["loss"][0], loss.item())
    params = list(m.parameters())
    grads = [p.grad.reshape(-1) if p.grad is not None else torch.zeros(p.numel()) for p in params]
    assert got["grad_norms"].dtype == np.float64 and got["grad_norms"].shape == (len(params),)
    assert np.allclose(got["grad_norms"], [float(g.double().norm()) for g in grads])
    assert got["grad_norms"][-1] == 0 and got["grad_norms"][-2] == 0
    flat = torch.cat(grads)
    idx = torch.randint(flat.numel(), (1000,), generator=torch.Generator().manual_seed(0)).sort().values
    assert np.array_equal(got["grad_sample"], flat[idx].numpy())
    big = torch.nn.Linear(4096, 4096, bias=False)
    big.weight.grad = torch.ones_like(big.weight)
    b.dump_outputs(str(tmp_path / "c"), big, torch.zeros(2, 6), torch.zeros(()))
    assert sum(f.stat().st_size for f in (tmp_path / "c").iterdir()) < 64 << 20
