"""co-st-gcn stream batches on the device (co_streams.hip, Model.stream_batch): every stream of a batch is the
restatement's stream (tests/costgcn_ref.py) over the frames it stepped, from its last restart; a stream's output does
not depend on B, its slot or its neighbours; skips leave state alone; one captured tick replays with changing masks."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from costgcn_ref import costgcn_stream, randomise  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-3

SMALL = dict(in_ch=[8, 8, 16], out_ch=[8, 16, 16], stride=[1, 2, 2])   # identity residual, residual conv, stride 2 twice
WIDE = dict(in_ch=[64], out_ch=[128], stride=[2])                      # 4 column tiles, 72 k-steps


@pytest.fixture(scope="module")
def P(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return pkg


def make_arch(graph, kernel, in_ch, out_ch, stride):
    nl = len(in_ch)
    return {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": 7, "graph": graph,
            "st-gcn": {"importance": True, "in_feat": 3, "stages": 1, "layers": nl, "kernel": kernel,
                       "in_ch": list(in_ch), "out_ch": list(out_ch), "stride": list(stride), "dilation": [1] * nl,
                       "residual": [1] * nl, "dropout": [0.0] * nl}}


def build(P, arch, seed):
    torch.manual_seed(seed)
    m = P.MODELS["co-st-gcn"](rank=None, **arch)
    sd = randomise(m.state_dict(), torch.Generator().manual_seed(seed + 1))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval(), sd


def run(batch, x, codes):
    """x (B, 3, T, V) on the device, codes (T, B) int (None: every stream steps every tick) -> (B, K, T)."""
    T = x.shape[2]
    outs = []
    for t in range(T):
        a = None if codes is None else codes[t].to(device=DEV, dtype=torch.int32)
        outs.append(batch.step(x[:, :, t:t + 1].contiguous(), a))
    torch.cuda.synchronize()
    return torch.cat(outs, dim=2)


def dirty(batch):
    """State a restart must not read: garbage rings, residuals and indices."""
    for ring, res_ring, idx in batch.state:
        ring.fill_(7.0)
        res_ring.fill_(-3.0)
        idx.fill_(1)


def case(P, kernel, widths, frames, B, seed, V=25, graph=None):
    """A model, B streams of ``frames`` random frames and the restatement of each in fp32, fp64 and bf16-rounded."""
    arch = make_arch(graph or P.PKU_MMD, kernel, **widths)
    m, sd = build(P, arch, seed)
    x = torch.randn(B, 3, frames, V, generator=torch.Generator().manual_seed(seed + 2))
    with torch.no_grad():
        ref32 = torch.cat([costgcn_stream(x[b:b + 1], sd, arch, sd["A"]) for b in range(B)])
        ref64 = torch.cat([costgcn_stream(x[b:b + 1], sd, arch, sd["A"], dtype=torch.float64) for b in range(B)])
        emu = torch.cat([costgcn_stream(x[b:b + 1], sd, arch, sd["A"], round_bf16=True) for b in range(B)])
    return dict(arch=arch, m=m, sd=sd, x=x, ref32=ref32, ref64=ref64, emu=emu)


@pytest.fixture(scope="module")
def small(P):
    return case(P, 3, SMALL, 12, 5, 61)


@pytest.fixture(scope="module")
def wide(P):
    return case(P, 9, WIDE, 20, 2, 71)


# ------------------------------------------------------------------------------------------------ 1. goldens, staggered
@pytest.mark.parametrize("name", ["costgcn_k9", "costgcn_k69"])
def test_goldens_staggered(P, golden, name):
    """B = 3; stream b is skipped before tick b, restarted (code 2, over garbage state) at tick b and fed the
    fixture's frames from there: each equals the reference's own output."""
    g = golden(name)
    arch = dict(g["arch"], graph=P.PKU_MMD)
    m = P.MODELS["co-st-gcn"](rank=None, **arch)
    m.load_state_dict({k[3:]: v for k, v in g.items() if k.startswith("sd/")}, strict=True)
    m = m.to(DEV).eval()
    B, F = 3, g["x"].shape[2]
    x = torch.zeros(B, 3, F + B - 1, 25)
    codes = torch.zeros(F + B - 1, B, dtype=torch.int32)
    for b in range(B):
        x[b, :, b:b + F] = g["x"][0]
        codes[b:b + F, b] = 1
        codes[b, b] = 2
    batch = m.stream_batch(B)
    dirty(batch)
    y = run(batch, x.to(DEV), codes)
    fifo = max(arch["st-gcn"]["stride"]) * (arch["kernel"] - 1) + 1
    n = min(fifo, F)
    assert_close(y[0:1, :, :n], g["y"][:, :, :n], TOL, f"co streams {name} stream 0, first {n} frames")
    for b in range(B):
        assert_close(y[b:b + 1, :, b:b + F], g["y"], TOL, f"co streams {name} stream {b}")
        assert not y[b, :, :b].any() and not y[b, :, b + F:].any()   # skipped ticks give zero rows


# ------------------------------------------------------------------------------------------------ 2. small shapes
@pytest.mark.parametrize("B", [5, 1])
def test_small_shapes(P, small, B):
    """Kt = 3, 8 -> 8 (identity residual, one zero-padded tile, one k-step), 8 -> 16 and 16 -> 16 at stride 2 (fifo 5),
    12 frames (every ring wraps more than twice); B = 5 leaves the last tap group partial."""
    y = run(small["m"].stream_batch(B), small["x"][:B].to(DEV), None)
    assert_close(y, small["ref32"][:B], TOL, f"co streams small B={B} vs fp32")
    assert_close(y, small["ref64"][:B], TOL, f"co streams small B={B} vs fp64")


def test_wide_layer(P, wide):
    """64 -> 128 at stride 2, Kt = 9, 20 frames (fifo 17): four column tiles, several k-steps per wave."""
    y = run(wide["m"].stream_batch(2), wide["x"].to(DEV), None)
    assert_close(y, wide["ref32"], TOL, "co streams 64->128 vs fp32")
    assert_close(y, wide["ref64"], TOL, "co streams 64->128 vs fp64")


# ------------------------------------------------------------------------------------------------ 3. independence
def test_independence(P, small):
    """One stream's content (with a skip and a restart of its own) in slot 0 of B = 1, slot 4 of B = 5 and slot 70 of
    B = 71 (18 tap groups): bit-identical, whatever the other streams do; at tick 5 all the others are skipped."""
    m, T = small["m"], 12
    mine = torch.tensor([2, 1, 1, 0, 1, 1, 1, 2, 1, 1, 0, 1], dtype=torch.int32)
    xm = small["x"][0]
    outs = []
    for B, slot in ((1, 0), (5, 4), (71, 70)):
        gen = torch.Generator().manual_seed(100 + B)
        x = torch.randn(B, 3, T, 25, generator=gen)
        codes = torch.randint(0, 3, (T, B), generator=gen, dtype=torch.int32)
        codes[0] = 2
        codes[5] = 0
        x[slot], codes[:, slot] = xm, mine
        batch = m.stream_batch(B)
        dirty(batch)
        outs.append(run(batch, x.to(DEV), codes)[slot])
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # and it is the restatement's stream from each restart, over the frames it stepped
    arch, sd = small["arch"], small["sd"]
    for t0, t1 in ((0, 7), (7, 12)):
        keep = [t for t in range(t0, t1) if mine[t] != 0]
        with torch.no_grad():
            ref = costgcn_stream(xm[None, :, keep], sd, arch, sd["A"])
        assert_close(outs[0][None, :, keep], ref, TOL, f"co streams segment from tick {t0}")


# ------------------------------------------------------------------------------------------------ 4. skip
def test_skip_leaves_state_untouched(P, small):
    batch = small["m"].stream_batch(5)
    xd = small["x"].to(DEV)
    run(batch, xd[:, :, :4], None)
    before = [[t[2].clone() for t in ts] for ts in batch.state]
    y = batch.step(xd[:, :, 4:5].contiguous(), [1, 1, 0, 1, 1])
    torch.cuda.synchronize()
    for ts, bs in zip(batch.state, before):
        for t, b in zip(ts, bs):
            assert torch.equal(t[2], b)
    assert not y[2].any() and y[[0, 1, 3, 4]].abs().sum() > 0


# ------------------------------------------------------------------------------------------------ 5. forced splits
def test_forced_splits(P, wide):
    m, xd = wide["m"], wide["x"].to(DEV)
    base = m.stream_batch(2)
    y = run(base, xd, None)
    default = base._desc()[0].layers[0].splits
    assert default >= 1
    for n in (1, 7):
        b1 = m.stream_batch(2, splits=n)
        assert b1._desc()[0].layers[0].splits == n
        yn = run(b1, xd, None)
        assert_close(yn, y, TOL, f"co streams splits={n} vs default ({default})")
        assert torch.equal(run(m.stream_batch(2, splits=n), xd, None), yn)


# ------------------------------------------------------------------------------------------------ 6. graph replay
def test_graph_replay(P, small):
    """One captured tick replayed over 12 ticks whose mask changes every tick (restarts included) equals eager."""
    m, B, T = small["m"], 5, 12
    gen = torch.Generator().manual_seed(7)
    codes = torch.randint(0, 3, (T, B), generator=gen, dtype=torch.int32)
    codes[0] = 2
    xd = small["x"].to(DEV)
    eager = run(m.stream_batch(B), xd, codes)
    batch = m.stream_batch(B)
    x_static = torch.zeros(B, 3, 1, 25, device=DEV)
    a_static = torch.ones(B, dtype=torch.int32, device=DEV)
    batch.step(x_static, a_static)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph):
            y_static = batch.step(x_static, a_static)
    torch.cuda.current_stream().wait_stream(s)
    batch.reset()
    outs = []
    for t in range(T):
        x_static.copy_(xd[:, :, t:t + 1])
        a_static.copy_(codes[t])
        graph.replay()
        outs.append(y_static.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(outs, dim=2), eager)


# ------------------------------------------------------------------------------------------------ 7. bf16
@pytest.mark.parametrize("which", ["small", "wide"])
def test_bf16(P, small, wide, which):
    """bf16 tap weights and rings against the fp64 restatement; the bar is twice the error of the fp32 restatement
    with the bf16 mode's operands rounded, against the same fp64 result (as test_gpu_costgcn.test_bf16)."""
    c = small if which == "small" else wide
    B = c["x"].shape[0]
    m = P.MODELS["co-st-gcn"](rank=None, **c["arch"])
    m.load_state_dict(c["sd"], strict=True)
    m = m.to(DEV).eval().set_compute_dtype("bf16")
    batch = m.stream_batch(B)
    assert batch.state[0][0].dtype == torch.bfloat16 and batch.state[0][1].dtype == torch.float32
    y = run(batch, c["x"].to(DEV), None).double().cpu()
    ref = c["ref64"]
    scale = ref.abs().max().item()
    bar = (c["emu"].double() - ref).abs().max().item() / scale
    err = (y - ref).abs().max().item() / scale
    print(f"[err] co streams bf16 {which}: kernels {err:.3e}, bf16-rounded restatement {bar:.3e}", flush=True)
    assert err <= 2 * bar, f"bf16 error {err:.3e} > 2 x {bar:.3e}"


# ------------------------------------------------------------------------------------------------ 8. stale state
def test_stale_state(P):
    """tcn.0.bias of layer 0 updated in place mid-stream: the batch rebuilds and restarts, so the next frames are a
    fresh stream under the new parameters."""
    arch = make_arch(P.PKU_MMD, 3, **SMALL)
    m, sd = build(P, arch, 81)
    x = torch.randn(2, 3, 12, 25, generator=torch.Generator().manual_seed(83))
    batch = m.stream_batch(2)
    xd = x.to(DEV)
    run(batch, xd[:, :, :5], None)
    rings = [ts[0].data_ptr() for ts in batch.state]
    with torch.no_grad():
        m.gcn_networks[0].tcn[0].bias.add_(0.5)
    sd2 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    y = run(batch, xd, None)
    assert rings == [ts[0].data_ptr() for ts in batch.state]   # the state buffers survive the rebuild
    with torch.no_grad():
        ref = torch.cat([costgcn_stream(x[b:b + 1], sd2, arch, sd2["A"]) for b in range(2)])
        old = torch.cat([costgcn_stream(x[b:b + 1], sd, arch, sd["A"]) for b in range(2)])
    assert (ref - old).abs().max().item() > 10 * TOL * ref.abs().max().item()  # the change is visible
    assert_close(y, ref, TOL, "co streams after an in-place parameter update")


# ------------------------------------------------------------------------------------------------ 9. 17 joints
def test_coco_17_joints(P):
    g = np.load(f"{ROOT}/tests/golden/graphs.npz")
    V, center = (int(v) for v in g["meta/coco"])
    graph = {"num_node": V, "edge": g["edge/coco"].tolist(), "center": center}
    c = case(P, 3, dict(in_ch=[8, 8], out_ch=[8, 16], stride=[1, 2]), 8, 2, 91, V=V, graph=graph)
    y = run(c["m"].stream_batch(2), c["x"].to(DEV), None)
    assert_close(y, c["ref32"], TOL, "co streams coco")


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals(P, small):
    m = small["m"]
    with pytest.raises(RuntimeError):
        m.stream_batch(0)
    batch = m.stream_batch(2)
    assert batch.state_bytes == sum(t.numel() * t.element_size() for ts in batch.state for t in ts) > 0
    with pytest.raises(RuntimeError):
        batch.step(torch.zeros(3, 3, 1, 25, device=DEV))
    with pytest.raises(RuntimeError):
        batch.step(torch.zeros(2, 3, 2, 25, device=DEV))
    with pytest.raises(RuntimeError):
        batch.step(torch.zeros(2, 3, 1, 25, device=DEV), torch.ones(3, dtype=torch.int32, device=DEV))
    cpu = P.MODELS["co-st-gcn"](rank=None, **small["arch"])
    with pytest.raises(RuntimeError):
        cpu.stream_batch(2)
