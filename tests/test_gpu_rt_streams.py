"""Batched multi-stream per-frame inference of the online LayerNorm rt-st-gcn (Model.stream_batch ->
RtStreamBatch, stgcn_rt_streams / rt_streams.hip) on the MI355X: against the reference's own online outputs
(tests/golden/rt_*.npz), the oracle's online form and the model's existing single-stream route; the per-stream
mask (skip / step / restart), bit-exact independence of a stream from B, its slot and the other streams, HIP
graph replay, more streams than CUs, a 17-joint graph, and the refusals."""
import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, load_golden, sub

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3

CONFIG3_LAYERS = {"layers": 9, "kernel": 9, "in_ch": [64, 64, 64, 64, 128, 128, 128, 256, 256],
                  "out_ch": [64, 64, 64, 128, 128, 128, 256, 256, 256], "residual": [1] * 9, "dropout": [0.0] * 9,
                  "latency": False, "importance": True, "in_feat": 3, "buffer": 1, "stages": 1}


@pytest.fixture(scope="module")
def P(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return pkg


def _online(P, arch, sd):
    m = P.MODELS["rt-st-gcn"](rank=None, **arch)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    m.prepare_benchmark(arch)
    return m


def _randomise(m, seed):
    """Non-trivial norms, biases and edge importance (test_gpu_rt.py's recipe)."""
    sd = m.state_dict()
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if "edge_importance" in k:
            sd[k] = 1 + 0.1 * torch.randn(sd[k].shape, generator=g)
        elif ("bn_relu" in k or "residual.1" in k or "norm_in" in k) and k.endswith("weight"):
            sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
    return sd


def _run(sb, x, codes):
    """x (B, 3, T, V) on the device, codes [T][B] -> (B, K, T)."""
    outs = []
    for t in range(x.shape[2]):
        a = None if codes is None else torch.tensor(codes[t], dtype=torch.int32, device=DEV)
        outs.append(sb.step(x[:, :, t:t + 1], a))
    return torch.cat(outs, dim=2)


def _oracle(x, sd, arch):
    from oracle import stgcn_oracle as O
    with torch.no_grad():
        return O.rt_model_online(x, {k: v.clone() for k, v in sd.items()}, arch)


@pytest.mark.parametrize("case", ["stride1", "ref_strides"])
def test_streams_golden_staggered(P, case):
    """Three streams fed the golden frames, stream b starting at tick 2b through the mask: each reproduces the
    reference's online outputs, and the rows of its inactive ticks are exactly zero."""
    d = load_golden("rt_" + case)
    m = _online(P, d["arch"], sub(d, "sd/"))
    x = d["x"][:, :, :30].to(DEV)
    F_, V = x.shape[2], x.shape[3]
    sb = m.stream_batch(3)
    xin = torch.zeros(3, 3, F_ + 4, V, device=DEV)
    for b in range(3):
        xin[b, :, 2 * b:2 * b + F_] = x[0]
    codes = [[int(2 * b <= t < 2 * b + F_) for b in range(3)] for t in range(F_ + 4)]
    y = _run(sb, xin, codes)
    torch.cuda.synchronize()
    for b in range(3):
        assert_close(y[b:b + 1, :, 2 * b:2 * b + F_], d["y_online"][:, :, :F_], TOL, f"{case} stream {b}")
        idle = torch.cat([y[b, :, :2 * b], y[b, :, 2 * b + F_:]], dim=1)
        assert idle.shape[1] == 4 and torch.count_nonzero(idle).item() == 0, f"stream {b}: an inactive tick wrote a non-zero row"


def test_streams_config3_widths(P):
    """Config 3's widths with the reference strides, 5 distinct streams over 20 frames (> the 17-frame FIFO: the
    rings wrap), vs the oracle's online form per stream (1e-3) and vs the model's two-launches-per-layer
    single-stream route run stream by stream (1e-4, the bar between two fp32 routes of test_rt_frame_block_counts)."""
    arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": 9, "output_type": "logits",
            "normalization": "LayerNorm", "segment": 500, "num_classes": 52,
            "rt-st-gcn": dict(CONFIG3_LAYERS, stride=[1, 1, 1, 2, 1, 1, 2, 1, 1]), "graph": P.PKU_MMD}
    torch.manual_seed(31)
    m = P.MODELS["rt-st-gcn"](rank=None, **arch)
    sd = _randomise(m, 32)
    B, F_ = 5, 20
    x = torch.randn(B, 3, F_, 25, generator=torch.Generator().manual_seed(33))
    ref = torch.cat([_oracle(x[b:b + 1], sd, arch) for b in range(B)], dim=0)
    m = _online(P, arch, sd)
    xd = x.to(DEV)
    y = _run(m.stream_batch(B), xd, None)
    R = P.routing.ROUTING
    prev = R.rt_one_launch
    try:
        R.rt_one_launch = False
        single = []
        with torch.no_grad():
            for b in range(B):
                m.reset_state()
                single.append(torch.cat([m(xd[b:b + 1, :, i:i + 1]) for i in range(F_)], dim=2))
    finally:
        R.rt_one_launch = prev
    torch.cuda.synchronize()
    for b in range(B):
        assert_close(y[b:b + 1], ref[b:b + 1], TOL, f"config-3 stream {b} vs oracle")
    for b in range(B):
        assert_close(y[b:b + 1], single[b], 1e-4, f"config-3 stream {b} vs per-layer route")


# ---------------------------------------------------------------------------------- mask, restart, independence
T_MASK = 24
RESTART_AT = 11


def _mask_codes():
    codes = [[1, 1 - t % 2, 1, 0] for t in range(T_MASK)]
    codes[RESTART_AT][2] = 2
    return codes


@pytest.fixture(scope="module")
def mask_run(P):
    """The eager 24-tick run of the mask test on the golden narrow 9-layer model (shared with the graph test)."""
    d = load_golden("rt_ref_strides")
    sd = sub(d, "sd/")
    m = _online(P, d["arch"], sd)
    V = d["x"].shape[3]
    x = torch.randn(4, 3, T_MASK, V, generator=torch.Generator().manual_seed(41))
    xd = x.to(DEV)
    sb = m.stream_batch(4)
    y = _run(sb, xd, _mask_codes())
    torch.cuda.synchronize()
    return {"d": d, "sd": sd, "m": m, "x": x, "xd": xd, "sb": sb, "y": y}


def test_streams_mask_restart_independence(P, mask_run):
    r = mask_run
    arch, sd, m, x, xd, sb, y = r["d"]["arch"], r["sd"], r["m"], r["x"], r["xd"], r["sb"], r["y"]
    # stream 3 never ran: zero outputs, state still zero
    assert torch.count_nonzero(y[3]).item() == 0
    for ts in sb.state:
        for t in ts:
            assert torch.count_nonzero(t[3]).item() == 0, "an inactive stream's state was written"
    # stream 1 saw its even-tick frames only
    assert torch.count_nonzero(y[1, :, 1::2]).item() == 0
    assert_close(y[1:2, :, 0::2], _oracle(x[1:2, :, 0::2], sd, arch), TOL, "stream 1 (even ticks)")
    # stream 2 restarts at tick 11: from there on a from-scratch run of those frames
    assert_close(y[2:3, :, RESTART_AT:], _oracle(x[2:3, :, RESTART_AT:], sd, arch), TOL, "stream 2 after restart")
    assert_close(y[2:3, :, :RESTART_AT], _oracle(x[2:3, :, :RESTART_AT], sd, arch), TOL, "stream 2 before restart")
    # bit-exact independence from B, the slot and the other streams' masks
    one = m.stream_batch(1)
    assert torch.equal(_run(one, xd[0:1], None), y[0:1])
    one.reset()
    assert torch.equal(_run(one, xd[1:2, :, 0::2], None), y[1:2, :, 0::2])
    one.reset()
    assert torch.equal(_run(one, xd[2:3, :, RESTART_AT:], None), y[2:3, :, RESTART_AT:])
    # reset([1]) + the same frames: stream 1's first run bit for bit; the others go on from their state
    sb.reset([1])
    codes = [[0, 1 - t % 2, 0, 0] for t in range(T_MASK)]
    y2 = _run(sb, xd, codes)
    assert torch.equal(y2[1], y[1])


def test_streams_graph_replay(P, mask_run):
    """One captured step (static x, static int32 mask, the returned output) replayed over the mask test's 24
    ticks: the mask is read on the device, so the replay follows its changing values, bit-equal to eager."""
    r = mask_run
    m, xd = r["m"], r["xd"]
    sb = m.stream_batch(4)
    x_static = torch.zeros_like(xd[:, :, :1])
    a_static = torch.ones(4, dtype=torch.int32, device=DEV)
    sb.step(x_static, a_static)  # builds the descriptor and packs the weights outside the capture
    sb.reset()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph):
            y_static = sb.step(x_static, a_static)
    torch.cuda.current_stream().wait_stream(s)
    sb.reset()
    outs = []
    for t, c in enumerate(_mask_codes()):
        x_static.copy_(xd[:, :, t:t + 1])
        a_static.copy_(torch.tensor(c, dtype=torch.int32))
        graph.replay()
        outs.append(y_static.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(outs, dim=2), r["y"])


def test_streams_more_than_cus(P, mask_run):
    """B = 300 workgroups (> 256 CUs, they queue) fed copies of 4 distinct inputs: rows that share an input are
    bit-equal, and equal to a stream_batch(1) run."""
    r = mask_run
    m, xd = r["m"], r["xd"][:, :, :3]
    B = 300
    y = _run(m.stream_batch(B), xd.repeat(B // 4, 1, 1, 1), None)
    torch.cuda.synchronize()
    for k in range(4):
        one = _run(m.stream_batch(1), xd[k:k + 1], None)
        assert torch.equal(y[k::4], one.expand(B // 4, -1, -1)), f"input {k}"


def test_streams_coco_17_joints(P):
    """V = 17 (zero-padded rows of the 32-row MFMA operand), widths 8 -> 16 -> 16 (below one 32-channel tile), one
    stride-2 layer, a residual conv (res_mode 2), an identity residual (1) and a layer without residual (0)."""
    g = np.load(f"{ROOT}/tests/golden/graphs.npz")
    V, center = (int(v) for v in g["meta/coco"])
    graph = {"num_node": V, "edge": g["edge/coco"].tolist(), "center": center}
    conf = {"layers": 3, "kernel": 9, "in_ch": [8, 16, 16], "out_ch": [16, 16, 16], "stride": [2, 1, 1],
            "residual": [1, 0, 1], "dropout": [0.0] * 3, "latency": False, "importance": True, "in_feat": 3,
            "buffer": 1, "stages": 1}
    arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": 9, "output_type": "logits",
            "normalization": "LayerNorm", "segment": 500, "num_classes": 7, "rt-st-gcn": conf, "graph": graph}
    torch.manual_seed(51)
    m = P.MODELS["rt-st-gcn"](rank=None, **arch)
    sd = _randomise(m, 52)
    x = torch.randn(2, 3, 12, V, generator=torch.Generator().manual_seed(53))
    ref = torch.cat([_oracle(x[b:b + 1], sd, arch) for b in range(2)], dim=0)
    m = _online(P, arch, sd)
    assert [2 if l.is_residual_conv else int(l.is_residual) for l in m.st_gcn] == [2, 0, 1]
    y = _run(m.stream_batch(2), x.to(DEV), None)
    torch.cuda.synchronize()
    for b in range(2):
        assert_close(y[b:b + 1], ref[b:b + 1], TOL, f"coco stream {b}")


def test_streams_refusals(P):
    d = load_golden("rt_ref_strides")
    V = d["x"].shape[3]
    m = P.MODELS["rt-st-gcn"](rank=None, **d["arch"]).to(DEV).eval()
    with pytest.raises(RuntimeError, match="prepare_benchmark"):
        m.stream_batch(2)
    m.prepare_benchmark(d["arch"])
    with pytest.raises(RuntimeError, match="B >= 1"):
        m.stream_batch(0)
    sb = m.stream_batch(2)
    with pytest.raises(RuntimeError, match="shape"):
        sb.step(torch.zeros(3, 3, 1, V, device=DEV))
    with pytest.raises(RuntimeError, match="shape"):
        sb.step(torch.zeros(2, 3, 1, V + 1, device=DEV))
    with pytest.raises(RuntimeError, match="active"):
        sb.step(torch.zeros(2, 3, 1, V, device=DEV), [1, 1, 1])
    bn = P.MODELS["rt-st-gcn"](rank=None, **dict(d["arch"], normalization="BatchNorm")).to(DEV).eval()
    bn.prepare_benchmark(d["arch"])
    with pytest.raises(RuntimeError, match="LayerNorm"):
        bn.stream_batch(2)
