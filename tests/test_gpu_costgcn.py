"""co-st-gcn on the device (co_frame.hip): reference fixtures, reset, the reference's widths eager and as a replayed
HIP graph, split-K at full depth, bf16 against an fp64 restatement, and parameter changes mid-stream."""
import os
import sys

import pytest
import torch

from conftest import assert_close

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from costgcn_ref import costgcn_stream, randomise  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-3

WIDTHS = dict(in_ch=[64, 64, 64, 64, 128, 128, 128, 256, 256], out_ch=[64, 64, 64, 128, 128, 128, 256, 256, 256],
              stride=[1, 1, 1, 2, 1, 1, 2, 1, 1])


@pytest.fixture(scope="module")
def P(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return pkg


def make_arch(P, kernel, in_ch, out_ch, stride):
    nl = len(in_ch)
    return {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": 7, "graph": P.PKU_MMD,
            "st-gcn": {"importance": True, "in_feat": 3, "stages": 1, "layers": nl, "kernel": kernel,
                       "in_ch": list(in_ch), "out_ch": list(out_ch), "stride": list(stride), "dilation": [1] * nl,
                       "residual": [1] * nl, "dropout": [0.0] * nl}}


def stream(m, xd):
    with torch.no_grad():
        y = torch.cat([m(xd[:, :, i:i + 1]) for i in range(xd.shape[2])], dim=2)
    torch.cuda.synchronize()
    return y


def build(P, arch, seed):
    torch.manual_seed(seed)
    m = P.MODELS["co-st-gcn"](rank=None, **arch)
    sd = randomise(m.state_dict(), torch.Generator().manual_seed(seed + 1))
    m.load_state_dict(sd, strict=True)
    return m, sd


@pytest.fixture(scope="module")
def widths(P):
    """The reference schedule at Kt = 9 over 24 frames (> the 17-frame FIFO at stride 2): model parameters, the
    stream, and the restatement in fp32, in fp64, and in fp32 with the bf16 mode's operands rounded."""
    arch = make_arch(P, 9, **WIDTHS)
    m, sd = build(P, arch, 31)
    x = torch.randn(1, 3, 24, 25, generator=torch.Generator().manual_seed(33))
    with torch.no_grad():
        ref32 = costgcn_stream(x, sd, arch, sd["A"])
        ref64 = costgcn_stream(x, sd, arch, sd["A"], dtype=torch.float64)
        emu = costgcn_stream(x, sd, arch, sd["A"], round_bf16=True)
    return dict(arch=arch, sd=sd, x=x, ref32=ref32, ref64=ref64, emu=emu)


@pytest.mark.parametrize("name", ["costgcn_k9", "costgcn_k69"])
def test_goldens(P, golden, name):
    """Reference fixtures frame by frame, fp32; construct -> load_state_dict -> .to(DEV) (a ring initialised before
    the weights arrive would start from the wrong ReLU(tcn.0.bias)); the first fifo frames also on their own."""
    g = golden(name)
    arch = dict(g["arch"], graph=P.PKU_MMD)
    m = P.MODELS["co-st-gcn"](rank=None, **arch)
    m.load_state_dict({k[3:]: v for k, v in g.items() if k.startswith("sd/")}, strict=True)
    m = m.to(DEV).eval()
    y = stream(m, g["x"].to(DEV))
    assert_close(y, g["y"], TOL, f"co-st-gcn {name}")
    fifo = max(arch["st-gcn"]["stride"]) * (arch["kernel"] - 1) + 1
    n = min(fifo, y.shape[2])
    assert_close(y[:, :, :n], g["y"][:, :, :n], TOL, f"co-st-gcn {name} first {n} frames")
    # reset: the same stream again, bit for bit
    m.reset_state()
    assert torch.equal(stream(m, g["x"].to(DEV)), y)


def test_widths_eager_and_graph(P, widths):
    m = P.MODELS["co-st-gcn"](rank=None, **widths["arch"])
    m.load_state_dict(widths["sd"], strict=True)
    m = m.to(DEV).eval()
    xd = widths["x"].to(DEV)
    F_ = xd.shape[2]
    y = stream(m, xd)
    assert_close(y, widths["ref32"], TOL, "co-st-gcn widths eager")
    m.reset_state()
    x_static = torch.zeros_like(xd[:, :, :1])
    with torch.no_grad():
        for i in range(3):
            x_static.copy_(xd[:, :, i:i + 1])
            m(x_static)
        m.reset_state()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph):
                y_static = m(x_static)
        torch.cuda.current_stream().wait_stream(s)
        m.reset_state()
        outs = []
        for i in range(F_):
            x_static.copy_(xd[:, :, i:i + 1])
            graph.replay()
            outs.append(y_static.clone())
    torch.cuda.synchronize()
    yg = torch.cat(outs, dim=2)
    assert_close(yg, widths["ref32"], TOL, "co-st-gcn widths graph")
    assert torch.equal(yg, y)


def test_split_k_full_depth(P):
    """One 256 -> 256 layer at Kt = 69 (K = 17 664) over 75 frames; the forced split counts 1 and 7 against the
    default split."""
    arch = make_arch(P, 69, [256], [256], [1])
    m, sd = build(P, arch, 41)
    x = torch.randn(1, 3, 75, 25, generator=torch.Generator().manual_seed(43))
    with torch.no_grad():
        ref = costgcn_stream(x, sd, arch, sd["A"])
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    y = stream(m, xd)
    assert m._plan[1]["descs"][0].splits > 1
    assert_close(y, ref, TOL, "co-st-gcn 256x69 default split")
    for n in (1, 7):
        m.set_k_splits(n)
        yn = stream(m, xd)
        assert m._plan[1]["descs"][0].splits == n
        assert_close(yn, y, 1e-5, f"co-st-gcn 256x69 splits={n} vs default")


def test_bf16(P, widths):
    """bf16 tap weights and ring against the fp64 restatement.  The bar is 2x the error of the fp32 restatement with
    the tap and graph-conv weights and the ring entries rounded to bf16, against the same fp64 result (the factor 2
    covers summation order and rounding-boundary flips)."""
    m = P.MODELS["co-st-gcn"](rank=None, **widths["arch"])
    m.load_state_dict(widths["sd"], strict=True)
    m = m.to(DEV).eval().set_compute_dtype("bf16")
    y = stream(m, widths["x"].to(DEV)).double().cpu()
    ref = widths["ref64"]
    scale = ref.abs().max().item()
    bar = (widths["emu"].double() - ref).abs().max().item() / scale
    err = (y - ref).abs().max().item() / scale
    if os.environ.get("STGCN_TEST_REPORT"):
        print(f"[err] co-st-gcn bf16: kernels {err:.3e}, bf16-rounded restatement {bar:.3e} (bar {2 * bar:.3e})",
              flush=True)
    assert err <= 2 * bar, f"bf16 error {err:.3e} > 2 x {bar:.3e}"


def test_stale_state(P):
    """tcn.0.bias of layer 0 changed through load_state_dict mid-stream, then reset_state(): the stream must be the
    restatement's with the new parameters (the ring's initial content depends on that bias)."""
    arch = make_arch(P, 9, [8, 8, 16], [8, 16, 16], [1, 2, 1])
    m, sd = build(P, arch, 51)
    x = torch.randn(1, 3, 20, 25, generator=torch.Generator().manual_seed(53))
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    stream(m, xd[:, :, :7])
    sd2 = dict(sd)
    sd2["gcn_networks.0.tcn.0.bias"] = sd["gcn_networks.0.tcn.0.bias"] + 0.5
    m.load_state_dict(sd2, strict=True)
    m.reset_state()
    with torch.no_grad():
        ref = costgcn_stream(x, sd2, arch, sd2["A"])
        old = costgcn_stream(x, sd, arch, sd["A"])
    assert (ref - old).abs().max().item() > 10 * TOL * ref.abs().max().item()  # the change is visible
    assert_close(stream(m, xd), ref, TOL, "co-st-gcn after load_state_dict + reset_state")
