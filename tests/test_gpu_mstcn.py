"""ms-tcn / ms-gcn on the device (ms_stage.hip): reference fixtures forward and backward, tile edges at the reference
width, the class widths of the small-width ends, bf16 against an fp64 restatement, run-to-run determinism, a replayed
HIP graph of the ms-gcn forward, the multi-stage loss and statistics, and one ms-gcn training step."""
import os
import sys

import pytest
import torch

from conftest import assert_close, grad_floor, sub

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mstcn_ref as R  # noqa: E402
from oracle import stgcn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-3


@pytest.fixture(scope="module")
def P(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return pkg


def make_stage(P, cin, cout, F_, nl, seed):
    torch.manual_seed(seed)
    st = P.mstcn.SingleStage(in_channels=cin, out_channels=cout, num_filters=F_, num_layers=nl, kernel=3, dropout=0.0)
    sd = R.randomise(st.state_dict(), torch.Generator().manual_seed(seed + 1))
    st.load_state_dict(sd, strict=True)
    return st, sd


def run_stage(st, x, g, dtype=None):
    """Forward + backward of sum(y * g) on the device -> (y, {param grads}, dx), all on the CPU."""
    st = st.to(DEV).train()
    st.compute_dtype = dtype or torch.float32
    st.zero_grad()
    xd = x.to(DEV).requires_grad_(True)
    y = st(xd)
    (y * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), {k: p.grad.cpu().clone() for k, p in st.named_parameters()}, xd.grad.cpu()


def check_all(y, grads, dx, ry, rgrads, rdx, name):
    assert_close(y, ry, TOL, f"{name} y")
    assert set(grads) == set(rgrads)
    for k, v in rgrads.items():
        assert_close(grads[k], v, TOL, f"{name} grad {k}", grad_floor(rgrads, k))
    if rdx is not None:
        assert_close(dx, rdx, TOL, f"{name} dx")


@pytest.mark.parametrize("V", [1, 3])
def test_golden_stage(P, golden, V):
    g = golden("mstcn_stage")
    p = f"v{V}/"
    st = P.mstcn.SingleStage(in_channels=7, out_channels=7, num_filters=16, num_layers=6, kernel=3, dropout=0.0)
    st.load_state_dict(sub(g, "sd/"), strict=True)
    y, grads, dx = run_stage(st, g[p + "x"], g[p + "g"])
    check_all(y, grads, dx, g[p + "y"], sub(g, p + "grad/"), g[p + "dx"], f"ms stage V={V}")


def model_input(g, name):
    return R.windows(g["capture"], g["arch"]["receptive_field"]) if name == "msgcn_model" else g["x"]


def load_model(P, g, name):
    arch = g["arch"]
    m = P.MODELS["ms-gcn" if name == "msgcn_model" else "ms-tcn"](rank=None, **arch)
    m.load_state_dict(sub(g, "sd/"), strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("name", ["mstcn_model", "msgcn_model", "mstcn_logsoftmax"])
def test_golden_models(P, golden, name):
    g = golden(name)
    m = load_model(P, g, name).train()
    y = m(model_input(g, name).to(DEV))
    assert y.dtype == torch.float32 and y.shape == g["y"].shape
    (y * g["g"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.cpu() for k, p in m.named_parameters()}
    check_all(y.detach().cpu(), grads, None, g["y"], sub(g, "grad/"), None, name)


@pytest.fixture(scope="module")
def wide(P):
    """One stage at the reference width (F = 64, 10 layers, dilations up to 512) with its inputs for the three tile
    cases, and the restatement's forward and backward of the largest one in fp64, fp32 and with bf16-rounded operands
    (computed once, shared, never modified)."""
    st, sd = make_stage(P, 7, 7, 64, 10, 61)
    gen = torch.Generator().manual_seed(63)
    cases = {}
    for Lx, V in ((1, 1), (65, 1), (130, 25)):
        x = torch.randn(1, 7, Lx, V, generator=gen)
        g = torch.randn(1, 7, Lx, V, generator=gen)
        cases[(Lx, V)] = (x, g, R.grads_of(lambda a, s: R.single_stage(a, s), x, sd, g, torch.float64, True))
    x, g, _ = cases[(130, 25)]
    ref32 = R.grads_of(lambda a, s: R.single_stage(a, s), x, sd, g, torch.float32, True)
    emu = R.grads_of(lambda a, s: R.single_stage(a, s, round_bf16=True), x, sd, g, torch.float32, True)
    return dict(st=st, cases=cases, ref32=ref32, emu=emu)


@pytest.mark.parametrize("Lx,V", [(1, 1), (65, 1), (130, 25)])
def test_tile_edges(P, wide, Lx, V):
    """A single row; one full + one 1-row partial tile with every dilation >= 128 out of range; 3250 rows over 26
    workgroups where the neighbour tiles of d*V = 800 .. 12800 rows fall out of range on one side or both."""
    x, g, (ry, rgrads, rdx) = wide["cases"][(Lx, V)]
    y, grads, dx = run_stage(wide["st"], x, g)
    check_all(y, grads, dx, ry, rgrads, rdx, f"ms stage F=64 L={Lx} V={V}")


@pytest.mark.parametrize("C,V,mode", [(52, 1, "softmax"), (3, 3, "logsoftmax"), (52, 1, "logits")])
def test_class_widths(P, C, V, mode):
    """ms_in / ms_out at C = 52 and C = 3 through the fused selector, with the joint mean at V = 3."""
    st, sd = make_stage(P, C, C, 16, 2, 71 + C)
    gen = torch.Generator().manual_seed(73)
    x = torch.randn(1, C, 41, V, generator=gen)
    g = torch.randn(41, C, generator=gen)
    sel = R.selector(mode)

    def fn(a, s):
        y = R.single_stage(sel(a), s)
        return y.mean(dim=3)[0].t()
    ry, rgrads, rdx = R.grads_of(fn, x, sd, g, torch.float64, True)
    st = st.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    rows = xd[0].permute(1, 2, 0).reshape(41 * V, C)
    y = st.run_rows(rows, V, V, P.native.MS_MODES[mode])
    (y * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.cpu() for k, p in st.named_parameters()}
    check_all(y.detach().cpu(), grads, xd.grad.cpu(), ry, rgrads, rdx, f"ms widths C={C} V={V} {mode}")


def test_bf16(P, wide):
    """bf16 operands against the fp64 restatement.  The bar is 2x the error of the fp32 restatement with the layers'
    weights, the operands staged into both GEMMs and h rounded to bf16, against the same fp64 result (the factor 2
    covers summation order and rounding-boundary flips).  Every gradient keeps cosine >= 0.95 to fp32."""
    x, g, (ry, _, _) = wide["cases"][(130, 25)]
    y, grads, dx = run_stage(wide["st"], x, g, torch.bfloat16)
    scale = ry.abs().max().item()
    bar = (wide["emu"][0].double() - ry).abs().max().item() / scale
    err = (y.double() - ry).abs().max().item() / scale
    if os.environ.get("STGCN_TEST_REPORT"):
        print(f"[err] ms stage bf16: kernels {err:.3e}, bf16-rounded restatement {bar:.3e} (bar {2 * bar:.3e})",
              flush=True)
    assert err <= 2 * bar, f"bf16 error {err:.3e} > 2 x {bar:.3e}"
    _, g32, dx32 = wide["ref32"]
    for k, v in list(g32.items()) + [("dx", dx32)]:
        got = dx if k == "dx" else grads[k]
        cos = torch.nn.functional.cosine_similarity(got.flatten().double(), v.flatten().double(), dim=0).item()
        if os.environ.get("STGCN_TEST_REPORT"):
            print(f"[cos] ms stage bf16 {k}: {cos:.5f}", flush=True)
        assert cos >= 0.95, f"bf16 gradient {k}: cosine {cos:.4f}"


def test_determinism(P, wide):
    x, g, _ = wide["cases"][(130, 25)]
    a = run_stage(wide["st"], x, g)
    b = run_stage(wide["st"], x, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_graph_capture(P, golden):
    """The ms-gcn inference forward at the fixture shape: a captured HIP graph replays bit-identically to eager."""
    g = golden("msgcn_model")
    m = load_model(P, g, "msgcn_model").eval()
    x = model_input(g, "msgcn_model").to(DEV)
    with torch.no_grad():
        eager = m(x).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                m(x)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                y_static = m(x)
        torch.cuda.current_stream().wait_stream(s)
        y_static.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert_close(eager, g["y"], TOL, "ms-gcn eval forward")
    assert torch.equal(y_static, eager)


def test_multistage_loss_and_statistics(P):
    gen = torch.Generator().manual_seed(81)
    pred = torch.randn(3, 1, 7, 20, generator=gen)
    labels = torch.randint(0, 7, (1, 19), generator=gen)
    dist = torch.rand(7, generator=gen) + 0.1
    pr = pred.clone().requires_grad_(True)
    ce = sum(O.loss(1, pr[k], labels, dist)[0] for k in range(3))
    mse = sum(O.loss(1, pr[k], labels, dist)[1] for k in range(3))
    (ce + mse).backward()
    pd = pred.to(DEV).requires_grad_(True)
    gce, gmse = P.loss.LossMultiStage(DEV, dist)(1, pd, labels.to(DEV))
    (gce + gmse).backward()
    assert_close(gce, ce, TOL, "multi-stage ce")
    assert_close(gmse, mse, TOL, "multi-stage mse")
    assert_close(pd.grad, pr.grad, TOL, "multi-stage dpred")
    got = P.loss.StatisticsMultiStage()(1, pd.detach(), labels.to(DEV))
    ref = O.statistics(1, pred[-1], labels)
    assert torch.equal(got[0].cpu(), ref[0]) and got[2:] == ref[2:]


def test_training_step(P, golden):
    """One step of the msgcn_model fixture: LossMultiStage, backward, optim.Adam.  The loss equals the restatement's
    and every parameter moves, the generator's included (the gradient crosses the series reshape)."""
    g = golden("msgcn_model")
    arch, sd = g["arch"], sub(g, "sd/")
    x = model_input(g, "msgcn_model")
    gen = torch.Generator().manual_seed(91)
    labels = torch.randint(0, 7, (1, x.shape[0]), generator=gen)
    dist = torch.rand(7, generator=gen) + 0.1
    with torch.no_grad():
        ry = R.msgcn_model(x, sd, arch)
    ref = sum(sum(O.loss(0, ry[k], labels, dist)) for k in range(ry.shape[0])).item()
    m = load_model(P, g, "msgcn_model").train()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = P.optim.Adam(m.parameters(), lr=1e-3)
    ce, mse = P.loss.LossMultiStage(DEV, dist)(0, m(x.to(DEV)), labels.to(DEV))
    loss = ce + mse
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert abs(loss.item() - ref) <= TOL * abs(ref), f"loss {loss.item():.6f} vs restatement {ref:.6f}"
    same = [k for k, p in m.named_parameters() if torch.equal(p.detach(), before[k])]
    assert not same, f"parameters untouched by the step: {same}"
