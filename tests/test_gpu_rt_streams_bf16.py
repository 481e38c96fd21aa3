"""bf16 conv operands of the rt-st-gcn stream batch (Model.stream_batch(B, "bf16"), rt_streams_kernel<bf16>) on the
MI355X: parity with the fp64 oracle at 2 x the error of the bf16-rounded restatement (E_REF, recorded in
tests/test_rt_streams_bf16_cpu.py, which also holds the networks and inputs), bit-exact independence of a stream
from B, its slot and its neighbours, the mask codes, HIP graph replay, the untouched fp32 route, type fidelity and
in-place weight updates."""
import pytest
import torch

from test_rt_streams_bf16_cpu import CASES, E_REF, build_case, oracle_fp64, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def _run(sb, x, codes=None):
    """x (B, 3, T, V) on the device, codes [T][B] -> (B, K, T)."""
    outs = []
    for t in range(x.shape[2]):
        a = None if codes is None else torch.tensor(codes[t], dtype=torch.int32, device=DEV)
        outs.append(sb.step(x[:, :, t:t + 1], a))
    return torch.cat(outs, dim=2)


_cache = {}


def _case(P, name):
    """The case's online model on the device, its inputs and the fp64 oracle outputs, built once per module."""
    if name not in _cache:
        arch, sd, x = build_case(P, name)
        _cache[name] = {"arch": arch, "sd": sd, "x": x, "xd": x.to(DEV), "ref": oracle_fp64(x, sd, arch),
                        "m": _online(P, arch, sd)}
    return _cache[name]


# ------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity(P, name):
    """bf16 stream outputs against the fp64 oracle over >= 2 x the longest FIFO; bar 2 x E_ref.  Measured on the
    MI355X (this test's [err] lines): see DESIGN 4.19 'Parity'."""
    c = _case(P, name)
    modes = sorted({2 if l.is_residual_conv else int(l.is_residual) for l in c["m"].st_gcn})
    sb = c["m"].stream_batch(c["x"].shape[0], "bf16")
    assert sb.dtype == torch.bfloat16
    y = _run(sb, c["xd"]).cpu()
    err = rel_err(y, c["ref"])
    print(f"[err] rt streams bf16 {name} (residual modes {modes}): kernel {err:.3e}, restatement {E_REF[name]:.3e}",
          flush=True)
    assert err <= 2 * E_REF[name], f"bf16 error {err:.3e} > 2 x {E_REF[name]:.3e}"


def test_residual_modes_all_present(P):
    seen = set()
    for name in CASES:
        seen |= {2 if l.is_residual_conv else int(l.is_residual) for l in _case(P, name)["m"].st_gcn}
    assert seen == {0, 1, 2}


# ------------------------------------------------------------------------------ fp32 untouched, type fidelity
def test_fp32_untouched_and_type_fidelity(P):
    name = "small_v25_p3"
    c = _case(P, name)
    m, xd, B = c["m"], c["xd"], c["x"].shape[0]
    y_def = _run(m.stream_batch(B), xd)
    sb32 = m.stream_batch(B, "fp32")
    assert sb32.dtype == torch.float32 and m.stream_batch(B, torch.float32).dtype == torch.float32
    assert torch.equal(_run(sb32, xd), y_def)
    assert rel_err(y_def.cpu(), c["ref"]) < 1e-5, "the default batch is the exact-fp32 route"
    try:
        m.set_compute_dtype("bf16")
        sb = m.stream_batch(B)
        assert sb.dtype == torch.float32
        assert torch.equal(_run(sb, xd), y_def), "set_compute_dtype changed stream_batch(B)"
    finally:
        m.set_compute_dtype("fp32")
    sbb = m.stream_batch(B, torch.bfloat16)
    y_bf = _run(sbb, xd)
    assert torch.equal(y_bf, _run(m.stream_batch(B, "bf16"), xd))
    assert not torch.equal(y_bf, y_def), "the operand type is ignored"
    d = ((y_bf - y_def).abs().max() / y_def.abs().max()).item()
    print(f"[err] rt streams bf16 vs fp32 {name}: {d:.3e}", flush=True)
    assert 0 < d <= 2 * E_REF[name]
    assert sbb.state_bytes == sb32.state_bytes == sum(t.numel() * t.element_size() for ts in sbb.state for t in ts)
    assert all(t.dtype == torch.float32 for ts in sbb.state for t in ts[:2])
    # a batch holds the weight images of its own type only
    kinds = lambda sb: {t.dtype for t in sb._desc()[1]}  # noqa: E731
    assert torch.bfloat16 in kinds(sbb) and torch.bfloat16 not in kinds(sb32)
    with pytest.raises(RuntimeError, match=r"fp32.*bf16"):
        m.stream_batch(B, torch.float16)


# ------------------------------------------------------------------------------- independence and the masks
T_MASK = 12
RESTART_AT = 7


def _mask_codes():
    """slot 0 steps, 1 steps on even ticks, 2 restarts mid-run, 3 never runs, 4 steps."""
    codes = [[1, 1 - t % 2, 1, 0, 1] for t in range(T_MASK)]
    codes[RESTART_AT][2] = 2
    return codes


@pytest.fixture(scope="module")
def mask_run(P):
    c = _case(P, "small_v25_p3")
    x = torch.randn(5, 3, T_MASK, 25, generator=torch.Generator().manual_seed(811))
    xd = x.to(DEV)
    sb = c["m"].stream_batch(5, "bf16")
    y = _run(sb, xd, _mask_codes())
    torch.cuda.synchronize()
    return {"m": c["m"], "xd": xd, "sb": sb, "y": y}


def test_independence_and_masks(P, mask_run):
    m, xd, sb, y = (mask_run[k] for k in ("m", "xd", "sb", "y"))
    # active = 0: zero rows, state untouched (slot 3 never ran: still zero)
    assert torch.count_nonzero(y[3]).item() == 0 and torch.count_nonzero(y[1, :, 1::2]).item() == 0
    for ts in sb.state:
        for t in ts:
            assert torch.count_nonzero(t[3]).item() == 0, "an inactive stream's state was written"
    # B = 1 against slots of B = 5, with neighbours that skip and restart
    one = m.stream_batch(1, "bf16")
    assert torch.equal(_run(one, xd[0:1]), y[0:1])
    one.reset()
    assert torch.equal(_run(one, xd[4:5]), y[4:5])
    one.reset()
    assert torch.equal(_run(one, xd[1:2, :, 0::2]), y[1:2, :, 0::2]), "skipped ticks must not touch the state"
    # active = 2 equals a fresh batch; the frames before it equal a fresh batch too
    assert torch.equal(_run(m.stream_batch(1, "bf16"), xd[2:3, :, RESTART_AT:]), y[2:3, :, RESTART_AT:])
    assert torch.equal(_run(m.stream_batch(1, "bf16"), xd[2:3, :, :RESTART_AT]), y[2:3, :, :RESTART_AT])
    # a different slot: stream 0's frames in slot 3 of the same batch after reset([3])
    x2 = xd.clone()
    x2[3] = xd[0]
    sb.reset([3])
    y2 = _run(sb, x2, [[0, 0, 0, 1, 0] for _ in range(T_MASK)])
    assert torch.equal(y2[3], y[0])
    # reset(streams) equals active = 2: slot 3 again, over its now dirty state, both ways
    sb.reset([3])
    y3 = _run(sb, x2[:, :, :4], [[0, 0, 0, 1, 0] for _ in range(4)])
    y4 = _run(sb, x2[:, :, :4], [[0, 0, 0, 2 if t == 0 else 1, 0] for t in range(4)])
    assert torch.equal(y3[3], y[0, :, :4]) and torch.equal(y4[3], y[0, :, :4])


def test_more_streams_than_cus(P, mask_run):
    """B = CU count + 3 workgroups (they queue), fed copies of 4 inputs: rows that share an input are bit-equal and
    equal a stream_batch(1) run."""
    m, xd = mask_run["m"], mask_run["xd"][:4, :, :3]
    B = torch.cuda.get_device_properties(0).multi_processor_count + 3
    xin = xd.repeat(-(-B // 4), 1, 1, 1)[:B]
    y = _run(m.stream_batch(B, "bf16"), xin)
    torch.cuda.synchronize()
    for k in range(4):
        one = _run(m.stream_batch(1, "bf16"), xd[k:k + 1])
        rows = y[k::4]
        assert torch.equal(rows, one.expand(rows.shape[0], -1, -1)), f"input {k}"


def test_graph_replay(P, mask_run):
    """One captured tick replayed over the mask run's ticks with `active` changed between replays: bit-equal to
    eager."""
    m, xd = mask_run["m"], mask_run["xd"]
    sb = m.stream_batch(5, "bf16")
    x_static = torch.zeros_like(xd[:, :, :1])
    a_static = torch.ones(5, dtype=torch.int32, device=DEV)
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
    assert torch.equal(torch.cat(outs, dim=2), mask_run["y"])


# --------------------------------------------------------------------------------------- weights follow updates
def test_weights_follow_updates(P):
    """An in-place parameter update between ticks is picked up by the next step (the bf16 images are repacked), and
    the stream state survives the rebuild."""
    arch, sd, x = build_case(P, "small_v25_p3")
    m = _online(P, arch, sd)  # a model of its own: the update must not leak into the shared one
    xd = x.to(DEV)
    B = xd.shape[0]
    sb = m.stream_batch(B, "bf16")
    _run(sb, xd[:, :, :6])
    saved = [[t.clone() for t in ts] for ts in sb.state]
    ptrs = [t.data_ptr() for ts in sb.state for t in ts]
    old = m.stream_batch(B, "bf16")
    for ts, ss in zip(old.state, saved):
        for t, s_ in zip(ts, ss):
            t.copy_(s_)
    y_old = old.step(xd[:, :, 6:7])
    with torch.no_grad():
        m.st_gcn[1].conv.weight.mul_(1.25)
        m.st_gcn[0].residual[0].weight.add_(0.05)
    y_new = sb.step(xd[:, :, 6:7])
    assert [t.data_ptr() for ts in sb.state for t in ts] == ptrs, "the state buffers were reallocated"
    fresh = m.stream_batch(B, "bf16")  # packs the updated weights; given the saved state
    for ts, ss in zip(fresh.state, saved):
        for t, s_ in zip(ts, ss):
            t.copy_(s_)
    assert torch.equal(fresh.step(xd[:, :, 6:7]), y_new)
    assert not torch.equal(y_new, y_old), "the update was not picked up"
