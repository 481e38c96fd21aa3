"""RtStreamBatch.step_clip (stgcn_rt_streams_clip, rt_streams_clip.hip) on the MI355X: B streams x T frames per call
on the stream batch's own state.  Against the reference's online outputs (tests/golden/rt_*.npz), against ``step`` tick
by tick, code 2 against reset + code 1, bit-exact independence from B, slot, T, neighbours and chunking, wide layers in
fp32 and bf16 against the fp64 restatement, graph replay with device-side codes and lengths, 17 joints, a parameter
change mid-stream and the BatchNorm refusal.  Bars are test_gpu_rt_streams.py's and test_gpu_rt_streams_bf16.py's."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, assert_close, load_golden, sub  # noqa: E402
from rt_streams_clip_ref import run_schedule, state_tensors  # noqa: E402
from test_gpu_rt_streams import _online, _randomise  # noqa: E402
from test_rt_streams_clip_cpu import small_net  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3        # test_gpu_rt_streams.py's bar against the reference's online outputs
TOL_ROUTES = 1e-4  # the project's bar between two fp32 routes (test_rt_frame_block_counts)


@pytest.fixture(scope="module")
def P(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return pkg


@pytest.fixture(scope="module")
def net(P):
    """The 4 -> 8 -> 8 -> 16 network on the device and 41 streams' worth of frames."""
    arch, sd = small_net(P, 25, 3)
    x = torch.randn(41, 3, 33, 25, generator=torch.Generator().manual_seed(61))
    return {"arch": arch, "sd": sd, "m": _online(P, arch, sd), "x": x, "xd": x.to(DEV)}


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _garbage(sb, seed):
    """Random FIFOs and accumulators, valid indices."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    for fifo, acc, idx in sb.state:
        fifo.normal_(generator=g)
        acc.normal_(generator=g)
        idx[:, 0] = torch.randint(0, fifo.shape[1], (idx.shape[0],), generator=g, device=DEV)
        idx[:, 1] = torch.randint(0, acc.shape[1], (idx.shape[0],), generator=g, device=DEV)


def _state(sb, b=None):
    return [t.clone() if b is None else t[b].clone() for ts in sb.state for t in ts]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("case", ["stride1", "ref_strides"])
def test_clip_golden_out_of_step(P, case):
    """Three streams over garbage state, restarted by code 2 and out of step through the lengths, and a skipped one:
    the T = 30 golden frames in one call reproduce the reference's online outputs; columns beyond n_b and the skipped
    stream's rows are exactly zero, and its garbage stays as it is."""
    d = load_golden("rt_" + case)
    m = _online(P, d["arch"], sub(d, "sd/"))
    T = 30
    x = d["x"][:, :, :T].to(DEV).expand(4, -1, -1, -1).contiguous()
    sb = m.stream_batch(4)
    _garbage(sb, 7)
    before = _state(sb, 3)
    lengths = (30, 27, 16, 30)
    y = sb.step_clip(x, _i32((2, 2, 2, 0)), _i32(lengths))
    torch.cuda.synchronize()
    assert y.shape == (4, d["y_online"].shape[1], T)
    for b in range(3):
        n = lengths[b]
        assert_close(y[b:b + 1, :, :n], d["y_online"][:, :, :n], TOL, f"{case} stream {b}")
        assert torch.count_nonzero(y[b, :, n:]).item() == 0
    assert torch.count_nonzero(y[3]).item() == 0 and _same(_state(sb, 3), before)


# ------------------------------------------------------------------------------------------------ against step
def test_clip_against_step(P, net):
    """Clips of lengths (0, 1, 5, 6, 33) and (8, 9, 10, 17, 18) of T = 33 (> the 17-slot FIFO: the scan subtracts its
    own z and the rings wrap), interleaved with step ticks, against a batch driven by step alone."""
    m, xd = net["m"], net["xd"][:5]
    T = 33
    extra = torch.randn(5, 3, 3, 25, generator=torch.Generator().manual_seed(62)).to(DEV)
    clip, tick = m.stream_batch(5), m.stream_batch(5)
    got, ref = [], []
    plan = [("clip", xd, (0, 1, 5, 6, 33)), ("step", extra[:, :, 0:1], None), ("step", extra[:, :, 1:2], None),
            ("clip", xd.flip(2), (8, 9, 10, 17, 18)), ("step", extra[:, :, 2:3], None)]
    for kind, x, lengths in plan:
        if kind == "step":
            got.append(clip.step(x))
            ref.append(tick.step(x))
            continue
        got.append(clip.step_clip(x, None, lengths))
        ref.append(torch.cat([tick.step(x[:, :, t:t + 1], _i32(int(t < n) for n in lengths)) for t in range(T)], dim=2))
    torch.cuda.synchronize()
    worst = max(_rel(g, r) for g, r in zip(got, ref))
    for (fc, ac, ic), (ft, at, it) in zip(clip.state, tick.state):
        worst = max(worst, _rel(fc, ft), _rel(ac, at))
        assert torch.equal(ic, it)
    print(f"[clip vs step] worst relative difference, outputs and state: {worst:.3e}", flush=True)
    assert worst <= TOL_ROUTES
    assert torch.count_nonzero(got[0][0]).item() == 0 and torch.count_nonzero(got[0][1, :, 1:]).item() == 0


# ------------------------------------------------------------------------------------------------ code 2
@pytest.mark.parametrize("n", [0, 3, 9, 20])
def test_clip_code2_is_reset_then_code1(P, net, n):
    m, xd = net["m"], net["xd"][:3, :, :20]
    a, b = m.stream_batch(3), m.stream_batch(3)
    alone = m.stream_batch(1)
    for sb in (a, b):
        sb.step_clip(net["xd"][:3, :, 20:25])
    alone.step_clip(net["xd"][:1, :, 20:25])
    idle = _state(a, 2)
    lengths = _i32((20, n, 7))
    ya = a.step_clip(xd, _i32((1, 2, 0)), lengths)
    b.reset([1])
    yb = b.step_clip(xd, _i32((1, 1, 0)), lengths)
    y1 = alone.step_clip(xd[:1])
    torch.cuda.synchronize()
    assert torch.equal(ya, yb) and _same(_state(a), _state(b))
    assert torch.equal(ya[0:1], y1) and _same(_state(a, 0), _state(alone, 0))
    assert _same(_state(a, 2), idle) and torch.count_nonzero(ya[2]).item() == 0
    assert torch.count_nonzero(ya[1, :, n:]).item() == 0
    if n == 0:
        assert all(torch.count_nonzero(t).item() == 0 for t in _state(a, 1)), "n = 0 leaves exactly the reset state"
    else:  # the slots a short clip does not write are cleared
        fifo, _, idx = a.state[0]
        assert torch.count_nonzero(fifo[1, n:]).item() == 0 and idx[1, 0].item() == n % fifo.shape[1]


# ------------------------------------------------------------------------------------------------ invariance
def test_clip_invariance(P, net):
    """One stream in slot 0 of 1, slot 4 of 5 and slot 40 of 41, its 33 frames in one call and in calls of
    (1, 2, 17, 13), clip_frames = 8 (chunks of 8, 1 and 1 frames), beside neighbours with other codes, lengths and
    contents: outputs and state are bit-identical."""
    m, xd = net["m"], net["xd"]
    want = None
    for B, slot in ((1, 0), (5, 4), (41, 40)):
        for split in ((33,), (1, 2, 17, 13)):
            sb = m.stream_batch(B)
            sb.clip_frames = 8
            _garbage(sb, 11 + B)
            for ts in sb.state:
                for t in ts:
                    t[slot] = 0
            x = xd[:B].roll(slot, 0).clone()  # the stream's frames are xd[0] in every batch
            x[slot] = xd[0]
            g = torch.Generator().manual_seed(B)
            outs, t0 = [], 0
            for j, n in enumerate(split):
                codes = torch.randint(0, 3, (B,), generator=g).tolist()
                lengths = torch.randint(-1, n + 2, (B,), generator=g).tolist()
                codes[slot], lengths[slot] = 1, n + j  # at or beyond the call's frames: all of them
                outs.append(sb.step_clip(x[:, :, t0:t0 + n], codes, lengths)[slot])
                t0 += n
            got = (torch.cat(outs, dim=1), _state(sb, slot))
            torch.cuda.synchronize()
            if want is None:
                want = got
            assert torch.equal(got[0], want[0]) and _same(got[1], want[1]), (B, slot, split)
    assert torch.count_nonzero(want[0]).item() > 0


# ------------------------------------------------------------------------------------------------ wide layers
def _wide_arch(P, cin, cout):
    conf = {"layers": 1, "kernel": 9, "in_ch": [cin], "out_ch": [cout], "stride": [1], "residual": [1],
            "dropout": [0.0], "latency": False, "importance": True, "in_feat": 3, "buffer": 1, "stages": 1}
    return {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": 9, "output_type": "logits",
            "normalization": "LayerNorm", "segment": 500, "num_classes": 5, "rt-st-gcn": conf, "graph": dict(P.PKU_MMD)}


@pytest.fixture(scope="module", params=[(64, 128), (256, 256)], ids=["c64_c128_resconv", "c256_c256"])
def wide(P, request):
    """fp32 and bf16 step_clip of B = 2, T = 20, lengths (20, 15), the fp64 restatement and the rounded one."""
    cin, cout = request.param
    arch = _wide_arch(P, cin, cout)
    torch.manual_seed(71 + cin)
    sd = _randomise(P.MODELS["rt-st-gcn"](rank=None, **arch), 72 + cin)
    x = torch.randn(2, 3, 20, 25, generator=torch.Generator().manual_seed(73))
    calls = [(x, None, (20, 15))]
    ref = run_schedule(calls, sd, arch)
    rounded = run_schedule(calls, sd, arch, dtype=torch.float32, round_bf16=True)
    m = _online(P, arch, sd)
    assert m.st_gcn[0].is_residual_conv == (cin != cout)
    out = {}
    for name in ("fp32", "bf16"):
        sb = m.stream_batch(2, name)
        out[name] = (sb.step_clip(x.to(DEV), None, (20, 15)).cpu(), [t.cpu() for t in _state(sb)])
    return {"ref": ref, "rounded": rounded, "out": out}


def test_clip_wide_fp32(wide):
    y, state = wide["out"]["fp32"]
    outs, states, _ = wide["ref"]
    e = _rel(y, outs[0])
    print(f"[wide fp32] {e:.3e}", flush=True)
    assert e <= 1e-4
    assert torch.count_nonzero(y[1, :, 15:]).item() == 0
    for b in range(2):
        fifo, acc, idx = state_tensors(states[b])[0]
        assert _rel(state[0][b], fifo) <= 1e-4 and _rel(state[1][b], acc) <= 1e-4 and torch.equal(state[2][b], idx)


def test_clip_wide_bf16(wide):
    """E against the fp64 restatement within 2 x E_ref, the rounded restatement's own error (DESIGN 4.18's rule)."""
    y, _ = wide["out"]["bf16"]
    ref = wide["ref"][0][0]
    e, e_ref = _rel(y, ref), _rel(wide["rounded"][0][0], ref)
    print(f"[wide bf16] E {e:.3e} E_ref {e_ref:.3e}", flush=True)
    assert e <= 2 * e_ref
    assert not torch.equal(y, wide["out"]["fp32"][0])


# ------------------------------------------------------------------------------------------------ more
def test_clip_graph_replay(P, net):
    """One captured step_clip (static x, codes, lengths) replayed over six calls whose codes and lengths change on the
    device between replays: bit-equal to the eager calls."""
    m, xd = net["m"], net["xd"][:3]
    T = 5
    plan = [((2, 1, 0), (5, 3, 5)), ((1, 1, 2), (0, 5, 2)), ((1, 0, 1), (4, 4, 9)), ((2, 2, 2), (5, 0, 1)),
            ((1, 1, 1), (5, 5, 5)), ((0, 1, 1), (5, -3, 5))]
    eager = m.stream_batch(3)
    want = [eager.step_clip(xd[:, :, T * j:T * j + T], _i32(c), _i32(n)) for j, (c, n) in enumerate(plan)]
    sb = m.stream_batch(3)
    x_s, a_s, l_s = torch.zeros_like(xd[:, :, :T]), _i32((1, 1, 1)), _i32((T, T, T))
    sb.step_clip(x_s, a_s, l_s)  # builds the descriptors and the scratch outside the capture
    sb.reset()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph):
            y_s = sb.step_clip(x_s, a_s, l_s)
    torch.cuda.current_stream().wait_stream(s)
    sb.reset()
    got = []
    for j, (c, n) in enumerate(plan):
        x_s.copy_(xd[:, :, T * j:T * j + T])
        a_s.copy_(torch.tensor(c, dtype=torch.int32))
        l_s.copy_(torch.tensor(n, dtype=torch.int32))
        graph.replay()
        got.append(y_s.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(got, dim=2), torch.cat(want, dim=2)) and _same(_state(sb), _state(eager))


def test_clip_coco_17_joints(P):
    """V = 17 (zero-padded rows of the 32-row MFMA operand), test_streams_coco_17_joints' network."""
    from oracle import stgcn_oracle as O
    g = np.load(f"{ROOT}/tests/golden/graphs.npz")
    V, center = (int(v) for v in g["meta/coco"])
    graph = {"num_node": V, "edge": g["edge/coco"].tolist(), "center": center}
    conf = {"layers": 3, "kernel": 9, "in_ch": [8, 16, 16], "out_ch": [16, 16, 16], "stride": [2, 1, 1],
            "residual": [1, 0, 1], "dropout": [0.0] * 3, "latency": False, "importance": True, "in_feat": 3,
            "buffer": 1, "stages": 1}
    arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": 9, "output_type": "logits",
            "normalization": "LayerNorm", "segment": 500, "num_classes": 7, "rt-st-gcn": conf, "graph": graph}
    torch.manual_seed(51)
    sd = _randomise(P.MODELS["rt-st-gcn"](rank=None, **arch), 52)
    x = torch.randn(2, 3, 12, V, generator=torch.Generator().manual_seed(53))
    with torch.no_grad():
        ref = torch.cat([O.rt_model_online(x[b:b + 1], {k: v.clone() for k, v in sd.items()}, arch) for b in range(2)])
    m = _online(P, arch, sd)
    y = m.stream_batch(2).step_clip(x.to(DEV))
    torch.cuda.synchronize()
    for b in range(2):
        assert_close(y[b:b + 1], ref[b:b + 1], TOL, f"coco stream {b}")


def test_clip_weights_follow_updates(P):
    """An in-place parameter update between clips is picked up by the next one (the images are repacked, the clip
    descriptors rebuilt) and the stream state survives, as with step."""
    arch, sd = small_net(P, 25, 3)
    m = _online(P, arch, sd)  # a model of its own: the update must not leak into the shared one
    x = torch.randn(2, 3, 10, 25, generator=torch.Generator().manual_seed(81)).to(DEV)
    sb = m.stream_batch(2)
    sb.step_clip(x[:, :, :6])
    saved, ptrs = _state(sb), [t.data_ptr() for ts in sb.state for t in ts]
    old = m.stream_batch(2)
    for t, s_ in zip([t for ts in old.state for t in ts], saved):
        t.copy_(s_)
    y_old = old.step_clip(x[:, :, 6:])
    with torch.no_grad():
        m.st_gcn[1].conv.weight.mul_(1.25)
        m.st_gcn[2].residual[0].weight.add_(0.05)
    y_new = sb.step_clip(x[:, :, 6:])
    assert [t.data_ptr() for ts in sb.state for t in ts] == ptrs, "the state buffers were reallocated"
    fresh = m.stream_batch(2)
    for t, s_ in zip([t for ts in fresh.state for t in ts], saved):
        t.copy_(s_)
    assert torch.equal(fresh.step_clip(x[:, :, 6:]), y_new)
    assert not torch.equal(y_new, y_old), "the update was not picked up"
    assert sb.scratch_bytes > 0 and sb.state_bytes == sum(t.numel() * t.element_size() for t in saved)


def test_clip_batchnorm_still_refused(P):
    d = load_golden("rt_ref_strides")
    bn = P.MODELS["rt-st-gcn"](rank=None, **dict(d["arch"], normalization="BatchNorm")).to(DEV).eval()
    bn.prepare_benchmark(d["arch"])
    with pytest.raises(RuntimeError, match="LayerNorm"):
        bn.stream_batch(2)
