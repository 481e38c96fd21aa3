"""Input heads with other than 3 features per joint on the MI355X: every online route of rt-st-gcn and co-st-gcn at
in_feat 6 on the reference's 7-node IMU graph (tests/golden/rt_infeat6.npz, costgcn_infeat6.npz: the reference's own
outputs), the edge shapes of the head (F * V = 2, 2-D pose, the 16 x 32 LDS bound over a 4-channel first layer, a
count that is no multiple of 4) against the fp64 references, the bitwise relations the in_feat-3 tests assert, bf16
and the refusals.  Bars are those of the in_feat-3 tests of each route (1e-3 of max|ref|); the bf16 bar is twice the
error of the reference restated with the kernels' rounding points (DESIGN 4.18's rule)."""
import os
import sys
from importlib import import_module

import pytest
import torch

from conftest import assert_close, load_golden, sub
from test_rt_streams_bf16_cpu import oracle_fp64, rel_err, restatement

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from costgcn_ref import costgcn_stream, randomise  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3  # test_gpu_rt.py, test_gpu_rt_streams.py, test_gpu_costgcn.py, test_gpu_co_streams.py, test_gpu_co_clip.py


@pytest.fixture(scope="module")
def P(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return pkg


# ------------------------------------------------------------------------------------------------ models and runs
def rt_online(P, arch, sd):
    m = P.MODELS["rt-st-gcn"](rank=None, **arch)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    m.prepare_benchmark(arch)
    return m


def co_model(P, arch, sd, dtype=None):
    m = P.MODELS["co-st-gcn"](rank=None, **arch)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    return m.set_compute_dtype(dtype) if dtype else m


def ticks(batch, x, codes=None):
    """x (B, F, T, V) on the device one tick at a time, codes [T][B] (None: every stream steps) -> (B, K, T)."""
    outs = []
    for t in range(x.shape[2]):
        a = None if codes is None else torch.tensor(codes[t], dtype=torch.int32, device=DEV)
        outs.append(batch.step(x[:, :, t:t + 1], a))
    torch.cuda.synchronize()
    return torch.cat(outs, dim=2)


def frames(m, x):
    with torch.no_grad():
        y = torch.cat([m(x[:, :, t:t + 1]) for t in range(x.shape[2])], dim=2)
    torch.cuda.synchronize()
    return y


def clips(m, x, n):
    """x through co-st-gcn's forward_clip in consecutive clips of n frames."""
    with torch.no_grad():
        y = torch.cat([m.forward_clip(x[:, :, t:t + n]) for t in range(0, x.shape[2], n)], dim=2)
    torch.cuda.synchronize()
    return y


@pytest.fixture(scope="module")
def rt6(P):
    """The rt fixture's model on the device, and five streams of 24 random frames (the FIFOs hold 9 and 17) with the
    oracle's fp64 outputs."""
    d = load_golden("rt_infeat6")
    sd = sub(d, "sd/")
    x = torch.randn(5, 6, 24, 7, generator=torch.Generator().manual_seed(611)) * 2 + 0.5
    return dict(d=d, arch=d["arch"], sd=sd, m=rt_online(P, d["arch"], sd), x=x, xd=x.to(DEV),
                ref64=oracle_fp64(x, sd, d["arch"]))


@pytest.fixture(scope="module")
def co6(P):
    g = load_golden("costgcn_infeat6")
    sd = sub(g, "sd/")
    x = torch.randn(5, 6, 24, 7, generator=torch.Generator().manual_seed(711)) * 2 + 0.5
    with torch.no_grad():
        ref64 = torch.cat([costgcn_stream(x[b:b + 1], sd, g["arch"], sd["A"], dtype=torch.float64) for b in range(5)])
    return dict(g=g, arch=g["arch"], sd=sd, m=co_model(P, g["arch"], sd), x=x, xd=x.to(DEV), ref64=ref64)


# ------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("route", ["one_launch", "per_layer"])
def test_rt_golden_single_stream(P, rt6, route, monkeypatch):
    """The one-launch route (stgcn_rt_frame) and the two-launches-per-layer route (stgcn_rt_frame_in_f first), not the
    generic kernels an in_feat other than 3 used to fall back to: the fused input head is counted."""
    native = import_module(P.__name__ + ".native")
    heads, head = [], native.rt_frame_in
    monkeypatch.setattr(native, "rt_frame_in", lambda *a: (heads.append(1), head(*a))[1])
    monkeypatch.setattr(P.routing.ROUTING, "rt_one_launch", route == "one_launch")
    m, d = rt6["m"], rt6["d"]
    m.reset_state()
    y = frames(m, d["x"].to(DEV))
    assert_close(y, d["y_online"], TOL, f"rt_infeat6 {route}")
    if route == "one_launch":  # the fast route ran (it builds the status word), and its barrier never gave up
        st = getattr(m, "_frame_status", None)
        assert not heads and st is not None and int(st.item()) == 0
    else:
        assert len(heads) == d["x"].shape[2], "the per-layer route did not take the fused input head"


def _staggered(batch, x1, F):
    """Three streams fed the fixture's frames, stream b from tick 2b through the mask (test_gpu_rt_streams.py)."""
    T, V = x1.shape[2], x1.shape[3]
    xin = torch.zeros(3, F, T + 4, V, device=DEV)
    for b in range(3):
        xin[b, :, 2 * b:2 * b + T] = x1[0]
    codes = [[int(2 * b <= t < 2 * b + T) for b in range(3)] for t in range(T + 4)]
    return ticks(batch, xin, codes)


def test_rt_golden_stream_batch_step(rt6):
    d = rt6["d"]
    T = d["x"].shape[2]
    y = _staggered(rt6["m"].stream_batch(3), d["x"].to(DEV), 6)
    for b in range(3):
        assert_close(y[b:b + 1, :, 2 * b:2 * b + T], d["y_online"], TOL, f"rt_infeat6 step stream {b}")
        idle = torch.cat([y[b, :, :2 * b], y[b, :, 2 * b + T:]], dim=1)
        assert torch.count_nonzero(idle).item() == 0


def test_rt_golden_stream_batch_step_clip(rt6):
    """Streams of lengths 40, 25 and 0 in one clip: the consumed columns are the reference's, the rest zero."""
    d = rt6["d"]
    T = d["x"].shape[2]
    lengths = [T, 25, 0]
    y = rt6["m"].stream_batch(3).step_clip(d["x"].to(DEV).expand(3, -1, -1, -1).contiguous(), None, lengths)
    torch.cuda.synchronize()
    for b, n in enumerate(lengths):
        if n:
            assert_close(y[b:b + 1, :, :n], d["y_online"][:, :, :n], TOL, f"rt_infeat6 step_clip stream {b}")
        assert torch.count_nonzero(y[b, :, n:]).item() == 0


def test_co_golden_forward_and_forward_clip(co6):
    g, m = co6["g"], co6["m"]
    xd = g["x"].to(DEV)
    m.reset_state()
    assert_close(frames(m, xd), g["y"], TOL, "costgcn_infeat6 forward")
    m.reset_state()
    y = clips(m, xd, xd.shape[2])
    assert_close(y, g["y"], TOL, "costgcn_infeat6 forward_clip")
    for n in (1, 3, 18):  # 18 = the longest FIFO + 1
        m.reset_state()
        assert torch.equal(clips(m, xd, n), y), f"costgcn_infeat6: clips of {n}"


def test_co_golden_stream_batch_step_and_step_clip(co6):
    g, m = co6["g"], co6["m"]
    xd = g["x"].to(DEV)
    T = xd.shape[2]
    y = _staggered(m.stream_batch(3), xd, 6)
    for b in range(3):
        assert_close(y[b:b + 1, :, 2 * b:2 * b + T], g["y"], TOL, f"costgcn_infeat6 step stream {b}")
    lengths = [T, 25, 0]
    yc = m.stream_batch(3).step_clip(xd.expand(3, -1, -1, -1).contiguous(), None, lengths)
    torch.cuda.synchronize()
    for b, n in enumerate(lengths):
        if n:
            assert_close(yc[b:b + 1, :, :n], g["y"][:, :, :n], TOL, f"costgcn_infeat6 step_clip stream {b}")
        assert torch.count_nonzero(yc[b, :, n:]).item() == 0


# ------------------------------------------------------------------------------------------------ 2. edge shapes
def _graph(P, V, imu):
    if V == 25:
        return dict(P.PKU_MMD)
    if V == 7:
        return dict(imu)
    return {"num_node": V, "edge": [[i, i] for i in range(V)] + [[i, i + 1] for i in range(V - 1)], "center": 0}


# (F, V, first width): n = F * V = 2 (the smallest the variance allows); 2-D pose; n = 512, the LDS bound, over the
# narrowest first layer (C0 = 4: the clip kernel's head scratch exceeds its three output rows); n = 35, no multiple of 4
EDGES = [(1, 2, 8), (2, 25, 8), (16, 32, 4), (5, 7, 8)]
EDGE_FRAMES = 24  # kernel 3: FIFOs of 3 and 5 frames


def _edge_confs(P, F, V, C0, imu):
    nl = 2
    conf = {"in_feat": F, "stages": 1, "layers": nl, "kernel": 3, "in_ch": [C0, 8], "out_ch": [8, 16],
            "stride": [1, 2], "residual": [1] * nl, "dropout": [0.0] * nl, "importance": True}
    top = {"strategy": "spatial", "in_feat": F, "stages": 1, "kernel": 3, "output_type": "logits",
           "normalization": "LayerNorm", "num_classes": 5, "graph": _graph(P, V, imu)}
    rt = dict(top, segment=500, **{"rt-st-gcn": dict(conf, latency=False, buffer=1)})
    co = dict(top, **{"st-gcn": dict(conf, dilation=[1] * nl)})
    return rt, co


def _edge_x(F, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, F, EDGE_FRAMES, V, generator=g) * (0.5 + 2 * torch.rand(1, F, 1, 1, generator=g)) + 0.3


@pytest.mark.parametrize("F,V,C0", EDGES)
def test_edge_shapes_rt_stream_batch(P, rt6, F, V, C0):
    arch, _ = _edge_confs(P, F, V, C0, rt6["arch"]["graph"])
    torch.manual_seed(800 + F)
    sd = randomise(P.MODELS["rt-st-gcn"](rank=None, **arch).state_dict(), torch.Generator().manual_seed(801 + F))
    gen = torch.Generator().manual_seed(802 + F)
    for k in sd:  # randomise() names co-st-gcn's norms; the online layers' are bn_relu.0
        if "bn_relu" in k and k.endswith("weight"):
            sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=gen)
    x = _edge_x(F, V, 803 + F)
    ref = oracle_fp64(x, sd, arch)
    m = rt_online(P, arch, sd)
    assert m.fcn_in.in_channels == F and m.fcn_in.out_channels == C0
    sb = m.stream_batch(2)
    y = ticks(sb, x.to(DEV))
    assert_close(y, ref, TOL, f"rt step F={F} V={V}")
    yc = m.stream_batch(2).step_clip(x.to(DEV))
    torch.cuda.synchronize()
    assert_close(yc, ref, TOL, f"rt step_clip F={F} V={V}")


@pytest.mark.parametrize("F,V,C0", EDGES)
def test_edge_shapes_co_forward_clip(P, co6, F, V, C0):
    _, arch = _edge_confs(P, F, V, C0, co6["arch"]["graph"])
    torch.manual_seed(900 + F)
    sd = randomise(P.MODELS["co-st-gcn"](rank=None, **arch).state_dict(), torch.Generator().manual_seed(901 + F))
    x = _edge_x(F, V, 903 + F)[:1]
    with torch.no_grad():
        ref = costgcn_stream(x, sd, arch, sd["A"], dtype=torch.float64)
    m = co_model(P, arch, sd)
    assert_close(clips(m, x.to(DEV), EDGE_FRAMES), ref, TOL, f"co forward_clip F={F} V={V}")
    m.reset_state()
    assert_close(frames(m, x.to(DEV)), ref, TOL, f"co forward F={F} V={V}")


# ------------------------------------------------------------------------------------------------ 3. bitwise relations
T_MASK, RESTART_AT = 24, 11


def _mask_codes():
    """Slot 0 steps, slot 1 steps on even ticks, slot 2 restarts at tick 11, slot 3 never runs, slot 4 steps."""
    codes = [[1, 1 - t % 2, 1, 0, 1] for t in range(T_MASK)]
    codes[RESTART_AT][2] = 2
    return codes


@pytest.mark.parametrize("kind", ["rt", "co"])
def test_stream_does_not_depend_on_batch_slot_or_neighbours(rt6, co6, kind):
    c = rt6 if kind == "rt" else co6
    m, xd = c["m"], c["xd"]
    y = ticks(m.stream_batch(5), xd, _mask_codes())
    assert torch.count_nonzero(y[3]).item() == 0 and torch.count_nonzero(y[1, :, 1::2]).item() == 0
    assert_close(y[0:1], c["ref64"][0:1], TOL, f"{kind} slot 0 of 5")
    for b, sel in ((0, slice(None)), (4, slice(None)), (1, slice(0, None, 2)), (2, slice(RESTART_AT, None))):
        one = m.stream_batch(1)
        assert torch.equal(ticks(one, xd[b:b + 1, :, sel]), y[b:b + 1, :, sel]), f"{kind} slot {b}"


def test_co_step_clip_is_forward_clip(co6):
    m, xd = co6["m"], co6["xd"]
    y = m.stream_batch(5).step_clip(xd)
    torch.cuda.synchronize()
    for b in (0, 3):
        m.reset_state()
        assert torch.equal(clips(m, xd[b:b + 1], T_MASK), y[b:b + 1]), f"stream {b}"
    assert_close(y, co6["ref64"], TOL, "co step_clip B=5")


@pytest.mark.parametrize("kind", ["rt", "co"])
def test_any_chunking_of_a_clip_gives_the_same_bits(rt6, co6, kind):
    c = rt6 if kind == "rt" else co6
    m, xd = c["m"], c["xd"]
    whole = m.stream_batch(5).step_clip(xd)
    assert_close(whole, c["ref64"], TOL, f"{kind} step_clip")
    for cuts in ((1,) * T_MASK, (7, 1, 16), (17, 7)):
        sb, t0, ys = m.stream_batch(5), 0, []
        for n in cuts:
            ys.append(sb.step_clip(xd[:, :, t0:t0 + n]))
            t0 += n
        torch.cuda.synchronize()
        assert t0 == T_MASK and torch.equal(torch.cat(ys, dim=2), whole), f"{kind} cuts {cuts}"
    sb = m.stream_batch(5)  # ticks, then a clip, on one batch
    mixed = torch.cat([ticks(sb, xd[:, :, :5]), sb.step_clip(xd[:, :, 5:])], dim=2)
    torch.cuda.synchronize()
    assert_close(mixed, c["ref64"], TOL, f"{kind} ticks then a clip")


@pytest.mark.parametrize("kind", ["rt", "co"])
def test_snapshot_continues_in_a_batch_of_another_size(rt6, co6, kind):
    c = rt6 if kind == "rt" else co6
    m, xd = c["m"], c["xd"]
    src = m.stream_batch(5)
    head = ticks(src, xd[:, :, :13])
    snap = src.export_state([3])
    dst = m.stream_batch(2)
    dst.import_state(snap, [1])
    tail = ticks(src, xd[:, :, 13:])
    x2 = torch.zeros(2, 6, T_MASK - 13, 7, device=DEV)
    x2[1] = xd[3, :, 13:]
    got = ticks(dst, x2, [[0, 1]] * (T_MASK - 13))
    assert torch.equal(got[1], tail[3])
    assert_close(torch.cat([head[3:4], got[1:2]], dim=2), c["ref64"][3:4], TOL, f"{kind} stream 3 across the snapshot")


# ------------------------------------------------------------------------------------------------ 4. bf16
def test_bf16_rt_stream_batch(rt6):
    """bf16 conv operands at in_feat 6 against the fp64 oracle; bar 2 x the error of the restatement that rounds the
    operands where rt_streams.hip does (tests/test_rt_streams_bf16_cpu.py, generic in in_feat)."""
    x, ref = rt6["x"][:2], rt6["ref64"][:2]
    bar = rel_err(restatement(x, rt6["sd"], rt6["arch"]), ref)
    sb = rt6["m"].stream_batch(2, "bf16")
    err = rel_err(ticks(sb, rt6["xd"][:2]).cpu(), ref)
    print(f"[err] rt streams bf16 in_feat 6: kernel {err:.3e}, restatement {bar:.3e}", flush=True)
    assert 2.0 ** -13 < bar < 2.0 ** -5
    assert err <= 2 * bar, f"bf16 error {err:.3e} > 2 x {bar:.3e}"


def test_bf16_co_stream_batch(P, co6):
    x, ref = co6["x"][:2], co6["ref64"][:2]
    with torch.no_grad():
        emu = torch.cat([costgcn_stream(x[b:b + 1], co6["sd"], co6["arch"], co6["sd"]["A"], round_bf16=True)
                         for b in range(2)])
    bar = rel_err(emu, ref)
    m = co_model(P, co6["arch"], co6["sd"], "bf16")
    batch = m.stream_batch(2)
    assert batch.state[0][0].dtype == torch.bfloat16
    err = rel_err(ticks(batch, co6["xd"][:2]).cpu(), ref)
    print(f"[err] co streams bf16 in_feat 6: kernels {err:.3e}, bf16-rounded restatement {bar:.3e}", flush=True)
    assert 2.0 ** -13 < bar < 2.0 ** -5
    assert err <= 2 * bar, f"bf16 error {err:.3e} > 2 x {bar:.3e}"


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(P, rt6, co6):
    arch = dict(rt6["arch"], in_feat=17)
    arch["rt-st-gcn"] = dict(arch["rt-st-gcn"], in_feat=17)
    m = P.MODELS["rt-st-gcn"](rank=None, **arch).to(DEV).eval()
    m.prepare_benchmark(arch)
    with pytest.raises(RuntimeError, match=r"1 <= in_feat <= 16, got 17"):
        m.stream_batch(2)
    arch = dict(co6["arch"], in_feat=17)
    arch["st-gcn"] = dict(arch["st-gcn"], in_feat=17)
    m = P.MODELS["co-st-gcn"](rank=None, **arch).to(DEV).eval()
    with pytest.raises(RuntimeError, match=r"1 <= in_feat <= 16, got 17"):
        m.stream_batch(2)
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"1 <= in_feat <= 16, got 17"):
        m(torch.zeros(1, 17, 1, 7, device=DEV))
    for c in (rt6, co6):
        sb = c["m"].stream_batch(2)
        with pytest.raises(RuntimeError, match=r"step expects x of shape \(2, 6, 1, 7\), got \(2, 3, 1, 7\)"):
            sb.step(torch.zeros(2, 3, 1, 7, device=DEV))
        with pytest.raises(RuntimeError, match=r"step_clip expects x of shape \(2, 6, T >= 1, 7\)"):
            sb.step_clip(torch.zeros(2, 3, 4, 7, device=DEV))
    with torch.no_grad(), pytest.raises(RuntimeError, match="rt_frame_in"):
        co6["m"](torch.zeros(1, 3, 1, 7, device=DEV))
