"""co-st-gcn clips on the device (Model.forward_clip, stgcn_co_clip): the reference fixtures in one clip and in chunks,
clips of every critical length mixed with per-frame calls on one stream (outputs and ring state), the clip against a
stream batch of one, the reference's widths in fp32 and bf16 and route against route, a T > fifo clip at Kt = 69 and
full width, graph replay, a parameter change mid-stream and the chunk cap.  Bars are test_gpu_costgcn.py's own."""
import os
import sys

import pytest
import torch

from conftest import assert_close

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coclip_ref import costgcn_clip  # noqa: E402
from costgcn_ref import costgcn_stream  # noqa: E402
from test_gpu_costgcn import DEV, TOL, P, build, make_arch, stream, widths  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def clips(m, xd, chunks):
    """The frames of xd through forward_clip in consecutive clips of the given lengths (the last one cut to fit)."""
    ys, t0 = [], 0
    with torch.no_grad():
        while t0 < xd.shape[2]:
            for n in chunks:
                if t0 < xd.shape[2]:
                    ys.append(m.forward_clip(xd[:, :, t0:t0 + n]))
                    t0 += n
    torch.cuda.synchronize()
    return torch.cat(ys, dim=2)


def device_state(m):
    """The rings read out through the head convention (idx = slot of the newest entry, age j in slot idx + j), in
    costgcn_ref's layout: per layer (fifo (1, C, fifo, V), fifo_res (1, C, Kt//2+1, V)) newest first, and idx."""
    out = []
    for l, ring, res_ring, idx in m._plan[1]["state"]:
        i0, i1 = idx.tolist()
        assert 0 <= i0 < ring.shape[0] and 0 <= i1 < res_ring.shape[0]
        f = ring.roll(-i0, 0).float().permute(2, 0, 1).unsqueeze(0).cpu()
        r = res_ring.roll(-i1, 0).permute(2, 0, 1).unsqueeze(0).cpu()
        out.append((f, r, (i0, i1)))
    return out


@pytest.mark.parametrize("name", ["costgcn_k9", "costgcn_k69"])
def test_goldens(P, golden, name):
    g = golden(name)
    arch = dict(g["arch"], graph=P.PKU_MMD)
    m = P.MODELS["co-st-gcn"](rank=None, **arch)
    m.load_state_dict({k[3:]: v for k, v in g.items() if k.startswith("sd/")}, strict=True)
    m = m.to(DEV).eval()
    xd = g["x"].to(DEV)
    y = clips(m, xd, (xd.shape[2],))
    assert_close(y, g["y"], TOL, f"co-st-gcn clip {name}")
    fifo = max(arch["st-gcn"]["stride"]) * (arch["kernel"] - 1) + 1
    for n in (1, 3, fifo + 1):
        m.reset_state()
        assert torch.equal(clips(m, xd, (n,)), y), f"{name}: chunks of {n}"


SMALL_T = [1, 2, 3, 5, 8, 9, 10, 16, 17, 18, 33]


@pytest.fixture(scope="module")
def small(P):
    """8/8/16 widths, strides 1/2/1, Kt = 9 (FIFOs of 9 and 17 frames), 40 frames: the model on the device, the
    frame-by-frame restatement, and the restatement's state after 7 + T frames for every tested T."""
    arch = make_arch(P, 9, [8, 8, 16], [8, 16, 16], [1, 2, 1])
    m, sd = build(P, arch, 51)
    x = torch.randn(1, 3, 40, 25, generator=torch.Generator().manual_seed(53))
    with torch.no_grad():
        ref = costgcn_stream(x, sd, arch, sd["A"])
        states = {T: costgcn_clip(x[:, :, :7 + T], sd, arch, sd["A"])[1] for T in SMALL_T}
    return dict(arch=arch, sd=sd, x=x, xd=x.to(DEV), ref=ref, states=states, m=m.to(DEV).eval())


@pytest.mark.parametrize("T", SMALL_T)
def test_mixed_with_frames(small, T):
    """Frames 0..6 through forward, one clip of T, the rest through forward.  The T cover: less than a tap block's row
    tiles and partial ones, T < fifo, T = fifo - 1, fifo, fifo + 1 of both strides (9 and 17), T > fifo of both (every
    ring slot overwritten), and the residual delay (4 frames) reaching back before the clip."""
    m, xd = small["m"], small["xd"]
    m.reset_state()
    with torch.no_grad():
        a = stream(m, xd[:, :, :7])
        b = m.forward_clip(xd[:, :, 7:7 + T])
        got = device_state(m)
        ys = [a, b] + ([stream(m, xd[:, :, 7 + T:])] if 7 + T < xd.shape[2] else [])
    torch.cuda.synchronize()
    assert tuple(b.shape) == (1, 7, T) and b.dtype == torch.float32
    assert_close(torch.cat(ys, dim=2), small["ref"], TOL, f"co-st-gcn frames + clip of {T} + frames")
    for i, ((f, r, idx), (rf, rr)) in enumerate(zip(got, small["states"][T])):
        nf, nr = rf.shape[2], rr.shape[2]
        assert idx == ((-(7 + T)) % nf, (-(7 + T)) % nr), f"layer {i}: idx {idx}"
        assert_close(f, rf, TOL, f"layer {i} ring after a clip of {T}")
        assert_close(r, rr, TOL, f"layer {i} residual ring after a clip of {T}", scale_floor=1e-3)


def test_chunk_invariance_of_state(small):
    """One clip of 33 frames and the same frames in clips of 1, 2, 17, 13: outputs, rings, residual rings and idx bit
    for bit."""
    m, xd = small["m"], small["xd"][:, :, :33]
    m.reset_state()
    y = clips(m, xd, (33,))
    one = [(ring.clone(), res.clone(), idx.clone()) for _, ring, res, idx in m._plan[1]["state"]]
    m.reset_state()
    assert torch.equal(clips(m, xd, (1, 2, 17, 13)), y)
    for (ring, res, idx), (_, ring2, res2, idx2) in zip(one, m._plan[1]["state"]):
        assert torch.equal(ring, ring2) and torch.equal(res, res2) and torch.equal(idx, idx2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 4, 5, 8, 9, 10])
def test_one_stream_is_a_batch_of_one(small, T, dtype):
    """forward_clip runs the stream batch's kernels with B = 1 and no codes or lengths, so its state launch carries
    fifo + Kt/2+1 blocks per layer of which those beyond min(T, slots) return.  From a stream 3 frames in, clips whose T
    straddles the residual ring (5 slots) and the activation ring of the stride-1 layers (9): the outputs against the
    same frames through forward from the same state (the file's bar), and outputs and state bit for bit against
    stream_batch(1).step_clip from the snapshot of that state."""
    m, xd = small["m"], small["xd"]
    clip = xd[:, :, :T]
    m.set_compute_dtype(dtype)
    try:
        m.reset_state()
        with torch.no_grad():
            stream(m, xd[:, :, -3:])
            snap = m.export_state()
            y = m.forward_clip(clip)
            state = m.export_state().data
            m.import_state(snap)
            frames = stream(m, clip)
            sb = m.stream_batch(1)
            sb.import_state(snap)
            yb = sb.step_clip(clip)
            state_b = sb.export_state().data
        torch.cuda.synchronize()
    finally:
        m.set_compute_dtype("fp32")
    assert_close(y, frames, TOL, f"co-st-gcn {dtype} clip of {T} vs per-frame, 3 frames in")
    assert torch.equal(y, yb), f"{dtype} clip of {T}: forward_clip vs stream_batch(1).step_clip outputs"
    assert torch.equal(state, state_b), f"{dtype} clip of {T}: forward_clip vs stream_batch(1).step_clip state"


def _rel(y, ref):
    return (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()


def test_widths_fp32(P, widths):
    m = P.MODELS["co-st-gcn"](rank=None, **widths["arch"])
    m.load_state_dict(widths["sd"], strict=True)
    m = m.to(DEV).eval()
    xd = widths["x"].to(DEV)
    y = clips(m, xd, (xd.shape[2],))
    assert_close(y, widths["ref32"], TOL, "co-st-gcn clip widths fp32")
    m.reset_state()
    yf = stream(m, xd)
    ref = widths["ref64"]
    e_clip, e_frame, e_ref32 = _rel(y, ref), _rel(yf, ref), _rel(widths["ref32"], ref)
    if os.environ.get("STGCN_TEST_REPORT"):
        print(f"[err] co-st-gcn widths vs fp64: clip {e_clip:.3e}, per-frame {e_frame:.3e}, fp32 restatement "
              f"{e_ref32:.3e} (bar {2 * max(e_frame, e_ref32):.3e})", flush=True)
    assert e_clip <= 2 * max(e_frame, e_ref32), f"clip {e_clip:.3e} > 2 x max({e_frame:.3e}, {e_ref32:.3e})"


def test_widths_bf16(P, widths):
    """test_bf16's bar: 2x the error of the bf16-rounded restatement against the fp64 one."""
    m = P.MODELS["co-st-gcn"](rank=None, **widths["arch"])
    m.load_state_dict(widths["sd"], strict=True)
    m = m.to(DEV).eval().set_compute_dtype("bf16")
    xd = widths["x"].to(DEV)
    y = clips(m, xd, (xd.shape[2],))
    ref = widths["ref64"]
    bar, err = _rel(widths["emu"], ref), _rel(y, ref)
    if os.environ.get("STGCN_TEST_REPORT"):
        print(f"[err] co-st-gcn clip bf16: kernels {err:.3e}, bf16-rounded restatement {bar:.3e} (bar {2 * bar:.3e})",
              flush=True)
    assert err <= 2 * bar, f"bf16 clip error {err:.3e} > 2 x {bar:.3e}"
    m.reset_state()
    assert torch.equal(clips(m, xd, (1, 7, 5)), y)  # chunk invariance with the bf16 ring


def test_full_depth_clip(P):
    """One 256 -> 256 layer at Kt = 69 (K = 17 664), 75 frames in one clip (T > fifo = 69): against the restatement, and
    against the per-frame route at the bar test_split_k_full_depth sets between two split orders of this layer."""
    arch = make_arch(P, 69, [256], [256], [1])
    m, sd = build(P, arch, 41)
    x = torch.randn(1, 3, 75, 25, generator=torch.Generator().manual_seed(43))
    with torch.no_grad():
        ref = costgcn_stream(x, sd, arch, sd["A"])
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    y = clips(m, xd, (75,))
    assert_close(y, ref, TOL, "co-st-gcn clip 256x69")
    m.reset_state()
    assert_close(y, stream(m, xd), 1e-5, "co-st-gcn clip 256x69 vs per-frame")


def test_graph_replay(small):
    m, xd = small["m"], small["xd"][:, :, :24]
    m.reset_state()
    y = clips(m, xd, (24,))
    x_static = torch.zeros_like(xd[:, :, :8])
    with torch.no_grad():
        x_static.copy_(xd[:, :, :8])
        m.forward_clip(x_static)  # the clip's buffers exist before the capture
        m.reset_state()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph):
                y_static = m.forward_clip(x_static)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            m.reset_state()
            outs = []
            for i in range(3):
                x_static.copy_(xd[:, :, 8 * i:8 * i + 8])
                graph.replay()
                outs.append(y_static.clone())
            torch.cuda.synchronize()
            assert torch.equal(torch.cat(outs, dim=2), y)


def test_stale_state_through_clips(P):
    """test_stale_state through forward_clip: tcn.0.bias of layer 0 changed mid-stream restarts the stream with rings
    that start from the new ReLU(tcn.0.bias)."""
    arch = make_arch(P, 9, [8, 8, 16], [8, 16, 16], [1, 2, 1])
    m, sd = build(P, arch, 51)
    x = torch.randn(1, 3, 20, 25, generator=torch.Generator().manual_seed(53))
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    clips(m, xd[:, :, :7], (7,))
    sd2 = dict(sd)
    sd2["gcn_networks.0.tcn.0.bias"] = sd["gcn_networks.0.tcn.0.bias"] + 0.5
    m.load_state_dict(sd2, strict=True)
    m.reset_state()
    with torch.no_grad():
        ref = costgcn_stream(x, sd2, arch, sd2["A"])
        old = costgcn_stream(x, sd, arch, sd["A"])
    assert (ref - old).abs().max().item() > 10 * TOL * ref.abs().max().item()  # the change is visible
    assert_close(clips(m, xd, (20,)), ref, TOL, "co-st-gcn clip after load_state_dict + reset_state")


def test_chunk_cap(small):
    m, xd = small["m"], small["xd"][:, :, :19]
    m.reset_state()
    y = clips(m, xd, (19,))
    m.reset_state()
    m.clip_chunk = 4
    try:
        assert torch.equal(clips(m, xd, (19,)), y)
    finally:
        m.clip_chunk = 256
