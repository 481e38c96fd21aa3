"""co-st-gcn stream-batch clips on the device (CoStreamBatch.step_clip, co_streams_clip.hip): the reference fixtures
with the streams out of step, every critical length mixed with per-frame ticks (outputs and ring state), restarts over
garbage state, a stream's independence of B, slot, neighbours and chunking bit for bit (and its bit-equality with
Model.forward_clip), the scratch bound, the reference's widths in fp32 and bf16, full depth, graph replay with
device-side codes and lengths, 17 joints and a parameter change mid-stream.  Bars are test_gpu_costgcn.py's own."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_co_streams as CS  # noqa: E402  (case, dirty, WIDE, run)
from coclip_ref import costgcn_clip  # noqa: E402
from costgcn_ref import costgcn_stream  # noqa: E402
from test_gpu_co_clip import small  # noqa: E402,F401
from test_gpu_costgcn import DEV, TOL, P, build, make_arch  # noqa: E402,F401

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("STGCN_TEST_REPORT")


def i32(v):
    return torch.as_tensor(v, dtype=torch.int32, device=DEV)


def stream_state(batch, b):
    """Stream b's rings read out through the head convention, as test_gpu_co_clip.device_state does for a model."""
    out = []
    for ring, res_ring, idx in batch.state:
        i0, i1 = idx[b].tolist()
        assert 0 <= i0 < ring.shape[1] and 0 <= i1 < res_ring.shape[1]
        f = ring[b].roll(-i0, 0).float().permute(2, 0, 1).unsqueeze(0).cpu()
        r = res_ring[b].roll(-i1, 0).permute(2, 0, 1).unsqueeze(0).cpu()
        out.append((f, r, (i0, i1)))
    return out


def raw_state(batch, b=None):
    sel = slice(None) if b is None else b
    return [tuple(t[sel].clone() for t in ts) for ts in batch.state]


def same_state(a, b):
    return all(torch.equal(t, u) for ts, us in zip(a, b) for t, u in zip(ts, us))


# ------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("name", ["costgcn_k9", "costgcn_k69"])
def test_goldens_out_of_step(P, golden, name):
    """B = 3 over garbage state, every stream restarted in the first call and fed the fixture from frame 0 in calls of
    7 frames; stream 1 takes one frame fewer in the first call and stream 2 is skipped in the second, so the streams
    sit at different frames of the fixture from then on."""
    g = golden(name)
    arch = dict(g["arch"], graph=P.PKU_MMD)
    m = P.MODELS["co-st-gcn"](rank=None, **arch)
    m.load_state_dict({k[3:]: v for k, v in g.items() if k.startswith("sd/")}, strict=True)
    m = m.to(DEV).eval()
    B, T, gx = 3, 7, g["x"][0]
    F = gx.shape[1]
    batch = m.stream_batch(B)
    CS.dirty(batch)
    at, cols, j = [0] * B, [[] for _ in range(B)], 0
    while min(at) < F:
        x = torch.zeros(B, 3, T, 25)
        codes, lengths = [2 if j == 0 else 1] * B, [0] * B
        for b in range(B):
            n = min(T, F - at[b]) - (1 if (j, b) == (0, 1) else 0)
            if (j, b) == (1, 2):
                codes[b], n = 0, T   # skipped: the length is not looked at
            else:
                x[b, :, :n] = gx[:, at[b]:at[b] + n]
            lengths[b] = n
        y = batch.step_clip(x.to(DEV), i32(codes), i32(lengths)).cpu()
        assert tuple(y.shape) == (B, 7, T) and y.dtype == torch.float32
        for b in range(B):
            n = 0 if codes[b] == 0 else lengths[b]
            assert not y[b, :, n:].any()   # exactly zero beyond the length and for the skipped stream
            cols[b].append(y[b, :, :n])
            at[b] += n
        j += 1
    for b in range(B):
        assert_close(torch.cat(cols[b], dim=1)[None], g["y"], TOL, f"co streams clip {name} stream {b}")


# ------------------------------------------------------------------------------------------------ 2. lengths and tiles
@pytest.mark.parametrize("lengths", [(0, 1, 5, 6, 33), (8, 9, 10, 17, 18)])
def test_lengths_and_tiles(small, lengths):
    """Frames 0..6 through step, one step_clip of T = 33 with a length per stream, the rest through step.  (0, 1, 5, 6,
    33): nothing, one frame, 125 rows = one tap block, 150 rows = a partial second block, all of it; (8, 9, 10, 17, 18):
    fifo - 1, fifo, fifo + 1 of both strides."""
    m, x, B = small["m"], small["x"], 5
    xd = small["xd"].expand(B, -1, -1, -1).contiguous()
    batch = m.stream_batch(B)
    a = CS.run(batch, xd[:, :, :7], None)
    y = batch.step_clip(xd[:, :, 7:40], None, list(lengths))
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B, 7, 33)
    got = [stream_state(batch, b) for b in range(B)]
    # the rest, tick by tick: stream b goes on at frame 7 + n_b and stops at frame 40
    rest = [[] for _ in range(B)]
    for k in range(33 - min(lengths)):
        at = [7 + n + k for n in lengths]
        xt = torch.stack([x[0, :, min(t, 39):min(t, 39) + 1] for t in at]).to(DEV)
        yt = batch.step(xt, [t < 40 for t in at])
        for b in range(B):
            if at[b] < 40:
                rest[b].append(yt[b])
    torch.cuda.synchronize()
    for b, n in enumerate(lengths):
        assert not y[b, :, n:].any()
        full = torch.cat([a[b], y[b, :, :n]] + rest[b], dim=1)[None]
        assert_close(full, small["ref"], TOL, f"co streams clip: frames + clip of {n} + frames")
        with torch.no_grad():
            want = costgcn_clip(x[:, :, :7 + n], small["sd"], small["arch"], small["sd"]["A"])[1]
        for i, ((f, r, idx), (rf, rr)) in enumerate(zip(got[b], want)):
            nf, nr = rf.shape[2], rr.shape[2]
            assert idx == ((-(7 + n)) % nf, (-(7 + n)) % nr), f"stream {b} layer {i}: idx {idx}"
            assert_close(f, rf, TOL, f"stream {b} layer {i} ring after a clip of {n}")
            assert_close(r, rr, TOL, f"stream {b} layer {i} residual ring after a clip of {n}", scale_floor=1e-3)


# ------------------------------------------------------------------------------------------------ 3. restart
@pytest.mark.parametrize("n", [0, 3, 9, 20])
def test_restart(small, n):
    """Code 2 over garbage state equals reset([b]) then code 1, bit for bit in outputs and state, whatever n is (n <
    fifo leaves ring slots the clip does not write); the code-1 neighbour goes on from its state, the code-0
    neighbour's state is untouched."""
    m, B = small["m"], 3
    xd = small["xd"][:, :, :25].expand(B, -1, -1, -1).contiguous()
    lengths = i32([n, 20, 20])
    got = []
    for restart_code in (True, False):
        batch = m.stream_batch(B)
        batch.step_clip(xd[:, :, :5])
        keep = raw_state(batch)
        if restart_code:
            CS.dirty(batch)
            for ts, ks in zip(batch.state, keep):
                for t, k in zip(ts, ks):
                    t[1:] = k[1:]   # only stream 0 holds garbage
            y = batch.step_clip(xd[:, :, 5:25], i32([2, 1, 0]), lengths)
        else:
            batch.reset([0])
            y = batch.step_clip(xd[:, :, 5:25], i32([1, 1, 0]), lengths)
        torch.cuda.synchronize()
        assert same_state(raw_state(batch, 2), [tuple(t[2] for t in ks) for ks in keep])
        assert not y[2].any() and not y[0, :, n:].any()
        got.append((y.clone(), raw_state(batch)))
    assert torch.equal(got[0][0], got[1][0])
    assert same_state(got[0][1], got[1][1])
    if n == 0:   # code 2 without a frame left exactly the reset state
        batch.reset([1])
        assert same_state([tuple(t[0] for t in ts) for ts in got[0][1]], raw_state(batch, 1))


# ------------------------------------------------------------------------------------------------ 4. independence
def test_independence_and_chunking(small):
    """One stream's 33 frames (restarted over garbage, 30 of them consumed, one call in which it is skipped) in slot 0
    of B = 1, slot 4 of B = 5 and slot 40 of B = 41, as one call of T = 33 and as calls of 1, 2, 17 and 13: the six
    outputs and final states are bit-identical, and bit-identical to Model.forward_clip on the 30 frames."""
    m, T, n_mine = small["m"], 33, 30
    xm = small["x"][0, :, :T]
    results = []
    for B, slot in ((1, 0), (5, 4), (41, 40)):
        for chunks in ((T,), (1, 2, 17, 13)):
            gen = torch.Generator().manual_seed(1000 * B + len(chunks))
            batch = m.stream_batch(B)
            CS.dirty(batch)
            cols, t0 = [], 0
            for j, n in enumerate(chunks):
                x = torch.randn(B, 3, n, 25, generator=gen)
                codes = torch.randint(0, 3, (B,), generator=gen, dtype=torch.int32)
                lengths = torch.randint(-1, n + 2, (B,), generator=gen, dtype=torch.int32)
                x[slot], codes[slot], lengths[slot] = xm[:, t0:t0 + n], 2 if j == 0 else 1, n_mine - t0
                cols.append(batch.step_clip(x.to(DEV), codes.to(DEV), lengths.to(DEV))[slot].clone())
                t0 += n
                if j == 0:   # a call in which the stream is skipped, the others are not
                    x = torch.randn(B, 3, 4, 25, generator=gen)
                    codes = torch.ones(B, dtype=torch.int32)
                    codes[slot] = 0
                    assert not batch.step_clip(x.to(DEV), codes.to(DEV))[slot].any()
            torch.cuda.synchronize()
            results.append((torch.cat(cols, dim=1), raw_state(batch, slot)))
    y, state = results[0]
    assert not y[:, n_mine:].any() and y[:, :n_mine].abs().sum() > 0
    for k, (yk, sk) in enumerate(results[1:], 1):
        assert torch.equal(yk, y), f"outputs of variant {k}"
        assert same_state(sk, state), f"state of variant {k}"
    # contract 6: the single-stream clip from an empty stream gives the same bits
    m.reset_state()
    with torch.no_grad():
        yc = m.forward_clip(small["xd"][:, :, :n_mine])
    torch.cuda.synchronize()
    assert torch.equal(yc[0], y[:, :n_mine])
    assert same_state([(ring, res, idx) for _, ring, res, idx in m._plan[1]["state"]], state)
    # against step tick by tick: within the bar; whether it is bit-equal is reported, not asserted
    batch = m.stream_batch(1)
    ys = CS.run(batch, small["xd"][:, :, :n_mine], None)
    assert_close(ys[0], y[:, :n_mine], TOL, "co streams clip vs step tick by tick")
    if REPORT:
        print(f"[report] step_clip vs step tick by tick: outputs bit-equal {torch.equal(ys[0], y[:, :n_mine])}, max "
              f"abs diff {(ys[0] - y[:, :n_mine]).abs().max().item():.3e}; state bit-equal "
              f"{same_state(raw_state(batch, 0), state)}", flush=True)


# ------------------------------------------------------------------------------------------------ 5. clip_frames
def test_clip_frames(small):
    m, B = small["m"], 5
    xd = torch.randn(B, 3, 19, 25, generator=torch.Generator().manual_seed(5)).to(DEV)
    lengths = i32([19, 0, 7, 18, 12])
    base = m.stream_batch(B)
    assert base.clip_frames == 1024 and base._clip_chunk() == 128
    before = base.scratch_bytes
    y = base.step_clip(xd, None, lengths)
    assert base.scratch_bytes > before   # the clip scratch is counted
    tight = m.stream_batch(B)
    tight.clip_frames = 8
    assert tight._clip_chunk() == 1
    y1 = tight.step_clip(xd, None, lengths)
    torch.cuda.synchronize()
    assert torch.equal(y1, y) and same_state(raw_state(tight), raw_state(base))
    assert tight.scratch_bytes < base.scratch_bytes


# ------------------------------------------------------------------------------------------------ 6. widths
@pytest.fixture(scope="module")
def wide(P):
    return CS.case(P, 9, CS.WIDE, 20, 2, 71)


def _rel(y, ref):
    return (y.double().cpu() - ref.double()).abs().max().item() / ref.abs().max().item()


def test_wide_fp32(wide):
    """64 -> 128 at stride 2, Kt = 9, T = 20 (fifo 17): four column tiles, several k-steps per wave."""
    y = wide["m"].stream_batch(2).step_clip(wide["x"].to(DEV))
    torch.cuda.synchronize()
    assert_close(y, wide["ref32"], TOL, "co streams clip 64->128 vs fp32")
    assert_close(y, wide["ref64"], TOL, "co streams clip 64->128 vs fp64")


def test_wide_bf16(P, wide):
    """The project's bf16 rule: the error against fp64 is at most twice that of the bf16-rounded restatement."""
    m = P.MODELS["co-st-gcn"](rank=None, **wide["arch"])
    m.load_state_dict(wide["sd"], strict=True)
    m = m.to(DEV).eval().set_compute_dtype("bf16")
    batch = m.stream_batch(2)
    assert batch.state[0][0].dtype == torch.bfloat16
    xd = wide["x"].to(DEV)
    y = batch.step_clip(xd)
    torch.cuda.synchronize()
    bar, err = _rel(wide["emu"], wide["ref64"]), _rel(y, wide["ref64"])
    if REPORT:
        print(f"[err] co streams clip bf16: kernels {err:.3e}, bf16-rounded restatement {bar:.3e} (bar {2 * bar:.3e})",
              flush=True)
    assert err <= 2 * bar, f"bf16 clip error {err:.3e} > 2 x {bar:.3e}"
    batch.reset()
    chunks = torch.cat([batch.step_clip(xd[:, :, a:b].contiguous()) for a, b in ((0, 1), (1, 8), (8, 20))], dim=2)
    assert torch.equal(chunks, y)   # chunk invariance with the bf16 ring


def test_full_depth(P):
    """One 256 -> 256 layer at Kt = 69 (K = 17 664), B = 2, 75 frames in one call (T > fifo = 69), lengths (75, 70):
    against the restatement at TOL, and against Model.forward_clip at test_full_depth_clip's route-against-route bar."""
    arch = make_arch(P, 69, [256], [256], [1])
    m, sd = build(P, arch, 41)
    x = torch.randn(2, 3, 75, 25, generator=torch.Generator().manual_seed(43))
    lengths = (75, 70)
    with torch.no_grad():
        refs = [costgcn_stream(x[b:b + 1, :, :n], sd, arch, sd["A"]) for b, n in enumerate(lengths)]
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    y = m.stream_batch(2).step_clip(xd, None, list(lengths))
    torch.cuda.synchronize()
    for b, n in enumerate(lengths):
        assert_close(y[b:b + 1, :, :n], refs[b], TOL, f"co streams clip 256x69 stream {b}")
        assert not y[b, :, n:].any()
        m.reset_state()
        with torch.no_grad():
            yc = m.forward_clip(xd[b:b + 1, :, :n])
        assert_close(y[b:b + 1, :, :n], yc, 1e-5, f"co streams clip 256x69 stream {b} vs forward_clip")


# ------------------------------------------------------------------------------------------------ 7. graph replay
def test_graph_replay(small):
    """One captured step_clip (B = 5, T = 8) replayed over six calls whose codes and lengths change on the device
    equals eager, outputs and state."""
    m, B, T, calls = small["m"], 5, 8, 6
    gen = torch.Generator().manual_seed(7)
    xs = torch.randn(calls, B, 3, T, 25, generator=gen).to(DEV)
    codes = torch.randint(0, 3, (calls, B), generator=gen, dtype=torch.int32)
    lengths = torch.randint(0, T + 1, (calls, B), generator=gen, dtype=torch.int32)
    codes[0] = 2
    lengths[1, 0], lengths[2, 1] = T, 0
    eager = m.stream_batch(B)
    want = [eager.step_clip(xs[j], codes[j].to(DEV), lengths[j].to(DEV)).clone() for j in range(calls)]
    batch = m.stream_batch(B)
    x_static = torch.zeros(B, 3, T, 25, device=DEV)
    a_static = torch.ones(B, dtype=torch.int32, device=DEV)
    n_static = torch.zeros(B, dtype=torch.int32, device=DEV)
    batch.step_clip(x_static, a_static, n_static)   # the clip's buffers exist before the capture
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph):
            y_static = batch.step_clip(x_static, a_static, n_static)
    torch.cuda.current_stream().wait_stream(s)
    batch.reset()
    for j in range(calls):
        x_static.copy_(xs[j])
        a_static.copy_(codes[j])
        n_static.copy_(lengths[j])
        graph.replay()
        assert torch.equal(y_static, want[j]), f"call {j}"
    torch.cuda.synchronize()
    assert same_state(raw_state(batch), raw_state(eager))


# ------------------------------------------------------------------------------------------------ 8. 17 joints
def test_coco_17_joints(P):
    g = np.load(f"{ROOT}/tests/golden/graphs.npz")
    V, center = (int(v) for v in g["meta/coco"])
    graph = {"num_node": V, "edge": g["edge/coco"].tolist(), "center": center}
    c = CS.case(P, 3, dict(in_ch=[8, 8], out_ch=[8, 16], stride=[1, 2]), 8, 2, 91, V=V, graph=graph)
    y = c["m"].stream_batch(2).step_clip(c["x"].to(DEV), None, [8, 5])
    torch.cuda.synchronize()
    assert_close(y[0:1], c["ref32"][0:1], TOL, "co streams clip coco stream 0")
    assert_close(y[1:2, :, :5], c["ref32"][1:2, :, :5], TOL, "co streams clip coco stream 1")
    assert not y[1, :, 5:].any()


# ------------------------------------------------------------------------------------------------ 9. stale state
def test_stale_state(P):
    """tcn.0.bias of layer 0 updated in place between two step_clip calls: the batch rebuilds and restarts, so the next
    clip is a fresh stream under the new parameters (test_gpu_co_streams.test_stale_state's pattern)."""
    arch = CS.make_arch(P.PKU_MMD, 3, **CS.SMALL)
    m, sd = CS.build(P, arch, 81)
    x = torch.randn(2, 3, 12, 25, generator=torch.Generator().manual_seed(83))
    batch = m.stream_batch(2)
    xd = x.to(DEV)
    batch.step_clip(xd[:, :, :5].contiguous())
    rings = [ts[0].data_ptr() for ts in batch.state]
    with torch.no_grad():
        m.gcn_networks[0].tcn[0].bias.add_(0.5)
    sd2 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    y = batch.step_clip(xd)
    torch.cuda.synchronize()
    assert rings == [ts[0].data_ptr() for ts in batch.state]   # the state buffers survive the rebuild
    with torch.no_grad():
        ref = torch.cat([costgcn_stream(x[b:b + 1], sd2, arch, sd2["A"]) for b in range(2)])
        old = torch.cat([costgcn_stream(x[b:b + 1], sd, arch, sd["A"]) for b in range(2)])
    assert (ref - old).abs().max().item() > 10 * TOL * ref.abs().max().item()  # the change is visible
    assert_close(y, ref, TOL, "co streams clip after an in-place parameter update")
