"""SURVEY §8(d) configs 3 and 5 on one MI355X (synthetic data, random-init weights).

config 3: RT-ST-GCN online inference (config/pku-mmd/ln/rtstgcn_local.json: LN, K=9, 9 layers),
          one (1, 3, 1, 25) frame at a time through OnlineLayer FIFOs; per-frame latency p50/p99
          eager (one Python-launched kernel sequence per frame) and as a replayed HIP graph (the
          per-frame step captured once; FIFO state and indices are device buffers, so replays
          advance the stream correctly).  Parity of the two against each other is checked.
config 5: AAGCN (config/pku-mmd/as_is/aagcn_local.json: 2 streams, BN, 9 layers) fwd+bwd, bf16,
          N=64 T=300 V=25: skeleton-frames/s.
f1:       window staging (config/pku-mmd/ln/stgcn_local.json: receptive_field 50, segment 1000): norm_in +
          fcn_in of one segment's 1000 windows from the padded capture (window.hip) vs the reference's
          order (unfold the windows, then norm_in and fcn_in on the copies — our HIP kernels on both sides),
          fwd and bwd, BatchNorm and LayerNorm, bf16.

co:       CoST-GCN continual inference (config/pku-mmd/ln/costgcn_local.json widths and strides, LN) at Kt = 9
          and Kt = 69, fp32 and bf16: per-frame p50 / p90 over graph-replayed frames after the FIFOs have filled,
          the tap-weight bytes one frame reads and the HBM-peak fraction they imply, and the plain-PyTorch
          restatement (tests/costgcn_ref.py) timed on the host.  Only with --only co.

ms:       MS-TCN refinement stage (F = 64, 10 layers, 52 classes, L = 2000; ms_stage.hip) forward and backward, fp32
          and bf16, with per-layer kernel times against the bytes a layer moves, and one ms-gcn training step
          (config/pku-mmd/as_is/msgcn_vsc.json: BatchNorm ST-GCN generator over 2000 windows of 50 frames + 3
          refinement stages; LossMultiStage, backward, Adam).  The plain-PyTorch restatement of the stage
          (tests/mstcn_ref.py) is timed on the host beside it.  Only with --only ms.

co_streams: co-st-gcn as a stream batch (Model.stream_batch, stgcn_co_streams) at Kt in {9, 69} x {fp32, bf16} x
          B in {1, 8, 64, 256}: one tick captured as a HIP graph, HIP-event device time over 200 replays after the
          rings filled, beside the single-stream route graph-replayed in the same run.  Only with --only co_streams.
co_clip:  co-st-gcn clip inference (Model.forward_clip, stgcn_co_clip) at Kt in {9, 69} x {fp32, bf16} x T in {1, 4,
          16, 64, 256}: device ms per captured clip and per frame, rings filled, beside the per-frame route
          graph-replayed in the same run in alternating windows; rows appended to profiles/co_clip.jsonl.  Only with
          --only co_clip.
co_streams_clip: co-st-gcn stream-batch clips (CoStreamBatch.step_clip, stgcn_co_streams_clip) at Kt in {9, 69} x
          {fp32, bf16} x B in {1, 8, 64} x T in {4, 16, 64}: device ms of one captured step_clip, rings filled, beside
          B replays of a captured forward_clip of T frames and T replays of a captured step of B streams in the same run
          in alternating windows; rows appended to profiles/co_streams_clip.jsonl.  Only with --only co_streams_clip.
rt_streams_clip: config 3 as stream-batch clips (RtStreamBatch.step_clip, stgcn_rt_streams_clip): B in {1, 8, 64, 256}
          x T in {4, 16, 64}, fp32 and bf16, one captured step_clip beside T replays of a captured step of the same
          batch, in alternating windows; rows appended to profiles/rt_streams_clip.jsonl.  Only with
          --only rt_streams_clip.
stream_state: snapshots of live co-st-gcn streams (CoStreamBatch.export_state / import_state, stgcn_stream_state_*) at
          Kt in {9, 69} x {fp32, bf16}, B = 64, all 64 streams: HIP-event device ms of the captured export and import,
          beside a captured torch.clone of the snapshot's bytes (the machine's copy rate at this size) and the
          torch-level composition (per stream and layer roll + copy_, the heads read back to the host) in the same run; rows
          appended to profiles/stream_state.jsonl.  Only with --only stream_state.
infeat:   the input head at a runtime in_feat.  (a) No regression at in_feat 3: the rt-st-gcn and the co-st-gcn (Kt 9)
          stream-batch tick at config 3's widths, V 25, B in {1, 64, 256}, fp32 and bf16, graph-replayed HIP-event
          time.  (b) The reference's freezing-of-gait model (in_feat 6, the 7-node IMU graph, config 3's nine
          layers): stream-batch ticks at B in {1, 64, 256, 1024}, and one stream per frame through Model.forward.
          --tree DIR runs the same measurement on another checkout of the project (its package and its library, in
          this process alone): the baseline is a checkout of the parent commit, run alternately with this one;
          what that checkout refuses is recorded as refused.  Rows appended to profiles/infeat.jsonl.  Only with
          --only infeat.
streams:  config 3 as a stream batch (Model.stream_batch, stgcn_rt_streams): B in {1, 8, 64, 256, 1024} streams
          advanced one frame per launch, HIP-event device time over 200 graph-replayed ticks after the FIFOs have
          filled, beside the single-stream one-launch route (stgcn_rt_frame) graph-replayed in the same run: ms per
          tick, frames/s, and the ratio against B sequential single-stream replays.  Both operand types (fp32,
          bf16) are measured in the same process, interleaved per B, --stream-repeats times over; the rows are also
          appended to profiles/rt_streams.jsonl.  Only with --only streams.

    python tools/bench_configs.py [--frames 2000] [--steps 10] [--only 3|5|ln|f1|co|ms|infeat|streams|co_streams|co_clip|co_streams_clip|rt_streams_clip|stream_state]
Prints one JSON line per config.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LAYERS = {"layers": 9, "kernel": 9, "in_ch": [64, 64, 64, 64, 128, 128, 128, 256, 256],
          "out_ch": [64, 64, 64, 128, 128, 128, 256, 256, 256], "stride": [1, 1, 1, 2, 1, 1, 2, 1, 1],
          "residual": [1] * 9, "dropout": [0.0] * 9}
RT_ARCH = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": 9, "output_type": "logits",
           "normalization": "LayerNorm", "segment": 500, "num_classes": 52,
           "rt-st-gcn": dict(LAYERS, latency=False, importance=True, in_feat=3, buffer=1, stages=1)}
AAGCN_ARCH = {"strategy": "spatial", "receptive_field": 50, "in_feat": 3, "stages": 1, "output_type": "softmax",
              "normalization": "BatchNorm", "num_classes": 52,
              "aa-gcn": dict(LAYERS, latency=False, importance=True, in_feat=3, stages=1)}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def config3(P, dev, frames):
    torch.manual_seed(0)
    m = P.MODELS["rt-st-gcn"](rank=None, **dict(RT_ARCH, graph=P.PKU_MMD)).to(dev)
    m.eval()
    m.prepare_benchmark(RT_ARCH)
    gen = torch.Generator(device=dev).manual_seed(3)
    stream = torch.randn(frames + 64, 1, 3, 1, 25, device=dev, generator=gen)
    R = P.routing.ROUTING
    prev = R.rt_one_launch
    try:
        R.rt_one_launch = False
        per_layer = _config3_route(m, stream, frames)
        R.rt_one_launch = True
        out = _config3_route(m, stream, frames)
    finally:
        R.rt_one_launch = prev
    out["per_layer_route"] = per_layer
    # workgroup count of the one-launch kernel: device time of 200 graph replays per count
    sweep = {}
    with torch.no_grad():
        for G in (16, 32, 64, 128, 256):
            m.reset_state()
            x_static = stream[0].clone()
            m(x_static)
            m._frame_pack[1][0].blocks = G
            g = torch.cuda.CUDAGraph()
            s_ = torch.cuda.Stream()
            s_.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s_):
                with torch.cuda.graph(g):
                    m(x_static)
            torch.cuda.current_stream().wait_stream(s_)
            for _ in range(20):
                g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            sweep[G] = round(e0.elapsed_time(e1) / 200, 4)
            assert int(m._frame_status.item()) == 0
        m._frame_pack[1][0].blocks = 0
    out["one_launch_blocks_device_ms"] = sweep
    return {"config": "3: rt-st-gcn online (ln/rtstgcn_local.json, LN, K=9, 9 layers), 1 frame (1,3,1,25)",
            "metric": "per-frame latency", "unit": "ms", "frames": frames, "dtype": "fp32",
            "route": "one persistent launch per frame (stgcn_rt_frame); per_layer_route: 2 launches per layer",
            "reference_cpu": "2.7 ms/frame (SURVEY §8(a12), 9 layers)", **out}


def _config3_route(m, stream, frames):
    out = {}
    with torch.no_grad():
        # eager: every kernel launched from Python per frame
        m.reset_state()
        lat, ys = [], []
        for i in range(frames):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = m(stream[i])
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
            if i < 64:
                ys.append(y.clone())
        warm = lat[32:]
        out["eager"] = {"p50_ms": round(1e3 * pct(warm, 0.5), 4), "p99_ms": round(1e3 * pct(warm, 0.99), 4)}
        # HIP graph: capture one per-frame step on a static input buffer, replay per frame
        m.reset_state()
        x_static = torch.zeros_like(stream[0])
        for i in range(3):  # warm-up launches (attribute setup, allocator) on the real stream
            x_static.copy_(stream[i])
            m(x_static)
        m.reset_state()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g):
                y_static = m(x_static)
        torch.cuda.current_stream().wait_stream(s)
        m.reset_state()  # the capture itself does not run the step
        lat, err = [], 0.0
        for i in range(frames):
            x_static.copy_(stream[i])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.replay()
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
            if i < 64:
                err = max(err, float((y_static - ys[i]).abs().max() / ys[i].abs().max().clamp_min(1e-12)))
        warm = lat[32:]
        out["graph"] = {"p50_ms": round(1e3 * pct(warm, 0.5), 4), "p99_ms": round(1e3 * pct(warm, 0.99), 4),
                        "max_rel_diff_vs_eager": err}
        # device time of one frame: HIP events around 200 back-to-back replays
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(200):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        out["graph"]["device_ms_per_frame"] = round(e0.elapsed_time(e1) / 200, 4)
    return out


def _replay_ms(step, fill, reps=200):
    """Device ms per replay of ``step`` captured as a HIP graph: ``fill`` replays first (the FIFOs fill), then HIP
    events around ``reps`` back-to-back replays."""
    step()  # descriptor, weight packs and launch attributes outside the capture
    g = torch.cuda.CUDAGraph()
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        with torch.cuda.graph(g):
            step()
    torch.cuda.current_stream().wait_stream(s_)
    for _ in range(fill):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def streams(P, dev, batches=(1, 8, 64, 256, 1024), repeats=1):
    torch.manual_seed(0)
    m = P.MODELS["rt-st-gcn"](rank=None, **dict(RT_ARCH, graph=P.PKU_MMD)).to(dev)
    m.eval()
    m.prepare_benchmark(RT_ARCH)
    gen = torch.Generator(device=dev).manual_seed(3)
    fill = 32  # > the 17-frame FIFO of the stride-2 layers
    R = P.routing.ROUTING
    prev = R.rt_one_launch
    rows = []
    with torch.no_grad():
        try:
            R.rt_one_launch = True
            x1 = torch.randn(1, 3, 1, 25, device=dev, generator=gen)
            single = _replay_ms(lambda: m(x1), fill)
        finally:
            R.rt_one_launch = prev
        for r in range(repeats):
            for B in batches:
                x = torch.randn(B, 3, 1, 25, device=dev, generator=gen)
                for dtype in ("fp32", "bf16"):  # interleaved: the two operand types see the same device state
                    sb = None  # the previous batch's state is freed before the next one is allocated
                    sb = m.stream_batch(B, dtype)
                    ms = _replay_ms(lambda: sb.step(x), fill)
                    rows.append({"config": "3 as a stream batch (stgcn_rt_streams): B streams, one frame each per "
                                           "launch", "dtype": dtype, "B": B, "repeat": r,
                                 "tick_device_ms": round(ms, 4), "frames_per_s": round(B / ms * 1e3, 1),
                                 "single_stream_one_launch_device_ms": round(single, 4),
                                 "ratio_vs_B_sequential": round(ms / (B * single), 4)})
    return rows


def _imu_graph():
    """The reference's 7-node IMU sensor graph (data/skeletons/imu_fogit_ABCD.json), from the graph fixtures."""
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "graphs.npz"))
    V, center = (int(v) for v in g["meta/imu_fogit_ABCD"])
    return {"num_node": V, "edge": g["edge/imu_fogit_ABCD"].tolist(), "center": center}


def infeat(P, dev, tree, repeat, emit, batches=(1, 64, 256), imu_batches=(1, 64, 256, 1024)):
    """Rows of DESIGN 4.25 for one checkout (``tree``: its label) in one process, each handed to ``emit`` as it is
    measured; see the module docstring."""
    gen = torch.Generator(device=dev).manual_seed(3)
    fill = 32  # > the 17-frame FIFOs of the stride-2 layers (kernel 9)

    def row(**kw):
        emit(dict(tree=tree, repeat=repeat, **kw))

    with torch.no_grad():
        # (a) in_feat 3: the shapes of profiles/rt_streams.jsonl
        torch.manual_seed(0)
        m = P.MODELS["rt-st-gcn"](rank=None, **dict(RT_ARCH, graph=P.PKU_MMD)).to(dev).eval()
        m.prepare_benchmark(RT_ARCH)
        for B in batches:
            x = torch.randn(B, 3, 1, 25, device=dev, generator=gen)
            for dtype in ("fp32", "bf16"):
                sb = None
                sb = m.stream_batch(B, dtype)
                row(config="3 as a stream batch (stgcn_rt_streams), in_feat 3, V 25", dtype=dtype, B=B,
                    tick_device_ms=round(_replay_ms(lambda: sb.step(x), fill), 4))
        sb = m = None
        for dtype in ("fp32", "bf16"):
            arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": 9, "output_type": "logits",
                    "normalization": "LayerNorm", "num_classes": 52, "graph": P.PKU_MMD,
                    "st-gcn": dict(LAYERS, latency=False, importance=True, in_feat=3, stages=1, dilation=[1] * 9)}
            torch.manual_seed(0)
            mc = P.MODELS["co-st-gcn"](rank=None, **arch).to(dev).eval().set_compute_dtype(dtype)
            for B in batches:
                x = torch.randn(B, 3, 1, 25, device=dev, generator=gen)
                sb = mc.stream_batch(B)
                row(config="co-st-gcn as a stream batch (stgcn_co_streams), Kt 9, in_feat 3, V 25", dtype=dtype, B=B,
                    tick_device_ms=round(_replay_ms(lambda: sb.step(x), fill), 4))
                sb = None
                torch.cuda.empty_cache()
        mc = None
        # (b) the reference's IMU model: in_feat 6, V 7
        graph = _imu_graph()
        V = graph["num_node"]
        arch = dict(RT_ARCH, in_feat=6, num_classes=2, graph=graph)
        arch["rt-st-gcn"] = dict(RT_ARCH["rt-st-gcn"], in_feat=6)
        name = "rt-st-gcn imu_fogit_ABCD (in_feat 6, V 7, config 3's nine layers, LN, K=9)"
        torch.manual_seed(0)
        m = P.MODELS["rt-st-gcn"](rank=None, **arch).to(dev).eval()
        m.prepare_benchmark(arch)
        for B in imu_batches:
            x = torch.randn(B, 6, 1, V, device=dev, generator=gen)
            for dtype in ("fp32", "bf16"):
                try:
                    sb = None
                    sb = m.stream_batch(B, dtype)
                except RuntimeError as e:  # before the feature: refused on the host, nothing ran
                    row(config=name + " as a stream batch", dtype=dtype, B=B, refused=str(e))
                    continue
                ms = _replay_ms(lambda: sb.step(x), fill)
                row(config=name + " as a stream batch", dtype=dtype, B=B, tick_device_ms=round(ms, 4),
                    frames_per_s=round(B / ms * 1e3, 1),
                    note="V = 7 fills 7 of the 32 rows of the MFMA operand")
        sb = None
        # one stream, one frame per Model.forward call, eager: wall time per synchronised frame and device time of
        # 200 back-to-back frames.  The route is the checkout's own: one persistent launch where the head takes
        # in_feat 6, the generic layer kernels where it does not.
        frames = torch.randn(264, 1, 6, 1, V, device=dev, generator=gen)
        m.reset_state()
        lat = []
        for i in range(264):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m(frames[i])
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(200):
            m(frames[i])
        e1.record()
        torch.cuda.synchronize()
        one = getattr(m, "_frame_pack", None) is not None
        out = {"eager_p50_ms": round(1e3 * pct(lat[64:], 0.5), 4),
               "eager_back_to_back_ms_per_frame": round(e0.elapsed_time(e1) / 200, 4)}
        if one:  # the one-launch route captures as config 3's does
            x1 = frames[0].clone()
            out["graph_device_ms_per_frame"] = round(_replay_ms(lambda: m(x1), fill), 4)
        row(config=name + ", one stream, one frame per call", dtype="fp32",
            route="one persistent launch (stgcn_rt_frame)" if one else "generic layer kernels, frame by frame", **out)


def config5(P, dev, steps, warmup):
    torch.manual_seed(1538574472)
    m = P.MODELS["aa-gcn"](rank=None, **dict(AAGCN_ARCH, graph=P.PKU_MMD)).to(dev).set_compute_dtype("bf16")
    opt = P.optim.Adam(m.parameters(), lr=5e-4)  # the package's one-launch Adam (as bench.py)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(64, 3, 300, 25, device=dev, generator=gen)
    labels = torch.randint(0, 52, (64,), device=dev, generator=gen)

    def step():
        y = m(x)
        loss = torch.nn.functional.nll_loss(torch.log(y.reshape(64, 52).clamp_min(1e-12)), labels)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"config": "5: aa-gcn (as_is/aagcn_local.json, 2 streams, BN, 9 layers) fwd+bwd+Adam, bf16, "
                      "N=64 T=300 V=25", "metric": "skeleton-frames/s", "value": round(steps * 64 * 300 / dt, 1),
            "ms_per_step": round(1e3 * dt / steps, 3), "steps": steps, "data": "synthetic"}


LN_ARCH = {"strategy": "spatial", "in_feat": 3, "normalization": "LayerNorm", "num_classes": 52,
           "output_type": "logits", "st-gcn": dict(LAYERS, importance=True, in_feat=3)}


def ln_train(P, dev, steps, warmup, reps=3, routes=(True, False)):
    """The LayerNorm st-gcn (ln/stgcn_vsc.json-style: LN, Kt = 9, config-2 widths) training step (fwd + loss +
    bwd + Adam, bf16, N=64 T=300) with its three 64 -> 64 layers' forward on the fused one-kernel layer
    (routing.fused_ln_train) and unfused (default), interleaved ``reps`` times."""
    R = P.routing.ROUTING
    torch.manual_seed(1538574472)
    m = P.MODELS["st-gcn"](rank=None, **dict(LN_ARCH, graph=P.PKU_MMD)).to(dev).set_compute_dtype("bf16")
    opt = P.optim.Adam(m.parameters(), lr=5e-4)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(64, 3, 300, 25, device=dev, generator=gen)
    labels = torch.randint(0, 52, (1, 64), device=dev, generator=gen)
    crit = P.loss.Loss(dev, torch.rand(52, device=dev, generator=gen) + 0.5)

    def step():
        ce, mse = crit(0, m(x).permute(2, 1, 0), labels)
        (ce + mse).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    out = {"config": "ln st-gcn (LayerNorm, Kt=9, 9 layers, config-2 widths) fwd+loss+bwd+Adam, bf16, N=64 T=300",
           "metric": "ms/step"}
    prev = R.fused_ln_train
    try:
        for rep in range(reps):
            for route in routes:
                R.fused_ln_train = route
                for _ in range(warmup):
                    step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step()
                torch.cuda.synchronize()
                k = "fused_ms_per_step" if route else "unfused_ms_per_step"
                out.setdefault(k, []).append(round(1e3 * (time.perf_counter() - t0) / steps, 3))
    finally:
        R.fused_ln_train = prev
    if "fused_ms_per_step" in out:
        out["fused_frames_per_s"] = round(64 * 300 / (min(out["fused_ms_per_step"]) * 1e-3), 1)
    return out


def staging(P, dev, reps=50):
    import torch.nn.functional as F
    W, nw, L, C, V, Cout = 50, 1000, 1000, 3, 25, 64
    gen = torch.Generator(device=dev).manual_seed(5)
    padded = F.pad(torch.randn(1, C, L, V, device=dev, generator=gen), (0, 0, W - 1, 0))
    w = torch.randn(Cout, C, 1, 1, device=dev, generator=gen).requires_grad_(True)
    b = torch.zeros(Cout, device=dev).requires_grad_(True)
    bf = torch.bfloat16
    out = {"config": "f1: window staging, 1000 windows x W=50 (ln/stgcn_local.json segment), C=3 -> 64, bf16",
           "out_bytes": nw * W * V * Cout * 2}
    for norm, mode in (("BatchNorm", 0), ("LayerNorm", 1)):
        if mode == 0:
            mod = P.BatchNorm1d(C * V).to(dev)
            gw, gb = mod.norm.weight, mod.norm.bias
        else:
            mod = P.LayerNorm([C, 1, V]).to(dev)
            gw, gb = mod.weight, mod.bias
        dy = torch.randn(nw, W, V, Cout, device=dev, generator=gen).to(bf).permute(0, 3, 1, 2)

        def staged():
            return P.layer_fn.WindowStageFunction.apply(padded, 0, nw, W, gw, gb, w, b, mode, bf)

        def unfolded():
            x = P.segment.WindowBatch(padded, 0, nw, W).materialize()
            x = mod(x)
            x = F.pad(x.permute(0, 2, 3, 1), (0, 8 - C)).permute(0, 3, 1, 2)
            return P.layer_fn.Conv1x1Function.apply(x, F.pad(w, (0, 0, 0, 0, 0, 8 - C)), b, bf)

        for name, fn in (("staged", staged), ("unfold_norm_conv", unfolded)):
            for _ in range(3):
                fn().backward(dy)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            tf = tb = 0.0
            for _ in range(reps):
                ev[0].record()
                y = fn()
                ev[1].record()
                y.backward(dy)
                ev[2].record()
                torch.cuda.synchronize()
                tf += ev[0].elapsed_time(ev[1])
                tb += ev[1].elapsed_time(ev[2])
            out["%s_%s_fwd_us" % (norm, name)] = round(1e3 * tf / reps, 1)
            out["%s_%s_bwd_us" % (norm, name)] = round(1e3 * tb / reps, 1)
        out["%s_staged_fwd_GBps" % norm] = round(out["out_bytes"] / (out["%s_staged_fwd_us" % norm] * 1e3), 1)
        out["%s_staged_bwd_GBps" % norm] = round(out["out_bytes"] / (out["%s_staged_bwd_us" % norm] * 1e3), 1)
    return out


HBM_PEAK_BPS = 8.0e12  # MI355X HBM3E specification peak


def costgcn(P, dev, kernel, dtype, frames=256, cpu_frames=3):
    """One line of the co-st-gcn table: the reference schedule at temporal kernel ``kernel`` in ``dtype``."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from costgcn_ref import costgcn_stream
    arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": 52, "graph": P.PKU_MMD,
            "st-gcn": dict(LAYERS, kernel=kernel, latency=False, importance=True, in_feat=3, stages=1,
                           dilation=[1] * 9)}
    torch.manual_seed(0)
    m = P.MODELS["co-st-gcn"](rank=None, **arch)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(dev).eval().set_compute_dtype(dtype)
    fill = max(arch["st-gcn"]["stride"]) * (kernel - 1) + 1
    gen = torch.Generator(device=dev).manual_seed(3)
    stream = torch.randn(fill + frames + 8, 1, 3, 1, 25, device=dev, generator=gen)
    es = 2 if dtype == "bf16" else 4
    wbytes = sum(kernel * c * c * es for c in LAYERS["out_ch"])
    with torch.no_grad():
        x_static = torch.zeros_like(stream[0])
        for i in range(3):
            x_static.copy_(stream[i])
            m(x_static)
        m.reset_state()
        g = torch.cuda.CUDAGraph()
        s_ = torch.cuda.Stream()
        s_.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s_):
            with torch.cuda.graph(g):
                m(x_static)
        torch.cuda.current_stream().wait_stream(s_)
        m.reset_state()
        for i in range(fill):  # fill every FIFO
            x_static.copy_(stream[i])
            g.replay()
        lat = []
        for i in range(frames):
            x_static.copy_(stream[fill + i])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.replay()
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / frames
        splits = [d.splits for d in m._plan[1]["descs"]]
        # the restatement on the host (the reference's own arithmetic: FIFOs in CPU tensors)
        xc = stream[:cpu_frames + 1, 0].permute(1, 2, 0, 3).reshape(1, 3, cpu_frames + 1, 25).cpu()
        costgcn_stream(xc[:, :, :1], sd, arch, sd["A"], round_bf16=dtype == "bf16")
        t0 = time.perf_counter()
        costgcn_stream(xc[:, :, 1:], sd, arch, sd["A"], round_bf16=dtype == "bf16")
        cpu_ms = 1e3 * (time.perf_counter() - t0) / cpu_frames
    return {"config": f"co-st-gcn continual inference (ln/costgcn_local.json widths, LN, 9 layers), Kt={kernel}, "
                      "1 frame (1,3,1,25)",
            "metric": "per-frame latency, HIP graph replay, FIFOs full", "unit": "ms", "dtype": dtype,
            "frames": frames, "p50_ms": round(1e3 * pct(lat, 0.5), 4), "p90_ms": round(1e3 * pct(lat, 0.9), 4),
            "device_ms_per_frame": round(dev_ms, 4), "k_splits": splits,
            "tap_weight_bytes_per_frame": wbytes,
            "hbm_peak_fraction": round(wbytes / (dev_ms * 1e-3) / HBM_PEAK_BPS, 4),
            "hbm_peak_note": "tap-weight bytes / device time / 8.0 TB/s; the packs fit the 256 MiB Infinity Cache, "
                             "so this is an equivalent rate, not measured HBM traffic",
            "host_restatement_ms_per_frame": round(cpu_ms, 2), "host_threads": torch.get_num_threads(),
            "reference_cited": "BASELINE.md: CoST-GCN per-frame 204 ms (Kt=9), 1.351 s (Kt=69)"}


def co_streams(P, dev, kernel, dtype, batches=(1, 8, 64, 256)):
    """Rows of the co-st-gcn stream-batch table: the reference schedule at temporal kernel ``kernel`` in ``dtype`` as
    a stream batch (Model.stream_batch, stgcn_co_streams) of B streams, one tick captured as a HIP graph, beside the
    single-stream route graph-replayed in the same run."""
    arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": 52, "graph": P.PKU_MMD,
            "st-gcn": dict(LAYERS, kernel=kernel, latency=False, importance=True, in_feat=3, stages=1,
                           dilation=[1] * 9)}
    torch.manual_seed(0)
    m = P.MODELS["co-st-gcn"](rank=None, **arch).to(dev).eval().set_compute_dtype(dtype)
    fill = max(arch["st-gcn"]["stride"]) * (kernel - 1) + 1
    gen = torch.Generator(device=dev).manual_seed(3)
    es = 2 if dtype == "bf16" else 4
    ring_bytes = sum(kernel * 25 * c * es for c in LAYERS["out_ch"])  # what one stream's tap stages read per tick
    wbytes = sum(kernel * c * c * es for c in LAYERS["out_ch"])
    rows = []
    with torch.no_grad():
        x1 = torch.randn(1, 3, 1, 25, device=dev, generator=gen)
        single = _replay_ms(lambda: m(x1), fill)
        for B in batches:
            sb = m.stream_batch(B)
            x = torch.randn(B, 3, 1, 25, device=dev, generator=gen)
            ms = _replay_ms(lambda: sb.step(x), fill)
            rows.append({"config": f"co-st-gcn as a stream batch (stgcn_co_streams), ln/costgcn_local.json widths, "
                                   f"Kt={kernel}: B streams, one frame each per tick",
                         "dtype": dtype, "Kt": kernel, "B": B, "tick_device_ms": round(ms, 4),
                         "frames_per_s": round(B / ms * 1e3, 1), "single_stream_graph_device_ms": round(single, 4),
                         "ratio_vs_B_sequential": round(ms / (B * single), 4),
                         "k_splits": [sb._desc()[0].layers[i].splits for i in range(9)],
                         "state_bytes_per_stream": sb.state_bytes // B,
                         "ring_bytes_per_tick": B * ring_bytes,
                         "tap_weight_bytes_per_tick": -(-B // 4) * wbytes,
                         "ring_hbm_peak_fraction": round(B * ring_bytes / (ms * 1e-3) / HBM_PEAK_BPS, 4),
                         "note": "HIP events around 200 graph replays after the rings filled; no per-kernel trace"})
            del sb
            torch.cuda.empty_cache()
    return rows


def _capture(step):
    step()  # descriptors, packs and buffers outside the capture
    g = torch.cuda.CUDAGraph()
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        with torch.cuda.graph(g):
            step()
    torch.cuda.current_stream().wait_stream(s_)
    return g


def _timed(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def co_clip(P, dev, kernel, dtype, Ts=(1, 4, 16, 64, 256), repeats=3):
    """Rows of the co-st-gcn clip table: the reference schedule at temporal kernel ``kernel`` in ``dtype``, one
    forward_clip of T frames captured as a HIP graph, beside the per-frame route graph-replayed in the same run.  Both
    act on the same stream with its rings filled; the timed windows alternate (per-frame, every T) ``repeats`` times and
    each row gives the median and the min / max of its windows."""
    arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": 52, "graph": P.PKU_MMD,
            "st-gcn": dict(LAYERS, kernel=kernel, latency=False, importance=True, in_feat=3, stages=1,
                           dilation=[1] * 9)}
    torch.manual_seed(0)
    m = P.MODELS["co-st-gcn"](rank=None, **arch).to(dev).eval().set_compute_dtype(dtype)
    fill = max(arch["st-gcn"]["stride"]) * (kernel - 1) + 1
    gen = torch.Generator(device=dev).manual_seed(3)
    es = 2 if dtype == "bf16" else 4
    wbytes = sum(kernel * c * c * es for c in LAYERS["out_ch"])
    with torch.no_grad():
        x1 = torch.randn(1, 3, 1, 25, device=dev, generator=gen)
        xs = {T: torch.randn(1, 3, T, 25, device=dev, generator=gen) for T in Ts}
        frame = _capture(lambda: m(x1))
        clip = {T: _capture(lambda T=T: m.forward_clip(xs[T])) for T in Ts}
        for _ in range(fill):
            frame.replay()
        reps = {T: max(10, 512 // T) for T in Ts}  # at least 512 frames per window
        for T in Ts:  # every shape once before a timed window
            clip[T].replay()
        t_frame, t_clip = [], {T: [] for T in Ts}
        for _ in range(repeats):
            t_frame.append(_timed(frame, 500))
            for T in Ts:
                t_clip[T].append(_timed(clip[T], reps[T]))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    d = m._clip_desc(m._plan[1], 1)
    rows = []
    for T in Ts:
        ms = med(t_clip[T])
        rows.append({"config": "co-st-gcn clip inference (stgcn_co_clip), ln/costgcn_local.json widths, "
                               f"Kt={kernel}: one clip of T frames on one stream",
                     "dtype": dtype, "Kt": kernel, "T": T, "clip_device_ms": round(ms, 4),
                     "clip_device_ms_min_max": [round(min(t_clip[T]), 4), round(max(t_clip[T]), 4)],
                     "clip_ms_per_frame": round(ms / T, 5),
                     "per_frame_route_ms_per_frame": round(med(t_frame), 4),
                     "per_frame_route_ms_min_max": [round(min(t_frame), 4), round(max(t_frame), 4)],
                     "ratio_per_frame_over_clip": round(med(t_frame) / (ms / T), 2),
                     "ratio_min_max": [round(min(t_frame) / (max(t_clip[T]) / T), 2),
                                       round(max(t_frame) / (min(t_clip[T]) / T), 2)],
                     "frames_per_s": round(T / ms * 1e3, 1), "k_splits": [d.layers[i].splits for i in range(9)],
                     "launches_per_clip": 2 + 5 * 9, "tap_weight_bytes": wbytes,
                     "note": f"HIP events around graph replays ({reps[T]} clips, 500 frames per window), {repeats} "
                             "alternating windows, rings filled; no per-kernel trace"})
    return rows


def co_streams_clip(P, dev, kernel, dtype, batches=(1, 8, 64), Ts=(4, 16, 64), repeats=3):
    """Rows of the co-st-gcn stream-batch clip table: the reference schedule at temporal kernel ``kernel`` in
    ``dtype``, one step_clip of B streams x T frames (one stgcn_co_streams_clip call: clip_frames raised to B * T)
    captured as a HIP graph, beside (a) B replays of a captured forward_clip of T frames and (b) T replays of a captured
    step of B streams, in the same run with the rings filled.  The timed windows alternate ``repeats`` times; each row
    gives the median and the min / max of its windows."""
    arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": 52, "graph": P.PKU_MMD,
            "st-gcn": dict(LAYERS, kernel=kernel, latency=False, importance=True, in_feat=3, stages=1,
                           dilation=[1] * 9)}
    torch.manual_seed(0)
    m = P.MODELS["co-st-gcn"](rank=None, **arch).to(dev).eval().set_compute_dtype(dtype)
    fill = max(arch["st-gcn"]["stride"]) * (kernel - 1) + 1
    gen = torch.Generator(device=dev).manual_seed(3)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rows = []
    with torch.no_grad():
        xc = {T: torch.randn(1, 3, T, 25, device=dev, generator=gen) for T in Ts}
        single = {T: _capture(lambda T=T: m.forward_clip(xc[T])) for T in Ts}
        for _ in range(-(-fill // min(Ts))):
            single[min(Ts)].replay()
        for B in batches:
            sb = m.stream_batch(B)
            sb.clip_frames = max(sb.clip_frames, B * max(Ts))
            x1 = torch.randn(B, 3, 1, 25, device=dev, generator=gen)
            tick = _capture(lambda: sb.step(x1))
            for _ in range(fill):
                tick.replay()
            for T in Ts:
                x = torch.randn(B, 3, T, 25, device=dev, generator=gen)
                clip = _capture(lambda: sb.step_clip(x))
                # every window at least ~256 frames of one stream and at least 3 replays
                reps = max(3, 256 // (B * T))
                t_clip, t_a, t_b = [], [], []
                for _ in range(repeats):
                    t_clip.append(_timed(clip, reps))
                    t_a.append(_timed(single[T], reps * B) * B)
                    t_b.append(_timed(tick, reps * T) * T)
                ms, a, b = med(t_clip), med(t_a), med(t_b)
                rows.append({"config": "co-st-gcn stream-batch clip (stgcn_co_streams_clip), ln/costgcn_local.json "
                                       f"widths, Kt={kernel}: one step_clip of B streams x T frames",
                             "dtype": dtype, "Kt": kernel, "B": B, "T": T, "step_clip_device_ms": round(ms, 4),
                             "step_clip_ms_min_max": [round(min(t_clip), 4), round(max(t_clip), 4)],
                             "B_forward_clips_device_ms": round(a, 4),
                             "B_forward_clips_ms_min_max": [round(min(t_a), 4), round(max(t_a), 4)],
                             "T_step_ticks_device_ms": round(b, 4),
                             "T_step_ticks_ms_min_max": [round(min(t_b), 4), round(max(t_b), 4)],
                             "ratio_B_forward_clips_over_step_clip": round(a / ms, 2),
                             "ratio_T_step_ticks_over_step_clip": round(b / ms, 2),
                             "frames_per_s": round(B * T / ms * 1e3, 1),
                             "k_splits": [sb._desc()[0].layers[i].splits for i in range(9)],
                             "launches_per_step_clip": 2 + 5 * 9, "clip_frames": sb.clip_frames,
                             "clip_scratch_bytes": sb.scratch_bytes - sb._step_bytes,
                             "state_bytes_per_stream": sb.state_bytes // B,
                             "note": f"HIP events around graph replays ({reps} step_clips, {reps * B} forward_clips, "
                                     f"{reps * T} ticks per window), {repeats} alternating windows, rings filled; no "
                                     "per-kernel trace"})
                del clip
            del sb, tick
            torch.cuda.empty_cache()
    return rows


def rt_streams_clip(P, dev, batches=(1, 8, 64, 256), Ts=(4, 16, 64), repeats=3):
    """Rows of the rt-st-gcn stream-batch clip table: config 3's widths and strides, V = 25, per operand type one
    step_clip of B streams x T frames (one stgcn_rt_streams_clip call: clip_frames raised to B * T) captured as a HIP
    graph, beside T replays of a captured step of B streams in the same run and process, rings filled.  The timed
    windows alternate ``repeats`` times; each row gives the median and the min / max of its windows."""
    torch.manual_seed(0)
    m = P.MODELS["rt-st-gcn"](rank=None, **dict(RT_ARCH, graph=P.PKU_MMD)).to(dev)
    m.eval()
    m.prepare_benchmark(RT_ARCH)
    gen = torch.Generator(device=dev).manual_seed(3)
    fill = 32  # > the 17-frame FIFO of the stride-2 layers
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rows = []
    with torch.no_grad():
        for B in batches:
            for dtype in ("fp32", "bf16"):
                sb = m.stream_batch(B, dtype)
                sb.clip_frames = max(sb.clip_frames, B * max(Ts))
                x1 = torch.randn(B, 3, 1, 25, device=dev, generator=gen)
                tick = _capture(lambda: sb.step(x1))
                for _ in range(fill):
                    tick.replay()
                for T in Ts:
                    x = torch.randn(B, 3, T, 25, device=dev, generator=gen)
                    clip = _capture(lambda: sb.step_clip(x))
                    reps = max(3, 256 // (B * T))  # every window at least ~256 frames of one stream and 3 replays
                    t_clip, t_tick = [], []
                    for _ in range(repeats):
                        t_clip.append(_timed(clip, reps))
                        t_tick.append(_timed(tick, reps * T) * T)
                    ms, b = med(t_clip), med(t_tick)
                    rows.append({"config": "3 as a stream-batch clip (stgcn_rt_streams_clip): one step_clip of B streams "
                                           "x T frames", "dtype": dtype, "B": B, "T": T,
                                 "step_clip_device_ms": round(ms, 4),
                                 "step_clip_ms_min_max": [round(min(t_clip), 4), round(max(t_clip), 4)],
                                 "T_step_ticks_device_ms": round(b, 4),
                                 "T_step_ticks_ms_min_max": [round(min(t_tick), 4), round(max(t_tick), 4)],
                                 "ratio_T_step_ticks_over_step_clip": round(b / ms, 2),
                                 "ratio_min_max": [round(min(t_tick) / max(t_clip), 2),
                                                   round(max(t_tick) / min(t_clip), 2)],
                                 "frames_per_s": round(B * T / ms * 1e3, 1), "launches_per_step_clip": 2 * 9 + 1,
                                 "clip_frames": sb.clip_frames, "clip_scratch_bytes": sb.scratch_bytes,
                                 "state_bytes_per_stream": sb.state_bytes // B,
                                 "note": f"HIP events around graph replays ({reps} step_clips, {reps * T} ticks per "
                                         f"window), {repeats} alternating windows, rings filled; no per-kernel trace"})
                    del clip
                del sb, tick
                torch.cuda.empty_cache()
    return rows


def stream_state(P, dev, kernel, dtype, B=64, reps=20):
    """One row of the snapshot table: the reference schedule at temporal kernel ``kernel`` in ``dtype`` as a batch of B
    streams out of step, every stream exported and imported in one launch each, beside torch.clone of the same number
    of bytes and the torch-level composition of the same copy."""
    arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": 52, "graph": P.PKU_MMD,
            "st-gcn": dict(LAYERS, kernel=kernel, latency=False, importance=True, in_feat=3, stages=1,
                           dilation=[1] * 9)}
    torch.manual_seed(0)
    m = P.MODELS["co-st-gcn"](rank=None, **arch).to(dev).eval().set_compute_dtype(dtype)
    gen = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        sb, dst = m.stream_batch(B), m.stream_batch(B)
        # heads everywhere: stream b has consumed 3 b + 1 frames
        sb.step_clip(torch.randn(B, 3, 3 * B + 1, 25, device=dev, generator=gen), None, [3 * b + 1 for b in range(B)])
        snap = sb.export_state()
        slots = torch.arange(B, dtype=torch.int32, device=dev)  # import's targets, read on the device
        # each call captured once and replayed: HIP events then bracket device work, not the host's launch path
        export_ms = _timed(_capture(lambda: sb.export_state()), reps)
        import_ms = _timed(_capture(lambda: dst.import_state(snap, slots)), reps)
        assert torch.equal(dst.export_state().data, snap.data)
        clone_ms = _timed(_capture(lambda: snap.data.clone()), reps)
        out = torch.empty_like(snap.data)
        V = snap.V

        def torch_export():
            for b in range(B):
                heads = torch.stack([idx[b] for _, _, idx in sb.state]).tolist()  # one read-back per stream
                for (ring, res, _), (C, n0, n1, off0, off1), (i0, i1) in zip(sb.state, snap.layout, heads):
                    out[b, off0:off1].view(n0, V, C).copy_(ring[b].roll(-i0, 0))
                    out[b, off1:off1 + n1 * V * C].view(n1, V, C).copy_(res[b].roll(-i1, 0))

        def torch_import():
            for b in range(B):
                for (ring, res, idx), (C, n0, n1, off0, off1) in zip(dst.state, snap.layout):
                    ring[b].copy_(snap.data[b, off0:off1].view(n0, V, C))
                    res[b].copy_(snap.data[b, off1:off1 + n1 * V * C].view(n1, V, C))
                    idx[b].zero_()

        torch_export_ms = _dev_ms(torch_export, 3, warm=1)
        assert torch.equal(out, snap.data)
        torch_import_ms = _dev_ms(torch_import, 3, warm=1)
        assert torch.equal(dst.export_state().data, snap.data)
    nbytes = snap.data.numel() * 4
    row = {"config": f"co-st-gcn stream snapshots (stgcn_stream_state_export / _import), ln/costgcn_local.json widths, "
                     f"Kt={kernel}: all B streams, one launch each way",
           "dtype": dtype, "Kt": kernel, "B": B, "snapshot_bytes": nbytes, "state_bytes": sb.state_bytes,
           "export_device_ms": round(export_ms, 4), "import_device_ms": round(import_ms, 4),
           "clone_device_ms": round(clone_ms, 4), "torch_export_ms": round(torch_export_ms, 3),
           "torch_import_ms": round(torch_import_ms, 3),
           "export_over_clone": round(export_ms / clone_ms, 3), "import_over_clone": round(import_ms / clone_ms, 3),
           "export_over_torch": round(export_ms / torch_export_ms, 5),
           "import_over_torch": round(import_ms / torch_import_ms, 5),
           "export_snapshot_GBps": round(nbytes / export_ms / 1e6, 1),
           "note": f"export, import and clone: HIP events around {reps} replays of the captured call; the torch "
                   "composition: HIP events around 3 eager runs, its B host read-backs included; no per-kernel trace"}
    del sb, dst, snap, out
    torch.cuda.empty_cache()
    return row


MS_TCN = {"latency": False, "importance": True, "stages": 3, "layers": [10, 10, 10], "kernel": [3, 3, 3],
          "filters": [64, 64, 64], "dropout": [0, 0, 0]}
MSGCN_ARCH = {"strategy": "spatial", "receptive_field": 50, "segment": 2000, "in_feat": 3, "stages": 4,
              "refine": "softmax", "output_type": "logits", "normalization": "BatchNorm", "num_classes": 52,
              "st-gcn": dict(LAYERS, latency=False, importance=True, in_feat=3, stages=1), "ms-tcn": MS_TCN}


def _dev_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def ms_stage(P, dev, dtype, L=2000, F=64, C=52, nl=10, reps=20):
    """One refinement stage on a (1, C, L, 1) series: forward, forward + backward, and each layer kernel alone."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mstcn_ref as R
    K = P.native
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    torch.manual_seed(0)
    st = P.mstcn.SingleStage(in_channels=C, out_channels=C, num_filters=F, num_layers=nl, kernel=3, dropout=0.0)
    sd = {k: v.clone() for k, v in st.state_dict().items()}
    st = st.to(dev).train()
    st.compute_dtype = dt
    x = torch.randn(L, C, device=dev, requires_grad=True)
    g = torch.randn(L, C, device=dev)

    def fwd():
        with torch.no_grad():
            st.run_rows(x, 1, 1, 2)

    def fwd_bwd():
        st.zero_grad(set_to_none=True)
        x.grad = None
        (st.run_rows(x, 1, 1, 2) * g).sum().backward()

    es = 2 if dtype == "bf16" else 4
    a = torch.randn(L, F, device=dev)
    layers = []
    for j, layer in enumerate(st.layers):
        wp = K.ms_pack_layer(layer.conv[0].weight, layer.conv[2].weight, dt)
        b1, b2 = layer.conv[0].bias, layer.conv[2].bias
        _, h = K.ms_layer_fwd(a, wp, b1, b2, 1, 2 ** j, dt, True)
        t_f = _dev_ms(lambda: K.ms_layer_fwd(a, wp, b1, b2, 1, 2 ** j, dt, True), 50)
        t_b = _dev_ms(lambda: K.ms_layer_bwd(a, wp, h, a, 1, 2 ** j, dt), 50)
        # algorithmic bytes: forward reads x and the W1 | W2 panels, writes y and h; backward (4 launches) reads dy
        # (three times), h (twice), x, g (twice), the transposed panels and the partials, writes g, dx, partials, grads
        by_f = L * F * (8 + es) + 4 * F * F * es
        by_b = L * F * (20 + 5 * es) + 4 * F * F * es + 2 * (4 * F * F + 2 * F) * 4 * P._lib.lib().stgcn_ms_wgrad_blocks(L)
        layers.append({"dilation": 2 ** j, "fwd_us": round(1e3 * t_f, 2), "bwd_us": round(1e3 * t_b, 2),
                       "fwd_bytes": by_f, "bwd_bytes": by_b, "fwd_GBps": round(by_f / (t_f * 1e-3) / 1e9, 1),
                       "bwd_GBps": round(by_b / (t_b * 1e-3) / 1e9, 1)})
    t_fwd, t_step = _dev_ms(fwd, reps), _dev_ms(fwd_bwd, reps)
    xc, gc = x.detach().cpu().t().reshape(1, C, L, 1), g.cpu().t().reshape(1, C, L, 1)

    def host():
        R.grads_of(lambda a_, s_: R.single_stage(torch.softmax(a_, 1), s_, round_bf16=dtype == "bf16"), xc, sd, gc,
                   input_grad=True)
    host()
    t0 = time.perf_counter()
    for _ in range(3):
        host()
    cpu_ms = 1e3 * (time.perf_counter() - t0) / 3
    return {"config": f"ms-tcn refinement stage: softmax + conv_in {C}->{F}, {nl} dilated residual layers, conv_out "
                      f"{F}->{C}, series (1,{C},{L},1)", "metric": "device time per call (HIP events, eager launches)",
            "unit": "ms", "dtype": dtype, "fwd_ms": round(t_fwd, 4), "fwd_bwd_ms": round(t_step, 4),
            "launches_fwd": 2 + 2 * nl, "launches_bwd": 4 + 4 * nl, "layers": layers,
            "host_restatement_fwd_bwd_ms": round(cpu_ms, 2), "host_threads": torch.get_num_threads()}


def msgcn_step(P, dev, dtype, steps, L=2000):
    """One ms-gcn training step on one trial of L frames (one segment of L windows)."""
    arch = dict(MSGCN_ARCH, graph=P.PKU_MMD)
    torch.manual_seed(0)
    m = P.MODELS["ms-gcn"](rank=None, **arch).to(dev).train().set_compute_dtype(dtype)
    W = arch["receptive_field"]
    capture = torch.randn(1, 3, L + W - 1, 25, device=dev)
    labels = torch.randint(0, 52, (1, L), device=dev)
    batch = P.segment.WindowBatch(capture, 0, L, W)
    loss_fn = P.loss.LossMultiStage(dev, torch.ones(52))
    opt = P.optim.Adam(m.parameters(), lr=5e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        ce, mse = loss_fn(0, m(batch), labels)
        (ce + mse).backward()
        opt.step()

    def refine_only():
        with torch.no_grad():
            y = torch.zeros(L, 52, device=dev)
        y.requires_grad_(True)
        out = P.mstcn.refine_and_stack(y, m.refinement_stages, m.refine_mode, m.out_mode)
        ce, mse = loss_fn(0, out, labels)
        (ce + mse).backward()

    t_step = _dev_ms(step, steps, warm=2)
    t_ref = _dev_ms(refine_only, steps, warm=2)
    return {"config": f"ms-gcn training step (as_is/msgcn_vsc.json: BatchNorm st-gcn generator, {L} windows of {W} "
                      "frames, 3 refinement stages of 10 layers, F=64, 52 classes), LossMultiStage + Adam",
            "metric": "device time per step (HIP events)", "unit": "ms", "dtype": dtype, "steps": steps,
            "step_ms": round(t_step, 3), "refinement_and_loss_fwd_bwd_ms": round(t_ref, 3),
            "refinement_share": round(t_ref / t_step, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--ln-reps", type=int, default=3)
    ap.add_argument("--ln-route", choices=("both", "fused", "unfused"), default="both")
    ap.add_argument("--stream-repeats", type=int, default=3)
    ap.add_argument("--tree", default=None, help="infeat: another checkout of the project to measure instead")
    ap.add_argument("--label", default="branch", help="infeat: the rows' tree label")
    ap.add_argument("--repeat", type=int, default=0, help="infeat: the rows' repeat index")
    args = ap.parse_args()
    if args.tree:  # that checkout's package and library; this file only measures
        import importlib.util
        spec = importlib.util.spec_from_file_location("graft_entry_tree", os.path.join(args.tree, "__graft_entry__.py"))
        other = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(other)
        P = other.load_package()
    else:
        P = ge.load_package()
    dev = torch.device("cuda", 0)
    if args.only in (None, "3"):
        print(json.dumps(config3(P, dev, args.frames)), flush=True)
    if args.only in (None, "5"):
        print(json.dumps(config5(P, dev, args.steps, args.warmup)), flush=True)
    if args.only in (None, "ln"):
        print(json.dumps(ln_train(P, dev, args.steps, args.warmup, args.ln_reps,
                                    {"both": (True, False), "fused": (True,), "unfused": (False,)}[args.ln_route])), flush=True)
    if args.only in (None, "f1"):
        print(json.dumps(staging(P, dev)), flush=True)
    if args.only == "ms":
        for dtype in ("fp32", "bf16"):
            print(json.dumps(ms_stage(P, dev, dtype)), flush=True)
        for dtype in ("fp32", "bf16"):
            print(json.dumps(msgcn_step(P, dev, dtype, min(args.steps, 5))), flush=True)
    if args.only == "infeat":
        with open(os.path.join(ROOT, "profiles", "infeat.jsonl"), "a") as f:
            def emit(row):
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
            infeat(P, dev, args.label, args.repeat, emit)
    if args.only == "streams":
        with open(os.path.join(ROOT, "profiles", "rt_streams.jsonl"), "a") as f:
            for row in streams(P, dev, repeats=args.stream_repeats):
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
    if args.only == "co_streams":
        for kernel in (9, 69):
            for dtype in ("fp32", "bf16"):
                for row in co_streams(P, dev, kernel, dtype):
                    print(json.dumps(row), flush=True)
    if args.only == "co_clip":
        with open(os.path.join(ROOT, "profiles", "co_clip.jsonl"), "a") as f:
            for kernel in (9, 69):
                for dtype in ("fp32", "bf16"):
                    for row in co_clip(P, dev, kernel, dtype):
                        print(json.dumps(row), flush=True)
                        f.write(json.dumps(row) + "\n")
    if args.only == "co_streams_clip":
        with open(os.path.join(ROOT, "profiles", "co_streams_clip.jsonl"), "a") as f:
            for kernel in (9, 69):
                for dtype in ("fp32", "bf16"):
                    for row in co_streams_clip(P, dev, kernel, dtype):
                        print(json.dumps(row), flush=True)
                        f.write(json.dumps(row) + "\n")
    if args.only == "rt_streams_clip":
        with open(os.path.join(ROOT, "profiles", "rt_streams_clip.jsonl"), "a") as f:
            for row in rt_streams_clip(P, dev):
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
    if args.only == "stream_state":
        with open(os.path.join(ROOT, "profiles", "stream_state.jsonl"), "a") as f:
            for kernel in (9, 69):
                for dtype in ("fp32", "bf16"):
                    row = stream_state(P, dev, kernel, dtype)
                    print(json.dumps(row), flush=True)
                    f.write(json.dumps(row) + "\n")
    if args.only == "co":
        for kernel in (9, 69):
            for dtype in ("fp32", "bf16"):
                print(json.dumps(costgcn(P, dev, kernel, dtype)), flush=True)


if __name__ == "__main__":
    main()
