"""Snapshot and restore of live streams on the device (export_state / import_state, stgcn_stream_state_*,
stream_state.hip): a moved stream continues bit for bit, neighbours stay untouched, the exported buffer is the
restatement's canonical image, snapshots survive disk and a device round trip, a stream moves between a single-stream
model and a batch slot, between an fp32 and a bf16 co-st-gcn batch, and both calls replay from a captured graph with
device-side slots; slots outside the batch are skipped.

Networks: three layers 8 -> 8 -> 16 -> 16, strides 1 / 2 / 1, an identity residual, a residual conv and no residual;
(V, Kt, P) in NETS.  P = 1 is the reference's 'uniform' strategy, whose adjacency is all zeros (graph.py): the zero A is
replaced by a dense one through the state dict, as tests/test_rt_streams_clip_cpu.small_net does for its single
partition, so that a stream's state depends on its frames."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_state_ref as R  # noqa: E402
from conftest import assert_close  # noqa: E402
from costgcn_ref import randomise  # noqa: E402
from test_gpu_costgcn import TOL as TOL_CO  # noqa: E402  (co-st-gcn's bar between a route and its reference)
from test_gpu_rt_streams import _randomise  # noqa: E402
from test_gpu_rt_streams_clip import TOL_ROUTES  # noqa: E402  (the project's bar between two fp32 rt-st-gcn routes)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

NETS = {"v25_k9_p3": (25, 9, 3), "v5_k3_p1": (5, 3, 1), "v5_k9_p3": (5, 9, 3), "v25_k3_p1": (25, 3, 1)}
FAMILIES = ["rt_fp32", "rt_bf16", "co_fp32", "co_bf16"]
CH_IN, CH_OUT, STRIDE, RESIDUAL = [8, 8, 16], [8, 16, 16], [1, 2, 1], [1, 1, 0]


@pytest.fixture(scope="module")
def P(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return pkg


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _graph(P, V):
    if V == 25:
        return dict(P.PKU_MMD)
    return {"num_node": 5, "edge": [[i, i] for i in range(5)] + [[0, 1], [1, 2], [2, 3], [3, 4]], "center": 2}


def _arch(P, family, V, Kt, parts):
    key = "rt-st-gcn" if family == "rt" else "st-gcn"
    conf = {"layers": 3, "kernel": Kt, "in_ch": list(CH_IN), "out_ch": list(CH_OUT), "stride": list(STRIDE),
            "residual": list(RESIDUAL), "dropout": [0.0] * 3, "dilation": [1] * 3, "latency": False, "importance": True,
            "in_feat": 3, "buffer": 1, "stages": 1}
    return {"strategy": "spatial" if parts == 3 else "uniform", "in_feat": 3, "stages": 1, "kernel": Kt,
            "output_type": "logits", "normalization": "LayerNorm", "segment": 500, "num_classes": 7, key: conf,
            "graph": _graph(P, V)}


_MODELS = {}


def model(P, family, net):
    """family 'rt' | 'co': (the fp32 model on the device, its state dict); built once per (family, net)."""
    if (family, net) in _MODELS:
        return _MODELS[family, net]
    V, Kt, parts = NETS[net]
    arch = _arch(P, family, V, Kt, parts)
    seed = 300 + 10 * sorted(NETS).index(net) + (family == "co")
    torch.manual_seed(seed)
    m = P.MODELS["rt-st-gcn" if family == "rt" else "co-st-gcn"](rank=None, **arch)
    sd = _randomise(m, seed + 1) if family == "rt" else randomise(m.state_dict(), torch.Generator().manual_seed(seed + 1))
    assert sd["A"].shape[0] == parts
    if parts == 1:
        sd["A"] = 0.2 + 0.3 * torch.rand(sd["A"].shape, generator=torch.Generator().manual_seed(seed + 2))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    if family == "rt":
        m.prepare_benchmark(arch)
    _MODELS[family, net] = (m, arch, sd)
    return _MODELS[family, net]


_BF16 = {}


def batch_of(P, fam, net, B):
    """A fresh batch of B streams of family ``fam`` (FAMILIES).  The bf16 co-st-gcn batches follow a second model
    with the same parameters and compute dtype bf16."""
    family, dt = fam.split("_")
    m, arch, sd = model(P, family, net)
    if family == "rt":
        return m.stream_batch(B, dtype=None if dt == "fp32" else "bf16")
    if dt == "bf16":
        if net not in _BF16:
            m16 = P.MODELS["co-st-gcn"](rank=None, **arch)
            m16.load_state_dict(sd, strict=True)
            _BF16[net] = m16.to(DEV).eval().set_compute_dtype(torch.bfloat16)
        m = _BF16[net]
    return m.stream_batch(B)


def frames(net, B, T, seed):
    return torch.randn(B, 3, T, NETS[net][0], generator=torch.Generator().manual_seed(seed)).to(DEV)


def slot_counts(batch):
    return [t.shape[1] for ts in batch.state for t in ts[:2]]


def lengths_for(batch):
    """[0, 1, n1, n2, n3]: never started; one frame; n1 = the least common multiple of every slot count (every head
    back at exactly 0 after wrapping); n2, n3 beyond twice the largest ring (every ring wrapped), one odd and one even,
    so that the stride-2 layer's two phases (accumulator / ring parity) differ between the streams."""
    counts = slot_counts(batch)
    big = 2 * max(counts)
    return [0, 1, math.lcm(*counts), big + 3, big + 4]


def state_clone(batch, b=None):
    return [t.clone() if b is None else t[b].clone() for ts in batch.state for t in ts]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def advanced(P, fam, net, seed=1):
    """A batch of 5 streams advanced by lengths_for's frame counts."""
    batch = batch_of(P, fam, net, 5)
    lengths = lengths_for(batch)
    batch.step_clip(frames(net, 5, max(lengths), seed), None, lengths)
    heads = [idx.cpu() for _, _, idx in batch.state]
    assert all(not h[0].any() and not h[2].any() for h in heads)            # never started; back at exactly 0
    assert all(h[3].any() for h in heads) and any((h[3] != h[4]).any() for h in heads)
    return batch, lengths


def cont(batch, x, ticks=3):
    """The continuation: the first frames as one clip, the last ``ticks`` one tick at a time -> (B, K, T)."""
    T = x.shape[2] - ticks
    ys = [batch.step_clip(x[:, :, :T])] + [batch.step(x[:, :, t:t + 1].contiguous()) for t in range(T, x.shape[2])]
    torch.cuda.synchronize()
    return torch.cat(ys, dim=2)


# ------------------------------------------------------------------------------------------------ 1. continuity
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("fam", FAMILIES)
def test_continuity_bit_for_bit(P, fam, net):
    """Streams 4, 2, 0, 1 of a batch of 5 are exported, rows 0, 1, 3 go into slots 1, 0, 2 of a fresh batch of 3, and
    both batches step over the same next 2 x (largest ring) frames: every moved stream's outputs equal those of the
    stream left in place, bit for bit.  Slots [1, 0, 2] are all of a batch of 3, so the slot that is not targeted is
    shown on a second fresh batch of 3 that takes rows 0, 1 into slots 1, 0: its slot 2 is a fresh stream."""
    src, lengths = advanced(P, fam, net)
    snap = src.export_state([4, 2, 0, 1])
    assert snap.n == 4 and snap.data.device == DEV and snap.data.dtype == torch.float32
    before = state_clone(src)
    dst = batch_of(P, fam, net, 3)
    dst.import_state(snap, [1, 0, 2], select=[0, 1, 3])
    part = batch_of(P, fam, net, 3)
    part.import_state(snap, [1, 0], select=[0, 1])
    fresh = batch_of(P, fam, net, 3)
    assert same(state_clone(src), before)                                     # exporting changes nothing
    T = 2 * max(slot_counts(src)) + 3
    x = frames(net, 5, T, 2)
    y_src = cont(src, x)
    moved = [4, 2, 1]                                                         # the streams now in slots 1, 0, 2
    y_dst = cont(dst, x[[2, 4, 1]].contiguous())
    for slot, b in zip([1, 0, 2], moved):
        assert torch.equal(y_dst[slot], y_src[b]), f"stream {b} in slot {slot} ({lengths[b]} frames before the move)"
    y_part = cont(part, x[[2, 4, 3]].contiguous())
    y_fresh = cont(fresh, x[[2, 4, 3]].contiguous())
    assert torch.equal(y_part[0], y_src[2]) and torch.equal(y_part[1], y_src[4])
    assert torch.equal(y_part[2], y_fresh[2])
    assert not torch.equal(y_fresh[0], y_src[2])                              # the history matters on these inputs


# ------------------------------------------------------------------------------------------------ 2. neighbours
@pytest.mark.parametrize("fam", FAMILIES)
def test_untouched_neighbours(P, fam):
    net = "v25_k9_p3"
    src, _ = advanced(P, fam, net)
    run = batch_of(P, fam, net, 4)
    run.step_clip(frames(net, 4, 21, 3), None, [21, 5, 13, 20])
    before = state_clone(run)
    run.import_state(src.export_state([3]), [2])
    torch.cuda.synchronize()
    after = state_clone(run)
    changed = False
    for t, u in zip(before, after):
        for b in (0, 1, 3):
            assert torch.equal(t[b], u[b])
        changed |= not torch.equal(t[2], u[2])
    assert changed
    assert all(not idx[2].any() for _, _, idx in run.state)                   # imported at rotation 0
    assert torch.equal(run.export_state([2]).data, src.export_state([3]).data)


# ------------------------------------------------------------------------------------------------ 3. canonical form
def host_layers(batch, b):
    return [(t0[b].float().cpu().numpy(), t1[b].cpu().numpy(), tuple(idx[b].tolist())) for t0, t1, idx in batch.state]


@pytest.mark.parametrize("net", ["v25_k9_p3", "v5_k3_p1"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_canonical_form(P, fam, net):
    """The exported buffer is the restatement's canonicalisation of the state read back to the host (a bf16 ring
    widened exactly), row by row and with the layout table the restatement computes; export -> import -> export
    returns the same buffer."""
    src, _ = advanced(P, fam, net)
    snap = src.export_state()
    assert snap.n == 5 and snap.kind == fam[:2]
    V = NETS[net][0]
    table, E = R.layout(V, [(t0.shape[-1], t0.shape[1], t1.shape[1]) for t0, t1, _ in src.state])
    assert snap.layout == tuple(table) and snap.E == E and snap.V == V
    got = snap.data.cpu()
    for b in range(5):
        assert torch.equal(got[b], torch.from_numpy(R.image(host_layers(src, b)))), f"stream {b}"
    order = [3, 0, 4, 1, 2]
    dst = batch_of(P, fam, net, 5)
    dst.import_state(snap, order)
    assert torch.equal(dst.export_state(order).data, snap.data)
    for b, slot in enumerate(order):                                          # the state itself: rotation 0, idx (0, 0)
        want = R.canonicalise(host_layers(src, b))
        for (t0, t1, idx), (w0, w1, _) in zip(host_layers(dst, slot), want):
            assert idx == (0, 0) and np.array_equal(t0, w0) and np.array_equal(t1, w1)


def test_unit_widths_of_a_bf16_ring(P):
    """V * C % 8 == 4 (V = 5, C = 12): a bf16 ring slot does not hold whole 16-byte units, the copy goes in units of 4
    elements; C = 16 beside it goes in units of 8."""
    arch = _arch(P, "co", 5, 3, 3)
    arch["st-gcn"].update(in_ch=[8, 12, 16], out_ch=[12, 16, 16])
    torch.manual_seed(77)
    m = P.MODELS["co-st-gcn"](rank=None, **arch)
    m.load_state_dict(randomise(m.state_dict(), torch.Generator().manual_seed(78)), strict=True)
    m = m.to(DEV).eval().set_compute_dtype(torch.bfloat16)
    src = m.stream_batch(3)
    src.step_clip(torch.randn(3, 3, 11, 5, generator=torch.Generator().manual_seed(79)).to(DEV), None, [11, 4, 7])
    assert src.state[0][0].dtype == torch.bfloat16
    snap = src.export_state()
    for b in range(3):
        assert torch.equal(snap.data[b].cpu(), torch.from_numpy(R.image(host_layers(src, b))))
    dst = m.stream_batch(3)
    dst.import_state(snap, [2, 0, 1])
    assert torch.equal(dst.export_state([2, 0, 1]).data, snap.data)
    x = torch.randn(3, 3, 12, 5, generator=torch.Generator().manual_seed(80)).to(DEV)
    assert torch.equal(cont(dst, x[[1, 2, 0]].contiguous())[[2, 0, 1]], cont(src, x))


# ------------------------------------------------------------------------------------------------ 4. disk and devices
@pytest.mark.parametrize("fam", FAMILIES)
def test_disk_and_device_round_trip(P, fam, tmp_path):
    net = "v5_k9_p3"
    src, lengths = advanced(P, fam, net)
    snap = src.export_state([3])
    torch.save(snap.to("cpu").state_dict(), tmp_path / "stream.pt")
    back = P.StreamSnapshot.from_state_dict(torch.load(tmp_path / "stream.pt", weights_only=True))
    assert back.device.type == "cpu" and torch.equal(back.data, snap.data.cpu()) and back.layout == snap.layout
    dst = batch_of(P, fam, net, 2)
    with pytest.raises(RuntimeError, match="snapshot.to"):
        dst.import_state(back, [1])
    dst.import_state(back.to(DEV), [1])
    x = frames(net, 5, 2 * max(slot_counts(src)) + 3, 4)
    assert torch.equal(cont(dst, x[[0, 3]].contiguous())[1], cont(src, x)[3])


# ------------------------------------------------------------------------------------------------ 5. single <-> batch
def test_single_and_batch_co(P):
    """A stream advanced by Model.forward and Model.forward_clip moves into a batch slot and a batch's stream into the
    model.  forward_clip and step_clip are documented as bit-identical: torch.equal; forward and step are two routes
    (co_frame.hip, co_streams.hip), held to test_gpu_costgcn.py's bar."""
    net = "v25_k9_p3"
    m, _, _ = model(P, "co", net)
    x = frames(net, 1, 80, 5)
    with torch.no_grad():
        m.reset_state()
        for t in range(5):
            m(x[:, :, t:t + 1])
        m.forward_clip(x[:, :, 5:28])
        snap = m.export_state()
        assert snap.n == 1 and snap.kind == "co"
        batch = m.stream_batch(3)
        assert snap.layout == batch.export_state([0]).layout
        batch.import_state(snap, [2])
        xb = x[:, :, 28:50].expand(3, -1, -1, -1).contiguous()
        assert torch.equal(batch.step_clip(xb)[2:3], m.forward_clip(x[:, :, 28:50]))
        for t in range(50, 54):
            yb = batch.step(x[:, :, t:t + 1].expand(3, -1, -1, -1).contiguous())
            assert_close(yb[2:3], m(x[:, :, t:t + 1]), TOL_CO, f"co forward vs step, frame {t}")
        # the reverse: slot 0 of the batch, 26 frames behind slot 2, into the model
        m.import_state(batch.export_state([0]))
        xb = x[:, :, 54:76].expand(3, -1, -1, -1).contiguous()
        assert torch.equal(m.forward_clip(x[:, :, 54:76]), batch.step_clip(xb)[0:1])
        for t in range(76, 80):
            yb = batch.step(x[:, :, t:t + 1].expand(3, -1, -1, -1).contiguous())
            assert_close(m(x[:, :, t:t + 1]), yb[0:1], TOL_CO, f"co forward after import vs step, frame {t}")
        with pytest.raises(RuntimeError, match="one stream"):
            m.import_state(batch.export_state([0, 1]))
    torch.cuda.synchronize()


@pytest.mark.parametrize("one_launch", [True, False])
def test_single_and_batch_rt(P, one_launch):
    """The online Model.forward (the one-launch route and the per-layer route) against the fp32 batch: two fp32
    routes, held to the project's bar between them (test_gpu_rt_streams.py: 1e-4)."""
    net = "v25_k9_p3"
    m, _, _ = model(P, "rt", net)
    x = frames(net, 1, 90, 6)
    routing = P.routing.ROUTING
    prev = routing.rt_one_launch
    try:
        routing.rt_one_launch = one_launch
        with torch.no_grad():
            m.reset_state()
            for t in range(23):
                m(x[:, :, t:t + 1])
            pack = getattr(m, "_frame_pack", None)
            assert pack is not None or not one_launch
            snap = m.export_state()
            assert snap.n == 1 and snap.kind == "rt"
            batch = m.stream_batch(3)
            batch.import_state(snap, [1])
            xb = x[:, :, 23:45].expand(3, -1, -1, -1).contiguous()
            yb = batch.step_clip(xb)[1:2]
            ym = torch.cat([m(x[:, :, t:t + 1]) for t in range(23, 45)], dim=2)
            assert_close(yb, ym, TOL_ROUTES, "rt forward vs batch after export")
            # the reverse: slot 2 (22 frames behind) into the model; the frame descriptor stays the one it was
            m.import_state(batch.export_state([2]))
            ym = torch.cat([m(x[:, :, t:t + 1]) for t in range(45, 67)], dim=2)
            assert getattr(m, "_frame_pack", None) is pack
            yb = batch.step_clip(x[:, :, 45:67].expand(3, -1, -1, -1).contiguous())[2:3]
            assert_close(ym, yb, TOL_ROUTES, "rt forward after import vs batch")
            fresh = m.stream_batch(1).step_clip(x[:, :, 45:50])  # while the FIFOs still hold the moved history
            assert (fresh - yb[:, :, :5]).abs().max().item() > 10 * TOL_ROUTES * yb.abs().max().item()
    finally:
        routing.rt_one_launch = prev
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. cross-dtype
def test_cross_dtype_co(P):
    """An fp32 snapshot continued in a bf16 batch for one ring length stays within twice the error an all-bf16 run of
    the same frames shows against the uninterrupted fp32 stream; a bf16 snapshot passes through an fp32 batch exactly."""
    net = "v25_k9_p3"
    b32, b16, bx = batch_of(P, "co_fp32", net, 1), batch_of(P, "co_bf16", net, 1), batch_of(P, "co_bf16", net, 2)
    ring = max(slot_counts(b32))
    k = 2 * ring + 3
    x = frames(net, 1, k + ring, 7)
    b32.step_clip(x[:, :, :k])
    b16.step_clip(x[:, :, :k])
    snap32 = b32.export_state()
    bx.import_state(snap32, [1])
    rounded = bx.export_state([1]).data
    assert torch.equal(rounded[:, snap32.layout[0][4]:snap32.layout[1][3]],      # the fp32 residual ring: as it was
                       snap32.data[:, snap32.layout[0][4]:snap32.layout[1][3]])
    n0 = snap32.layout[0][4]
    assert torch.equal(rounded[:, :n0], snap32.data[:, :n0].to(torch.bfloat16).float())  # the ring: nearest even
    tail = x[:, :, k:]
    y32 = b32.step_clip(tail)
    y16 = b16.step_clip(tail)
    yx = bx.step_clip(tail.expand(2, -1, -1, -1).contiguous())[1:2]
    torch.cuda.synchronize()
    err_x, err_16 = (yx - y32).abs().max().item(), (y16 - y32).abs().max().item()
    print(f"[cross-dtype] fp32 snapshot in bf16: {err_x:.3e}; all-bf16: {err_16:.3e}", flush=True)
    assert err_16 > 0 and err_x <= 2 * err_16
    snap16 = b16.export_state()
    back = batch_of(P, "co_fp32", net, 3)
    back.import_state(snap16, [1])
    assert torch.equal(back.export_state([1]).data, snap16.data)


# ------------------------------------------------------------------------------------------------ 7. capture
@pytest.mark.parametrize("fam", ["rt_fp32", "co_bf16"])
def test_device_slots_and_capture(P, fam):
    """export_state and import_state with int32 device slot tensors, captured once (one stream of work, no parallel
    branches) and replayed with other slots: the same snapshot and the same state as the eager calls."""
    net = "v5_k9_p3"
    src, _ = advanced(P, fam, net)
    dst_g, dst_e = batch_of(P, fam, net, 4), batch_of(P, fam, net, 4)
    for d in (dst_g, dst_e):
        d.step_clip(frames(net, 4, 6, 8))
    s_out, s_in = i32([1, 3]), i32([0, 2])
    dst_g.import_state(src.export_state(s_out), s_in)  # warm-up: nothing left to build inside the capture
    dst_e.import_state(src.export_state(s_out), s_in)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph):
            snap_g = src.export_state(s_out)
            dst_g.import_state(snap_g, s_in)
    torch.cuda.current_stream().wait_stream(side)
    for out_slots, in_slots in (([1, 3], [0, 2]), ([2, 0], [3, 1]), ([4, 4], [1, 0])):
        s_out.copy_(i32(out_slots))
        s_in.copy_(i32(in_slots))
        graph.replay()
        snap_e = src.export_state(out_slots)
        dst_e.import_state(snap_e, in_slots)
        torch.cuda.synchronize()
        assert torch.equal(snap_g.data, snap_e.data), (out_slots, in_slots)
        assert same(state_clone(dst_g), state_clone(dst_e)), (out_slots, in_slots)
    x = frames(net, 4, 2 * max(slot_counts(src)), 9)
    assert torch.equal(cont(dst_g, x), cont(dst_e, x))


# ------------------------------------------------------------------------------------------------ 8. slots out of range
@pytest.mark.parametrize("fam", ["rt_bf16", "co_fp32"])
def test_out_of_range_slots(P, fam):
    """A device slot tensor holding B and -1 beside valid slots: import leaves every state tensor as it was except the
    valid slots, export leaves the rows of the other entries zero, and nothing else is written."""
    net = "v25_k3_p1"
    src, _ = advanced(P, fam, net)
    snap = src.export_state(i32([2, 5, -1, 4]))
    want = src.export_state([2, 4])
    torch.cuda.synchronize()
    assert torch.equal(snap.data[[0, 3]], want.data) and not snap.data[[1, 2]].any()
    dst = batch_of(P, fam, net, 3)
    dst.step_clip(frames(net, 3, 9, 10), None, [9, 4, 7])
    before = state_clone(dst)
    filler = torch.full_like(snap.data, 123.0)
    filler[0], filler[3] = want.data[0], want.data[1]
    dst.import_state(P.StreamSnapshot(snap.kind, snap.V, snap.layout, filler), i32([1, 3, -1, 2]))
    torch.cuda.synchronize()
    after = state_clone(dst)
    for t, u in zip(before, after):
        assert torch.equal(t[0], u[0])                                        # not named: untouched
    assert torch.equal(dst.export_state([1, 2]).data, want.data)             # rows 0 and 3 arrived, nothing of 1 and 2
    only = batch_of(P, fam, net, 3)
    only.step_clip(frames(net, 3, 9, 10), None, [9, 4, 7])
    only.import_state(want, [1, 2])
    assert same(state_clone(only), after)
