"""co-st-gcn stream-batch clips without a GPU: the schedule restatement (costreams_clip_ref.run_schedule) pinned to the
frame-by-frame one per stream, planted slips that the test inputs must expose, and the host side of
stgcn_co_streams_clip*: descriptor layout, exported symbols, refusals, the split rule, step_clip's own refusals."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from costgcn_ref import costgcn_stream, randomise  # noqa: E402
from costreams_clip_ref import run_schedule  # noqa: E402
from test_coclip_ref_cpu import _arch  # noqa: E402
from test_cpu_host import _c_layout  # noqa: E402

FAKE = 64  # a non-null pointer the host never dereferences
TOL = 1e-3  # the GPU tests' bar: a planted slip has to move the output by more than 10 x this

# three calls of 7 frames over B = 3: stream 1 is one frame short in the first call and restarts in the third, stream 2
# is skipped in the second, stream 0 is short in the third
SCHEDULE = (((2, 2, 2), (7, 6, 7)), ((1, 1, 0), (7, 7, 9)), ((1, 2, 1), (3, 7, -1)))


@pytest.fixture(scope="module")
def case(pkg):
    arch = _arch(pkg, 9, (8, 8, 16), (8, 16, 16), (1, 2, 1))
    torch.manual_seed(51)
    m = pkg.MODELS["co-st-gcn"](rank=None, **arch)
    sd = randomise(m.state_dict(), torch.Generator().manual_seed(52))
    x = torch.randn(3, 3, 21, 25, generator=torch.Generator().manual_seed(53), dtype=torch.float64)
    calls = [(x[:, :, 7 * j:7 * j + 7], codes, lengths) for j, (codes, lengths) in enumerate(SCHEDULE)]
    with torch.no_grad():
        outs, states, segments = run_schedule(calls, sd, arch, sd["A"], dtype=torch.float64)
    return dict(arch=arch, sd=sd, x=x, calls=calls, outs=outs, states=states, segments=segments)


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def test_schedule_equals_stream_per_stream(case):
    """Every run of a stream, from the start or from a restart, is costgcn_stream over the frames it consumed."""
    sd, arch = case["sd"], case["arch"]
    assert [len(s) for s in case["segments"]] == [1, 2, 1]
    consumed = [[f.shape[2] for f, _ in s] for s in case["segments"]]
    assert consumed == [[7 + 7 + 3], [6 + 7, 7], [7]]   # stream 2: skipped, then lengths -1 -> nothing
    with torch.no_grad():
        for s in case["segments"]:
            for frames, cols in s:
                assert _rel(cols, costgcn_stream(frames, sd, arch, sd["A"], dtype=torch.float64)) <= 1e-12
    # zero columns: beyond the length, and every column of a skipped stream
    o0, o1, o2 = case["outs"]
    assert not o0[1, :, 6:].any() and o0[1, :, :6].any()
    assert not o1[2].any() and not o2[2].any() and not o2[0, :, 3:].any()


def test_schedule_chunking_and_state(case):
    """The same frames per stream in other calls (T = 21 with the total lengths, and one frame per call) leave the same
    state and the same consumed columns."""
    sd, arch, x = case["sd"], case["arch"], case["x"]
    with torch.no_grad():
        # stream 0 takes 17 frames, stream 2 takes 7; stream 1's restart needs a call of its own, so it stays out
        outs, states, _ = run_schedule([(x, (1, 0, 1), (17, 0, 7))], sd, arch, sd["A"], dtype=torch.float64)
        x0 = torch.cat((x[0:1, :, :14], x[0:1, :, 14:17]), dim=2)
        assert _rel(outs[0][0:1, :, :17], costgcn_stream(x0, sd, arch, sd["A"], dtype=torch.float64)) <= 1e-12
    for b in (0, 2):
        for (f, r), (f1, r1) in zip(states[b], case["states"][b]):
            assert _rel(f, f1) <= 1e-12 and (r - r1).abs().max().item() <= 1e-12 * max(1.0, r1.abs().max().item())


@pytest.mark.parametrize("slip", ["restart", "length", "advance"])
def test_planted_slips_show(case, slip):
    with torch.no_grad():
        outs, _, _ = run_schedule(case["calls"], case["sd"], case["arch"], case["sd"]["A"], dtype=torch.float64, slip=slip)
    assert _rel(torch.cat(outs, dim=2), torch.cat(case["outs"], dim=2)) > 10 * TOL, slip


# ------------------------------------------------------------------------------------------------ the C ABI
def make_desc(L, B=3, T=8, t0=0, V=25, C0=8, layers=((8, 8, 9, 1, 1),), dtype=0):
    """Every pointer and shape valid; layers: (Cin, Cout, Kt, S, res_mode)."""
    d = L.CoStreamsClipDesc(B=B, T=T, t0=t0, V=V, L=len(layers), C0=C0, K=4, dtype=dtype, x_stride=T * V,
                            x_bstride=3 * T * V, out_bstride=T * 4, x=FAKE, active=FAKE, lengths=FAKE, ln_w=FAKE,
                            ln_b=FAKE, w_in=FAKE, b_in=FAKE, w_out=FAKE, b_out=FAKE, h0=FAKE, out=FAKE)
    for i, (cin, cout, kt, s, res) in enumerate(layers):
        y = d.layers[i]
        y.Cin, y.Cout, y.P, y.Kt, y.S, y.res_mode = cin, cout, 3, kt, s, res
        for f, t in L.CoStreamsClipLayer._fields_:
            if t is L.c_void_p:
                setattr(y, f, FAKE)
    return d


def test_descriptor_layout(pkg, tmp_path):
    L = pkg._lib
    got, expect = _c_layout(tmp_path, {"stgcn_co_streams_clip_layer": L.CoStreamsClipLayer,
                                       "stgcn_co_streams_clip_desc": L.CoStreamsClipDesc})
    assert got == expect


def test_symbols_exported(pkg):
    lib = pkg._lib.load_library()
    for name in ("stgcn_co_streams_clip_splits", "stgcn_co_streams_clip_workspace", "stgcn_co_streams_clip"):
        assert hasattr(lib, name) and name in pkg._lib.EXPORTS
    assert lib.stgcn_abi_version() == 7


def test_refuses_bad_descriptors(pkg):
    L = pkg._lib
    lib = L.load_library()
    assert lib.stgcn_co_streams_clip(None, None) == 1
    assert lib.stgcn_co_streams_clip_splits(None, 0) == -1 and lib.stgcn_co_streams_clip_workspace(None, 0) == -1
    assert lib.stgcn_co_streams_clip(L.CoStreamsClipDesc(), None) == 1
    good = make_desc(L)
    assert lib.stgcn_co_streams_clip_splits(good, 0) >= 1 and lib.stgcn_co_streams_clip_workspace(good, 0) > 0
    assert lib.stgcn_co_streams_clip_splits(good, 1) == -1 and lib.stgcn_co_streams_clip_splits(good, -1) == -1

    def refused(d, code=1):
        assert lib.stgcn_co_streams_clip(d, None) == code
        assert lib.stgcn_co_streams_clip_splits(d, 0) == -1 and lib.stgcn_co_streams_clip_workspace(d, 0) == -1

    refused(make_desc(L, B=0))
    refused(make_desc(L, T=0))
    refused(make_desc(L, T=L.CO_CLIP_MAX_T + 1))
    refused(make_desc(L, t0=-1))
    refused(make_desc(L, V=33))
    refused(make_desc(L, V=1))
    refused(make_desc(L, C0=6, layers=((6, 6, 9, 1, 1),)))        # C % 4 != 0
    refused(make_desc(L, layers=((8, 8, 8, 1, 1),)))              # even Kt
    refused(make_desc(L, layers=((8, 8, 71, 1, 1),)))
    refused(make_desc(L, layers=((8, 8, 9, 3, 1),)))              # stride 3
    refused(make_desc(L, layers=((8, 260, 9, 1, 2),)))
    refused(make_desc(L, layers=((8, 16, 9, 1, 1),)))             # identity residual needs Cin == Cout
    refused(make_desc(L, layers=((8, 8, 9, 1, 3),)))              # residual code
    refused(make_desc(L, layers=((8, 8, 9, 1, 1), (16, 16, 9, 1, 1))))  # Cin != the previous Cout
    refused(make_desc(L, dtype=2), code=2)
    d = make_desc(L)
    d.L = 13
    refused(d)
    d = make_desc(L)
    d.layers[0].P = 4
    refused(d)
    # shapes fine, a required pointer missing: the queries answer, the launch entry refuses
    for field in ("x", "active", "lengths", "ln_w", "ln_b", "w_in", "b_in", "w_out", "h0", "out"):
        d = make_desc(L)
        setattr(d, field, None)
        assert lib.stgcn_co_streams_clip(d, None) == 1, field
        assert lib.stgcn_co_streams_clip_splits(d, 0) >= 1
    for field in ("A", "wp", "ln1_w", "ln1_b", "ln2_w", "ln2_b", "wt", "ring", "res_ring", "idx", "z_buf", "hist", "resq",
                  "partial", "y"):
        d = make_desc(L)
        setattr(d.layers[0], field, None)
        assert lib.stgcn_co_streams_clip(d, None) == 1, field
    for field in ("wrp", "lnr_w", "lnr_b", "r_buf"):
        d = make_desc(L, layers=((8, 16, 9, 2, 2),))
        setattr(d.layers[0], field, None)
        assert lib.stgcn_co_streams_clip(d, None) == 1, field
    for field, value in (("x_stride", 8 * 25 - 1), ("x_bstride", 3 * 8 * 25 - 1), ("out_bstride", 8 * 4 - 1)):
        d = make_desc(L)
        setattr(d, field, value)  # channels, streams of x or streams of out would overlap
        assert lib.stgcn_co_streams_clip(d, None) == 1, field


def test_splits_follow_the_shape_alone(pkg):
    """The split count, and so the order of a frame's sums, is the same for every B, T and t0 and is stgcn_co_clip's
    and stgcn_co_streams'; the workspace grows with B * T only."""
    L = pkg._lib
    lib = L.load_library()
    for layer in ((256, 256, 69, 1, 1), (64, 64, 9, 1, 1), (64, 128, 69, 2, 2), (8, 8, 9, 1, 1)):
        counts = set()
        for B, T, t0 in ((1, 1, 0), (3, 5, 0), (3, 5, 40), (64, 64, 0), (1000, 256, 512)):
            d = make_desc(L, B=B, T=T, t0=t0, C0=layer[0], layers=(layer,))
            n = lib.stgcn_co_streams_clip_splits(d, 0)
            counts.add(n)
            assert lib.stgcn_co_streams_clip_workspace(d, 0) == B * T * n * 25 * layer[1] * 4
        assert len(counts) == 1
        c = L.CoClipDesc(T=8, V=25, L=1, C0=layer[0], K=4)
        s = L.CoStreamsDesc(B=3, V=25, L=1, C0=layer[0], K=4)
        for y in (c.layers[0], s.layers[0]):
            y.Cin, y.Cout, y.P, y.Kt, y.S, y.res_mode = layer[0], layer[1], 3, layer[2], layer[3], layer[4]
        assert counts == {lib.stgcn_co_clip_splits(c, 0)} == {lib.stgcn_co_streams_splits(s, 0)}
    d = make_desc(L, C0=256, layers=((256, 256, 69, 1, 1),))
    d.layers[0].splits = 7
    assert lib.stgcn_co_streams_clip_splits(d, 0) == 7


def test_step_clip_refuses_on_the_host(pkg):
    """The shape checks come before anything touches a device.  A batch cannot be constructed without one, so the
    checks run on a bare instance with the attributes they read."""
    from importlib import import_module
    cls = import_module(pkg.__name__ + ".costgcn").CoStreamBatch
    batch = object.__new__(cls)
    batch.B, batch.V, batch.clip_frames = 2, 25, 1024
    for shape in ((3, 4, 25), (2, 3, 4, 25, 1), (3, 3, 4, 25), (2, 3, 4, 24), (2, 2, 4, 25), (2, 3, 0, 25)):
        with pytest.raises(RuntimeError, match="step_clip expects x"):
            batch.step_clip(torch.zeros(*shape))
    x = torch.zeros(2, 3, 4, 25)
    with pytest.raises(RuntimeError, match="expects active"):
        batch.step_clip(x, active=[1, 1, 1])
    with pytest.raises(RuntimeError, match="expects active"):
        batch.step_clip(x, active=torch.ones(2, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="expects lengths"):
        batch.step_clip(x, lengths=torch.ones(3, dtype=torch.int32))
    batch.clip_frames = 0
    with pytest.raises(RuntimeError, match="clip_frames"):
        batch.step_clip(x)
    batch.clip_frames = 1024
    with pytest.raises(RuntimeError, match="HIP device only"):  # a CPU tensor: no fallback
        batch.step_clip(x)
    # the chunk: B * chunk <= clip_frames, a power of two, at most STGCN_CO_CLIP_MAX_T
    for B, frames, chunk in ((2, 1024, 256), (5, 1024, 128), (5, 8, 1), (64, 1024, 16), (41, 1024, 16), (3000, 1024, 1)):
        batch.B, batch.clip_frames = B, frames
        assert batch._clip_chunk() == chunk
