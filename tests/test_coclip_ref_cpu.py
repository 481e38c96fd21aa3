"""co-st-gcn clips without a GPU: the whole-clip restatement (coclip_ref.costgcn_clip) against the frame-by-frame one
under several chunkings, planted slips that the test inputs must expose, forward_clip's host refusals, and host-side
argument validation and descriptor layout of the stgcn_co_clip* entry points."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coclip_ref import costgcn_clip  # noqa: E402
from costgcn_ref import costgcn_stream, randomise  # noqa: E402
from test_cpu_host import _c_layout  # noqa: E402

FAKE = 64  # a non-null pointer the host never dereferences
TOL = 1e-3  # the GPU tests' bar: a planted slip has to move the output by more than 10 x this


def _arch(P, kernel, in_ch, out_ch, stride):
    nl = len(in_ch)
    return {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": 7, "graph": P.PKU_MMD,
            "st-gcn": {"importance": True, "in_feat": 3, "stages": 1, "layers": nl, "kernel": kernel,
                       "in_ch": list(in_ch), "out_ch": list(out_ch), "stride": list(stride), "dilation": [1] * nl,
                       "residual": [1] * nl, "dropout": [0.0] * nl}}


MODELS = {"small": dict(kernel=9, in_ch=(8, 8, 16), out_ch=(8, 16, 16), stride=(1, 2, 1), seed=51, frames=40),
          "k69": dict(kernel=69, in_ch=(8,), out_ch=(8,), stride=(1,), seed=61, frames=140)}


@pytest.fixture(scope="module", params=sorted(MODELS))
def case(pkg, request):
    """Model, fp64 input and the frame-by-frame restatement from an empty state, computed once."""
    c = MODELS[request.param]
    arch = _arch(pkg, c["kernel"], c["in_ch"], c["out_ch"], c["stride"])
    torch.manual_seed(c["seed"])
    m = pkg.MODELS["co-st-gcn"](rank=None, **arch)
    sd = randomise(m.state_dict(), torch.Generator().manual_seed(c["seed"] + 1))
    x = torch.randn(1, 3, c["frames"], 25, generator=torch.Generator().manual_seed(c["seed"] + 2), dtype=torch.float64)
    with torch.no_grad():
        ref = costgcn_stream(x, sd, arch, sd["A"], dtype=torch.float64)
    fifo = max(c["stride"]) * (c["kernel"] - 1) + 1
    return dict(arch=arch, sd=sd, x=x, ref=ref, fifo=fifo)


def _chunked(case, chunks, **kw):
    x, state, ys, t0 = case["x"], None, [], 0
    with torch.no_grad():
        for n in chunks:
            y, state = costgcn_clip(x[:, :, t0:t0 + n], case["sd"], case["arch"], case["sd"]["A"], state=state,
                                    dtype=torch.float64, **kw)
            ys.append(y)
            t0 += n
    return torch.cat(ys, dim=2), state


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def test_clip_equals_stream(case):
    F_, fifo = case["x"].shape[2], case["fifo"]
    y, state = _chunked(case, (F_,))
    assert y.shape == case["ref"].shape
    assert _rel(y, case["ref"]) <= 1e-12
    for chunks in ((1,) * F_, (5, 7, 12), (fifo - 1, 1, fifo + 1)):
        n = sum(chunks)
        assert n <= F_
        yc, sc = _chunked(case, chunks)
        assert _rel(yc, case["ref"][:, :, :n]) <= 1e-12, chunks
    # the state after the whole clip is the state after the frames one at a time
    y1, s1 = _chunked(case, (1,) * F_)
    for (f, r), (f1, r1) in zip(state, s1):
        assert f.shape == f1.shape and r.shape == r1.shape
        assert _rel(f, f1) <= 1e-12 and (r - r1).abs().max().item() <= 1e-12 * max(1.0, r1.abs().max().item())


@pytest.mark.parametrize("slip", ["delay+1", "delay-1", "taps", "dilation", "dropped"])
def test_planted_slips_show(case, slip):
    """Each slip moves the output by more than 10 x the GPU tests' tolerance on these inputs.  The chunks reach past the
    FIFO length: at Kt = 69 the residual delay (34 frames) shows only from frame 34 on."""
    chunks = (case["fifo"] - 1, 1, case["fifo"] + 1)
    n = sum(chunks)
    ref = case["ref"][:, :, :n]
    if slip == "dilation" and max(case["arch"]["st-gcn"]["stride"]) == 1:  # nothing to get wrong without a stride-2 layer
        assert _rel(_chunked(case, chunks, slip=slip)[0], ref) <= 1e-12
        return
    if slip == "dropped":  # every chunk from an empty state: the carried state ignored
        with torch.no_grad():
            ys, t0 = [], 0
            for c in chunks:
                ys.append(costgcn_clip(case["x"][:, :, t0:t0 + c], case["sd"], case["arch"], case["sd"]["A"],
                                       dtype=torch.float64)[0])
                t0 += c
        y = torch.cat(ys, dim=2)
    else:
        y, _ = _chunked(case, chunks, slip=slip)
    assert _rel(y, ref) > 10 * TOL, slip


def test_forward_clip_refuses_on_the_host(pkg):
    m = pkg.MODELS["co-st-gcn"](rank=None, **_arch(pkg, 9, (8, 8, 16), (8, 16, 16), (1, 2, 1)))
    assert m.clip_chunk == 256
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_clip(torch.zeros(1, 3, 4, 25))
    with torch.no_grad():
        for shape in ((3, 4, 25), (1, 3, 4, 25, 1), (2, 3, 4, 25), (1, 3, 4, 24), (1, 2, 4, 25), (1, 3, 0, 25)):
            with pytest.raises(RuntimeError, match="clip of batch 1"):
                m.forward_clip(torch.zeros(*shape))
        m.clip_chunk = 257
        with pytest.raises(RuntimeError, match="clip_chunk"):
            m.forward_clip(torch.zeros(1, 3, 4, 25))
        m.clip_chunk = 256
        with pytest.raises(RuntimeError, match="HIP device only"):  # a CPU tensor: no fallback
            m.forward_clip(torch.zeros(1, 3, 4, 25))
    with torch.no_grad(), pytest.raises(RuntimeError, match="one frame"):  # forward keeps refusing clips
        m(torch.zeros(1, 3, 4, 25))


def make_desc(L, T=8, V=25, C0=8, layers=((8, 8, 9, 1, 1),), dtype=0):
    """Every pointer and shape valid; layers: (Cin, Cout, Kt, S, res_mode)."""
    d = L.CoClipDesc(T=T, V=V, L=len(layers), C0=C0, K=4, dtype=dtype, x_stride=T * V, x=FAKE, ln_w=FAKE, ln_b=FAKE,
                     w_in=FAKE, b_in=FAKE, w_out=FAKE, b_out=FAKE, h0=FAKE, out=FAKE)
    for i, (cin, cout, kt, s, res) in enumerate(layers):
        y = d.layers[i]
        y.Cin, y.Cout, y.P, y.Kt, y.S, y.res_mode = cin, cout, 3, kt, s, res
        for f, t in L.CoClipLayer._fields_:
            if t is L.c_void_p:
                setattr(y, f, FAKE)
    return d


def test_co_clip_descriptor_layout(pkg, tmp_path):
    L = pkg._lib
    got, expect = _c_layout(tmp_path, {"stgcn_co_clip_layer": L.CoClipLayer, "stgcn_co_clip_desc": L.CoClipDesc})
    assert got == expect


def test_co_clip_symbols_exported(pkg):
    lib = pkg._lib.load_library()
    for name in ("stgcn_co_clip_splits", "stgcn_co_clip_workspace", "stgcn_co_clip"):
        assert hasattr(lib, name) and name in pkg._lib.EXPORTS
    assert lib.stgcn_abi_version() == 7


def test_co_clip_refuses_bad_descriptors(pkg):
    L = pkg._lib
    lib = L.load_library()
    assert lib.stgcn_co_clip(None, None) == 1
    assert lib.stgcn_co_clip_splits(None, 0) == -1 and lib.stgcn_co_clip_workspace(None, 0) == -1
    assert lib.stgcn_co_clip(L.CoClipDesc(), None) == 1

    def refused(d, code=1):
        assert lib.stgcn_co_clip(d, None) == code
        assert lib.stgcn_co_clip_splits(d, 0) == -1 and lib.stgcn_co_clip_workspace(d, 0) == -1

    refused(make_desc(L, T=0))
    refused(make_desc(L, T=L.CO_CLIP_MAX_T + 1))
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
    # shapes fine, a required pointer missing: refused by the launch entry only
    for field in ("x", "ln_w", "w_in", "w_out", "h0", "out"):
        d = make_desc(L)
        setattr(d, field, None)
        assert lib.stgcn_co_clip(d, None) == 1
    for field in ("A", "wp", "ln1_w", "ln2_b", "wt", "ring", "res_ring", "idx", "z_buf", "hist", "resq", "partial", "y"):
        d = make_desc(L)
        setattr(d.layers[0], field, None)
        assert lib.stgcn_co_clip(d, None) == 1
    d = make_desc(L, layers=((8, 16, 9, 2, 2),))
    d.layers[0].wrp = None
    assert lib.stgcn_co_clip(d, None) == 1
    d = make_desc(L)
    d.x_stride = 8 * 25 - 1  # channels of x would overlap
    assert lib.stgcn_co_clip(d, None) == 1


def test_co_clip_splits_follow_the_shape_alone(pkg):
    """The split count and so the order of a frame's sums: the same for every T, co_streams' rule; the workspace grows
    with T only."""
    L = pkg._lib
    lib = L.load_library()
    for layer in ((256, 256, 69, 1, 1), (64, 64, 9, 1, 1), (64, 128, 69, 2, 2)):
        counts = set()
        for T in (1, 5, 64, 256):
            d = make_desc(L, T=T, C0=layer[0], layers=(layer,))
            n = lib.stgcn_co_clip_splits(d, 0)
            counts.add(n)
            assert lib.stgcn_co_clip_workspace(d, 0) == T * n * 25 * layer[1] * 4
        assert len(counts) == 1
        s = L.CoStreamsDesc(B=3, V=25, L=1, C0=layer[0], K=4)
        y = s.layers[0]
        y.Cin, y.Cout, y.P, y.Kt, y.S, y.res_mode = layer[0], layer[1], 3, layer[2], layer[3], layer[4]
        assert counts == {lib.stgcn_co_streams_splits(s, 0)}
    d = make_desc(L, C0=256, layers=((256, 256, 69, 1, 1),))
    d.layers[0].splits = 7
    assert lib.stgcn_co_clip_splits(d, 0) == 7
    assert lib.stgcn_co_clip_splits(d, 1) == -1 and lib.stgcn_co_clip_splits(d, -1) == -1
