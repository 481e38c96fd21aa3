"""rt-st-gcn stream-batch clips without a GPU: the schedule restatement (rt_streams_clip_ref.run_schedule) pinned to
oracle.rt_model_online per stream, planted slips that the test inputs must expose, and the host side of
stgcn_rt_streams_clip: descriptor layout, exported symbol, refusals, step_clip's own refusals and the chunk rule.

The networks of the GPU tests (tests/test_gpu_rt_streams_clip.py) live here so that both files use the same ones."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub  # noqa: E402
from oracle import stgcn_oracle as O  # noqa: E402
from rt_streams_clip_ref import run_schedule  # noqa: E402
from test_cpu_host import _c_layout  # noqa: E402
from test_rt_streams_bf16_cpu import _default_dtype, _randomise, _small_arch  # noqa: E402

FAKE = 64  # a non-null pointer the host never dereferences
TOL = 1e-3  # the GPU tests' bar against the oracle: a planted slip has to move the output by more than 10 x this

# three calls of 7 frames over B = 3: stream 1 is one frame short in the first call and restarts in the third, stream 2
# is skipped in the second, stream 0 is short in the third
SCHEDULE = (((2, 2, 2), (7, 6, 7)), ((1, 1, 0), (7, 7, 9)), ((1, 2, 1), (3, 7, -1)))


def small_net(P, V, nparts, seed=900):
    """(arch, sd) of the random network 4 -> 8 -> 8 -> 16: Kt = 9, an identity residual, a layer without one and a
    stride-2 layer with a residual conv (17-slot FIFO, two accumulators)."""
    arch = _small_arch(P, V, nparts)
    arch["kernel"] = 9
    arch["rt-st-gcn"].update(kernel=9, in_ch=[4, 8, 8], out_ch=[8, 8, 16], stride=[1, 1, 2], residual=[1, 1, 1])
    torch.manual_seed(seed + V + nparts)
    sd = _randomise(P.MODELS["rt-st-gcn"](rank=None, **arch), seed + 50 + V + nparts)
    if sd["A"].shape[0] == 1:  # a dense single partition instead of the hop-0 diagonal
        sd["A"] = sd["A"] + 0.3 * torch.rand(sd["A"].shape, generator=torch.Generator().manual_seed(seed + 70))
    return arch, sd


def _case(P, name):
    if name.startswith("rt_"):
        d = load_golden(name)
        arch, sd = d["arch"], sub(d, "sd/")
        x = torch.stack([d["x"][0, :, o:o + 21] for o in (0, 4, 8)]).double()
    else:
        _, v, p = name.split("_")
        arch, sd = small_net(P, int(v[1:]), int(p[1:]))
        x = torch.randn(3, 3, 21, int(v[1:]), generator=torch.Generator().manual_seed(53), dtype=torch.float64)
    calls = [(x[:, :, 7 * j:7 * j + 7], codes, lengths) for j, (codes, lengths) in enumerate(SCHEDULE)]
    return arch, sd, x, calls


def _online64(frames, sd, arch):
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad(), _default_dtype(torch.float64):
        return O.rt_model_online(frames.double(), sd64, arch)


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


CASES = ["rt_stride1", "rt_ref_strides", "net_v25_p3", "net_v2_p1", "net_v25_p1", "net_v2_p3"]


@pytest.fixture(scope="module")
def runs(pkg):
    out = {}
    for name in CASES:
        arch, sd, x, calls = _case(pkg, name)
        out[name] = (arch, sd, x, calls) + run_schedule(calls, sd, arch)
    return out


@pytest.mark.parametrize("name", CASES)
def test_schedule_equals_online_per_stream(runs, name):
    """Every run of a stream, from the start or from a restart, is rt_model_online over the frames it consumed."""
    arch, sd, x, calls, outs, states, segments = runs[name]
    assert [len(s) for s in segments] == [1, 2, 1]
    assert [[f.shape[2] for f, _ in s] for s in segments] == [[17], [13, 7], [7]]
    for s in segments:
        for frames, cols in s:
            assert _rel(cols, _online64(frames, sd, arch)) <= 1e-12
    o0, o1, o2 = outs
    assert not o0[1, :, 6:].any() and o0[1, :, :6].any()
    assert not o1[2].any() and not o2[2].any() and not o2[0, :, 3:].any()


@pytest.mark.parametrize("name", ["rt_ref_strides", "net_v25_p3"])
def test_schedule_chunking_and_state(runs, name):
    """The same frames per stream in one call of T = 21 with the total lengths leave the same state and columns."""
    arch, sd, x, calls, outs, states, _ = runs[name]
    one, st1, _ = run_schedule([(x, (1, 0, 1), (17, 0, 7))], sd, arch)
    assert _rel(one[0][0:1, :, :17], _online64(x[0:1, :, :17], sd, arch)) <= 1e-12
    for b in (0, 2):
        for l, l1 in zip(states[b], st1[b]):
            assert (l["fi"], l["ai"]) == (l1["fi"], l1["ai"])
            for k in ("fifo", "acc"):
                assert (l[k] - l1[k]).abs().max().item() <= 1e-12 * max(1.0, l1[k].abs().max().item())
    # the indices are the consumed frames modulo the ring sizes
    conf = arch["rt-st-gcn"]
    for b, n in ((0, 17), (1, 7), (2, 7)):
        for i, l in enumerate(states[b]):
            S = conf["stride"][i]
            assert (l["fi"], l["ai"]) == (n % (S * (conf["kernel"] - 1) + 1), n % S)


@pytest.mark.parametrize("slip", ["restart", "length", "advance"])
def test_planted_slips_show(runs, slip):
    arch, sd, x, calls, outs, _, _ = runs["net_v25_p3"]
    bad, _, _ = run_schedule(calls, sd, arch, slip=slip)
    moved = _rel(torch.cat(bad, dim=2), torch.cat(outs, dim=2))
    print(f"[slip] {slip}: {moved:.3e}", flush=True)
    assert moved > 10 * TOL, slip


def test_rounded_restatement_differs_only_by_rounding(runs):
    arch, sd, x, calls, outs, _, _ = runs["net_v25_p3"]
    q, _, _ = run_schedule(calls, sd, arch, round_bf16=True)
    e = _rel(torch.cat(q, dim=2), torch.cat(outs, dim=2))
    assert 2.0 ** -13 < e < 2.0 ** -5, e  # bf16's unit roundoff is 2^-9


# ------------------------------------------------------------------------------------------------ the C ABI
def make_desc(L, B=3, T=8, t0=0, V=25, C0=8, layers=((8, 8, 17, 1, 1),), dtype=0):
    """Every pointer and shape valid; layers: (Cin, Cout, fifo_size, S, res_mode)."""
    d = L.RtStreamsClipDesc(B=B, T=T, t0=t0, V=V, L=len(layers), C0=C0, K=4, dtype=dtype, x_stride=T * V,
                            x_bstride=3 * T * V, out_bstride=T * 4, fstride=V * max([C0] + [y[1] for y in layers]),
                            x=FAKE, active=FAKE, lengths=FAKE, ln_w=FAKE, ln_b=FAKE, w_in=FAKE, b_in=FAKE, w_out=FAKE,
                            b_out=FAKE, xb=FAKE, z=FAKE, r=FAKE, a=FAKE, out=FAKE)
    for i, (cin, cout, fifo, s, res) in enumerate(layers):
        y = d.layers[i]
        y.Cin, y.Cout, y.P, y.fifo_size, y.S, y.res_mode = cin, cout, 3, fifo, s, res
        for f, t in L.RtStreamsLayer._fields_:
            if t is L.c_void_p:
                setattr(y, f, FAKE)
    return d


def test_descriptor_layout(pkg, tmp_path):
    L = pkg._lib
    got, expect = _c_layout(tmp_path, {"stgcn_rt_streams_clip_desc": L.RtStreamsClipDesc,
                                       "stgcn_rt_streams_layer": L.RtStreamsLayer})
    assert got == expect
    assert L.RT_CLIP_MAX_T == 256
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stgcn_amd.h")) as f:
        assert "#define STGCN_RT_CLIP_MAX_T 256" in f.read()


def test_symbol_exported(pkg):
    lib = pkg._lib.load_library()
    assert hasattr(lib, "stgcn_rt_streams_clip") and "stgcn_rt_streams_clip" in pkg._lib.EXPORTS
    assert lib.stgcn_abi_version() == 7


def test_refuses_bad_descriptors(pkg):
    """Every refusal comes before any launch: no device is needed to get it."""
    L = pkg._lib
    lib = L.load_library()
    call = lib.stgcn_rt_streams_clip
    assert call(None, None) == 1
    assert call(L.RtStreamsClipDesc(), None) == 1
    for kw in (dict(B=0), dict(T=0), dict(T=L.RT_CLIP_MAX_T + 1), dict(t0=-1), dict(V=33), dict(V=1),
               dict(B=1 << 24, T=256),                                # B * T beyond a grid
               dict(C0=6, layers=((6, 8, 17, 1, 2),)),                # C % 4 != 0
               dict(C0=260, layers=((260, 8, 17, 1, 2),)),
               dict(layers=((8, 260, 17, 1, 2),)),
               dict(V=32, layers=((8, 256, 17, 1, 2),)),              # V * C > 7680
               dict(layers=((8, 16, 17, 1, 1),)),                     # identity residual needs Cin == Cout
               dict(layers=((8, 8, 17, 1, 3),)),                      # residual code
               dict(layers=((8, 8, 0, 1, 1),)), dict(layers=((8, 8, 17, 0, 1),)),
               dict(layers=((8, 8, 17, 1, 1), (16, 16, 17, 1, 1)))):  # Cin != the previous Cout
        assert call(make_desc(L, **kw), None) == 1, kw
    assert call(make_desc(L, dtype=2), None) == 2
    assert call(make_desc(L, dtype=-1), None) == 2
    d = make_desc(L)
    d.L = 13
    assert call(d, None) == 1
    d = make_desc(L)
    d.layers[0].P = 4
    assert call(d, None) == 1
    for field in ("x", "active", "lengths", "ln_w", "ln_b", "w_in", "b_in", "w_out", "xb", "z", "a", "out"):
        d = make_desc(L)
        setattr(d, field, None)
        assert call(d, None) == 1, field
    for field in ("A", "wp", "ln_w", "ln_b", "fifo", "acc", "idx"):
        d = make_desc(L)
        setattr(d.layers[0], field, None)
        assert call(d, None) == 1, field
    for field in ("wrp", "lnr_w", "lnr_b"):
        d = make_desc(L, layers=((8, 16, 17, 2, 2),))
        setattr(d.layers[0], field, None)
        assert call(d, None) == 1, field
    d = make_desc(L, layers=((8, 16, 17, 2, 2),))
    d.r = None                                                        # a residual conv needs its scratch
    assert call(d, None) == 1
    for field, value in (("x_stride", 8 * 25 - 1), ("x_bstride", 3 * 8 * 25 - 1), ("out_bstride", 8 * 4 - 1),
                         ("fstride", 8 * 25 - 4), ("fstride", 8 * 25 + 2)):
        d = make_desc(L)
        setattr(d, field, value)  # channels, streams or frames would overlap; float4 rows need fstride % 4 == 0
        assert call(d, None) == 1, field


def test_step_clip_refuses_on_the_host(pkg):
    """The shape checks come before anything touches a device.  A batch cannot be constructed without one, so the
    checks run on a bare instance with the attributes they read."""
    from importlib import import_module
    cls = import_module(pkg.__name__ + ".rtstgcn").RtStreamBatch
    batch = object.__new__(cls)
    batch.B, batch.V = 2, 25
    assert batch.clip_frames == 1024
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
    with pytest.raises(RuntimeError, match="expects lengths"):
        batch.step_clip(x, lengths=[4])
    batch.clip_frames = 0
    with pytest.raises(RuntimeError, match="clip_frames"):
        batch.step_clip(x)
    batch.clip_frames = 1024
    with pytest.raises(RuntimeError, match="HIP device only"):  # a CPU tensor: no fallback
        batch.step_clip(x)


def test_chunk_rule(pkg):
    """B * chunk <= clip_frames (one frame at the least), a power of two, at most STGCN_RT_CLIP_MAX_T; the calls tile
    the clip in order, restarts can only fall on the first (t0 = 0), and a call's scratch capacity is the next power of
    two at or above its frames."""
    from importlib import import_module
    cls = import_module(pkg.__name__ + ".rtstgcn").RtStreamBatch
    batch = object.__new__(cls)
    for B, frames, chunk in ((2, 1024, 256), (5, 1024, 128), (5, 8, 1), (64, 1024, 16), (41, 1024, 16), (3000, 1024, 1),
                             (1, 8, 8), (1, 10 ** 6, 256), (256, 1024, 4)):
        batch.B, batch.clip_frames = B, frames
        assert batch._clip_chunk() == chunk
        for T in (1, 2, 3, chunk, chunk + 1, 33, 300):
            calls = batch._clip_calls(T)
            assert [t0 for t0, _, _ in calls] == list(range(0, T, chunk))
            assert sum(n for _, n, _ in calls) == T and all(1 <= n <= chunk for _, n, _ in calls)
            assert all(n == chunk for _, n, _ in calls[:-1])
            for _, n, cap in calls:
                assert n <= cap <= chunk and cap & (cap - 1) == 0 and (cap < 2 * n)
