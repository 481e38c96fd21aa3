"""Stream snapshots without a GPU: the canonical image's restatement (stream_state_ref) and the rotation equivalence it
rests on, pinned on the existing restatements of both stream batches; the host side of StreamSnapshot and of
export_state / import_state (layout table, state_dict, cat, row selection, every refusal); and the C-ABI of
stgcn_stream_state_*: exported symbols, descriptor layout, every refusal before a launch."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_state_ref as R  # noqa: E402
from costgcn_ref import randomise  # noqa: E402
from rt_streams_clip_ref import advance, empty_state  # noqa: E402
from test_coclip_ref_cpu import _arch  # noqa: E402
from test_cpu_host import _c_layout  # noqa: E402
from test_rt_streams_bf16_cpu import _randomise, _small_arch  # noqa: E402

FAKE = 64  # a non-null pointer the host never dereferences


# ------------------------------------------------------------------------------------------------ the restatement
def _random_layers(shapes, V, heads, seed=3):
    g = np.random.default_rng(seed)
    return [(g.standard_normal((n0, V, C)).astype(np.float32), g.standard_normal((n1, V, C)).astype(np.float32), h)
            for (C, n0, n1), h in zip(shapes, heads)]


def test_canonicalise_is_a_rotation():
    shapes, V = [(8, 3, 1), (16, 5, 2)], 5
    layers = _random_layers(shapes, V, [(2, 0), (4, 1)])
    canon = R.canonicalise(layers)
    for (t0, t1, (i0, i1)), (c0, c1, idx) in zip(layers, canon):
        assert idx == (0, 0)
        for k in range(t0.shape[0]):
            assert np.array_equal(c0[k], t0[(i0 + k) % t0.shape[0]])
        for k in range(t1.shape[0]):
            assert np.array_equal(c1[k], t1[(i1 + k) % t1.shape[0]])
    # heads already at 0: unchanged; twice is once
    again = R.canonicalise(canon)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(canon, again))
    # image and back: rotation 0, the same values; a bf16 ring rounds t0 only, to nearest even
    table, E = R.layout(V, shapes)
    row = R.image(layers)
    assert row.shape == (E,) and row.dtype == np.float32
    back = R.from_image(row, V, table)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and b[2] == (0, 0)
               for a, b in zip(canon, back))
    half = R.from_image(row, V, table, bf16_t0=True)
    for (c0, c1, _), (h0, h1, _) in zip(canon, half):
        want = torch.from_numpy(c0).to(torch.bfloat16).float().numpy()
        assert np.array_equal(h0, want) and np.array_equal(h1, c1)


def test_layout_table_by_hand(pkg):
    """Three layers at V = 5: 8 channels with 3 + 1 slots, 16 with 5 + 2, 16 with 3 + 1."""
    S = import_module(pkg.__name__ + ".streams")
    want = ((8, 3, 1, 0, 120), (16, 5, 2, 160, 560), (16, 3, 1, 720, 960))
    table, E = S.state_layout(5, [(8, 3, 1), (16, 5, 2), (16, 3, 1)])
    assert table == want and E == 1040
    assert R.layout(5, [(8, 3, 1), (16, 5, 2), (16, 3, 1)]) == ([tuple(r) for r in want], 1040)
    state = [(torch.zeros(4, n0, 5, C), torch.zeros(4, n1, 5, C), torch.zeros(4, 2, dtype=torch.int32))
             for C, n0, n1 in ((8, 3, 1), (16, 5, 2), (16, 3, 1))]
    assert S.layout_of_state(state) == (5, want, 1040)
    assert S.layout_of_state([tuple(t[0] for t in ts) for ts in state]) == (5, want, 1040)  # a single stream's


# ------------------------------------------------------------------------------------------------ rotation equivalence
@pytest.fixture(scope="module")
def rt_case(pkg):
    arch = _small_arch(pkg, 25, 3)  # kernel 3, strides 1 / 2 / 1: FIFOs of 3, 5 and 3 slots, 1, 2 and 1 accumulators
    torch.manual_seed(11)
    sd = _randomise(pkg.MODELS["rt-st-gcn"](rank=None, **arch), 12)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x = torch.randn(1, 3, 40, 25, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    return arch, sd, x


@pytest.mark.parametrize("k", [0, 7, 15, 30])
def test_rt_rotation_equivalence(rt_case, k):
    """k frames, canonicalise, m more frames from both states: the same bits.  k = 0: never stepped; 7: every head
    wrapped and non-zero (7 % 3, 7 % 5, 7 % 2); 15: every FIFO head at exactly 0 after wrapping, the stride-2
    accumulator at 1; 30: every index 0 after wrapping."""
    arch, sd, x = rt_case
    state = empty_state(arch, 25)
    with torch.no_grad():
        if k:
            advance(x[:, :, :k], sd, arch, state)
        heads = [(s["fi"], s["ai"]) for s in state]
        assert heads == [(k % 3, 0), (k % 5, k % 2), (k % 3, 0)]
        canon = R.rt_from_layers(R.canonicalise(R.rt_to_layers(state)))
        assert all((s["fi"], s["ai"]) == (0, 0) for s in canon)
        a = advance(x[:, :, k:k + 9], sd, arch, state)
        b = advance(x[:, :, k:k + 9], sd, arch, canon)
    assert np.array_equal(a.numpy(), b.numpy())
    # and the states stay rotations of one another: the same image after the m frames
    assert np.array_equal(R.image(R.rt_to_layers(state)), R.image(R.rt_to_layers(canon)))
    if k == 7:  # a rotation the other way round is not equivalent: the inputs tell
        wrong = R.rt_from_layers([(np.roll(t0, i0, axis=0), np.roll(t1, i1, axis=0), (0, 0))
                                  for t0, t1, (i0, i1) in R.rt_to_layers(state)])
        with torch.no_grad():
            c = advance(x[:, :, k + 9:k + 12], sd, arch, wrong)
            d = advance(x[:, :, k + 9:k + 12], sd, arch, state)
        assert not np.array_equal(c.numpy(), d.numpy())


@pytest.fixture(scope="module")
def co_case(pkg):
    arch = _arch(pkg, 3, (8, 8, 16), (8, 16, 16), (1, 2, 1))  # rings of 3, 5 and 3 slots, residual rings of 2
    torch.manual_seed(21)
    m = pkg.MODELS["co-st-gcn"](rank=None, **arch)
    sd = randomise(m.state_dict(), torch.Generator().manual_seed(22))
    sd = {k: v.double() for k, v in sd.items()}
    x = torch.randn(1, 3, 50, 25, generator=torch.Generator().manual_seed(23), dtype=torch.float64)
    return arch, sd, x


@pytest.mark.parametrize("k", [0, 7, 30])
def test_co_rotation_equivalence(co_case, k):
    """As above on the ring addressing over coclip_ref: k = 7 leaves every head wrapped and non-zero ((-7) % 3, % 5,
    % 2), k = 30 every head at exactly 0 after wrapping, k = 0 is the empty stream."""
    arch, sd, x = co_case
    state = R.co_empty(sd, arch, sd["A"])
    if k:
        _, state = R.co_advance(x[:, :, :k], sd, arch, sd["A"], state)
    assert [s[2] for s in state] == [((-k) % 3, (-k) % 2), ((-k) % 5, (-k) % 2), ((-k) % 3, (-k) % 2)]
    canon = R.canonicalise(state)
    a, sa = R.co_advance(x[:, :, k:k + 11], sd, arch, sd["A"], state)
    b, sb = R.co_advance(x[:, :, k:k + 11], sd, arch, sd["A"], canon)
    assert np.array_equal(a.numpy(), b.numpy())
    assert np.array_equal(R.image(sa), R.image(sb))
    # the ring model is coclip_ref's stream: frame by frame through the rings equals one clip from the start
    from coclip_ref import costgcn_clip
    with torch.no_grad():
        whole = costgcn_clip(x[:, :, :k + 11], sd, arch, sd["A"], dtype=torch.float64)[0]
    assert (whole[:, :, k:] - a).abs().max().item() <= 1e-12 * whole.abs().max().item()
    if k == 7:
        wrong = [(np.roll(t0, i0, axis=0), np.roll(t1, i1, axis=0), (0, 0)) for t0, t1, (i0, i1) in state]
        c, _ = R.co_advance(x[:, :, k:k + 3], sd, arch, sd["A"], wrong)
        assert not np.array_equal(c.numpy(), a[:, :, :3].numpy())


# ------------------------------------------------------------------------------------------------ StreamSnapshot
SHAPES = [(8, 3, 1), (16, 5, 2), (16, 3, 1)]


def _snap(pkg, n=4, kind="rt", V=5, shapes=SHAPES, seed=5):
    S = import_module(pkg.__name__ + ".streams")
    table, E = S.state_layout(V, shapes)
    data = torch.randn(n, E, generator=torch.Generator().manual_seed(seed))
    return S.StreamSnapshot(kind, V, table, data)


def test_snapshot_surface(pkg, tmp_path):
    S = import_module(pkg.__name__ + ".streams")
    assert pkg.StreamSnapshot is S.StreamSnapshot
    snap = _snap(pkg)
    assert snap.n == 4 and len(snap) == 4 and snap.kind == "rt" and snap.V == 5 and snap.E == 1040
    assert snap.layout == ((8, 3, 1, 0, 120), (16, 5, 2, 160, 560), (16, 3, 1, 720, 960))
    # state_dict: plain tensors and ints, through torch.save / torch.load
    d = snap.state_dict()
    assert all(isinstance(v, (int, torch.Tensor)) for v in d.values())
    path = tmp_path / "snap.pt"
    torch.save(d, path)
    back = S.StreamSnapshot.from_state_dict(torch.load(path, weights_only=True))
    assert (back.kind, back.V, back.layout, back.E) == (snap.kind, snap.V, snap.layout, snap.E)
    assert torch.equal(back.data, snap.data)
    # rows and cat
    assert torch.equal(snap[2].data, snap.data[2:3]) and snap[2].n == 1
    assert torch.equal(snap[[3, 0]].data, snap.data[[3, 0]])
    assert torch.equal(snap[-1].data, snap.data[3:4])
    with pytest.raises(IndexError):
        snap[4]
    both = S.StreamSnapshot.cat([snap[[1]], snap[[0, 2]]])
    assert both.n == 3 and torch.equal(both.data, snap.data[[1, 0, 2]])
    assert snap.to("cpu").data.device.type == "cpu"
    with pytest.raises(RuntimeError, match="kind 'rt' != 'co'"):
        S.StreamSnapshot.cat([snap, _snap(pkg, kind="co")])
    with pytest.raises(RuntimeError, match="at least one"):
        S.StreamSnapshot.cat([])
    # a snapshot that contradicts itself is refused when it is made
    with pytest.raises(RuntimeError, match="kind"):
        S.StreamSnapshot("xx", 5, snap.layout, snap.data)
    with pytest.raises(RuntimeError, match="offsets"):
        S.StreamSnapshot("rt", 5, ((8, 3, 1, 0, 124),) + snap.layout[1:], snap.data)
    with pytest.raises(RuntimeError, match="data must be fp32 of shape"):
        S.StreamSnapshot("rt", 5, snap.layout, snap.data[:, :-4])
    with pytest.raises(RuntimeError, match="data must be fp32 of shape"):
        S.StreamSnapshot("rt", 5, snap.layout, snap.data.double())
    bad = dict(d, E=1044)
    with pytest.raises(RuntimeError, match="names E"):
        S.StreamSnapshot.from_state_dict(bad)
    with pytest.raises(RuntimeError, match="version"):
        S.StreamSnapshot.from_state_dict(dict(d, version=2))


def _bare_batch(pkg, kind, B=3, V=5, shapes=SHAPES):
    """A batch cannot be constructed without a device, so the host checks run on a bare instance with the attributes
    they read: B, V and state tensors of the right shapes."""
    mod, cls = {"rt": ("rtstgcn", "RtStreamBatch"), "co": ("costgcn", "CoStreamBatch")}[kind]
    batch = object.__new__(getattr(import_module(f"{pkg.__name__}.{mod}"), cls))
    batch.B, batch.V, batch.dtype = B, V, torch.float32
    batch.state = [(torch.zeros(B, n0, V, C), torch.zeros(B, n1, V, C), torch.zeros(B, 2, dtype=torch.int32))
                   for C, n0, n1 in shapes]
    batch._desc = lambda: None
    return batch


@pytest.mark.parametrize("kind", ["rt", "co"])
def test_import_state_refuses_on_the_host(pkg, kind):
    batch = _bare_batch(pkg, kind)
    good = _snap(pkg, kind=kind)
    other = "co" if kind == "rt" else "rt"
    with pytest.raises(RuntimeError, match="expects a StreamSnapshot"):
        batch.import_state(good.data)
    with pytest.raises(RuntimeError, match=f"kind '{other}' != '{kind}'"):
        batch.import_state(_snap(pkg, kind=other))
    with pytest.raises(RuntimeError, match="layer count 2 != 3"):
        batch.import_state(_snap(pkg, kind=kind, shapes=SHAPES[:2]))
    with pytest.raises(RuntimeError, match="V 7 != 5"):
        batch.import_state(_snap(pkg, kind=kind, V=7))
    with pytest.raises(RuntimeError, match="layer 1: C 12 != 16"):
        batch.import_state(_snap(pkg, kind=kind, shapes=[SHAPES[0], (12, 5, 2), SHAPES[2]]))
    with pytest.raises(RuntimeError, match=r"layer 1: .*\(n0.* 9 != 5"):   # another kernel size or stride
        batch.import_state(_snap(pkg, kind=kind, shapes=[SHAPES[0], (16, 9, 2), SHAPES[2]]))
    with pytest.raises(RuntimeError, match=r"layer 2: .*\(n1.* 2 != 1"):
        batch.import_state(_snap(pkg, kind=kind, shapes=[SHAPES[0], SHAPES[1], (16, 3, 2)]))
    with pytest.raises(RuntimeError, match="slot 1 is targeted twice"):
        batch.import_state(good, streams=[1, 0, 1, 2])
    with pytest.raises(RuntimeError, match=r"slot 3 outside \[0, 3\)"):
        batch.import_state(good[[0]], streams=[3])
    with pytest.raises(RuntimeError, match=r"slot -1 outside"):
        batch.import_state(good[[0]], streams=[-1])
    with pytest.raises(RuntimeError, match="4 rows for 2 slots"):
        batch.import_state(good, streams=[0, 1])
    with pytest.raises(RuntimeError, match="2 rows for 3 slots"):
        batch.import_state(good, streams=[0, 1, 2], select=[0, 1])
    with pytest.raises(RuntimeError, match=r"select row 4 outside \[0, 4\)"):
        batch.import_state(good, streams=[0], select=[4])
    with pytest.raises(RuntimeError, match="slot 3 outside"):  # the default slots 0 .. n-1 of 4 rows in a batch of 3
        batch.import_state(good)
    with pytest.raises(RuntimeError, match="nothing to import"):
        batch.import_state(good, streams=[], select=[])
    with pytest.raises(RuntimeError, match=r"slot 5 outside"):
        batch.export_state([0, 5])
    with pytest.raises(RuntimeError, match="HIP device only"):   # everything fits: no CPU fallback
        batch.import_state(good, streams=[2, 0], select=[1, 3])
    with pytest.raises(RuntimeError, match="HIP device only"):
        batch.export_state([0])


def test_model_surface(pkg):
    for mod in ("rtstgcn", "costgcn"):
        M = import_module(f"{pkg.__name__}.{mod}").Model
        assert callable(M.export_state) and callable(M.import_state)
        assert "parameters it was taken under" in (M.export_state.__doc__ + pkg.StreamSnapshot.__doc__)
    arch = _small_arch(pkg, 25, 3)
    m = pkg.MODELS["rt-st-gcn"](rank=None, **arch)
    with pytest.raises(RuntimeError, match="prepare_benchmark first"):
        m.export_state()
    with pytest.raises(RuntimeError, match="prepare_benchmark first"):
        m.import_state(_snap(pkg, n=1))


# ------------------------------------------------------------------------------------------------ the C ABI
def make_desc(L, kind=0, V=5, B=3, n=2, dtype=0, shapes=SHAPES):
    """Every pointer and shape valid, the offsets the dense layer-major ones."""
    d = L.StreamStateDesc(kind=kind, V=V, L=len(shapes), B=B, n=n, dtype=dtype, slots=FAKE, snap=FAKE)
    table, E = R.layout(V, shapes)
    d.E = E
    for y, row in zip(d.layers, table):
        y.s0 = y.s1 = y.idx = FAKE
        y.C, y.n0, y.n1, y.off0, y.off1 = row
    return d


def test_descriptor_layout(pkg, tmp_path):
    L = pkg._lib
    got, expect = _c_layout(tmp_path, {"stgcn_stream_state_layer": L.StreamStateLayer,
                                       "stgcn_stream_state_desc": L.StreamStateDesc})
    assert got == expect
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stgcn_amd.h")).read()
    assert "#define STGCN_STREAM_STATE_RT 0" in hdr and "#define STGCN_STREAM_STATE_CO 1" in hdr
    assert (L.STREAM_STATE_RT, L.STREAM_STATE_CO) == (0, 1)
    S = import_module(pkg.__name__ + ".streams")
    assert S.KINDS == ("rt", "co")


def test_integration_stub_matches_bindings(pkg):
    """The stub structs INTEGRATION.md shows for the new descriptor are the package's own, field for field."""
    import ctypes
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    m = re.search(r"^class StreamStateLayer\(ctypes\.Structure\):.*?^class StreamStateDesc\(ctypes\.Structure\):.*?"
                  r"(?=^\S)", text, flags=re.M | re.S)
    assert m, "INTEGRATION.md no longer shows the stream-state stubs"
    ns = {"ctypes": ctypes}
    exec(m.group(0), ns)
    L = pkg._lib
    for name in ("StreamStateLayer", "StreamStateDesc"):
        stub, own = ns[name], getattr(L, name)
        assert ctypes.sizeof(stub) == ctypes.sizeof(own)
        assert [(f, getattr(stub, f).offset) for f, _ in stub._fields_] == \
               [(f, getattr(own, f).offset) for f, _ in own._fields_]


def test_symbols_exported(pkg):
    lib = pkg._lib.load_library()
    for name in ("stgcn_stream_state_check", "stgcn_stream_state_export", "stgcn_stream_state_import"):
        assert hasattr(lib, name) and name in pkg._lib.EXPORTS
    assert lib.stgcn_abi_version() == 7


def test_refuses_bad_descriptors(pkg):
    """Every refusal comes before any launch: no device is needed to get it."""
    L = pkg._lib
    lib = L.load_library()
    calls = (lib.stgcn_stream_state_export, lib.stgcn_stream_state_import)

    def refused(d, code=1):
        assert lib.stgcn_stream_state_check(d) == code
        for call in calls:
            assert call(d, None) == code

    for call in calls:
        assert call(None, None) == 1
    assert lib.stgcn_stream_state_check(None) == 1
    refused(L.StreamStateDesc())
    for kind in (0, 1):
        for dtype in (0, 1):
            assert lib.stgcn_stream_state_check(make_desc(L, kind=kind, dtype=dtype)) == 0
    for kw in (dict(n=0), dict(n=-1), dict(B=0), dict(V=1), dict(V=33), dict(shapes=[]), dict(shapes=SHAPES * 5),
               dict(kind=2), dict(kind=-1),
               dict(shapes=[(6, 3, 1)]), dict(shapes=[(0, 3, 1)]),       # C % 4 != 0, no channels
               dict(shapes=[(8, 0, 1)]), dict(shapes=[(8, 3, 0)])):      # no slots
        refused(make_desc(L, **kw))
    assert lib.stgcn_stream_state_check(make_desc(L, shapes=SHAPES * 4)) == 0  # 12 layers: the most
    refused(make_desc(L, dtype=2), 2)
    refused(make_desc(L, dtype=-1), 2)
    refused(make_desc(L, V=33, dtype=2))                                   # shapes first, then the dtype
    for field in ("slots", "snap"):
        d = make_desc(L)
        setattr(d, field, None)
        refused(d)
    for field in ("s0", "s1", "idx"):
        d = make_desc(L)
        setattr(d.layers[2], field, None)
        refused(d)
    # E and the offsets: the dense layer-major image and nothing else
    for delta in (-4, 4):
        d = make_desc(L)
        d.E += delta
        refused(d)
    for layer, field in ((0, "off0"), (0, "off1"), (1, "off0"), (2, "off1")):
        d = make_desc(L)
        setattr(d.layers[layer], field, getattr(d.layers[layer], field) + 4)
        refused(d)
    d = make_desc(L)                                                       # s1 in front of s0
    d.layers[0].off0, d.layers[0].off1 = 40, 0
    refused(d)
    # more workgroups than a grid holds
    refused(make_desc(L, V=32, n=1 << 26, shapes=[(256, 137, 35)] * 12))
