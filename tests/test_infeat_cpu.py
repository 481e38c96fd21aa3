"""Input heads with other than 3 features per joint, host side, no GPU: the descriptors' ``F`` field (header and
ctypes layouts, 0 read as 3, the refusals before any launch), the stgcn_rt_frame_in_f entry, and the two in_feat-6
fixtures (tests/golden/make_golden_infeat.py: the reference's 7-node IMU graph, six features per node) against the
fp32 references the GPU tests of tests/test_gpu_infeat.py are measured with."""
import os
import sys

import pytest
import torch

from conftest import assert_close, load_golden, sub
from oracle import stgcn_oracle as O
from test_cpu_host import _c_layout

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from costgcn_ref import costgcn_stream  # noqa: E402

HEAD_DESCS = {"stgcn_rt_frame_desc": "RtFrameDesc", "stgcn_rt_streams_desc": "RtStreamsDesc",
              "stgcn_co_streams_desc": "CoStreamsDesc", "stgcn_co_clip_desc": "CoClipDesc",
              "stgcn_co_streams_clip_desc": "CoStreamsClipDesc", "stgcn_rt_streams_clip_desc": "RtStreamsClipDesc"}


def test_descriptors_have_F_and_match_the_header(pkg, tmp_path):
    """Each of the six head-carrying descriptors has an int ``F`` among its leading ints, zero in a fresh descriptor
    (read as 3), and the ctypes mirror has the size and the field offsets gcc gives the header's struct."""
    L = pkg._lib
    structs = {c: getattr(L, p) for c, p in HEAD_DESCS.items()}
    for cname, cls in structs.items():
        fields = dict(cls._fields_)
        assert fields.get("F") is L.c_int, cname
        assert cls().F == 0
        assert cls.F.offset < cls.ln_w.offset, f"{cname}: F sits with the shape ints, ahead of the pointers"
    got, expect = _c_layout(tmp_path, structs)
    assert got == expect
    assert L.MAX_IN_FEAT == 16
    assert L.load_library().stgcn_abi_version() == 7


def _fill(L, d, layer_ints):
    """Every pointer and stride of ``d`` and of its first layer non-null (never dereferenced: each call below is
    refused or answered on the host), the layer's ints from ``layer_ints``."""
    for n, t in type(d)._fields_:
        if t is L.c_void_p:
            setattr(d, n, 64)
        elif t is L.c_long:
            setattr(d, n, 1 << 20)
    y = d.layers[0]
    for n, t in type(y)._fields_:
        if t is L.c_void_p:
            setattr(y, n, 64)
    for k, v in layer_ints.items():
        setattr(y, k, v)
    return d


RT_LAYER = dict(Cin=8, Cout=8, P=3, fifo_size=9, S=1, res_mode=1)
CO_LAYER = dict(Cin=8, Cout=8, P=3, Kt=9, S=1, res_mode=1)


def _descs(L):
    """(entry point, a descriptor that passes every host check but for F) for the six entries."""
    return [
        ("stgcn_rt_frame", _fill(L, L.RtFrameDesc(V=7, L=1, C0=8, K=4, blocks=0), RT_LAYER)),
        ("stgcn_rt_streams", _fill(L, L.RtStreamsDesc(V=7, L=1, C0=8, K=4, B=2), RT_LAYER)),
        ("stgcn_co_streams", _fill(L, L.CoStreamsDesc(B=2, V=7, L=1, C0=8, K=4), CO_LAYER)),
        ("stgcn_co_clip", _fill(L, L.CoClipDesc(T=4, V=7, L=1, C0=8, K=4), CO_LAYER)),
        ("stgcn_co_streams_clip", _fill(L, L.CoStreamsClipDesc(B=2, T=4, t0=0, V=7, L=1, C0=8, K=4), CO_LAYER)),
        ("stgcn_rt_streams_clip", _fill(L, L.RtStreamsClipDesc(B=2, T=4, t0=0, V=7, L=1, C0=8, K=4), RT_LAYER)),
    ]


@pytest.mark.parametrize("bad", [17, -1, 1 << 20])
def test_F_out_of_range_is_refused_before_any_launch(pkg, bad):
    """F outside [0, 16] returns 1 (bad shape) from every descriptor entry point; the pointers are fake (never
    dereferenced on the host), so the answer comes from the host checks alone.  The shape-only queries of the co-st-gcn entries answer -1."""
    L = pkg._lib
    lib = L.load_library()
    for entry, d in _descs(L):
        d.F = bad
        assert getattr(lib, entry)(d, None) == 1, entry
        if entry.startswith("stgcn_co_"):
            assert getattr(lib, entry + "_splits")(d, 0) == -1, entry
            assert getattr(lib, entry + "_workspace")(d, 0) == -1, entry


@pytest.mark.parametrize("F", [0, 1, 3, 6, 16])
def test_F_in_range_passes_the_shape_checks(pkg, F):
    """The shape-only queries (no pointer is read, nothing is launched) accept F = 0 (read as 3) and 1 .. 16, and the
    split count does not depend on F."""
    L = pkg._lib
    lib = L.load_library()
    for entry, d in _descs(L):
        if entry.startswith("stgcn_co_"):
            d.F = F
            assert getattr(lib, entry + "_splits")(d, 0) >= 1, entry


def test_rt_frame_in_f_is_exported_and_checks_F(pkg):
    L = pkg._lib
    lib = L.load_library()
    fn = lib.stgcn_rt_frame_in_f
    assert len(fn.argtypes) == 10
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "stgcn_amd.h")).read()
    assert "int stgcn_rt_frame_in_f(const float* x, int F, int V," in hdr
    assert fn(None, 6, 7, None, None, None, None, 8, None, None) == 1      # null pointers
    for bad in (0, -1, 17):                                                  # the entry takes F itself: no 0 = 3 here
        assert fn(64, bad, 7, 64, 64, 64, 64, 8, 64, None) == 1
    assert fn(64, 6, 33, 64, 64, 64, 64, 8, 64, None) == 1                  # V > 32
    assert lib.stgcn_rt_frame_in(None, 7, None, None, None, None, 8, None, None) == 1


def test_stream_batch_shape_messages(pkg):
    """``step`` / ``step_clip`` name the batch's own in_feat in the expected shape; at in_feat 3 the text is what it
    was.  On bare instances: the checks run before anything touches a device."""
    from importlib import import_module
    for mod, cls in (("rtstgcn", "RtStreamBatch"), ("costgcn", "CoStreamBatch")):
        batch = object.__new__(getattr(import_module(pkg.__name__ + "." + mod), cls))
        batch.B, batch.V, batch.clip_frames = 2, 7, 1024
        assert batch.F == 3
        with pytest.raises(RuntimeError, match=rf"{cls}\.step expects x of shape \(2, 3, 1, 7\), got \(2, 6, 1, 7\)"):
            batch.step(torch.zeros(2, 6, 1, 7))
        batch.F = 6
        with pytest.raises(RuntimeError, match=rf"{cls}\.step expects x of shape \(2, 6, 1, 7\), got \(2, 3, 1, 7\)"):
            batch.step(torch.zeros(2, 3, 1, 7))
        with pytest.raises(RuntimeError, match=rf"{cls}\.step_clip expects x of shape \(2, 6, T >= 1, 7\), got "
                                               r"\(2, 3, 4, 7\)"):
            batch.step_clip(torch.zeros(2, 3, 4, 7))
        with pytest.raises(RuntimeError, match="HIP device only"):  # the right shape gets as far as the device check
            batch.step(torch.zeros(2, 6, 1, 7))


# ------------------------------------------------------------------------------------------------ the fixtures
def test_fixtures_are_the_imu_shape():
    for name, key in (("rt_infeat6", "rt-st-gcn"), ("costgcn_infeat6", "st-gcn")):
        g = load_golden(name)
        arch = g["arch"]
        assert arch["in_feat"] == 6 and arch[key]["in_feat"] == 6 and arch["normalization"] == "LayerNorm"
        assert arch["graph"]["num_node"] == 7 and arch["graph"]["center"] == 0 and len(arch["graph"]["edge"]) == 13
        assert (arch[key]["in_ch"], arch[key]["out_ch"], arch[key]["stride"]) == ([8, 8, 16], [8, 16, 16], [1, 2, 1])
        assert arch["kernel"] == 9 and arch[key]["residual"] == [1, 1, 1] and arch["num_classes"] == 7
        assert tuple(g["x"].shape) == (1, 6, 40, 7)
        assert tuple(g["sd/norm_in.weight"].shape) == (6, 1, 7) and tuple(g["sd/fcn_in.weight"].shape) == (8, 6, 1, 1)
        assert tuple(g["sd/A"].shape) == (3, 7, 7)
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")
        assert os.path.getsize(path) < 1 << 20


def test_oracle_reproduces_rt_infeat6():
    """oracle.rt_model_online against the reference's own online outputs at in_feat 6, test_oracle_golden.py's bar."""
    d = load_golden("rt_infeat6")
    with torch.no_grad():
        yo = O.rt_model_online(d["x"], {k: v.clone() for k, v in sub(d, "sd/").items()}, d["arch"])
    assert_close(yo, d["y_online"], 1e-4, "rt_infeat6 online y")


def test_restatement_reproduces_costgcn_infeat6():
    """costgcn_ref.costgcn_stream against the reference's own outputs at in_feat 6, test_oracle_golden.py's bar."""
    g = load_golden("costgcn_infeat6")
    sd = sub(g, "sd/")
    with torch.no_grad():
        y = costgcn_stream(g["x"], sd, g["arch"], sd["A"])
    assert_close(y, g["y"], 1e-4, "costgcn_infeat6 y")


def test_in_feat_limit_is_refused_on_the_host(pkg):
    """in_feat 17: the rt stream batch names the limit (no device is needed to get that far)."""
    d = load_golden("rt_infeat6")
    arch = dict(d["arch"], in_feat=17)
    arch["rt-st-gcn"] = dict(arch["rt-st-gcn"], in_feat=17)
    m = pkg.MODELS["rt-st-gcn"](rank=None, **arch).eval()
    m.prepare_benchmark(arch)
    with pytest.raises(RuntimeError, match=r"1 <= in_feat <= 16, got 17"):
        m.stream_batch(2)
