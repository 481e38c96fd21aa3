"""co-st-gcn without a GPU: the restatement against reference-generated fixtures, state_dict compatibility with
st-gcn, the refused configurations, and host-side argument validation of the stgcn_co_* entry points."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from costgcn_ref import costgcn_stream  # noqa: E402


def _arch(P, kernel=9, in_ch=(8, 8, 16), out_ch=(8, 16, 16), stride=(1, 2, 1), normalization="LayerNorm"):
    nl = len(in_ch)
    return {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": normalization, "num_classes": 7, "graph": P.PKU_MMD,
            "st-gcn": {"importance": True, "in_feat": 3, "stages": 1, "layers": nl, "kernel": kernel,
                       "in_ch": list(in_ch), "out_ch": list(out_ch), "stride": list(stride), "dilation": [1] * nl,
                       "residual": [1] * nl, "dropout": [0.0] * nl}}


@pytest.mark.parametrize("name", ["costgcn_k9", "costgcn_k69"])
def test_restatement_reproduces_reference(golden, name):
    g = golden(name)
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd/")}
    with torch.no_grad():
        y = costgcn_stream(g["x"], sd, g["arch"], sd["A"])
    ref = g["y"]
    assert y.shape == ref.shape
    err = (y - ref).abs().max().item() / ref.abs().max().item()
    if os.environ.get("STGCN_TEST_REPORT"):
        print(f"[err] restatement {name}: {err:.2e}")
    assert err <= 1e-5, f"{name}: restatement vs reference {err:.2e}"


def test_state_dict_matches_stgcn(pkg):
    P = pkg
    arch = _arch(P, in_ch=(64, 64, 64, 64, 128, 128, 128, 256, 256), out_ch=(64, 64, 64, 128, 128, 128, 256, 256, 256),
                 stride=(1, 1, 1, 2, 1, 1, 2, 1, 1))
    torch.manual_seed(3)
    st = P.MODELS["st-gcn"](rank=None, **arch)
    co = P.MODELS["co-st-gcn"](rank=None, **arch)
    ks, kc = st.state_dict(), co.state_dict()
    assert len(ks) == 96 and set(ks) == set(kc)
    assert all(ks[k].shape == kc[k].shape for k in ks)
    co.load_state_dict(ks, strict=True)
    st.load_state_dict(co.state_dict(), strict=True)
    assert all(torch.equal(co.state_dict()[k], ks[k]) for k in ks)
    assert co.prepare_benchmark(arch) is arch


def test_batchnorm_refused(pkg):
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        pkg.MODELS["co-st-gcn"](rank=None, **_arch(pkg, normalization="BatchNorm"))


def test_forward_refuses_grad_and_shapes(pkg):
    m = pkg.MODELS["co-st-gcn"](rank=None, **_arch(pkg))
    with pytest.raises(RuntimeError, match="inference only"):
        m(torch.zeros(1, 3, 1, 25))
    with torch.no_grad(), pytest.raises(RuntimeError, match="one frame"):
        m(torch.zeros(1, 3, 2, 25))
    with torch.no_grad(), pytest.raises(RuntimeError, match="one frame"):
        m(torch.zeros(2, 3, 1, 25))


def _desc(L, **kw):
    """A descriptor whose every pointer is non-null (never dereferenced: the calls below are refused on the host)."""
    d = L.CoLayer(V=25, Cin=8, Cout=8, P=3, Kt=9, S=1, res_mode=1, dtype=0, splits=0)
    for n, t in L.CoLayer._fields_:
        if t is L.c_void_p:
            setattr(d, n, 64)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_co_abi_rejects_bad_args_without_gpu(pkg):
    L = pkg._lib
    lib = L.load_library()
    entries = (lib.stgcn_co_gcn, lib.stgcn_co_push, lib.stgcn_co_taps, lib.stgcn_co_finish)
    for fn in entries:
        assert fn(L.CoLayer(), None) == 1                                   # all-null descriptor
        assert fn(L.CoLayer(V=25, Cin=8, Cout=8, P=3, Kt=9, S=1), None) == 1  # good shapes, null pointers
        assert fn(_desc(L, V=33), None) == 1
        assert fn(_desc(L, Cin=6, Cout=6), None) == 1                      # C % 4 != 0
        assert fn(_desc(L, Kt=8), None) == 1                               # even Kt
        assert fn(_desc(L, Kt=71), None) == 1
        assert fn(_desc(L, S=3), None) == 1
        assert fn(_desc(L, Cout=260), None) == 1
        assert fn(_desc(L, Cin=8, Cout=16, res_mode=1), None) == 1         # identity residual needs Cin == Cout
        assert fn(_desc(L, wt=None), None) == 1
    assert lib.stgcn_co_pack_weight(None, 8, 8, 9, None, 0, None) == 1
    assert lib.stgcn_co_pack_weight(64, 8, 8, 8, 64, 0, None) == 1          # even Kt
    assert lib.stgcn_co_pack_weight(64, 6, 6, 9, 64, 0, None) == 1
    assert lib.stgcn_co_pack_elems(8, 8, 8) == -1
    assert lib.stgcn_co_pack_elems(256, 256, 69) == 8 * (69 * 256 // 16) * 512
    assert lib.stgcn_co_workspace(_desc(L, V=33), None) == -1
    assert lib.stgcn_co_splits(_desc(L, Kt=8), None) == -1
    assert lib.stgcn_co_splits(_desc(L, Cin=256, Cout=256, Kt=69, splits=7), None) == 7
    assert lib.stgcn_co_workspace(_desc(L, Cin=256, Cout=256, Kt=69, splits=7), None) == 7 * 25 * 256 * 4
