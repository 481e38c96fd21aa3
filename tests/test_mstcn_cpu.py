"""ms-tcn / ms-gcn without a GPU: the restatement against reference-generated fixtures (outputs and every gradient),
state_dict compatibility, the registry, the refused configurations and host-side validation of the stgcn_ms_* ABI."""
import os
import sys

import pytest
import torch

from conftest import sub

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mstcn_ref as R  # noqa: E402

BAR = 1e-5


def _close(got, ref, name):
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} != {tuple(ref.shape)}"
    err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    if os.environ.get("STGCN_TEST_REPORT"):
        print(f"[err] restatement {name}: {err:.2e}")
    assert err <= BAR, f"{name}: restatement vs reference {err:.2e}"


def _check(y, grads, dx, g, name, prefix=""):
    _close(y, g[prefix + "y"], f"{name} y")
    ref = sub(g, prefix + "grad/")
    assert set(grads) == set(ref)
    for k, v in ref.items():
        _close(grads[k], v, f"{name} grad {k}")
    if dx is not None:
        _close(dx, g[prefix + "dx"], f"{name} dx")


def model_fn(name, g):
    """(fn(x, sd), x) of a model fixture for mstcn_ref.grads_of."""
    if name == "msgcn_model":
        return (lambda x, sd: R.msgcn_model(x, sd, g["arch"])), R.windows(g["capture"], g["arch"]["receptive_field"])
    return (lambda x, sd: R.mstcn_model(x, sd, g["arch"])), g["x"]


@pytest.mark.parametrize("V", [1, 3])
def test_restatement_stage(golden, V):
    g = golden("mstcn_stage")
    p = f"v{V}/"
    y, grads, dx = R.grads_of(lambda x, sd: R.single_stage(x, sd), g[p + "x"], sub(g, "sd/"), g[p + "g"],
                              input_grad=True)
    _check(y, grads, dx, g, f"stage V={V}", p)


@pytest.mark.parametrize("name", ["mstcn_model", "msgcn_model", "mstcn_logsoftmax"])
def test_restatement_models(golden, name):
    g = golden(name)
    fn, x = model_fn(name, g)
    y, grads, _ = R.grads_of(fn, x, sub(g, "sd/"), g["g"])
    _check(y, grads, None, g, name)


@pytest.mark.parametrize("name", ["mstcn_model", "msgcn_model", "mstcn_logsoftmax"])
def test_state_dict_matches_reference(pkg, golden, name):
    g = golden(name)
    ref = sub(g, "sd/")
    kind = "ms-gcn" if name == "msgcn_model" else "ms-tcn"
    m = pkg.MODELS[kind](rank=None, **g["arch"])
    own = m.state_dict()
    assert set(own) == set(ref)
    assert all(own[k].shape == ref[k].shape for k in ref)
    m.load_state_dict(ref, strict=True)
    assert all(torch.equal(m.state_dict()[k], ref[k]) for k in ref)
    if kind == "ms-gcn":  # the reference's DataParallel-wrapped generator
        dp = {k.replace("generator_stage.", "generator_stage.module."): v + 1 for k, v in ref.items()}
        m.load_state_dict(dp, strict=True)
        assert all(torch.equal(m.state_dict()[k], ref[k] + 1) for k in ref)


def test_stage_state_dict(pkg, golden):
    ref = sub(golden("mstcn_stage"), "sd/")
    st = pkg.mstcn.SingleStage(in_channels=7, out_channels=7, num_filters=16, num_layers=6, kernel=3, dropout=0.0)
    assert {k: v.shape for k, v in st.state_dict().items()} == {k: v.shape for k, v in ref.items()}
    assert ref["layers.5.conv.0.weight"].shape == (16, 16, 3, 1) and ref["conv_in.weight"].shape == (16, 7, 1, 1)
    st.load_state_dict(ref, strict=True)


def test_registry_and_helpers(pkg):
    assert {"ms-tcn", "ms-gcn"} <= set(pkg.MODELS)
    assert issubclass(pkg.loss.LossMultiStage, pkg.loss.Loss)
    assert issubclass(pkg.loss.StatisticsMultiStage, pkg.loss.Statistics)
    arch = dict(stages=3, num_classes=7, graph={"num_node": 25}, in_feat=3, receptive_field=20, segment=37)
    seg = pkg.segment.WindowSegmentMultiStage(rank="cpu", world_size=1, **arch)
    p = torch.zeros(3, 1, 7, 37)
    assert seg.mask_segment(37, 19, 0, p) is p and seg.pad_sequence(37) == (19, 0)
    one = pkg.segment.WindowSegmentOneToOneMultiStage(rank="cpu", world_size=1, **arch)
    assert one.pad_sequence(37) == (0, 0) and one.get_segment(p) is p and one.mask_segment(37, 0, 0, p) is p


def _arch(stages=2, layers=(2, 2), kernel=3, filters=16, dropout=0.0, classes=7):
    return {"in_feat": 3, "stages": stages, "refine": "softmax", "output_type": "logits", "num_classes": classes,
            "ms-tcn": {"in_feat": 3, "stages": stages, "layers": list(layers), "kernel": [kernel] * stages,
                       "filters": [filters] * stages, "dropout": [dropout] * stages}}


def test_refusals_on_the_host(pkg):
    """Every unsupported argument raises before any launch: no device is present or needed here."""
    M = pkg.MODELS["ms-tcn"]
    with pytest.raises(NotImplementedError, match="kernel 3"):
        M(rank=None, **_arch(kernel=5))
    for f in (8, 24, 80):
        with pytest.raises(NotImplementedError, match="filters"):
            M(rank=None, **_arch(filters=f))
    with pytest.raises(NotImplementedError, match="num_classes"):
        M(rank=None, **_arch(classes=65))
    x = torch.zeros(1, 3, 37, 25)
    m = M(rank=None, **_arch(dropout=0.5))
    with pytest.raises(NotImplementedError, match="dropout"):
        m.train()(x)
    m = M(rank=None, **_arch())
    with pytest.raises(NotImplementedError, match="32 joints"):
        m(torch.zeros(1, 3, 37, 33))
    with pytest.raises(NotImplementedError, match=r"one \(1, in_feat, L, V\)"):
        m(torch.zeros(2, 3, 37, 25))
    deep = M(rank=None, **_arch(layers=(24, 2)))   # dilation 2^23 * 925 rows > 2^31 - 1
    with pytest.raises(NotImplementedError, match="int row arithmetic"):
        deep(x)
    # a supported call then needs the device: there is no eager path
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.eval()(x)
    g = pkg.MODELS["ms-gcn"]
    with pytest.raises(NotImplementedError, match="kernel 3"):
        g(rank=None, **dict(_arch(kernel=5), strategy="spatial", normalization="LayerNorm", graph=pkg.PKU_MMD,
                            **{"st-gcn": {"importance": True, "in_feat": 3, "layers": 1, "kernel": 9, "in_ch": [8],
                                          "out_ch": [8], "stride": [1], "residual": [1], "dropout": [0]}}))


def _ptrs(d, L):
    for n, t in d._fields_:
        if t is L.c_void_p:
            setattr(d, n, 64)   # never dereferenced: the calls below are refused on the host
    return d


def test_ms_abi_rejects_bad_args_without_gpu(pkg):
    L = pkg._lib
    lib = L.load_library()
    for name in ("stgcn_ms_pack_elems", "stgcn_ms_pack_layer", "stgcn_ms_wgrad_blocks", "stgcn_ms_layer_fwd",
                 "stgcn_ms_layer_bwd", "stgcn_ms_lin_blocks", "stgcn_ms_in_fwd", "stgcn_ms_in_bwd", "stgcn_ms_out_fwd",
                 "stgcn_ms_out_bwd", "stgcn_ms_prob_fwd", "stgcn_ms_prob_bwd"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.stgcn_abi_version() == 7

    def layer(**kw):
        d = _ptrs(L.MsLayer(R=925, V=25, F=64, dil=4, dtype=0), L)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for fn in (lib.stgcn_ms_layer_fwd, lib.stgcn_ms_layer_bwd):
        assert fn(L.MsLayer(), None) == 1
        assert fn(L.MsLayer(R=925, V=25, F=64, dil=4), None) == 1     # good shapes, null pointers
        for bad in (dict(F=8), dict(F=24), dict(F=80), dict(R=926), dict(dil=0), dict(R=25 * 2 ** 20, dil=2 ** 9)):
            assert fn(layer(**bad), None) == 1, bad
        assert fn(layer(dtype=2), None) == 2
    assert lib.stgcn_ms_pack_layer(64, 64, 64, 5, 64, 0, None) == 1    # kernel != 3
    assert lib.stgcn_ms_pack_layer(64, 64, 40, 3, 64, 0, None) == 1
    assert lib.stgcn_ms_pack_layer(None, 64, 64, 3, 64, 0, None) == 1
    assert lib.stgcn_ms_pack_layer(64, 64, 64, 3, 64, 3, None) == 2
    assert lib.stgcn_ms_pack_elems(24) == -1
    assert lib.stgcn_ms_pack_elems(64) == 2 * 2 * 512 * (12 + 4)
    assert lib.stgcn_ms_pack_elems(16) == 2 * 512 * (3 + 1)
    assert lib.stgcn_ms_wgrad_blocks(0) == -1 and lib.stgcn_ms_wgrad_blocks(129) == 2
    assert lib.stgcn_ms_wgrad_blocks(10 ** 6) == 256 and lib.stgcn_ms_lin_blocks(33) == 2

    def lin(**kw):
        d = _ptrs(L.MsLin(rows=37, pool=1, I=7, O=16, mode=2), L)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for fn in (lib.stgcn_ms_in_fwd, lib.stgcn_ms_in_bwd):
        assert fn(L.MsLin(), None) == 1
        for bad in (dict(I=65), dict(O=24), dict(pool=2), dict(mode=3), dict(rows=0), dict(w=None)):
            assert fn(lin(**bad), None) == 1, bad
    for fn in (lib.stgcn_ms_out_fwd, lib.stgcn_ms_out_bwd):
        for bad in (dict(I=16, O=65, mode=0), dict(I=16, O=7, mode=1), dict(I=20, O=7, mode=0),
                    dict(I=16, O=7, mode=0, pool=33)):
            assert fn(lin(**bad), None) == 1, bad
    assert lib.stgcn_ms_prob_fwd(64, 37, 65, 1, 64, None) == 1
    assert lib.stgcn_ms_prob_fwd(64, 37, 7, 0, 64, None) == 1
    assert lib.stgcn_ms_prob_bwd(64, None, 37, 7, 1, 64, None) == 1
