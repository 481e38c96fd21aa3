"""bf16 conv operands of the rt-st-gcn stream batch (Model.stream_batch(B, dtype), stgcn_rt_streams with
desc.dtype = 1), host side, no GPU: the Python surface and its refusals, the C-ABI additions, and the yardstick of
the GPU parity test (tests/test_gpu_rt_streams_bf16.py): a restatement of the online network with the operands
rounded to bf16 exactly where rt_streams.hip rounds them, and its error E_ref against the oracle in fp64.

The networks, inputs and recorded E_ref of the GPU test live here so that both files use the same ones."""
import contextlib
import inspect

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub
from oracle import stgcn_oracle as O

# ------------------------------------------------------------------------------------------------ the cases
PKU_V = 25


def _small_arch(P, V, nparts):
    """Three layers, widths 4 -> 20 -> 36 (-> 36): a k tail below one 16-step (Cin = 4, 20, 36), a column tail below
    one 32-tile (Cout = 20, 36), two residual convs and a layer without residual (the oracle's online form needs
    Cin == Cout there; the identity residual is wide_c256's and the golden models'), one stride-2 layer; kernel 3, so
    the FIFOs hold 3 and 5 frames."""
    if V == 2:
        graph = {"num_node": 2, "edge": [[0, 0], [1, 1], [0, 1]], "center": 0}
    else:
        graph = dict(P.PKU_MMD)
    strategy = "spatial"
    if nparts == 1:  # one partition: the hop-0 'distance' graph (its A is replaced by a dense one in build_case)
        strategy, graph = "distance", dict(graph, max_hop=0)
    conf = {"layers": 3, "kernel": 3, "in_ch": [4, 20, 36], "out_ch": [20, 36, 36], "stride": [1, 2, 1],
            "residual": [1, 1, 0], "dropout": [0.0] * 3, "latency": False, "importance": True, "in_feat": 3,
            "buffer": 1, "stages": 1}
    return {"strategy": strategy, "in_feat": 3, "stages": 1, "kernel": 3, "output_type": "logits",
            "normalization": "LayerNorm", "segment": 500, "num_classes": 7, "rt-st-gcn": conf, "graph": graph}


def _wide_arch(P):
    """A layer pair at C = 256, V = 25 (V * C = 6400 <= 7680): 8 column tiles x 3 partitions, 16 k-steps."""
    conf = {"layers": 2, "kernel": 3, "in_ch": [256, 256], "out_ch": [256, 256], "stride": [1, 1],
            "residual": [1, 1], "dropout": [0.0] * 2, "latency": False, "importance": True, "in_feat": 3,
            "buffer": 1, "stages": 1}
    return {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": 3, "output_type": "logits",
            "normalization": "LayerNorm", "segment": 500, "num_classes": 5, "rt-st-gcn": conf, "graph": dict(P.PKU_MMD)}


# name -> (streams, frames); frames >= 2 x the longest FIFO (S * (kernel - 1) + 1) of the case
CASES = {"small_v25_p3": (2, 12), "small_v2_p1": (2, 12), "small_v25_p1": (2, 12), "small_v2_p3": (2, 12),
         "wide_c256": (1, 6), "golden_stride1": (1, 20), "golden_ref_strides": (1, 36)}

# E_ref = max|restatement - oracle(fp64)| / max|oracle(fp64)| per case, recorded from
#   python -m pytest tests/test_rt_streams_bf16_cpu.py -k e_ref -s
# (the [e_ref] lines).  The GPU test's bar is 2 x these constants (DESIGN 4.18's rule for bf16 stages).
E_REF = {"small_v25_p3": 1.773e-3, "small_v2_p1": 3.139e-3, "small_v25_p1": 1.718e-3, "small_v2_p3": 2.817e-3,
         "wide_c256": 9.139e-4, "golden_stride1": 1.453e-3, "golden_ref_strides": 1.420e-3}


def _randomise(m, seed):
    """Non-trivial norms, biases and edge importance (test_gpu_rt_streams.py's recipe)."""
    sd = m.state_dict()
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if "edge_importance" in k:
            sd[k] = 1 + 0.1 * torch.randn(sd[k].shape, generator=g)
        elif ("bn_relu" in k or "residual.1" in k or "norm_in" in k) and k.endswith("weight"):
            sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
    return sd


def build_case(P, name):
    """(arch, state dict, x (streams, 3, frames, V)) of a case, on the CPU, the same on every machine."""
    B, frames = CASES[name]
    seed = 700 + sorted(CASES).index(name)
    if name.startswith("golden_"):
        d = load_golden("rt_" + name[len("golden_"):])
        arch, sd = d["arch"], sub(d, "sd/")
    else:
        if name == "wide_c256":
            arch = _wide_arch(P)
        else:
            _, v, p = name.split("_")
            arch = _small_arch(P, int(v[1:]), int(p[1:]))
        torch.manual_seed(seed)
        sd = _randomise(P.MODELS["rt-st-gcn"](rank=None, **arch), seed + 50)
        if sd["A"].shape[0] == 1:  # a dense single partition instead of the hop-0 diagonal
            g = torch.Generator().manual_seed(seed + 70)
            sd["A"] = sd["A"] + 0.3 * torch.rand(sd["A"].shape, generator=g)
    V = sd["A"].shape[-1]
    x = torch.randn(B, 3, frames, V, generator=torch.Generator().manual_seed(seed + 90))
    return arch, sd, x


# ------------------------------------------------------------------------------------------ the restatement
def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def rt_model_online_bf16(frames, sd, arch):
    """oracle.rt_model_online with rt_streams.hip's bf16 rounding points: gcn.conv's and residual.0's weights once,
    each layer's input once as it is staged for those two convs; the biases, the A-mix, the FIFO step, the norms,
    the identity residual (the UNROUNDED layer input), the ReLUs and both heads in fp32."""
    conf, kind = arch["rt-st-gcn"], arch["normalization"]
    V, A = frames.shape[-1], sd["A"]
    P = A.shape[0]
    states = [O.RtOnlineState(conf["out_ch"][i], V, conf["kernel"], conf["stride"][i]) for i in range(conf["layers"])]
    wq = {k: _bf16(v) for k, v in sd.items() if k.endswith("conv.weight") or k.endswith("residual.0.weight")}
    outs = []
    for t in range(frames.shape[2]):
        x = O.layernorm_cv(frames[:, :, t:t + 1], sd["norm_in.weight"], sd["norm_in.bias"])
        x = F.conv2d(x, sd["fcn_in.weight"], sd["fcn_in.bias"])
        for i in range(conf["layers"]):
            pre = "st_gcn.%d." % i
            cin, cout, S = conf["in_ch"][i], conf["out_ch"][i], conf["stride"][i]
            residual = bool(conf["residual"][i])
            xq = _bf16(x)
            if not residual:
                res = x * 0.0
            elif cin == cout and S == 1:
                res = x
            else:
                res = O.norm(kind, F.conv2d(xq, wq[pre + "residual.0.weight"]), sd[pre + "residual.1.weight"],
                             sd[pre + "residual.1.bias"])
            Aeff = A * sd[pre + "edge_importance"] if conf["importance"] else A
            z = F.conv2d(xq, wq[pre + "conv.weight"], sd[pre + "conv.bias"]).view(P, cout, V)
            z = torch.einsum("pcv,pvw->cw", z, Aeff)
            z = states[i].push(z).view(1, cout, 1, V)
            h = torch.relu(O.norm(kind, z, sd[pre + "bn_relu.0.weight"], sd[pre + "bn_relu.0.bias"]))
            x = torch.relu(h + res) if residual else h + res
        x = x.mean(dim=3, keepdim=True)
        outs.append(F.conv2d(x, sd["fcn_out.weight"], sd["fcn_out.bias"]).squeeze(-1))
    return torch.cat(outs, dim=2)


@contextlib.contextmanager
def _default_dtype(dt):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(prev)


def oracle_fp64(x, sd, arch):
    """The oracle's online form in fp64 (its state buffers take the default dtype), stream by stream."""
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad(), _default_dtype(torch.float64):
        return torch.cat([O.rt_model_online(x[b:b + 1].double(), sd64, arch) for b in range(x.shape[0])], dim=0)


def restatement(x, sd, arch):
    with torch.no_grad():
        return torch.cat([rt_model_online_bf16(x[b:b + 1], sd, arch) for b in range(x.shape[0])], dim=0)


def rel_err(y, ref):
    return ((y.double() - ref).abs().max() / ref.abs().max()).item()


# --------------------------------------------------------------------------------------------------- tests
def test_restatement_is_the_oracle_without_rounding(pkg, monkeypatch):
    """With the rounding switched off the restatement IS oracle.rt_model_online (same functions, same order)."""
    arch, sd, x = build_case(pkg, "small_v25_p3")
    monkeypatch.setitem(globals(), "_bf16", lambda t: t)
    with torch.no_grad():
        assert torch.equal(restatement(x[:1], sd, arch), O.rt_model_online(x[:1], dict(sd), arch))


@pytest.mark.parametrize("name", sorted(CASES))
def test_e_ref(pkg, name):
    """E_ref of the case, recomputed: the recorded constant is this number.  bf16 has 8 significant bits (unit
    roundoff 2^-9 = 2.0e-3), so E_ref sits within a small factor of that; a different CPU's fp32 sum order can flip
    single bf16 roundings of the staged inputs, which moves the max-norm by a fraction of itself, hence 25 %."""
    arch, sd, x = build_case(pkg, name)
    B, frames = CASES[name]
    conf = arch["rt-st-gcn"]
    assert frames >= 2 * max(s * (conf["kernel"] - 1) + 1 for s in conf["stride"]), "every FIFO must wrap"
    ref = oracle_fp64(x, sd, arch)
    e = rel_err(restatement(x, sd, arch), ref)
    print(f"[e_ref] {name}: {e:.3e}", flush=True)
    assert 2.0 ** -13 < e < 2.0 ** -5, "bf16 operand rounding should cost between 1e-4 and 3e-2 of max|y|"
    assert E_REF[name] is not None and abs(e - E_REF[name]) <= 0.25 * E_REF[name], (e, E_REF[name])
    # the fp32 oracle itself is orders of magnitude closer: the yardstick measures the rounding, nothing else
    with torch.no_grad():
        y32 = torch.cat([O.rt_model_online(x[b:b + 1], dict(sd), arch) for b in range(B)], dim=0)
    assert rel_err(y32, ref) < 1e-5


def test_stream_batch_dtype_argument(pkg):
    """stream_batch(B, dtype=None): the dtype is resolved before anything else, so an unsupported one is refused
    with both supported names, and a supported one gets as far as the next check, with no device."""
    sig = inspect.signature(pkg.MODELS["rt-st-gcn"].stream_batch)
    assert list(sig.parameters) == ["self", "B", "dtype"] and sig.parameters["dtype"].default is None
    arch = _small_arch(pkg, 25, 3)
    m = pkg.MODELS["rt-st-gcn"](rank=None, **arch)
    for bad in ("fp16", torch.float16, torch.float64, "int8", 16, ["bf16"]):
        with pytest.raises(RuntimeError, match=r"fp32.*bf16"):
            m.stream_batch(2, bad)
    for good in (None, "fp32", "bf16", torch.float32, torch.bfloat16):
        with pytest.raises(RuntimeError, match="prepare_benchmark"):
            m.stream_batch(2, good)
    assert "fp32" in pkg.MODELS["rt-st-gcn"].stream_batch.__doc__


def test_abi_dtype_field_and_pack_entry(pkg):
    L = pkg._lib
    lib = L.load_library()
    names = [n for n, _ in L.RtStreamsDesc._fields_]
    assert names[:6] == ["V", "L", "C0", "K", "B", "dtype"] and L.RtStreamsDesc.dtype.offset == 20
    assert L.RtStreamsDesc().dtype == 0                             # a zero-filled descriptor is fp32
    assert lib.stgcn_abi_version() == 7
    # a valid descriptor (fake non-null pointers, never dereferenced on the host) with an unknown operand type
    d = L.RtStreamsDesc(V=25, L=1, C0=8, K=4, B=4, x=64, active=64, ln_w=64, ln_b=64, w_in=64, b_in=64, w_out=64,
                        b_out=64, out=64)
    y = d.layers[0]
    y.Cin, y.Cout, y.P, y.fifo_size, y.S, y.res_mode = 8, 8, 3, 9, 1, 1
    y.A = y.wp = y.bias2d = y.ln_w = y.ln_b = y.fifo = y.acc = y.idx = 64
    for bad in (2, -1, 7):
        d.dtype = bad
        assert lib.stgcn_rt_streams(d, None) == 2                   # unsupported dtype, before any launch
    d.dtype, d.V = 1, 33
    assert lib.stgcn_rt_streams(d, None) == 1                       # the shape limits hold for bf16 too
    fn = lib.stgcn_rt_streams_pack_weight_as
    assert len(fn.argtypes) == 7
    assert fn(None, 3, 64, 64, None, 1, None) == 1
    assert fn(64, 4, 64, 64, 64, 1, None) == 1                      # more groups than partitions
    assert fn(64, 3, 64, 6, 64, 1, None) == 1                       # Cin % 4
    assert fn(64, 3, 64, 64, 64, 2, None) == 2                      # unknown dtype


@pytest.mark.parametrize("groups", [1, 3])
def test_pack_elems_formula(pkg, groups):
    """Per group [ceil(Cout/32) tiles][ceil(Cin/16) k-steps][64 lanes][8], the same count in fp32 and bf16."""
    lib = pkg._lib.load_library()
    for Cin in (4, 16, 20, 256):
        for Cout in (4, 32, 36, 256):
            n = lib.stgcn_rt_streams_pack_elems(Cout, Cin)
            assert n == -(-Cout // 32) * -(-Cin // 16) * 64 * 8
            assert groups * n == groups * -(-Cout // 32) * -(-Cin // 16) * 512
