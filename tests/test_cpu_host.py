"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol include/stgcn_amd.h
declares, the host-side Graph matches the reference's, modules keep the reference's API and
state_dict layout, and the product refuses to run without the HIP device (no CPU fallback)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def test_header_symbols_exported(pkg):
    hdr = open(f"{ROOT}/include/stgcn_amd.h").read()
    declared = set(re.findall(r"^\s*(?:int|long)\s+(stgcn_\w+)\s*\(", hdr, flags=re.M))
    assert declared, "no declarations parsed"
    lib = pkg._lib.load_library()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared but not exported"
    assert declared == set(pkg._lib.EXPORTS), "ctypes binding and header disagree"
    assert lib.stgcn_abi_version() == pkg._lib.ABI_VERSION
    m = re.search(r"^#define STGCN_ABI_VERSION (\d+)", hdr, flags=re.M)
    assert m and int(m.group(1)) == pkg._lib.ABI_VERSION, "header and ctypes binding name different ABI versions"


def test_abi_rejects_bad_args_without_gpu(pkg):
    L = pkg._lib
    lib = L.load_library()
    d = L.ConvDesc()  # all-null descriptor: validated on the host, no launch
    assert lib.stgcn_conv_rows(d, 0, None) == 1
    assert lib.stgcn_conv_rows(d, 7, None) == 2
    assert lib.stgcn_conv_rows_col_tile(64) == 64 and lib.stgcn_conv_rows_col_tile(256) == 128
    # stgcn_tconv_frame's contract (header): 16 < V <= 25 and 16-B aligned rows; anything else is refused on the
    # host before a launch (the callers route those shapes to stgcn_conv_rows)
    d = L.ConvDesc(in_=16, out=16, w_frag=16, N=2, T_in=8, T_out=8, V=25, Cin=64, Cout=64, Cin_pad=64, Cout_pad=64,
                   Kt=9, stride=1, pad=4, trans=1, in_ld=64, out_ld=68)
    assert lib.stgcn_tconv_frame(d, None) == 1          # out_ld % 8 == 4
    d.out_ld, d.V = 64, 32
    assert lib.stgcn_tconv_frame(d, None) == 1          # V > 25: no reference skeleton, no kernel form
    g = L.GconvWgradDesc(phase=3)                       # phase outside {0, 1, 2}
    assert lib.stgcn_gconv_wgrad(g, 1, None) == 1
    r = L.RtFrameDesc()                                 # null pointers: refused before the barrier-counter memset
    assert lib.stgcn_rt_frame(r, None) == 1


# (plan, dtype, Cin, Cout, NT) -> workspace bytes (without, with row sums) at V = 25 and the PKU-MMD graph's J = 5:
# one shape per plan of the graph-conv weight gradient.  The byte counts were recorded from the library as it was
# before the plan moved into one function (gconv_wgrad.hip, plan_wgrad); they pin each shape's kernel family, row
# parts and buffer layout.
WGRAD_PLAN_BYTES = [
    ("fp32", 0, 64, 64, 320, (0, 0)),
    ("per-pair kernel", 1, 24, 40, 320, (1440000, 1440000)),
    ("register-staged joint-grouped", 1, 64, 128, 320, (40960000, 41088000)),
    ("ring with slab, 64 -> 64", 1, 64, 64, 320, (20480000, 20544000)),
    ("ring with slab, 128 -> 256", 1, 128, 256, 320, (32768000, 32819200)),
    ("ring direct split, 192 -> 256", 1, 192, 256, 320, (49306800, 49306800)),
    ("ring direct split, 256 -> 128", 1, 256, 128, 14, (32871200, 32871200)),
    ("wide, one row part", 1, 256, 256, 18, (0, 0)),
    ("wide, two row parts", 1, 256, 256, 600, (78848800, 78848800)),
]


def test_gconv_wgrad_plan_workspace(pkg):
    L = pkg._lib
    lib = L.load_library()
    sup = pkg.native.GraphSupport(torch.tensor(pkg.Graph(**pkg.PKU_MMD).A, dtype=torch.float32))
    assert (sup.V, sup.J) == (25, 5)
    for plan, dtype, Cin, Cout, NT, expect in WGRAD_PLAN_BYTES:
        for rowsum, nbytes in zip((None, 16), expect):  # the size depends only on whether row sums are asked for
            d = L.GconvWgradDesc(NT=NT, V=sup.V, J=sup.J, Cin=Cin, Cout=Cout, x_ld=Cin, dy_ld=Cout, rowsum=rowsum)
            assert lib.stgcn_gconv_wgrad_workspace(d, dtype) == nbytes, (plan, bool(rowsum))


@pytest.mark.parametrize("key,name", [("pku_mmd", "pku-mmd"), ("ntu_rgbpd", "ntu"), ("openpose", "op"),
                                      ("coco", "coco"), ("imu_fogit_ABCD", "imu"), ("hugadb", "hugadb")])
def test_graph_golden(pkg, key, name):
    g = np.load(f"{ROOT}/tests/golden/graphs.npz")
    V, center = g["meta/" + key]
    edge = g["edge/" + key].tolist()
    G = pkg.Graph(int(V), edge, int(center))
    np.testing.assert_allclose(G.A, g["A/" + key], rtol=0, atol=1e-12)
    np.testing.assert_allclose(G.get_adjacency_raw(), g["Araw/" + key], rtol=0, atol=0)
    for strat in ("distance", "uniform"):
        np.testing.assert_allclose(pkg.Graph(int(V), edge, int(center), strategy=strat).A,
                                   g["A_%s/%s" % (strat, key)], rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", ["stgcn_bn_1layer", "stgcn_bn_1layer_t64", "stgcn_ln_1layer_t64", "stgcn_bn_9layer_narrow",
                                  "stgcn_ln_9layer_narrow_k69"])
def test_model_state_dict_layout(pkg, case):
    d = load_golden("model_" + case)
    m = pkg.MODELS["st-gcn"](rank=None, **d["arch"])
    ref_keys = {k[3:]: v.shape for k, v in d.items() if k.startswith("sd/")}
    ours = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert set(ours) == set(ref_keys)
    for k, s in ref_keys.items():
        assert ours[k] == tuple(s), k
    m.load_state_dict({k[3:]: v for k, v in d.items() if k.startswith("sd/")}, strict=True)


def test_config2_model_size(pkg):
    arch = {"strategy": "spatial", "graph": pkg.PKU_MMD, "in_feat": 3, "normalization": "BatchNorm",
            "num_classes": 52, "st-gcn": {"in_feat": 3, "layers": 9, "kernel": 9, "importance": True,
                                           "in_ch": [64, 64, 64, 64, 128, 128, 128, 256, 256],
                                           "out_ch": [64, 64, 64, 128, 128, 128, 256, 256, 256],
                                           "stride": [1, 1, 1, 2, 1, 1, 2, 1, 1], "residual": [1] * 9,
                                           "dropout": [0] * 9}}
    m = pkg.MODELS["st-gcn"](rank=None, **arch)
    # as_is ST-GCN = 3 057 205 fp32 params, 96 state_dict keys
    assert sum(p.numel() for p in m.parameters()) == 3057205
    assert len(m.state_dict()) == 96


def test_no_cpu_fallback(pkg):
    layer = pkg.StgcnLayer(8, 8, (9, 25), 3, 25, normalization="BatchNorm")
    A = torch.tensor(pkg.Graph(**pkg.PKU_MMD).A, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="HIP device only"):
        layer(torch.randn(1, 8, 4, 25), A)


def test_bench_multi_gpu_launch_rejected_cleanly_without_devices():
    """`bench.py --gpus N` starts its own ranks only when N HIP devices are visible; here (no GPU) it
    must refuse with a message, not a traceback; a launcher's WORLD_SIZE must agree with --gpus."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("devices present")
    bench = os.path.join(ROOT, "bench.py")
    r = subprocess.run([sys.executable, bench, "--gpus", "2", "--steps", "1"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "needs 2 HIP devices" in r.stderr and "Traceback" not in r.stderr
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, bench, "--gpus", "0", "--steps", "1"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=3" in r.stderr and "Traceback" not in r.stderr


def test_bench_dump_outputs_float32_and_bounded(tmp_path, monkeypatch):
    """bench.py --dump-outputs writes float32 .npy files; over the size limit every array is cut to the same
    fixed (seed 0) sample of its elements, so two runs keep the same ones."""
    import bench
    arrays = {"a": torch.arange(1000, dtype=torch.float64).reshape(10, 100),
              "b.w": torch.ones(7, dtype=torch.bfloat16), "s": torch.tensor(2.5)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    got = {k: np.load(tmp_path / "whole" / f"{k}.npy", allow_pickle=False) for k in arrays}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["a"].shape == (10, 100) and np.array_equal(got["a"].ravel(), np.arange(1000)) and got["s"] == 2.5
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1024)
    cut = []
    for d in ("cut1", "cut2"):
        bench.dump_outputs(str(tmp_path / d), arrays)
        cut.append({k: np.load(tmp_path / d / f"{k}.npy", allow_pickle=False) for k in arrays})
    assert sum(v.nbytes for v in cut[0].values()) <= 1024
    assert 0 < cut[0]["a"].size < 1000 and set(cut[0]["a"]) <= set(range(1000)) and cut[0]["s"] == 2.5
    assert all(np.array_equal(cut[0][k], cut[1][k]) for k in arrays)


class _FakeDev:
    def __init__(self, i):
        self.index = i


class _FakeCuda:
    """Stands in for a CUDA tensor on device ``i`` (the guard only reads .is_cuda and .device.index)."""

    def __init__(self, i):
        self.is_cuda = True
        self.device = _FakeDev(i)


def test_device_guard_follows_tensor(pkg, monkeypatch):
    """SURVEY 8(b) threading: every autograd Function runs under native.device_of(first CUDA input), so a
    launch takes the tensor's device (its current stream, its allocations) even when the caller has another
    device current, and the caller's device is restored afterwards (also on error)."""
    K = pkg.native
    state = {"cur": 0, "sets": []}
    monkeypatch.setattr(torch._C, "_cuda_getDevice", lambda: state["cur"])

    def setdev(i):
        state["sets"].append(i)
        state["cur"] = i
    monkeypatch.setattr(torch._C, "_cuda_setDevice", setdev)
    seen = []
    with K.device_of(_FakeCuda(1)):
        seen.append(state["cur"])
    assert seen == [1] and state["cur"] == 0 and state["sets"] == [1, 0]
    state["sets"].clear()
    with K.device_of(_FakeCuda(0)):  # already current: no device switch at all
        pass
    assert state["sets"] == []
    with pytest.raises(ValueError):
        with K.device_of(_FakeCuda(3)):
            raise ValueError("inside")
    assert state["cur"] == 0

    @K.on_tensor_device
    class Fn:
        @staticmethod
        def forward(ctx, x, y):
            return state["cur"]

        @staticmethod
        def backward(ctx, g):
            return state["cur"]

    # the decorator picks the first CUDA torch.Tensor argument: a CPU tensor that reports cuda:2
    t = torch.zeros(1)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: _FakeDev(2)))
    assert Fn.forward(None, 5, t) == 2 and Fn.backward(None, t) == 2 and state["cur"] == 0
    # every autograd Function of the package is wrapped
    import inspect
    for mod in (pkg.layer_fn, pkg.loss):
        for name, cls in inspect.getmembers(mod, inspect.isclass):
            if issubclass(cls, torch.autograd.Function) and cls.__module__ == mod.__name__:
                assert cls.forward.__wrapped__ is not None, name


def test_prep_plan_builds_and_validates(pkg):
    """The one-launch weight preparation of the config-2 model (stgcn.Model._prepared -> native.PrepPlan):
    the per-layer jobs are recorded and validated on the host (stgcn_prep_check fills each job's thread
    count) — 9 layers x (graph conv fwd + data grad, temporal conv fwd + data grad) + 2 residual convs x 2 +
    the head's 2 x 2, where the stride-2 temporal packs take two jobs each (plain + folded image), and the frame
    kernel's graph-conv forward two (weight image + bias through A)."""
    import bench
    m = pkg.MODELS["st-gcn"](rank=None, **dict(bench.ARCH, graph=pkg.PKU_MMD)).set_compute_dtype("bf16")
    K, LF = pkg.native, pkg.layer_fn
    plan = K.PrepPlan(torch.device("cpu"))
    layers = []
    for i, gcn in enumerate(m.gcn_networks):
        gcn.bind_graph(m.A)
        layers.append(LF.plan_layer_packs(plan, gcn, m.A, m.edge_importance[i], torch.bfloat16))
    head = (LF.plan_conv1x1_packs(plan, m.fcn_in.weight, torch.bfloat16),
            LF.plan_conv1x1_packs(plan, m.fcn_out.weight, torch.bfloat16))
    plan.finalize()
    assert all(p is not None for p in layers)
    # per layer: effective weights both ways, the bias through A (kind 3), temporal packs both ways
    assert plan.njobs == 9 * 5 + 2 * 2 + 2 * 2 + 2 * 2
    assert plan.nblocks > 0
    # frag images where the kernels expect them
    assert layers[0].wt[0].frag_stride == 1 and layers[3].wt[0].frag_stride == 2 and layers[3].wtT[0].frag_stride == 2
    assert head[0][0][1] == 64 and head[0][0][2] == 32


def _c_layout(tmp_path, structs):
    """sizeof and offsetof of every field of each named header struct, as gcc lays them out."""
    import ctypes
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "stgcn_amd.h")}"',
             'int main(void) {']
    expect = []
    for cname, cls in structs.items():
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        expect.append(ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            cf = "in" if fname == "in_" else fname
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {cf}));')
            expect.append(getattr(cls, fname).offset)
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    return got, expect


def test_integration_stub_matches_header(tmp_path):
    """The reference-side ctypes binding INTEGRATION.md shows a maintainer (its GconvDesc) has exactly the size and
    field offsets of include/stgcn_amd.h's stgcn_gconv_desc: the stub is executed from the markdown, so a
    descriptor change not mirrored there fails here (round-5 verdict: the stub was 24 B short)."""
    import ctypes
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^class GconvDesc\(ctypes\.Structure\):.*?(?=^\S)", text, flags=re.M | re.S)
    assert m, "INTEGRATION.md no longer shows the GconvDesc stub"
    ns = {"ctypes": ctypes}
    exec(m.group(0), ns)
    names = [f for f, _ in ns["GconvDesc"]._fields_]
    hdr = open(os.path.join(ROOT, "include", "stgcn_amd.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} stgcn_gconv_desc;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    hfields = [("in_" if f == "in" else f) for decl in body.split(";") if decl.strip()
               for f in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip().split(None, 1)[1] if "*" not in decl
                                   else decl.strip().rsplit("*", 1)[1])]
    assert names == hfields, f"stub fields {names} != header fields {hfields}"
    got, expect = _c_layout(tmp_path, {"stgcn_gconv_desc": ns["GconvDesc"]})
    assert got == expect


def test_descriptor_layouts_match_header(pkg, tmp_path):
    """Every ctypes descriptor of _lib.py has the size and field offsets the C compiler gives the struct of
    include/stgcn_amd.h (the boundary's pointer-and-size structs; a field appended on one side only would make
    the library read garbage).  Compiled with gcc on the host: no GPU, no HIP headers (the header is plain C)."""
    L = pkg._lib
    structs = {"stgcn_conv_desc": L.ConvDesc, "stgcn_wgrad_desc": L.WgradDesc, "stgcn_amix_desc": L.AmixDesc,
               "stgcn_gconv_desc": L.GconvDesc,
               "stgcn_gconv_wgrad_desc": L.GconvWgradDesc, "stgcn_bn_bwd_desc": L.BnBwdDesc,
               "stgcn_layer_fused_desc": L.LayerFusedDesc, "stgcn_prep_job": L.PrepJob,
               "stgcn_adam_entry": L.AdamEntry, "stgcn_rt_layer": L.RtLayer, "stgcn_rt_frame_desc": L.RtFrameDesc}
    got, expect = _c_layout(tmp_path, structs)
    assert got == expect
