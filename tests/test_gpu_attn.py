"""The AAGCN attention kernels alone on the MI355X (attn.hip, mode 2 of jmix.hip) against the fp64 restatement of
tests/attn_ref.py, with inputs that make the softmax peaked (so dS is not negligible) and the reference's own C fed
to the backward (a forward error can neither mask a backward error nor leak into it).

Bars: fp32 1e-4 of max|ref| (the fp32 kernel-level bar of test_gpu_kernels.py; the restatement evaluated in fp32 sits
<= 5e-6 from fp64, test_attn_ref_cpu.py); bf16-stored dtheta / dphi 2^-8 (half an ulp of the storage rounding, times
two), the fp32 C of the bf16 instantiations 1e-4 (products of bf16 values are exact in fp32).
tests/test_attn_ref_cpu.py shows that the comparison used here rejects a transposed dS, a wrong partition's coefficients, a lost T chunk, a
uniform C and another sample's coefficients at these bars.

Largest measured errors (STGCN_TEST_REPORT=1, MI355X), relative to max|ref|, next to the bar:
    fp32  C       3.9e-7  (1e-4)   P = 4, V = 32; atomic route 2.9e-7, slab route 2.5e-7, padded rows 2.8e-7
    fp32  dtheta  8.2e-7  (1e-4)   ce = 64; stacked halves 2.8e-7, padded rows 2.2e-7, under autograd 3.3e-7
    fp32  dphi    6.8e-7  (1e-4)   ce = 64; stacked halves 2.9e-7, padded rows 2.1e-7, under autograd 2.7e-7
    bf16  C       3.5e-7  (1e-4)   fp32 out
    bf16  dtheta  2.5e-3  (2^-8 = 3.9e-3)   the storage rounding alone
    bf16  dphi    2.4e-3  (2^-8 = 3.9e-3)
Every library call on these shapes returned STGCN_OK, in both dtypes.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [R.shape_id(s) for s in R.SHAPES]
BIG = 1e30  # what the padding channels of the inputs hold: finite, and fatal to any sum it reaches


@pytest.fixture(scope="module")
def K(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return pkg.native


def rows(x, ld=None, dtype=torch.float32, fill=0.0, buf=None, col0=0):
    """The logical (N, CH, T, V) CPU tensor ``x`` as channels-last rows on the device: a view of channels
    col0 .. col0+CH of an [N][T][V][ld] buffer whose other channels hold ``fill``."""
    N, CH, T, V = x.shape
    if buf is None:
        buf = torch.full((N, T, V, ld or CH), fill, dtype=dtype, device=DEV)
    buf[..., col0:col0 + CH] = x.permute(0, 2, 3, 1).to(DEV, dtype)
    return buf.permute(0, 3, 1, 2)[:, col0:col0 + CH]


def dev_case(case):
    return rows(case.theta), rows(case.phi), case.C.to(DEV, torch.float32).contiguous(), case.dC.to(DEV)


def lib_scores(L, th, ph, ld, shape, dtype, work=True):
    """stgcn_attn_scores called directly; ``work`` False: NULL workspace (the atomic route)."""
    N, P, ce, T, V = shape
    C = torch.full((N, P, V, V), float("nan"), device=DEV)
    ws = torch.empty(max(1, L.lib().stgcn_attn_scores_workspace(N, T, V, P) // 4), device=DEV) if work else None
    rc = L.lib().stgcn_attn_scores(th.data_ptr(), ph.data_ptr(), ld, N, T, V, P, ce, C.data_ptr(), L.ptr(ws),
                                   L.dtype_code(dtype), L.stream())
    torch.cuda.synchronize()
    return rc, C


def lib_bwd(L, th, ph, ld, shape, C, dC, dth, dph, dtype):
    N, P, ce, T, V = shape
    dS = torch.empty_like(C)
    rc = L.lib().stgcn_attn_bwd(th.data_ptr(), ph.data_ptr(), ld, N, T, V, P, ce, C.data_ptr(), dC.data_ptr(),
                                dS.data_ptr(), dth.data_ptr(), dph.data_ptr(), L.dtype_code(dtype), L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_attn_scores_fp32(K, shape):
    case = R.attn_case(shape)
    th, ph, _, _ = dev_case(case)
    R.attn_compare({"C": K.attn_scores(th, ph, case.P)}, case, name="fp32 " + R.shape_id(shape))


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_attn_bwd_fp32(K, shape):
    case = R.attn_case(shape)
    th, ph, C, dC = dev_case(case)
    dth, dph = K.attn_bwd(th, ph, case.P, C, dC)
    assert dth.shape == dph.shape == case.theta.shape
    R.attn_compare({"dtheta": dth, "dphi": dph}, case, name="fp32 " + R.shape_id(shape))


@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=IDS[:2])
def test_attn_stacked_halves(K, shape):
    """theta and phi as the two channel halves of one row buffer (ld = 2*CH, the bf16 models' route): the same bits as
    two separate tensors, and the gradients come back as the two halves of one buffer."""
    case = R.attn_case(shape)
    N, P, ce, T, V = shape
    CH = case.CH
    th, ph, C, dC = dev_case(case)
    buf = torch.empty((N, T, V, 2 * CH), device=DEV)
    th2 = rows(case.theta, buf=buf)
    ph2 = rows(case.phi, buf=buf, col0=CH)
    assert K.rows_ld(th2) == K.rows_ld(ph2) == 2 * CH and ph2.data_ptr() - th2.data_ptr() == CH * 4
    assert torch.equal(K.attn_scores(th2, ph2, P), K.attn_scores(th, ph, P))
    dth, dph = K.attn_bwd(th, ph, P, C, dC)
    dth2, dph2 = K.attn_bwd(th2, ph2, P, C, dC)
    assert dph.data_ptr() - dth.data_ptr() != CH * 4  # the separate-tensor route: two buffers
    assert dph2.data_ptr() - dth2.data_ptr() == CH * 4
    assert K.rows_ld(dth2) == K.rows_ld(dph2) == 2 * CH
    assert torch.equal(dth2, dth) and torch.equal(dph2, dph)
    R.attn_compare({"dtheta": dth2, "dphi": dph2}, case, name="stacked " + R.shape_id(shape))


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[3], R.SHAPES[6]], ids=[IDS[0], IDS[3], IDS[6]])
def test_attn_scores_atomic_and_slab_routes(K, pkg, shape):
    """work == NULL adds the T chunks' partials with fp32 atomics (same bar; 5 chunks at the first shape, one at the
    others); with a workspace they are summed in a fixed order, so two runs agree bit for bit."""
    L = pkg._lib
    case = R.attn_case(shape)
    th, ph, _, _ = dev_case(case)
    rc, C_atomic = lib_scores(L, th, ph, case.CH, shape, torch.float32, work=False)
    assert rc == 0
    R.attn_compare({"C": C_atomic}, case, name="atomic " + R.shape_id(shape))
    rc1, C1 = lib_scores(L, th, ph, case.CH, shape, torch.float32)
    rc2, C2 = lib_scores(L, th, ph, case.CH, shape, torch.float32)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(C1, C2)
    R.attn_compare({"C": C1}, case, name="slab " + R.shape_id(shape))


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[3], R.SHAPES[4], R.SHAPES[8]],
                         ids=[IDS[0], IDS[3], IDS[4], IDS[8]])
def test_attn_padding_channels(K, pkg, shape):
    """ld > CH with separate tensors: the channels past CH of theta / phi (1e30 here) reach neither C nor the
    gradients, and those of dtheta / dphi are left as they were (jmix's masked last block at the first three shapes,
    the gather mix at the last)."""
    L = pkg._lib
    case = R.attn_case(shape)
    CH, ld = case.CH, case.CH + 4
    N, P, ce, T, V = shape
    th, ph = rows(case.theta, ld, fill=BIG), rows(case.phi, ld, fill=BIG)
    C, dC = case.C.to(DEV, torch.float32).contiguous(), case.dC.to(DEV)
    rc, C_got = lib_scores(L, th, ph, ld, shape, torch.float32)
    assert rc == 0
    R.attn_compare({"C": C_got}, case, name="padded " + R.shape_id(shape))
    dth = torch.full((N, T, V, ld), -7.0, device=DEV)
    dph = torch.full((N, T, V, ld), -9.0, device=DEV)
    assert lib_bwd(L, th, ph, ld, shape, C, dC, dth, dph, torch.float32) == 0
    assert bool((dth[..., CH:] == -7.0).all()) and bool((dph[..., CH:] == -9.0).all())
    R.attn_compare({"dtheta": dth[..., :CH].permute(0, 3, 1, 2), "dphi": dph[..., :CH].permute(0, 3, 1, 2)}, case,
                   name="padded " + R.shape_id(shape))


@pytest.mark.parametrize("stacked", [False, True], ids=["separate", "stacked"])
def test_attention_function_autograd(K, pkg, stacked):
    """layer_fn.AttentionFunction under autograd with requires_grad leaves, on both routes of native.attn_bwd."""
    LF = pkg.layer_fn
    shape = R.SHAPES[0]
    case = R.attn_case(shape)
    CH = case.CH
    if stacked:
        buf = torch.empty((shape[0], shape[3], shape[4], 2 * CH), device=DEV)
        th, ph = rows(case.theta, buf=buf), rows(case.phi, buf=buf, col0=CH)
    else:
        th, ph = rows(case.theta), rows(case.phi)
    th, ph = th.detach().requires_grad_(True), ph.detach().requires_grad_(True)
    C = LF.AttentionFunction.apply(th, ph, case.P, torch.float32)
    (C * case.dC.to(DEV)).sum().backward()
    R.attn_compare({"C": C, "dtheta": th.grad, "dphi": ph.grad}, case, name="autograd stacked=%d" % stacked)


# (shape index, ld - CH): the first, fourth and eighth shapes with dense rows (bf16 rows of 36 channels are not
# 16-B aligned, so the fourth takes the gather mix there), and the fourth with rows padded to 40 channels, which
# jmix serves: three partitions in one block and a 16-B unit that straddles the end of the row's channels
@pytest.mark.parametrize("idx,pad", [(0, 0), (3, 0), (3, 4), (7, 0)])
def test_attn_bf16_instantiations(K, pkg, idx, pad):
    """The bf16 instantiations through the C-ABI, against fp64 on the bf16-rounded theta / phi."""
    L = pkg._lib
    shape = R.SHAPES[idx]
    case = R.attn_case(shape, True)
    N, P, ce, T, V = shape
    CH, ld = case.CH, case.CH + pad
    bf = torch.bfloat16
    th, ph = rows(case.theta, ld, bf, fill=BIG), rows(case.phi, ld, bf, fill=BIG)
    assert torch.equal(th.float().cpu(), case.theta)  # the rounded values are what the device holds
    name = "bf16 %s ld+%d" % (R.shape_id(shape), pad)
    rc, C_got = lib_scores(L, th, ph, ld, shape, bf)
    assert rc == 0, f"stgcn_attn_scores returned {rc} for a documented shape"
    R.attn_compare({"C": C_got}, case, name=name)
    C, dC = case.C.to(DEV, torch.float32).contiguous(), case.dC.to(DEV)
    dth = torch.full((N, T, V, ld), -7.0, dtype=bf, device=DEV)
    dph = torch.full((N, T, V, ld), -9.0, dtype=bf, device=DEV)
    rc = lib_bwd(L, th, ph, ld, shape, C, dC, dth, dph, bf)
    assert rc == 0, f"stgcn_attn_bwd returned {rc} for a documented shape"
    assert bool((dth[..., CH:] == -7.0).all()) and bool((dph[..., CH:] == -9.0).all())
    R.attn_compare({"dtheta": dth[..., :CH].permute(0, 3, 1, 2), "dphi": dph[..., :CH].permute(0, 3, 1, 2)}, case,
                   rel_grad=R.BF16_STORE_REL, name=name)
