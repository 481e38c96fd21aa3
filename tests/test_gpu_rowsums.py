"""The row reductions of norm.hip alone on the MI355X: stgcn_rowgroup_sum (the GCN bias gradient's per-joint column
sums, shared and per sample), stgcn_pool_rows / stgcn_unpool_rows (every model's head and its gradient), against fp64
sums over the values as stored (bf16 inputs are rounded first).

Bars, relative to max|ref|: fp32 outputs 1e-5 (test_amix's bar: fp32 sums of at most a few hundred terms); outputs
stored as bf16 (pool / unpool of bf16 rows) 2^-8, half an ulp of the storage rounding times two.

Largest measured errors (STGCN_TEST_REPORT=1, MI355X), relative to max|ref|, next to the bar:
    rowgroup_sum  fp32 rows  1.0e-7 shared, 7.4e-8 per sample  (1e-5)
    rowgroup_sum  bf16 rows  4.4e-8 shared, 4.7e-8 per sample  (1e-5)   fp32 out
    pool_rows     fp32 1.8e-7 (1e-5)    bf16 2.4e-3 (2^-8 = 3.9e-3)
    unpool_rows   fp32 4.2e-8 (1e-5)    bf16 3.0e-3 (2^-8)
    PoolFunction  fp32 out 1.4e-7, dx 5.0e-8 (1e-5)    bf16 out 1.8e-3, dx 3.3e-3 (2^-8)
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_REL = 1e-5
BF16_STORE_REL = 2.0 ** -8
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["fp32", "bf16"]
BIG = 1e30  # padding channels of the inputs: finite, and fatal to any sum they reach

# (N, T, V, C): C = 6, 10 take the scalar loads in both dtypes, 24 the 16-B loads in both, 64 likewise; T = 37 leaves a
# one-frame last block of the per-sample grid (4 frames per block), T = 5 and 1 are below one four-in-flight round
ROWGROUP_SHAPES = [(2, 37, 25, 64), (3, 5, 18, 24), (1, 1, 25, 6), (2, 9, 3, 10)]
# (N, R, C): C = 96 a partial second 64-channel block; 52 = whole 16-B units in fp32, a partial one in bf16 (where
# only the rows padded to 56 channels are 16-B multiples; dense bf16 rows of 52 take the scalar loads); 6 all scalar; R = 130 past one four-in-flight round of the 16 (fp32) / 32 (bf16) row groups, R = 25, 3, 1 below the groups
POOL_SHAPES = [(2, 7 * 25, 256), (3, 25, 96), (2, 130, 52), (1, 1, 6), (4, 3, 64)]
# row stride - C: dense; padded keeping 16-B rows; padded by 4 (C = 52 in bf16 has 16-B rows only then: six whole
# units and a partial one); padded to rows that are not 16-B multiples (scalar loads)
POOL_PADS = [0, 8, 4, 2]


@pytest.fixture(scope="module")
def K(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return pkg.native


def draw(shape, seed, dtype):
    """Seeded CPU draw, rounded to ``dtype`` (returned in fp32: the values as stored)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).float()


def rows(x, ld, dtype, fill=BIG):
    """Logical (N, C, T, V) CPU tensor -> channels-last device rows with row stride ld (padding channels: fill)."""
    N, C, T, V = x.shape
    buf = torch.full((N, T, V, ld), fill, dtype=dtype, device=DEV)
    buf[..., :C] = x.permute(0, 2, 3, 1).to(DEV, dtype)
    return buf.permute(0, 3, 1, 2)[:, :C]


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("N,T,V,C", ROWGROUP_SHAPES)
def test_rowgroup_sum(K, N, T, V, C, dtype, per_sample, pad):
    x = draw((N, C, T, V), 11, dtype)
    xd = rows(x, C + pad, dtype)
    x64 = x.double().permute(0, 2, 3, 1)  # [N][T][V][C]
    ref = x64.sum(dim=1) if per_sample else x64.sum(dim=(0, 1))
    name = "rowgroup %s N%d T%d V%d C%d ld+%d %s" % ("per-sample" if per_sample else "shared", N, T, V, C, pad,
                                                      "bf16" if dtype == torch.bfloat16 else "fp32")
    S = K.rowgroup_sum(xd, N * T * V, C, V, per_sample=per_sample)
    assert S.dtype == torch.float32 and S.shape == ref.shape
    assert_close(S, ref, FP32_REL, name)
    # the += contract: into a non-zero out
    out0 = draw(tuple(ref.shape), 12, torch.float32)
    out = out0.to(DEV)
    S2 = K.rowgroup_sum(xd, N * T * V, C, V, per_sample=per_sample, out=out)
    assert S2.data_ptr() == out.data_ptr()
    assert_close(out, out0.double() + ref, FP32_REL, name + " +=")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_rowgroup_sum_bad_shape(K, pkg, dtype):
    """M % G != 0 (and a per-sample period that is no multiple of G) is refused before any launch."""
    L = pkg._lib
    N, T, V, C = 2, 3, 5, 8
    xd = rows(draw((N, C, T, V), 13, dtype), C, dtype)
    M = N * T * V
    S = torch.full((N, V, C), 3.0, device=DEV)
    work = torch.empty(max(1, L.lib().stgcn_rowgroup_sum_workspace(M, C, V, 0)) + 4096, device=DEV)
    for m, period in ((M - 1, 0), (M, T * V - 1), (M, M - V)):
        rc = L.lib().stgcn_rowgroup_sum(xd.data_ptr(), C, m, C, V, period, S.data_ptr(), work.data_ptr(),
                                        L.dtype_code(dtype), L.stream())
        assert rc == 1, f"M {m} period {period}: returned {rc}"  # STGCN_EBADSHAPE
    torch.cuda.synchronize()
    assert bool((S == 3.0).all())
    with pytest.raises(RuntimeError, match="rowgroup_sum"):
        K.rowgroup_sum(xd, M - 1, C, V)


@pytest.mark.parametrize("pad", POOL_PADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("N,R,C", POOL_SHAPES)
def test_pool_rows(K, N, R, C, dtype, pad):
    x = draw((N, C, R, 1), 21, dtype)
    xd = rows(x, C + pad, dtype)
    ref = x.double().mean(dim=(2, 3), keepdim=True)
    out = K.pool_rows(xd, N, R, C)
    assert out.dtype == dtype and out.shape == (N, C, 1, 1)
    bf = dtype == torch.bfloat16
    assert_close(out.float(), ref, BF16_STORE_REL if bf else FP32_REL,
                 "pool N%d R%d C%d ld+%d %s" % (N, R, C, pad, "bf16" if bf else "fp32"))


@pytest.mark.parametrize("pad", POOL_PADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("N,R,C", POOL_SHAPES)
def test_unpool_rows(K, N, R, C, dtype, pad):
    """dx[m] = dp[m / R] / R over M = N*R rows; the padding channels of dx are left as they were."""
    dp = draw((N, C, 1, 1), 22, dtype)
    dpd = rows(dp, C + pad, dtype)
    ld = C + pad
    dx = torch.full((N, R, 1, ld), -7.0, dtype=dtype, device=DEV)
    out = K.unpool_rows(dpd, R, C, N * R, dx.permute(0, 3, 1, 2)[:, :C])
    ref = (dp.double() / R).expand(N, C, R, 1)
    bf = dtype == torch.bfloat16
    assert_close(out.float(), ref, BF16_STORE_REL if bf else FP32_REL,
                 "unpool N%d R%d C%d ld+%d %s" % (N, R, C, pad, "bf16" if bf else "fp32"))
    assert bool((dx[..., C:] == -7.0).all())


@pytest.mark.parametrize("joints_only", [False, True], ids=["all-rows", "joints-only"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_pool_function_autograd(K, pkg, dtype, joints_only):
    """layer_fn.PoolFunction (the models' heads) under autograd, both modes, against avg_pool2d in fp64."""
    LF = pkg.layer_fn
    N, C, T, V = 2, 24, 5, 18
    x = draw((N, C, T, V), 23, dtype)
    kernel = (1, V) if joints_only else (T, V)
    xr = x.double().requires_grad_(True)
    ref = F.avg_pool2d(xr, kernel)
    dp = draw(tuple(ref.shape), 24, dtype)
    ref.backward(dp.double())
    xd = x.to(DEV, dtype).requires_grad_(True)
    out = LF.PoolFunction.apply(xd, dtype, joints_only)
    assert out.shape == ref.shape and out.dtype == dtype
    out.backward(dp.to(DEV, dtype))
    bf = dtype == torch.bfloat16
    rel = BF16_STORE_REL if bf else FP32_REL
    name = "PoolFunction %s %s" % ("joints-only" if joints_only else "all-rows", "bf16" if bf else "fp32")
    assert_close(out.float(), ref, rel, name + " out")
    assert_close(xd.grad.float(), xr.grad, rel, name + " dx")
