"""norm_ref.py checked without a GPU.

1. The float64 references against independent ground truth: torch autograd through F.batch_norm(training=True),
   oracle.stgcn_oracle.layernorm_cv in float64, and the reference-generated ``norms`` fixture.
2. Planted slips: each is applied to a copy of a reference output and handed to the comparison the GPU modules use
   (norm_ref.compare at the GPU bar); every one must be rejected.  The LN backward's E-for-(E-1) slip changes dx by
   |xhat * k2| / E: it is shown at E = V*C = 150 and 400 (the scalar C = 6 and the C = 16 routes); at E >= 6400 it is
   below the fp32 backward bar of 1e-4, which is what that bar means, not a gap of the helper.
3. The documented statistics algorithm emulated in float32 numpy (per-thread shifted sums, fp32 (n, mean, M2), fp64
   power sums) on the hard-statistics inputs: it fixes the |mean| / std ratio the GPU tests use from the algorithm,
   not from the code under test.  The bar is 1e-5 of max|mean| and of max|rstd|; the emulation must keep 10x to spare.
       BN fp32 rows (C = 64, M = 5000, 4 rows per thread): ratio 1e3 -> rstd 1.6e-6 (too close), ratio 300 -> 8.2e-7
       BN bf16 rows (2 rows per thread, so more of M2 passes through the fp32 merges of fp32-rounded means):
           ratio 1e3 -> 1.3e-5, 300 -> 1.3e-6, 100 -> 1.8e-7
       LN (fp32, E = 1600): ratio 1e3 -> mean 3.0e-8, rstd 1.1e-7
   so BN_HARD_RATIO = 300 (fp32) / 100 (bf16) and LN_HARD_RATIO = 1e3; means stay below 1e-7 everywhere.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from conftest import load_golden, sub
from oracle import stgcn_oracle as O

BN_HARD_RATIO = R.BN_HARD_RATIO
LN_HARD_RATIO = R.LN_HARD_RATIO


def rejected(got, ref, rel, name, scale_floor=0.0):
    with pytest.raises(AssertionError):
        R.compare(got, ref, rel, name, scale_floor)


# ------------------------------------------------------------------------------------------ ground truth
def _bn_case(M=300, C=12, seed=1):
    x = R.draw((M, C), seed, R.F32, 2.0, 1.0)
    g = torch.rand(C, generator=R.gen(seed + 1), dtype=torch.float64) + 0.5
    b = torch.randn(C, generator=R.gen(seed + 2), dtype=torch.float64)
    return x, g, b


@pytest.mark.parametrize("mode", ["none", "identity", "bn2"])
def test_bn_refs_against_autograd(mode):
    """Statistics, apply and backward (sums, out1, out2, column sums) == autograd of relu(BN(u) + res) in float64."""
    M, C = 300, 12
    u, g, b = _bn_case(M, C, 1)
    r, gr, br = _bn_case(M, C, 5)
    dy = R.draw((M, C), 9, R.F32)
    ut, rt = u.clone().requires_grad_(True), r.clone().requires_grad_(True)
    gt, bt = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    nchw = lambda t: t.t().reshape(1, C, M, 1)
    pre = F.batch_norm(nchw(ut), None, None, gt, bt, training=True, eps=R.EPS)
    if mode == "identity":
        pre = pre + nchw(rt)
    elif mode == "bn2":
        pre = pre + F.batch_norm(nchw(rt), None, None, gr, br, training=True, eps=R.EPS)
    y = torch.relu(pre)
    y.backward(nchw(dy))
    mean, var, rstd = R.bn_moments(u)
    # statistics through partials of uneven sizes, one of them empty
    cuts = [0, 1, 1, 70, 299, 300]
    parts = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        blk = u[a:e]
        mu = blk.mean(0) if e > a else torch.zeros(C, dtype=torch.float64)
        parts.append(torch.stack([torch.full((C,), float(e - a), dtype=torch.float64), mu,
                                  ((blk - mu) ** 2).sum(0), torch.zeros(C, dtype=torch.float64)], 1))
    fm, fr, sc, sh = R.bn_finalize(torch.stack(parts), g, b)
    R.compare(fm, mean, 1e-12, "merged mean")
    R.compare(fr, rstd, 1e-12, "merged rstd")
    mg = R.bn_merge(torch.stack(parts))
    R.compare(mg[:, 2] / mg[:, 0], var, 1e-12, "bn_merge var")
    rm, _, rr = R.bn_moments(r)
    kw = {"none": {}, "identity": dict(res_mode=1, r=r),
          "bn2": dict(res_mode=2, r=r, rsc=gr * rr, rsh=br - rm * gr * rr)}[mode]
    yr, _ = R.bn_apply(u, sc, sh, relu=1, **kw)
    R.compare(yr, y.detach().reshape(C, M).t(), 1e-12, "bn_apply")
    bw = R.bn_bwd(dy, 1, mref=yr, x1=u, mr1=torch.stack([mean, rstd], 1), g1=g,
                  x2=r if mode == "bn2" else None, mr2=torch.stack([rm, rr], 1), g2=gr, identity2=mode == "identity")
    R.compare(bw["out1"], ut.grad, 1e-11, "out1")
    R.compare(bw["S0"], bt.grad, 1e-11, "S0 = dbeta")
    R.compare(bw["S1"], gt.grad, 1e-11, "S1 = dgamma")
    R.compare(bw["osum1"], ut.grad.sum(0), 1e-11, "osum1", ut.grad.abs().sum(0).max().item())
    if mode != "none":
        R.compare(bw["out2"], rt.grad, 1e-11, "out2")
    if mode == "none":  # mask 2 on the pre-activation selects the same elements as mask 1 on y
        assert torch.equal(R.relu_mask(2, u, sc, sh), yr > 0)


def test_bits_layout():
    pos = torch.zeros(2, 16, dtype=torch.bool)
    pos[0, 0] = pos[0, 9] = pos[1, 15] = True
    bits = R.pack_bits(pos)
    assert bits.tolist() == [[1, 2], [0, 128]]
    assert torch.equal(R.unpack_bits(bits, 16), pos)
    y = torch.tensor([[1e-45, -0.0, 0.0, 3.0, -2.0, 1e-3, 0.0, 5.0]], dtype=torch.float64)
    assert R.bn_bits(y, R.BF16).tolist() == [[0b10101000]]  # 1e-45 stores as 0 in bf16


def _ln_case(F_=5, V=25, C=8, seed=3):
    x = R.draw((F_, V, C), seed, R.F32, 2.0, -1.0)
    g = torch.rand(C, V, generator=R.gen(seed + 1), dtype=torch.float64) + 0.5
    b = torch.randn(C, V, generator=R.gen(seed + 2), dtype=torch.float64) * 0.1
    return x, g, b


@pytest.mark.parametrize("res_mode", [0, 1, 2])
def test_ln_refs_against_oracle(res_mode):
    F_, V, C = 5, 25, 8
    x, g, b = _ln_case(F_, V, C)
    r, rg, rb = _ln_case(F_, V, C, 11)
    dy = R.draw((F_, V, C), 21, R.F32)
    n4 = lambda t: t.permute(0, 2, 1).unsqueeze(2)  # [F][V][C] -> (F, C, 1, V)
    xt, gt, bt = (t.clone().requires_grad_(True) for t in (x, g, b))
    pre = O.layernorm_cv(n4(xt), gt.view(C, 1, V), bt.view(C, 1, V))
    if res_mode == 1:
        pre = pre + n4(r)
    elif res_mode == 2:
        pre = pre + O.layernorm_cv(n4(r), rg.view(C, 1, V), rb.view(C, 1, V))
    y = torch.relu(pre)
    y.backward(n4(dy))
    st = torch.stack(R.ln_stats(x), 1)
    rst = torch.stack(R.ln_stats(r), 1)
    yr = R.ln_apply(x, st, g, b, res_mode, r, rst, rg, rb, relu=1)
    R.compare(n4(yr), y.detach(), 1e-12, "ln_apply")
    mask = dict(mask=2) if res_mode == 0 else dict(mask=1, mref=yr)
    dx, dg, db = R.ln_bwd(dy, x, st, g, b, **mask)
    R.compare(dx, xt.grad, 1e-11, "ln dx")
    R.compare(dg, gt.grad, 1e-11, "ln dgamma")
    R.compare(db, bt.grad, 1e-11, "ln dbeta")
    dx2, _, _ = R.ln_bwd(dy, x, st, g, b, old=r, **mask)
    R.compare(dx2, dx + r, 1e-12, "ln accumulate")


def test_refs_against_norms_golden():
    d = load_golden("norms")
    x4 = d["ln_x"].double()
    N, C, T, V = x4.shape
    ln = sub(d, "ln_sd/")
    g, b = ln["weight"].double().view(C, V), ln["bias"].double().view(C, V)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(N * T, V, C)
    x = rows(x4)
    st = torch.stack(R.ln_stats(x), 1)
    R.compare(R.ln_apply(x, st, g, b, relu=0), rows(d["ln_y"]), 1e-5, "golden ln y")
    dx, dg, _ = R.ln_bwd(rows(d["ln_dy"].double()), x, st, g, b)
    R.compare(dx, rows(d["ln_dx"]), 1e-5, "golden ln dx")
    R.compare(dg, d["ln_grad/weight"].view(C, V), 1e-5, "golden ln dw")
    # BatchNorm1d(V*C) input norm: rows (n, t), channels v*C + c
    x4 = d["bn_x"].double()
    N, C, T, V = x4.shape
    bn = sub(d, "bn_sd/")
    mat = lambda t: t.permute(0, 2, 3, 1).reshape(N * T, V * C)
    xm = mat(x4)
    mean, _, rstd = R.bn_moments(xm)
    gam, bet = bn["norm.weight"].double(), bn["norm.bias"].double()
    y, _ = R.bn_apply(xm, gam * rstd, bet - mean * gam * rstd, relu=0)
    R.compare(y, mat(d["bn_y"]), 1e-5, "golden bn y")
    bw = R.bn_bwd(mat(d["bn_dy"].double()), 0, x1=xm, mr1=torch.stack([mean, rstd], 1), g1=gam)
    R.compare(bw["out1"], mat(d["bn_dx"]), 1e-5, "golden bn dx")
    R.compare(bw["S0"], d["bn_grad/norm.bias"], 1e-5, "golden bn db")


# ------------------------------------------------------------------------------------------ input makers
@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["fp32", "bf16"])
def test_push_out_clears_the_band(dtype):
    C = 16
    t = R.draw((4000, C), 2, dtype, 2.0, 0.3)
    sc = torch.rand(C, generator=R.gen(3), dtype=torch.float64) + 0.5
    sh = torch.randn(C, generator=R.gen(4), dtype=torch.float64)
    out = R.push_out(t, sc, sh, dtype)
    pre = out * sc + sh
    assert pre.abs().min().item() >= R.MARGIN * pre.abs().max().item()
    assert torch.equal(out, R.rnd(out, dtype))
    assert 0 < (out != t).double().mean().item() <= 0.01
    with pytest.raises(AssertionError):  # a band that would move more than 1 % of the elements
        R.push_out(t, sc, sh, dtype, rel=0.05)


def test_hard_stats_ratio():
    x = R.hard_stats((4000, 6), 5, R.F32, 300.0, 1)
    mean, var, _ = R.bn_moments(x)
    ratio = mean.abs() / var.sqrt()
    assert bool(((ratio > 270) & (ratio < 330)).all())
    assert (mean > 0).tolist() == [True, False] * 3


# ------------------------------------------------------------------------------------------ planted slips
def test_slip_ln_biased_variance():
    """At the largest frame of the GPU table (V = 25, C = 512): rstd off by 1/(2E) = 3.9e-5."""
    x = R.draw((3, 25, 512), 31, R.F32, 2.0, 1.0)
    _, rstd = R.ln_stats(x)
    R.compare(rstd, rstd.clone(), R.FP32_FWD, "rstd")
    rejected(R.ln_stats(x, unbiased=False)[1], rstd, R.FP32_FWD, "biased LN variance")


@pytest.mark.parametrize("V,C", [(25, 6), (25, 16)])
def test_slip_ln_bwd_e_for_e_minus_1(V, C):
    x, g, b = _ln_case(7, V, C, 41)
    st = torch.stack(R.ln_stats(x), 1)
    dy = R.ln_dy(x, st, 43, R.F32)
    dx, _, _ = R.ln_bwd(dy, x, st, g, b, mask=2)
    rejected(R.ln_bwd(dy, x, st, g, b, mask=2, e_minus=0)[0], dx, R.FP32_BWD, "E for E - 1")


def _bwd_case(M=5000, C=8, seed=51):
    u, g, b = _bn_case(M, C, seed)
    r = R.draw((M, C), seed + 3, R.F32)
    mean, _, rstd = R.bn_moments(u)
    mr = torch.stack([mean, rstd], 1).float().double()
    dy = R.rnd(torch.randn(M, C, generator=R.gen(seed + 4), dtype=torch.float64) + 0.5 * (u - mean) * rstd, R.F32)
    return u, g, b, r, mr, dy


def test_slip_mask_before_residual():
    u, g, b, r, mr, dy = _bwd_case()
    sc, sh = g * mr[:, 1], b - mr[:, 0] * g * mr[:, 1]
    y, _ = R.bn_apply(u, sc, sh, 1, r)
    good = R.bn_bwd(dy, 1, mref=y, x1=u, mr1=mr, g1=g)
    bad = R.bn_bwd(dy, 2, mref=u, msc=sc, msh=sh, x1=u, mr1=mr, g1=g)  # the sign of the branch without r
    rejected(bad["out1"], good["out1"], R.FP32_BWD, "mask before residual: out1")
    rejected(bad["S0"], good["S0"], R.FP32_BWD, "mask before residual: S0")
    assert not torch.equal(R.pack_bits(u * sc + sh > 0), R.bn_bits(y, R.F32))


def test_slip_block_missing_from_sum():
    u, g, b, r, mr, dy = _bwd_case()
    good = R.bn_bwd(dy, 0, x1=u, mr1=mr, g1=g)
    keep = torch.ones(dy.shape[0], dtype=torch.bool)
    keep[64:128] = False
    xh = (u - mr[:, 0]) * mr[:, 1]
    rejected(dy[keep].sum(0), good["S0"], R.FP32_BWD, "S0 less one block")
    rejected((dy * xh)[keep].sum(0), good["S1"], R.FP32_BWD, "S1 less one block")
    rejected(good["out1"][keep].sum(0), good["osum1"], R.FP32_BWD, "osum less one block",
             good["out1"].abs().sum(0).max().item())
    mean, _, rstd = R.bn_moments(u)
    rejected(R.bn_moments(u[keep])[2], rstd, R.FP32_FWD, "rstd less one block")


def test_slip_row_group_0_only():
    """Channel c merging only the first row slot's partial: every RPI-th row (C = 64 fp32: RPI = 16)."""
    u = R.draw((5000, 64), 61, R.F32, 3.0, 2.0)
    mean, _, rstd = R.bn_moments(u)
    sel = torch.cat([torch.arange(mb, min(5000, mb + 64))[::16] for mb in range(0, 5000, 64)])
    m0, _, r0 = R.bn_moments(u[sel])
    rejected(m0, mean, R.FP32_FWD, "mean of row group 0")
    rejected(r0, rstd, R.FP32_FWD, "rstd of row group 0")
    dy = R.draw((5000, 64), 62, R.F32)
    rejected(dy[sel].sum(0), dy.sum(0), R.FP32_BWD, "S0 of row group 0")


def test_slip_k3_without_k2_mean():
    u, g, b, r, mr, dy = _bwd_case()
    good = R.bn_bwd(dy, 0, x1=u, mr1=mr, g1=g)
    M = dy.shape[0]
    k1 = g * mr[:, 1]
    k2 = -g * mr[:, 1] ** 2 * good["S1"] / M
    k3 = -g * mr[:, 1] * good["S0"] / M - k2 * mr[:, 0]
    R.compare(k1 * dy + k2 * u + k3, good["out1"], 1e-12, "k1/k2/k3 form")
    rejected(k1 * dy + k2 * u + (k3 + k2 * mr[:, 0]), good["out1"], R.FP32_BWD, "k3 without -k2*mean")


def test_slip_dgamma_dbeta_swapped():
    x, g, b = _ln_case(7, 25, 16, 71)
    st = torch.stack(R.ln_stats(x), 1)
    dy = R.ln_dy(x, st, 73, R.F32)
    _, dg, db = R.ln_bwd(dy, x, st, g, b, mask=2)
    rejected(db, dg, R.FP32_BWD, "dgamma <- dbeta")
    rejected(dg, db, R.FP32_BWD, "dbeta <- dgamma")


def test_slip_bits_zero_as_positive():
    u, g, b, r, mr, dy = _bwd_case(M=300)
    y, _ = R.bn_apply(R.rnd(u, R.BF16), g, b, relu=1)
    assert not torch.equal(R.pack_bits(R.rnd(y, R.BF16) >= 0), R.bn_bits(y))


# ------------------------------------------------------------------------------------------ fp32 emulation
@pytest.mark.parametrize("dtype,vec", [(R.F32, 4), (R.BF16, 8)], ids=["fp32", "bf16"])
def test_emulated_bn_stats_meet_the_bar_with_margin(dtype, vec):
    x = R.hard_stats((5000, 64), 3, dtype, BN_HARD_RATIO[dtype], 1)
    mean, _, rstd = R.bn_moments(x)
    em, er = R.emulate_bn_stats_fp32(x.float().numpy(), vec, 64)
    R.compare(em, mean, R.FP32_FWD / 10, "emulated BN mean")
    assert (er - rstd).abs().max().item() <= R.FP32_FWD / 10 * rstd.abs().max().item()


def test_emulated_ln_stats_meet_the_bar_with_margin():
    x = R.hard_stats((12, 25, 64), 4, R.F32, LN_HARD_RATIO, 0)
    mean, rstd = R.ln_stats(x)
    em, er = R.emulate_ln_stats_fp32(x.reshape(12, -1).float().numpy())
    R.compare(em, mean, R.FP32_FWD / 10, "emulated LN mean")
    assert (er - rstd).abs().max().item() <= R.FP32_FWD / 10 * rstd.abs().max().item()


def test_emulation_is_the_plain_statistics_on_easy_data():
    x = R.draw((700, 24), 81, R.F32, 2.0, 1.0)
    mean, _, rstd = R.bn_moments(x)
    em, er = R.emulate_bn_stats_fp32(x.float().numpy(), 4, 64)
    R.compare(em, mean, 1e-6, "emulated mean, easy")
    R.compare(er, rstd, 1e-6, "emulated rstd, easy")
    assert np.isfinite(er.numpy()).all()
