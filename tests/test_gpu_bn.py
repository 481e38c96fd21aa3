"""The BatchNorm kernels of norm.hip and bn_fused.hip alone on the MI355X, every route, through the C-ABI wrappers of
native.py, against the float64 references of norm_ref.py on inputs already rounded to the storage dtype.

Routes are named in the test ids: v = channels per load (8 bf16 / 4 fp32 = one 16-B unit, 1 = element-wise), CU =
units per row, RPI = rows per block iteration (256 / CU).  Row blocks: 64 rows for the statistics and the unfused
reduce (M <= 65536), 32 rows for the element-wise kernels, 8*RPI rows for the fused backward at these sizes.

Bars (norm_ref.py), relative to max|ref|: fp32 forward results and every statistic 1e-5; fp32 backward results and
all fp32-accumulated sums (in the bf16 instantiations too) 1e-4; tensors stored as bf16 2^-8.  Column sums of a
BN-branch gradient are 0 in exact arithmetic and take scale_floor = max_c sum_m |out| as test_bn_bwd_fused does.

Masks come from pre-activations kept 1e-3 * max|pre| away from zero (norm_ref.push_out), so a mask can only differ
through a kernel defect.  A view whose stride or base pointer rules out the 16-B units takes the element-wise route
(unfused kernels) or is refused with STGCN_EBADSHAPE (bits output, fused backward); only that guarded behaviour is
exercised.

Largest measured errors (STGCN_TEST_REPORT=1, MI355X), relative to max|ref|, next to the bar:
    statistics      mean 5.9e-7, rstd 1.8e-6 (C = 1024, M = 70), hard data rstd 1.8e-7 bf16, shift 7.4e-7    (1e-5)
    finalize/merge  mean 3.6e-8, rstd 3.9e-8, shift 9.3e-8, merge -> finalize vs direct 7.3e-8                (1e-5)
    bn_apply        fp32 8.7e-8 (1e-5)    bf16 3.0e-3 (2^-8 = 3.9e-3)    bits exact
    unfused bwd     sums 1.8e-7, dx fp32 1.4e-7 (1e-4)    dx bf16 3.7e-3 (2^-8)
    fused bwd       sums 7.2e-7, column sums 5.3e-6, out fp32 1.9e-7 (1e-4)    out bf16 3.4e-3 (2^-8)
The bf16 figures are the storage rounding (half an ulp is up to 2^-8 of the value).
"""
import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1e30      # padding of inputs: finite, fatal to any sum it reaches
CANARY = -7.0   # padding of outputs: must stay
EBADSHAPE = 1
DT = {"fp32": R.F32, "bf16": R.BF16}


@pytest.fixture(scope="module")
def K(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return pkg.native


def unit(dtype):
    return 8 if dtype == R.BF16 else 4


def vec_of(C, dtype, aligned=True):
    return unit(dtype) if aligned and C % unit(dtype) == 0 else 1


def route(C, dtype, aligned=True):
    v = vec_of(C, dtype, aligned)
    return "v%d-CU%d-RPI%d" % (v, C // v, max(256 // (C // v), 1))


def dev_rows(x, dtype, ld=None, off=0, fill=BIG):
    """[M][C] float64 (values of dtype) -> logical (1, C, M, 1) device view, row stride ld, starting ``off`` elements
    into its buffer; the rest of the buffer holds ``fill``."""
    M, C = x.shape
    ld = ld or C
    assert off + C <= ld
    buf = torch.full((M, ld), fill, dtype=dtype, device=DEV)
    buf[:, off:off + C] = x.to(DEV, dtype)
    return buf[:, off:off + C].unflatten(0, (1, M, 1)).permute(0, 3, 1, 2), buf


def host(view):
    """(1, C, M, 1) device view -> [M][C] float64 on the CPU."""
    return view.permute(0, 2, 3, 1).reshape(view.shape[2], view.shape[1]).double().cpu()


def f32(t):
    return t.float().to(DEV).contiguous()


def affine(C, seed):
    g = torch.rand(C, generator=R.gen(seed), dtype=torch.float64) + 0.5
    b = torch.randn(C, generator=R.gen(seed + 1), dtype=torch.float64)
    return g.float().double(), b.float().double()


def moments32(x):
    """[C][2] (mean, rstd) of x as the kernels receive them: float32 values, in float64."""
    mean, _, rstd = R.bn_moments(x)
    return torch.stack([mean, rstd], 1).float().double()


# ------------------------------------------------------------------------------------------ statistics
MS = [1, 63, 64, 65, 5000]
STAT_CASES = [(C, dt, M, 0, False) for C, dts in ((64, ("fp32", "bf16")), (24, ("fp32",)), (48, ("bf16",)),
                                                   (75, ("fp32", "bf16")), (256, ("fp32", "bf16")))
              for dt in dts for M in MS]
STAT_CASES += [(8, "fp32", 129, 0, False), (8, "bf16", 129, 0, False), (1024, "fp32", 70, 0, False)]
STAT_CASES += [(64, "fp32", 5000, 4, False), (64, "bf16", 5000, 8, False), (75, "fp32", 65, 1, False),
               (48, "bf16", 65, 8, False)]                                   # ld = C + vec views
STAT_CASES += [(64, "fp32", 5000, 0, True), (64, "bf16", 5000, 0, True)]   # hard statistics


def _stat_id(c):
    C, dt, M, pad, hard = c
    return "%s-C%d-%s-M%d%s%s" % (dt, C, route(C, DT[dt]), M, "-ld+%d" % pad if pad else "", "-hard" if hard else "")


@pytest.mark.parametrize("case", STAT_CASES, ids=_stat_id)
def test_bn_stats(K, case):
    """bn_stats_partial then bn_finalize: mean, rstd and the folded affine.  M = 1, 63 leave most row slots empty
    (n = 0 into the merge), M = 65 and 5000 end in a one-row / 8-row block."""
    C, dt, M, pad, hard = case
    dtype = DT[dt]
    x = R.hard_stats((M, C), 3, dtype, R.BN_HARD_RATIO[dtype], 1) if hard else R.draw((M, C), 3, dtype, 3.0, 2.0)
    xd, _ = dev_rows(x, dtype, C + pad)
    g, b = affine(C, 5)
    part, nb, _ = K.bn_stats_partial(xd, M, C, ld=C + pad)
    assert nb == (M + 63) // 64
    mr, sc, sh = K.bn_finalize(part, nb, C, C, f32(g), f32(b))
    mean, _, rstd = R.bn_moments(x)
    name = "bn stats " + _stat_id(case)
    R.compare(part[:, :, 0].sum(0), torch.full((C,), float(M)), 0.0, name + " count")
    R.compare(mr[:, 0], mean, R.FP32_FWD, name + " mean")
    R.compare(mr[:, 1], rstd, R.FP32_FWD, name + " rstd")
    R.compare(sc, g * rstd, R.FP32_FWD, name + " scale")
    R.compare(sh, b - mean * g * rstd, R.FP32_FWD, name + " shift")


def test_bn_stats_unaligned_views_take_the_scalar_route(K):
    """A row stride or a base pointer that rules out 16-B loads: element-wise loads, same result."""
    M, C = 130, 64
    for dt, (ld, off) in [(d, v) for d in ("fp32", "bf16") for v in ((C + 1, 0), (C + 8, 1))]:
        dtype = DT[dt]
        x = R.draw((M, C), 7, dtype, 3.0, 2.0)
        xd, _ = dev_rows(x, dtype, ld, off)
        part, nb, _ = K.bn_stats_partial(xd, M, C, ld=ld)
        mr, _, _ = K.bn_finalize(part, nb, C, C, None, None)
        mean, _, rstd = R.bn_moments(x)
        R.compare(mr[:, 0], mean, R.FP32_FWD, f"bn stats {dt} ld {ld} off {off} mean")
        R.compare(mr[:, 1], rstd, R.FP32_FWD, f"bn stats {dt} ld {ld} off {off} rstd")


def test_bn_stats_bad_shape(K, pkg):
    """A row that does not fit the block's 256 threads: C = 257 fp32 (element-wise), and C = 1024 fp32 once its
    stride rules out the 16-B units."""
    L = pkg._lib
    part = torch.full((4, 1025, 4), 3.0, device=DEV)
    x = torch.zeros(70, 1025, device=DEV)
    for C, ld in ((257, 257), (1024, 1025)):
        rc = L.lib().stgcn_bn_stats_partial(x.data_ptr(), ld, 70, C, part.data_ptr(), 0, L.stream())
        assert rc == EBADSHAPE, f"C {C} ld {ld}: returned {rc}"
    torch.cuda.synchronize()
    assert bool((part == 3.0).all())
    with pytest.raises(RuntimeError, match="bn_stats_partial"):
        K.bn_stats_partial(x, 70, 257, ld=257)


# ------------------------------------------------------------------------------------------ finalize / merge
@pytest.mark.parametrize("affine_on", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("nb", [1, 255, 2048, 2049, 8193],
                         ids=["nb1-256t", "nb255-256t", "nb2048-256t", "nb2049-1024t", "nb8193-1024t-2trips"])
def test_bn_finalize_and_merge_synthetic(K, pkg, nb, affine_on):
    """Synthetic (count, mean, M2) lists, no row kernel: zero counts, means 100 +- 0.1 against M2 ~ 1, ld_part > C."""
    C, ldp = 5, 8
    parts = R.synth_partials(nb, C, 100 + nb)
    buf = torch.full((nb, ldp, 4), BIG, device=DEV)
    buf[:, :C] = parts.to(DEV)
    g, b = affine(C, 9) if affine_on else (None, None)
    mr, sc, sh = K.bn_finalize(buf, nb, ldp, C, f32(g) if affine_on else None, f32(b) if affine_on else None)
    mean, rstd, rsc, rsh = R.bn_finalize(parts, g, b)
    name = "bn finalize nb%d" % nb
    R.compare(mr[:, 0], mean, R.FP32_FWD, name + " mean")
    R.compare(mr[:, 1], rstd, R.FP32_FWD, name + " rstd")
    R.compare(sc, rsc, R.FP32_FWD, name + " scale")
    R.compare(sh, rsh, R.FP32_FWD, name + " shift")
    merged = K.bn_merge(buf, nb, ldp, C)
    mref = R.bn_merge(parts)
    for col, what in enumerate(("count", "mean", "M2", "pad")):
        R.compare(merged[:, col], mref[:, col], R.FP32_FWD, name + " merge " + what)
    mr1, sc1, sh1 = K.bn_finalize(merged, 1, C, C, f32(g) if affine_on else None, f32(b) if affine_on else None)
    for got, direct, ref, what in ((mr1[:, 0], mr[:, 0], mean, "mean"), (mr1[:, 1], mr[:, 1], rstd, "rstd"),
                                   (sc1, sc, rsc, "scale")):
        R.compare(got, ref, R.FP32_FWD, name + " merge->finalize " + what)
        R.compare(got, direct.double().cpu(), R.FP32_FWD, name + " merge->finalize vs direct " + what)


def test_bn_merge_bad_shape(K, pkg):
    L = pkg._lib
    buf = torch.zeros(4, 8, 4, device=DEV)
    out = torch.full((8, 4), 3.0, device=DEV)
    assert L.lib().stgcn_bn_merge(buf.data_ptr(), 4, 4, 5, out.data_ptr(), L.stream()) == EBADSHAPE  # ldp < C
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ------------------------------------------------------------------------------------------ bn_apply
APPLY_SHAPES = [(64, dt, M) for dt in ("fp32", "bf16") for M in (33, 129, 4100)] + [(75, "fp32", 129), (48, "bf16", 129)]


def _apply_inputs(M, C, dtype, seed=11):
    u = R.draw((M, C), seed, dtype, 2.0, 0.3)
    r = R.draw((M, C), seed + 1, dtype, 1.0, -0.2)
    sc, sh = affine(C, seed + 2)
    rsc, rsh = affine(C, seed + 4)
    return u, r, sc, sh, rsc, rsh


@pytest.mark.parametrize("relu", [0, 1, 2, 3], ids=["relu0", "relu1", "relu2", "relu3"])
@pytest.mark.parametrize("res_mode", [0, 1, 2], ids=["res0", "res1", "res2"])
@pytest.mark.parametrize("C,dt,M", APPLY_SHAPES, ids=["%s-C%d-%s-M%d" % (dt, C, route(C, DT[dt]), M)
                                                     for C, dt, M in APPLY_SHAPES])
def test_bn_apply(K, C, dt, M, res_mode, relu):
    """Distinct ldu, ldr, ldy (all keeping the route); the output's padding columns stay untouched.  M = 33, 129: a
    one-row last block of 32; M = 4100: three-row blocks (rpb = 32 up to 65536 rows), 129 blocks."""
    dtype = DT[dt]
    v = vec_of(C, dtype)
    u, r, sc, sh, rsc, rsh = _apply_inputs(M, C, dtype)
    ud, _ = dev_rows(u, dtype, C + v)
    rd, _ = dev_rows(r, dtype, C + 2 * v)
    yd, ybuf = dev_rows(torch.zeros(M, C, dtype=torch.float64), dtype, C + 3 * v, fill=CANARY)
    kw = {0: {}, 1: dict(r=rd), 2: dict(r=rd, rsc=f32(rsc), rsh=f32(rsh))}[res_mode]
    K.bn_apply(ud, f32(sc), f32(sh), M, C, res_mode=res_mode, relu=relu, out=yd, ldu=C + v, ldy=C + 3 * v, **kw)
    ref, _ = R.bn_apply(u, sc, sh, res_mode, r, rsc, rsh, relu)
    R.compare(host(yd), ref, R.store_bar(dtype), "bn apply %s C%d M%d res%d relu%d" % (dt, C, M, res_mode, relu))
    assert bool((ybuf[:, C:] == CANARY).all())


def _bits_inputs(M, C, res_mode, relu, dtype=R.BF16):
    """Inputs whose final pre-activation (the value the sign bit is taken from) is out of the margin band: the last
    term added is the one that is moved (r with a residual, else u)."""
    u, r, sc, sh, rsc, rsh = _apply_inputs(M, C, dtype, 21)
    t = u * sc + sh
    if res_mode == 0:
        u = R.push_out(u, sc, sh, dtype)
    else:
        base = t.clamp(min=0) if relu & 2 else t
        one = torch.ones(C, dtype=torch.float64)
        r = R.push_out(r, rsc if res_mode == 2 else one, base + (rsh if res_mode == 2 else 0.0), dtype)
    return u, r, sc, sh, rsc, rsh


@pytest.mark.parametrize("res_mode,relu", [(0, 1), (1, 1), (2, 3), (1, 0), (2, 1)])
@pytest.mark.parametrize("C", [8, 256], ids=["C8-v8-CU1-RPI256", "C256-v8-CU32-RPI8"])
def test_bn_apply_bits(K, C, res_mode, relu):
    """The sign-bit output: byte [m][c / 8], bit c % 8 = stored y > 0 (zero is not positive)."""
    M = 129
    u, r, sc, sh, rsc, rsh = _bits_inputs(M, C, res_mode, relu)
    ud, _ = dev_rows(u, R.BF16)
    rd, _ = dev_rows(r, R.BF16)
    kw = {0: {}, 1: dict(r=rd), 2: dict(r=rd, rsc=f32(rsc), rsh=f32(rsh))}[res_mode]
    bits = torch.full((M + 1, C // 8), 0xA5, dtype=torch.uint8, device=DEV)
    y = K.bn_apply(ud, f32(sc), f32(sh), M, C, res_mode=res_mode, relu=relu, bits=bits, **kw)
    ref, _ = R.bn_apply(u, sc, sh, res_mode, r, rsc, rsh, relu)
    R.compare(host(y), ref, R.BF16_STORE, "bn apply bits C%d res%d relu%d" % (C, res_mode, relu))
    assert torch.equal(bits[:M].cpu(), R.bn_bits(ref))
    assert torch.equal(bits[:M].cpu(), R.pack_bits(host(y) > 0))
    assert bool((bits[M] == 0xA5).all())


@pytest.mark.parametrize("how", ["stride", "pointer"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_bn_apply_unaligned_view(K, dt, how):
    """An input view that rules out the 16-B units (odd row stride / base pointer one element in): the element-wise
    route, same values; with the bits output requested it is refused."""
    dtype, M, C = DT[dt], 70, 64
    u, r, sc, sh, rsc, rsh = _apply_inputs(M, C, dtype, 31)
    ld, off = (C + 1, 0) if how == "stride" else (C + 8, 1)
    ud, _ = dev_rows(u, dtype, ld, off)
    rd, _ = dev_rows(r, dtype)
    yd, ybuf = dev_rows(torch.zeros(M, C, dtype=torch.float64), dtype, C + 8, fill=CANARY)
    K.bn_apply(ud, f32(sc), f32(sh), M, C, res_mode=2, r=rd, rsc=f32(rsc), rsh=f32(rsh), relu=1, out=yd, ldu=ld,
               ldy=C + 8)
    ref, _ = R.bn_apply(u, sc, sh, 2, r, rsc, rsh, 1)
    R.compare(host(yd), ref, R.store_bar(dtype), f"bn apply unaligned {how} {dt}")
    assert bool((ybuf[:, C:] == CANARY).all())
    if dtype == R.BF16:
        bits = torch.full((M, C // 8), 0xA5, dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError, match="bn_apply_bits"):
            K.bn_apply(ud, f32(sc), f32(sh), M, C, relu=1, out=yd, ldu=ld, ldy=C + 8, bits=bits)
        torch.cuda.synchronize()
        assert bool((bits == 0xA5).all())


# ------------------------------------------------------------------------------------------ unfused backward
BWD_SHAPES = [(C, dt, M) for C in (64, 75, 24) for dt in ("fp32", "bf16") for M in (65, 5000)]


def _bwd_inputs(M, C, dtype, mask, seed=41):
    """x (the BN input), its statistics, gamma, the mask reference with its margin, dy with a component along xhat."""
    x = R.draw((M, C), seed, dtype, 2.0, 0.5)
    g, b = affine(C, seed + 1)
    mr = moments32(x)
    sc, sh = (g * mr[:, 1]).float().double(), (b - mr[:, 0] * g * mr[:, 1]).float().double()
    mref = None
    if mask == 2:       # the mask reference is the BN input itself: pre = x*sc + sh
        x = R.push_out(x, sc, sh, dtype)
        mref = x
    elif mask == 1:     # the stored forward output relu(pre + r)
        r = R.draw((M, C), seed + 3, dtype)
        r = R.push_out(r, torch.ones(C, dtype=torch.float64), x * sc + sh, dtype)
        mref = R.rnd((x * sc + sh + r).clamp(min=0), dtype)
        assert bool(((mref > 0) == (x * sc + sh + r > 0)).all())
    dy = R.bn_dy(x, mr, seed + 5, dtype)
    return x, g, mr, sc, sh, mref, dy


@pytest.mark.parametrize("variant", ["bn", "bn-acc-nogamma", "identity", "identity-acc"])
@pytest.mark.parametrize("mask", [0, 1, 2], ids=["mask0", "mask1", "mask2"])
@pytest.mark.parametrize("C,dt,M", BWD_SHAPES, ids=["%s-C%d-%s-M%d" % (dt, C, route(C, DT[dt]), M)
                                                   for C, dt, M in BWD_SHAPES])
def test_bn_bwd_unfused(K, C, dt, M, mask, variant):
    """bn_bwd_reduce (S0 = sum dz, S1 = sum dz*xhat; S1 = 0 without x) and bn_bwd_apply (dx (+)= ...; identity:
    dx (+)= dz)."""
    dtype = DT[dt]
    x, g, mr, sc, sh, mref, dy = _bwd_inputs(M, C, dtype, mask)
    identity, acc = variant.startswith("identity"), "acc" in variant
    gam = None if (identity or "nogamma" in variant) else g
    dyd, _ = dev_rows(dy, dtype)
    xd = None if identity else dev_rows(x, dtype)[0]
    mk = {}
    if mask:
        mk = dict(mask=mask, mref=xd if (mask == 2 and xd is not None) else dev_rows(mref, dtype)[0])
        if mask == 2:
            mk.update(msc=f32(sc), msh=f32(sh))
    mrd = None if identity else f32(mr)
    ref = R.bn_bwd(dy, mask, mref, sc, sh, x1=None if identity else x, mr1=mr, g1=gam)
    name = "bn bwd %s C%d M%d mask%d %s" % (dt, C, M, mask, variant)
    sums = K.bn_bwd_reduce(dyd, M, C, x=xd, mean_rstd=mrd, **mk)
    R.compare(sums[:, 0], ref["S0"], R.FP32_BWD, name + " S0")
    R.compare(sums[:, 1], ref["S1"], R.FP32_BWD, name + " S1", 1.0)
    old = R.draw((M, C), 47, dtype)
    dxd, _ = dev_rows(old, dtype)
    sums_ref = f32(torch.stack([ref["S0"], ref["S1"]], 1))
    K.bn_bwd_apply(dyd, M, C, dxd, x=xd, mean_rstd=mrd, gamma=None if gam is None else f32(gam), sums=sums_ref,
                   accumulate=acc, **mk)
    R.compare(host(dxd), ref["out1"] + (old if acc else 0.0), R.store_bar(dtype, True), name + " dx")


# ------------------------------------------------------------------------------------------ fused backward
FUSED_SHAPES = [(8, "bf16"), (4, "fp32"), (48, "bf16"), (128, "bf16"), (256, "fp32")]


def fused_rpb(C, dtype):
    """Rows per block of the fused passes at M <= 8 * RPI * (block target): two iterations of four rows per thread."""
    return 2 * 4 * (256 // (C // unit(dtype)))


FUSED_CASES = [(C, dt, mk) for C, dt in FUSED_SHAPES for mk in ("7", "rpb", "rpb+1", "3rpb-5")]


def _fused_m(C, dtype, mk):
    rpb = fused_rpb(C, dtype)
    return {"7": 7, "rpb": rpb, "rpb+1": rpb + 1, "3rpb-5": 3 * rpb - 5}[mk]


@pytest.mark.parametrize("out2", ["none", "identity", "x2"])
@pytest.mark.parametrize("mask", [1, 2, 3], ids=["mask1", "mask2", "mask3"])
@pytest.mark.parametrize("C,dt,mk", FUSED_CASES, ids=["%s-C%d-%s-M%s" % (dt, C, route(C, DT[dt]), mk)
                                                     for C, dt, mk in FUSED_CASES])
def test_bn_bwd_fused_sweep(K, C, dt, mk, mask, out2):
    """acc2 x bias_sums inside; sums, column sums, out1 and out2 against float64.  mask 2 runs with mref the same
    tensor as x1 (one load serves both) and with a separate copy: bit-equal.  mask 3 at fp32 is refused."""
    dtype = DT[dt]
    M = _fused_m(C, dtype, mk)
    real_mask = 1 if mask == 3 else mask
    x1, g1, mr1, sc, sh, mref, dy = _bwd_inputs(M, C, dtype, real_mask, 51)
    x2 = R.draw((M, C), 61, dtype, 1.0, -0.3)
    g2, _ = affine(C, 63)
    mr2 = moments32(x2)
    old2 = R.draw((M, C), 65, dtype)
    dyd, x1d, x2d = (dev_rows(t, dtype)[0] for t in (dy, x1, x2))
    if mask == 3:
        if dtype != R.BF16:
            o1 = torch.empty_like(x1d)
            with pytest.raises(RuntimeError, match="bn_bwd_fused"):
                K.bn_bwd_fused(dyd, M, C, mask=3, mref=torch.zeros(M, max(C // 8, 1), dtype=torch.uint8, device=DEV),
                               x1=x1d, mr1=f32(mr1), g1=f32(g1), out1=o1)
            return
        mrefs = [R.bn_bits(mref).to(DEV)]
    elif mask == 2:
        mrefs = [x1d, x1d.clone()]
    else:
        mrefs = [dev_rows(mref, dtype)[0]]
    mkw = dict(mask=mask, msc=f32(sc), msh=f32(sh)) if mask == 2 else dict(mask=mask)
    name = "bn fused %s C%d M%d mask%d %s" % (dt, C, M, mask, out2)
    for acc2 in ((False, True) if out2 != "none" else (False,)):
        ref = R.bn_bwd(dy, real_mask, mref, sc, sh, x1=x1, mr1=mr1, g1=g1, x2=x2 if out2 == "x2" else None, mr2=mr2,
                       g2=g2, identity2=out2 == "identity", old2=old2 if acc2 else None)
        for bias_sums in (False, True):
            got = []
            for mrefd in mrefs:
                o1 = torch.full_like(x1d, CANARY)
                o2 = dev_rows(old2, dtype)[0] if out2 != "none" else None
                kw = dict(x2=x2d, mr2=f32(mr2), g2=f32(g2)) if out2 == "x2" else {}
                sums, osum = K.bn_bwd_fused(dyd, M, C, mref=mrefd, x1=x1d, mr1=f32(mr1), g1=f32(g1), out1=o1, out2=o2,
                                            acc2=acc2, bias_sums=bias_sums, **kw, **mkw)
                torch.cuda.synchronize()
                got.append((o1, o2, sums.clone(), None if osum is None else osum.clone()))
            o1, o2, sums, osum = got[0]
            tag = "%s acc%d osum%d" % (name, acc2, bias_sums)
            R.compare(sums[0], ref["S0"], R.FP32_BWD, tag + " S0")
            R.compare(sums[1], ref["S1"], R.FP32_BWD, tag + " S1")
            if out2 == "x2":
                R.compare(sums[2], ref["S2"], R.FP32_BWD, tag + " S2")
            R.compare(host(o1), ref["out1"], R.store_bar(dtype, True), tag + " out1")
            if o2 is not None:
                R.compare(host(o2), ref["out2"], R.store_bar(dtype, True), tag + " out2")
            assert (osum is not None) == bias_sums
            if bias_sums:
                R.compare(osum[0], ref["osum1"], R.FP32_BWD, tag + " osum1", ref["out1"].abs().sum(0).max().item())
                if o2 is not None:
                    floor = ref["out2"].abs().sum(0).max().item() if out2 == "x2" and not acc2 else 0.0
                    R.compare(osum[1], ref["osum2"], R.FP32_BWD, tag + " osum2", floor)
            if len(got) == 2:  # mask 2: mref is x1 vs a separate copy
                for a_, b_ in zip(got[0], got[1]):
                    assert (a_ is None and b_ is None) or torch.equal(a_, b_), tag + " same_x"


@pytest.mark.parametrize("which", ["dy", "mref", "x1", "x2", "out1", "out2"])
def test_bn_bwd_fused_refuses_unaligned_pointers(K, which):
    """No element-wise route in the fused backward: a base pointer one element into a 16-B unit is STGCN_EBADSHAPE
    in both passes, as an odd row stride already was; nothing is written."""
    dtype, M, C = R.BF16, 40, 64
    t = {k: dev_rows(R.draw((M, C), 70 + i, dtype), dtype, C + 8, 1 if k == which else 0, fill=CANARY)
         for i, k in enumerate(["dy", "mref", "x1", "x2", "out1", "out2"])}
    mr = f32(moments32(R.draw((M, C), 80, dtype)))
    g = f32(affine(C, 81)[0])
    args = dict(mask=1, mref=t["mref"][0], x1=t["x1"][0], mr1=mr, g1=g, x2=t["x2"][0], mr2=mr, g2=g, out2=t["out2"][0])
    with pytest.raises(RuntimeError, match="bn_bwd_fused_reduce"):
        K.bn_bwd_fused(t["dy"][0], M, C, out1=t["out1"][0], **args)
    torch.cuda.synchronize()
    for k in ("out1", "out2"):   # the buffers still hold what they held
        view, buf = t[k]
        off = 1 if k == which else 0
        assert bool((buf[:, :off] == CANARY).all()) and bool((buf[:, off + C:] == CANARY).all())
        assert torch.equal(host(view), R.draw((M, C), 70 + ["dy", "mref", "x1", "x2", "out1", "out2"].index(k), dtype))
