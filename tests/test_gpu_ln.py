"""The LayerNorm kernels of ln.hip alone on the MI355X (ln_stats, ln_apply, ln_bwd), every route, through the C-ABI
wrappers of native.py, against the float64 references of norm_ref.py on inputs already rounded to the storage dtype.

The route of ln_bwd is worked out by hand from bwd_r / bwd_threads (units per frame U = V * C / vec / R must fit 512
threads, else 1024; R = vectors per unit; prefetch ring PF = 4 at R1, 2 at R2, 1 at R4 / R8, at most 2 at 1024
threads) and stated in the test ids, so a change of route renames a test.  Blocks: min(F, 512 at 256 threads else
256), doubled without dgb; frames per block fpb = ceil(F / blocks).

ln_apply and ln_bwd are fed the reference statistics (rounded to fp32), so each kernel is judged on its own; ln_stats
is compared on the same frames.  Masks come from pre-activations kept 1e-3 * max|pre| away from zero.

Bars (norm_ref.py), relative to max|ref|: statistics and fp32 forward 1e-5; fp32 backward, dgamma / dbeta (fp32 sums
in the bf16 instantiations too) 1e-4; tensors stored as bf16 2^-8.

Largest measured errors (STGCN_TEST_REPORT=1, MI355X), relative to max|ref|, next to the bar:
    ln_stats   fp32 rows mean 3.4e-7, rstd 1.8e-7; bf16 rows (C = 512) mean 2.4e-6, rstd 3.2e-6; hard frames 5.4e-8  (1e-5)
    ln_apply   fp32 1.1e-7 (1e-5)    bf16 3.7e-3 (2^-8 = 3.9e-3)
    ln_bwd     dx fp32 1.3e-7, dgamma 1.4e-7, dbeta 1.2e-7 (1e-4)    dx bf16 3.9e-3 (2^-8)
The bf16 figures are the storage rounding (half an ulp is up to 2^-8 of the value).
"""
import math

import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1e30
CANARY = -7.0
EBADSHAPE = 1
DT = {"fp32": R.F32, "bf16": R.BF16}


@pytest.fixture(scope="module")
def K(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return pkg.native


# name: (dtype, V, C, odd-stride rows, R, threads, PF) -- R / threads / PF by hand, checked against the rule below
ROUTES = {
    "fp32-C16-R1-256t-PF4": ("fp32", 25, 16, False, 1, 256, 4),
    "fp32-C64-R1-512t-PF4": ("fp32", 25, 64, False, 1, 512, 4),
    "fp32-C128-R2-512t-PF2": ("fp32", 25, 128, False, 2, 512, 2),
    "fp32-C256-R2-1024t-PF2": ("fp32", 25, 256, False, 2, 1024, 2),
    "bf16-C64-R1-256t-PF4": ("bf16", 25, 64, False, 1, 256, 4),
    "bf16-C256-R2-512t-PF2": ("bf16", 25, 256, False, 2, 512, 2),
    "bf16-C512-R2-1024t-PF2": ("bf16", 25, 512, False, 2, 1024, 2),
    "fp32-scalar-C6-R1-256t-PF4": ("fp32", 25, 6, False, 1, 256, 4),
    "fp32-scalar-C32-odd-R2-512t-PF2": ("fp32", 25, 32, True, 2, 512, 2),
    "bf16-scalar-C64-odd-R4-512t-PF1": ("bf16", 25, 64, True, 4, 512, 1),
    "fp32-scalar-C256-odd-R8-1024t-PF1": ("fp32", 25, 256, True, 8, 1024, 1),
    "bf16-V18-C64-R1-256t-PF4": ("bf16", 18, 64, False, 1, 256, 4),
}
LONG = [("bf16-C64-R1-256t-PF4", 2601, True), ("bf16-C64-R1-256t-PF4", 1037, False),
        ("bf16-C256-R2-512t-PF2", 1283, True), ("bf16-C512-R2-1024t-PF2", 1283, True)]
CASES = [(n, F, None) for n, r in ROUTES.items() for F in (1, 7, r[6] + 1)] + LONG


def vec_of(dtype, C, odd):
    v = 8 if dtype == R.BF16 else 4
    return 1 if (odd or C % v) else v


def route_rule(V, C, vec):
    """(R, threads, PF) from the documented rule."""
    for lim in (512, 1024):
        for r in ((1, 2) if vec > 1 else (1, 2, 4, 8)):
            if (C // vec) % r == 0 and V * (C // vec // r) <= lim:
                U = V * (C // vec // r)
                nt = 256 if U <= 256 else (512 if U <= 512 else 1024)
                pf = {1: 4, 2: 2, 4: 1, 8: 1}[r]
                return r, nt, min(pf, 2) if nt == 1024 else pf
    return None


def test_route_table_matches_the_rule():
    for name, (dt, V, C, odd, r, nt, pf) in ROUTES.items():
        assert route_rule(V, C, vec_of(DT[dt], C, odd)) == (r, nt, pf), name
        assert ("R%d-%dt-PF%d" % (r, nt, pf)) in name
    assert route_rule(25, 512, 4) is None
    for name, F, dgb in LONG:  # with dgb the run per block exceeds the ring and some block's run is no multiple of it
        nt, pf = ROUTES[name][5], ROUTES[name][6]
        nb = min(F, (512 if nt == 256 else 256) * (1 if dgb else 2))
        fpb = -(-F // nb)
        last = F - (-(-F // fpb) - 1) * fpb
        if dgb:
            assert fpb > pf and (fpb % pf or last % pf), (name, fpb, last)
        else:
            assert -(-F // fpb) > (512 if nt == 256 else 256)


def ln_rows(x, dtype, odd=False, off=0, fill=BIG):
    """[F][V][C] float64 -> logical (F, C, 1, V) device view; odd: row stride C + 1; off: the view starts ``off``
    elements into a buffer of row stride C + 8."""
    F, V, C = x.shape
    ld = C + 1 if odd else (C + 8 if off else C)
    buf = torch.full((F, V, ld), fill, dtype=dtype, device=DEV)
    buf[..., off:off + C] = x.to(DEV, dtype)
    return buf[..., off:off + C].unsqueeze(1).permute(0, 3, 1, 2), buf


def host(view):
    return view.permute(0, 2, 3, 1).squeeze(1).double().cpu()  # (F, C, 1, V) -> [F][V][C]


def f32(t):
    return t.float().to(DEV).contiguous()


def affine(C, V, seed):
    g = torch.rand(C, V, generator=R.gen(seed), dtype=torch.float64) + 0.5
    b = torch.randn(C, V, generator=R.gen(seed + 1), dtype=torch.float64) * 0.3
    return g.float().double(), b.float().double()


def stats32(x):
    return torch.stack(R.ln_stats(x), 1).float().double()


_INPUTS = {}


def inputs(F, V, C, dtype):
    """x with its mask-2 pre-activation out of the margin band under its own fp32 statistics, the affine, a residual
    r whose sum with the pre-activation is out of the band (mask 1's stored y), dy with a component along xhat.
    Computed once per shape and left unchanged."""
    key = (F, V, C, dtype)
    if key not in _INPUTS:
        x = R.draw((F, V, C), 3, dtype, 2.0, -1.0)
        g, b = affine(C, V, 5)
        for _ in range(6):
            st = stats32(x)
            slope = st[:, 1, None, None] * g.t()
            offset = b.t() - st[:, 0, None, None] * slope
            pre = x * slope + offset
            if pre.abs().min().item() >= R.MARGIN * pre.abs().max().item():
                break
            x = R.push_out(x, slope, offset, dtype)
        else:
            raise AssertionError("margin not reached")
        r = R.push_out(R.draw((F, V, C), 7, dtype), torch.ones(1, dtype=torch.float64), pre, dtype)
        y = R.rnd((pre + r).clamp(min=0), dtype)
        dy = R.ln_dy(x, st, 9, dtype)
        if F > 300:  # the long runs are used once
            return x, g, b, st, r, y, dy
        _INPUTS[key] = (x, g, b, st, r, y, dy)
    return _INPUTS[key]


@pytest.mark.parametrize("name,F,dgb_on", CASES, ids=["%s-F%d%s" % (n, F, "" if d is None else ("-dgb" if d else "-nodgb"))
                                                     for n, F, d in CASES])
def test_ln_route(K, name, F, dgb_on):
    """ln_stats, ln_apply (all res_mode x relu at the short F, two at the long) and ln_bwd on one route.  The backward's
    mode rotates with the route and F so that every route sees mask 0 / 1 / 2, accumulate on / off and dgb on / off."""
    dt, V, C, odd, r_, nt, pf = ROUTES[name]
    dtype = DT[dt]
    x, g, b, st, r, y, dy = inputs(F, V, C, dtype)
    gd, bd, std = f32(g.reshape(-1)), f32(b.reshape(-1)), f32(st)
    xd, _ = ln_rows(x, dtype, odd)
    # --- statistics
    got = K.ln_stats(xd, F, V, C)
    mean, rstd = R.ln_stats(x)
    R.compare(got[:, 0], mean, R.FP32_FWD, name + " mean")
    R.compare(got[:, 1], rstd, R.FP32_FWD, name + " rstd")
    # --- apply
    rd, _ = ln_rows(r, dtype, odd)
    rg, rb = affine(C, V, 11)
    rst = stats32(r)
    combos = [(m, a) for m in (0, 1, 2) for a in (0, 1, 2, 3)] if F <= 8 else [(2, 3), (1, 1)]
    for res_mode, relu in combos:
        yd, ybuf = ln_rows(torch.zeros(F, V, C, dtype=torch.float64), dtype, odd, fill=CANARY)
        kw = {0: {}, 1: dict(r=rd), 2: dict(r=rd, rst=f32(rst), rg=f32(rg.reshape(-1)), rb=f32(rb.reshape(-1)))}[res_mode]
        K.ln_apply(xd, std, gd, bd, F * V, V, C, res_mode=res_mode, relu=relu, out=yd, **kw)
        ref = R.ln_apply(x, st, g, b, res_mode, r, rst, rg, rb, relu)
        R.compare(host(yd), ref, R.store_bar(dtype), "%s apply res%d relu%d" % (name, res_mode, relu))
        assert bool((ybuf[..., C:] == CANARY).all())
    # --- backward
    i = list(ROUTES).index(name)
    j = {1: 0, 7: 1}.get(F, 2)
    mask, acc = (i + j) % 3, bool((i + j) % 2) if F <= 8 else True
    dgb_on = (j != 1) if dgb_on is None else dgb_on
    dyd, _ = ln_rows(dy, dtype, odd)
    old = R.draw((F, V, C), 13, dtype)
    dxd, dbuf = ln_rows(old, dtype, odd, fill=CANARY)
    dgb0 = R.draw((2, C * V), 15, R.F32)
    dgb = f32(dgb0) if dgb_on else None
    mk = dict(mask=1, mref=ln_rows(y, dtype, odd)[0]) if mask == 1 else dict(mask=mask)
    K.ln_bwd(dyd, xd, std, gd, bd, F, V, C, dxd, accumulate=acc, dgb=dgb, **mk)
    dx, dgam, dbet = R.ln_bwd(dy, x, st, g, b, mask, y, old if acc else None)
    tag = "%s bwd mask%d acc%d dgb%d" % (name, mask, acc, dgb_on)
    R.compare(host(dxd), dx, R.store_bar(dtype, True), tag + " dx")
    assert bool((dbuf[..., C:] == CANARY).all())
    if dgb_on:  # += into a non-zero buffer
        R.compare(dgb[0], dgb0[0] + dgam.reshape(-1), R.FP32_BWD, tag + " dgamma")
        R.compare(dgb[1], dgb0[1] + dbet.reshape(-1), R.FP32_BWD, tag + " dbeta")


def test_ln_bwd_too_wide_frame(K, pkg):
    """fp32 C = 512 at V = 25: 3200 vectors per frame, no unit width brings it to 1024 threads."""
    L = pkg._lib
    F, V, C = 2, 25, 512
    t = torch.zeros(F, V, C, device=DEV)
    dx = torch.full((F, V, C), CANARY, device=DEV)
    st = torch.ones(F, 2, device=DEV)
    g = torch.ones(C * V, device=DEV)
    rc = L.lib().stgcn_ln_bwd(t.data_ptr(), C, 0, None, 0, t.data_ptr(), C, st.data_ptr(), g.data_ptr(), g.data_ptr(), F,
                              V, C, dx.data_ptr(), C, 0, None, None, 0, 0, L.stream())
    assert rc == EBADSHAPE
    torch.cuda.synchronize()
    assert bool((dx == CANARY).all())


def test_ln_dgb_accumulates_and_is_deterministic(K):
    name = "bf16-C256-R2-512t-PF2"
    dt, V, C, odd, *_ = ROUTES[name]
    F, dtype = 300, DT[dt]
    x, g, b, st, r, y, dy = inputs(F, V, C, dtype)
    xd, dyd = ln_rows(x, dtype)[0], ln_rows(dy, dtype)[0]
    dxd = ln_rows(x, dtype)[0]
    outs = []
    for _ in range(2):
        dgb = torch.zeros(2, C * V, device=DEV)
        K.ln_bwd(dyd, xd, f32(st), f32(g.reshape(-1)), f32(b.reshape(-1)), F, V, C, dxd, mask=2, dgb=dgb)
        outs.append(dgb.clone())
    assert torch.equal(outs[0], outs[1])
    K.ln_bwd(dyd, xd, f32(st), f32(g.reshape(-1)), f32(b.reshape(-1)), F, V, C, dxd, mask=2, dgb=dgb)
    _, dgam, dbet = R.ln_bwd(dy, x, st, g, b, 2)
    R.compare(dgb[0], 2 * dgam.reshape(-1), R.FP32_BWD, "dgamma twice")
    R.compare(dgb[1], 2 * dbet.reshape(-1), R.FP32_BWD, "dbeta twice")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_ln_unaligned_base_pointer_takes_the_scalar_route(K, dt):
    """Views starting one element into 16-B aligned rows: element-wise loads (R4 at C = 64), same values."""
    dtype, F, V, C = DT[dt], 7, 25, 64
    x, g, b, st, r, y, dy = inputs(F, V, C, dtype)
    gd, bd, std = f32(g.reshape(-1)), f32(b.reshape(-1)), f32(st)
    xd, _ = ln_rows(x, dtype, off=1)
    got = K.ln_stats(xd, F, V, C)
    R.compare(got[:, 0], st[:, 0], R.FP32_FWD, "unaligned mean")
    R.compare(got[:, 1], st[:, 1], R.FP32_FWD, "unaligned rstd")
    yd, ybuf = ln_rows(torch.zeros(F, V, C, dtype=torch.float64), dtype, off=1, fill=CANARY)
    K.ln_apply(xd, std, gd, bd, F * V, V, C, res_mode=1, r=ln_rows(r, dtype, off=1)[0], relu=1, out=yd)
    R.compare(host(yd), R.ln_apply(x, st, g, b, 1, r, relu=1), R.store_bar(dtype), "unaligned apply")
    dxd, dbuf = ln_rows(torch.zeros(F, V, C, dtype=torch.float64), dtype, off=1, fill=CANARY)
    dgb = torch.zeros(2, C * V, device=DEV)
    K.ln_bwd(ln_rows(dy, dtype, off=1)[0], xd, std, gd, bd, F, V, C, dxd, mask=1, mref=yd, dgb=dgb)
    dx, dgam, dbet = R.ln_bwd(dy, x, st, g, b, 1, R.rnd((R.ln_apply(x, st, g, b, 1, r, relu=1)), dtype))
    R.compare(host(dxd), dx, R.store_bar(dtype, True), "unaligned dx")
    R.compare(dgb[0], dgam.reshape(-1), R.FP32_BWD, "unaligned dgamma")
    for buf in (ybuf, dbuf):
        assert bool((buf[..., 0] == CANARY).all()) and bool((buf[..., C + 1:] == CANARY).all())


def apply_fstep(U, F):
    """Frames between a thread's visits in ln_apply: the grid is a multiple of U / gcd(U, 256) blocks, about 2048,
    and no more than one sweep of the F frames needs."""
    g0 = U // math.gcd(U, 256)
    k = max(2048 // g0, 1)
    need = (F * U + 255) // 256
    while k > 1 and g0 * (k - 1) >= need:
        k -= 1
    return g0 * k * 256 // U


@pytest.mark.parametrize("dF", [-1, 0, 1], ids=["2fstep-1", "2fstep", "2fstep+1"])
def test_ln_apply_two_frame_loop_and_tail(K, dF):
    """F around 2 * fstep on the scalar C = 6 route (the fewest elements that reach it): threads that run the
    two-frame loop once, once plus the tail, and the tail only."""
    V, C, dtype = 25, 6, R.F32
    fstep = apply_fstep(V * C, 10 ** 6)
    F = 2 * fstep + dF
    assert apply_fstep(V * C, F) == fstep and fstep == 3456
    x = R.draw((F, V, C), 21, dtype, 2.0, -1.0)
    r = R.draw((F, V, C), 22, dtype)
    g, b = affine(C, V, 23)
    st, rst = stats32(x), stats32(r)
    yd, _ = ln_rows(torch.zeros(F, V, C, dtype=torch.float64), dtype)
    K.ln_apply(ln_rows(x, dtype)[0], f32(st), f32(g.reshape(-1)), f32(b.reshape(-1)), F * V, V, C, res_mode=2,
               r=ln_rows(r, dtype)[0], rst=f32(rst), rg=f32(b.reshape(-1)), rb=f32(g.reshape(-1)), relu=3, out=yd)
    R.compare(host(yd), R.ln_apply(x, st, g, b, 2, r, rst, b, g, 3), R.FP32_FWD, "ln apply F %d" % F)


def test_ln_stats_constant_and_hard_frames(K):
    """A constant frame: variance exactly 0, rstd = 1/sqrt(eps) to fp32 rounding.  Frames with |mean| = 1e3 * std
    (alternating sign), the case the shift by the frame's first element exists for; U = 150 (scalar) and 1600."""
    for dt, V, C in (("fp32", 25, 6), ("fp32", 25, 256), ("bf16", 25, 512)):
        dtype = DT[dt]
        x = R.hard_stats((9, V, C), 31, dtype, R.LN_HARD_RATIO, 0)
        x[4] = 3.25
        got = K.ln_stats(ln_rows(x, dtype)[0], 9, V, C)
        mean, rstd = R.ln_stats(x)
        R.compare(got[:, 0], mean, R.FP32_FWD, "ln hard mean %s C%d" % (dt, C))
        R.compare(got[:, 1], rstd, R.FP32_FWD, "ln hard rstd %s C%d" % (dt, C))
        exact = 1.0 / math.sqrt(float(torch.tensor(R.EPS, dtype=torch.float32)))
        assert got[4, 0].item() == 3.25
        assert abs(got[4, 1].item() - exact) <= exact * 2.0 ** -22  # one fp32 ulp: a square root and a division
