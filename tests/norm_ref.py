"""float64 references of the BatchNorm and LayerNorm kernels (norm.hip, bn_fused.hip, ln.hip), the input makers of
their kernel-level tests and the comparison bars.  Plain torch / numpy, importable without a GPU.

Written from the formulas in the header comments of norm.hip and ln.hip, on [rows][channels] matrices (BN) and
[frames][V][C] blocks (LN); nothing here follows the kernels' blocking.

  BN statistics  biased variance, eps 1e-5; (count, mean, M2) partials merged pairwise (Chan et al.)
  bn_apply       y = act(u*sc + sh + res), res: 0 none | 1 r | 2 r*rsc + rsh; relu bit 1 (value 2) on the
                 normalised branch before the add, bit 0 after it; bits: byte [m][c / 8], bit c % 8 = stored y > 0
  BN backward    dz = dy*mask (0 none | 1 mref > 0 | 2 mref*msc + msh > 0 | 3 the bits); S = (sum dz, sum dz*xhat1,
                 sum dz*xhat2); out = g*rstd*(dz - S0/M - xhat*S/M); identity residual out2 (+)= dz
  LN             per frame over its V*C elements, UNBIASED variance; affine element [c][v];
                 dx = rstd*(gz - mean(gz) - xhat*sum(gz*xhat)/(E-1)), gz = dz*gamma; dgamma = sum_f dz*xhat,
                 dbeta = sum_f dz

Inputs are rounded to the storage dtype first, so a reference sees the values a kernel loads.  Wherever a mask is
taken from a pre-activation, push_out() moves the few elements that lie within 1e-3 * max|pre| of zero out of
that band (and asserts it moved at most 1 % of them): a mask disagreement in a test is then a kernel defect, never
the last bit of an FMA.
"""
import numpy as np
import torch

from conftest import assert_close

EPS = 1e-5
# the project's bars, relative to max|ref| (conftest.assert_close), against fp64 on inputs as stored
FP32_FWD = 1e-5          # fp32 forward / elementwise results, and every statistic
FP32_BWD = 1e-4          # fp32 backward results and sums (fp32-accumulated sums of the bf16 instantiations too)
BF16_STORE = 2.0 ** -8   # tensors stored as bf16
MARGIN = 1e-3
# |mean| / std of the hard-statistics inputs, fixed by the fp32 emulation of the documented algorithm
# (test_norm_ref_cpu.py): the largest of 1e3, 300, 100 at which it meets the statistics bar with 10x to spare
BN_HARD_RATIO = {torch.float32: 300.0, torch.bfloat16: 100.0}
LN_HARD_RATIO = 1e3
BF16 = torch.bfloat16
F32 = torch.float32


def store_bar(dtype, backward=False):
    """Bar of a tensor the kernel stores in ``dtype``."""
    return BF16_STORE if dtype == BF16 else (FP32_BWD if backward else FP32_FWD)


def compare(got, ref, rel, name, scale_floor=0.0):
    """The one comparison of the GPU modules (and of the planted-slip tests): conftest.assert_close, unchanged."""
    assert_close(got, ref, rel, name, scale_floor)


def rnd(t, dtype):
    """Values as stored in ``dtype``, in float64."""
    return t.to(dtype).double()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------ input makers
def draw(shape, seed, dtype, scale=1.0, shift=0.0):
    return rnd(torch.randn(*shape, generator=gen(seed), dtype=torch.float64) * scale + shift, dtype)


def push_out(t, slope, offset, dtype, rel=MARGIN, max_frac=0.01):
    """``t`` (float64 values of ``dtype``) with pre = t*slope + offset: the elements whose |pre| < rel * max|pre| are
    moved (in ``t``, staying values of ``dtype``) until no pre-activation is inside that band.  Asserts that at most
    ``max_frac`` of the elements moved.  Returns the new ``t``."""
    slope = torch.as_tensor(slope, dtype=torch.float64)
    offset = torch.as_tensor(offset, dtype=torch.float64)
    assert bool((torch.as_tensor(slope) != 0).all())
    pre = t * slope + offset
    band = rel * pre.abs().max().item()
    moved = torch.zeros_like(t, dtype=torch.bool)
    out = t.clone()
    for mult in range(2, 40):
        pre = out * slope + offset
        inside = pre.abs() < band
        if not bool(inside.any()):
            break
        moved |= inside
        target = torch.where(pre < 0, -1.0, 1.0) * (mult * band)
        cand = rnd((target - offset) / slope, dtype)
        out = torch.where(inside, cand.expand_as(out), out)
    pre = out * slope + offset
    assert not bool((pre.abs() < rel * pre.abs().max().item()).any()), "push_out: band not cleared"
    frac = moved.double().mean().item()
    assert frac <= max_frac, f"push_out moved {frac:.3%} of the elements"
    return out


def hard_stats(shape, seed, dtype, ratio, axis):
    """|mean| = ratio * std along every slice of ``axis`` (BN: one per channel, axis = the channel axis of [M][C];
    LN: one per frame, axis 0 of [F][V][C]); std in [0.5, 2), the mean's sign alternates."""
    g = gen(seed)
    n = shape[axis]
    bshape = [1] * len(shape)
    bshape[axis] = n
    std = (torch.rand(n, generator=g, dtype=torch.float64) * 1.5 + 0.5).view(bshape)
    sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0).double().view(bshape)
    return rnd(torch.randn(*shape, generator=g, dtype=torch.float64) * std + sign * ratio * std, dtype)


# ------------------------------------------------------------------------------------------ BN statistics
def bn_moments(x):
    """(mean, biased var, rstd) per channel of x [M][C]."""
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def chan_merge(parts):
    """parts [nb][C][>=3] (count, mean, M2) -> (n, mean, M2) per channel: pairwise merge, partial after partial."""
    parts = parts.double()
    n = torch.zeros(parts.shape[1], dtype=torch.float64)
    mean, m2 = n.clone(), n.clone()
    for b in range(parts.shape[0]):
        nb_, mb, qb = parts[b, :, 0], parts[b, :, 1], parts[b, :, 2]
        tot = n + nb_
        safe = torch.where(tot > 0, tot, torch.ones_like(tot))
        d = mb - mean
        mean = mean + d * nb_ / safe
        m2 = m2 + qb + d * d * n * nb_ / safe
        n = tot
    return n, mean, m2


def bn_finalize(parts, gamma=None, beta=None, eps=EPS):
    """(mean, rstd, scale, shift) of the merged partials: biased variance M2 / n; scale = g*rstd, shift = b - mean*scale."""
    n, mean, m2 = chan_merge(parts)
    var = m2 / torch.where(n > 0, n, torch.ones_like(n))
    rstd = 1.0 / torch.sqrt(var + eps)
    g = torch.ones_like(mean) if gamma is None else gamma.double()
    b = torch.zeros_like(mean) if beta is None else beta.double()
    return mean, rstd, g * rstd, b - mean * g * rstd


def bn_merge(parts):
    """[C][4]: one (count, mean, M2, 0) entry per channel."""
    n, mean, m2 = chan_merge(parts)
    return torch.stack([n, mean, m2, torch.zeros_like(n)], 1)


def synth_partials(nb, C, seed, counts=(0, 1, 7, 64)):
    """[nb][C][4] float32 partials: counts drawn from ``counts`` (at least one 0, at least one > 0 per channel), means
    100 +- 0.1 and M2 of order 1 (0 where count <= 1; zero-count entries all 0): the merged variance is ~1e-1 under
    mean^2 = 1e4, which power sums survive in fp64 only."""
    g = gen(seed)
    cnt = torch.tensor(counts, dtype=torch.float64)[torch.randint(len(counts), (nb, C), generator=g)]
    if nb > 1:
        cnt[0] = 0.0
        cnt[-1] = counts[-1]
    else:
        cnt[0] = counts[-1]
    mean = (torch.randn(nb, C, generator=g, dtype=torch.float64) * 0.1 + 100) * (cnt > 0)
    m2 = torch.rand(nb, C, generator=g, dtype=torch.float64) * (cnt > 1)
    return torch.stack([cnt, mean, m2, torch.zeros_like(cnt)], -1).float()


# ------------------------------------------------------------------------------------------ bn_apply
def bn_apply(u, sc, sh, res_mode=0, r=None, rsc=None, rsh=None, relu=1):
    """y [M][C] (float64, before the storage rounding) and the value the final ReLU (or none) is applied to."""
    t = u * sc + sh
    if relu & 2:
        t = t.clamp(min=0)
    if res_mode == 1:
        t = t + r
    elif res_mode == 2:
        t = t + r * rsc + rsh
    return (t.clamp(min=0) if relu & 1 else t), t


def pack_bits(pos):
    """bool [M][C] -> uint8 [M][C / 8], bit c % 8 of byte c / 8."""
    M, C = pos.shape
    w = (2 ** torch.arange(8)).to(torch.int64)
    return (pos.view(M, C // 8, 8).to(torch.int64) * w).sum(-1).to(torch.uint8)


def bn_bits(y, dtype=BF16):
    """The sign bits of the STORED output: > 0, i.e. nonzero with the sign clear."""
    return pack_bits(rnd(y, dtype) > 0)


def unpack_bits(bits, C):
    M = bits.shape[0]
    return ((bits.view(M, C // 8, 1).to(torch.int64) >> torch.arange(8)) & 1).view(M, C).bool()


# ------------------------------------------------------------------------------------------ BN backward
def relu_mask(mask, mref=None, msc=None, msh=None, C=None):
    if mask == 0:
        return None
    if mask == 1:
        return mref > 0
    if mask == 2:
        return mref * msc + msh > 0
    return unpack_bits(mref, C)


def bn_bwd(dy, mask=0, mref=None, msc=None, msh=None, x1=None, mr1=None, g1=None, x2=None, mr2=None, g2=None,
           identity2=False, old2=None):
    """Everything the BN backward kernels produce, float64, from [M][C] inputs; mr = [C][2] (mean, rstd).
    x1 None: out1 = dz (the unfused kernels' identity branch).  out2: BN branch when x2 is given, dz when
    ``identity2``; ``old2`` (acc2 / accumulate) is added.  Returns a dict."""
    M, C = dy.shape
    m = relu_mask(mask, mref, msc, msh, C)
    dz = dy if m is None else dy * m
    S0 = dz.sum(0)
    out = {"dz": dz, "S0": S0}

    def branch(x, mr, g):
        xh = (x - mr[:, 0]) * mr[:, 1]
        S = (dz * xh).sum(0)
        gg = torch.ones(C, dtype=torch.float64) if g is None else g.double()
        return S, gg * mr[:, 1] * (dz - S0 / M - xh * S / M)

    if x1 is not None:
        out["S1"], out["out1"] = branch(x1, mr1.double(), g1)
    else:
        out["S1"], out["out1"] = torch.zeros_like(S0), dz.clone()
    out["S2"] = torch.zeros_like(S0)
    if x2 is not None:
        out["S2"], out["out2"] = branch(x2, mr2.double(), g2)
    elif identity2:
        out["out2"] = dz.clone()
    if "out2" in out and old2 is not None:
        out["out2"] = out["out2"] + old2
    out["osum1"] = out["out1"].sum(0)
    if "out2" in out:
        out["osum2"] = out["out2"].sum(0)
    return out


# ------------------------------------------------------------------------------------------ LayerNorm
def ln_stats(x, eps=EPS, unbiased=True):
    """x [F][V][C] -> (mean [F], rstd [F]); unbiased variance (torch.var's default)."""
    F = x.shape[0]
    flat = x.reshape(F, -1)
    mean = flat.mean(1)
    E = flat.shape[1]
    var = ((flat - mean[:, None]) ** 2).sum(1) / (E - 1 if unbiased else E)
    return mean, 1.0 / torch.sqrt(var + eps)


def ln_norm(x, st, g, b):
    """xhat [F][V][C] and xhat*g + b; st [F][2]; g, b [C][V] (element c*V + v of the kernels' flat vectors)."""
    xh = (x - st[:, 0, None, None]) * st[:, 1, None, None]
    return xh, xh * g.t() + b.t()


def ln_apply(u, st, g, b, res_mode=0, r=None, rst=None, rg=None, rb=None, relu=1):
    _, t = ln_norm(u, st, g, b)
    if relu & 2:
        t = t.clamp(min=0)
    if res_mode == 1:
        t = t + r
    elif res_mode == 2:
        t = t + ln_norm(r, rst, rg, rb)[1]
    return t.clamp(min=0) if relu & 1 else t


def ln_bwd(dy, x, st, g, b, mask=0, mref=None, old=None, e_minus=1):
    """(dx [F][V][C], dgamma [C][V], dbeta [C][V]); mask 0 none | 1 mref > 0 | 2 xhat*g + b > 0."""
    xh, pre = ln_norm(x, st, g, b)
    dz = dy
    if mask == 1:
        dz = dy * (mref > 0)
    elif mask == 2:
        dz = dy * (pre > 0)
    E = x.shape[1] * x.shape[2]
    gz = dz * g.t()
    k1 = gz.sum((1, 2), keepdim=True) / E
    k2 = (gz * xh).sum((1, 2), keepdim=True) / (E - e_minus)
    dx = st[:, 1, None, None] * (gz - k1 - xh * k2)
    if old is not None:
        dx = dx + old
    return dx, (dz * xh).sum(0).t(), dz.sum(0).t()


def ln_dy(x, st, seed, dtype):
    """Upstream gradient with a component along xhat, so the backward's second term (xhat * sum(gz*xhat) / (E-1)) is
    of the order of the first."""
    xh = (x - st[:, 0, None, None]) * st[:, 1, None, None]
    return rnd(torch.randn(x.shape, generator=gen(seed), dtype=torch.float64) + 0.7 * xh, dtype)


def bn_dy(x, mr, seed, dtype):
    """The same for BN: dy = noise + 0.5 * xhat, so S1 (and with it k2, k3) is of the order of M."""
    return rnd(torch.randn(x.shape, generator=gen(seed), dtype=torch.float64) + 0.5 * (x - mr[:, 0]) * mr[:, 1], dtype)


# ------------------------------------------------------------------------------------------ fp32 emulation
def emulate_bn_stats_fp32(x, vec, rpb):
    """The documented BN statistics algorithm in float32 numpy, on x [M][C] (float32 values): every thread owns the
    rows (block start + row slot + k * RPI) of one channel unit and keeps sums of (x - k0) and (x - k0)^2 shifted by
    its first value k0; its (n, mean, M2) is merged with the other row slots' in fp32 (Chan), and the blocks'
    partials are merged through fp64 power sums (n, sum n*mean, sum M2 + n*mean^2).  Returns fp64 (mean, rstd) as
    the kernel would hand them on, rounded to fp32."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    M, C = x.shape
    rpi = max(256 // (C // vec), 1)
    n_t = s1_t = s2_t = 0.0
    for mb in range(0, M, rpb):
        blk = x[mb:min(M, mb + rpb)]
        wn = np.zeros(C, f)
        wm = np.zeros(C, f)
        wq = np.zeros(C, f)
        for rs in range(rpi):
            rows_ = blk[rs::rpi]
            n = f(rows_.shape[0])
            if n > 0:
                k0 = rows_[0]
                s1 = np.zeros(C, f)
                s2 = np.zeros(C, f)
                for row in rows_:
                    d = (row - k0).astype(f)
                    s1 = (s1 + d).astype(f)
                    s2 = (s2 + (d * d).astype(f)).astype(f)
                mean = (k0 + (s1 / n).astype(f)).astype(f)
                m2 = np.maximum((s2 - ((s1 * s1).astype(f) / n).astype(f)).astype(f), f(0))
            else:
                mean = np.zeros(C, f)
                m2 = np.zeros(C, f)
            tot = f(wn[0] + n)
            if tot == 0:
                continue
            d = (mean - wm).astype(f)
            fb = f(n / tot)
            wq = (((wq + m2).astype(f)) + (((d * d).astype(f) * wn).astype(f) * fb).astype(f)).astype(f)
            wm = (wm + (d * fb).astype(f)).astype(f)
            wn = np.full(C, tot, f)
        cnt, mu = wn.astype(np.float64), wm.astype(np.float64)
        n_t = n_t + cnt
        s1_t = s1_t + cnt * mu
        s2_t = s2_t + wq.astype(np.float64) + cnt * mu * mu
    m = s1_t / n_t
    var = np.maximum(s2_t / n_t - m * m, 0.0)
    rstd = (1.0 / np.sqrt(var + EPS)).astype(f)
    return torch.from_numpy(m.astype(f).astype(np.float64)), torch.from_numpy(rstd.astype(np.float64))


def emulate_ln_stats_fp32(x):
    """ln_stats as documented, float32 numpy, x [F][E] (float32 values, the frame's elements in memory order with the
    unit structure flattened away): 64 lanes, lane l takes elements l, l + 64, ...; sums of (x - K) and (x - K)^2
    with K the frame's first element; a butterfly over the lanes; var = (s2 - s1*s1/E) / (E - 1)."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    F, E = x.shape
    mean = np.zeros(F, f)
    rstd = np.zeros(F, f)
    for i in range(F):
        K = x[i, 0]
        pad = (-E) % 64
        d = np.concatenate([(x[i] - K).astype(f), np.zeros(pad, f)]).reshape(-1, 64)
        s1 = np.zeros(64, f)
        s2 = np.zeros(64, f)
        for row in d:
            s1 = (s1 + row).astype(f)
            s2 = (s2 + (row * row).astype(f)).astype(f)
        for o in (32, 16, 8, 4, 2, 1):
            idx = np.arange(64) ^ o
            s1 = (s1 + s1[idx]).astype(f)
            s2 = (s2 + s2[idx]).astype(f)
        md = f(s1[0] / f(E))
        var = max(f(f(s2[0] - f(s1[0] * md)) / f(E - 1)), f(0))
        mean[i] = f(K + md)
        rstd[i] = f(1) / np.sqrt(f(var + f(EPS)))
    return torch.from_numpy(mean.astype(np.float64)), torch.from_numpy(rstd.astype(np.float64))
