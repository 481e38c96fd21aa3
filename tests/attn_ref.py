"""Plain-PyTorch restatement of the AAGCN attention adjacency (models/aagcn/aagcn.py:142-145) on logical
(N, P*ce, T, V) tensors, in any dtype: what tests/test_gpu_attn.py holds attn.hip and mode 2 of jmix.hip to.

    S[n,p,v,w] = sum_{t,c} theta[n,p*ce+c,t,v] * phi[n,p*ce+c,t,w];   C = softmax_w(S)

``attn_ref`` takes the gradients from autograd.  ``attn_manual`` writes the same backward out by hand (dS = C * (dC -
sum_w dC*C), dtheta = dS-mix of phi, dphi = dS^T-mix of theta) so that it can also be evaluated *wrongly*, the way a
subtly broken kernel would: tests/test_attn_ref_cpu.py feeds those variants to the GPU test's own comparison
(``attn_compare``) and requires each to be rejected.

The inputs are scaled so that the logits have a standard deviation of about 2: with the near-uniform softmax of
freshly initialised projections dS is tiny and a wrong dtheta / dphi would change nothing a test can see.  Every
reference built here asserts that its softmax is peaked (``assert_peaked``).
"""
import functools
from types import SimpleNamespace

import torch

from conftest import assert_close

# (N, P, ce, T, V): the GPU parametrisation, one line of intent each
SHAPES = [
    (2, 3, 16, 37, 25),  # 16-B score loads; 5 T chunks, the last of 5 frames; blocks straddling partitions + 16-ch tail
    (3, 3, 16, 5, 25),   # one wave walks 30 items across three samples (coefficients reloaded twice)
    (1, 3, 16, 1, 25),   # 2 items: a ring shorter than its depth; K = 16 < 64
    (3, 3, 12, 8, 18),   # scalar score loads; jmix block 0 holds three partitions, block 1 is a 4-channel tail
    (1, 3, 4, 9, 25),    # the narrow-golden width (12 channels: three partitions in a partial block)
    (2, 2, 64, 19, 25),  # ce > 32: blocks inside a partition
    (2, 1, 8, 1, 3),     # smallest
    (1, 4, 16, 20, 32),  # P = 4: jmix declines, the gather mix runs; V = VMAX
    (2, 3, 6, 11, 25),   # ce % 4 != 0: gather mix + scalar score loads
]
PEAK_RANGE = (0.25, 0.9)
FP32_REL = 1e-4          # the fp32 kernel-level bar of tests/test_gpu_kernels.py
BF16_STORE_REL = 2.0 ** -8  # outputs stored as bf16: half an ulp of the storage rounding (2^-9 of the value), times two


def shape_id(s):
    return "N%d-P%d-ce%d-T%d-V%d" % s


def attn_inputs(N, P, ce, T, V, seed):
    """theta, phi ~ randn * (4 / (T*ce))**0.25 (logits: T*ce products of variance 4/(T*ce), std ~2) and a unit-normal
    dC, fp32 on the CPU from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    s = (4.0 / (T * ce)) ** 0.25
    theta = torch.randn(N, P * ce, T, V, generator=g) * s
    phi = torch.randn(N, P * ce, T, V, generator=g) * s
    dC = torch.randn(N, P, V, V, generator=g)
    return theta, phi, dC


def _scores(theta, phi, P):
    N, CH, T, V = theta.shape
    ce = CH // P
    th = theta.reshape(N, P, ce, T, V)
    ph = phi.reshape(N, P, ce, T, V)
    return torch.einsum("npctv,npctw->npvw", th, ph)


def attn_ref(theta, phi, P, dC, dtype=torch.float64):
    """(C, dtheta, dphi) in ``dtype``: the forward above and autograd's gradients of sum(C * dC)."""
    th = theta.detach().to(dtype).requires_grad_(True)
    ph = phi.detach().to(dtype).requires_grad_(True)
    C = torch.softmax(_scores(th, ph, P), dim=3)
    dth, dph = torch.autograd.grad(C, (th, ph), dC.to(dtype))
    return C.detach(), dth, dph


def peakedness(C):
    return C.max(dim=3).values.mean().item()


def assert_peaked(C, name=""):
    m = peakedness(C)
    assert PEAK_RANGE[0] <= m <= PEAK_RANGE[1], \
        f"{name}: mean max_w C = {m:.3f} outside {PEAK_RANGE}: the softmax is not peaked, the backward test is blind"


VARIANTS = ("ds_untransposed", "block_first_partition", "last_t_chunk_dropped", "uniform_c", "sample0_coefficients")


def variant_applies(variant, shape):
    """Whether the wrong variant differs from the right answer at this shape at all."""
    N, P, ce, T, V = shape
    if variant == "block_first_partition":  # some 32-channel block must hold more than one partition
        return any((32 * b) // ce != min(P * ce - 1, 32 * b + 31) // ce for b in range((P * ce + 31) // 32))
    if variant == "sample0_coefficients":
        return N > 1
    return True


def attn_manual(theta, phi, P, dC, dtype=torch.float64, variant=None):
    """(C, dtheta, dphi) written out by hand; ``variant`` (one of VARIANTS) evaluates a known-wrong kernel:

    ds_untransposed        dphi mixed with dS instead of dS^T
    block_first_partition  every channel of a 32-channel block mixed with the block's first partition's coefficients
    last_t_chunk_dropped   the last chunk of 8 frames missing from S
    uniform_c              C = 1/V
    sample0_coefficients   the mixes of every sample use sample 0's dS
    """
    assert variant is None or variant in VARIANTS
    th, ph, g = theta.to(dtype), phi.to(dtype), dC.to(dtype)
    N, CH, T, V = th.shape
    ce = CH // P
    if variant == "last_t_chunk_dropped":
        keep = 8 * ((T - 1) // 8)
        S = _scores(th[:, :, :keep], ph[:, :, :keep], P)
    else:
        S = _scores(th, ph, P)
    C = torch.softmax(S, dim=3)
    if variant == "uniform_c":
        C = torch.full_like(C, 1.0 / V)
    dS = C * (g - (g * C).sum(dim=3, keepdim=True))  # [N][P][v][w]
    if variant == "sample0_coefficients":
        dS = dS[:1].expand(N, -1, -1, -1)
    part = torch.arange(CH) // ce  # partition whose coefficients mix channel ch
    if variant == "block_first_partition":
        part = (32 * (torch.arange(CH) // 32)) // ce
    M = dS[:, part]  # [N][CH][v][w]
    dth = torch.einsum("ncvw,nctw->nctv", M, ph)
    if variant == "ds_untransposed":
        dph = torch.einsum("ncwv,nctv->nctw", M, th)
    else:
        dph = torch.einsum("ncvw,nctv->nctw", M, th)
    return C, dth, dph


def attn_compare(got, ref, rel=FP32_REL, rel_grad=None, name=""):
    """The GPU tests' acceptance: each of C / dtheta / dphi present in ``got`` against the reference, max-norm
    relative to max|ref| (conftest.assert_close).  ``rel_grad``: another bar for dtheta / dphi (bf16 storage)."""
    rel_grad = rel if rel_grad is None else rel_grad
    for key, r in (("C", rel), ("dtheta", rel_grad), ("dphi", rel_grad)):
        if got.get(key) is not None:
            assert_close(got[key], getattr(ref, key), r, f"{name} {key}".strip())


@functools.lru_cache(maxsize=None)
def attn_case(shape, bf16=False):
    """Inputs and fp64 reference of one shape, computed once and shared (treat as read-only).  ``bf16``: theta and
    phi rounded to bf16 first (what the bf16 instantiations are given), the reference evaluated on those values."""
    N, P, ce, T, V = shape
    theta, phi, dC = attn_inputs(N, P, ce, T, V, seed=1000 + SHAPES.index(shape))
    if bf16:
        theta, phi = theta.bfloat16().float(), phi.bfloat16().float()
    C, dth, dph = attn_ref(theta, phi, P, dC, torch.float64)
    assert_peaked(C, shape_id(shape))
    return SimpleNamespace(shape=shape, P=P, CH=P * ce, theta=theta, phi=phi, dC=dC, C=C, dtheta=dth, dphi=dph)
