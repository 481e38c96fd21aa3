"""The attention restatement of tests/attn_ref.py without a GPU: it is the oracle's formula, its inputs make the
softmax peaked at every shape the GPU test uses, and the GPU test's acceptance rejects known-wrong kernels."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402
from conftest import assert_close  # noqa: E402
from oracle import stgcn_oracle as O  # noqa: E402

IDS = [R.shape_id(s) for s in R.SHAPES]


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_restatement_is_the_oracle_formula(shape, monkeypatch):
    """oracle.stgcn_oracle.agcn_layer itself, with the StgcnLayer it ends in replaced by a probe that returns the
    adjacency it is handed (A = B = 0, so A + B + C = C): view(N, P, ce*L, V), matmul, softmax(dim=3)."""
    N, P, ce, T, V = shape
    CH = P * ce
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, 5, T, V, generator=g, dtype=torch.float64)
    sd = {"theta.weight": torch.randn(CH, 5, 1, 1, generator=g, dtype=torch.float64),
          "theta.bias": torch.randn(CH, generator=g, dtype=torch.float64),
          "phi.weight": torch.randn(CH, 5, 1, 1, generator=g, dtype=torch.float64),
          "phi.bias": torch.randn(CH, generator=g, dtype=torch.float64),
          "B": torch.zeros(P, V, V, dtype=torch.float64)}
    monkeypatch.setattr(O, "stgcn_layer", lambda x_, A_eff, *a, **k: A_eff)
    C_oracle = O.agcn_layer(x, torch.zeros(P, V, V, dtype=torch.float64), sd, "", 9, 1, True, "BatchNorm", P)
    theta = torch.nn.functional.conv2d(x, sd["theta.weight"], sd["theta.bias"])
    phi = torch.nn.functional.conv2d(x, sd["phi.weight"], sd["phi.bias"])
    C, _, _ = R.attn_ref(theta, phi, P, torch.zeros(N, P, V, V), torch.float64)
    assert C.shape == C_oracle.shape == (N, P, V, V)
    assert (C - C_oracle).abs().max().item() <= 1e-13


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32-inputs", "bf16-inputs"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_inputs_make_the_softmax_peaked(shape, bf16):
    """attn_case asserts the condition itself; this runs it for the whole GPU parametrisation and checks the
    logits' scale the condition comes from."""
    case = R.attn_case(shape, bf16)
    assert R.PEAK_RANGE[0] <= R.peakedness(case.C) <= R.PEAK_RANGE[1]
    if os.environ.get("STGCN_TEST_REPORT"):
        print(f"[peak] {R.shape_id(shape)} bf16={bf16}: {R.peakedness(case.C):.3f}", flush=True)
    if case.C.numel() >= 1000:  # enough logits for a standard deviation
        std = R._scores(case.theta.double(), case.phi.double(), case.P).std().item()
        assert 1.5 <= std <= 2.5, f"logit std {std:.2f}"


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_manual_backward_and_fp32_floor(shape):
    """The hand-written backward (what the wrong variants are cut from) is autograd's to fp64 rounding, and the
    reference evaluated in fp32 sits far below the bar the kernels are held to (<= 5e-6 against 1e-4)."""
    case = R.attn_case(shape)
    C, dth, dph = R.attn_manual(case.theta, case.phi, case.P, case.dC)
    R.attn_compare({"C": C, "dtheta": dth, "dphi": dph}, case, rel=1e-12)
    C32, dth32, dph32 = R.attn_ref(case.theta, case.phi, case.P, case.dC, torch.float32)
    R.attn_compare({"C": C32, "dtheta": dth32, "dphi": dph32}, case, rel=5e-6, name="fp32 reference")


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_wrong_variants_are_rejected(shape, variant):
    """The GPU test's comparison at its fp32 tolerance raises for each known-wrong kernel, on every shape where the
    variant differs from the right answer at all."""
    case = R.attn_case(shape)
    C, dth, dph = R.attn_manual(case.theta, case.phi, case.P, case.dC, variant=variant)
    got = {"C": C, "dtheta": dth, "dphi": dph}
    if not R.variant_applies(variant, shape):
        R.attn_compare(got, case, rel=1e-12)  # the variant is the right answer here: nothing to reject
        return
    with pytest.raises(AssertionError):
        R.attn_compare(got, case, rel=R.FP32_REL)
    # and at the bf16 storage bar for the gradients (C keeps the fp32 bar there)
    with pytest.raises(AssertionError):
        R.attn_compare(got, case, rel=R.FP32_REL, rel_grad=R.BF16_STORE_REL)


def test_every_variant_applies_somewhere():
    for variant in R.VARIANTS:
        assert any(R.variant_applies(variant, s) for s in R.SHAPES), variant
    # the straddling shapes the issue names are among them
    assert R.variant_applies("block_first_partition", R.SHAPES[0])
    assert R.variant_applies("block_first_partition", R.SHAPES[3])


def test_compare_accepts_rounding_noise():
    """The acceptance is not so tight that fp32 rounding of a right answer fails it."""
    case = R.attn_case(R.SHAPES[0])
    got = {k: getattr(case, k).float() for k in ("C", "dtheta", "dphi")}
    R.attn_compare(got, case, rel=R.FP32_REL)
    assert_close(case.dtheta.bfloat16(), case.dtheta, R.BF16_STORE_REL, "bf16 storage")
