"""MS-TCN (models/mstcn/mstcn.py) on the HIP kernels of ms_stage.hip: ``SingleStage``, ``DilatedResidualLayer`` and
the ``ms-tcn`` ``Model``; msgcn.py builds ``ms-gcn`` from the same stage.

Parameter names and shapes are the reference's (``generator_stage.conv_in.weight`` (F, Cin, 1, 1),
``...layers.{j}.conv.0.weight`` (F, F, 3, 1), ``...conv.2.weight``, ``conv_out.*``, ``refinement_stages.{i}...``), so
checkpoints load with ``strict=True`` both ways.  The modules hold parameters only; a stage runs as one autograd
function (``StageFunction``): conv_in with the ``refine`` selector fused in front, one launch per dilated residual
layer (plus its weight pack), and conv_out with the mean over the joints fused in front; the backward runs the
matching gradient kernels.  The residual stream stays fp32; ``set_compute_dtype('bf16')`` rounds the layers' MFMA
operands and the saved hidden activations to bf16.  There is no eager path: off the device every stage raises.

``Model.forward(x (1, in_feat, L, V)) -> (stages, 1, num_classes, L)`` fp32: slice 0 is the generator stage pooled
over the joints, slice i the i-th refinement stage, each through the ``output_type`` selector.

Scope (anything else is refused on the host, before any launch): kernel 3 (the reference's ``padding=dilation`` keeps
the length only then), filters in {16, 32, 48, 64}, dropout 0 when training, num_classes and in_feat <= 64,
V <= 32 and batch 1, and L * V * dilation within int range.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from . import native as K
from .modules import resolve_dtype

INT_MAX = 2 ** 31 - 1


def check_stage_config(num_filters, kernel, in_channels, out_channels):
    if kernel != 3:
        raise NotImplementedError(f"stgcn_amd: ms-tcn stages support kernel 3 only, got {kernel} (the reference's "
                                  "padding=dilation keeps the sequence length only for kernel 3)")
    if num_filters % 16 or not 16 <= num_filters <= 64:
        raise NotImplementedError(f"stgcn_amd: ms-tcn stages support filters in {{16, 32, 48, 64}}, got {num_filters}")
    if not (1 <= in_channels <= 64 and 1 <= out_channels <= 64):
        raise NotImplementedError(f"stgcn_amd: ms-tcn stages support at most 64 input features / classes "
                                  f"(num_classes), got {in_channels} -> {out_channels}")


class DilatedResidualLayer(nn.Module):
    """mstcn.py:97-116: x + conv1x1(ReLU(dilated conv3(x))); the parameters of one ms_layer launch."""

    def __init__(self, in_channels=64, out_channels=64, kernel=3, dilation=1, dropout=0.5):
        super().__init__()
        check_stage_config(out_channels, kernel, in_channels, out_channels)
        if in_channels != out_channels:
            raise NotImplementedError("stgcn_amd: a dilated residual layer keeps its width")
        self.dilation = dilation
        self.dropout = dropout
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, (kernel, 1), padding=(dilation, 0), dilation=(dilation, 1)),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_channels, out_channels, 1),
            nn.Dropout(dropout, inplace=True))

    def forward(self, x):
        raise RuntimeError("stgcn_amd: a DilatedResidualLayer runs inside its SingleStage (one fused stage function)")


@K.on_tensor_device
class StageFunction(torch.autograd.Function):
    """rows [L * V][Cin] fp32 -> [L * V / pool][Cout]: selector(mode) + conv_in, the dilated residual layers (row
    offset dilation * V), mean over ``pool`` joints + conv_out.  params: conv_in w, b; per layer conv.0 w, b,
    conv.2 w, b; conv_out w, b."""

    @staticmethod
    def forward(ctx, x, V, pool, mode, dtype, *params):
        nl = (len(params) - 4) // 4
        save = any(ctx.needs_input_grad)
        x = K._rows32(x.detach())
        w_in, b_in, w_out, b_out = params[0], params[1], params[-2], params[-1]
        a, p = K.ms_lin_fwd("in", x, w_in, b_in, 1, mode, save)
        xs, hs, packs = [], [], []
        for j in range(nl):
            w1, b1, w2, b2 = params[2 + 4 * j:6 + 4 * j]
            wp = K.ms_pack_layer(w1, w2, dtype)
            y, h = K.ms_layer_fwd(a, wp, b1, b2, V, 2 ** j, dtype, save)
            if save:
                xs.append(a), hs.append(h), packs.append(wp)
            a = y
        out, am = K.ms_lin_fwd("out", a, w_out, b_out, pool, 0, save)
        if save:
            ctx.save_for_backward(p, am, w_in.detach(), w_out.detach(), *xs, *hs, *packs)
        ctx.cfg = (V, pool, mode, dtype, nl, tuple(t.shape for t in params))
        return out

    @staticmethod
    def backward(ctx, dout):
        V, pool, mode, dtype, nl, shapes = ctx.cfg
        p, am, w_in, w_out, *rest = ctx.saved_tensors
        xs, hs, packs = rest[:nl], rest[nl:2 * nl], rest[2 * nl:]
        grads = [None] * len(shapes)

        def put(i, flat, o):
            n = shapes[i].numel()
            grads[i] = flat[o:o + n].view(shapes[i])
            return o + n

        d, g = K.ms_lin_bwd("out", K._rows32(dout), am, w_out, pool, 0, True)
        put(len(shapes) - 1, g, put(len(shapes) - 2, g, 0))
        for j in reversed(range(nl)):
            d, g = K.ms_layer_bwd(xs[j], packs[j], hs[j], d, V, 2 ** j, dtype)
            o = 0
            for i in range(2 + 4 * j, 6 + 4 * j):
                o = put(i, g, o)
        din, g = K.ms_lin_bwd("in", d, p, w_in, 1, mode, ctx.needs_input_grad[0])
        put(1, g, put(0, g, 0))
        return (din, None, None, None, None, *grads)


@K.on_tensor_device
class ProbFunction(torch.autograd.Function):
    """The ``output_type`` selector on rows [L][C]: log-softmax (mode 1) | softmax (mode 2) over the classes."""

    @staticmethod
    def forward(ctx, x, mode):
        y = K.ms_prob_fwd(K._rows32(x.detach()), mode)
        ctx.save_for_backward(y)
        ctx.mode = mode
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return K.ms_prob_bwd(y, K._rows32(dy), ctx.mode), None


class SingleStage(nn.Module):
    """mstcn.py:68-94."""

    def __init__(self, in_channels=None, out_channels=None, num_filters=64, num_layers=10, kernel=3, dropout=0.0):
        super().__init__()
        check_stage_config(num_filters, kernel, in_channels, out_channels)
        self.dropout = dropout
        self.conv_in = nn.Conv2d(in_channels, num_filters, 1)
        self.layers = nn.Sequential(*[DilatedResidualLayer(in_channels=num_filters, out_channels=num_filters,
                                                           kernel=kernel, dilation=2 ** i, dropout=dropout)
                                      for i in range(num_layers)])
        self.conv_out = nn.Conv2d(num_filters, out_channels, 1)
        self.compute_dtype = torch.float32

    def run_rows(self, rows, V, pool=1, mode=0):
        """rows [L * V][Cin] -> [L * V / pool][Cout] (see StageFunction); every refusal precedes the device check."""
        if self.training and self.dropout > 0:
            raise NotImplementedError("stgcn_amd: ms-tcn stages do not implement dropout > 0 in training")
        if rows.dim() != 2 or rows.shape[1] != self.conv_in.in_channels or rows.shape[0] < 1 or rows.shape[0] % V:
            raise RuntimeError(f"stgcn_amd: stage expects [L * {V}][{self.conv_in.in_channels}] rows, got "
                               f"{tuple(rows.shape)}")
        if pool not in (1, V) or V > 32 and pool > 1:
            raise NotImplementedError(f"stgcn_amd: ms-tcn pools over at most 32 joints, got V = {V}")
        if len(self.layers) and rows.shape[0] * 2 ** (len(self.layers) - 1) > INT_MAX:
            raise NotImplementedError(f"stgcn_amd: L * V * dilation = {rows.shape[0]} * "
                                      f"{2 ** (len(self.layers) - 1)} exceeds the kernels' int row arithmetic")
        L.require_device(rows)
        params = [self.conv_in.weight, self.conv_in.bias]
        for layer in self.layers:
            params += [layer.conv[0].weight, layer.conv[0].bias, layer.conv[2].weight, layer.conv[2].bias]
        params += [self.conv_out.weight, self.conv_out.bias]
        return StageFunction.apply(rows, V, pool, mode, self.compute_dtype, *params)

    def forward(self, x):
        """(1, Cin, L, V) -> (1, Cout, L, V), like the reference's stage (no pooling, no selector)."""
        if x.dim() != 4 or x.shape[0] != 1:
            raise NotImplementedError(f"stgcn_amd: ms-tcn stages take batch 1, got {tuple(x.shape)}")
        _, C, Lx, V = x.shape
        y = self.run_rows(x[0].permute(1, 2, 0).reshape(Lx * V, C).float(), V)
        return y.view(Lx, V, -1).permute(2, 0, 1).unsqueeze(0)


def selector_mode(name, what):
    if name not in K.MS_MODES:
        raise ValueError(f"unknown {what} {name!r}")
    return K.MS_MODES[name]


def refine_and_stack(x, stages, refine_mode, out_mode):
    """x [L][C]: the generator's series.  Runs the refinement stages (selector fused into each conv_in) and returns
    (1 + len(stages), 1, C, L) with the ``output_type`` selector on every slice (mstcn.py:60-65)."""
    outs = [x]
    for stage in stages:
        x = stage.run_rows(x, 1, 1, refine_mode)
        outs.append(x)
    if out_mode:
        outs = [ProbFunction.apply(o, out_mode) for o in outs]
    return torch.stack(outs).permute(0, 2, 1).unsqueeze(1)


class Model(nn.Module):
    """mstcn.py:6-65."""

    def __init__(self, rank=None, **kwargs):
        super().__init__()
        conf = kwargs["ms-tcn"]
        self.stages = conf["stages"]
        self.num_classes = kwargs["num_classes"]
        self.generator_stage = SingleStage(in_channels=conf["in_feat"], out_channels=kwargs["num_classes"],
                                           num_filters=conf["filters"][0], num_layers=conf["layers"][0],
                                           kernel=conf["kernel"][0], dropout=conf["dropout"][0])
        self.refinement_stages = nn.ModuleList([
            SingleStage(in_channels=kwargs["num_classes"], out_channels=kwargs["num_classes"],
                        num_filters=conf["filters"][i], num_layers=conf["layers"][i], kernel=conf["kernel"][i],
                        dropout=conf["dropout"][i]) for i in range(1, conf["stages"])])
        self.refine_mode = selector_mode(kwargs["refine"], "refine")
        self.out_mode = selector_mode(kwargs["output_type"], "output_type")
        self.compute_dtype = torch.float32

    def set_compute_dtype(self, dtype):
        """fp32 (parity) or bf16 MFMA operands and saved activations in every stage."""
        self.compute_dtype = resolve_dtype(dtype)
        for m in self.modules():
            if isinstance(m, SingleStage):
                m.compute_dtype = self.compute_dtype
        return self

    def forward(self, x):
        if x.dim() != 4 or x.shape[0] != 1:
            raise NotImplementedError(f"stgcn_amd: ms-tcn takes one (1, in_feat, L, V) capture, got {tuple(x.shape)}")
        _, C, Lx, V = x.shape
        if V > 32:
            raise NotImplementedError(f"stgcn_amd: ms-tcn pools over at most 32 joints, got V = {V}")
        rows = x[0].permute(1, 2, 0).reshape(Lx * V, C).float()
        y = self.generator_stage.run_rows(rows, V, V, 0)                                    # mstcn.py:55-60
        return refine_and_stack(y, self.refinement_stages, self.refine_mode, self.out_mode)

    def prepare_benchmark(self, arch_conf):
        return arch_conf
