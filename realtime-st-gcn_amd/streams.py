"""What the per-frame (continual inference) routes share on the host: the stream-batch surface of
``rtstgcn.RtStreamBatch`` and ``costgcn.CoStreamBatch``, and the helpers their descriptor builders fill with."""
from __future__ import annotations

import torch

from . import layer_fn as LF
from . import native as K


class Keep(list):
    """The tensors a descriptor points to, kept alive with it: ``keep(t)`` records ``t`` and returns its address."""

    def __call__(self, t):
        self.append(t)
        return t.data_ptr()


def f32(t):
    return t.detach().float().contiguous()


def res_mode_of(layer):
    """The kernels' residual code: 0 none, 1 identity, 2 residual conv + LayerNorm."""
    return 2 if layer.is_residual_conv else (1 if layer.is_residual else 0)


def ln_rows(t, C, V):
    """LayerNorm([C,1,V]) affine (C,1,V) -> the rows' [V][C] layout."""
    return t.detach().float().reshape(C, V).t().contiguous()


def fill_heads(d, model, keep):
    """The six head pointers of a per-frame descriptor (RtFrameDesc, RtStreamsDesc, CoStreamsDesc): norm_in, fcn_in,
    fcn_out of ``model``."""
    d.ln_w, d.ln_b = keep(LF._flat_ln(model.norm_in.weight)), keep(LF._flat_ln(model.norm_in.bias))
    d.w_in = keep(f32(model.fcn_in.weight).reshape(model.fcn_in.out_channels, -1))
    d.b_in = keep(f32(model.fcn_in.bias))
    d.w_out = keep(f32(model.fcn_out.weight).reshape(model.fcn_out.out_channels, -1))
    d.b_out = keep(f32(model.fcn_out.bias))


class StreamBatch:
    """B independent skeleton streams of one per-frame model.  A subclass keeps ``state`` (per layer, a tuple of
    stream-major device tensors), builds its descriptor in ``_desc()`` -> (descriptor, keep-alive list) and launches
    one tick in ``_launch(d, x, active, out)``."""

    @staticmethod
    def _check_B(B):
        if int(B) != B or B < 1:
            raise RuntimeError(f"stgcn_amd: stream_batch needs B >= 1, got {B}")

    def __init__(self, model, B):
        self._check_B(B)
        K.L.require_device(model.A)
        self.model, self.B, self.V = model, int(B), model.A.shape[-1]
        self._all = torch.ones(self.B, dtype=torch.int32, device=model.A.device)
        self.state, self._pack = [], None

    @property
    def state_bytes(self):
        return sum(t.numel() * t.element_size() for ts in self.state for t in ts)

    def step(self, x, active=None):
        """x (B, 3, 1, V) -> (B, num_classes, 1).  ``active``: None (every stream steps), an int32 device tensor
        [B] of codes (0 skip: state untouched, zero output row; 1 step; 2 restart then step) used as given with no
        host sync, or a bool tensor / Python list converted on the host (True = step)."""
        B, V, name = self.B, self.V, type(self).__name__
        if x.dim() != 4 or tuple(x.shape) != (B, 3, 1, V):
            raise RuntimeError(f"stgcn_amd: {name}.step expects x of shape {(B, 3, 1, V)}, got {tuple(x.shape)}")
        K.L.require_device(x)
        x = K._f32c(x)
        if active is None:
            active = self._all
        elif not (torch.is_tensor(active) and active.dtype == torch.int32 and active.is_cuda):
            active = torch.as_tensor(active).to(device=x.device, dtype=torch.int32)
        if tuple(active.shape) != (B,) or not active.is_contiguous():
            raise RuntimeError(f"stgcn_amd: {name}.step expects active of shape ({B},)")
        d, _keep = self._desc()
        out = torch.empty((B, d.K, 1), dtype=torch.float32, device=x.device)
        return self._launch(d, x, active, out)
