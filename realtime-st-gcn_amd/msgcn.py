"""MS-GCN (models/msgcn/msgcn.py): an ST-GCN generator over sliding windows followed by MS-TCN refinement stages over
the window series, on the HIP kernels.

``generator_stage`` is ``stgcn.Model`` (its own kernels, including the window staging of a ``segment.WindowBatch``);
its (N, num_classes, 1) output is read as a series of length L = N (msgcn.py:55-58) and every one of the
``arch['ms-tcn']['stages']`` stages refines it (mstcn.StageFunction, ms_stage.hip).  forward -> (1 + stages, 1,
num_classes, N) fp32, slice 0 the generator's output.  The gradient reaches the generator through the series.

state_dict keys are the reference's on one device (``generator_stage.*``, ``refinement_stages.{i}.*``).  The reference
wraps the generator in ``nn.DataParallel`` when it sees several devices, which prefixes its keys with ``module.``;
there is no such wrapper here, and ``load_state_dict`` accepts either spelling.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .mstcn import SingleStage, refine_and_stack, selector_mode
from .modules import resolve_dtype
from .stgcn import Model as Stgcn


class Model(nn.Module):
    def __init__(self, rank=None, **kwargs):
        super().__init__()
        self.stages = kwargs["stages"]
        self.num_classes = kwargs["num_classes"]
        conf = kwargs["ms-tcn"]
        self.generator_stage = Stgcn(rank=rank, **kwargs)
        self.refinement_stages = nn.ModuleList([
            SingleStage(in_channels=kwargs["num_classes"], out_channels=kwargs["num_classes"],
                        num_filters=conf["filters"][i], num_layers=conf["layers"][i], kernel=conf["kernel"][i],
                        dropout=conf["dropout"][i]) for i in range(conf["stages"])])
        self.refine_mode = selector_mode(kwargs["refine"], "refine")
        self.out_mode = selector_mode(kwargs["output_type"], "output_type")
        self.compute_dtype = torch.float32

    def set_compute_dtype(self, dtype):
        self.compute_dtype = resolve_dtype(dtype)
        self.generator_stage.set_compute_dtype(dtype)
        for stage in self.refinement_stages:
            stage.compute_dtype = self.compute_dtype
        return self

    def load_state_dict(self, state_dict, *args, **kwargs):
        pre = "generator_stage.module."
        state_dict = {("generator_stage." + k[len(pre):] if k.startswith(pre) else k): v
                      for k, v in state_dict.items()}
        return super().load_state_dict(state_dict, *args, **kwargs)

    def forward(self, x):
        y = self.generator_stage(x)                      # (N, C, 1)
        return refine_and_stack(y.squeeze(-1), self.refinement_stages, self.refine_mode, self.out_mode)

    def prepare_benchmark(self, arch_conf):
        return arch_conf
