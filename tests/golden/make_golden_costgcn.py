"""Generate tests/golden/costgcn_k9.npz and costgcn_k69.npz from the REFERENCE CoST-GCN (models/costgcn/costgcn.py).

Run only where the reference checkout is available (STGCN_REFERENCE, default /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_costgcn.py

Imports the reference's own ``MODELS['co-st-gcn']``, gives it randomised norm affines, biases and edge importance,
feeds it a seeded stream frame by frame on the CPU in fp32 and stores the config (``arch``), the parameters under
the reference's state_dict names (``sd/*``), the input stream ``x`` (1, 3, L, 25) and the per-frame outputs ``y``
(1, 7, L).  Data only: nothing of the reference's code is stored.

  costgcn_k9 : Kt = 9,  layers 8->8 (S=1), 8->16 (S=2), 16->16 (S=1), 40 frames
  costgcn_k69: Kt = 69, layers 8->8 (S=1), 8->16 (S=2), 150 frames (> the 137-frame FIFO of the stride-2 layer)
"""
import json
import os
import sys

import numpy as np
import torch

REF = os.environ.get("STGCN_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))

from models import MODELS  # noqa: E402  (reference)
from costgcn_ref import randomise  # noqa: E402

torch.set_num_threads(8)


def make(name, kernel, in_ch, out_ch, stride, frames, seed):
    with open(os.path.join(REF, "data", "skeletons", "pku-mmd.json")) as f:
        graph = json.load(f)
    nl = len(in_ch)
    arch = {"strategy": "spatial", "in_feat": 3, "stages": 1, "kernel": kernel, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": 7, "graph": graph,
            "st-gcn": {"latency": False, "importance": True, "in_feat": 3, "stages": 1, "layers": nl, "kernel": kernel,
                       "in_ch": in_ch, "out_ch": out_ch, "stride": stride, "dilation": [1] * nl,
                       "residual": [1] * nl, "dropout": [0.0] * nl}}
    torch.manual_seed(seed)
    m = MODELS["co-st-gcn"](**arch)
    gen = torch.Generator().manual_seed(seed + 1)
    sd = randomise(m.state_dict(), gen)
    m.load_state_dict(sd, strict=True)
    m.eval()
    x = torch.randn(1, 3, frames, graph["num_node"], generator=gen)
    with torch.no_grad():
        y = torch.cat([m(x[:, :, t:t + 1]) for t in range(frames)], dim=2)
    arrays = {"arch": np.frombuffer(json.dumps(arch).encode(), dtype=np.uint8), "x": x.numpy(), "y": y.numpy()}
    for k, v in sd.items():
        arrays["sd/" + k] = v.detach().numpy().astype(np.float32)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: y {tuple(y.shape)} max|y| {y.abs().max():.3f}  {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    make("costgcn_k9", 9, [8, 8, 16], [8, 16, 16], [1, 2, 1], 40, 100)
    make("costgcn_k69", 69, [8, 8], [8, 16], [1, 2], 150, 200)
