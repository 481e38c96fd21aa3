"""Generate the MS-TCN / MS-GCN fixtures from the REFERENCE (models/mstcn/mstcn.py, models/msgcn/msgcn.py).

Run only where the reference checkout is available (STGCN_REFERENCE, default /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mstcn.py

The reference's ``Model.forward`` of both models allocates its result on ``x.get_device()``, which is -1 on the CPU,
so it cannot run there.  Its submodules can: this script imports the reference's ``MODELS`` / ``SingleStage``,
composes ``generator_stage``, ``refinement_stages[i]`` and the model's own ``probability`` / ``out`` callables
exactly as ``forward`` does, and stores data only: the config (``arch``), the randomised parameters under the
reference's state_dict names (``sd/*``), inputs, outputs ``y``, a seeded cotangent ``g`` and the gradients of
``sum(y * g)`` for every parameter (``grad/*``); the stage fixture also stores the input gradient ``dx``.

  mstcn_stage : one SingleStage 7 -> 16 -> 7, 6 layers (dilations 1..32), L = 37, at V = 1 (``v1/*``) and V = 3 (``v3/*``)
  mstcn_model : ms-tcn, 3 stages, layers [4, 3, 3], F = 16, in_feat 3, V = 25, L = 37, 7 classes, refine softmax
  msgcn_model : ms-gcn, generator 8->8 (S=1), 8->16 (S=2), kernel 9, receptive field 20, LayerNorm, N = L = 37
                windows of ``capture`` (1, 3, 56, 25), 2 refinement stages, refine softmax
  mstcn_logsoftmax : ms-tcn, 2 stages, layers [2, 2], V = 5, L = 19, refine logsoftmax, output_type softmax
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("STGCN_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))

from models import MODELS  # noqa: E402  (reference)
from models.mstcn.mstcn import SingleStage  # noqa: E402  (reference)
from mstcn_ref import randomise, windows  # noqa: E402

torch.set_num_threads(8)


def backward(module, y, gen, arrays, prefix=""):
    g = torch.randn(y.shape, generator=gen)
    module.zero_grad()
    (y * g).sum().backward()
    arrays[prefix + "y"] = y.detach().numpy()
    arrays[prefix + "g"] = g.numpy()
    for k, p in module.named_parameters():
        arrays[prefix + "grad/" + k.replace("generator_stage.module.", "generator_stage.")] = p.grad.numpy().copy()


def save(name, arrays, sd, arch=None):
    if arch is not None:
        arrays["arch"] = np.frombuffer(json.dumps(arch).encode(), dtype=np.uint8)
    for k, v in sd.items():
        arrays["sd/" + k] = v.detach().numpy()
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {len(arrays)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")


def load_randomised(m, seed):
    gen = torch.Generator().manual_seed(seed)
    sd = randomise(m.state_dict(), gen)
    m.load_state_dict(sd, strict=True)
    m.train()  # dropout 0 everywhere; BatchNorm is not used
    return sd, gen


def make_stage():
    torch.manual_seed(10)
    m = SingleStage(in_channels=7, out_channels=7, num_filters=16, num_layers=6, kernel=3, dropout=0.0)
    sd, gen = load_randomised(m, 11)
    arrays = {}
    for V in (1, 3):
        x = torch.randn(1, 7, 37, V, generator=gen).requires_grad_(True)
        backward(m, m(x), gen, arrays, f"v{V}/")
        arrays[f"v{V}/x"] = x.detach().numpy()
        arrays[f"v{V}/dx"] = x.grad.numpy().copy()
    save("mstcn_stage", arrays, sd)


def mstcn_forward(m, x):
    """mstcn.py:55-65 without the device-indexed result tensor."""
    x = m.generator_stage(x)
    x = F.avg_pool2d(x, (1, x.size(-1)))
    outs = [m.out(x.squeeze(-1))]
    for stage in m.refinement_stages:
        x = stage(m.probability(x))
        outs.append(m.out(x.squeeze(-1)))
    return torch.stack(outs)


def msgcn_forward(m, x):
    """msgcn.py:55-63 without the device-indexed result tensor."""
    N = x.size(0)
    x = m.generator_stage(x)
    x = x.view(1, N, m.num_classes, 1).permute(0, 2, 1, 3)
    outs = [m.out(x[:, :, :, 0])]
    for stage in m.refinement_stages:
        x = stage(m.probability(x))
        outs.append(m.out(x.squeeze(-1)))
    return torch.stack(outs)


def make_mstcn(name, stages, layers, V, L, refine, output_type, seed):
    arch = {"in_feat": 3, "stages": stages, "refine": refine, "output_type": output_type, "num_classes": 7,
            "ms-tcn": {"in_feat": 3, "stages": stages, "layers": layers, "kernel": [3] * stages,
                       "filters": [16] * stages, "dropout": [0.0] * stages}}
    torch.manual_seed(seed)
    m = MODELS["ms-tcn"](**arch)
    sd, gen = load_randomised(m, seed + 1)
    x = torch.randn(1, 3, L, V, generator=gen)
    arrays = {"x": x.numpy()}
    backward(m, mstcn_forward(m, x), gen, arrays)
    save(name, arrays, sd, arch)


def make_msgcn():
    with open(os.path.join(REF, "data", "skeletons", "pku-mmd.json")) as f:
        graph = json.load(f)
    arch = {"strategy": "spatial", "receptive_field": 20, "segment": 37, "in_feat": 3, "stages": 3,
            "refine": "softmax", "output_type": "logits", "normalization": "LayerNorm", "num_classes": 7,
            "graph": graph,
            "st-gcn": {"latency": False, "importance": True, "in_feat": 3, "stages": 1, "layers": 2, "kernel": 9,
                       "in_ch": [8, 8], "out_ch": [8, 16], "stride": [1, 2], "residual": [1, 1], "dropout": [0, 0]},
            "ms-tcn": {"stages": 2, "layers": [3, 3], "kernel": [3, 3], "filters": [16, 16], "dropout": [0, 0]}}
    torch.manual_seed(30)
    m = MODELS["ms-gcn"](**arch)
    sd, gen = load_randomised(m, 31)
    capture = torch.randn(1, 3, 37 + 20 - 1, 25, generator=gen)
    arrays = {"capture": capture.numpy()}
    backward(m, msgcn_forward(m, windows(capture, 20)), gen, arrays)
    save("msgcn_model", arrays, sd, arch)


if __name__ == "__main__":
    make_stage()
    make_mstcn("mstcn_model", 3, [4, 3, 3], 25, 37, "softmax", "logits", 20)
    make_msgcn()
    make_mstcn("mstcn_logsoftmax", 2, [2, 2], 5, 19, "logsoftmax", "softmax", 40)
