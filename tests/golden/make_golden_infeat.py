"""Generate tests/golden/rt_infeat6.npz and costgcn_infeat6.npz from the REFERENCE models at in_feat 6.

Run only where the reference checkout is available (STGCN_REFERENCE, default /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_infeat.py

The shape is the reference's freezing-of-gait deployment (config/imu_fogit_ABCD: six IMU features per node, the
7-node sensor graph of data/skeletons/imu_fogit_ABCD.json) on a narrow network.  Imports the reference's own
``MODELS``, gives the model randomised norm affines, biases and edge importance, feeds it a seeded stream frame by
frame on the CPU in fp32 and stores the config (``arch``, the graph's num_node / edge / center inside it), the
parameters under the reference's state_dict names (``sd/*``), the input stream ``x`` (1, 6, 40, 7) and the per-frame
outputs.  Data only: nothing of the reference's code is stored.

  rt_infeat6     : rt-st-gcn online (LayerNorm), kernel 9, layers 8->8 (S=1), 8->16 (S=2), 16->16 (S=1), residual
                   [1,1,1], 40 frames, 7 classes; outputs ``y_online`` (1, 7, 40)
  costgcn_infeat6: co-st-gcn, the same graph and widths, Kt 9, 40 frames; outputs ``y`` (1, 7, 40)
"""
import copy
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

IN_FEAT, KERNEL, CLASSES, FRAMES = 6, 9, 7, 40
IN_CH, OUT_CH, STRIDE = [8, 8, 16], [8, 16, 16], [1, 2, 1]


def arch_of(key):
    with open(os.path.join(REF, "data", "skeletons", "imu_fogit_ABCD.json")) as f:
        graph = json.load(f)
    nl = len(IN_CH)
    conf = {"latency": False, "importance": True, "in_feat": IN_FEAT, "stages": 1, "layers": nl, "kernel": KERNEL,
            "in_ch": IN_CH, "out_ch": OUT_CH, "stride": STRIDE, "residual": [1] * nl, "dropout": [0.0] * nl}
    if key == "rt-st-gcn":
        conf["buffer"] = 1
    else:
        conf["dilation"] = [1] * nl
    return {"strategy": "spatial", "in_feat": IN_FEAT, "stages": 1, "kernel": KERNEL, "output_type": "logits",
            "normalization": "LayerNorm", "num_classes": CLASSES, "graph": graph, key: conf}


def save(name, arch, sd, x, outputs):
    arrays = {"arch": np.frombuffer(json.dumps(arch).encode(), dtype=np.uint8), "x": x.numpy()}
    for k, y in outputs.items():
        arrays[k] = y.numpy().astype(np.float32)
    for k, v in sd.items():
        if torch.is_tensor(v):
            arrays["sd/" + k] = v.detach().numpy().astype(np.float32)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    y = next(iter(outputs.values()))
    print(f"{name}: y {tuple(y.shape)} max|y| {y.abs().max():.3f}  {os.path.getsize(path) / 1e3:.1f} KB")


def frames(gen, V):
    # IMU channels are not unit scale: a per-feature scale and offset, so that the input LayerNorm has work to do
    x = torch.randn(1, IN_FEAT, FRAMES, V, generator=gen)
    scale = 0.5 + torch.rand(1, IN_FEAT, 1, 1, generator=gen) * 2
    return x * scale + torch.randn(1, IN_FEAT, 1, 1, generator=gen)


def make_rt(seed):
    arch = arch_of("rt-st-gcn")
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed + 1)
    m = MODELS["rt-st-gcn"](rank="cpu", **copy.deepcopy(arch))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "edge_importance" in name:
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=gen))
            elif name.endswith("weight") and p.dim() == 3:  # LayerNorm([C,1,V]) affines
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=gen))
            elif name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = frames(gen, arch["graph"]["num_node"])
    # online, frame by frame (rtstgcn.py:160-187, 522-525, 528-627): eval_ folds the edge importance, as intended
    m.eval()
    with torch.no_grad():
        m._swap_layers_for_inference()
        for layer in m.st_gcn:
            layer.eval_()
        y = torch.cat([m(x[:, :, t:t + 1]) for t in range(FRAMES)], dim=2)
    save("rt_infeat6", arch, sd, x, {"y_online": y})


def make_co(seed):
    arch = arch_of("st-gcn")
    arch["st-gcn"].pop("buffer", None)
    torch.manual_seed(seed)
    m = MODELS["co-st-gcn"](**copy.deepcopy(arch))
    gen = torch.Generator().manual_seed(seed + 1)
    sd = randomise(m.state_dict(), gen)
    m.load_state_dict(sd, strict=True)
    m.eval()
    x = frames(gen, arch["graph"]["num_node"])
    with torch.no_grad():
        y = torch.cat([m(x[:, :, t:t + 1]) for t in range(FRAMES)], dim=2)
    save("costgcn_infeat6", arch, sd, x, {"y": y})


if __name__ == "__main__":
    make_rt(600)
    make_co(700)
