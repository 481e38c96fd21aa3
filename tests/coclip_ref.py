"""The co-st-gcn clip (Model.forward_clip) written as whole-clip tensor ops on the CPU, carrying the stream state in
and out: what T frame-by-frame steps of costgcn_ref.costgcn_stream compute, restated without a loop over frames.

The state is, per layer, ``(fifo, fifo_res)`` in costgcn_ref's layout, newest entry first: ``fifo`` (1, C, S*(Kt-1)+1,
V) holds ReLU(LN1(z)) of the last frames (an empty one is ReLU(tcn.0.bias)), ``fifo_res`` (1, C, Kt//2+1, V) the last
residual rows (zeros when empty).

Per layer the clip is: the carried FIFO entries, oldest first, in front of the clip's own ReLU(LN1(z)); one causal
convolution with dilation S over that (tap k meets the frame k*S before, so the kernel is flipped along its taps for
conv2d's correlation); LN2; plus the residual of the frame Kt//2 before, from the carried residual rows where that
frame precedes the clip.

``slip`` plants one mistake for tests/test_coclip_ref_cpu.py to show that its inputs tell right from wrong:
"delay+1" / "delay-1" (residual delay Kt//2 +- 1), "taps" (tap order reversed), "dilation" (dilation 1 in every layer).
"""
import torch
import torch.nn.functional as F

from costgcn_ref import _bf, _ln


def empty_state(sd, arch, graph_A, dtype=torch.float32, round_bf16=False):
    conf = arch["st-gcn"]
    Kt, V = conf["kernel"], graph_A.shape[-1]
    rd = _bf if round_bf16 else (lambda t: t)
    state = []
    for i in range(conf["layers"]):
        C, S = conf["out_ch"][i], conf["stride"][i]
        b = sd[f"gcn_networks.{i}.tcn.0.bias"].detach().to(dtype)
        state.append((rd(torch.relu(b)).reshape(1, C, 1, V).repeat(1, 1, S * (Kt - 1) + 1, 1),
                      torch.zeros(1, C, Kt // 2 + 1, V, dtype=dtype)))
    return state


def costgcn_clip(x, sd, arch, graph_A, state=None, dtype=torch.float32, round_bf16=False, slip=None):
    """x (1, in_feat, T, V), state (None: empty) -> (y (1, num_classes, T), the state after the clip)."""
    conf = arch["st-gcn"]
    if state is None:
        state = empty_state(sd, arch, graph_A, dtype, round_bf16)
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    A = graph_A.to(dtype)
    Kt, P, T = conf["kernel"], A.shape[0], x.shape[2]
    rd = _bf if round_bf16 else (lambda t: t)
    delay = Kt // 2 + {"delay+1": 1, "delay-1": -1}.get(slip, 0)
    h = _ln(x.to(dtype), sd["norm_in.weight"], sd["norm_in.bias"])
    h = F.conv2d(h, sd["fcn_in.weight"], sd["fcn_in.bias"])
    out_state = []
    for i, (fifo, fifo_res) in enumerate(state):
        pre = f"gcn_networks.{i}."
        Cin, C, S = conf["in_ch"][i], conf["out_ch"][i], conf["stride"][i]
        nf, nr = fifo.shape[2], fifo_res.shape[2]
        if not conf["residual"][i]:
            res = torch.zeros(1, C, T, h.shape[3], dtype=dtype)
        elif not (Cin == C and S == 1):
            res = _ln(F.conv2d(h, sd[pre + "residual.0.weight"], sd[pre + "residual.0.bias"]),
                      sd[pre + "residual.1.weight"], sd[pre + "residual.1.bias"])
        else:
            res = h
        Ai = A * sd[f"edge_importance.{i}"] if conf["importance"] else A
        z = F.conv2d(h, rd(sd[pre + "gcn.conv.weight"]), sd[pre + "gcn.conv.bias"])
        z = torch.einsum("nkctv,kvw->nctw", z.view(1, P, C, T, -1), Ai)
        a = rd(torch.relu(_ln(z, sd[pre + "tcn.0.weight"], sd[pre + "tcn.0.bias"])))
        hist = torch.cat((fifo.flip(2), a), dim=2)        # time ascending: nf carried entries, then the clip
        resq = torch.cat((fifo_res.flip(2), res), dim=2)  # nr carried rows, then the clip
        w = rd(sd[pre + "tcn.2.weight"])
        if slip != "taps":
            w = w.flip(2)
        dil = 1 if slip == "dilation" else S
        span = dil * (Kt - 1)
        y = F.conv2d(hist[:, :, nf - span:], w, sd[pre + "tcn.2.bias"], dilation=(dil, 1))
        y = _ln(y, sd[pre + "tcn.3.weight"], sd[pre + "tcn.3.bias"])
        h = torch.relu(y + resq[:, :, nr - delay:nr - delay + T])
        out_state.append((hist.flip(2)[:, :, :nf].contiguous(), resq.flip(2)[:, :, :nr].contiguous()))
    y = F.conv2d(h.mean(dim=3, keepdim=True), sd["fcn_out.weight"], sd["fcn_out.bias"]).squeeze(-1)
    return y, out_state
