"""RtStreamBatch.step_clip restated on the CPU as a schedule: a sequence of calls (x, codes, lengths) over B streams
with a state per stream (per layer: fifo, acc and the two indices).  A frame is oracle.stgcn_oracle.rt_model_online's
layer arithmetic, the same functions in the same order; the temporal stage is the recurrence itself,

    a = acc[ai] + z - fifo[fi];  acc[ai] = a;  fifo[fi] = z;  fi = (fi + 1) % fifo_size;  ai = (ai + 1) % S

applied frame after frame.  Code 0 skips the stream (zero columns, state kept), code 2 restarts it from the zero state
first, any other code advances it; stream b consumes frames 0 .. n_b - 1 of a call, n_b = clamp(lengths[b], 0, T), and
every column t >= n_b is zero.

``round_bf16`` rounds the operands where rt_streams_clip.hip rounds them for dtype bf16: gcn.conv's and residual.0's
weights once, and each layer's staged input once (tests/test_rt_streams_bf16_cpu.py's recipe).

``slip`` plants one mistake for tests/test_rt_streams_clip_cpu.py to show that its inputs tell right from wrong:
"restart" (code 2 treated as code 1), "length" (every non-skipped stream consumes all T frames), "advance" (the right
columns, but the indices advanced by T in place of n_b)."""
import copy

import torch
import torch.nn.functional as F

from oracle import stgcn_oracle as O


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def empty_state(arch, V, dtype=torch.float64):
    conf = arch["rt-st-gcn"]
    st = []
    for i in range(conf["layers"]):
        S, C = conf["stride"][i], conf["out_ch"][i]
        fifo = S * (conf["kernel"] - 1) + 1
        st.append({"fifo": torch.zeros(C, fifo, V, dtype=dtype), "acc": torch.zeros(C, S, V, dtype=dtype), "fi": 0,
                   "ai": 0})
    return st


def _push(s, z):
    fi, ai = s["fi"], s["ai"]
    a = s["acc"][:, ai] + z - s["fifo"][:, fi]
    s["acc"][:, ai] = a
    s["fifo"][:, fi] = z
    s["fi"], s["ai"] = (fi + 1) % s["fifo"].shape[1], (ai + 1) % s["acc"].shape[1]
    return a.clone()


def advance(frames, sd, arch, state, round_bf16=False):
    """frames (1, 3, n, V) through one stream from ``state`` (updated in place) -> (1, K, n)."""
    conf, kind = arch["rt-st-gcn"], arch["normalization"]
    V, A = frames.shape[-1], sd["A"]
    P = A.shape[0]
    rnd = _bf16 if round_bf16 else (lambda t: t)
    wq = {k: rnd(v) for k, v in sd.items() if k.endswith("conv.weight") or k.endswith("residual.0.weight")}
    outs = []
    for t in range(frames.shape[2]):
        x = O.layernorm_cv(frames[:, :, t:t + 1], sd["norm_in.weight"], sd["norm_in.bias"])
        x = F.conv2d(x, sd["fcn_in.weight"], sd["fcn_in.bias"])
        for i in range(conf["layers"]):
            pre = "st_gcn.%d." % i
            cin, cout, S = conf["in_ch"][i], conf["out_ch"][i], conf["stride"][i]
            residual = bool(conf["residual"][i])
            xq = rnd(x)
            if not residual:
                res = x * 0.0
            elif cin == cout and S == 1:
                res = x
            else:
                res = O.norm(kind, F.conv2d(xq, wq[pre + "residual.0.weight"]), sd[pre + "residual.1.weight"],
                             sd[pre + "residual.1.bias"])
            Aeff = A * sd[pre + "edge_importance"] if conf["importance"] else A
            z = F.conv2d(xq, wq[pre + "conv.weight"], sd[pre + "conv.bias"]).view(P, cout, V)
            z = torch.einsum("pcv,pvw->cw", z, Aeff)
            z = _push(state[i], z).view(1, cout, 1, V)
            h = torch.relu(O.norm(kind, z, sd[pre + "bn_relu.0.weight"], sd[pre + "bn_relu.0.bias"]))
            x = torch.relu(h + res) if residual else h + res
        x = x.mean(dim=3, keepdim=True)
        outs.append(F.conv2d(x, sd["fcn_out.weight"], sd["fcn_out.bias"]).squeeze(-1))
    return torch.cat(outs, dim=2)


def run_schedule(calls, sd, arch, states=None, dtype=torch.float64, round_bf16=False, slip=None):
    """calls: [(x (B, 3, T, V), codes ([B] ints or None), lengths ([B] ints or None))]; states: per stream a state as
    empty_state returns it, or None for the zero one.  Returns (outs: per call (B, K, T); states after the last call;
    segments: per stream [(frames (1, 3, n, V), columns (1, K, n))] with one entry per run from a restart (or from the
    start) over the frames the stream actually consumed)."""
    B, V = calls[0][0].shape[0], calls[0][0].shape[3]
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    K = sd["fcn_out.weight"].shape[0]
    states = [copy.deepcopy(s) if s is not None else empty_state(arch, V, dtype) for s in (states or [None] * B)]
    runs = [[([], [])] for _ in range(B)]
    outs = []
    with torch.no_grad():
        for x, codes, lengths in calls:
            T = x.shape[2]
            out = torch.zeros(B, K, T, dtype=dtype)
            for b in range(B):
                code = 1 if codes is None else int(codes[b])
                n = T if lengths is None else max(0, min(int(lengths[b]), T))
                if code == 0:
                    continue
                if slip == "length":
                    n = T
                if code == 2 and slip != "restart":
                    states[b] = empty_state(arch, V, dtype)
                    runs[b].append(([], []))
                if n:
                    xb = x[b:b + 1, :, :n].to(dtype)
                    y = advance(xb, sd, arch, states[b], round_bf16)
                    out[b, :, :n] = y[0]
                    runs[b][-1][0].append(xb)
                    runs[b][-1][1].append(y)
                if slip == "advance":
                    for s in states[b]:
                        s["fi"] = (s["fi"] + T - n) % s["fifo"].shape[1]
                        s["ai"] = (s["ai"] + T - n) % s["acc"].shape[1]
            outs.append(out)
    segments = [[(torch.cat(f, dim=2), torch.cat(y, dim=2)) for f, y in r if f] for r in runs]
    return outs, states, segments


def state_tensors(state):
    """A stream's state in the batch's layout: per layer (fifo [fifo][V][C], acc [S][V][C], idx [2])."""
    return [(s["fifo"].permute(1, 2, 0).contiguous(), s["acc"].permute(1, 2, 0).contiguous(),
             torch.tensor([s["fi"], s["ai"]], dtype=torch.int32)) for s in state]
