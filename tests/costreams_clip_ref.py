"""CoStreamBatch.step_clip restated on the CPU as a schedule: a sequence of calls (x, codes, lengths) over B streams,
each mapped onto coclip_ref.costgcn_clip with a state per stream.  Code 0 skips the stream (zero columns, state kept),
code 2 restarts it from the empty state first, any other code advances it; stream b consumes frames 0 .. n_b - 1 of a
call, n_b = clamp(lengths[b], 0, T), and every column t >= n_b is zero.

``slip`` plants one mistake for tests/test_co_streams_clip_cpu.py to show that its inputs tell right from wrong:
"restart" (code 2 treated as code 1), "length" (every non-skipped stream consumes all T frames), "advance" (the right
columns, but the state advanced by all T frames in place of n_b)."""
import torch

from coclip_ref import costgcn_clip, empty_state


def run_schedule(calls, sd, arch, graph_A, states=None, dtype=torch.float32, round_bf16=False, slip=None):
    """calls: [(x (B, 3, T, V), codes ([B] ints or None), lengths ([B] ints or None))]; states: per stream a
    costgcn_clip state, or None for the empty one.  Returns (outs: per call (B, K, T); states after the last call;
    segments: per stream [(frames (1, 3, n, V), columns (1, K, n))] with one entry per run from a restart (or from the
    start) over the frames the stream actually consumed)."""
    B = calls[0][0].shape[0]
    K = sd["fcn_out.weight"].shape[0]
    kw = dict(dtype=dtype, round_bf16=round_bf16)
    states = [s if s is not None else empty_state(sd, arch, graph_A, **kw) for s in (states or [None] * B)]
    runs = [[([], [])] for _ in range(B)]
    outs = []
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
                states[b] = empty_state(sd, arch, graph_A, **kw)
                runs[b].append(([], []))
            if n == 0 and slip != "advance":
                continue
            xb = x[b:b + 1]
            if n:
                y, after = costgcn_clip(xb[:, :, :n], sd, arch, graph_A, state=states[b], **kw)
                out[b, :, :n] = y[0]
                runs[b][-1][0].append(xb[:, :, :n])
                runs[b][-1][1].append(y)
            if slip == "advance":
                after = costgcn_clip(xb, sd, arch, graph_A, state=states[b], **kw)[1]
            states[b] = after
        outs.append(out)
    segments = [[(torch.cat(f, dim=2), torch.cat(y, dim=2)) for f, y in r if f] for r in runs]
    return outs, states, segments
