"""The canonical image of a stream (stgcn_stream_state_export / _import, stream_state.hip) restated in numpy, and the
adapters that put it under the existing CPU restatements of the two stream batches.

A stream's state is, per layer, ``(t0 [n0][V][C], t1 [n1][V][C], (i0, i1))``: rt-st-gcn's (fifo, acc, (fi, ai)) or
co-st-gcn's (ring, res_ring, (idx0, idx1)), in the batches' own per-stream layout.

* ``canonicalise``: both tensors rotated along the slot axis so that slot k of the result is slot (i + k) % n of the
  original, the indices zeroed.  Nothing is recomputed.
* ``image`` / ``from_image``: the flat fp32 row [E] of a snapshot, layer-major (t0 then t1), and back at rotation 0;
  ``bf16_t0`` rounds t0 to bf16 (nearest even) on the way back, as an import into a bf16 co-st-gcn batch does.
* ``layout``: per layer (C, n0, n1, off0, off1) and E, from the shapes alone.

The rt-st-gcn restatement (rt_streams_clip_ref) keeps explicit indices and addresses fifo[fi], acc[ai], so its states
convert one to one (``rt_to_layers`` / ``rt_from_layers``).  The co-st-gcn restatement (coclip_ref) keeps FIFOs newest
first without a head; ``co_advance`` wraps it in the kernels' ring addressing: slot (idx + j) % n holds the entry of age
j, n frames move idx to (idx - n) % n (clip_ops.h advance_idx, frame_ops.h ring_head) and the new entries land where
that rule says."""
import numpy as np
import torch

from coclip_ref import costgcn_clip


# ------------------------------------------------------------------------------------------------ the image
def canonicalise(layers):
    return [(np.roll(t0, -i0, axis=0), np.roll(t1, -i1, axis=0), (0, 0)) for t0, t1, (i0, i1) in layers]


def layout(V, shapes):
    """shapes: per layer (C, n0, n1) -> ([(C, n0, n1, off0, off1)], E)."""
    at, table = 0, []
    for C, n0, n1 in shapes:
        table.append((C, n0, n1, at, at + n0 * V * C))
        at += (n0 + n1) * V * C
    return table, at


def image(layers):
    """The snapshot row of one stream: fp32 [E]."""
    parts = []
    for t0, t1, _ in canonicalise(layers):
        parts += [np.asarray(t0, dtype=np.float32).ravel(), np.asarray(t1, dtype=np.float32).ravel()]
    return np.concatenate(parts)


def round_bf16(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32 (finite values)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + (((u >> 16) & 1) + 0x7FFF)) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def from_image(row, V, table, bf16_t0=False):
    """A snapshot row back into per-layer state at rotation 0, indices (0, 0)."""
    out = []
    for C, n0, n1, off0, off1 in table:
        t0 = row[off0:off0 + n0 * V * C].reshape(n0, V, C).copy()
        t1 = row[off1:off1 + n1 * V * C].reshape(n1, V, C).copy()
        out.append((round_bf16(t0) if bf16_t0 else t0, t1, (0, 0)))
    return out


# ------------------------------------------------------------------------------------------------ rt-st-gcn adapters
def rt_to_layers(state):
    """rt_streams_clip_ref's per-layer dicts (fifo (C, F, V), acc (C, S, V), fi, ai) -> the batch's layout."""
    return [(s["fifo"].permute(1, 2, 0).contiguous().numpy(), s["acc"].permute(1, 2, 0).contiguous().numpy(),
             (s["fi"], s["ai"])) for s in state]


def rt_from_layers(layers):
    return [{"fifo": torch.from_numpy(np.ascontiguousarray(t0)).permute(2, 0, 1).contiguous(),
             "acc": torch.from_numpy(np.ascontiguousarray(t1)).permute(2, 0, 1).contiguous(), "fi": int(i0),
             "ai": int(i1)} for t0, t1, (i0, i1) in layers]


# ------------------------------------------------------------------------------------------------ co-st-gcn rings
def co_empty(sd, arch, graph_A, dtype=torch.float64):
    """A never-stepped stream in the batch's layout: ReLU(tcn.0.bias) in every ring slot, zero residuals, idx (0, 0)."""
    from coclip_ref import empty_state
    return [(f[0].permute(1, 2, 0).contiguous().numpy(), r[0].permute(1, 2, 0).contiguous().numpy(), (0, 0))
            for f, r in empty_state(sd, arch, graph_A, dtype)]


def co_advance(x, sd, arch, graph_A, layers, dtype=torch.float64):
    """x (1, 3, n, V) through one stream whose state is ``layers`` (ring addressing as the kernels') -> (y (1, K, n),
    the state after)."""
    fifos = []
    for t0, t1, (i0, i1) in layers:  # the entry of age j sits in slot (idx + j) % slots
        f = torch.from_numpy(np.roll(t0, -i0, axis=0).copy()).permute(2, 0, 1).unsqueeze(0)
        r = torch.from_numpy(np.roll(t1, -i1, axis=0).copy()).permute(2, 0, 1).unsqueeze(0)
        fifos.append((f, r))
    n = x.shape[2]
    with torch.no_grad():
        y, after = costgcn_clip(x, sd, arch, graph_A, state=fifos, dtype=dtype)
    out = []
    for (t0, t1, (i0, i1)), (f, r) in zip(layers, after):
        new = []
        for old, fifo, i in ((t0, f, i0), (t1, r, i1)):
            slots = old.shape[0]
            j0 = (i - n) % slots
            ring = np.empty_like(old)
            ages = fifo[0].permute(1, 2, 0).numpy()  # [age][V][C]
            for j in range(slots):
                ring[(j0 + j) % slots] = ages[j]
            new.append((ring, j0))
        out.append((new[0][0], new[1][0], (new[0][1], new[1][1])))
    return y, out
