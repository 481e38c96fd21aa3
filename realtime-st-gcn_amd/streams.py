"""What the per-frame (continual inference) routes share on the host: the stream-batch surface of
``rtstgcn.RtStreamBatch`` and ``costgcn.CoStreamBatch``, the helpers their descriptor builders fill with, and the
snapshot of live streams (``StreamSnapshot``, stgcn_stream_state_export / _import)."""
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
    """The six head pointers and in_feat (F) of a per-frame or clip descriptor: norm_in, fcn_in, fcn_out of
    ``model``."""
    d.F = model.fcn_in.in_channels
    d.ln_w, d.ln_b = keep(LF._flat_ln(model.norm_in.weight)), keep(LF._flat_ln(model.norm_in.bias))
    d.w_in = keep(f32(model.fcn_in.weight).reshape(model.fcn_in.out_channels, -1))
    d.b_in = keep(f32(model.fcn_in.bias))
    d.w_out = keep(f32(model.fcn_out.weight).reshape(model.fcn_out.out_channels, -1))
    d.b_out = keep(f32(model.fcn_out.bias))


# ---------------------------------------------------------------------------------------------- stream snapshots
KINDS = ("rt", "co")  # STGCN_STREAM_STATE_RT, STGCN_STREAM_STATE_CO
LAYOUT_FIELDS = ("C", "n0", "n1", "off0", "off1")


def state_layout(V, shapes):
    """The layout table of a stream's canonical image: per layer (C, n0, n1, off0, off1) from ``shapes`` = per layer
    (C, n0, n1), n0 / n1 the slot counts of the layer's two state tensors (rt: fifo, acc; co: ring, res_ring), each
    stored [slots][V][C], layer-major and dense.  Returns (table, E = elements per stream)."""
    at, table = 0, []
    for C, n0, n1 in shapes:
        C, n0, n1 = int(C), int(n0), int(n1)
        table.append((C, n0, n1, at, at + n0 * V * C))
        at += (n0 + n1) * V * C
    return tuple(table), at


def layout_of_state(state):
    """(V, layout table, E) of per-layer state tensors (t0 [B or none][n0][V][C], t1 [...][n1][V][C], idx)."""
    V = state[0][0].shape[-2]
    table, E = state_layout(V, [(t0.shape[-1], t0.shape[-3], t1.shape[-3]) for t0, t1, _ in state])
    return V, table, E


class StreamSnapshot:
    """The state of ``n`` streams taken out of a stream batch or a single-stream model: ``data`` [n][E] fp32, one
    canonical image per stream (every layer's two state tensors rotated so that both stored indices are 0; fp32
    whatever the batch's dtype), ``kind`` ("rt" | "co"), ``V`` and ``layout``: per layer (C, n0, n1, off0, off1), the
    slot counts of the layer's two tensors and their offsets in a row.

    Weights are not part of a snapshot: it is only meaningful for the parameters it was taken under (a co-st-gcn ring
    caches ReLU(LN1(z)), an rt-st-gcn accumulator sums graph-conv outputs).  Rows can be selected (``snap[i]``,
    ``snap[[i, j]]``), joined (``StreamSnapshot.cat``), moved (``to``) and saved (``state_dict`` / ``from_state_dict``
    through ``torch.save`` / ``torch.load``)."""

    def __init__(self, kind, V, layout, data):
        if kind not in KINDS:
            raise RuntimeError(f"stgcn_amd: StreamSnapshot kind must be one of {KINDS}, got {kind!r}")
        layout = tuple(tuple(int(v) for v in row) for row in layout)
        if not layout or any(len(row) != len(LAYOUT_FIELDS) for row in layout):
            raise RuntimeError("stgcn_amd: StreamSnapshot layout needs one (C, n0, n1, off0, off1) row per layer")
        want, E = state_layout(int(V), [row[:3] for row in layout])
        if want != layout:
            raise RuntimeError("stgcn_amd: StreamSnapshot layout offsets are not the dense layer-major ones")
        if not torch.is_tensor(data) or data.dim() != 2 or data.shape[1] != E or data.dtype != torch.float32:
            raise RuntimeError(f"stgcn_amd: StreamSnapshot data must be fp32 of shape (n, {E}), got "
                               f"{tuple(data.shape) if torch.is_tensor(data) else type(data).__name__}")
        self.kind, self.V, self.layout, self.E, self.data = kind, int(V), layout, E, data.contiguous()

    @property
    def n(self):
        return self.data.shape[0]

    def __len__(self):
        return self.n

    @property
    def device(self):
        return self.data.device

    def to(self, device):
        return StreamSnapshot(self.kind, self.V, self.layout, self.data.to(device))

    def __getitem__(self, rows):
        if isinstance(rows, int):
            rows = [rows]
        rows = torch.as_tensor(list(rows), dtype=torch.long)
        if rows.numel() and (int(rows.min()) < -self.n or int(rows.max()) >= self.n):
            raise IndexError(f"stgcn_amd: StreamSnapshot row out of range for {self.n} streams")
        return StreamSnapshot(self.kind, self.V, self.layout, self.data[rows.to(self.data.device)])

    @staticmethod
    def cat(snaps):
        snaps = list(snaps)
        if not snaps:
            raise RuntimeError("stgcn_amd: StreamSnapshot.cat needs at least one snapshot")
        for s in snaps[1:]:
            why = layout_mismatch((snaps[0].kind, snaps[0].V, snaps[0].layout), (s.kind, s.V, s.layout))
            if why:
                raise RuntimeError(f"stgcn_amd: StreamSnapshot.cat: snapshots differ: {why}")
        return StreamSnapshot(snaps[0].kind, snaps[0].V, snaps[0].layout, torch.cat([s.data for s in snaps], dim=0))

    def state_dict(self):
        """Plain tensors and ints: ``torch.save`` / ``torch.load`` round-trips it."""
        return {"version": 1, "kind": KINDS.index(self.kind), "V": self.V, "E": self.E,
                "layout": torch.tensor(self.layout, dtype=torch.int64), "data": self.data}

    @staticmethod
    def from_state_dict(d):
        if d.get("version") != 1:
            raise RuntimeError(f"stgcn_amd: unknown StreamSnapshot version {d.get('version')!r}")
        if d["kind"] not in (0, 1):
            raise RuntimeError(f"stgcn_amd: unknown StreamSnapshot kind code {d['kind']!r}")
        snap = StreamSnapshot(KINDS[d["kind"]], d["V"], d["layout"].tolist(), d["data"])
        if snap.E != d["E"]:
            raise RuntimeError(f"stgcn_amd: StreamSnapshot state_dict names E = {d['E']}, its layout gives {snap.E}")
        return snap


def layout_mismatch(have, want):
    """None when (kind, V, layout) ``have`` equals ``want``, else a sentence naming the first differing field."""
    if have[0] != want[0]:
        return f"kind {have[0]!r} != {want[0]!r}"
    if len(have[2]) != len(want[2]):
        return f"layer count {len(have[2])} != {len(want[2])}"
    if have[1] != want[1]:
        return f"V {have[1]} != {want[1]}"
    names = {"rt": ("C", "fifo slots (n0)", "accumulator slots (n1 = stride)", "off0", "off1"),
             "co": ("C", "ring slots (n0 = S*(Kt-1)+1)", "residual ring slots (n1 = Kt/2+1)", "off0", "off1")}[have[0]]
    for l, (a, b) in enumerate(zip(have[2], want[2])):
        for name, u, v in zip(names, a, b):
            if u != v:
                return f"layer {l}: {name} {u} != {v}"
    return None


def check_slots(streams, B, what, unique):
    """A Python sequence of slots, checked on the host: every slot in [0, B), and no slot twice when ``unique``."""
    slots = [int(s) for s in streams]
    for s in slots:
        if not 0 <= s < B:
            raise RuntimeError(f"stgcn_amd: {what}: slot {s} outside [0, {B})")
    if unique and len(set(slots)) != len(slots):
        dup = next(s for i, s in enumerate(slots) if s in slots[:i])
        raise RuntimeError(f"stgcn_amd: {what}: slot {dup} is targeted twice")
    return slots


def is_device_slots(t):
    return torch.is_tensor(t) and t.dtype == torch.int32 and t.is_cuda


def state_desc(kind, V, B, dtype, state, layout, E, slots, data):
    """The stgcn_stream_state_desc of per-layer state tensors (t0, t1, idx) with a leading stream axis of B (or none
    when B == 1), ``slots`` int32 [n] and ``data`` fp32 [n][E], both on the state's device."""
    d = K.L.StreamStateDesc()
    d.kind, d.V, d.L, d.B, d.n, d.dtype = KINDS.index(kind), V, len(state), B, slots.shape[0], K.L.dtype_code(dtype)
    d.slots, d.snap, d.E = slots.data_ptr(), data.data_ptr(), E
    for y, (t0, t1, idx), row in zip(d.layers, state, layout):
        y.s0, y.s1, y.idx = t0.data_ptr(), t1.data_ptr(), idx.data_ptr()
        y.C, y.n0, y.n1, y.off0, y.off1 = row
    return d


def export_streams(kind, B, dtype, state, streams, what):
    """``StreamBatch.export_state`` on any per-layer state (a batch's, or a single-stream model's with B = 1)."""
    V, layout, E = layout_of_state(state)
    dev = state[0][0].device
    K.L.require_device(state[0][0])
    with K.device_of(state[0][0]):
        if streams is None:
            slots = torch.arange(B, dtype=torch.int32, device=dev)
        elif is_device_slots(streams):
            slots = streams.contiguous()
        else:
            slots = torch.tensor(check_slots(streams, B, what, False), dtype=torch.int32, device=dev)
        if slots.dim() != 1 or slots.shape[0] < 1:
            raise RuntimeError(f"stgcn_amd: {what}: streams must name at least one slot in one dimension")
        # a device slot tensor may hold entries the kernel skips: their rows stay zero
        data = (torch.zeros if is_device_slots(streams) else torch.empty)((slots.shape[0], E), dtype=torch.float32,
                                                                         device=dev)
        K.stream_state_export(state_desc(kind, V, B, dtype, state, layout, E, slots, data))
    return StreamSnapshot(kind, V, layout, data)


def check_import(kind, B, state, snap, streams, select, what):
    """The host refusals of ``import_state``, before anything touches a device -> (rows of snap or None, slots)."""
    if not isinstance(snap, StreamSnapshot):
        raise RuntimeError(f"stgcn_amd: {what} expects a StreamSnapshot, got {type(snap).__name__}")
    V, layout, _ = layout_of_state(state)
    why = layout_mismatch((snap.kind, snap.V, snap.layout), (kind, V, layout))
    if why:
        raise RuntimeError(f"stgcn_amd: {what}: the snapshot does not fit this model: {why}")
    rows = None
    if select is not None:
        rows = [int(r) for r in ([select] if isinstance(select, int) else select)]
        for r in rows:
            if not 0 <= r < snap.n:
                raise RuntimeError(f"stgcn_amd: {what}: select row {r} outside [0, {snap.n})")
    n = snap.n if rows is None else len(rows)
    if n < 1:
        raise RuntimeError(f"stgcn_amd: {what}: nothing to import (no rows)")
    if streams is None:
        streams = list(range(n))
    if is_device_slots(streams):
        if streams.dim() != 1 or streams.shape[0] != n:
            raise RuntimeError(f"stgcn_amd: {what}: {n} rows for streams of shape {tuple(streams.shape)}")
        return rows, streams.contiguous()
    slots = check_slots(streams, B, what, True)
    if len(slots) != n:
        raise RuntimeError(f"stgcn_amd: {what}: {n} rows for {len(slots)} slots")
    return rows, slots


def import_streams(kind, B, dtype, state, snap, streams, select, what):
    """``StreamBatch.import_state`` on any per-layer state (a batch's, or a single-stream model's with B = 1)."""
    rows, slots = check_import(kind, B, state, snap, streams, select, what)
    K.L.require_device(state[0][0])
    dev = state[0][0].device
    if snap.device != dev:
        raise RuntimeError(f"stgcn_amd: {what}: the snapshot lives on {snap.device}, the state on {dev}: move it with "
                           "snapshot.to(device)")
    with K.device_of(state[0][0]):
        data = snap.data if rows is None else snap.data[torch.tensor(rows, dtype=torch.long, device=dev)]
        if not torch.is_tensor(slots):
            slots = torch.tensor(slots, dtype=torch.int32, device=dev)
        V, layout, E = layout_of_state(state)
        K.stream_state_import(state_desc(kind, V, B, dtype, state, layout, E, slots, data))


class StreamBatch:
    """B independent skeleton streams of one per-frame model.  A subclass keeps ``state`` (per layer, a tuple of
    stream-major device tensors), builds its descriptor in ``_desc()`` -> (descriptor, keep-alive list) and launches
    one tick in ``_launch(d, x, active, out)``.  For ``step_clip`` it gives ``CLIP_MAX_T``, builds a clip descriptor
    in ``_build_clip_desc(cap)`` -> (descriptor, keep-alive list) and launches one call of up to ``cap`` frames in
    ``_launch_clip(d, x, t0, n, active, lengths, out)``."""

    CLIP_MAX_T = None  # the most frames the subclass's clip entry takes per call
    clip_frames = 1024  # step_clip's scratch bound: B * (frames per chunk) stays at or below this
    F = 3  # features per joint of the input frames; __init__ takes the model's in_feat

    @staticmethod
    def _check_B(B):
        if int(B) != B or B < 1:
            raise RuntimeError(f"stgcn_amd: stream_batch needs B >= 1, got {B}")

    def __init__(self, model, B):
        self._check_B(B)
        K.L.require_device(model.A)
        self.model, self.B, self.V, self.F = model, int(B), model.A.shape[-1], model.fcn_in.in_channels
        self._all = torch.ones(self.B, dtype=torch.int32, device=model.A.device)
        self._full = torch.full((self.B,), 2 ** 30, dtype=torch.int32, device=model.A.device)  # lengths=None
        self.state, self._pack = [], None
        self._clips = (None, {})  # (the pack the descriptors point into, {frame capacity: (descriptor, keep, bytes)})

    @property
    def state_bytes(self):
        return sum(t.numel() * t.element_size() for ts in self.state for t in ts)

    # ------------------------------------------------------------------ snapshots: streams out of and into slots
    kind = None  # "rt" | "co": the subclass's state family (stgcn_stream_state_desc.kind)

    def _state_dtype(self):
        """The batch's compute dtype as stgcn_stream_state_desc.dtype takes it."""
        return self.state[0][0].dtype

    def export_state(self, streams=None):
        """The state of the given slots as a ``StreamSnapshot`` on the batch's device, in one launch
        (stgcn_stream_state_export): ``streams`` None (all B, in slot order), a Python list of slots, or an int32 device
        tensor used as given with no host sync (an entry outside [0, B) leaves its row zero).  The batch is not changed.
        The snapshot is only meaningful for the parameters it was taken under."""
        name = f"{type(self).__name__}.export_state"
        if streams is not None and not is_device_slots(streams):
            streams = check_slots(streams, self.B, name, False)
        self._desc()
        return export_streams(self.kind, self.B, self._state_dtype(), self.state, streams, name)

    def import_state(self, snap, streams=None, select=None):
        """Rows ``select`` of ``snap`` (default: all) into slots ``streams`` (default: 0 .. n-1), in one launch
        (stgcn_stream_state_import); other slots are untouched.  ``streams``: a Python list (checked on the host: in
        range, no slot twice) or an int32 device tensor used as given with no host sync (an entry outside [0, B) is
        skipped; a slot named twice ends with undefined content).  A snapshot whose kind or layout table differs from
        this batch's model is refused.  Values are cast to the state's dtype (a bf16 ring rounds to nearest even; fp32
        is exact), and the stream continues bit for bit as the exported one would have under the same parameters."""
        name = f"{type(self).__name__}.import_state"
        check_import(self.kind, self.B, self.state, snap, streams, select, name)
        self._desc()  # a rebuild restarts every stream (co-st-gcn): it has to come first
        import_streams(self.kind, self.B, self._state_dtype(), self.state, snap, streams, select, name)

    def step(self, x, active=None):
        """x (B, in_feat, 1, V) -> (B, num_classes, 1).  ``active``: None (every stream steps), an int32 device tensor
        [B] of codes (0 skip: state untouched, zero output row; 1 step; 2 restart then step) used as given with no
        host sync, or a bool tensor / Python list converted on the host (True = step)."""
        B, V, name, F = self.B, self.V, type(self).__name__, self.F
        if x.dim() != 4 or tuple(x.shape) != (B, F, 1, V):
            raise RuntimeError(f"stgcn_amd: {name}.step expects x of shape {(B, F, 1, V)}, got {tuple(x.shape)}")
        K.L.require_device(x)
        x = K._f32c(x)
        active = self._codes(active, self._all, x.device)
        if tuple(active.shape) != (B,) or not active.is_contiguous():
            raise RuntimeError(f"stgcn_amd: {name}.step expects active of shape ({B},)")
        d, _keep = self._desc()
        out = torch.empty((B, d.K, 1), dtype=torch.float32, device=x.device)
        return self._launch(d, x, active, out)

    @staticmethod
    def _codes(a, default, device):
        """``active`` / ``lengths`` as the kernels read them: ``default`` for None, an int32 device tensor as given (no
        host sync), anything else converted on the host."""
        if a is None:
            return default
        if torch.is_tensor(a) and a.dtype == torch.int32 and a.is_cuda:
            return a
        return torch.as_tensor(a).to(device=device, dtype=torch.int32)

    # ------------------------------------------------------------------ clips: n_b frames of stream b per call
    def _clip_chunk(self):
        """Frames per clip call: B * chunk <= clip_frames, a power of two, at most CLIP_MAX_T."""
        n = min(self.CLIP_MAX_T, max(1, int(self.clip_frames) // self.B))
        return 1 << (n.bit_length() - 1)

    def _clip_calls(self, T):
        """The calls a clip of T frames runs as: [(t0, frames, scratch capacity)], t0 a multiple of the chunk, the
        capacity the next power of two >= frames (at most the chunk)."""
        chunk = self._clip_chunk()
        return [(t0, min(chunk, T - t0), min(chunk, 1 << (min(chunk, T - t0) - 1).bit_length()))
                for t0 in range(0, T, chunk)]

    @property
    def scratch_bytes(self):
        """What was allocated beside the state: ``step_clip``'s scratch for every frame capacity used (a subclass adds
        what its ``step`` needs)."""
        return sum(nbytes for _, _, nbytes in self._clips[1].values())

    def _clip_desc(self, cap):
        """The clip descriptor for calls of up to ``cap`` frames: the state, weight packs and norm parameters of
        ``_desc()``'s descriptor plus stream-major scratch for ``cap`` frames, shared by every layer.  One descriptor
        per capacity is kept with the batch until the packs are rebuilt, so a captured call keeps its buffers."""
        self._desc()
        if self._clips[0] is not self._pack:
            self._clips = (self._pack, {})
        clips = self._clips[1]
        if cap not in clips:
            with K.device_of(self.model.A):
                d, keep = self._build_clip_desc(cap)
            clips[cap] = (d, keep, sum(t.numel() * t.element_size() for t in keep))
        return clips[cap][0]

    def step_clip(self, x, active=None, lengths=None):
        """x (B, in_feat, T, V), T >= 1 -> (B, num_classes, T) fp32: stream b consumes frames 0 .. n_b - 1, n_b =
        clamp(lengths[b], 0, T).  Column t < n_b of stream b is what ``step`` would return for that frame, the frames
        fed one tick at a time from the stream's current state, and its state ends where those n_b ticks would have
        left it; columns t >= n_b, and every column of a skipped stream, are zero.  ``active`` as in ``step`` (code 2:
        ``reset([b])`` first, on the device).  ``lengths``: None (all T frames), an int32 device tensor [B] used as
        given with no host sync, or a host sequence.  Both are read on the device, so a captured call replays with
        other codes and lengths.

        A stream's outputs and state are bit-identical whatever B, its slot, T, the other streams and the chunking into
        consecutive ``step_clip`` calls are.  ``step``, ``step_clip`` and ``reset`` mix freely.  Calls run in chunks of
        min(CLIP_MAX_T, clip_frames // B) frames (a power of two), which bounds the scratch."""
        B, V, name, F = self.B, self.V, type(self).__name__, self.F
        if x.dim() != 4 or x.shape[0] != B or x.shape[1] != F or x.shape[2] < 1 or x.shape[3] != V:
            raise RuntimeError(f"stgcn_amd: {name}.step_clip expects x of shape ({B}, {F}, T >= 1, {V}), got "
                               f"{tuple(x.shape)}")
        for what, a in (("active", active), ("lengths", lengths)):
            if a is not None and (len(a) if not torch.is_tensor(a) else (a.shape[0] if a.dim() == 1 else -1)) != B:
                raise RuntimeError(f"stgcn_amd: {name}.step_clip expects {what} of shape ({B},)")
        if int(self.clip_frames) < 1:
            raise RuntimeError(f"stgcn_amd: {name}.clip_frames must be >= 1, got {self.clip_frames}")
        K.L.require_device(x)
        x = K._f32c(x)
        active = self._codes(active, self._all, x.device).contiguous()
        lengths = self._codes(lengths, self._full, x.device).contiguous()
        with torch.no_grad():
            d0, _ = self._desc()
            out = torch.empty((B, x.shape[2], d0.K), dtype=torch.float32, device=x.device)
            with K.device_of(x):
                for t0, n, cap in self._clip_calls(x.shape[2]):
                    self._launch_clip(self._clip_desc(cap), x, t0, n, active, lengths, out)
        return out.transpose(1, 2)
