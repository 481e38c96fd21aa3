"""CoST-GCN (models/costgcn/costgcn.py): continual per-frame ST-GCN inference on the HIP kernels (co_frame.hip).

``Model(**arch)`` reads ``arch['st-gcn']`` like the reference and keeps the ST-GCN parameter names
(``gcn_networks.i.gcn.conv``, ``.tcn.0``, ``.tcn.2``, ``.tcn.3``, ``.residual.0``, ``.residual.1``,
``edge_importance.i``, buffer ``A``): a checkpoint of ``MODELS['st-gcn']`` loads with ``strict=True`` and back.

forward(x (1, in_feat, 1, V)) -> (1, num_classes, 1), one frame per call.  Every layer keeps the last
``S*(Kt-1)+1`` frames of its graph conv and evaluates the learned Kt-tap temporal conv (dilation S, tap 0 on the
newest frame) over them each frame (costgcn.py:192-211); the residual is delayed by Kt//2 frames.  The reference
holds those FIFOs in CPU tensors; here they are device rings the kernels update, so one captured HIP graph of a
frame replays a stream.  The activation ring caches ReLU(tcn.0(z)) (tcn.0 is a per-frame LayerNorm), so an empty
FIFO is ``ReLU(tcn.0.bias)`` in every slot, not zero: the ring content depends on a parameter, and the rings (and
the weight packs) are rebuilt whenever parameters may have changed — ``load_state_dict``, ``train()`` /
``eval()``, a device or dtype move, or an in-place parameter update seen by the version counters.  A rebuild
restarts the stream.  ``reset_state()`` restarts it explicitly and keeps the buffers (a captured graph stays valid).

Scope: LayerNorm only (the reference's BatchNorm variant takes statistics over whatever the FIFO holds), batch 1,
inference only, 1 <= in_feat <= 16, V <= 32, P <= 3, channels % 4 == 0 and <= 256, odd Kt <= 69, stride 1 or 2.

``forward_clip(x (1, in_feat, T, V)) -> (1, num_classes, T)`` advances the same stream by T frames in one call
(stgcn_co_clip): every layer's temporal conv becomes one GEMM with T*V rows that reads the tap weights once per clip.
Its columns and the state it leaves are those of T ``forward`` calls within rounding, and bit for bit those of any
other chunking of the same frames through ``forward_clip``.

``Model.stream_batch(B)`` serves B independent streams per call (CoStreamBatch, co_streams.hip) with state of its own;
``forward`` stays the call for one stream.  ``CoStreamBatch.step_clip(x (B, in_feat, T, V), active, lengths)`` is the
two together: stream b advances by lengths[b] frames in one call (co_streams_clip.hip), bit for bit as
``forward_clip``, its B = 1 case, would advance it.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import layer_fn as LF
from . import native as K
from .graph import Graph
from .modules import ConvTemporalGraphical, LayerNorm, resolve_dtype
from .streams import Keep, StreamBatch, export_streams, f32, fill_heads, import_streams, res_mode_of


class CoStgcnLayer(nn.Module):
    """Parameter holder of one continual layer (costgcn.py:106-189); the arithmetic runs in Model.forward."""

    def __init__(self, in_channels, out_channels, kernel_size, partitions, num_joints, stride=1, dilation=1, dropout=0,
                 residual=True, normalization="LayerNorm"):
        super().__init__()
        assert len(kernel_size) == 2
        assert kernel_size[0] % 2 == 1
        if normalization != "LayerNorm":
            raise NotImplementedError("stgcn_amd: co-st-gcn supports normalization='LayerNorm' only (the reference's "
                                      "BatchNorm variant takes batch statistics over the FIFO content)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.gamma = kernel_size[0]
        self.stride = stride
        self.fifo_size = stride * (self.gamma - 1) + 1
        self.is_residual = residual
        self.is_residual_conv = residual and not ((in_channels == out_channels) and (stride == 1))
        self.gcn = ConvTemporalGraphical(in_channels, out_channels, kernel_size[1], partitions)
        self.tcn = nn.Sequential(
            LayerNorm([out_channels, 1, num_joints]),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_channels, out_channels, (kernel_size[0], 1), dilation=(stride, 1), padding="valid"),
            LayerNorm([out_channels, 1, num_joints]),
            nn.Dropout(dropout, inplace=True))
        if self.is_residual_conv:
            self.residual = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1),
                                          LayerNorm([out_channels, 1, num_joints]))
        else:
            self.residual = nn.Identity()


def empty_ring_row(l, V):
    """An empty FIFO as the activation ring caches it: ReLU(LN1(0)) = ReLU(tcn.0.bias), rows [V][C] fp32."""
    return torch.relu(l.tcn[0].bias.detach().float()).reshape(l.out_channels, V).t()


def _check_in_feat(model):
    F = model.fcn_in.in_channels
    if not 1 <= F <= K.L.MAX_IN_FEAT or model.norm_in.weight.shape[0] != F:
        raise RuntimeError(f"stgcn_amd: co-st-gcn per-frame input head takes 1 <= in_feat <= {K.L.MAX_IN_FEAT}, got "
                           f"{F}")


def _fill_layer(y, l, A_eff, keep, dt):
    """The fields stgcn_co_layer and stgcn_co_streams_layer both carry, from layer ``l`` (``A_eff`` = A * importance,
    ``dt`` the tap weights' dtype); the caller adds its conv weights (raw or packed) and its buffers."""
    C = l.out_channels
    y.A = keep(A_eff)
    y.bias2d = keep(K.gcn_bias(A_eff, f32(l.gcn.conv.bias), 1, C))
    if l.is_residual_conv:
        y.br = keep(f32(l.residual[0].bias))
        y.lnr_w, y.lnr_b = keep(LF._flat_ln(l.residual[1].weight)), keep(LF._flat_ln(l.residual[1].bias))
    y.ln1_w, y.ln1_b = keep(LF._flat_ln(l.tcn[0].weight)), keep(LF._flat_ln(l.tcn[0].bias))
    y.ln2_w, y.ln2_b = keep(LF._flat_ln(l.tcn[3].weight)), keep(LF._flat_ln(l.tcn[3].bias))
    y.wt, y.bt = keep(K.co_pack_weight(l.tcn[2].weight, dt)), keep(f32(l.tcn[2].bias))


# the layer fields a clip descriptor takes over from the per-frame descriptor it is built beside (CoLayer,
# CoStreamsLayer): shapes, parameters and state
CLIP_LAYER_FIELDS = ("Cin", "Cout", "P", "Kt", "S", "res_mode", "A", "bias2d", "br", "ln1_w", "ln1_b", "ln2_w", "ln2_b",
                     "lnr_w", "lnr_b", "wt", "bt", "ring", "res_ring", "idx")


def _clip_scratch(d, B, layers, dt, dev, workspace):
    """The scratch of clip descriptor ``d`` (CoClipDesc with B = 1, CoStreamsClipDesc; shapes, T and the layers' forced
    splits filled in) for B streams of d.T frames: every layer's split count by ``workspace`` (the descriptor's
    K.co_*clip_workspace, which raises on unsupported shapes), then h0, z, r, two alternating y, hist (``dt``
    elements), resq and the split partials, stream-major, each sized for the largest layer and shared by all.
    Assigns them and returns the keep-alive list."""
    nbytes = []
    for i in range(d.L):
        d.layers[i].splits, nb = workspace(d, i)
        nbytes.append(nb)
    keep = Keep()

    def buf(n, dtype=torch.float32):
        return keep(torch.empty(B * n, dtype=dtype, device=dev))

    cap, V, cmax = d.T, d.V, max(l.out_channels for l in layers)
    d.h0 = buf(cap * V * d.C0)
    z, r, ys = buf(cap * V * cmax), buf(cap * V * cmax), (buf(cap * V * cmax), buf(cap * V * cmax))
    hist = buf(max((l.fifo_size - 1 + cap) * V * l.out_channels for l in layers), dt)
    resq = buf(max((l.gamma // 2 + cap) * V * l.out_channels for l in layers))
    partial = keep(K._workspace(max(nbytes), dev))
    for i in range(d.L):
        y = d.layers[i]
        y.z_buf, y.r_buf, y.hist, y.resq, y.partial, y.y = z, r, hist, resq, partial, ys[i & 1]
    return keep


class Model(nn.Module):
    def __init__(self, rank=None, **kwargs):
        super().__init__()
        conf = kwargs["st-gcn"]
        if kwargs["normalization"] != "LayerNorm":
            raise NotImplementedError("stgcn_amd: co-st-gcn supports normalization='LayerNorm' only (the reference's "
                                      "BatchNorm variant takes batch statistics over the FIFO content)")
        self.graph = Graph(strategy=kwargs["strategy"], **kwargs["graph"])
        A = torch.tensor(self.graph.A, dtype=torch.float32, requires_grad=False).contiguous()
        self.register_buffer("A", A)
        kernel_size = (conf["kernel"], kwargs["graph"]["num_node"])
        dilation = conf.get("dilation", [1] * conf["layers"])
        self.norm_in = LayerNorm([kwargs["in_feat"], 1, A.size(1)])
        self.fcn_in = nn.Conv2d(in_channels=conf["in_feat"], out_channels=conf["in_ch"][0], kernel_size=1)
        self.gcn_networks = nn.ModuleList([
            CoStgcnLayer(in_channels=conf["in_ch"][i], out_channels=conf["out_ch"][i], kernel_size=kernel_size,
                         partitions=A.size(0), num_joints=A.size(1), stride=conf["stride"][i], dilation=dilation[i],
                         residual=not not conf["residual"][i], dropout=conf["dropout"][i],
                         normalization=kwargs["normalization"])
            for i in range(conf["layers"])])
        if conf["importance"]:
            self.edge_importance = nn.ParameterList([nn.Parameter(torch.ones(self.A.size()))
                                                     for _ in self.gcn_networks])
        else:
            self.edge_importance = [1] * len(self.gcn_networks)
        self.fcn_out = nn.Conv2d(conf["out_ch"][-1], out_channels=kwargs["num_classes"], kernel_size=1)
        self.compute_dtype = torch.float32
        self.k_splits = 0  # stgcn_co_layer.splits of every layer: 0 = the library's choice (tests force others)
        self.clip_chunk = 256  # forward_clip runs longer clips in chunks of this many frames (<= STGCN_CO_CLIP_MAX_T)
        self._plan = None  # (key, _Plan): descriptors, weight packs and ring state; never part of the state_dict

    # ------------------------------------------------------------------ whatever may change a parameter drops the plan
    def _drop(self):
        self._plan = None

    def train(self, mode: bool = True):
        self._drop()
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self._drop()
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._drop()
        return super()._apply(fn, *args, **kwargs)

    def set_compute_dtype(self, dtype):
        """fp32, or bf16 tap weights and activation ring (fp32 accumulation; norms, residual ring and layer outputs
        stay fp32).  Restarts the stream."""
        self.compute_dtype = resolve_dtype(dtype)
        self._drop()
        return self

    def set_k_splits(self, n: int):
        """Force the tap kernel's K-split count (0: chosen by the library).  Restarts the stream."""
        self.k_splits = int(n)
        self._drop()
        return self

    # ------------------------------------------------------------------ plan: packs + rings + descriptors
    def _key(self):
        ts = [self.A] + list(self.parameters())
        return (self.compute_dtype, self.k_splits) + tuple((t.data_ptr(), t._version) for t in ts)

    def _ring_init(self, layer, ring, res_ring, idx):
        """An empty FIFO as the ring caches it: ReLU(LN1(0)) = ReLU(tcn.0.bias) in every slot; residuals zero."""
        ring.copy_(empty_ring_row(layer, self.A.shape[-1]).unsqueeze(0).expand_as(ring))
        res_ring.zero_()
        idx.zero_()

    def _build(self):
        dev, dt = self.A.device, self.compute_dtype
        K.L.require_device(self.A)
        V, P = self.A.shape[-1], self.A.shape[0]
        if len(self.gcn_networks) > K.L.RT_MAX_LAYERS:
            raise RuntimeError(f"stgcn_amd: co-st-gcn supports at most {K.L.RT_MAX_LAYERS} layers")
        _check_in_feat(self)
        p = keep = Keep()
        descs, state = [], []
        for i, l in enumerate(self.gcn_networks):
            Cin, C, Kt = l.in_channels, l.out_channels, l.gamma
            A_eff = f32(self.A * self.edge_importance[i])
            d = K.L.CoLayer()
            d.V, d.Cin, d.Cout, d.P, d.Kt, d.S = V, Cin, C, P, Kt, l.stride
            d.res_mode = res_mode_of(l)
            d.dtype, d.splits = K.L.dtype_code(dt), self.k_splits
            d.splits, nbytes = K.co_workspace(d)  # raises on shapes the kernels do not take
            _fill_layer(d, l, A_eff, keep, dt)
            d.w = p(f32(l.gcn.conv.weight).reshape(P * C, Cin))
            if l.is_residual_conv:
                d.wr = p(f32(l.residual[0].weight).reshape(C, Cin))
                d.r_buf = p(torch.empty(V * C, dtype=torch.float32, device=dev))
            ring = torch.empty((l.fifo_size, V, C), dtype=dt, device=dev)
            res_ring = torch.empty((Kt // 2 + 1, V, C), dtype=torch.float32, device=dev)
            idx = torch.empty(2, dtype=torch.int32, device=dev)
            self._ring_init(l, ring, res_ring, idx)
            state.append((l, ring, res_ring, idx))
            d.ring, d.res_ring, d.idx = p(ring), p(res_ring), p(idx)
            d.z_buf = p(torch.empty(V * C, dtype=torch.float32, device=dev))
            d.partial = p(K._workspace(nbytes, dev))
            y = K.cl_empty(1, C, 1, V, torch.float32, dev)
            d.y = p(y)
            if descs:
                d.x = descs[-1].y
            descs.append(d)
        head = (LF._flat_ln(self.norm_in.weight), LF._flat_ln(self.norm_in.bias),
                f32(self.fcn_in.weight).reshape(self.fcn_in.out_channels, -1), f32(self.fcn_in.bias),
                f32(self.fcn_out.weight).reshape(self.fcn_out.out_channels, -1), f32(self.fcn_out.bias))
        return {"descs": descs, "state": state, "keep": keep, "head": head, "y": keep[-1]}

    def _ensure(self):
        key = self._key()
        pk = self._plan
        if pk is None or pk[0] != key:
            with K.device_of(self.A):
                pk = (key, self._build())
            self._plan = pk
            return pk[1], True
        return pk[1], False

    def reset_state(self):
        """Restart the stream: rings back to an empty FIFO (ReLU(tcn.0.bias) / zero), indices cleared.  Buffers are
        kept when the parameters are unchanged, so a captured graph of a frame stays valid."""
        plan, fresh = self._ensure()
        if not fresh:
            for l, ring, res_ring, idx in plan["state"]:
                self._ring_init(l, ring, res_ring, idx)

    @torch.no_grad()
    def _frame(self, x):
        plan, _ = self._ensure()
        g_in, b_in, w_in, bias_in, w_out, bias_out = plan["head"]
        y = K.rt_frame_in(x, g_in, b_in, w_in, bias_in)
        descs = plan["descs"]
        descs[0].x = y.data_ptr()
        for d in descs:
            K.co_layer_frame(d)
        return K.rt_frame_out(plan["y"], w_out, bias_out)

    def forward(self, x):
        if torch.is_grad_enabled() and any(q.requires_grad for q in self.parameters()):
            raise RuntimeError("stgcn_amd: co-st-gcn is inference only (call under torch.no_grad() or freeze the "
                               "parameters)")
        if x.dim() != 4 or x.shape[0] != 1 or x.shape[2] != 1 or x.shape[3] != self.A.shape[-1]:
            raise RuntimeError("stgcn_amd: co-st-gcn processes one frame of batch 1: x (1, in_feat, 1, V), got "
                               f"{tuple(x.shape)}")
        return self._frame(x)

    # ------------------------------------------------------------------ clips: T frames per call on the same rings
    def _clip_desc(self, plan, T):
        """The stgcn_co_clip_desc for a clip of T <= clip_chunk frames: the plan's own rings, tap packs and norm
        affines, plus scratch for the next power of two >= T (capped at clip_chunk), shared by every layer.  One
        descriptor per capacity is kept with the plan, so a captured graph of a clip keeps its buffers."""
        cap = min(int(self.clip_chunk), 1 << (T - 1).bit_length())
        clips = plan.setdefault("clips", {})
        if cap in clips:
            return clips[cap][0]
        dev, dt = self.A.device, self.compute_dtype
        V, P, layers = self.A.shape[-1], self.A.shape[0], self.gcn_networks
        with K.device_of(self.A):
            if "clip_packs" not in plan:  # the graph conv as co_streams.hip packs it, once per plan
                plan["clip_packs"] = [(K.rt_streams_pack_weight(l.gcn.conv.weight, P),
                                       K.rt_streams_pack_weight(l.residual[0].weight, 1) if l.is_residual_conv else None)
                                      for l in layers]
            d = K.L.CoClipDesc()
            d.T, d.V, d.L, d.C0, d.K = cap, V, len(layers), self.fcn_in.out_channels, self.fcn_out.out_channels
            d.dtype = K.L.dtype_code(dt)
            for y, c, (wp, wrp) in zip(d.layers, plan["descs"], plan["clip_packs"]):
                for n in CLIP_LAYER_FIELDS:
                    setattr(y, n, getattr(c, n))
                y.splits, y.wp, y.wrp = self.k_splits, wp.data_ptr(), K.L.ptr(wrp)
            keep = _clip_scratch(d, 1, layers, dt, dev, K.co_clip_workspace)
            fill_heads(d, self, keep)
        clips[cap] = (d, keep)
        return d

    def forward_clip(self, x):
        """x (1, in_feat, T, V), T >= 1 -> (1, num_classes, T) fp32: column t is what ``forward`` would return for
        frame t, the frames fed one at a time from the stream's current state, and the state afterwards is what those
        T calls would have left (stgcn_co_clip: every layer's temporal conv as one GEMM over the clip).
        ``forward``, ``forward_clip`` and ``reset_state()`` mix freely on one stream.  Clips longer than ``clip_chunk``
        frames run in chunks; any chunking, T = 1 pieces included, gives the same bits."""
        if torch.is_grad_enabled() and any(q.requires_grad for q in self.parameters()):
            raise RuntimeError("stgcn_amd: co-st-gcn is inference only (call under torch.no_grad() or freeze the "
                               "parameters)")
        if x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != self.fcn_in.in_channels or x.shape[2] < 1 or \
                x.shape[3] != self.A.shape[-1]:
            raise RuntimeError("stgcn_amd: co-st-gcn processes a clip of batch 1: x (1, in_feat, T >= 1, V), got "
                               f"{tuple(x.shape)}")
        chunk = int(self.clip_chunk)
        if not 1 <= chunk <= K.L.CO_CLIP_MAX_T:
            raise RuntimeError(f"stgcn_amd: co-st-gcn clip_chunk must be in [1, {K.L.CO_CLIP_MAX_T}], got {chunk}")
        K.L.require_device(x)
        with torch.no_grad():
            plan, _ = self._ensure()
            x = K._f32c(x)
            T = x.shape[2]
            out = torch.empty((T, self.fcn_out.out_channels), dtype=torch.float32, device=x.device)
            with K.device_of(x):
                for t0 in range(0, T, chunk):
                    n = min(chunk, T - t0)
                    K.co_clip(self._clip_desc(plan, n), x, t0, n, out)
        return out.t().unsqueeze(0)

    def _own_state(self):
        plan, _ = self._ensure()  # a rebuild restarts the stream: it has to come first
        return [(ring, res_ring, idx) for _, ring, res_ring, idx in plan["state"]]

    def export_state(self):
        """The model's own stream (the one ``forward`` / ``forward_clip`` advance) as a one-row StreamSnapshot: the
        plan's rings and indices have a stream batch's per-stream layout, so stgcn_stream_state_export runs on them with
        B = 1, and the snapshot imports into a slot of ``stream_batch(B)`` (and back).  Only meaningful for the
        parameters it was taken under."""
        return export_streams("co", 1, self.compute_dtype, self._own_state(), None, "Model.export_state")

    def import_state(self, snap):
        """A one-row StreamSnapshot into the model's own stream (cast to the ring's dtype).  The buffers keep their
        addresses, so a captured graph of a frame or a clip stays valid."""
        if getattr(snap, "n", 1) != 1:
            raise RuntimeError(f"stgcn_amd: Model.import_state takes a snapshot of one stream, got {snap.n}")
        import_streams("co", 1, self.compute_dtype, self._own_state(), snap, None, None, "Model.import_state")

    def stream_batch(self, B, splits=0):
        """B independent skeleton streams of this model, advanced together one frame per call (CoStreamBatch,
        stgcn_co_streams).  ``splits`` forces the tap stage's K-split count of every layer (0: the library's choice, a
        function of the layer's shape alone).  The model's own single-stream state and forward are not touched."""
        return CoStreamBatch(self, B, splits)

    def prepare_benchmark(self, arch_conf):
        return arch_conf


class CoStreamBatch(StreamBatch):
    """B independent skeleton streams of one co-st-gcn (Model.stream_batch): every stream has its own activation
    ring, residual ring and indices for every layer, and ``step`` advances the active ones by one frame
    (stgcn_co_streams, co_streams.hip: the tap GEMM runs groups of streams against one read of the weights).  Follows
    the model's ``compute_dtype``: fp32, or bf16 tap weights and rings.  ``step_clip`` advances stream b by up to T
    frames per call on the same state (stgcn_co_streams_clip, co_streams_clip.hip), bit for bit as
    ``Model.forward_clip`` would on the same frames from the same state; its scratch is bounded by ``clip_frames``.

    The state buffers live here (``state``: per layer (ring, res_ring, idx); ``state_bytes`` / ``scratch_bytes``: what
    was allocated) and survive a rebuild of the weight packs and the descriptor, which follows ``Model._key()``.  An
    empty FIFO is ReLU(tcn.0.bias), so a parameter change makes the stream state stale: a rebuild restarts every
    stream, as it does for the single-stream model."""

    kind = "co"

    def __init__(self, model, B, splits=0):
        super().__init__(model, B)
        _check_in_feat(model)
        if len(model.gcn_networks) > K.L.RT_MAX_LAYERS:
            raise RuntimeError(f"stgcn_amd: co-st-gcn supports at most {K.L.RT_MAX_LAYERS} layers")
        self.splits, self._scratch, self._dtype = int(splits), None, None
        self._desc()

    # ------------------------------------------------------------------ buffers: once per (device, compute dtype)
    def _shapes(self):
        """The descriptor with B, the shapes and the split counts filled in; raises on unsupported shapes."""
        m = self.model
        d = K.L.CoStreamsDesc()
        d.B, d.V, d.L, d.C0, d.K = self.B, self.V, len(m.gcn_networks), m.fcn_in.out_channels, m.fcn_out.out_channels
        d.dtype = K.L.dtype_code(m.compute_dtype)
        for i, l in enumerate(m.gcn_networks):
            y = d.layers[i]
            y.Cin, y.Cout, y.P, y.Kt, y.S = l.in_channels, l.out_channels, m.A.shape[0], l.gamma, l.stride
            y.res_mode = res_mode_of(l)
            y.splits = self.splits
        nbytes = []
        for i in range(d.L):
            d.layers[i].splits, nb = K.co_streams_workspace(d, i)
            nbytes.append(nb)
        return d, nbytes

    def _alloc(self, d, nbytes):
        m, B, V = self.model, self.B, self.V
        dev, dt = m.A.device, m.compute_dtype
        self.state, scratch = [], []
        for i, l in enumerate(m.gcn_networks):
            C = l.out_channels
            self.state.append((torch.empty((B, l.fifo_size, V, C), dtype=dt, device=dev),
                               torch.empty((B, l.gamma // 2 + 1, V, C), dtype=torch.float32, device=dev),
                               torch.empty((B, 2), dtype=torch.int32, device=dev)))
            scratch.append(dict(z=torch.empty((B, V, C), device=dev),
                                r=torch.empty((B, V, C), device=dev) if l.is_residual_conv else None,
                                partial=torch.empty(nbytes[i] // 4, device=dev),
                                y=torch.empty((B, V, C), device=dev)))
        self._scratch = dict(layers=scratch, h0=torch.empty((B, V, d.C0), device=dev),
                             order=torch.zeros(B + 1, dtype=torch.int32, device=dev))
        self._dtype = (dt, dev)
        self._step_bytes = sum(t.numel() * t.element_size() for sc in scratch for t in sc.values() if t is not None) \
            + sum(self._scratch[k].numel() * 4 for k in ("h0", "order"))

    @property
    def scratch_bytes(self):
        """What was allocated beside the state: ``step``'s scratch, and ``step_clip``'s for every frame capacity used."""
        return self._step_bytes + super().scratch_bytes

    def _desc(self):
        m = self.model
        key = m._key()
        if self._pack is not None and self._pack[0] == key:
            return self._pack[1]
        with K.device_of(m.A):
            d, nbytes = self._shapes()
            if self._dtype != (m.compute_dtype, m.A.device):
                self._alloc(d, nbytes)
            P, dt = m.A.shape[0], m.compute_dtype
            p = keep = Keep()
            fill_heads(d, m, keep)
            d.h0, d.order = self._scratch["h0"].data_ptr(), self._scratch["order"].data_ptr()
            for i, l in enumerate(m.gcn_networks):
                y, sc = d.layers[i], self._scratch["layers"][i]
                _fill_layer(y, l, f32(m.A * m.edge_importance[i]), keep, dt)
                y.wp = p(K.rt_streams_pack_weight(l.gcn.conv.weight, P))
                if l.is_residual_conv:
                    y.wrp, y.r_buf = p(K.rt_streams_pack_weight(l.residual[0].weight, 1)), sc["r"].data_ptr()
                y.ring, y.res_ring, y.idx = (t.data_ptr() for t in self.state[i])
                y.z_buf, y.partial, y.y = sc["z"].data_ptr(), sc["partial"].data_ptr(), sc["y"].data_ptr()
            self._pack = (key, (d, keep))
            self.reset()  # the rings' empty content depends on tcn.0.bias: every stream restarts
        return self._pack[1]

    def _launch(self, d, x, active, out):
        with K.device_of(x):
            return K.co_streams(d, x, active, out)

    # ------------------------------------------------------------------ clips: stgcn_co_streams_clip
    CLIP_MAX_T = K.L.CO_CLIP_MAX_T
    _launch_clip = staticmethod(K.co_streams_clip)

    def _build_clip_desc(self, cap):
        """The stgcn_co_streams_clip_desc for calls of up to ``cap`` frames: ``_desc()``'s heads, split counts, packs
        and state, plus ``_clip_scratch`` for B streams."""
        d0, _ = self._desc()
        m = self.model
        d = K.L.CoStreamsClipDesc()
        d.B, d.T, d.V, d.L, d.C0, d.K, d.dtype, d.F = self.B, cap, self.V, d0.L, d0.C0, d0.K, d0.dtype, d0.F
        for n in ("ln_w", "ln_b", "w_in", "b_in", "w_out", "b_out"):
            setattr(d, n, getattr(d0, n))
        for y, c in zip(d.layers, d0.layers):
            for n in CLIP_LAYER_FIELDS + ("splits", "wp", "wrp"):
                setattr(y, n, getattr(c, n))
        return d, _clip_scratch(d, self.B, m.gcn_networks, m.compute_dtype, m.A.device, K.co_streams_clip_workspace)

    @torch.no_grad()
    def reset(self, streams=None):
        """Restart the given streams (an iterable of stream indices), or all of them: rings back to an empty FIFO
        (ReLU(tcn.0.bias) / zero), indices cleared.  The buffers are kept, so a captured graph of a tick stays valid."""
        sel = slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.long,
                                                                    device=self.model.A.device)
        for l, (ring, res_ring, idx) in zip(self.model.gcn_networks, self.state):
            ring[sel] = empty_ring_row(l, self.V).to(ring.dtype)
            res_ring[sel] = 0
            idx[sel] = 0
