"""Forward/backward of one ST-GCN layer as a sequence of HIP kernel launches.

StgcnLayer.forward (models/stgcn/stgcn.py:181-193) is

    res = identity(x) | norm_r(conv1x1_s(x)) | 0
    g   = ConvTemporalGraphical(x, A)                 tgcn.py:58-79   (1x1 conv -> @A -> sum_P)
    u   = conv_Kt_s(relu(norm1(g)))                    stgcn.py:151-159
    y   = relu(norm2(u) + res)                         stgcn.py:160,193

with norm = BatchNorm2d(track_running_stats=False) or the custom LayerNorm([C,1,V]).

Host path.  A module builds one LayerCfg (RtLayerCfg for the rt-st-gcn offline layer) by keyword per call and
passes it to the Function as its one non-tensor argument; forward keeps its tensors with _save_named (all through
ctx.save_for_backward, None allowed) and backward reads them back by name with _saved.

Kernel schedule (forward, BatchNorm), graph conv by route:
  gathered (batch-shared sparse A with bound support lists; the model's layers):
    gconv_weights(A, Wg, b)       -> per-joint effective weights + bias2d[V][C]   (or the model's PrepPlan packs)
    gconv(x, Weff, bias2d)        -> g   + BN1 partial stats (epilogue); no XA in HBM
  A-first (per-sample 4-D A, dense support, bare ConvTemporalGraphical, rt-st-gcn offline): gcn_forward
    amix_fwd(x, A)                -> XA                     (A applied first, exact)
    gcn_bias(A, b)                -> bias2d[V][C]
    conv_rows(XA, Wg, bias2d)     -> g   + BN1 partial stats (epilogue)
  then
  bn_finalize                   -> scale1/shift1
  conv_rows(g, Wt, pro=BN1+ReLU)-> u   + BN2 partial stats (prologue applies norm1+ReLU on load)
  [conv_rows(x, Wr, s) -> r + stats ; finalize]
  bn_finalize, bn_apply(u, +res, ReLU) -> y
LayerNorm: ln_stats / ln_apply in place of the BN pairs (h = relu(LN1(g)) materialised), or for a bf16 64 -> 64
stride-1 layer the whole forward as one kernel (fused_layer_forward).
Backward mirrors it: the fused BN reduce/apply pair (bn_bwd_fused) or _norm_backward, the transposed convs
(conv_rows trans=1 / tconv_frame), the weight-gradient kernels (conv_wgrad_w), and for the graph part gconv
trans + gconv_wgrad + finish (gathered) or gcn_backward (A-first: amix_trans / amix_dA / conv_wgrad and the bias
pushed through A by _bias_through_A).  gcn_forward / gcn_backward are the only A-first implementation.
Everything is a HIP kernel of libstgcn_amd.so; the only torch work here is allocation, weight re-packing (tiny
tensors) and, for a per-sample A only, the (P x V)-sized einsums of the A/bias gradients.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import NamedTuple

import torch

from . import native as K
from .routing import ROUTING
from .syncbn import active_sync

BN, LN = "BatchNorm", "LayerNorm"


class LayerCfg(NamedTuple):
    """StgcnLayerFunction's non-tensor argument, built by keyword once per layer call."""
    kt: int
    stride: int
    residual: bool
    norm: str
    dtype: torch.dtype
    sup: object = None       # native.GraphSupport of the bound graph (None: per-sample A, the A-first route)
    dense_dA: bool = False   # caller-owned A: its gradient is wanted off the support too
    infer: bool = False      # no autograd graph will be built: the one-kernel forward may run
    cache: dict = None       # the layer's pack / statistics-arena cache
    packs: object = None     # LayerPacks of the model's PrepPlan launch
    sync: object = None      # syncbn.BnSync of a SyncBatchNorm run


class RtLayerCfg(NamedTuple):
    """RtOfflineLayerFunction's non-tensor argument."""
    Kt: int
    S: int
    residual: bool
    norm: str
    dtype: torch.dtype
    sync: object = None


def _save_named(ctx, **tensors):
    """save_for_backward under names: every value (a tensor or None) goes through ctx.save_for_backward, so
    version-counter checks and lifetime are autograd's; only the names are kept on ctx."""
    ctx.saved_names = tuple(tensors)
    ctx.save_for_backward(*tensors.values())


def _saved(ctx):
    """What _save_named kept, attribute-addressable."""
    return SimpleNamespace(**dict(zip(ctx.saved_names, ctx.saved_tensors)))


def _f32(p):
    """Detached fp32 contiguous form of a parameter or adjacency (what the kernels read)."""
    return p.detach().float().contiguous()


def _flat_ln(p):
    """LayerNorm([C,1,V]) parameter (C,1,V) -> flat fp32 [C*V] indexed c*V+v (kernel convention)."""
    return p.detach().reshape(-1).float().contiguous()


def _wg_rows(wg, P, Cout, Cin):
    """Graph-conv weight (P*Cout, Cin, 1, 1) as the A-first GEMM's rows [1][Cout][P*Cin]."""
    return wg.detach().float().view(P, Cout, Cin).permute(1, 0, 2).reshape(1, Cout, P * Cin)


def _wg_rows_T(wg, P, Cout, Cin):
    """The transposed form [1][P*Cin][Cout] (data gradient)."""
    return wg.detach().float().view(P, Cout, Cin).permute(0, 2, 1).reshape(1, P * Cin, Cout)


def gcn_forward(x, A32, wg, bg, dtype, stats=None):
    """ConvTemporalGraphical forward on rows: XA = A-mix(x); g = XA @ Wg' + bias2d (+ BatchNorm partial statistics
    into ``stats`` from the same epilogue).  Returns (XA, g, cp)."""
    N, Cin, T, V = x.shape
    P = A32.shape[-3]
    Cout = wg.shape[0] // P
    XA = K.amix_fwd(x, A32)
    wgp, cp, kp = K.pack_weight(_wg_rows(wg, P, Cout, Cin), dtype)
    bias2d = K.gcn_bias(A32, _f32(bg), N, Cout)
    g = K.conv_rows(XA, wgp, P * Cin, Cout, cp, kp, T, T, bias=bias2d, bias_mode=3 if A32.dim() == 4 else 2,
                    stats=stats)
    return XA, g, cp


def gcn_stats_buffer(M, Cout, dev):
    cp = -(-Cout // K.col_tile(Cout)) * K.col_tile(Cout)
    return torch.zeros((K.row_blocks(M, Cout), cp, 4), dtype=torch.float32, device=dev), cp


def _gcn_dgrad_rows(dg, wg, P, Cin, Cout, T, dtype):
    """DW[(n,t,w)][p*Cin+ci] = sum_c dg[(n,t,w)][c] Wg[p*Cout+c][ci]: dg through the transposed 1x1 weights."""
    wgTp, cq, kq = K.pack_weight(_wg_rows_T(wg, P, Cout, Cin), dtype)
    return K.conv_rows(dg, wgTp, Cout, P * Cin, cq, kq, T, T)


def gcn_backward(x, A32, XA, wg, bg, dg, dx, accumulate, dtype, z_S=None):
    """Backward of gcn_forward given dg: dx (+)= A^T-mix(dg @ Wg), returns (dA fp32, dWg, dbg).  ``z_S``: a zeroed
    buffer for the per-joint row sums of dg (_bias_through_A), else allocated."""
    N, Cin, T, V = x.shape
    P = A32.shape[-3]
    Cout = wg.shape[0] // P
    DW = _gcn_dgrad_rows(dg, wg, P, Cin, Cout, T, dtype)
    K.amix_trans(DW, A32, Cin, dx, accumulate=accumulate)
    dA = K.amix_dA(x, DW, A32)
    dwg = K.conv_wgrad(XA, dg, P * Cin, Cout, T, T, Kt=1)                # [1][Cout][P*Cin]
    dwg = dwg.view(Cout, P, Cin).permute(1, 0, 2).reshape(P * Cout, Cin, 1, 1)
    dA, dbg = _bias_through_A(dA, A32, bg, dg, z_S=z_S)
    return dA, dwg, dbg


def _bias_through_A(dA, A32, bg, dg, S=None, z_S=None):
    """The conv bias pushed through A: dA[p][v][w] += sum_c b_p[c] S[w][c] (independent of v), S = per-joint row
    sums of dg (``S``: already produced by the joint-grouped weight-gradient kernel; else summed here, into the
    zeroed ``z_S`` when given).  Returns (dA, dbg)."""
    N, Cout, T, V = dg.shape
    M = N * T * V
    if A32.dim() == 4:
        Sn = K.rowgroup_sum(dg, M, Cout, V, per_sample=True, out=z_S)   # [N][V(w)][Cout]
        dA = dA + torch.einsum("pc,nwc->npw", bg.detach().float().view(-1, Cout), Sn).unsqueeze(2)
        colsum = A32.sum(dim=2)                                         # [N][P][W]
        return dA, torch.einsum("npw,nwc->pc", colsum, Sn).reshape(-1)
    if S is None:
        S = K.rowgroup_sum(dg, M, Cout, V, out=z_S)                     # [V(w)][Cout]
    if not dA.is_contiguous():
        dA = dA.contiguous()
    return dA, K.gcn_bias_bwd(A32, _f32(bg), S, dA, Cout)


def _packs(cache, wg, wt, P, Cin, Cout, dtype):
    """Packed graph-conv (the fused layer's W' image) and temporal-conv (fragment image) weights, reused while the
    parameters are unchanged (keyed by storage and in-place version): inference packs once."""
    key = (wg.data_ptr(), wg._version, wt.data_ptr(), wt._version, dtype)
    if cache is not None and cache.get("key") == key:
        return cache["val"]
    wimg, cpg, kwg = K.pack_gcn_weight(_wg_rows(wg, P, Cout, Cin)[0], dtype)
    wt3 = wt.detach().float().squeeze(-1).permute(2, 0, 1)  # [Kt][Cout][Cin]
    wtp, _, _ = K.pack_weight(wt3, dtype, stride=1)
    val = (wimg, cpg, kwg, wtp)
    if cache is not None:
        cache["key"], cache["val"] = key, val
    return val


class LayerPacks:
    """Packed operands of one StgcnLayer's training step, filled by the model's PrepPlan launch
    (native.PrepPlan): graph-conv effective weights + bias through A (forward), their data-gradient form,
    temporal conv (forward / data gradient) and residual 1x1 conv (forward / data gradient) packs, each as
    the (tensor, Cout_pad, Cin_pad) triple pack_weight returns (gw: (weights, bias2d))."""
    __slots__ = ("gw", "gwT", "wt", "wtT", "wr", "wrT")

    def __init__(self):
        self.gw = self.gwT = self.wt = self.wtT = self.wr = self.wrT = None


def plan_layer_packs(plan, layer, A, M, dtype):
    """Record in ``plan`` every pack StgcnLayerFunction builds per call for ``layer`` fed ``A * M`` (the
    model's graph and the layer's edge importance, M None without importance); None when the layer takes a
    route that packs differently (per-sample or dense A: the A-first graph conv)."""
    sup = layer._gsup
    P, V = A.shape[0], A.shape[-1]
    conv = layer.tcn[2]
    Cout, Cin = conv.out_channels, layer.gcn.conv.in_channels
    kt, stride = layer.kernel_size[0], layer.stride
    if sup is None or A.dim() != 3 or sup.dense(P):
        return None
    pk = LayerPacks()
    wg2 = layer.gcn.conv.weight.detach().reshape(P * Cout, Cin)
    pk.gw = K.gconv_weights(A, wg2, sup, Cout, Cin, False, dtype, bias=layer.gcn.conv.bias.detach(), plan=plan, M=M)
    pk.gwT = K.gconv_weights(A, wg2, sup, Cout, Cin, True, dtype, plan=plan, M=M)
    wt = conv.weight.detach().squeeze(-1)
    pk.wt = K.pack_weight(wt.permute(2, 0, 1), dtype, stride=stride, plan=plan)
    pk.wtT = K.pack_weight(wt.permute(2, 1, 0), dtype, stride=stride, trans=True, plan=plan)
    if layer.is_residual_conv:
        wr = layer.residual[0].weight.detach().view(Cout, Cin)
        pk.wr = K.pack_weight(wr.unsqueeze(0), dtype, plan=plan)
        pk.wrT = K.pack_weight(wr.t().unsqueeze(0), dtype, plan=plan)
    return pk


def fused_layer_forward(x, A32, wg, bg, n1w, n1b, wt, bt, n2w, n2b, residual, dtype, tag=None, cache=None,
                        train=False, packs=None):
    """StgcnLayer.forward (stgcn.py:181-193) of a LayerNorm layer through layer_fused.hip: both norms are per frame,
    so the whole layer is one kernel (g and h stay on chip).  ``train``: the kernel also writes what the unfused
    backward reads and this returns (y, g, u, ls1, ls2, h).  x: channels-last bf16 (N, 64, T, V).  ``packs``: the
    step's LayerPacks (training): the temporal-conv fragment image and the bias through A come from the model's one
    prep launch instead of per-layer launches."""
    N, Cin, T, V = x.shape
    P = A32.shape[0]
    Cout = wt.shape[0]
    if packs is not None and packs.wt is not None and packs.gw is not None:
        bias2d = packs.gw[1]
        wimg, cpg, kwg = K.pack_gcn_weight(_wg_rows(wg, P, Cout, Cin)[0], dtype)
        wtp = packs.wt[0]
    else:
        bias2d = K.gcn_bias(A32, _f32(bg), N, Cout)
        wimg, cpg, kwg, wtp = _packs(cache, wg, wt, P, Cin, Cout, dtype)
    # the LayerNorm([64,1,V]) parameters as per-joint [V][64] rows, re-laid-out when one changed (every training
    # step): one stacking launch for the four (the kernel reads 16-B channel runs per joint)
    lkey = tuple((t.data_ptr(), t._version) for t in (n1w, n1b, n2w, n2b))
    if cache is not None and cache.get("ln_key") == lkey:
        ln = cache["ln_val"]
    else:
        ln = tuple(torch.stack([p.detach().float().reshape(Cout, V).t() for p in (n1w, n1b, n2w, n2b)]).unbind(0))
        if cache is not None:
            cache["ln_key"], cache["ln_val"] = lkey, ln
    return K.layer_fused(x, A32, wimg, bias2d, wtp, _f32(bt), ln, tag=tag, residual=residual, train=train)


def _stats_arena(cache, dev, dtype, shapes, route):
    """The BatchNorm partial-statistics buffers of a layer's forward.  The producing GEMM epilogues overwrite
    the same (row block, channel) entries on every call of one route and shape, and the entries they never
    write (rows past the kernel's row-block count, padded channels) must read as zero for bn_finalize — so a
    buffer kept per (device, dtype, shapes, route) in the layer's cache is zero-filled ONCE, not per forward.
    Streams: consumed by the layer's own bn_finalize right after, in stream order; the layer's next forward
    writes it again only after that.  Without a cache (bare calls): a fresh zeroed arena.  ``cache`` is the
    layer's sub-dict of this device (StgcnLayerFunction.forward), so eviction never touches another device's."""
    if cache is None:
        return K.zeros_arena(dev, *shapes)
    key = ("bn_stats", str(dev), dtype, tuple(map(tuple, shapes)), route)
    st = cache.get(key)
    if st is None:
        old = [k for k in list(cache) if isinstance(k, tuple) and k[:1] == ("bn_stats",)]
        for k in old[:-6]:  # keep a few shapes and routes (config 4 alternates 64- and 65-window units)
            del cache[k]
        st = cache[key] = K.zeros_arena(dev, *shapes)
    return st


@K.on_tensor_device
class StgcnLayerFunction(torch.autograd.Function):
    """Autograd node for the whole StgcnLayer (BN or LN variant)."""

    @staticmethod
    def forward(ctx, x, A, wg, bg, n1w, n1b, wt, bt, n2w, n2b, wr, br, nrw, nrb, cfg):
        kt, stride, residual, norm, dtype, sup, packs = (cfg.kt, cfg.stride, cfg.residual, cfg.norm, cfg.dtype,
                                                         cfg.sup, cfg.packs)
        dev = x.device
        x = K.to_rows(x, dtype)
        N, Cin, T, V = x.shape
        P = A.shape[-3]
        Cout = wt.shape[0]
        pad = (kt - 1) // 2
        T_out = (T + 2 * pad - kt) // stride + 1
        M1, M2 = N * T * V, N * T_out * V
        A32 = _f32(A)
        res_conv = residual and not (Cin == Cout and stride == 1)
        # the layer's cache, one sub-dict per device: DataParallel replicas share the module's dict (shallow
        # __dict__ copy) and run in one thread per device, so each thread only ever touches its own sub-dict
        # (dict.setdefault is atomic under the GIL)
        cache = cfg.cache.setdefault(("dev", str(dev)), {}) if cfg.cache is not None else None
        # SyncBatchNorm (syncbn.py): the statistics of every rank, else this rank's (the reference's DataParallel)
        bn_finalize = cfg.sync.finalize if cfg.sync is not None else K.bn_finalize

        # ---- graph convolution: g = sum_p A_p-mix(x) W_p + bias2d
        gather = sup is not None and A32.dim() == 3 and not sup.dense(P)
        if (gather and cfg.infer and ROUTING.fused_inference and norm == LN
                and K.layer_fused_ok(sup, P, Cin, Cout, V, kt, stride, dtype)):
            # inference of a LayerNorm 64 -> 64 stride-1 layer: the one-kernel layer (g never leaves the chip;
            # nothing saved for backward): 0.12 vs 0.15-0.21 ms unfused
            return fused_layer_forward(x, A32, wg, bg, n1w, n1b, wt, bt, n2w, n2b, residual, dtype, cache=cache)
        if (gather and norm == LN and ROUTING.fused_ln_train and not cfg.infer
                and K.layer_fused_ok(sup, P, Cin, Cout, V, kt, stride, dtype)):
            # training forward of a LayerNorm 64 -> 64 stride-1 layer: the one-kernel layer (g and h on chip for
            # the temporal conv) also writes g, u and both LN statistics — exactly what the unfused forward
            # saves — so the backward below is unchanged (ln/ configs)
            y, g, u, ls1, ls2, h = fused_layer_forward(x, A32, wg, bg, n1w, n1b, wt, bt, n2w, n2b, residual, dtype,
                                                       cache=cache, train=True, packs=packs)
            ctx.cfg = cfg
            ctx.sup = sup
            ctx.dims = (N, Cin, Cout, T, T_out, V, P, pad, False)
            _save_named(ctx, x=x, A32=A32, XA=None, g=g, u=u, y=y, wg=wg, bg=bg, wt=wt, n1w=n1w, n1b=n1b, n2w=n2w,
                        n2b=n2b, ls1=ls1, ls2=ls2, h=h)
            ctx.in_dtype = A.dtype
            return y
        st1 = st2 = str_ = None
        if norm == BN:  # all BatchNorm partial-statistics buffers of the layer from one zero fill
            cpo = -(-Cout // K.col_tile(Cout)) * K.col_tile(Cout)
            rb1 = K.gconv_row_blocks(N * T, V) if gather else K.row_blocks(M1, Cout)
            rb2 = K.row_blocks(M2, Cout)
            st_shapes = [(rb1, cpo, 4), (rb2, cpo, 4)] + ([(K.row_blocks(M2, Cout), cpo, 4)] if res_conv else [])
            st_all = _stats_arena(cache, dev, x.dtype, st_shapes, gather)
            st1, st2 = st_all[0], st_all[1]
            str_ = st_all[2] if res_conv else None
        # ---- residual branch: independent of the graph conv -> temporal conv chain until the output norm
        r = None
        if res_conv:
            wrp, cpr, kpr = packs.wr if packs is not None else K.pack_weight(_f32(wr).view(1, Cout, Cin), dtype)
            r = K.conv_rows(x, wrp, Cin, Cout, cpr, kpr, T, T_out, Kt=1, stride=stride, pad=0, bias=_f32(br),
                            stats=str_)
            if norm == BN:
                strr, scr, shr = bn_finalize(str_, str_.shape[0], cpr, Cout, _f32(nrw), _f32(nrb))
            else:
                strr = K.ln_stats(r, N * T_out, V, Cout)

        if gather:  # joint-gathered GEMM over per-joint effective weights (gconv.hip), no XA in HBM
            if packs is not None and packs.gw is not None:
                wgp, bias2d = packs.gw
            else:
                wgp, bias2d = K.gconv_weights(A32, _f32(wg).reshape(P * Cout, Cin), sup, Cout, Cin, False, dtype,
                                              bias=_f32(bg))
            cpg = wgp.shape[2]
            if norm == BN:
                assert cpg == cpo
            g = K.gconv(x, wgp, sup, Cin, Cout, bias=bias2d, stats=st1)
            XA = None
        else:  # per-sample or dense A: A-mix first, BN1 partials from the same GEMM epilogue
            XA, g, cpg = gcn_forward(x, A32, wg, bg, dtype, stats=st1)
        if norm == BN:
            mr1, sc1, sh1 = bn_finalize(st1, st1.shape[0], cpg, Cout, _f32(n1w), _f32(n1b))
            pro1 = dict(pro=1, pro_a=sc1, pro_b=sh1)
        else:
            # LayerNorm: h = relu(LN1(g)) is materialised (one HBM-bound pass, ln.hip) and the temporal conv runs
            # without a prologue on the persistent kernels; a per-frame-statistics, per-(c,v)-affine prologue
            # in the conv tiles measured 304 us vs ~85 us for this pass + conv_wide at 64 -> 64.  h is kept for
            # the weight gradient.
            ls1 = K.ln_stats(g, N * T, V, Cout)
            h = K.ln_apply(g, ls1, _flat_ln(n1w), _flat_ln(n1b), M1, V, Cout, relu=True)
            pro1 = {}

        # ---- temporal conv on relu(norm1(g)) (norm applied in the prologue)
        wtp, cpt, kpt = packs.wt if packs is not None else \
            K.pack_weight(wt.detach().float().squeeze(-1).permute(2, 0, 1), dtype, stride=stride)  # [Kt][Cout][Cin]
        u = K.conv_rows(g if norm == BN else h, wtp, Cout, Cout, cpt, kpt, T, T_out, Kt=kt, stride=stride,
                        pad=pad, bias=_f32(bt), stats=st2, tag=f"tcn_fwd_c{Cout}" if stride == 1 else None, **pro1)

        # ---- y = relu(norm2(u) + res)
        if norm == BN:
            mr2, sc2, sh2 = bn_finalize(st2, st2.shape[0], cpt, Cout, _f32(n2w), _f32(n2b))
            # the output's sign bits for the backward's ReLU mask (the fused BN backward reads them instead of y:
            # 1/16 of the bytes in both of its passes)
            ybits = torch.empty((M2, Cout // 8), dtype=torch.uint8, device=dev) \
                if (ROUTING.bn_mask_bits and dtype == torch.bfloat16 and K.bn_fused_ok(Cout, dtype) and Cout % 8 == 0) \
                else None
            if res_conv:
                y = K.bn_apply(u, sc2, sh2, M2, Cout, res_mode=2, r=r, rsc=scr, rsh=shr, bits=ybits)
            else:
                y = K.bn_apply(u, sc2, sh2, M2, Cout, res_mode=1 if residual else 0, r=x if residual else None,
                               bits=ybits)
        else:
            ls2 = K.ln_stats(u, N * T_out, V, Cout)
            g2, b2 = _flat_ln(n2w), _flat_ln(n2b)
            if res_conv:
                y = K.ln_apply(u, ls2, g2, b2, M2, V, Cout, res_mode=2, r=r, rst=strr, rg=_flat_ln(nrw),
                               rb=_flat_ln(nrb))
            else:
                y = K.ln_apply(u, ls2, g2, b2, M2, V, Cout, res_mode=1 if residual else 0,
                               r=x if residual else None)

        ctx.cfg = cfg
        ctx.sup = sup if gather else None
        ctx.dims = (N, Cin, Cout, T, T_out, V, P, pad, res_conv)
        saved = dict(x=x, A32=A32, XA=XA, g=g, u=u, y=y, wg=wg, bg=bg, wt=wt, n1w=n1w, n1b=n1b, n2w=n2w, n2b=n2b)
        if norm == BN:
            saved.update(mr1=mr1, sc1=sc1, sh1=sh1, mr2=mr2, ybits=ybits)
        else:
            saved.update(ls1=ls1, ls2=ls2, h=h)
        if res_conv:  # strr: the residual norm's (mean, rstd), BatchNorm per channel / LayerNorm per frame
            saved.update(r=r, wr=wr, nrw=nrw, nrb=nrb, strr=strr)
        _save_named(ctx, **saved)
        ctx.in_dtype = A.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        cfg, s = ctx.cfg, _saved(ctx)
        kt, stride, residual, norm, dtype, packs, sync = (cfg.kt, cfg.stride, cfg.residual, cfg.norm, cfg.dtype,
                                                          cfg.packs, cfg.sync)
        N, Cin, Cout, T, T_out, V, P, pad, res_conv = ctx.dims
        x, A32, g, u, y, wg, bg, wt = s.x, s.A32, s.g, s.u, s.y, s.wg, s.bg, s.wt
        # (mean, rstd) of norm1 / norm2: BatchNorm per channel, LayerNorm per frame
        st1, st2 = (s.mr1, s.mr2) if norm == BN else (s.ls1, s.ls2)
        ybits = s.ybits if norm == BN else None
        dev = x.device
        dy = K.to_rows(dy, dtype)
        M1, M2 = N * T * V, N * T_out * V
        grads = {}
        # the temporal / residual weight gradients come back in nn.Conv2d order, overwritten (conv_wgrad_w); the
        # graph-conv accumulation targets (dW, dA, per-joint row sums) are zero-filled only on the routes that
        # accumulate into them (one fill for all three)
        zl = {}

        def zero_targets():
            if not zl:
                zl["t"] = K.zeros_arena(dev, (P * Cout, Cin), (P, V, V),
                                        (N, V, Cout) if A32.dim() == 4 else (V, Cout))
            return zl["t"]

        # ---- through relu(norm2(u) + res): dz = dy * [y > 0]
        du = K.cl_empty(N, Cout, T_out, V, dtype, dev)
        dx = K.cl_empty(N, Cin, T, V, dtype, dev)
        dx_written = False
        fused = norm == BN and K.bn_fused_ok(Cout, dtype)
        # identity residual with the forward's sign bits and the gathered graph conv: its masked gradient
        # dy * [y > 0] is added in the graph conv's data-gradient epilogue (not written to dx by the BN backward)
        res_in_gconv = fused and residual and not res_conv and ybits is not None and ctx.sup is not None
        if fused:
            # one reduce + one apply pass: du, the residual branch's dr (or dx = dz), and the conv-bias
            # gradients (column sums of du / dr) together
            kw = dict(mask=1, mref=y, x1=u, mr1=st2, g1=_f32(s.n2w), out1=du, bias_sums=True)
            if ybits is not None:
                kw.update(mask=3, mref=ybits)
            if res_conv:
                dr = K.cl_empty(N, Cout, T_out, V, dtype, dev)
                kw.update(x2=s.r, mr2=s.strr, g2=_f32(s.nrw), out2=dr)
            elif residual and not res_in_gconv:
                kw.update(out2=dx)
                dx_written = True
            sums2, osum2 = K.bn_bwd_fused(dy, M2, Cout, sync=sync, **kw)
            grads["n2w"], grads["n2b"] = sums2[1], sums2[0]
            grads["bt"] = osum2[0]
            if res_conv:  # nrb == n2b numerically; own storage so no two parameters share a grad tensor
                grads["nrw"], grads["nrb"] = sums2[2], sums2[0].clone()
                grads["br"] = osum2[1]
        else:
            grads["n2w"], grads["n2b"] = _norm_backward(norm, dy, u, st2, s.n2w, s.n2b, du, sync, mask=1, mref=y)

        if res_conv:
            if not fused:
                dr = K.cl_empty(N, Cout, T_out, V, dtype, dev)
                grads["nrw"], grads["nrb"] = _norm_backward(norm, dy, s.r, s.strr, s.nrw, s.nrb, dr, sync,
                                                            mask=1, mref=y)
                grads["br"] = K.bn_bwd_reduce(dr, M2, Cout)[:, 0].clone()
            # residual conv (1x1, stride s, bias): data grad (transposed), weight grad
            wrTp, cq, kq = packs.wrT if packs is not None else \
                K.pack_weight(_f32(s.wr).view(Cout, Cin).t().unsqueeze(0), dtype)
            grads["wr"] = K.conv_wgrad_w(x, dr, Cin, Cout, T, T_out, Kt=1, stride=stride, pad=0).view(Cout, Cin, 1, 1)
            K.conv_rows(dr, wrTp, Cout, Cin, cq, kq, T_out, T, Kt=1, stride=stride, pad=0, trans=True, out=dx)
            dx_written = True
        elif residual and not fused:
            K.bn_bwd_apply(dy, M2, Cin, dx, mask=1, mref=y)  # dx = dz
            dx_written = True

        # ---- temporal conv: dh = conv^T(du), dWt, dbt
        # [Kt][Cin=Cout][Cout]: W[co][ci][dt] -> [dt][ci][co]
        wtTp, cq, kq = packs.wtT if packs is not None else \
            K.pack_weight(wt.detach().float().squeeze(-1).permute(2, 1, 0), dtype, stride=stride, trans=True)
        if norm == BN:
            pro1, hin = dict(pro=1, pro_a=s.sc1, pro_b=s.sh1), g
        else:  # the forward's h = relu(LN1(g)), recomputed should a forward route not keep it
            pro1 = {}
            hin = s.h if s.h is not None else \
                K.ln_apply(g, st1, _flat_ln(s.n1w), _flat_ln(s.n1b), M1, V, Cout, relu=True)
        grads["wt"] = K.conv_wgrad_w(hin, du, Cout, Cout, T, T_out, Kt=kt, stride=stride, pad=pad,
                                     **pro1).unsqueeze(-1)  # (co, ci, Kt, 1)
        if K.tconv_frame_ok(Cout, kt, stride, V, dtype) and getattr(wtTp, "frag_stride", None) == 1:
            dh = K.tconv_frame(du, wtTp, cq, kq, trans=True)
        else:
            dh = K.conv_rows(du, wtTp, Cout, Cout, cq, kq, T_out, T, Kt=kt, stride=stride, pad=pad, trans=True)
        if not fused:
            grads["bt"] = K.bn_bwd_reduce(du, M2, Cout)[:, 0].clone()

        # ---- through relu(norm1(g))
        dg = K.cl_empty(N, Cout, T, V, dtype, dev)
        if fused:
            s1, _ = K.bn_bwd_fused(dh, M1, Cout, mask=2, mref=g, msc=s.sc1, msh=s.sh1, x1=g, mr1=st1,
                                   g1=_f32(s.n1w), out1=dg, sync=sync)
            grads["n1w"], grads["n1b"] = s1[1], s1[0]
        else:  # the mask is relu(norm1(g)) > 0: the BatchNorm kernels recompute it from g, scale1, shift1
            m1 = dict(mask=2, mref=g, msc=s.sc1, msh=s.sh1) if norm == BN else dict(mask=2)
            grads["n1w"], grads["n1b"] = _norm_backward(norm, dh, g, st1, s.n1w, s.n1b, dg, sync, **m1)

        # ---- graph convolution backward
        if ctx.sup is not None:
            # data grad: same gather GEMM on dg over the reverse lists with transposed effective weights;
            # weight / adjacency / bias grads through the per-joint dWeff[w][j] = sum_i dg[(i,w)] x[(i,S(w)_j)]^T blocks
            sup = ctx.sup
            wg2 = _f32(wg).reshape(P * Cout, Cin)
            dA, grads["wg"], grads["bg"] = _gconv_wgrad_dweff(x, dg, A32, wg2, bg, sup,
                                                              cfg.dense_dA and ctx.needs_input_grad[1], zero_targets,
                                                              dtype)
            wgT = packs.gwT if packs is not None and packs.gwT is not None else \
                K.gconv_weights(A32, wg2, sup, Cout, Cin, True, dtype)
            K.gconv(dg, wgT, sup, Cout, Cin, trans=True, out=dx, accumulate=dx_written,
                    res=(dy, ybits) if res_in_gconv else None)
        else:
            dA, grads["wg"], grads["bg"] = gcn_backward(x, A32, s.XA, wg, bg, dg, dx, dx_written, dtype,
                                                        z_S=zero_targets()[2])

        def gr(name, like):
            v = grads.get(name)
            if v is None or like is None or not like.requires_grad:
                return None
            return v.to(like.dtype).view(like.shape)

        wr_, nrw_, nrb_ = (s.wr, s.nrw, s.nrb) if res_conv else (None, None, None)
        return (dx, dA.to(ctx.in_dtype), gr("wg", wg), gr("bg", bg), gr("n1w", s.n1w), gr("n1b", s.n1b), gr("wt", wt),
                grads["bt"], gr("n2w", s.n2w), gr("n2b", s.n2b), gr("wr", wr_),
                grads.get("br"), gr("nrw", nrw_), gr("nrb", nrb_), None)


def _norm_backward(norm, dy, x, st, gamma, beta, out, sync=None, **mask):
    """Backward of one norm (norm1, norm2, a residual norm) of rows x (N, C, T, V) with saved (mean, rstd) ``st``:
    the input gradient of ``dy`` (under ``mask``: the kernels' mask / mref / msc / msh arguments) into ``out``.
    BatchNorm: reduce, SyncBatchNorm exchange of the sums, apply; LayerNorm: ln_bwd.  Returns (dgamma, dbeta),
    this rank's own."""
    N, C, T, V = x.shape
    M = N * T * V
    if norm == BN:
        sums = K.bn_bwd_reduce(dy, M, C, x=x, mean_rstd=st, **mask)
        dgamma, dbeta = sums[:, 1].clone(), sums[:, 0].clone()
        if sync is not None:
            sync.all_reduce_sums(sums, M)
        K.bn_bwd_apply(dy, M, C, out, x=x, mean_rstd=st, gamma=_f32(gamma), sums=sums, **mask)
        return dgamma, dbeta
    dgb = torch.zeros((2, C * V), dtype=torch.float32, device=x.device)
    K.ln_bwd(dy, x, st, _flat_ln(gamma), _flat_ln(beta), N * T, V, C, out, dgb=dgb, **mask)
    return dgb[0].view(gamma.shape), dgb[1].view(beta.shape)


def _gconv_wgrad_dweff(x, dg, A32, wg2, bg, sup, dense_dA, zero_targets, dtype):
    """Graph-conv weight / adjacency / bias gradients of the gathered route through the per-joint
    dWeff[w][j] = sum_i dg[(i,w)] x[(i,S(w)_j)]^T blocks (gconv_wgrad + finish).  ``dense_dA``: caller-owned A,
    whose gradient is also wanted off the support.  Returns (dA, dWg [P*Cout][Cin], dbg)."""
    N, Cin, T, V = x.shape
    P, Cout = A32.shape[-3], dg.shape[1]
    fuse_s = A32.dim() == 3 and K.gconv_wgrad_rowsum_ok(sup, Cin, Cout, dtype)
    # row sums: overwritten by the joint-grouped wgrad kernel
    S_rows = torch.empty((V, Cout), dtype=torch.float32, device=x.device) if fuse_s else None
    dweff = K.gconv_wgrad(x, dg, sup, Cin, Cout, rowsum=S_rows)
    if fuse_s and not dense_dA and K.gconv_finish_bias_ok(A32, sup):
        # dW, dA (support + bias through A) and db in two launches, outputs overwritten
        dwg2, dA, dbg = K.gconv_finish_bias(dweff, A32, wg2, sup, Cout, Cin, _f32(bg), S_rows)
        return dA, dwg2, dbg
    z_dwg, z_dA, z_S = zero_targets()
    dwg2, dA = K.gconv_finish(dweff, A32, wg2, sup, Cout, Cin, dW=z_dwg, dA=z_dA)
    if dense_dA:
        # the reference's dA is dense (also off the graph's support), so take it from the A-first
        # factorisation dA_p[v][w] = sum x[(i,v)] . (dg W_p)[(i,w)]
        dA = K.amix_dA(x, _gcn_dgrad_rows(dg, wg2, P, Cin, Cout, T, dtype), A32)
    dA, dbg = _bias_through_A(dA, A32, bg, dg, S=S_rows, z_S=z_S)
    return dA, dwg2, dbg


@K.on_tensor_device
class GcnFunction(torch.autograd.Function):
    """ConvTemporalGraphical.forward alone (models/utils/tgcn.py:58-79): conv1x1(+bias) -> @A -> sum_P."""

    @staticmethod
    def forward(ctx, x, A, wg, bg, dtype):
        x = K.to_rows(x, dtype)
        A32 = _f32(A)
        XA, g, _ = gcn_forward(x, A32, wg, bg, dtype)
        ctx.save_for_backward(x, A32, XA, wg, bg)
        ctx.meta = (dtype, A.dtype)
        return g

    @staticmethod
    def backward(ctx, dg):
        x, A32, XA, wg, bg = ctx.saved_tensors
        dtype, adt = ctx.meta
        dx = K.cl_empty(*x.shape, dtype, x.device)
        dA, dwg, dbg = gcn_backward(x, A32, XA, wg, bg, K.to_rows(dg, dtype), dx, False, dtype)
        return dx, dA.to(adt), dwg.to(wg.dtype), dbg.to(bg.dtype), None


def plan_conv1x1_packs(plan, w, dtype):
    """Forward and data-gradient packs of a 1x1 conv weight (Cout, Cin', 1, 1) for Conv1x1Function; Cin' may
    be below the activation's channel count (fcn_in: 3 input features in 8-channel rows), the packs pad."""
    Cout, Ci = w.shape[0], w.shape[1]
    w2 = w.detach().view(Cout, Ci)
    return K.pack_weight(w2.unsqueeze(0), dtype, plan=plan), K.pack_weight(w2.t().unsqueeze(0), dtype, plan=plan)


@K.on_tensor_device
class Conv1x1Function(torch.autograd.Function):
    """Pointwise conv on channels-last rows (fcn_in / fcn_out, stgcn.py:49,74): y = W x + b.  w may have fewer
    input channels than x (fcn_in's 3 features in 8-channel rows: the missing columns act as zeros); packs =
    plan_conv1x1_packs(...) filled by the model's PrepPlan launch, or None (packed here)."""

    @staticmethod
    def forward(ctx, x, w, b, dtype, packs=None):
        x = K.to_rows(x, dtype)
        N, Cin, T, V = x.shape
        Cout, Ci = w.shape[0], w.shape[1]
        wp, cp, kp = packs[0] if packs is not None else \
            K.pack_weight(w.detach().float().view(Cout, Ci).unsqueeze(0), dtype)
        y = K.conv_rows(x, wp, Cin, Cout, cp, kp, T, T, bias=_f32(b))
        ctx.save_for_backward(x, w)
        ctx.dtype = dtype
        ctx.packT = packs[1] if packs is not None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dtype = ctx.dtype
        N, Cin, T, V = x.shape
        Cout, Ci = w.shape[0], w.shape[1]
        dy = K.to_rows(dy, dtype)
        wT, cq, kq = ctx.packT if ctx.packT is not None else \
            K.pack_weight(w.detach().float().view(Cout, Ci).t().unsqueeze(0), dtype)
        dx = K.conv_rows(dy, wT, Cout, Cin, cq, kq, T, T, trans=True)
        dw = K.conv_wgrad_w(x, dy, Cin, Cout, T, T).view(Cout, Cin, 1, 1)
        if Ci < Cin:
            dw = dw[:, :Ci]
        db = K.bn_bwd_reduce(dy, N * T * V, Cout)[:, 0]
        return dx, dw.to(w.dtype), db.to(w.dtype), None, None


@K.on_tensor_device
class InputBatchNormFunction(torch.autograd.Function):
    """BatchNorm1d(V*C) on (N, V*C, T) (models/utils/batchnorm.py:13-23): per-(v,c) batch stats over
    (N,T).  Channels-last NTVC rows are exactly [N*T][V*C], so it is a row BatchNorm with V*C channels."""

    @staticmethod
    def forward(ctx, x, w, b, dtype, sync=None):
        x = K.to_rows(x, dtype)
        N, C, T, V = x.shape
        if K.rows_ld(x) != C:
            x = x.contiguous(memory_format=torch.channels_last)
        F_, CV = N * T, V * C
        part, nb, _ = K.bn_stats_partial(x, F_, CV, ld=CV)
        # reference weight index = v*C + c == channels-last (v, c) order
        mr, sc, sh = (sync.finalize if sync is not None else K.bn_finalize)(part, nb, CV, CV, w.detach().float(),
                                                                            b.detach().float())
        y = K.cl_empty(N, C, T, V, dtype, x.device)
        K.bn_apply(x, sc, sh, F_, CV, relu=False, out=y, ldu=CV, ldy=CV)
        ctx.save_for_backward(x, w, mr)
        ctx.dtype = dtype
        ctx.sync = sync
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mr = ctx.saved_tensors
        N, C, T, V = x.shape
        F_, CV = N * T, V * C
        dy = K.to_rows(dy, ctx.dtype)
        if K.rows_ld(dy) != C:
            dy = dy.contiguous(memory_format=torch.channels_last)
        sums = _bn_reduce_flat(dy, x, mr, F_, CV)
        dw, db = sums[:, 1].to(w.dtype), sums[:, 0].to(w.dtype)
        if ctx.sync is not None:  # the parameter gradients keep this rank's own sums (copies: sums is exchanged)
            dw, db = dw.clone(), db.clone()
            ctx.sync.all_reduce_sums(sums, F_)
        dx = K.cl_empty(N, C, T, V, ctx.dtype, x.device)
        _bn_apply_flat(dy, x, mr, w.detach().float(), sums, F_, CV, dx)
        return dx, dw, db, None, None


@K.on_tensor_device
class WindowStageFunction(torch.autograd.Function):
    """norm_in + fcn_in of a batch of sliding windows (WindowSegment, segment_generator.py:132-145; stgcn.py:
    82-85) straight from the padded capture (1, Cin, Lp, V): windows [n0, n0+nw) of W frames, never formed
    (window.hip).  mode 0: BatchNorm1d(V*Cin) with the windowed batch's statistics (each frame weighted by
    the windows holding it); mode 1: the per-frame LayerNorm([Cin,1,V]).  Returns the first activation
    (nw, Cout, W, V) channels-last; backward gives the norm and fcn_in parameter gradients (the capture
    takes none, as in the reference where it is data)."""

    @staticmethod
    def forward(ctx, capture, n0, nw, W, norm_w, norm_b, w, b, mode, dtype, sync=None):
        Cout = w.shape[0]
        w2 = w.detach().float().reshape(Cout, -1)
        bias = b.detach().float() if b is not None else None
        g, be = norm_w.detach().float().reshape(-1), norm_b.detach().float().reshape(-1)
        if mode == 0:
            part, nb = K.window_stats(capture, W, n0, nw, 0)
            VC = part.shape[1]
            # SyncBatchNorm: only the forward statistics are exchanged (the capture takes no gradient, and the
            # parameter gradients are this rank's own sums)
            st, sc, sh = (sync.finalize if sync is not None else K.bn_finalize)(part, nb, VC, VC, g, be)
            y = K.window_expand(capture, W, n0, nw, 0, sc, sh, None, w2, bias, dtype)
        else:
            st, _ = K.window_stats(capture, W, n0, nw, 1)
            y = K.window_expand(capture, W, n0, nw, 1, g, be, st, w2, bias, dtype)
        ctx.save_for_backward(capture, norm_w, norm_b, w, b, st)
        ctx.cfg = (n0, nw, W, mode)
        return y

    @staticmethod
    def backward(ctx, dy):
        capture, norm_w, norm_b, w, b, st = ctx.saved_tensors
        n0, nw, W, mode = ctx.cfg
        dy = K.to_rows(dy, dy.dtype)
        Cout = w.shape[0]
        dg, dbe, dw, db = K.window_grad(dy, capture, W, n0, nw, mode, st, norm_w.detach().float().reshape(-1),
                                        norm_b.detach().float().reshape(-1), w.detach().float().reshape(Cout, -1))
        return (None, None, None, None, dg.view(norm_w.shape).to(norm_w.dtype), dbe.view(norm_b.shape).to(norm_b.dtype),
                dw.view(w.shape).to(w.dtype), None if b is None else db.to(b.dtype), None, None, None)


def stage_window_batch(xb, norm_in, fcn_in, dtype):
    """norm_in (modules.BatchNorm1d or LayerNorm) + fcn_in of a segment.WindowBatch, from its capture."""
    ln = not hasattr(norm_in, "norm")  # modules.BatchNorm1d wraps nn.BatchNorm1d as .norm
    g, b = (norm_in.weight, norm_in.bias) if ln else (norm_in.norm.weight, norm_in.norm.bias)
    return WindowStageFunction.apply(xb.capture, xb.n0, xb.nw, xb.W, g, b, fcn_in.weight, fcn_in.bias,
                                     1 if ln else 0, dtype, None if ln else active_sync(norm_in))


def _as_rows(t, F_, CV):
    # a (F_, 1, 1, CV) contiguous buffer viewed as logical (F_, CV, 1, 1) channels-last
    return t.permute(0, 2, 3, 1).contiguous().view(F_, 1, 1, CV).permute(0, 3, 1, 2)


def _bn_reduce_flat(dy, x, mr, F_, CV):
    return K.bn_bwd_reduce(_as_rows(dy, F_, CV), F_, CV, x=_as_rows(x, F_, CV), mean_rstd=mr)


def _bn_apply_flat(dy, x, mr, gamma, sums, F_, CV, dx):
    out = _as_rows(dx, F_, CV)
    K.bn_bwd_apply(_as_rows(dy, F_, CV), F_, CV, out, x=_as_rows(x, F_, CV), mean_rstd=mr, gamma=gamma, sums=sums)
    return out


@K.on_tensor_device
class LayerNormFunction(torch.autograd.Function):
    """Custom LayerNorm([C,1,V]) (models/utils/layernorm.py:22-28) on channels-last rows."""

    @staticmethod
    def forward(ctx, x, w, b, dtype):
        x = K.to_rows(x, dtype)
        N, C, T, V = x.shape
        st = K.ln_stats(x, N * T, V, C)
        y = K.ln_apply(x, st, _flat_ln(w), _flat_ln(b), N * T * V, V, C, relu=False)
        ctx.save_for_backward(x, w, b, st)
        ctx.dtype = dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, st = ctx.saved_tensors
        N, C, T, V = x.shape
        dy = K.to_rows(dy, ctx.dtype)
        dx = K.cl_empty(N, C, T, V, ctx.dtype, x.device)
        dgb = torch.zeros((2, C * V), dtype=torch.float32, device=x.device)
        K.ln_bwd(dy, x, st, _flat_ln(w), _flat_ln(b), N * T, V, C, dx, dgb=dgb)
        return dx, dgb[0].view(w.shape).to(w.dtype), dgb[1].view(b.shape).to(b.dtype), None


@K.on_tensor_device
class PoolFunction(torch.autograd.Function):
    """F.avg_pool2d(x, x.size()[2:]) (stgcn.py:92) -> (N, C, 1, 1); joints_only=True is the RT head's
    AvgPool2d((1, V)) (rtstgcn.py:127,149) -> (N, C, T, 1)."""

    @staticmethod
    def forward(ctx, x, dtype, joints_only=False):
        x = K.to_rows(x, dtype)
        N, C, T, V = x.shape
        ctx.shape = (N, C, T, V)
        ctx.dtype = dtype
        ctx.joints_only = joints_only
        if joints_only:
            return K.pool_rows(x, N * T, V, C).reshape(N, T, 1, C).permute(0, 3, 1, 2)
        return K.pool_rows(x, N, T * V, C)

    @staticmethod
    def backward(ctx, dp):
        N, C, T, V = ctx.shape
        dp = K.to_rows(dp, ctx.dtype)
        dx = K.cl_empty(N, C, T, V, ctx.dtype, dp.device)
        if ctx.joints_only:
            dp = dp.permute(0, 2, 3, 1).reshape(N * T, 1, 1, C).permute(0, 3, 1, 2)
            K.unpool_rows(dp, V, C, N * T * V, dx)
        else:
            K.unpool_rows(dp, T * V, C, N * T * V, dx)
        return dx, None, None


def _strided_rows_ok(t, dtype) -> bool:
    """A (N, C, T, V) tensor the row kernels can read in place: the dtype, unit channel stride and evenly
    strided rows (K.rows_ld)."""
    if t.dtype != dtype or t.dim() != 4 or t.stride(1) != 1 or not t.is_cuda:
        return False
    try:
        K.rows_ld(t)
    except RuntimeError:
        return False
    return True


@K.on_tensor_device
class AttentionFunction(torch.autograd.Function):
    """C = softmax(theta^T phi) per (n, p) (models/aagcn/aagcn.py:142-145), theta/phi channels-last rows."""

    @staticmethod
    def forward(ctx, theta, phi, P, dtype):
        # strided rows are fine (the kernels take a row stride): attn_proj's theta / phi are the two channel
        # halves of one row buffer, and keeping them there lets attn_bwd return both gradients in one buffer
        theta = theta if _strided_rows_ok(theta, dtype) else K.to_rows(theta, dtype)
        phi = phi if _strided_rows_ok(phi, dtype) else K.to_rows(phi, dtype)
        C = K.attn_scores(theta, phi, P)
        ctx.save_for_backward(theta, phi, C)
        ctx.P = P
        ctx.dtype = dtype
        return C

    @staticmethod
    def backward(ctx, dC):
        theta, phi, C = ctx.saved_tensors
        dth, dph = K.attn_bwd(theta, phi, ctx.P, C, dC.float().contiguous())
        return dth, dph, None, None


def attn_proj_ok(x, Cin, Nt, Np, dtype) -> bool:
    return dtype == torch.bfloat16 and Cin % 16 == 0 and Cin <= 256 and Nt % 4 == 0 and Np % 4 == 0


@K.on_tensor_device
class AttnProjFunction(torch.autograd.Function):
    """AgcnLayer's theta and phi 1x1 convs (aagcn.py:139-141) for a bf16 model: one fp32-output projection
    of the bf16 activation (stgcn_attn_proj: no fp32 copy of x, no fp32 GEMM), theta and phi the two
    channel halves of one row buffer.  Backward: the two gradients (one buffer from attn_bwd) rounded to
    bf16 once, then the bf16 transposed 1x1 conv (dx) and weight-gradient kernels; the bias gradients are
    column sums of the fp32 gradients."""

    @staticmethod
    def forward(ctx, x, wt, bt, wp, bp):
        x = K.to_rows(x, torch.bfloat16)
        Nt, Np = wt.shape[0], wp.shape[0]
        Cin = x.shape[1]
        W = torch.cat([wt.detach().float().reshape(Nt, Cin), wp.detach().float().reshape(Np, Cin)])
        b = torch.cat([bt.detach().float(), bp.detach().float()])
        out = K.attn_proj(x, W, b)
        ctx.save_for_backward(x, W)
        ctx.split = (Nt, Np)
        ctx.shapes = (wt.shape, wp.shape, wt.dtype)
        return out[:, :Nt], out[:, Nt:]

    @staticmethod
    def backward(ctx, dth, dph):
        x, W = ctx.saved_tensors
        Nt, Np = ctx.split
        N, Cin, T, V = x.shape
        Nout = Nt + Np
        es = dth.element_size()
        if (dth.dim() == 4 and K.rows_ld(dth) == Nout and K.rows_ld(dph) == Nout
                and dph.data_ptr() - dth.data_ptr() == Nt * es):
            D = torch.as_strided(dth, (N, Nout, T, V), dth.stride())  # the attn_bwd buffer, both halves
        else:
            D = torch.cat([dth, dph], 1).contiguous(memory_format=torch.channels_last)
        D = D.float()
        # the bf16 GEMM operand and the bias gradients (column sums of the fp32 values) from one read of D
        D16, db = K.cast_colsum(D, N * T * V, Nout)
        wT, cq, kq = K.pack_weight(W.t().reshape(1, Cin, Nout), torch.bfloat16)
        dx = K.conv_rows(D16, wT, Nout, Cin, cq, kq, T, T, trans=True)
        dW = K.conv_wgrad(x, D16, Cin, Nout, T, T).view(Nout, Cin)
        wts, wps, wdt = ctx.shapes
        return (dx, dW[:Nt].reshape(wts).to(wdt), db[:Nt].to(wdt), dW[Nt:].reshape(wps).to(wdt),
                db[Nt:].to(wdt))


@K.on_tensor_device
class RtOfflineLayerFunction(torch.autograd.Function):
    """OfflineLayer.forward (models/rtstgcn/rtstgcn.py:343-389) with the Toeplitz matmul it intends
    (rtstgcn.py:366-379) evaluated as the causal K//S-tap box sum it is:

        res = 0 | x | norm_r(conv1x1_nobias(x))
        b   = boxsum_{K,S}( sum_p A_p-mix( conv1x1(x) ) )          (A = A_graph * edge_importance)
        y   = relu(relu(norm(b)) + res)      (residual)     |     relu(norm(b))     (no residual)
    """

    @staticmethod
    def forward(ctx, x, A, wc, bc, nw, nb, wr, nrw, nrb, cfg):
        Kt, S, residual, norm, dtype, sync = cfg.Kt, cfg.S, cfg.residual, cfg.norm, cfg.dtype, cfg.sync
        bn_finalize = sync.finalize if sync is not None else K.bn_finalize
        dev = x.device
        x = K.to_rows(x, dtype)
        N, Cin, L, V = x.shape
        P = A.shape[-3]
        Cout = wc.shape[0] // P
        M = N * L * V
        A32 = _f32(A)
        res_conv = residual and not (Cin == Cout and S == 1)
        XA, z, _ = gcn_forward(x, A32, wc, bc, dtype)
        b = K.box_sum(z, Kt, S)
        relu_mode = 3 if residual else 2
        r = str_ = None
        if res_conv:
            wrp, cq, kq = K.pack_weight(_f32(wr).view(1, Cout, Cin), dtype)
            if norm == BN:
                str_, _ = gcn_stats_buffer(M, Cout, dev)
            r = K.conv_rows(x, wrp, Cin, Cout, cq, kq, L, L, stats=str_)
        if norm == BN:
            part, nbk, _ = K.bn_stats_partial(b, M, Cout)
            st, sc, sh = bn_finalize(part, nbk, Cout, Cout, _f32(nw), _f32(nb))
            if res_conv:
                stn, scr, shr = bn_finalize(str_, str_.shape[0], str_.shape[1], Cout, _f32(nrw), _f32(nrb))
                y = K.bn_apply(b, sc, sh, M, Cout, res_mode=2, r=r, rsc=scr, rsh=shr, relu=relu_mode)
            else:
                y = K.bn_apply(b, sc, sh, M, Cout, res_mode=1 if residual else 0, r=x if residual else None,
                               relu=relu_mode)
        else:
            st = K.ln_stats(b, N * L, V, Cout)
            if res_conv:
                stn = K.ln_stats(r, N * L, V, Cout)
                y = K.ln_apply(b, st, _flat_ln(nw), _flat_ln(nb), M, V, Cout, res_mode=2, r=r, rst=stn,
                               rg=_flat_ln(nrw), rb=_flat_ln(nrb), relu=relu_mode)
            else:
                y = K.ln_apply(b, st, _flat_ln(nw), _flat_ln(nb), M, V, Cout, res_mode=1 if residual else 0,
                               r=x if residual else None, relu=relu_mode)
        # st / stn: (mean, rstd) of the norm / the residual norm
        saved = dict(x=x, A32=A32, XA=XA, b=b, y=y, st=st, wc=wc, bc=bc, nw=nw, nb=nb)
        if norm == BN:
            saved.update(sc=sc, sh=sh)
        if res_conv:
            saved.update(r=r, stn=stn, wr=wr, nrw=nrw, nrb=nrb)
        _save_named(ctx, **saved)
        ctx.cfg = cfg
        ctx.res_conv = res_conv
        ctx.in_dtype = A.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        cfg, s, res_conv = ctx.cfg, _saved(ctx), ctx.res_conv
        Kt, S, residual, norm, dtype, sync = cfg.Kt, cfg.S, cfg.residual, cfg.norm, cfg.dtype, cfg.sync
        x, b, y = s.x, s.b, s.y
        N, Cin, L, V = x.shape
        Cout = b.shape[1]
        dev = x.device
        M = N * L * V
        dy = K.to_rows(dy, dtype)
        # dq = grad w.r.t. (relu(norm(b)) + res)
        if residual:
            dq = K.cl_empty(N, Cout, L, V, dtype, dev)
            K.bn_bwd_apply(dy, M, Cout, dq, mask=1, mref=y)
        else:
            dq = dy
        dx = K.cl_empty(N, Cin, L, V, dtype, dev)
        dx_written = False
        g = {}
        if res_conv:
            dr = K.cl_empty(N, Cout, L, V, dtype, dev)
            g["nrw"], g["nrb"] = _norm_backward(norm, dq, s.r, s.stn, s.nrw, s.nrb, dr, sync)
            wrT, cq, kq = K.pack_weight(_f32(s.wr).view(Cout, Cin).t().reshape(1, Cin, Cout), dtype)
            K.conv_rows(dr, wrT, Cout, Cin, cq, kq, L, L, trans=True, out=dx)
            dx_written = True
            g["wr"] = K.conv_wgrad_w(x, dr, Cin, Cout, L, L).view(Cout, Cin, 1, 1)
        elif residual:
            K.bn_bwd_apply(dq, M, Cin, dx)  # dx = dq
            dx_written = True
        # through relu(norm(b)): the BatchNorm kernels recompute the mask from b, scale, shift
        db = K.cl_empty(N, Cout, L, V, dtype, dev)
        m = dict(mask=2, mref=b, msc=s.sc, msh=s.sh) if norm == BN else dict(mask=2)
        g["nw"], g["nb"] = _norm_backward(norm, dq, b, s.st, s.nw, s.nb, db, sync, **m)
        dz = K.box_sum(db, Kt, S, trans=True)
        dA, dwc, dbc = gcn_backward(x, s.A32, s.XA, s.wc, s.bc, dz, dx, dx_written, dtype)

        def gr(name, like):
            v = g.get(name)
            return None if v is None or like is None or not like.requires_grad else v.to(like.dtype).view(like.shape)

        return (dx, dA.to(ctx.in_dtype), dwc.to(s.wc.dtype), dbc.to(s.bc.dtype), gr("nw", s.nw), gr("nb", s.nb),
                gr("wr", s.wr if res_conv else None), gr("nrw", s.nrw if res_conv else None),
                gr("nrb", s.nrb if res_conv else None), None)
