"""CORAL second-stage refiner -- host-side mirror of models/UDLR.py::SparseRefiner (eval and training-mode forward).

Same constructor / ``from_config`` (reads ``config.window_size``, ``config.threshold``), same sub-module tree and therefore
the same state-dict names as the reference (``HRE.CSF.attn.{norm_q,norm_kv,attn.in_proj_*,attn.out_proj,mlp.0,mlp.2,norm_mlp}``,
``HRE.CSF.depthwise_conv``, ``HRE.CSF.mask_dec``, ``GE.alpha``, ``GE.fuser.{0,2}``) and the same
``forward(input_features, h_inputs, preds, h_targets=None) -> (outputs, ex_loss, opt)`` with the reference's ``opt`` keys
(UDLR.py:77-86).  nn modules are parameter containers (built in the reference's order, so a seeded default init reproduces
the reference's); the arithmetic is HIP: window gather + NCHW->token transpose, LayerNorm, bf16 MFMA projections, the
head_dim-96 cross-attention kernel, fused depthwise-7x7 + mask head, window scatter, gated ensembling.

``ex_loss`` is 0 in eval mode exactly as ``cal_ex_loss`` returns (UDLR.py:52-55).  In training mode (``.train()``) the forward is the same
arithmetic (every dropout of the module is 0, there is no BatchNorm) and ``cal_ex_loss`` adds the IoU-weighted window loss of
UDLR.py:56-75 from ``h_targets`` (HIP: ``ucod_window_loss``), with ``opt['window_targets']`` as the reference sets it.  The loss VALUE is
what the reference defines; it ships no second-stage training loop (``LocalRefineTrainLoop: pass``, engine/runner/loop_CORAL.py:38-39).

The window branch can be trained: in training mode with grad mode on, ``h_targets`` given, at least one window selected and at least one
``HRE.CSF`` parameter requiring grad, ``ex_loss`` hangs on torch autograd through ``_WindowBranchFunction`` (the idiom of
models/discriminator.py::_DiscFunction): its inputs are the 18 ``HRE.CSF`` parameters, its forward is the same arithmetic with the activations
saved, its backward is HIP throughout -- ``ucod_window_loss_grad``, ``ucod_dwconv7_maskdec_bwd``, the dgrad / weight-gradient GEMMs,
``ucod_layernorm_bwd_ex`` / ``ucod_layernorm_param_grad``, ``ucod_cross_attention96_bwd`` -- and returns d ex_loss / d parameter.  ``outputs``,
``opt[...]`` and the GE parameters stay outside the graph unless the module was built with ``train_outputs``.

``train_outputs`` (build-only config key ``config.train_outputs``, default False; the idiom of the ``allow_*`` keys): with it on, in training mode with
grad mode on and at least one of the 22 parameters (the 18 ``HRE.CSF`` ones, ``GE.fuser.{0,2}.{weight,bias}``) requiring grad, ``outputs`` -- and
``ex_loss`` where it exists -- hang on autograd through ``_RefinerFunction``: the same forward arithmetic, bit for bit, and a backward that is HIP
throughout: ``ucod_gated_ensemble_bwd`` (dl2 and the four fuser gradients from the saved ``GE_w``), ``ucod_window_gather`` (the scatter's adjoint, added
into the ``g`` of ``ucod_window_loss_grad``) and ONE ``_csf_backward`` on the sum of the two window cotangents; none when no window is selected (then
``h_preds == 0`` and ``outputs`` depends on the fuser alone).  ``preds``, ``input_features`` and ``h_inputs`` are detached: ``preds`` reaches ``outputs``
through the entropy weight, the 19x19 average and the batch-wide max, and in the CORAL setting all three come from a frozen first stage.  ``GE.alpha``, which
the forward never reads, gets no gradient, as in the reference.  With ``train_outputs`` off every path is what it was.

``direct_wgrad`` (build-only config key ``config.direct_wgrad``, default False): the six weight gradients of ``_csf_backward`` -- the nn.Linear layers of
models/modules/mlp.py:122,141-143 differentiated in their weights -- come from ``ucod_wgrad_bf16_det`` (csrc/wgrad.hip: the token-major bf16 operands read where
they lie, the token axis split deterministically) instead of two transposes and the plain GEMM: the same operand values, another order of the f32 additions.
``loss_and_grads`` is the training forward and the backward with no torch autograd, into caller-owned gradient buffers: what the second-stage training loop calls
(engine/runner/loop_CORAL.py::LocalRefineTrainLoop; the reference's is ``pass``, engine/runner/loop_CORAL.py:38-39, under the optimizer of
engine/runner/runner.py:444-460).  An in-place update of the weights that changes neither ``data_ptr`` nor ``_version`` has to set ``_prepared = None``.
"""
import math

import numpy as np
import torch
from torch import nn

from .. import native as N, ops
from ..engine.registry import MODULE_REGISTRY

LN_EPS = 1e-5
HEADS = 8


class CrossAttentionBlock(nn.Module):
    def __init__(self, dim, num_heads=8, mlp_ratio=4.0):
        super().__init__()
        self.norm_q = nn.LayerNorm(dim)
        self.norm_kv = nn.LayerNorm(dim)
        self.attn = nn.MultiheadAttention(embed_dim=dim, num_heads=num_heads, dropout=0.0, batch_first=True)
        self.drop_path = nn.Identity()
        hidden = int(dim * mlp_ratio)
        self.mlp = nn.Sequential(nn.Linear(dim, hidden), nn.GELU(), nn.Linear(hidden, dim), nn.Dropout(0.0))
        self.norm_mlp = nn.LayerNorm(dim)


class CSF(nn.Module):
    def __init__(self, dim=768):
        super().__init__()
        self.attn = CrossAttentionBlock(dim=dim)
        self.depthwise_conv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.mask_dec = nn.Conv2d(dim, 1, kernel_size=1, padding=0)


class HRE(nn.Module):
    def __init__(self, window_size, dim=768):
        super().__init__()
        self.window_size = window_size
        self.CSF = CSF()


class GatedEnsembler(nn.Module):
    def __init__(self, num_classes):
        super().__init__()
        self.alpha = nn.Parameter(torch.tensor(0.5))
        self.fuser = nn.Sequential(nn.Conv2d(num_classes, 64, kernel_size=1), nn.ReLU(), nn.Conv2d(64, num_classes, kernel_size=1))


class EntropySelector(nn.Module):
    def __init__(self, threshold, window_size):
        super().__init__()
        self.threshold = threshold
        self.window_size = window_size


class _WindowBranchFunction(torch.autograd.Function):
    """ex_loss of the selected windows under torch autograd: tensor inputs = the HRE.CSF parameters, in ``named_parameters`` order.
    forward: CSF on the windows with its activations saved, then the window loss; -> (ex_loss, window_preds, window_targets, window_ious), only
    ex_loss differentiable.  backward: one gradient per parameter in its own shape and dtype, None where it does not require grad."""

    @staticmethod
    def forward(ctx, module, args, *params):
        saved = {}
        win = module._csf(*args["csf"], save=saved)
        loss, sel, ious, aux = module._window_loss(win, *args["loss"])
        ctx.module, ctx.saved, ctx.aux = module, saved, aux
        ctx.mark_non_differentiable(win, sel, ious)
        return loss, win, sel, ious

    @staticmethod
    def backward(ctx, gloss, *_unused):
        grads = ctx.module._csf_backward(ctx.saved, ctx.aux, gloss)
        params = [p for _, p in ctx.module.HRE.CSF.named_parameters()]
        return (None, None) + tuple(g.view(p.shape).to(p.dtype) if need else None for g, p, need in zip(grads, params, ctx.needs_input_grad[2:]))


class _RefinerFunction(torch.autograd.Function):
    """``outputs`` (and ``ex_loss`` where it exists) under torch autograd: tensor inputs = the 18 HRE.CSF parameters in ``named_parameters`` order, then
    GE.fuser.0.weight, GE.fuser.0.bias, GE.fuser.2.weight, GE.fuser.2.bias.  forward -> (outputs, ex_loss or None, window_preds, h_preds, GE_w,
    window_targets or None, window_ious or None); only outputs and ex_loss are differentiable.  backward: a missing cotangent is skipped, the CSF chain
    runs at most once (on the sum of the two window cotangents) and not at all without a selected window."""

    @staticmethod
    def forward(ctx, module, args, *params):
        P, Nw = args["P"], args["Nw"]
        saved, aux, loss, sel, ious = None, None, None, None, None
        if Nw > 0:
            saved = {} if args["save"] else None
            win = module._csf(*args["csf"], save=saved)
            if args["loss"] is not None:
                loss, sel, ious, aux = module._window_loss(win, *args["loss"])
        else:
            win = args["no_windows"]
        outputs, h_preds, ge_w, l1 = module._ensemble(P, win, *args["ensemble"])
        ctx.module, ctx.saved, ctx.aux, ctx.P, ctx.Nw = module, saved, aux, P, Nw
        ctx.ge = (l1, h_preds, ge_w)
        ctx.where = args["ensemble"][:2]                                     # (coords, image index) of the windows
        ctx.set_materialize_grads(False)
        # (without a saved CSF forward nothing can flow back from ex_loss: it leaves as a constant, as it does with train_outputs off)
        ctx.mark_non_differentiable(*[t for t in (win, h_preds, ge_w, sel, ious, loss if saved is None else None) if t is not None])
        return outputs, loss, win, h_preds, ge_w, sel, ious

    @staticmethod
    def backward(ctx, gout, gloss, *_unused):
        m, P = ctx.module, ctx.P
        need = ctx.needs_input_grad[2:]
        csf_params = [p for _, p in m.HRE.CSF.named_parameters()]
        fuser = [m.GE.fuser[0].weight, m.GE.fuser[0].bias, m.GE.fuser[2].weight, m.GE.fuser[2].bias]
        g_csf, g_fuser, dl2 = [None] * 18, [None] * 4, None
        if gout is not None:
            l1, h_preds, ge_w = ctx.ge
            dl2, d_a, d_c, d_d, d_b = ops.gated_ensemble_bwd(l1, h_preds, ge_w, P["f0w"], P["f0b"], P["f2w"], gout.detach().to(l1.device, torch.float32).contiguous())
            g_fuser = [d_a, d_c, d_d, d_b]
        if ctx.Nw > 0 and ctx.saved is not None and any(need[:18]) and (dl2 is not None or (gloss is not None and ctx.aux is not None)):
            g_csf = m._csf_backward(ctx.saved, ctx.aux, gloss if ctx.aux is not None else None, dwin=None if dl2 is None else (dl2,) + tuple(ctx.where))
        grads = [g.view(p.shape).to(p.dtype) if (g is not None and n) else None for g, p, n in zip(list(g_csf) + g_fuser, csf_params + fuser, need)]
        return (None, None) + tuple(grads)


@MODULE_REGISTRY.register()
class SparseRefiner(nn.Module):
    def __init__(self, config, window_size: int, threshold: float, dim: int = 768, train_outputs: bool = False, direct_wgrad: bool = False):
        super().__init__()
        self.config = config
        self.selector = EntropySelector(threshold, window_size)
        self.HRE = HRE(window_size, dim)
        self.GE = GatedEnsembler(1)
        self.window_size = window_size
        self.threshold = threshold
        self.train_outputs = bool(train_outputs)     # opt-in: `outputs` under autograd (module docstring); off: every path as it was
        self.direct_wgrad = bool(direct_wgrad)       # opt-in: the six weight gradients by ucod_wgrad_bf16_det (ops.weight_grad_direct); off: every path as it was
        self.csf_backward_calls = 0                  # how often _csf_backward ran on this instance (one per backward that reaches the CSF parameters)
        self._prepared = None

    @classmethod
    def from_config(cls, config):
        return cls(config, config.window_size, config.threshold, train_outputs=bool(getattr(config, "train_outputs", False)),
                   direct_wgrad=bool(getattr(config, "direct_wgrad", False)))

    # ------------------------------------------------------------------ weight preparation (bf16 GEMM operands, tap-major dw)
    def _prepare(self, dev):
        key = (dev, tuple((p.data_ptr(), p._version) for p in self.parameters()))           # an optimizer step changes the weights: prepare again
        if self._prepared is not None and self._prepared["key"] == key:
            return self._prepared
        blk = self.HRE.CSF.attn
        C = blk.norm_q.weight.shape[0]
        hd = C // HEADS
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()  # noqa: E731
        W, b = f32(blk.attn.in_proj_weight), f32(blk.attn.in_proj_bias)
        qscale = torch.full((C,), (hd ** -0.5) * math.log2(math.e), dtype=torch.float32, device=dev)
        p = dict(dev=dev, key=key, C=C,
                 wq=ops.cast_bf16(W[:C].contiguous()), bq=b[:C].contiguous(), qscale=qscale,
                 wkv=ops.cast_bf16(W[C:].contiguous()), bkv=b[C:].contiguous(),
                 wo=ops.cast_bf16(f32(blk.attn.out_proj.weight)), bo=f32(blk.attn.out_proj.bias),
                 w1=ops.cast_bf16(f32(blk.mlp[0].weight)), b1=f32(blk.mlp[0].bias),
                 w2=ops.cast_bf16(f32(blk.mlp[2].weight)), b2=f32(blk.mlp[2].bias),
                 ones=torch.ones(C, dtype=torch.float32, device=dev),
                 nq=(f32(blk.norm_q.weight), f32(blk.norm_q.bias)), nkv=(f32(blk.norm_kv.weight), f32(blk.norm_kv.bias)),
                 nm=(f32(blk.norm_mlp.weight), f32(blk.norm_mlp.bias)),
                 dwT=f32(self.HRE.CSF.depthwise_conv.weight).reshape(C, 49).t().contiguous(), dwb=f32(self.HRE.CSF.depthwise_conv.bias),
                 mw=f32(self.HRE.CSF.mask_dec.weight).reshape(C), mb=float(self.HRE.CSF.mask_dec.bias.detach().item()),
                 f0w=f32(self.GE.fuser[0].weight).reshape(64), f0b=f32(self.GE.fuser[0].bias), f2w=f32(self.GE.fuser[2].weight).reshape(64),
                 f2b=float(self.GE.fuser[2].bias.detach().item()))
        self._prepared = p
        return p

    # ------------------------------------------------------------------ CSF on the selected windows (CSF.py:38-43)
    def _csf(self, P, l_feats, h_inputs, l_idx, h_idx, H, W, save=None):
        """``save`` (a dict): the training-mode pass -- the same kernels with the attention's base-2 log-sum-exp and the fc1 pre-activation written as well,
        and every activation the backward reads kept in ``save``."""
        lib = N.load()
        dev, C = P["dev"], P["C"]
        Nw, HW = int(h_idx.numel()), H * W
        st = N.stream()
        q_tok = torch.empty(Nw * HW, C, dtype=torch.float32, device=dev)          # residual `query`, token-major
        c_tok = torch.empty(Nw * HW, C, dtype=torch.float32, device=dev)
        N.check(lib.ucod_gather_tokens(N.ptr(h_inputs), N.ptr(h_idx), N.ptr(q_tok), Nw, C, HW, st), "ucod_gather_tokens")
        N.check(lib.ucod_gather_tokens(N.ptr(l_feats), N.ptr(l_idx), N.ptr(c_tok), Nw, C, HW, st), "ucod_gather_tokens")
        qn = ops.layernorm(q_tok, *P["nq"], LN_EPS)
        cn = ops.layernorm(c_tok, *P["nkv"], LN_EPS)
        M = Nw * HW
        q = torch.empty(M, C, dtype=torch.bfloat16, device=dev)
        ops.gemm_bf16(N.EPI_BIAS_BF16, qn, P["wq"], q, M, C, C, bias=P["bq"], scale=P["qscale"])      # softmax scale folded in
        kv = torch.empty(M, 2 * C, dtype=torch.bfloat16, device=dev)
        ops.gemm_bf16(N.EPI_BIAS_BF16, cn, P["wkv"], kv, M, 2 * C, C, bias=P["bkv"])
        att = torch.empty(M, C, dtype=torch.bfloat16, device=dev)
        lse = None
        if save is None:
            N.check(lib.ucod_cross_attention96_fwd(N.ptr(q), C, N.ptr(kv), kv.data_ptr() + C * 2, 2 * C, N.ptr(att), Nw, HW, HW, HEADS, st),
                    "ucod_cross_attention96_fwd")
        else:
            lse = torch.empty(Nw, HEADS, HW, dtype=torch.float32, device=dev)
            N.check(lib.ucod_cross_attention96_fwd_lse(N.ptr(q), C, N.ptr(kv), kv.data_ptr() + C * 2, 2 * C, N.ptr(att), N.ptr(lse), Nw, HW, HW, HEADS, st),
                    "ucod_cross_attention96_fwd_lse")
        x = ops.linear_scale_resid(att, P["wo"], P["bo"], P["ones"], q_tok)        # query + out_proj(attn)
        hn = ops.layernorm(x, *P["nm"], LN_EPS)
        pre = None
        if save is None:
            g = ops.linear_bf16(hn, P["w1"], P["b1"], gelu=True)
        else:
            g = torch.empty(M, P["w1"].shape[0], dtype=torch.bfloat16, device=dev)
            pre = torch.empty_like(g)
            N.check(lib.ucod_gemm_bf16_train(N.EPI_BIAS_GELU_SAVE_BF16, N.ptr(hn), N.ptr(P["w1"]), N.ptr(g), M, g.shape[1], C, N.ptr(P["b1"]), None, N.ptr(pre), 0,
                                             st), "ucod_gemm_bf16_train")
        x2 = ops.linear_scale_resid(g, P["w2"], P["b2"], P["ones"], x)             # x + mlp(norm_mlp(x)); stays token-major
        win = torch.empty(Nw, 1, H, W, dtype=torch.float32, device=dev)
        N.check(lib.ucod_dwconv7_maskdec(N.ptr(x2), N.ptr(P["dwT"]), N.ptr(P["dwb"]), N.ptr(P["mw"]), P["mb"], N.ptr(win), Nw, H, W, C, st),
                "ucod_dwconv7_maskdec")
        if save is not None:
            save.update(P=P, Nw=Nw, H=H, W=W, q_tok=q_tok, c_tok=c_tok, qn=qn, cn=cn, q=q, kv=kv, att=att, lse=lse, x=x, hn=hn, pre=pre, gact=g, x2=x2, win=win)
        return win

    # ------------------------------------------------------------------ d ex_loss / d HRE.CSF parameters (UDLR.py:52-75 through CSF.py:38-43, mlp.py:134-148)
    def _csf_backward(self, S, aux, gloss, dwin=None, out=None):
        """The 18 gradients in ``HRE.CSF.named_parameters()`` order, f32, flat or in the GEMM's [N, K] shape.  ``gloss``: the cotangent of ex_loss, or None;
        ``dwin``: None, or (dl2, coords, image index) -- the cotangent of h_preds, gathered into the same window cotangent ``g``.  ``out``: None, or 18
        contiguous f32 buffers of the parameters' sizes (any shape) that the kernels write instead of fresh tensors (the arena views of a training loop); the
        values are the same bits.  With ``direct_wgrad`` the six weight gradients come from ``ops.weight_grad_direct`` on the bf16 operands the chain holds
        anyway (the values ``ops.weight_grad`` rounds to; only the order of the f32 additions differs) and share one workspace."""
        self.csf_backward_calls += 1
        lib, st = N.load(), N.stream()
        P, Nw, H, W = S["P"], S["Nw"], S["H"], S["W"]
        dev, C = P["dev"], P["C"]
        M = Nw * H * W
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        if out is not None and (len(out) != 18 or any(o.dtype != torch.float32 or not o.is_contiguous() or not o.is_cuda for o in out)):
            raise ValueError("_csf_backward: out must be 18 contiguous float32 device buffers")
        f32 = new
        buf = (lambda i, *shape: new(*shape)) if out is None else (lambda i, *shape: out[i].view(*shape))          # noqa: E731
        if self.direct_wgrad:
            F4 = P["w1"].shape[0]
            wsb_w = torch.empty(max(16, max(lib.ucod_wgrad_bf16_det_workspace_bytes(M, n, k) for n, k in ((C, C), (2 * C, C), (F4, C), (C, F4)))),
                                dtype=torch.uint8, device=dev)
            wgrad = lambda dy16, dy, x, o: ops.weight_grad_direct(dy16, x, out=o, ws=wsb_w)                          # noqa: E731
        else:
            wgrad = lambda dy16, dy, x, o: ops.weight_grad(dy, x, out=o)                                              # noqa: E731
        wt = ops.transpose_pad_bf16                                                 # W bf16 [N, K] -> W^T [K, N]: the B operand of a dgrad product
        g = f32(Nw, 1, H, W)
        if gloss is not None:
            up = gloss.detach().to(dev, torch.float32).reshape(1).contiguous()
            N.check(lib.ucod_window_loss_grad(N.ptr(S["win"]), N.ptr(aux["h_targets"]), N.ptr(aux["win_flat"]), N.ptr(aux["l_up"]), N.ptr(aux["ious"]), N.ptr(up),
                                              N.ptr(g), Nw, aux["B"], H, W, self.window_size, st), "ucod_window_loss_grad")
        if dwin is not None:
            ops.window_gather(dwin[0], dwin[1], dwin[2], g, gloss is not None, H, W, self.window_size)
        # depthwise conv + mask head
        wsb = f32(min(Nw * H, 64) * 49 * C)
        d_dw, d_dwb, d_mw, d_mb, dx2 = buf(14, C, 49), buf(15, C), buf(16, C), buf(17, 1), f32(M, C)
        N.check(lib.ucod_dwconv7_maskdec_bwd(N.ptr(g), N.ptr(S["x2"]), N.ptr(P["dwT"]), N.ptr(P["dwb"]), N.ptr(P["mw"]), N.ptr(d_dw), N.ptr(d_dwb), N.ptr(d_mw),
                                             N.ptr(d_mb), N.ptr(dx2), N.ptr(wsb), wsb.numel() * 4, Nw, H, W, C, st), "ucod_dwconv7_maskdec_bwd")
        # x2 = x + fc2(gelu(fc1(norm_mlp(x))))
        d_b2 = ops.colsum_det(dx2, out=buf(11, C))
        dx2s = ops.cast_bf16(dx2)
        d_w2 = wgrad(dx2s, dx2, S["gact"], buf(10, C, S["gact"].shape[1]))
        dpre = ops.dgrad_bf16(dx2s, wt(P["w2"]), gelu_pre=S["pre"])
        d_b1 = ops.colsum_det(dpre, out=buf(9, dpre.shape[1]))
        d_w1 = wgrad(dpre, dpre, S["hn"], buf(8, dpre.shape[1], C))
        dhn = ops.dgrad_bf16(dpre, wt(P["w1"]))
        d_nm_g, d_nm_b = ops.layernorm_param_grad(dhn, S["x"], LN_EPS, out=(buf(12, C), buf(13, C)))
        dx, dxs = f32(M, C), torch.empty(M, C, dtype=torch.bfloat16, device=dev)   # the residual cotangent in front of norm_mlp, and its bf16 GEMM operand
        N.check(lib.ucod_layernorm_bwd_ex(N.ptr(dhn), N.ptr(S["x"]), N.LNB_DY_BF16, N.ptr(P["nm"][0]), N.ptr(dx2), None, N.ptr(dx), N.ptr(dxs), M, C, LN_EPS, st),
                "ucod_layernorm_bwd_ex")
        # x = query + out_proj(attention); the gathered query / context rows are frozen features: no cotangent for them
        d_bo = ops.colsum_det(dx, out=buf(7, C))
        d_wo = wgrad(dxs, dx, S["att"], buf(6, C, C))
        datt = ops.dgrad_bf16(dxs, wt(P["wo"]))
        HW = H * W
        delta = f32(Nw, HEADS, HW)
        dq = torch.empty(M, C, dtype=torch.bfloat16, device=dev)
        dkv = torch.empty(M, 2 * C, dtype=torch.bfloat16, device=dev)
        q, kv = S["q"], S["kv"]
        N.check(lib.ucod_cross_attention96_bwd(N.ptr(q), C, N.ptr(kv), kv.data_ptr() + C * 2, 2 * C, N.ptr(S["att"]), N.ptr(datt), N.ptr(S["lse"]), N.ptr(delta),
                                               N.ptr(dq), C, N.ptr(dkv), dkv.data_ptr() + C * 2, 2 * C, Nw, HW, HW, HEADS, st), "ucod_cross_attention96_bwd")
        d_inw, d_inb = buf(4, 3 * C, C), buf(5, 3 * C)
        wgrad(dq, dq, S["qn"], d_inw[:C])
        wgrad(dkv, dkv, S["cn"], d_inw[C:])
        ops.colsum_det(dq, out=d_inb[:C])
        ops.colsum_det(dkv, out=d_inb[C:])
        d_nq_g, d_nq_b = ops.layernorm_param_grad(ops.dgrad_bf16(dq, wt(P["wq"])), S["q_tok"], LN_EPS, out=(buf(0, C), buf(1, C)))
        d_nkv_g, d_nkv_b = ops.layernorm_param_grad(ops.dgrad_bf16(dkv, wt(P["wkv"])), S["c_tok"], LN_EPS, out=(buf(2, C), buf(3, C)))
        return (d_nq_g, d_nq_b, d_nkv_g, d_nkv_b, d_inw, d_inb, d_wo, d_bo, d_w1, d_b1, d_w2, d_b2, d_nm_g, d_nm_b, d_dw, d_dwb, d_mw, d_mb)

    def cal_ex_loss(self, opt, win_flat=None):
        """UDLR.py:52-75.  Eval mode / no selected window: 0 (python int, as the reference returns).  Training mode: a 0-d f32 tensor."""
        loss = 0
        if not self.training:
            return loss, opt
        window_preds, preds, h_targets = opt["window_preds"], opt["preds"], opt["h_targets"]
        n = int(window_preds.shape[0])
        if n == 0:                                                          # mask.sum() == 0
            return loss, opt
        if h_targets is None:
            raise ValueError("SparseRefiner in training mode needs h_targets [B*ws*ws, 1, h, w] (models/UDLR.py:62)")
        loss, sel, ious, _ = self._window_loss(window_preds, preds, h_targets, win_flat)
        opt["window_targets"] = sel                                        # UDLR.py:71
        opt["window_ious"] = ious
        return loss, opt

    def _window_loss(self, window_preds, preds, h_targets, win_flat):
        """UDLR.py:62-75 on n >= 1 selected windows -> (loss 0-d f32, window_targets, ious, what the loss gradient reads)."""
        n = int(window_preds.shape[0])
        lib, dev, ws = N.load(), window_preds.device, self.window_size
        h, w = window_preds.shape[-2:]
        B = preds.shape[0]
        h_targets = h_targets.detach().to(dev, torch.float32).contiguous()
        if tuple(h_targets.shape) not in ((B * ws * ws, 1, h, w), (B * ws * ws, h, w)):
            raise ValueError(f"h_targets shape {tuple(h_targets.shape)} != {(B * ws * ws, 1, h, w)}")
        sel = h_targets.view(B * ws * ws, 1, h, w).index_select(0, win_flat.long())
        logits = int(sel.max().item() > 1)                                  # binary_iou's "already a probability?" test (one host sync)
        l_up = ops.bilinear_resize(preds, h * ws, w * ws)
        part = torch.empty(n, dtype=torch.float32, device=dev)
        ious = torch.empty(n, dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        N.check(lib.ucod_window_loss(N.ptr(window_preds), N.ptr(h_targets), N.ptr(win_flat), N.ptr(l_up), logits, N.ptr(part), N.ptr(ious), N.ptr(out),
                                     n, B, h, w, ws, N.stream()), "ucod_window_loss")
        return out[0], sel, ious, dict(h_targets=h_targets, win_flat=win_flat, l_up=l_up, ious=ious, B=B)

    def _ensemble(self, P, window_preds, cd, l_idx, preds, hH, hW):
        """window scatter (HRE.py:18-39) + GatedEnsembler (GE_pix_level.py:16-25) -> (outputs, h_preds, GE_w, the resized first-stage logits)."""
        lib, st, dev, ws = N.load(), N.stream(), preds.device, self.window_size
        B, Nw = preds.shape[0], int(window_preds.shape[0])
        h_preds = torch.empty(B, 1, ws * hH, ws * hW, dtype=torch.float32, device=dev)
        N.check(lib.ucod_window_scatter(N.ptr(window_preds) if Nw else None, N.ptr(cd) if Nw else None, N.ptr(l_idx) if Nw else None,
                                        N.ptr(h_preds), Nw, B, hH, hW, ws, st), "ucod_window_scatter")
        h2, w2 = h_preds.shape[-2:]
        l1 = ops.bilinear_resize(preds, h2, w2)
        outputs = torch.empty_like(h_preds)
        ge_w = torch.empty_like(h_preds)
        wsb = torch.empty(lib.ucod_gated_ensemble_workspace_bytes(B, h2, w2), dtype=torch.uint8, device=dev)
        N.check(lib.ucod_gated_ensemble(N.ptr(l1), N.ptr(h_preds), N.ptr(P["f0w"]), N.ptr(P["f0b"]), N.ptr(P["f2w"]), P["f2b"], N.ptr(outputs),
                                        N.ptr(ge_w), N.ptr(wsb), B, h2, w2, st), "ucod_gated_ensemble")
        return outputs, h_preds, ge_w, l1

    def _select(self, input_features, h_inputs, preds):
        """EntropySelector (ASR.py:41-51) on the first-stage logits -> (input_features, h_inputs, preds as contiguous f32, mask, entropy, sel, coords_list)."""
        if not input_features.is_cuda:
            raise RuntimeError("SparseRefiner runs on the HIP path only: move the module and its inputs to 'cuda'")
        lib = N.load()
        dev = input_features.device
        ws = self.window_size
        input_features = input_features.float().contiguous()
        h_inputs = h_inputs.float().contiguous()
        preds = preds.float().contiguous()
        B, C, H, W = input_features.shape
        ph, pw = preds.shape[-2:]
        st = N.stream()
        # the "already a probability?" heuristic is a data-dependent branch -> one host sync
        lo, hi = torch.aminmax(preds)
        use_sigmoid = 0 if (lo.item() >= 0 and hi.item() <= 1) else 1
        entropy = torch.empty_like(preds)
        scores = torch.empty(B, ws, ws, dtype=torch.float32, device=dev)
        N.check(lib.ucod_entropy_scores(N.ptr(preds), use_sigmoid, N.ptr(entropy), N.ptr(scores), B, ph, pw, ws, st), "ucod_entropy_scores")
        mask = (scores > self.threshold).view(B, 1, ws, ws)
        mask_h = mask.view(B, ws * ws).cpu().numpy()
        sel = np.argwhere(mask_h)                                             # rows (b, j) in (b-major, raster) order
        coords_np = np.stack([sel[:, 1] // ws, sel[:, 1] % ws], 1).astype(np.int64) if len(sel) else np.zeros((0, 2), np.int64)
        coords_list = torch.from_numpy(coords_np).to(dev)
        return input_features, h_inputs, preds, mask, entropy, sel, coords_list

    def _window_indices(self, sel, coords_list, dev):
        """(image index, flat window index, coords) of the selected windows as int32 device tensors"""
        ws = self.window_size
        if len(sel) == 0:
            return (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, 2, dtype=torch.int32, device=dev))
        l_idx = torch.from_numpy(sel[:, 0].astype(np.int32)).to(dev)
        h_idx = torch.from_numpy((sel[:, 0] * ws * ws + sel[:, 1]).astype(np.int32)).to(dev)
        return l_idx, h_idx, coords_list.to(torch.int32).contiguous()

    def loss_and_grads(self, input_features, h_inputs, preds, h_targets, grads, outputs_cotangent=None):
        """The training forward and the backward with no torch autograd, into caller-owned gradient buffers -> (outputs, ex_loss, opt), as ``forward`` returns them.
        ``grads``: 18 contiguous f32 device buffers of the ``HRE.CSF`` parameters' sizes in ``named_parameters`` order, or 22 with those of
        ``GE.fuser.{0.weight, 0.bias, 2.weight, 2.bias}`` behind them -- the order of ``_RefinerFunction``'s inputs.  The gradient is that of ``ex_loss``; with
        ``outputs_cotangent(outputs, opt) -> G`` (d loss / d ``outputs``, [B,1,h,w]) it is that of ex_loss + loss(outputs): the fuser gradients need the 22 buffers,
        and the CSF chain runs ONCE on the sum of the two window cotangents, exactly as ``_RefinerFunction.backward`` does.  Nothing to differentiate -- no selected
        window (or no ``h_targets``) and no ``outputs_cotangent`` -- : ex_loss is 0 and no buffer is touched.  ``opt['grads_written']`` = (CSF, fuser) says which
        of the two groups of buffers this call wrote.  ``preds`` and the features carry no gradient (they come from a frozen first stage)."""
        if len(grads) not in (18, 22):
            raise ValueError(f"loss_and_grads: grads must have 18 or 22 entries, got {len(grads)}")
        input_features, h_inputs, preds, mask, entropy, sel, coords_list = self._select(input_features, h_inputs, preds)
        dev = input_features.device
        P = self._prepare(dev)
        Nw = len(sel)
        hH, hW = h_inputs.shape[-2:]
        l_idx, h_idx, cd = self._window_indices(sel, coords_list, dev)
        saved, aux, loss, tsel, ious = None, None, None, None, None
        if Nw > 0:
            saved = {}
            window_preds = self._csf(P, input_features, h_inputs, l_idx, h_idx, hH, hW, save=saved)
            if h_targets is not None:
                loss, tsel, ious, aux = self._window_loss(window_preds, preds, h_targets, h_idx)
        else:
            window_preds = torch.zeros(0, 1, hH, hW, dtype=torch.float32, device=dev)
        outputs, h_preds, ge_w, l1 = self._ensemble(P, window_preds, cd, l_idx, preds, hH, hW)
        opt = {"mask": mask, "entropy": entropy, "h_preds": h_preds, "window_preds": window_preds, "GE_w": ge_w, "preds": preds,
               "coords_list": coords_list, "h_targets": h_targets, "grads_written": (False, False)}
        if loss is not None:
            opt["window_targets"], opt["window_ious"] = tsel, ious
        G = None if outputs_cotangent is None else outputs_cotangent(outputs, opt)
        dl2 = None
        if G is not None:
            if len(grads) != 22:
                raise ValueError("loss_and_grads: an outputs_cotangent needs the 22 gradient buffers (the four GE.fuser ones behind the 18)")
            dl2, d_a, d_c, d_d, d_b = ops.gated_ensemble_bwd(l1, h_preds, ge_w, P["f0w"], P["f0b"], P["f2w"], G.detach().to(dev, torch.float32).contiguous())
            for dst, src in zip(grads[18:], (d_a, d_c, d_d, d_b)):
                dst.view(-1).copy_(src.view(-1))
        csf = Nw > 0 and (dl2 is not None or aux is not None)
        if csf:
            one = torch.ones(1, dtype=torch.float32, device=dev) if aux is not None else None
            self._csf_backward(saved, aux, one, dwin=None if dl2 is None else (dl2, cd, l_idx), out=list(grads[:18]))
        opt["grads_written"] = (csf, G is not None)
        return outputs, (loss if loss is not None else 0), opt

    def forward(self, input_features, h_inputs, preds, h_targets=None):
        input_features, h_inputs, preds, mask, entropy, sel, coords_list = self._select(input_features, h_inputs, preds)
        dev = input_features.device
        P = self._prepare(dev)
        ws = self.window_size
        B = input_features.shape[0]
        Nw = len(sel)
        hH, hW = h_inputs.shape[-2:]
        csf_params = [p for _, p in self.HRE.CSF.named_parameters()]
        # the window branch under autograd: only where a loss exists and somebody asks for its gradient; everything else is the plain forward
        graph = (self.training and torch.is_grad_enabled() and Nw > 0 and h_targets is not None and any(p.requires_grad for p in csf_params))
        fuser_params = [self.GE.fuser[0].weight, self.GE.fuser[0].bias, self.GE.fuser[2].weight, self.GE.fuser[2].bias]
        # `outputs` under autograd as well: opt-in (train_outputs), and only where somebody asks for a gradient
        graph_out = (self.train_outputs and self.training and torch.is_grad_enabled() and any(p.requires_grad for p in csf_params + fuser_params))
        trained, whole = None, None
        if Nw > 0:
            l_idx = torch.from_numpy(sel[:, 0].astype(np.int32)).to(dev)
            h_idx = torch.from_numpy((sel[:, 0] * ws * ws + sel[:, 1]).astype(np.int32)).to(dev)
            cd = coords_list.to(torch.int32).contiguous()
            if graph_out:
                window_preds = None
            elif graph:
                trained = _WindowBranchFunction.apply(self, dict(csf=(P, input_features.detach(), h_inputs.detach(), l_idx, h_idx, hH, hW),
                                                                 loss=(preds.detach(), h_targets, h_idx)), *csf_params)
                window_preds = trained[1]
            else:
                window_preds = self._csf(P, input_features, h_inputs, l_idx, h_idx, hH, hW)
        else:
            l_idx = torch.zeros(0, dtype=torch.int32, device=dev)
            h_idx = torch.zeros(0, dtype=torch.int32, device=dev)
            window_preds = torch.zeros(0, 1, hH, hW, dtype=torch.float32, device=dev)
            cd = torch.zeros(0, 2, dtype=torch.int32, device=dev)
        if graph_out:
            # the activations are saved exactly where the window branch alone would save them: the forward is bit for bit the one with train_outputs off
            whole = _RefinerFunction.apply(self, dict(P=P, Nw=Nw, save=any(p.requires_grad for p in csf_params), no_windows=window_preds,
                                                      csf=(P, input_features.detach(), h_inputs.detach(), l_idx, h_idx, hH, hW),
                                                      loss=None if h_targets is None else (preds.detach(), h_targets, h_idx),
                                                      ensemble=(cd, l_idx, preds.detach(), hH, hW)), *csf_params, *fuser_params)
            window_preds = whole[2]
            if whole[1] is not None:
                trained = (whole[1], None, whole[5], whole[6])
        if whole is not None:
            outputs, h_preds, ge_w = whole[0], whole[3], whole[4]
        else:
            outputs, h_preds, ge_w, _ = self._ensemble(P, window_preds, cd, l_idx, preds, hH, hW)
        opt = {"mask": mask, "entropy": entropy, "h_preds": h_preds, "window_preds": window_preds, "GE_w": ge_w, "preds": preds,
               "coords_list": coords_list, "h_targets": h_targets}
        if trained is not None:
            ex_loss, opt["window_targets"], opt["window_ious"] = trained[0], trained[2], trained[3]
        else:
            ex_loss, opt = self.cal_ex_loss(opt, h_idx)
        return outputs, ex_loss, opt
