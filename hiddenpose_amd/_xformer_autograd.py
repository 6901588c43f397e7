"""Training paths of the transformer heads (NlosPoseSformer, TimeSformer, TokenPose-L): one torch.autograd.Function per
head whose forward runs the no-graph forward's kernels in the same order (so its output is bit-identical) while keeping
what the backward needs, and whose backward is a chain of HIP kernels (include/hiddenpose_hip.h, "NlosPoseSformer
backward").  PyTorch only allocates, zero-fills and copies.

The op-level helpers (layernorm_backward, linear_backward, geglu_backward, gelu_backward) are written for any row-major
token matrix; the sublayer helpers (pre-norm attention, GEGLU / GELU feed-forward) serve TimeSformer and TokenPose-L.

Dropout.  Every nn.Dropout of the reference modules is a *site*: its position in the reference's forward
order.  A Function takes `drop`, None or (seed, step, p, p) with the module's two probabilities; a sublayer helper takes
`drop`, None or (seed, step, p) for its own sites, and `site`, the index of its first one.  The mask of a site is a pure
function of (seed, (step << 20) | site, flat element index, p) (hp_dropout_forward), so the backward regenerates it and no
mask is stored.  A site with p == 0 keeps its index and launches nothing; with drop None the code below is the code that ran
before dropout was built, launch for launch."""
from __future__ import annotations

import torch

from . import _lib


def _st(t):
    return _lib.current_stream_handle(t.device)


def _ws(nbytes, dev):
    return torch.empty(max(1, (int(nbytes) + 3) // 4), dtype=torch.float32, device=dev)


_M64 = (1 << 64) - 1


def dropout_stream(step, site):
    """The Philox stream of dropout site `site` at training step `step`."""
    return ((int(step) << 20) | int(site)) & _M64


def active_dropout(m, p0, p1):
    """The `drop` tuple (seed, step, p0, p1) of a module's forward, or None: dropout is active when the module is in training
    mode, one of its two probabilities is > 0 and its dropout_seed is an int."""
    seed = m.dropout_seed
    if not m.training or not (p0 > 0 or p1 > 0) or not isinstance(seed, int) or isinstance(seed, bool):
        return None
    return (seed, int(m.dropout_step), float(p0), float(p1))


def _dropping(drop):
    return drop is not None and drop[2] > 0


def dropout(x, drop, site, addend=None, out=None):
    """out = dropout(x) (+ addend) over the whole contiguous tensor x (hp_dropout_forward); out defaults to x (in place) and
    may also be addend.  drop = (seed, step, p)."""
    seed, step, p = drop
    out = x if out is None else out
    _lib.check(_lib.lib().hp_dropout_forward(x.data_ptr(), _lib.ptr(addend), out.data_ptr(), x.numel(), 0, float(p), int(seed) & _M64,
                                             dropout_stream(step, site), _st(x)), "hp_dropout_forward")
    return out


def dropout_mask(n, first, p, seed, stream, device):
    """(n,) uint8 keep mask of elements first .. first + n - 1 (hp_dropout_mask): for tests and debugging."""
    m = torch.empty(n, dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().hp_dropout_mask(m.data_ptr(), n, first, float(p), int(seed) & _M64, int(stream) & _M64,
                                          _lib.current_stream_handle(device)), "hp_dropout_mask")
    return m


def linear(x2d, weight, bias=None, precision=0, addend=None):
    """y = x @ W^T + b (+ addend) into a fresh tensor."""
    M, K = x2d.shape
    N = weight.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x2d.device)
    _lib.check(_lib.lib().hp_linear_forward(x2d.data_ptr(), weight.data_ptr(), _lib.ptr(bias), _lib.ptr(addend), y.data_ptr(), M, K, N,
                                            precision, _st(x2d)), "hp_linear_forward")
    return y


def linear_backward(x2d, dy, weight, precision=0, with_bias=True, need_dx=True):
    """(dx, dW, db) of y = x W^T + b; dx is None unless need_dx, db None unless with_bias."""
    L = _lib.lib()
    M, K = x2d.shape
    N = weight.shape[0]
    dev = x2d.device
    dx = None
    if need_dx:
        dx = torch.empty(M, K, dtype=torch.float32, device=dev)
        nb = L.hp_linear_backward_data_workspace_bytes(K, N)
        ws = _ws(nb, dev)
        _lib.check(L.hp_linear_backward_data(dy.data_ptr(), weight.data_ptr(), None, dx.data_ptr(), M, K, N, precision, ws.data_ptr(), nb,
                                             _st(dy)), "hp_linear_backward_data")
    dw = torch.empty(N, K, dtype=torch.float32, device=dev)
    db = torch.empty(N, dtype=torch.float32, device=dev) if with_bias else None
    nb = L.hp_linear_backward_weight_workspace_bytes(M, K, N)
    ws = _ws(nb, dev)
    _lib.check(L.hp_linear_backward_weight(x2d.data_ptr(), dy.data_ptr(), dw.data_ptr(), _lib.ptr(db), M, K, N, precision, ws.data_ptr(),
                                           nb, _st(dy)), "hp_linear_backward_weight")
    return dx, dw, db


def layernorm_backward(x, dy, dx, norm_weight, eps, rows, dim, rows_per_batch=0, batch_stride_rows=0):
    """dx += LN^T(dy) (rows addressed as the forward addresses them); returns (dgamma, dbeta)."""
    L = _lib.lib()
    dev = x.device
    dg = torch.empty(dim, dtype=torch.float32, device=dev)
    db = torch.empty(dim, dtype=torch.float32, device=dev)
    nb = L.hp_layernorm_backward_workspace_bytes(rows, dim)
    ws = _ws(nb, dev)
    _lib.check(L.hp_layernorm_backward(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, dim,
                                       norm_weight.data_ptr(), eps, rows_per_batch, batch_stride_rows, ws.data_ptr(), nb, _st(x)),
               "hp_layernorm_backward")
    return dg, db


def geglu_backward(u, dg, drop=None, site=0):
    """du of the GEGLU; with `drop` dg first goes through dropout site `site`'s mask (hp_geglu_backward_dropout)."""
    rows, hid = dg.shape
    du = torch.empty(rows, 2 * hid, dtype=torch.float32, device=u.device)
    if _dropping(drop):
        seed, step, p = drop
        _lib.check(_lib.lib().hp_geglu_backward_dropout(u.data_ptr(), dg.data_ptr(), du.data_ptr(), rows, hid, float(p), int(seed) & _M64,
                                                        dropout_stream(step, site), _st(u)), "hp_geglu_backward_dropout")
        return du
    _lib.check(_lib.lib().hp_geglu_backward(u.data_ptr(), dg.data_ptr(), du.data_ptr(), rows, hid, _st(u)), "hp_geglu_backward")
    return du


def attention_backward(q, k, k0, v, out, dout, lse, b, heads, dh, ntok, nj, n, frames, precision=0):
    """(dQ, dK, dK0, dV).  precision 0: the exact-fp32 backward; 1 (bf16) / 4 (fp16): the patch queries' part on the 16-bit
    matrix cores (hp_sformer_attention_backward_p; dim_head 32 or 64), the joint queries' part exact fp32."""
    L = _lib.lib()
    dq, dk, dk0, dv = (torch.empty_like(q) for _ in range(4))
    if precision == 0:
        nb = L.hp_sformer_attention_backward_workspace_bytes(b, heads, dh, ntok, nj, frames)
        ws = _ws(nb, q.device)
        _lib.check(L.hp_sformer_attention_backward(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(),
                                                   lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(), dv.data_ptr(), b, heads, dh, ntok,
                                                   nj, n, frames, ws.data_ptr(), nb, _st(q)), "hp_sformer_attention_backward")
        return dq, dk, dk0, dv
    nb = L.hp_sformer_attention_backward_p_workspace_bytes(b, heads, dh, ntok, nj, frames, precision)
    ws = _ws(nb, q.device)
    _lib.check(L.hp_sformer_attention_backward_p(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(),
                                                 lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(), dv.data_ptr(), b, heads, dh, ntok,
                                                 nj, n, frames, precision, ws.data_ptr(), nb, _st(q)), "hp_sformer_attention_backward_p")
    return dq, dk, dk0, dv


def _layer_params(layer):
    _time_attn, spatial, ff = layer
    a = spatial.fn
    return [spatial.norm.weight, spatial.norm.bias, a.to_qkv.weight, a.to_out[0].weight, a.to_out[0].bias, ff.norm.weight,
            ff.norm.bias, ff.fn.net[0].weight, ff.fn.net[0].bias, ff.fn.net[3].weight, ff.fn.net[3].bias]


PER_LAYER = 11


def trainable_params(m):
    """The parameters the forward reads, in the order SformerFunction takes them (the time-attention weights, allocated
    but never run, are not among them: their .grad stays None)."""
    ps = [m.to_patch_embedding.weight, m.to_patch_embedding.bias, m.joints_token]
    for layer in m.layers:
        ps += _layer_params(layer)
    ps += [m.to_out[0].weight, m.to_out[0].bias, m.to_out[1].weight, m.to_out[1].bias]
    return ps


class SformerFunction(torch.autograd.Function):
    """video (b, f, c, H, W), module, three precisions, drop, *trainable_params(m) -> (b, num_joints, 4, out_dim / 4).
    drop: None or (seed, step, attn_dropout, ff_dropout); sites per layer: 2 i the spatial attention's to_out, 2 i + 1 the
    feed-forward's hidden activation (the time attention is never run and has no site)."""

    @staticmethod
    def forward(ctx, video, m, prec, aprec, bprec, drop, *params):
        """prec, aprec, bprec: HP_PRECISION_* of the Linear layers, the patch attention's forward and the attention backward."""
        d_attn = None if drop is None else (drop[0], drop[1], drop[2])
        d_ff = None if drop is None else (drop[0], drop[1], drop[3])
        L = _lib.lib()
        b, f, c, H, W = video.shape
        ps, nj, heads, dh = m.patch_size, m.num_joints, m.heads, m.dim_head
        hp, wp = H // ps, W // ps
        n = hp * wp
        ntok = nj + f * n
        dim = m.joints_token.shape[-1]
        dev = video.device
        st = _st(video)
        pe_w, pe_b, jtok = params[:3]
        tokens = torch.empty(b * f * n, ps * ps * c, dtype=torch.float32, device=dev)
        _lib.check(L.hp_sformer_patchify(video.data_ptr(), tokens.data_ptr(), b, f, c, H, W, ps, st), "hp_sformer_patchify")
        emb = linear(tokens, pe_w, pe_b)
        x = torch.empty(b, ntok, dim, dtype=torch.float32, device=dev)
        x[:, :nj] = jtok
        x[:, nj:] = emb.view(b, f * n, dim)
        sin_t, cos_t = m.image_rot_emb.tables(hp, wp, dev)
        rot_dim = sin_t.shape[-1]
        rows = b * ntok
        inner = heads * dh
        aws = torch.empty(int(L.hp_sformer_attention_workspace_bytes(b, heads, dh)) // 4, dtype=torch.float32, device=dev)
        saved = []
        for i, layer in enumerate(m.layers):
            ln1_w, ln1_b, wqkv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2 = params[3 + PER_LAYER * i: 3 + PER_LAYER * (i + 1)]
            scale, eps1, eps2 = layer[1].fn.scale, layer[1].norm.eps, layer[2].norm.eps
            h1 = torch.empty_like(x)
            _lib.check(L.hp_layernorm_forward(x.data_ptr(), h1.data_ptr(), rows, dim, ln1_w.data_ptr(), ln1_b.data_ptr(), eps1, 0, 0, st),
                       "hp_layernorm_forward")
            qkv = linear(h1.view(rows, dim), wqkv, None, prec)
            q = torch.empty(b, heads, ntok, dh, dtype=torch.float32, device=dev)
            k, k0, v = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
            _lib.check(L.hp_sformer_qkv_prepare(qkv.data_ptr(), q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), b, ntok, heads, dh,
                                                nj, n, scale, sin_t.data_ptr(), cos_t.data_ptr(), rot_dim, st), "hp_sformer_qkv_prepare")
            del qkv
            att = torch.empty(b, ntok, inner, dtype=torch.float32, device=dev)
            lse = None
            if aprec == 0:
                lse = torch.empty(b, heads, ntok, dtype=torch.float32, device=dev)
                _lib.check(L.hp_sformer_attention_lse(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), att.data_ptr(), lse.data_ptr(),
                                                      b, heads, dh, ntok, nj, n, f, aws.data_ptr(), st), "hp_sformer_attention_lse")
            elif bprec != 0:   # a 16-bit backward recomputes P from the 16-bit forward's own lse
                lse = torch.empty(b, heads, ntok, dtype=torch.float32, device=dev)
                _lib.check(L.hp_sformer_attention_lse_p(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), att.data_ptr(), lse.data_ptr(),
                                                        b, heads, dh, ntok, nj, n, f, aprec, aws.data_ptr(), st), "hp_sformer_attention_lse_p")
            else:
                _lib.check(L.hp_sformer_attention(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), att.data_ptr(), b, heads, dh,
                                                  ntok, nj, n, f, aprec, aws.data_ptr(), st), "hp_sformer_attention")
            if _dropping(d_attn):
                x1 = linear(att.view(rows, inner), wo, bo, prec)
                x1 = dropout(x1, d_attn, 2 * i, addend=x).view(b, ntok, dim)
            else:
                x1 = linear(att.view(rows, inner), wo, bo, prec, addend=x.view(rows, dim)).view(b, ntok, dim)
            h2 = torch.empty_like(x)
            _lib.check(L.hp_layernorm_forward(x1.data_ptr(), h2.data_ptr(), rows, dim, ln2_w.data_ptr(), ln2_b.data_ptr(), eps2, 0, 0, st),
                       "hp_layernorm_forward")
            hid = w2.shape[1]
            g = torch.empty(rows, hid, dtype=torch.float32, device=dev)
            if hid % 64 == 0 and w1.shape[0] == 2 * hid:   # as _xformer.geglu_ff: the GEGLU in the GEMM's epilogue
                _lib.check(L.hp_linear_geglu_forward(h2.data_ptr(), w1.data_ptr(), _lib.ptr(b1), g.data_ptr(), rows, dim, 2 * hid, prec, st),
                           "hp_linear_geglu_forward")
            else:
                u = linear(h2.view(rows, dim), w1, b1, prec)
                _lib.check(L.hp_geglu_forward(u.data_ptr(), g.data_ptr(), rows, hid, st), "hp_geglu_forward")
                del u
            if _dropping(d_ff):
                dropout(g, d_ff, 2 * i + 1)     # the saved activation is the dropped one: what W2's gradient needs
            x2 = linear(g, w2, b2, prec, addend=x1.view(rows, dim)).view(b, ntok, dim)
            saved += [x, h1, q, k, k0, v, att, lse, x1, h2, g]
            x = x2
        jt = torch.empty(b * nj, dim, dtype=torch.float32, device=dev)
        _lib.check(L.hp_layernorm_forward(x.data_ptr(), jt.data_ptr(), b * nj, dim, params[-4].data_ptr(), params[-3].data_ptr(),
                                          m.to_out[0].eps, nj, ntok, st), "hp_layernorm_forward")
        out = linear(jt, params[-2], params[-1])
        ctx.geom = (b, f, c, H, W, ps, nj, heads, dh, n, ntok, dim, rot_dim, prec, aprec, bprec)
        ctx.consts = [(layer[1].fn.scale, layer[1].norm.eps, layer[2].norm.eps) for layer in m.layers] + [m.to_out[0].eps]
        ctx.depth = len(m.layers)
        ctx.drops = (d_attn, d_ff)
        ctx.nsaved = len(saved)
        ctx.save_for_backward(*saved, tokens, x, jt, sin_t, cos_t, *params)
        return out.view(b, nj, 4, -1)

    @staticmethod
    def backward(ctx, dout):
        b, f, c, H, W, ps, nj, heads, dh, n, ntok, dim, rot_dim, prec, aprec, bprec = ctx.geom
        if aprec != 0 and bprec == 0:
            raise _lib.HiddenPoseHipError("NlosPoseSformer backward: training needs attention_precision = \"fp32\" (the bf16 / fp16 "
                                          "patch attention has no fp32 backward) or attention_backward_precision = \"bf16\" / "
                                          "\"fp16\"")
        L = _lib.lib()
        allt = ctx.saved_tensors
        saved, (tokens, xl, jt, sin_t, cos_t), params = allt[:ctx.nsaved], allt[ctx.nsaved:ctx.nsaved + 5], allt[ctx.nsaved + 5:]
        dev = dout.device
        st = _st(dout)
        rows, inner = b * ntok, heads * dh
        d_attn, d_ff = ctx.drops
        grads = [None] * len(params)
        dout = dout.contiguous().view(b * nj, -1)
        # head: LN(x[:, :nj]) -> Linear
        djt, grads[-2], grads[-1] = linear_backward(jt, dout, params[-2])
        dx = torch.zeros(b, ntok, dim, dtype=torch.float32, device=dev)
        grads[-4], grads[-3] = layernorm_backward(xl, djt, dx, params[-4], ctx.consts[-1], b * nj, dim, nj, ntok)
        for i in reversed(range(ctx.depth)):
            x, h1, q, k, k0, v, att, lse, x1, h2, g = saved[11 * i: 11 * (i + 1)]
            base = 3 + PER_LAYER * i
            ln1_w, ln1_b, wqkv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2 = params[base: base + PER_LAYER]
            scale, eps1, eps2 = ctx.consts[i]
            # feed-forward: x2 = x1 + W2 (a * gelu(t)) + b2, [a | t] = u = W1 LN2(x1) + b1
            d2 = dx.view(rows, dim)
            dg, grads[base + 9], grads[base + 10] = linear_backward(g, d2, w2, prec)
            u = linear(h2.view(rows, dim), w1, b1, prec)
            du = geglu_backward(u, dg, d_ff, 2 * i + 1)
            del u, dg
            dh2, grads[base + 7], grads[base + 8] = linear_backward(h2.view(rows, dim), du, w1, prec)
            del du
            grads[base + 5], grads[base + 6] = layernorm_backward(x1, dh2, dx, ln2_w, eps2, rows, dim)   # dx := dx1
            del dh2
            # attention: x1 = x + Wo att + bo
            dlin = dropout(d2, d_attn, 2 * i, out=torch.empty_like(d2)) if _dropping(d_attn) else d2
            datt, grads[base + 3], grads[base + 4] = linear_backward(att.view(rows, inner), dlin, wo, prec)
            del dlin
            dq, dk, dk0, dv = attention_backward(q, k, k0, v, att, datt, lse, b, heads, dh, ntok, nj, n, f, bprec)
            del datt
            dqkv = torch.empty(rows, 3 * inner, dtype=torch.float32, device=dev)
            _lib.check(L.hp_sformer_qkv_prepare_backward(dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(), dv.data_ptr(), dqkv.data_ptr(), b,
                                                         ntok, heads, dh, nj, n, scale, sin_t.data_ptr(), cos_t.data_ptr(), rot_dim, st),
                       "hp_sformer_qkv_prepare_backward")
            del dq, dk, dk0, dv
            dh1, grads[base + 2], _ = linear_backward(h1.view(rows, dim), dqkv, wqkv, prec, with_bias=False)
            del dqkv
            grads[base], grads[base + 1] = layernorm_backward(x, dh1, dx, ln1_w, eps1, rows, dim)   # dx := dx of the layer input
            del dh1
        # token assembly: joints_token is shared by the batch; the patch rows go back through the embedding and patchify
        djtok = torch.empty(1, nj, dim, dtype=torch.float32, device=dev)
        _lib.check(L.hp_sformer_joint_token_backward(dx.data_ptr(), djtok.data_ptr(), b, nj, ntok, dim, st),
                   "hp_sformer_joint_token_backward")
        grads[2] = djtok
        demb = dx[:, nj:].contiguous().view(b * f * n, dim)
        need_video = ctx.needs_input_grad[0]
        dtok, grads[0], grads[1] = linear_backward(tokens, demb, params[0], need_dx=need_video)
        dvideo = None
        if need_video:
            dvideo = torch.empty(b, f, c, H, W, dtype=torch.float32, device=dev)
            _lib.check(L.hp_sformer_unpatchify(dtok.data_ptr(), dvideo.data_ptr(), b, f, c, H, W, ps, st), "hp_sformer_unpatchify")
        return (dvideo, None, None, None, None, None, *grads)


# ---------------------------------------------------------------------------------------------------------------------
# TimeSformer and TokenPose-L training paths.  The sublayer helpers below take the layer input x (b, ntok, dim) and return a
# fresh x + sublayer(x) together with what their backward needs; their backward ADDS the sublayer's input gradient into dx
# (the residual stream's gradient, which already holds d(x + sublayer(x))) and returns the parameter gradients.

FP32_BACKWARD_AFTER_16BIT_FORWARD = ("{} backward: training needs attention_precision = \"fp32\" (the bf16 / fp16 patch attention "
                                     "has no fp32 backward) or attention_backward_precision = \"bf16\" / \"fp16\"")


def gelu_backward(u, dy, drop=None, site=0):
    """du = dy * gelu'(u) (hp_gelu_backward, written over dy); with `drop` dy first goes through dropout site `site`'s mask
    (hp_gelu_backward_dropout)."""
    if _dropping(drop):
        seed, step, p = drop
        _lib.check(_lib.lib().hp_gelu_backward_dropout(u.data_ptr(), dy.data_ptr(), dy.data_ptr(), u.numel(), float(p), int(seed) & _M64,
                                                       dropout_stream(step, site), _st(u)), "hp_gelu_backward_dropout")
        return dy
    _lib.check(_lib.lib().hp_gelu_backward(u.data_ptr(), dy.data_ptr(), dy.data_ptr(), u.numel(), _st(u)), "hp_gelu_backward")
    return dy


def attention_backward_masked(q, k, k0, v, out, dout, lse, b, heads, dh, ntok, nj, n, groups, key_mask, mask_patch_queries,
                              grouped=False, precision=0):
    """(dQ, dK, dK0, dV) of the fp32 attention with a key mask (hp_sformer_attention_backward_masked, or its grouped form
    for n <= 64 tokens per group at dim_head 16 / 24 / 32; the two are bit-equal).  precision 1 (bf16) / 4 (fp16):
    hp_sformer_attention_backward_masked_p (the patch queries on the 16-bit matrix cores; not grouped, mask_patch_queries False)."""
    L = _lib.lib()
    dq, dk, dk0, dv = (torch.empty_like(q) for _ in range(4))
    if precision != 0:
        assert not grouped, "the grouped attention backward is exact fp32"
        nb = L.hp_sformer_attention_backward_masked_p_workspace_bytes(b, heads, dh, ntok, nj, groups, precision)
        ws = _ws(nb, q.device)
        _lib.check(L.hp_sformer_attention_backward_masked_p(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(),
                                                            dout.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(),
                                                            dv.data_ptr(), b, heads, dh, ntok, nj, n, groups, key_mask.data_ptr(),
                                                            int(bool(mask_patch_queries)), precision, ws.data_ptr(), nb, _st(q)),
                   "hp_sformer_attention_backward_masked_p")
        return dq, dk, dk0, dv
    name = "hp_sformer_attention_backward_grouped_masked" if grouped else "hp_sformer_attention_backward_masked"
    nb = getattr(L, name + "_workspace_bytes")(b, heads, dh, ntok, nj, groups)
    ws = _ws(nb, q.device)
    _lib.check(getattr(L, name)(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(), dv.data_ptr(), b, heads, dh, ntok, nj, n, groups,
                                key_mask.data_ptr(), int(bool(mask_patch_queries)), ws.data_ptr(), nb, _st(q)), name)
    return dq, dk, dk0, dv


def attention_backward_grouped(q, k, k0, v, out, dout, lse, b, heads, dh, ntok, nj, n, groups):
    """attention_backward for short groups (hp_sformer_attention_backward_grouped): n <= 64 tokens per group."""
    L = _lib.lib()
    dq, dk, dk0, dv = (torch.empty_like(q) for _ in range(4))
    nb = L.hp_sformer_attention_backward_grouped_workspace_bytes(b, heads, dh, ntok, nj, groups)
    ws = _ws(nb, q.device)
    _lib.check(L.hp_sformer_attention_backward_grouped(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(),
                                                       dout.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(),
                                                       dv.data_ptr(), b, heads, dh, ntok, nj, n, groups, ws.data_ptr(), nb, _st(q)),
               "hp_sformer_attention_backward_grouped")
    return dq, dk, dk0, dv


# time attention's backward: "grouped" (hp_sformer_attention_backward_grouped) or "generic" (hp_sformer_attention_backward);
# DESIGN 4.4.2 records the A/B that chose it
TIME_ATTENTION_BACKWARD = "grouped"
GROUPED_DIM_HEADS = (16, 24, 32)   # the grouped entry is not built for dim_head 64: that width takes the generic one


def time_perm(t, f, n):
    """[cls | (f, n) frame-major rows] -> [cls | (n, f)]: the time attention's groups become contiguous (a copy)."""
    b, ntok, d = t.shape
    o = torch.empty_like(t)
    o[:, :1] = t[:, :1]
    o[:, 1:] = t[:, 1:].view(b, f, n, d).transpose(1, 2).reshape(b, n * f, d)
    return o


def time_unperm(t, f, n):
    """Inverse (and adjoint) of time_perm."""
    b, ntok, d = t.shape
    o = torch.empty_like(t)
    o[:, :1] = t[:, :1]
    o[:, 1:] = t[:, 1:].view(b, n, f, d).transpose(1, 2).reshape(b, f * n, d)
    return o


def token_shift_adjoint(g, frames, nj=1):
    """Adjoint of transformer._token_shift: the shifted thirds of the patch rows move back the opposite way (zeros at the
    clip ends); the other channels and the class rows pass through.  Plain slice copies."""
    b, ntok, d = g.shape
    n = (ntok - nj) // frames
    p = g[:, nj:].view(b, frames, n, d)
    out = g.clone()
    o = out[:, nj:].view(b, frames, n, d)
    c = d // 3
    o[:, :, :, :c] = 0
    o[:, 1:, :, :c] = p[:, :-1, :, :c]                      # forward: frame j took frame j + 1
    o[:, :, :, 2 * c:3 * c] = 0
    o[:, :-1, :, 2 * c:3 * c] = p[:, 1:, :, 2 * c:3 * c]    # forward: frame j took frame j - 1
    return out


def layernorm(x, w, b, eps, rows, dim, rows_per_batch=0, batch_stride_rows=0):
    y = torch.empty(rows, dim, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hp_layernorm_forward(x.data_ptr(), y.data_ptr(), rows, dim, w.data_ptr(), b.data_ptr(), eps, rows_per_batch,
                                               batch_stride_rows, _st(x)), "hp_layernorm_forward")
    return y


def prenorm_attention_forward(x, p, eps, scale, heads, dh, nj, n, groups, sin_t, cos_t, prec, pre=None, perm=None, unperm=None,
                              key_mask=None, mask_patch_queries=False, aprec=0, drop=None, site=0):
    """x + Wo unperm(Attn(perm(pre(LN(x))))) + bo for the token layout [nj | groups x n] of the permuted rows, as
    _xformer.attention runs it (with lse; key_mask (b, ntok) uint8 in the permuted rows' order selects
    hp_sformer_attention_lse_masked).  aprec: HP_PRECISION_* of the patch queries (0; 1 / 4 take the _p entries).
    p = (ln_w, ln_b, wqkv, wo, bo).  drop / site: dropout on to_out's output, before the residual.  -> (x1, saved)."""
    L = _lib.lib()
    ln_w, ln_b, wqkv, wo, bo = p
    b, ntok, dim = x.shape
    rows, inner = b * ntok, heads * dh
    dev = x.device
    st = _st(x)
    h = layernorm(x, ln_w, ln_b, eps, rows, dim).view(b, ntok, dim)
    if pre is not None:
        h = pre(h)
    if perm is not None:
        h = perm(h)
    qkv = linear(h.view(rows, dim), wqkv, None, prec)
    q = torch.empty(b, heads, ntok, dh, dtype=torch.float32, device=dev)
    k, k0, v = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    rot_dim = 0 if sin_t is None else sin_t.shape[-1]
    _lib.check(L.hp_sformer_qkv_prepare(qkv.data_ptr(), q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), b, ntok, heads, dh, nj, n,
                                        scale, _lib.ptr(sin_t), _lib.ptr(cos_t), rot_dim, st), "hp_sformer_qkv_prepare")
    del qkv
    att = torch.empty(b, ntok, inner, dtype=torch.float32, device=dev)
    lse = torch.empty(b, heads, ntok, dtype=torch.float32, device=dev)
    aws = _ws(L.hp_sformer_attention_workspace_bytes(b, heads, dh), dev)
    if key_mask is None and aprec == 0:
        _lib.check(L.hp_sformer_attention_lse(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), att.data_ptr(), lse.data_ptr(), b,
                                              heads, dh, ntok, nj, n, groups, aws.data_ptr(), st), "hp_sformer_attention_lse")
    elif key_mask is None:
        _lib.check(L.hp_sformer_attention_lse_p(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), att.data_ptr(), lse.data_ptr(), b,
                                                heads, dh, ntok, nj, n, groups, aprec, aws.data_ptr(), st), "hp_sformer_attention_lse_p")
    elif aprec != 0:
        _lib.check(L.hp_sformer_attention_lse_masked_p(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), att.data_ptr(),
                                                       lse.data_ptr(), b, heads, dh, ntok, nj, n, groups, key_mask.data_ptr(),
                                                       int(bool(mask_patch_queries)), aprec, aws.data_ptr(), st),
                   "hp_sformer_attention_lse_masked_p")
    else:
        _lib.check(L.hp_sformer_attention_lse_masked(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), att.data_ptr(),
                                                     lse.data_ptr(), b, heads, dh, ntok, nj, n, groups, key_mask.data_ptr(),
                                                     int(bool(mask_patch_queries)), aws.data_ptr(), st),
                   "hp_sformer_attention_lse_masked")
    ab = unperm(att) if unperm is not None else att
    if _dropping(drop):
        x1 = linear(ab.view(rows, inner), wo, bo, prec)
        x1 = dropout(x1, drop, site, addend=x).view(b, ntok, dim)
    else:
        x1 = linear(ab.view(rows, inner), wo, bo, prec, addend=x.view(rows, dim)).view(b, ntok, dim)
    return x1, (x, h, q, k, k0, v, att, lse, ab)


def prenorm_attention_backward(dx, saved, p, eps, scale, heads, dh, nj, n, groups, sin_t, cos_t, prec, pre_adjoint=None, perm=None,
                               unperm=None, grouped=False, key_mask=None, mask_patch_queries=False, bprec=0, drop=None, site=0):
    """dx += d(sublayer input); returns [d ln_w, d ln_b, d wqkv, d wo, d bo].  key_mask / mask_patch_queries: the forward's.
    bprec: HP_PRECISION_* of the patch queries' part of the attention backward (0; 1 / 4 only without `grouped`)."""
    L = _lib.lib()
    ln_w, _ln_b, wqkv, wo, _bo = p
    x, h, q, k, k0, v, att, lse, ab = saved
    b, ntok, dim = x.shape
    rows, inner = b * ntok, heads * dh
    dlin = dx.view(rows, dim)
    if _dropping(drop):
        dlin = dropout(dlin, drop, site, out=torch.empty_like(dlin))
    dab, dwo, dbo = linear_backward(ab.view(rows, inner), dlin, wo, prec)
    del dlin
    datt = perm(dab.view(b, ntok, inner)) if perm is not None else dab     # the adjoint of unperm is perm
    del dab
    if key_mask is None and bprec != 0:
        assert not grouped, "the grouped attention backward is exact fp32"
        dq, dk, dk0, dv = attention_backward(q, k, k0, v, att, datt, lse, b, heads, dh, ntok, nj, n, groups, bprec)
    elif key_mask is None:
        bwd = attention_backward_grouped if grouped else attention_backward
        dq, dk, dk0, dv = bwd(q, k, k0, v, att, datt, lse, b, heads, dh, ntok, nj, n, groups)
    else:
        dq, dk, dk0, dv = attention_backward_masked(q, k, k0, v, att, datt, lse, b, heads, dh, ntok, nj, n, groups, key_mask,
                                                    mask_patch_queries, grouped, bprec)
    del datt
    dqkv = torch.empty(rows, 3 * inner, dtype=torch.float32, device=x.device)
    rot_dim = 0 if sin_t is None else sin_t.shape[-1]
    _lib.check(L.hp_sformer_qkv_prepare_backward(dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(), dv.data_ptr(), dqkv.data_ptr(), b, ntok,
                                                 heads, dh, nj, n, scale, _lib.ptr(sin_t), _lib.ptr(cos_t), rot_dim, _st(dx)),
               "hp_sformer_qkv_prepare_backward")
    del dq, dk, dk0, dv
    dh_, dwqkv, _ = linear_backward(h.view(rows, dim), dqkv, wqkv, prec, with_bias=False)
    del dqkv
    dh_ = dh_.view(b, ntok, dim)
    if unperm is not None:
        dh_ = unperm(dh_)
    if pre_adjoint is not None:
        dh_ = pre_adjoint(dh_)
    dg, db = layernorm_backward(x, dh_, dx, ln_w, eps, rows, dim)
    return [dg, db, dwqkv, dwo, dbo]


def geglu_ff_forward(x, p, eps, prec, pre=None, drop=None, site=0):
    """x + W2 GEGLU(W1 pre(LN(x)) + b1) + b2 as _xformer.geglu_ff runs it.  p = (ln_w, ln_b, w1, b1, w2, b2).  drop / site:
    dropout on the hidden activation (in place: the saved g is the dropped one, what W2's gradient needs)."""
    L = _lib.lib()
    ln_w, ln_b, w1, b1, w2, b2 = p
    b, ntok, dim = x.shape
    rows = b * ntok
    st = _st(x)
    h = layernorm(x, ln_w, ln_b, eps, rows, dim).view(b, ntok, dim)
    if pre is not None:
        h = pre(h)
    hid = w2.shape[1]
    g = torch.empty(rows, hid, dtype=torch.float32, device=x.device)
    if hid % 64 == 0 and w1.shape[0] == 2 * hid:
        _lib.check(L.hp_linear_geglu_forward(h.data_ptr(), w1.data_ptr(), _lib.ptr(b1), g.data_ptr(), rows, dim, 2 * hid, prec, st),
                   "hp_linear_geglu_forward")
    else:
        u = linear(h.view(rows, dim), w1, b1, prec)
        _lib.check(L.hp_geglu_forward(u.data_ptr(), g.data_ptr(), rows, hid, st), "hp_geglu_forward")
        del u
    if _dropping(drop):
        dropout(g, drop, site)
    x1 = linear(g, w2, b2, prec, addend=x.view(rows, dim)).view(b, ntok, dim)
    return x1, (x, h, g)


def geglu_ff_backward(dx, saved, p, eps, prec, pre_adjoint=None, drop=None, site=0):
    """dx += d(sublayer input); returns [d ln_w, d ln_b, d w1, d b1, d w2, d b2].  u is recomputed from the saved input."""
    ln_w, _ln_b, w1, b1, w2, _b2 = p
    x, h, g = saved
    b, ntok, dim = x.shape
    rows = b * ntok
    dg, dw2, db2 = linear_backward(g, dx.view(rows, dim), w2, prec)
    u = linear(h.view(rows, dim), w1, b1, prec)
    du = geglu_backward(u, dg, drop, site)
    del u, dg
    dh_, dw1, db1 = linear_backward(h.view(rows, dim), du, w1, prec)
    del du
    dh_ = dh_.view(b, ntok, dim)
    if pre_adjoint is not None:
        dh_ = pre_adjoint(dh_)
    dg_, db_ = layernorm_backward(x, dh_, dx, ln_w, eps, rows, dim)
    return [dg_, db_, dw1, db1, dw2, db2]


def gelu_ff_forward(x, p, eps, prec, drop=None, site=0):
    """x + W2 gelu(W1 LN(x) + b1) + b2 as _xformer.gelu_ff runs it, with the GELU out of place (u is kept).  drop: dropout on the
    hidden activation (site `site`, in place: the saved a is the dropped one) and on W2's output (site + 1)."""
    ln_w, ln_b, w1, b1, w2, b2 = p
    b, ntok, dim = x.shape
    rows = b * ntok
    h = layernorm(x, ln_w, ln_b, eps, rows, dim)
    u = linear(h, w1, b1, prec)
    a = torch.empty_like(u)
    _lib.check(_lib.lib().hp_gelu_forward(u.data_ptr(), a.data_ptr(), u.numel(), _st(x)), "hp_gelu_forward")
    if _dropping(drop):
        dropout(a, drop, site)
        x1 = linear(a, w2, b2, prec)
        x1 = dropout(x1, drop, site + 1, addend=x).view(b, ntok, dim)
    else:
        x1 = linear(a, w2, b2, prec, addend=x.view(rows, dim)).view(b, ntok, dim)
    return x1, (x, h, u, a)


def gelu_ff_backward(dx, saved, p, eps, prec, drop=None, site=0):
    ln_w, _ln_b, w1, _b1, w2, _b2 = p
    x, h, u, a = saved
    b, ntok, dim = x.shape
    rows = b * ntok
    dlin = dx.view(rows, dim)
    if _dropping(drop):
        dlin = dropout(dlin, drop, site + 1, out=torch.empty_like(dlin))
    da, dw2, db2 = linear_backward(a, dlin, w2, prec)
    del dlin
    du = gelu_backward(u, da, drop, site)
    dh_, dw1, db1 = linear_backward(h, du, w1, prec)
    del du
    dg_, db_ = layernorm_backward(x, dh_, dx, ln_w, eps, rows, dim)
    return [dg_, db_, dw1, db1, dw2, db2]


def _joint_sum(dx, rows):
    """sum over the batch of dx[:, :rows] (hp_sformer_joint_token_backward) -> (1, rows, dim)."""
    b, ntok, dim = dx.shape
    out = torch.empty(1, rows, dim, dtype=torch.float32, device=dx.device)
    _lib.check(_lib.lib().hp_sformer_joint_token_backward(dx.data_ptr(), out.data_ptr(), b, rows, ntok, dim, _st(dx)),
               "hp_sformer_joint_token_backward")
    return out


def _unwrap(m, shift):
    return m.fn if shift else m


TS_PER_LAYER = 16


def timesformer_params(m):
    """The parameters TimeSformerFunction takes, in its order (every parameter of the module)."""
    ps = [m.to_patch_embedding.weight, m.to_patch_embedding.bias, m.cls_token]
    for time_attn, spatial, ff in m.layers:
        for sub in (time_attn, spatial):
            a = _unwrap(sub.fn, m.shift_tokens)
            ps += [sub.norm.weight, sub.norm.bias, a.to_qkv.weight, a.to_out[0].weight, a.to_out[0].bias]
        f = _unwrap(ff.fn, m.shift_tokens)
        ps += [ff.norm.weight, ff.norm.bias, f.net[0].weight, f.net[0].bias, f.net[3].weight, f.net[3].bias]
    return ps + [m.to_out[0].weight, m.to_out[0].bias, m.to_out[1].weight, m.to_out[1].bias]


class TimeSformerFunction(torch.autograd.Function):
    """video (b, f, c, H, W), module, precision, the frame mask's two (b, 1 + f n) uint8 key masks (natural [cls | f n] and
    time-permuted [cls | n f] order; both None without a frame mask; not differentiable), drop (None or (seed, step,
    attn_dropout, ff_dropout); sites per layer: 3 i the time attention's to_out, on the un-permuted rows, 3 i + 1 the spatial
    attention's, 3 i + 2 the feed-forward's hidden activation), *timesformer_params(m) -> (b, 72).
    Per layer: time attention (the rotary frame tables, on the transposed token grid: groups = hp*wp patch positions of f
    tokens; every query applies the mask), space attention (the axial tables, groups = f frames of hp*wp patches; only the
    class query applies it), GEGLU feed-forward; token shift before each when m.shift_tokens."""

    @staticmethod
    def forward(ctx, video, m, prec, aprec, bprec, mask_nat, mask_time, drop, *params):
        """aprec, bprec: HP_PRECISION_* of the spatial attention's patch queries, forward and backward (the time attention and
        the class queries are exact fp32)."""
        from .transformer import _token_shift

        L = _lib.lib()
        b, f, c, H, W = video.shape
        ps, heads, dh = m.patch_size, m.heads, m.dim_head
        hp, wp = H // ps, W // ps
        n = hp * wp
        ntok = 1 + f * n
        dim = m.cls_token.shape[-1]
        dev = video.device
        tokens = torch.empty(b * f * n, ps * ps * c, dtype=torch.float32, device=dev)
        _lib.check(L.hp_sformer_patchify(video.data_ptr(), tokens.data_ptr(), b, f, c, H, W, ps, _st(video)), "hp_sformer_patchify")
        emb = linear(tokens, params[0], params[1])
        x = torch.empty(b, ntok, dim, dtype=torch.float32, device=dev)
        x[:, :1] = params[2]
        x[:, 1:] = emb.view(b, f * n, dim)
        del emb
        sin_s, cos_s = m.image_rot_emb.tables(hp, wp, dev)
        sin_t, cos_t = m._frame_tables(f, dev)
        pre = (lambda t: _token_shift(t, f)) if m.shift_tokens else None
        perm, unperm = (lambda t: time_perm(t, f, n)), (lambda t: time_unperm(t, f, n))
        saved, consts = [], []
        d_attn = None if drop is None else (drop[0], drop[1], drop[2])
        d_ff = None if drop is None else (drop[0], drop[1], drop[3])
        for i, (time_attn, spatial, ff) in enumerate(m.layers):
            lp = params[3 + TS_PER_LAYER * i: 3 + TS_PER_LAYER * (i + 1)]
            sc_t, sc_s = _unwrap(time_attn.fn, m.shift_tokens).scale, _unwrap(spatial.fn, m.shift_tokens).scale
            eps = (time_attn.norm.eps, spatial.norm.eps, ff.norm.eps)
            x, s_t = prenorm_attention_forward(x, lp[0:5], eps[0], sc_t, heads, dh, 1, f, n, sin_t, cos_t, prec, pre, perm, unperm,
                                               key_mask=mask_time, mask_patch_queries=True, drop=d_attn, site=3 * i)
            x, s_s = prenorm_attention_forward(x, lp[5:10], eps[1], sc_s, heads, dh, 1, n, f, sin_s, cos_s, prec, pre,
                                               key_mask=mask_nat, mask_patch_queries=False, aprec=aprec, drop=d_attn, site=3 * i + 1)
            x, s_f = geglu_ff_forward(x, lp[10:16], eps[2], prec, pre, drop=d_ff, site=3 * i + 2)
            saved += [*s_t, *s_s, *s_f]
            consts.append((sc_t, sc_s) + eps)
        cls = layernorm(x, params[-4], params[-3], m.to_out[0].eps, b, dim, 1, ntok)
        out = linear(cls, params[-2], params[-1])
        ctx.geom = (b, f, c, H, W, ps, heads, dh, n, ntok, dim, prec, m.shift_tokens, m.to_out[0].eps)
        ctx.aprecs = (aprec, bprec)
        ctx.consts = consts
        ctx.drops = (d_attn, d_ff)
        ctx.nsaved = len(saved)
        ctx.masks = (mask_nat, mask_time)   # (uint8, no gradient: kept on ctx, not among the saved tensors)
        ctx.save_for_backward(*saved, tokens, x, cls, sin_s, cos_s, sin_t, cos_t, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        b, f, c, H, W, ps, heads, dh, n, ntok, dim, prec, shift, eps_out = ctx.geom
        aprec, bprec = ctx.aprecs
        if aprec != 0 and bprec == 0:
            raise _lib.HiddenPoseHipError(FP32_BACKWARD_AFTER_16BIT_FORWARD.format("TimeSformer"))
        L = _lib.lib()
        allt = ctx.saved_tensors
        saved = allt[:ctx.nsaved]
        tokens, xl, cls, sin_s, cos_s, sin_t, cos_t = allt[ctx.nsaved:ctx.nsaved + 7]
        params = allt[ctx.nsaved + 7:]
        dev = dout.device
        grads = [None] * len(params)
        dout = dout.contiguous()
        dcls, grads[-2], grads[-1] = linear_backward(cls, dout, params[-2])
        dx = torch.zeros(b, ntok, dim, dtype=torch.float32, device=dev)
        grads[-4], grads[-3] = layernorm_backward(xl, dcls, dx, params[-4], eps_out, b, dim, 1, ntok)
        del dcls
        pre_adj = (lambda t: token_shift_adjoint(t, f)) if shift else None
        perm, unperm = (lambda t: time_perm(t, f, n)), (lambda t: time_unperm(t, f, n))
        grouped = TIME_ATTENTION_BACKWARD == "grouped" and dh in GROUPED_DIM_HEADS
        mask_nat, mask_time = ctx.masks
        d_attn, d_ff = ctx.drops
        per = 9 + 9 + 3
        for i in reversed(range(len(ctx.consts))):
            sv = saved[per * i: per * (i + 1)]
            base = 3 + TS_PER_LAYER * i
            lp = params[base: base + TS_PER_LAYER]
            sc_t, sc_s, e_t, e_s, e_f = ctx.consts[i]
            grads[base + 10: base + 16] = geglu_ff_backward(dx, sv[18:21], lp[10:16], e_f, prec, pre_adj, drop=d_ff, site=3 * i + 2)
            grads[base + 5: base + 10] = prenorm_attention_backward(dx, sv[9:18], lp[5:10], e_s, sc_s, heads, dh, 1, n, f, sin_s, cos_s,
                                                                    prec, pre_adj, key_mask=mask_nat, mask_patch_queries=False,
                                                                    bprec=bprec, drop=d_attn, site=3 * i + 1)
            grads[base: base + 5] = prenorm_attention_backward(dx, sv[0:9], lp[0:5], e_t, sc_t, heads, dh, 1, f, n, sin_t, cos_t, prec,
                                                               pre_adj, perm, unperm, grouped=grouped, key_mask=mask_time,
                                                               mask_patch_queries=True, drop=d_attn, site=3 * i)
        grads[2] = _joint_sum(dx, 1).view(1, dim)      # cls_token (1, dim), shared by the batch
        demb = dx[:, 1:].contiguous().view(b * f * n, dim)
        need_video = ctx.needs_input_grad[0]
        dtok, grads[0], grads[1] = linear_backward(tokens, demb, params[0], need_dx=need_video)
        dvideo = None
        if need_video:
            dvideo = torch.empty(b, f, c, H, W, dtype=torch.float32, device=dev)
            _lib.check(L.hp_sformer_unpatchify(dtok.data_ptr(), dvideo.data_ptr(), b, f, c, H, W, ps, _st(dout)), "hp_sformer_unpatchify")
        return (dvideo, None, None, None, None, None, None, None, *grads)


TP_PER_LAYER = 11


def tokenpose_params(m):
    """The tensors TokenPoseFunction takes, in its order: patch embedding, keypoint_token, pos_embedding (frozen in the
    sine modes: requires_grad False, so it gets no gradient), the three stages' layers, the heat-map head."""
    ps = [m.patch_to_embedding.weight, m.patch_to_embedding.bias, m.keypoint_token, m.pos_embedding]
    for t in (m.transformer1, m.transformer2, m.transformer3):
        for attn, ff in t.layers:
            a, fw = attn.fn.fn, ff.fn.fn
            ps += [attn.fn.norm.weight, attn.fn.norm.bias, a.to_qkv.weight, a.to_out[0].weight, a.to_out[0].bias, ff.fn.norm.weight,
                   ff.fn.norm.bias, fw.net[0].weight, fw.net[0].bias, fw.net[3].weight, fw.net[3].bias]
    return ps + [m.mlp_head[0].weight, m.mlp_head[0].bias, m.mlp_head[1].weight, m.mlp_head[1].bias]


class TokenPoseFunction(torch.autograd.Function):
    """feature (b, c, H, W), module, three precisions, drop, *tokenpose_params(m) -> (b, num_keypoints, h_hm, w_hm).  Three
    stages of {x += MHA(LN(x)); x += W2 gelu(W1 LN(x))} over [keypoint tokens | patches] (one all-to-all group, no rotary
    tables).  drop: None or (seed, step, dropout, emb_dropout); site 0 is the assembled token matrix (emb_dropout), then per
    layer l (counted through the three stages) 1 + 3 l the attention's to_out, 2 + 3 l the hidden activation after the GELU,
    3 + 3 l the feed-forward's output (all `dropout`)."""

    @staticmethod
    def forward(ctx, feature, m, prec, aprec, bprec, drop, *params):
        """aprec, bprec: HP_PRECISION_* of the attention (every token is a patch query), forward and backward."""
        d_lay = None if drop is None else (drop[0], drop[1], drop[2])
        d_emb = None if drop is None else (drop[0], drop[1], drop[3])
        from . import hip_ops as ops

        L = _lib.lib()
        b, c, H, W = feature.shape
        nk, dim, ps = m.num_keypoints, m.keypoint_token.shape[-1], m.patch_size[0]
        dev = feature.device
        tok = torch.empty(b * (H // ps) * (W // ps), ps * ps * c, dtype=torch.float32, device=dev)
        _lib.check(L.hp_sformer_patchify(feature.data_ptr(), tok.data_ptr(), b, 1, c, H, W, ps, _st(feature)), "hp_sformer_patchify")
        emb = linear(tok, params[0], params[1]).view(b, -1, dim)
        n = emb.shape[1]
        ntok = nk + n
        pos = params[3]
        x = torch.empty(b, ntok, dim, dtype=torch.float32, device=dev)
        x[:, :nk] = params[2]
        if m.pos_embedding_type in ("sine", "sine-full"):
            x[:, nk:] = ops.add(emb.contiguous(), pos[:, :n].expand(b, -1, -1).contiguous())
        else:
            x[:, nk:] = emb
            x = ops.add(x, pos[:, :n + nk].expand(b, -1, -1).contiguous())
        del emb
        if _dropping(d_emb):
            dropout(x, d_emb, 0)
        saved, consts, outs = [], [], []
        i = 0
        for t in (m.transformer1, m.transformer2, m.transformer3):
            for idx, (attn, ff) in enumerate(t.layers):
                lp = params[4 + TP_PER_LAYER * i: 4 + TP_PER_LAYER * (i + 1)]
                if idx > 0 and t.all_attn:   # 'sine-full': the (frozen) table re-added to the patch rows
                    x = x.clone()
                    x[:, nk:] = ops.add(x[:, nk:].contiguous(), pos.expand(b, -1, -1).contiguous())
                a = attn.fn.fn
                dh = dim // a.heads
                x, s_a = prenorm_attention_forward(x, lp[0:5], attn.fn.norm.eps, a.scale, a.heads, dh, 0, ntok, 1, None, None, prec,
                                                   aprec=aprec, drop=d_lay, site=1 + 3 * i)
                x, s_f = gelu_ff_forward(x, lp[5:11], ff.fn.norm.eps, prec, drop=d_lay, site=2 + 3 * i)
                saved += [*s_a, *s_f]
                consts.append((a.scale, a.heads, dh, attn.fn.norm.eps, ff.fn.norm.eps))
                i += 1
            outs.append(x)
        cat = torch.cat([o[:, :nk] for o in outs], dim=2).contiguous().view(b * nk, 3 * dim)
        y = layernorm(cat, params[-4], params[-3], m.mlp_head[0].eps, b * nk, 3 * dim)
        out = linear(y, params[-2], params[-1])
        depths = [len(t.layers) for t in (m.transformer1, m.transformer2, m.transformer3)]
        ctx.geom = (b, c, H, W, ps, nk, n, ntok, dim, prec, m.pos_embedding_type, m.mlp_head[0].eps, depths)
        ctx.aprecs = (aprec, bprec)
        ctx.consts = consts
        ctx.drops = (d_lay, d_emb)
        ctx.nsaved = len(saved)
        ctx.save_for_backward(*saved, tok, cat, y, *params)
        return out.view(b, nk, m.heatmap_size[0], m.heatmap_size[1])

    @staticmethod
    def backward(ctx, dout):
        from . import hip_ops as ops

        b, c, H, W, ps, nk, n, ntok, dim, prec, pe_type, eps_head, depths = ctx.geom
        aprec, bprec = ctx.aprecs
        if aprec != 0 and bprec == 0:
            raise _lib.HiddenPoseHipError(FP32_BACKWARD_AFTER_16BIT_FORWARD.format("TokenPose"))
        L = _lib.lib()
        allt = ctx.saved_tensors
        saved = allt[:ctx.nsaved]
        tok, cat, y = allt[ctx.nsaved:ctx.nsaved + 3]
        params = allt[ctx.nsaved + 3:]
        dev = dout.device
        grads = [None] * len(params)
        dy, grads[-2], grads[-1] = linear_backward(y, dout.contiguous().view(b * nk, -1), params[-2])
        dcat = torch.zeros(b * nk, 3 * dim, dtype=torch.float32, device=dev)
        grads[-4], grads[-3] = layernorm_backward(cat, dy, dcat, params[-4], eps_head, b * nk, 3 * dim)
        del dy
        dcat = dcat.view(b, nk, 3 * dim)
        d_lay, d_emb = ctx.drops
        per = 9 + 4
        i = sum(depths)
        dx = None
        for s in (2, 1, 0):
            # the stage's output gradient: what flows back from the next stage + its keypoint rows' share of the head
            share = dcat[:, :, s * dim:(s + 1) * dim].contiguous()
            if dx is None:
                dx = torch.zeros(b, ntok, dim, dtype=torch.float32, device=dev)
                dx[:, :nk] = share
            else:
                dx[:, :nk] = ops.add(dx[:, :nk].contiguous(), share)
            for _ in range(depths[s]):   # ('sine-full' re-adds a frozen table: an identity on the gradient)
                i -= 1
                sv = saved[per * i: per * (i + 1)]
                base = 4 + TP_PER_LAYER * i
                lp = params[base: base + TP_PER_LAYER]
                scale, heads, dh, e_a, e_f = ctx.consts[i]
                grads[base + 5: base + 11] = gelu_ff_backward(dx, sv[9:13], lp[5:11], e_f, prec, drop=d_lay, site=2 + 3 * i)
                grads[base: base + 5] = prenorm_attention_backward(dx, sv[0:9], lp[0:5], e_a, scale, heads, dh, 0, ntok, 1, None, None, prec,
                                                                   bprec=bprec, drop=d_lay, site=1 + 3 * i)
        if _dropping(d_emb):
            dropout(dx, d_emb, 0)   # site 0's mask on the token matrix's gradient, before the assembly's gradients
        # token assembly: keypoint_token and the learnable pos_embedding are shared by the batch
        if ctx.needs_input_grad[6 + 2]:
            grads[2] = _joint_sum(dx, nk)
        if pe_type == "learnable" and ctx.needs_input_grad[6 + 3]:
            grads[3] = _joint_sum(dx, ntok)
        demb = dx[:, nk:].contiguous().view(b * n, dim)
        need_feat = ctx.needs_input_grad[0]
        dtok, grads[0], grads[1] = linear_backward(tok, demb, params[0], need_dx=need_feat)
        dfeat = None
        if need_feat:
            dfeat = torch.empty(b, c, H, W, dtype=torch.float32, device=dev)
            _lib.check(L.hp_sformer_unpatchify(dtok.data_ptr(), dfeat.data_ptr(), b, 1, c, H, W, ps, _st(dout)), "hp_sformer_unpatchify")
        return (dfeat, None, None, None, None, None, *grads)
