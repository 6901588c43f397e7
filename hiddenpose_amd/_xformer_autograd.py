"""Training path of NlosPoseSformer: one torch.autograd.Function whose forward runs the no-graph forward's kernels in the
same order (so its output is bit-identical) while keeping what the backward needs, and whose backward is a chain of HIP
kernels (include/hiddenpose_hip.h, "NlosPoseSformer backward").  PyTorch only allocates, zero-fills and copies.

The op-level helpers (layernorm_backward, linear_backward, geglu_backward) are written for any row-major token matrix, so
the other transformer heads can reuse them."""
from __future__ import annotations

import torch

from . import _lib


def _st(t):
    return _lib.current_stream_handle(t.device)


def _ws(nbytes, dev):
    return torch.empty(max(1, (int(nbytes) + 3) // 4), dtype=torch.float32, device=dev)


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


def geglu_backward(u, dg):
    rows, hid = dg.shape
    du = torch.empty(rows, 2 * hid, dtype=torch.float32, device=u.device)
    _lib.check(_lib.lib().hp_geglu_backward(u.data_ptr(), dg.data_ptr(), du.data_ptr(), rows, hid, _st(u)), "hp_geglu_backward")
    return du


def attention_backward(q, k, k0, v, out, dout, lse, b, heads, dh, ntok, nj, n, frames):
    L = _lib.lib()
    dq, dk, dk0, dv = (torch.empty_like(q) for _ in range(4))
    nb = L.hp_sformer_attention_backward_workspace_bytes(b, heads, dh, ntok, nj, frames)
    ws = _ws(nb, q.device)
    _lib.check(L.hp_sformer_attention_backward(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(),
                                               lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(), dv.data_ptr(), b, heads, dh, ntok,
                                               nj, n, frames, ws.data_ptr(), nb, _st(q)), "hp_sformer_attention_backward")
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
    """video (b, f, c, H, W), *trainable_params(m) -> (b, num_joints, 4, out_dim / 4)."""

    @staticmethod
    def forward(ctx, video, m, prec, aprec, *params):
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
            else:
                _lib.check(L.hp_sformer_attention(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), att.data_ptr(), b, heads, dh,
                                                  ntok, nj, n, f, aprec, aws.data_ptr(), st), "hp_sformer_attention")
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
            x2 = linear(g, w2, b2, prec, addend=x1.view(rows, dim)).view(b, ntok, dim)
            saved += [x, h1, q, k, k0, v, att, lse, x1, h2, g]
            x = x2
        jt = torch.empty(b * nj, dim, dtype=torch.float32, device=dev)
        _lib.check(L.hp_layernorm_forward(x.data_ptr(), jt.data_ptr(), b * nj, dim, params[-4].data_ptr(), params[-3].data_ptr(),
                                          m.to_out[0].eps, nj, ntok, st), "hp_layernorm_forward")
        out = linear(jt, params[-2], params[-1])
        ctx.geom = (b, f, c, H, W, ps, nj, heads, dh, n, ntok, dim, rot_dim, prec, aprec)
        ctx.consts = [(layer[1].fn.scale, layer[1].norm.eps, layer[2].norm.eps) for layer in m.layers] + [m.to_out[0].eps]
        ctx.depth = len(m.layers)
        ctx.nsaved = len(saved)
        ctx.save_for_backward(*saved, tokens, x, jt, sin_t, cos_t, *params)
        return out.view(b, nj, 4, -1)

    @staticmethod
    def backward(ctx, dout):
        b, f, c, H, W, ps, nj, heads, dh, n, ntok, dim, rot_dim, prec, aprec = ctx.geom
        if aprec != 0:
            raise _lib.HiddenPoseHipError("NlosPoseSformer backward: training needs attention_precision = \"fp32\" (the bf16 / fp16 "
                                          "patch attention has no backward)")
        L = _lib.lib()
        allt = ctx.saved_tensors
        saved, (tokens, xl, jt, sin_t, cos_t), params = allt[:ctx.nsaved], allt[ctx.nsaved:ctx.nsaved + 5], allt[ctx.nsaved + 5:]
        dev = dout.device
        st = _st(dout)
        rows, inner = b * ntok, heads * dh
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
            du = geglu_backward(u, dg)
            del u, dg
            dh2, grads[base + 7], grads[base + 8] = linear_backward(h2.view(rows, dim), du, w1, prec)
            del du
            grads[base + 5], grads[base + 6] = layernorm_backward(x1, dh2, dx, ln2_w, eps2, rows, dim)   # dx := dx1
            del dh2
            # attention: x1 = x + Wo att + bo
            datt, grads[base + 3], grads[base + 4] = linear_backward(att.view(rows, inner), d2, wo, prec)
            dq, dk, dk0, dv = attention_backward(q, k, k0, v, att, datt, lse, b, heads, dh, ntok, nj, n, f)
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
        return (dvideo, None, None, None, *grads)
