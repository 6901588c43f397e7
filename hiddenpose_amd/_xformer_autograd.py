"""Training paths of the transformer heads (NlosPoseSformer, TimeSformer, TokenPose-L): one torch.autograd.Function per
head whose forward runs the no-graph forward's kernels in the same order (so its output is bit-identical) while keeping
what the backward needs, and whose backward is a chain of HIP kernels (include/hiddenpose_hip.h, "NlosPoseSformer
backward").  PyTorch only allocates, zero-fills and copies.

The op-level helpers (layernorm_backward, linear_backward, geglu_backward, gelu_backward) are written for any row-major
token matrix; all three Functions are built from the same sublayer helpers (pre-norm attention, GEGLU / GELU feed-forward)
and the token assembly of _xformer.embed_tokens with its adjoint (rotary_emb=False: _xformer.assemble_tokens and
assemble_tokens_backward, one HIP pass each).

Dropout.  Every nn.Dropout of the reference modules is a *site*: its position in the reference's forward
order.  A Function takes `drop`, None or (seed, step, p, p) with the module's two probabilities; a sublayer helper takes
`drop`, None or (seed, step, p) for its own sites, and `site`, the index of its first one.  The mask of a site is a pure
function of (seed, (step << 20) | site, flat element index, p) (hp_dropout_forward), so the backward regenerates it and no
mask is stored.  A site with p == 0 keeps its index and launches nothing; with drop None the code below is the code that ran
before dropout was built, launch for launch."""
from __future__ import annotations

import torch

from . import _lib
from . import _xformer as X
from ._xformer import _st


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


def training_gate(m, x, params, p0, p1, head, p0_name, p1_name):
    """(build an autograd graph?, drop) of a head's forward on input x.  A graph is built with dropout active (under no_grad
    too), or when grad mode is on, the module is in training mode or x requires grad, and x or one of `params` requires
    grad.  A graph without a seed while one of the two probabilities is > 0 is refused."""
    drop = active_dropout(m, p0, p1)
    graph = drop is not None or (torch.is_grad_enabled() and (m.training or x.requires_grad)
                                 and (x.requires_grad or any(p.requires_grad for p in params)))
    if graph and drop is None and (m.dropout_seed is None or m.training) and (p0 > 0 or p1 > 0):
        raise _lib.HiddenPoseHipError(f"{head} training: dropout is not built without a seed ({p0_name} / {p1_name} must be 0; "
                                      "set dropout_seed to enable)")
    return graph, drop


def _split(drop):
    """A Function's (seed, step, p0, p1) -> its two sublayer tuples (seed, step, p0), (seed, step, p1); None -> None, None."""
    return (None, None) if drop is None else ((drop[0], drop[1], drop[2]), (drop[0], drop[1], drop[3]))


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


def attention_backward(q, k, k0, v, out, dout, lse, b, heads, dh, ntok, nj, n, frames, precision=0, key_mask=None,
                       mask_patch_queries=False, grouped=False):
    """(dQ, dK, dK0, dV): the one place that chooses among the backward entries and sizes their workspace.  precision 0: the
    exact-fp32 backward; 1 (bf16) / 4 (fp16): the patch queries' part on the 16-bit matrix cores (dim_head 32 or 64), the
    joint queries' part exact fp32.  key_mask / mask_patch_queries: the forward's (a 16-bit precision needs mask_patch_queries
    False).  grouped: the fp32 entry for n <= 64 tokens per group at dim_head 16 / 24 / 32, bit-equal to the generic one."""
    L = _lib.lib()
    assert not (grouped and precision), "the grouped attention backward is exact fp32"
    masked = key_mask is not None
    if precision:
        entry, size = ((L.hp_sformer_attention_backward_masked_p, L.hp_sformer_attention_backward_masked_p_workspace_bytes) if masked
                       else (L.hp_sformer_attention_backward_p, L.hp_sformer_attention_backward_p_workspace_bytes))
    elif grouped:
        entry, size = ((L.hp_sformer_attention_backward_grouped_masked, L.hp_sformer_attention_backward_grouped_masked_workspace_bytes)
                       if masked else (L.hp_sformer_attention_backward_grouped, L.hp_sformer_attention_backward_grouped_workspace_bytes))
    else:
        entry, size = ((L.hp_sformer_attention_backward_masked, L.hp_sformer_attention_backward_masked_workspace_bytes) if masked
                       else (L.hp_sformer_attention_backward, L.hp_sformer_attention_backward_workspace_bytes))
    mask = (key_mask.data_ptr(), int(bool(mask_patch_queries))) if masked else ()
    prec = (precision,) if precision else ()
    dq, dk, dk0, dv = (torch.empty_like(q) for _ in range(4))
    nb = size(b, heads, dh, ntok, nj, frames, *prec)
    ws = _ws(nb, q.device)
    _lib.check(entry(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                     dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(), dv.data_ptr(), b, heads, dh, ntok, nj, n, frames, *mask, *prec,
                     ws.data_ptr(), nb, _st(q)), entry.__name__)
    return dq, dk, dk0, dv


def attention_backward_grouped(q, k, k0, v, out, dout, lse, b, heads, dh, ntok, nj, n, groups):
    """attention_backward for short groups: n <= 64 tokens per group."""
    return attention_backward(q, k, k0, v, out, dout, lse, b, heads, dh, ntok, nj, n, groups, grouped=True)


# ---------------------------------------------------------------------------------------------------------------------
# The sublayer helpers of the three heads' training paths take the layer input x (b, ntok, dim) and return a fresh
# x + sublayer(x) together with what their backward needs; their backward ADDS the sublayer's input gradient into dx (the
# residual stream's gradient, which already holds d(x + sublayer(x))) and returns the parameter gradients.

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


# time attention's backward: "grouped" (attention_backward's grouped entry) or "generic"; DESIGN 4.4.2 records the A/B that
# chose it
TIME_ATTENTION_BACKWARD = "grouped"
GROUPED_DIM_HEADS = (16, 24, 32)   # the grouped entry is not built for dim_head 64: that width takes the generic one


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
                              key_mask=None, mask_patch_queries=False, aprec=0, drop=None, site=0, need_lse=True):
    """x + Wo unperm(Attn(perm(pre(LN(x))))) + bo for the token layout [nj | groups x n] of the permuted rows, as
    _xformer.attention runs it, but with the soft-max's lse unless need_lse is False (the backward then has nothing to
    recompute P from); key_mask (b, ntok) uint8 in the permuted rows' order.  aprec: HP_PRECISION_* of the patch queries.
    p = (ln_w, ln_b, wqkv, wo, bo).  drop / site: dropout on to_out's output, before the residual.  -> (x1, saved)."""
    L = _lib.lib()
    ln_w, ln_b, wqkv, wo, bo = p
    b, ntok, dim = x.shape
    rows, inner = b * ntok, heads * dh
    dev = x.device
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
                                        scale, _lib.ptr(sin_t), _lib.ptr(cos_t), rot_dim, _st(x)), "hp_sformer_qkv_prepare")
    del qkv
    att = torch.empty(b, ntok, inner, dtype=torch.float32, device=dev)
    lse = torch.empty(b, heads, ntok, dtype=torch.float32, device=dev) if need_lse else None
    X.attention_forward(q, k, k0, v, att, lse, b, heads, dh, ntok, nj, n, groups, X.attention_workspace(b, heads, dh, dev), key_mask,
                        mask_patch_queries, aprec)
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
    dq, dk, dk0, dv = attention_backward(q, k, k0, v, att, datt, lse, b, heads, dh, ntok, nj, n, groups, bprec, key_mask,
                                         mask_patch_queries, grouped)
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


def assemble_tokens_backward(dx, lead_rows, pos_shape, need_lead, need_pos):
    """Adjoint of _xformer.assemble_tokens in one pass over dx (b, ntok, dim) (hp_tokens_assemble_backward): -> (dlead (lead_rows,
    dim), the batch sum of the leading rows, or None unless need_lead; dpos of pos_shape, the batch sum of every row with
    exact zeros in the table's rows past ntok, or None unless need_pos; demb (b, ntok - lead_rows, dim), the patch rows'
    contiguous copy for embed_tokens_backward)."""
    b, ntok, dim = dx.shape
    dev = dx.device
    dlead = torch.empty(lead_rows, dim, dtype=torch.float32, device=dev) if need_lead else None
    dpos = torch.empty(pos_shape, dtype=torch.float32, device=dev) if need_pos else None
    demb = torch.empty(b, ntok - lead_rows, dim, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().hp_tokens_assemble_backward(dx.data_ptr(), _lib.ptr(dlead), _lib.ptr(dpos), demb.data_ptr(), b, lead_rows, ntok,
                                                      dim, pos_shape[0], _st(dx)), "hp_tokens_assemble_backward")
    return dlead, dpos, demb


def embed_tokens_backward(dx, tokens, weight, lead_rows, video_shape, patch, need_input, demb=None):
    """Adjoint of _xformer.embed_tokens below the lead_rows leading rows of dx (b, ntok, dim): -> (dvideo (b, f, c, H, W), or
    None unless need_input; dW; db) through the embedding's Linear and unpatchify.  demb: those rows' contiguous copy where
    assemble_tokens_backward has made it already."""
    b, f, c, H, W = video_shape
    demb = (dx[:, lead_rows:].contiguous() if demb is None else demb).view(tokens.shape[0], -1)
    dtok, dw, db = linear_backward(tokens, demb, weight, need_dx=need_input)
    dvideo = None
    if need_input:
        dvideo = torch.empty(b, f, c, H, W, dtype=torch.float32, device=dx.device)
        _lib.check(_lib.lib().hp_sformer_unpatchify(dtok.data_ptr(), dvideo.data_ptr(), b, f, c, H, W, patch, _st(dx)),
                   "hp_sformer_unpatchify")
    return dvideo, dw, db


def _layer_params(layer):
    _time_attn, spatial, ff = layer
    a = spatial.fn
    return [spatial.norm.weight, spatial.norm.bias, a.to_qkv.weight, a.to_out[0].weight, a.to_out[0].bias, ff.norm.weight,
            ff.norm.bias, ff.fn.net[0].weight, ff.fn.net[0].bias, ff.fn.net[3].weight, ff.fn.net[3].bias]


PER_LAYER = 11


def _table_param(m):
    """[the learned position table] of a rotary_emb=False head, [] of a rotary one."""
    table = m.position_table()
    return [] if table is None else [table]


def trainable_params(m):
    """The parameters the forward reads, in the order SformerFunction takes them (the time-attention weights, allocated
    but never run, are not among them: their .grad stays None).  With rotary_emb=False the position table follows
    joints_token."""
    ps = [m.to_patch_embedding.weight, m.to_patch_embedding.bias, m.joints_token] + _table_param(m)
    for layer in m.layers:
        ps += _layer_params(layer)
    ps += [m.to_out[0].weight, m.to_out[0].bias, m.to_out[1].weight, m.to_out[1].bias]
    return ps


class SformerFunction(torch.autograd.Function):
    """video (b, f, c, H, W), module, three precisions, drop, *trainable_params(m) -> (b, num_joints, 4, out_dim / 4).
    Per layer: space attention (the axial tables, groups = f frames of hp*wp patches behind the num_joints joint tokens) and
    GEGLU feed-forward.  drop: None or (seed, step, attn_dropout, ff_dropout); sites per layer: 2 i the spatial attention's
    to_out, 2 i + 1 the feed-forward's hidden activation (the time attention is never run and has no site).
    With rotary_emb=False params[3] is the position table: the token matrix is assembled with it (X.assemble_tokens; not a
    dropout site) and every attention runs without rotary tables."""

    @staticmethod
    def forward(ctx, video, m, prec, aprec, bprec, drop, *params):
        """prec, aprec, bprec: HP_PRECISION_* of the Linear layers, the patch attention's forward and the attention backward."""
        b, f, c, H, W = video.shape
        ps, nj, heads, dh = m.patch_size, m.num_joints, m.heads, m.dim_head
        hp, wp = H // ps, W // ps
        n = hp * wp
        first = 3 if m.use_rotary_emb else 4     # index of the first layer's parameters
        if m.use_rotary_emb:
            tokens, x = X.embed_tokens(video, ps, *params[:3])
            sin_t, cos_t = m.image_rot_emb.tables(hp, wp, video.device)
        else:
            tokens, x = X.assemble_tokens(video, ps, *params[:4])
            sin_t = cos_t = None
        ntok, dim = x.shape[1:]
        d_attn, d_ff = _split(drop)
        # a 16-bit backward recomputes P from the 16-bit forward's own lse; a 16-bit forward with the fp32 backward (which
        # backward() refuses) keeps none
        need_lse = aprec == 0 or bprec != 0
        saved, consts = [], []
        for i, (_time_attn, spatial, ff) in enumerate(m.layers):
            lp = params[first + PER_LAYER * i: first + PER_LAYER * (i + 1)]
            scale, e_a, e_f = spatial.fn.scale, spatial.norm.eps, ff.norm.eps
            x, s_a = prenorm_attention_forward(x, lp[0:5], e_a, scale, heads, dh, nj, n, f, sin_t, cos_t, prec, aprec=aprec,
                                               drop=d_attn, site=2 * i, need_lse=need_lse)
            x, s_f = geglu_ff_forward(x, lp[5:11], e_f, prec, drop=d_ff, site=2 * i + 1)
            saved += [*s_a, *s_f]
            consts.append((scale, e_a, e_f))
        jt = layernorm(x, params[-4], params[-3], m.to_out[0].eps, b * nj, dim, nj, ntok)
        out = linear(jt, params[-2], params[-1])
        ctx.geom = (tuple(video.shape), ps, nj, heads, dh, n, prec, aprec, bprec, m.to_out[0].eps)
        ctx.first = first
        ctx.consts = consts
        ctx.drops = (d_attn, d_ff)
        ctx.nsaved = len(saved)
        ctx.save_for_backward(*saved, tokens, x, jt, sin_t, cos_t, *params)
        return out.view(b, nj, 4, -1)

    @staticmethod
    def backward(ctx, dout):
        video_shape, ps, nj, heads, dh, n, prec, aprec, bprec, eps_out = ctx.geom
        if aprec != 0 and bprec == 0:
            raise _lib.HiddenPoseHipError(FP32_BACKWARD_AFTER_16BIT_FORWARD.format("NlosPoseSformer"))
        allt = ctx.saved_tensors
        saved, (tokens, xl, jt, sin_t, cos_t), params = allt[:ctx.nsaved], allt[ctx.nsaved:ctx.nsaved + 5], allt[ctx.nsaved + 5:]
        b, f = video_shape[:2]
        ntok, dim = xl.shape[1:]
        grads = [None] * len(params)
        # head: LN(x[:, :nj]) -> Linear
        djt, grads[-2], grads[-1] = linear_backward(jt, dout.contiguous().view(b * nj, -1), params[-2])
        dx = torch.zeros(b, ntok, dim, dtype=torch.float32, device=dout.device)
        grads[-4], grads[-3] = layernorm_backward(xl, djt, dx, params[-4], eps_out, b * nj, dim, nj, ntok)
        del djt
        d_attn, d_ff = ctx.drops
        per = 9 + 3
        first = ctx.first
        for i in reversed(range(len(ctx.consts))):
            sv = saved[per * i: per * (i + 1)]
            base = first + PER_LAYER * i
            lp = params[base: base + PER_LAYER]
            scale, e_a, e_f = ctx.consts[i]
            grads[base + 5: base + 11] = geglu_ff_backward(dx, sv[9:12], lp[5:11], e_f, prec, drop=d_ff, site=2 * i + 1)
            grads[base: base + 5] = prenorm_attention_backward(dx, sv[0:9], lp[0:5], e_a, scale, heads, dh, nj, n, f, sin_t, cos_t, prec,
                                                               bprec=bprec, drop=d_attn, site=2 * i)
        demb = None
        if first == 4:     # joints_token and the position table, both shared by the batch, and the patch rows in one pass
            dlead, grads[3], demb = assemble_tokens_backward(dx, nj, params[3].shape, ctx.needs_input_grad[6 + 2], ctx.needs_input_grad[6 + 3])
            grads[2] = None if dlead is None else dlead.view(1, nj, dim)
        else:
            grads[2] = _joint_sum(dx, nj)      # joints_token (1, nj, dim), shared by the batch
        dvideo, grads[0], grads[1] = embed_tokens_backward(dx, tokens, params[0], nj, video_shape, ps, ctx.needs_input_grad[0], demb)
        return (dvideo, None, None, None, None, None, *grads)


def _unwrap(m, shift):
    return m.fn if shift else m


TS_PER_LAYER = 16


def timesformer_params(m):
    """The parameters TimeSformerFunction takes, in its order (every parameter of the module; with rotary_emb=False the
    position table follows cls_token)."""
    ps = [m.to_patch_embedding.weight, m.to_patch_embedding.bias, m.cls_token] + _table_param(m)
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
    class query applies it), GEGLU feed-forward; token shift before each when m.shift_tokens.
    With rotary_emb=False params[3] is the position table: the token matrix is assembled with it (X.assemble_tokens; not a
    dropout site) and both attentions run without rotary tables."""

    @staticmethod
    def forward(ctx, video, m, prec, aprec, bprec, mask_nat, mask_time, drop, *params):
        """aprec, bprec: HP_PRECISION_* of the spatial attention's patch queries, forward and backward (the time attention and
        the class queries are exact fp32)."""
        from .transformer import _token_shift

        b, f, c, H, W = video.shape
        ps, heads, dh = m.patch_size, m.heads, m.dim_head
        hp, wp = H // ps, W // ps
        n = hp * wp
        dev = video.device
        first = 3 if m.use_rotary_emb else 4     # index of the first layer's parameters
        if m.use_rotary_emb:
            tokens, x = X.embed_tokens(video, ps, *params[:3])
            sin_s, cos_s = m.image_rot_emb.tables(hp, wp, dev)
            sin_t, cos_t = m._frame_tables(f, dev)
        else:
            tokens, x = X.assemble_tokens(video, ps, *params[:4])
            sin_s = cos_s = sin_t = cos_t = None
        ntok, dim = x.shape[1:]
        pre = (lambda t: _token_shift(t, f)) if m.shift_tokens else None
        perm, unperm = (lambda t: X.time_perm(t, f, n)), (lambda t: X.time_unperm(t, f, n))
        saved, consts = [], []
        d_attn, d_ff = _split(drop)
        for i, (time_attn, spatial, ff) in enumerate(m.layers):
            lp = params[first + TS_PER_LAYER * i: first + TS_PER_LAYER * (i + 1)]
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
        ctx.geom = (tuple(video.shape), ps, heads, dh, n, prec, m.shift_tokens, m.to_out[0].eps)
        ctx.aprecs = (aprec, bprec)
        ctx.first = first
        ctx.consts = consts
        ctx.drops = (d_attn, d_ff)
        ctx.nsaved = len(saved)
        ctx.masks = (mask_nat, mask_time)   # (uint8, no gradient: kept on ctx, not among the saved tensors)
        ctx.save_for_backward(*saved, tokens, x, cls, sin_s, cos_s, sin_t, cos_t, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        video_shape, ps, heads, dh, n, prec, shift, eps_out = ctx.geom
        aprec, bprec = ctx.aprecs
        if aprec != 0 and bprec == 0:
            raise _lib.HiddenPoseHipError(FP32_BACKWARD_AFTER_16BIT_FORWARD.format("TimeSformer"))
        allt = ctx.saved_tensors
        saved = allt[:ctx.nsaved]
        tokens, xl, cls, sin_s, cos_s, sin_t, cos_t = allt[ctx.nsaved:ctx.nsaved + 7]
        params = allt[ctx.nsaved + 7:]
        b, f = video_shape[:2]
        ntok, dim = xl.shape[1:]
        dev = dout.device
        grads = [None] * len(params)
        dout = dout.contiguous()
        dcls, grads[-2], grads[-1] = linear_backward(cls, dout, params[-2])
        dx = torch.zeros(b, ntok, dim, dtype=torch.float32, device=dev)
        grads[-4], grads[-3] = layernorm_backward(xl, dcls, dx, params[-4], eps_out, b, dim, 1, ntok)
        del dcls
        pre_adj = (lambda t: token_shift_adjoint(t, f)) if shift else None
        perm, unperm = (lambda t: X.time_perm(t, f, n)), (lambda t: X.time_unperm(t, f, n))
        grouped = TIME_ATTENTION_BACKWARD == "grouped" and dh in GROUPED_DIM_HEADS
        mask_nat, mask_time = ctx.masks
        d_attn, d_ff = ctx.drops
        per = 9 + 9 + 3
        first = ctx.first
        for i in reversed(range(len(ctx.consts))):
            sv = saved[per * i: per * (i + 1)]
            base = first + TS_PER_LAYER * i
            lp = params[base: base + TS_PER_LAYER]
            sc_t, sc_s, e_t, e_s, e_f = ctx.consts[i]
            grads[base + 10: base + 16] = geglu_ff_backward(dx, sv[18:21], lp[10:16], e_f, prec, pre_adj, drop=d_ff, site=3 * i + 2)
            grads[base + 5: base + 10] = prenorm_attention_backward(dx, sv[9:18], lp[5:10], e_s, sc_s, heads, dh, 1, n, f, sin_s, cos_s,
                                                                    prec, pre_adj, key_mask=mask_nat, mask_patch_queries=False,
                                                                    bprec=bprec, drop=d_attn, site=3 * i + 1)
            grads[base: base + 5] = prenorm_attention_backward(dx, sv[0:9], lp[0:5], e_t, sc_t, heads, dh, 1, f, n, sin_t, cos_t, prec,
                                                               pre_adj, perm, unperm, grouped=grouped, key_mask=mask_time,
                                                               mask_patch_queries=True, drop=d_attn, site=3 * i)
        demb = None
        if first == 4:     # cls_token and the position table, both shared by the batch, and the patch rows in one pass
            grads[2], grads[3], demb = assemble_tokens_backward(dx, 1, params[3].shape, ctx.needs_input_grad[8 + 2], ctx.needs_input_grad[8 + 3])
        else:
            grads[2] = _joint_sum(dx, 1).view(1, dim)      # cls_token (1, dim), shared by the batch
        dvideo, grads[0], grads[1] = embed_tokens_backward(dx, tokens, params[0], 1, video_shape, ps, ctx.needs_input_grad[0], demb)
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
        d_lay, d_emb = _split(drop)
        b, c, H, W = feature.shape
        nk, ps, pos = m.num_keypoints, m.patch_size[0], params[3]
        tok, x = X.embed_tokens(feature.view(b, 1, c, H, W), ps, *params[:3])
        x = X.add_position_embedding(x, pos, nk, m.pos_embedding_type)
        ntok, dim = x.shape[1:]
        if _dropping(d_emb):
            dropout(x, d_emb, 0)
        saved, consts, outs = [], [], []
        i = 0
        for t in (m.transformer1, m.transformer2, m.transformer3):
            for idx, (attn, ff) in enumerate(t.layers):
                lp = params[4 + TP_PER_LAYER * i: 4 + TP_PER_LAYER * (i + 1)]
                if idx > 0 and t.all_attn:   # 'sine-full': the (frozen) table re-added to the patch rows
                    x = X.add_position_embedding(x.clone(), pos, nk, m.pos_embedding_type)
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
        ctx.geom = ((b, 1, c, H, W), ps, nk, ntok, dim, prec, m.pos_embedding_type, m.mlp_head[0].eps, depths)
        ctx.aprecs = (aprec, bprec)
        ctx.consts = consts
        ctx.drops = (d_lay, d_emb)
        ctx.nsaved = len(saved)
        ctx.save_for_backward(*saved, tok, cat, y, *params)
        return out.view(b, nk, m.heatmap_size[0], m.heatmap_size[1])

    @staticmethod
    def backward(ctx, dout):
        from . import hip_ops as ops

        video_shape, ps, nk, ntok, dim, prec, pe_type, eps_head, depths = ctx.geom
        b = video_shape[0]
        aprec, bprec = ctx.aprecs
        if aprec != 0 and bprec == 0:
            raise _lib.HiddenPoseHipError(FP32_BACKWARD_AFTER_16BIT_FORWARD.format("TokenPose"))
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
        dfeat, grads[0], grads[1] = embed_tokens_backward(dx, tok, params[0], nk, video_shape, ps, ctx.needs_input_grad[0])
        if dfeat is not None:
            dfeat = dfeat.view(b, *video_shape[2:])     # the feature map went through as one frame
        return (dfeat, None, None, None, None, None, *grads)
