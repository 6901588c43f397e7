"""Building blocks shared by the transformer heads (transformer.TimeSformer, tokenpose.TokenPose_L_base): every
arithmetic step is a kernel of libhiddenpose_hip.so (Linear = the MFMA GEMM, LayerNorm, qkv split + rotary,
flash-style attention, GEGLU / GELU); PyTorch only owns the buffers.  These are the no-graph (inference) forms; the
training paths of the heads are in _xformer_autograd.py, which shares attention_forward, embed_tokens, assemble_tokens (the
rotary_emb=False heads' assembly with their learned position table), add_position_embedding and time_perm / time_unperm with
them."""
from __future__ import annotations

import torch

from . import _lib
from . import hip_ops as ops

PREC = {"fp32": 0, "bf16": 1, "bf16x3": 2, "bf16x6": 3}
ATTENTION_PREC = {"fp32": 0, "bf16": 1, "fp16": 4}   # HP_PRECISION_* of the attention's patch queries


def attention_precisions(module, dim_head, training):
    """HP_PRECISION_* codes of module.attention_precision and (training only, else 0) module.attention_backward_precision,
    with the rules of all three heads: a name outside fp32 / bf16 / fp16 and a 16-bit precision at a dim_head other than
    32 / 64 raise HiddenPoseHipError."""
    names = ("attention_precision", "attention_backward_precision") if training else ("attention_precision",)
    codes = []
    for name in names:
        value = getattr(module, name)
        if value not in ATTENTION_PREC:
            raise _lib.HiddenPoseHipError(f"{name} {value!r}: one of \"fp32\", \"bf16\", \"fp16\"")
        codes.append(ATTENTION_PREC[value])
    if any(codes) and dim_head not in (32, 64):
        raise _lib.HiddenPoseHipError("bf16 / fp16 attention is built for dim_head 32 and 64 only")
    return (codes + [0])[:2]


def _st(t):
    return _lib.current_stream_handle(t.device)


def linear(x2d, weight, bias=None, precision=0, residual=None):
    """y = x @ W^T + b (+ residual, accumulated in place into `residual`)."""
    M, K = x2d.shape
    N = weight.shape[0]
    y = residual if residual is not None else torch.empty(M, N, dtype=torch.float32, device=x2d.device)
    _lib.check(_lib.lib().hp_linear_forward(x2d.data_ptr(), weight.data_ptr(), _lib.ptr(bias), _lib.ptr(residual), y.data_ptr(),
                                            M, K, N, precision, _st(x2d)), "hp_linear_forward")
    return y


def layernorm(x2d, norm, rows=None, rows_per_batch=0, batch_stride_rows=0):
    rows = x2d.shape[0] if rows is None else rows
    dim = x2d.shape[-1]
    y = torch.empty(rows, dim, dtype=torch.float32, device=x2d.device)
    _lib.check(_lib.lib().hp_layernorm_forward(x2d.data_ptr(), y.data_ptr(), rows, dim, norm.weight.data_ptr(), norm.bias.data_ptr(),
                                               norm.eps, rows_per_batch, batch_stride_rows, _st(x2d)), "hp_layernorm_forward")
    return y


def attention(h2d, to_qkv, b, ntok, heads, dh, nj, n, frames, scale, sin_t=None, cos_t=None, precision=0, key_mask=None,
              mask_patch_queries=False, attention_precision=0):
    """Multi-head attention over tokens [nj class / joint tokens | frames groups of n tokens]: the class tokens attend
    to every token (keys without rotary embedding), a group's tokens to [class tokens | their group] with the rotary
    tables (n, rot_dim) applied to q and k.  h2d: (b * ntok, dim) normalised input -> (b, ntok, heads * dh).
    key_mask: None (today's call, launch for launch) or a (b, ntok) uint8 tensor in this call's token order, nonzero =
    attendable: the class queries leave the masked tokens out, the group queries too when mask_patch_queries.
    attention_precision: HP_PRECISION_* of the group (patch) queries, 0 / 1 (bf16) / 4 (fp16); the 16-bit kernels need dh 32
    or 64 and, with a key_mask, mask_patch_queries False.  The class queries are always exact fp32."""
    L = _lib.lib()
    dev = h2d.device
    inner = heads * dh
    qkv = linear(h2d, to_qkv.weight, None, precision)
    q = torch.empty(b, heads, ntok, dh, dtype=torch.float32, device=dev)
    k, k0, v = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    rot_dim = 0 if sin_t is None else sin_t.shape[-1]
    _lib.check(L.hp_sformer_qkv_prepare(qkv.data_ptr(), q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), b, ntok, heads, dh, nj,
                                        n, scale, _lib.ptr(sin_t), _lib.ptr(cos_t), rot_dim, _st(h2d)), "hp_sformer_qkv_prepare")
    att = torch.empty(b, ntok, inner, dtype=torch.float32, device=dev)
    if key_mask is not None:
        check_key_mask(key_mask, b, ntok, dev)
    attention_forward(q, k, k0, v, att, None, b, heads, dh, ntok, nj, n, frames, attention_workspace(b, heads, dh, dev), key_mask,
                      mask_patch_queries, attention_precision)
    return att


def attention_workspace(b, heads, dh, dev):
    nbytes = int(_lib.lib().hp_sformer_attention_workspace_bytes(b, heads, dh))
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=dev)


def attention_forward(q, k, k0, v, att, lse, b, heads, dh, ntok, nj, n, groups, ws, key_mask=None, mask_patch_queries=False,
                      precision=0):
    """The attention of q, k, k0, v (b, heads, ntok, dh) over [nj | groups x n] into att (b, ntok, heads * dh) and, unless
    None, the soft-max's log-sum-exp into lse (b, heads, ntok): the one place that chooses among the forward entries.  ws:
    attention_workspace(b, heads, dh, device).  Without lse the precision (HP_PRECISION_* of the patch queries) is an argument
    of the entry; with lse the fp32 and the 16-bit kernels have entries of their own."""
    L = _lib.lib()
    mask = () if key_mask is None else (key_mask.data_ptr(), int(bool(mask_patch_queries)))
    if lse is None:
        entry = L.hp_sformer_attention if key_mask is None else L.hp_sformer_attention_masked_p
        tail = (*mask, precision)
    elif precision == 0:
        entry = L.hp_sformer_attention_lse if key_mask is None else L.hp_sformer_attention_lse_masked
        tail = mask
    else:
        entry = L.hp_sformer_attention_lse_p if key_mask is None else L.hp_sformer_attention_lse_masked_p
        tail = (*mask, precision)
    out = (att.data_ptr(),) if lse is None else (att.data_ptr(), lse.data_ptr())
    _lib.check(entry(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), *out, b, heads, dh, ntok, nj, n, groups, *tail,
                     ws.data_ptr(), _st(q)), entry.__name__)


def check_key_mask(key_mask, b, ntok, dev):
    """The masked attention entries read b * ntok bytes at key_mask's address: anything else is refused here."""
    if (key_mask.dtype != torch.uint8 or tuple(key_mask.shape) != (b, ntok) or key_mask.device != dev
            or not key_mask.is_contiguous()):
        raise ValueError(f"key_mask must be a contiguous uint8 tensor of shape ({b}, {ntok}) on {dev}; got "
                         f"{key_mask.dtype} {tuple(key_mask.shape)} on {key_mask.device}")


def geglu_ff(x2d_resid, h2d, lin_in, lin_out, precision=0):
    """x += W2 (u[:, :H] * gelu(u[:, H:])),  u = W1 h  (models/transformer.py:58-74).  With a hidden width that is a multiple
    of 64 the GEGLU rides in the first GEMM's epilogue (u is never written); otherwise Linear, hp_geglu_forward, Linear."""
    hid = lin_out.weight.shape[1]
    rows = h2d.shape[0]
    g = torch.empty(rows, hid, dtype=torch.float32, device=h2d.device)
    if hid % 64 == 0 and lin_in.weight.shape[0] == 2 * hid:
        # the Linear's own weight / bias: the kernel pairs value and gate rows inside its gather (no cached reordered copy)
        _lib.check(_lib.lib().hp_linear_geglu_forward(h2d.data_ptr(), lin_in.weight.data_ptr(), _lib.ptr(lin_in.bias), g.data_ptr(), rows,
                                                      h2d.shape[1], 2 * hid, precision, _st(h2d)), "hp_linear_geglu_forward")
    else:
        u = linear(h2d, lin_in.weight, lin_in.bias, precision)
        _lib.check(_lib.lib().hp_geglu_forward(u.data_ptr(), g.data_ptr(), rows, hid, _st(h2d)), "hp_geglu_forward")
    return linear(g, lin_out.weight, lin_out.bias, precision, residual=x2d_resid)


def gelu_ff(x2d_resid, h2d, lin_in, lin_out, precision=0):
    """x += W2 gelu(W1 h)  (models/tokenpose.py:268-281)."""
    u = linear(h2d, lin_in.weight, lin_in.bias, precision)
    _lib.check(_lib.lib().hp_gelu_forward(u.data_ptr(), u.data_ptr(), u.numel(), _st(h2d)), "hp_gelu_forward")
    return linear(u, lin_out.weight, lin_out.bias, precision, residual=x2d_resid)


def patchify(video, patch):
    """'b f c (h p1) (w p2) -> (b f h w) (p1 p2 c)'"""
    b, f, c, H, W = video.shape
    tokens = torch.empty(b * f * (H // patch) * (W // patch), patch * patch * c, dtype=torch.float32, device=video.device)
    _lib.check(_lib.lib().hp_sformer_patchify(video.data_ptr(), tokens.data_ptr(), b, f, c, H, W, patch, _st(video)), "hp_sformer_patchify")
    return tokens


def embed_tokens(video, patch, weight, bias, lead):
    """video (b, f, c, H, W) -> (tokens, x): the patch rows (b f h w, p1 p2 c) and the token matrix [lead | Linear(tokens)]
    (b, nl + f h w, dim), lead (1, nl, dim) or (nl, dim) being the leading (class / joint / keypoint) tokens every sample
    shares.  The assembly is plain copies."""
    b = video.shape[0]
    tokens = patchify(video, patch)
    emb = linear(tokens, weight, bias)
    nl, dim = lead.shape[-2], emb.shape[1]
    x = torch.empty(b, nl + emb.shape[0] // b, dim, dtype=torch.float32, device=video.device)
    x[:, :nl] = lead
    x[:, nl:] = emb.view(b, -1, dim)
    return tokens, x


def check_table_rows(head, table, nl, f, n):
    """The learned position table (rows, dim) of a rotary_emb=False head covers tokens 0 .. rows - 1; a clip of f frames of n
    patches behind nl leading tokens needs nl + f n of them.  A longer clip is an IndexError, as in the reference (whose
    nn.Embedding lookup raises it), before anything is launched."""
    ntok, rows = nl + f * n, table.shape[0]
    if ntok > rows:
        raise IndexError(f"{head} (rotary_emb=False): ntok {ntok} = {nl} + {f} frames x {n} patches exceeds the position table's "
                         f"{rows} rows; the longest clip that fits has {max(0, (rows - nl) // n)} frames")


def assemble_tokens(video, patch, weight, bias, lead, pos):
    """embed_tokens plus the learned position table pos (rows, dim), rows >= the token count, added to every token, the
    leading ones included: [lead | Linear(tokens)] + pos[:ntok] in one pass (hp_tokens_assemble_forward), where embed_tokens is
    two slice copies.  -> (tokens, x)."""
    b = video.shape[0]
    tokens = patchify(video, patch)
    emb = linear(tokens, weight, bias)
    nl, dim = lead.shape[-2], emb.shape[1]
    ntok = nl + emb.shape[0] // b
    x = torch.empty(b, ntok, dim, dtype=torch.float32, device=video.device)
    _lib.check(_lib.lib().hp_tokens_assemble_forward(lead.data_ptr(), emb.data_ptr(), pos.data_ptr(), x.data_ptr(), b, nl, ntok, dim,
                                                     pos.shape[0], _st(video)), "hp_tokens_assemble_forward")
    return tokens, x


def add_position_embedding(x, pos, nk, pe_type):
    """TokenPose's token matrix x (b, nk + n, dim) plus its position embedding: the sine tables (1, n, dim) cover the patch
    rows only (added into x, which is returned), the learnable one (1, n + nk, dim) every row (a fresh tensor)."""
    b, ntok, _ = x.shape
    if pe_type in ("sine", "sine-full"):
        x[:, nk:] = ops.add(x[:, nk:].contiguous(), pos[:, :ntok - nk].expand(b, -1, -1).contiguous())
        return x
    return ops.add(x, pos[:, :ntok].expand(b, -1, -1).contiguous())


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
