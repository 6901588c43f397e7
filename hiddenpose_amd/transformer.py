"""TimeSformer: divided space-time attention with one class token, axial / temporal rotary embeddings, GEGLU
feed-forward and optional token shift.

Drop-in for models/transformer.py `TimeSformer(**kwargs)` (:152-257): same constructor keywords, same
state_dict keys, `forward(video (b, f, c, H, W), mask=None) -> (b, 72)`.  Per layer (:251-254): x += TimeAttn(LN(x)) over the f
tokens that share a patch position; x += SpaceAttn(LN(x)) over the n patches of a frame; x += GEGLU-FF(LN(x)).  In
both attentions the class token attends to all tokens with un-rotated keys, the patch tokens to [class | their group]
(:110-141).  All arithmetic is in libhiddenpose_hip.so (see _xformer.py); the '(b n) f' regrouping of the time
attention is a transposed copy of the token matrix.  Trainable: autograd runs _xformer_autograd.TimeSformerFunction, whose
backward is a chain of HIP kernels (csrc/sformer_backward.hip).

`mask` (b, f) bool, True = the frame is valid (:208-253: a batch of clips of unequal length).  The tokens of a padded frame
are left out of every soft-max a valid token or the class token takes part in: in the time attention a patch query attends to
[class | the valid frames of its patch position], in both attentions the class query attends to [class | every valid token];
the spatial attention's patch queries are not masked (:253 passes only the class mask).  The class key is always attendable,
so a sample without a valid frame is legal.  The masked kernels are csrc/sformer_masked.hip (exact fp32; an all-True mask
gives the bits of mask=None).  With shift_tokens the content of padded frames leaks through the shift, as in the reference.

`attention_precision` / `attention_backward_precision` ("fp32" default, "bf16", "fp16"; NlosPoseSformer's attributes and
rules: dim_head 32 or 64, a 16-bit forward needs a 16-bit backward, a 16-bit backward takes either forward) put the SPATIAL
attention's patch queries on the 16-bit matrix cores, forward and backward, with and without `mask`: n patches per frame
attend to [class | their frame], which is where the attention's work is.  The time attention stays exact fp32 (its groups
have f + 1 keys: a 32-key MFMA tile would be mostly padding, and its backward is the grouped fp32 kernel), and so do the class
queries in both attentions (one query over every token, the only query that applies the spatial mask).

Dropout (`attn_dropout` / `ff_dropout`, the reference's keywords) is opt-in by seed, because the HIP path cannot draw from
torch's global generator: set `dropout_seed` to an int.  It is then ACTIVE while the module is in training mode and one of the
two probabilities is > 0: every nn.Dropout of the reference's forward is a site whose keep mask is a pure function of
(dropout_seed, dropout_step, site, element index, p) (Philox4x32-10, hp_dropout_forward), each forward draws its masks and then
adds 1 to `dropout_step` (also under torch.no_grad(), as torch's dropout follows the training flag alone), setting
`dropout_step` back replays the same masks, and the backward regenerates them: no mask is stored.  Neither attribute is part
of the state_dict.  With `dropout_seed` None nothing changes: a training forward with a probability > 0 is refused, the
no-grad path ignores dropout.  In eval mode nothing is drawn, with or without a seed.  Sites per layer: the time attention's
to_out (on the un-permuted rows, as in the reference), the spatial attention's to_out (both attn_dropout), the feed-forward's
hidden activation after the GEGLU (ff_dropout).

`rotary_emb=False` (:182-187, :229-235) is the learned-position variant: the module owns `pos_emb = nn.Embedding(num_frames *
num_patches + 1, dim)` (default initialisation; the checkpoint key is `pos_emb.weight`) and neither rotary module.  The table's
first ntok rows are added to the token matrix, class token included, once before the first layer -- in the pass that assembles
[class | patch embedding] (hp_tokens_assemble_forward; its adjoint hp_tokens_assemble_backward gives the table's, the class
token's and the patch embedding's gradients from one read of the token gradient) -- and every attention of every
layer then runs without rotation (rot_dim 0: the class query sees K0 = K), masked and 16-bit entries alike.  A clip shorter
than num_frames uses the table's prefix and leaves an exactly zero gradient in the rows behind it; a clip with more tokens than
the table has rows raises IndexError before anything is launched.  mask, shift_tokens, the precisions and dropout compose with
it unchanged (the table add is not a dropout site).  A frozen table (requires_grad False) gets no gradient and costs none."""
from __future__ import annotations

from math import log, pi

import torch
from torch import nn

from . import _lib
from . import _xformer as X
from . import _xformer_autograd as _xa
from .NlosPoseSformer import AxialRotaryEmbedding, RotaryEmbedding, _Attention, _FeedForward, _PreNorm


class _PreTokenShift(nn.Module):
    """models/transformer.py:33-54 -- parameter-free wrapper: the first three thirds of the feature dim of the patch
    tokens are taken from the previous / same / next frame (zero at the clip ends)."""

    def __init__(self, frames, fn):
        super().__init__()
        self.frames, self.fn = frames, fn


def _token_shift(x, frames, nj=1):
    """x (b, nj + f*n, d) -> shifted copy (plain slice copies: data movement only)."""
    b, ntok, d = x.shape
    n = (ntok - nj) // frames
    p = x[:, nj:].view(b, frames, n, d)
    out = x.clone()
    o = out[:, nj:].view(b, frames, n, d)
    c = d // 3
    o[:, :, :, :c] = 0
    o[:, :-1, :, :c] = p[:, 1:, :, :c]            # shift(t, -1): frame j takes frame j + 1
    o[:, :, :, 2 * c:3 * c] = 0
    o[:, 1:, :, 2 * c:3 * c] = p[:, :-1, :, 2 * c:3 * c]   # shift(t, +1): frame j takes frame j - 1
    return out


class TimeSformer(nn.Module):
    linear_precision = "fp32"
    # the spatial attention's patch queries, forward / backward: "fp32" (exact, default), "bf16" or "fp16" (see the module docstring)
    attention_precision = "fp32"
    attention_backward_precision = "fp32"
    # None: no dropout (training with attn_dropout / ff_dropout > 0 is refused); an int: seeded dropout (module docstring)
    dropout_seed = None

    def __init__(self, *, dim, num_frames, num_classes=None, image_size=224, patch_size=16, channels=3, depth=12, heads=8,
                 dim_head=64, attn_dropout=0.0, ff_dropout=0.0, rotary_emb=True, shift_tokens=False):
        super().__init__()
        assert image_size % patch_size == 0, "Image dimensions must be divisible by the patch size."
        _lib.lib()
        self.heads, self.dim_head, self.patch_size, self.num_frames, self.shift_tokens = heads, dim_head, patch_size, num_frames, shift_tokens
        self.attn_dropout, self.ff_dropout = attn_dropout, ff_dropout
        self.dropout_step = 0   # training forwards drawn so far with dropout active (plain attribute, not in the state_dict)
        self.to_patch_embedding = nn.Linear(channels * patch_size ** 2, dim)
        self.cls_token = nn.Parameter(torch.randn(1, dim))
        self.use_rotary_emb = rotary_emb
        if rotary_emb:
            self.frame_rot_emb = RotaryEmbedding(dim_head)
            self.image_rot_emb = AxialRotaryEmbedding(dim_head)
        else:   # :186-187: one learned row per token of a full clip, the class token's first
            self.pos_emb = nn.Embedding(num_frames * (image_size // patch_size) ** 2 + 1, dim)
        wrap = (lambda m: _PreTokenShift(num_frames, m)) if shift_tokens else (lambda m: m)
        self.layers = nn.ModuleList([
            nn.ModuleList([_PreNorm(dim, wrap(_Attention(dim, dim_head, heads))), _PreNorm(dim, wrap(_Attention(dim, dim_head, heads))),
                           _PreNorm(dim, wrap(_FeedForward(dim)))]) for _ in range(depth)])
        self.to_out = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, 24 * 3))

    def position_table(self):
        """The learned position table (num_frames * num_patches + 1, dim) of the rotary_emb=False variant, else None."""
        return None if self.use_rotary_emb else self.pos_emb.weight

    def _frame_tables(self, f, device):
        freqs = torch.arange(f, device=device, dtype=torch.float32)[:, None] * self.frame_rot_emb.inv_freqs.to(device)[None, :]
        freqs = torch.cat((freqs, freqs), dim=-1).contiguous()     # models/rotary.py:57-61
        return freqs.sin().contiguous(), freqs.cos().contiguous()

    @staticmethod
    def _key_masks(mask, video, n):
        """(b, f) bool frame mask -> the two (b, 1 + f n) uint8 key masks of the attention calls: natural [cls | (f, n)]
        order (spatial attention) and time-permuted [cls | (n, f)] order (time attention).  Indexing only."""
        b, f = video.shape[:2]
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != (b, f) or mask.device != video.device:
            got = (f"{mask.dtype} {tuple(mask.shape)} on {mask.device}" if isinstance(mask, torch.Tensor) else type(mask).__name__)
            raise ValueError(f"TimeSformer.forward: mask must be a bool tensor of shape ({b}, {f}) on {video.device}; got {got}")
        m8 = mask.to(torch.uint8)
        nat = torch.ones(b, 1 + f * n, dtype=torch.uint8, device=video.device)
        nat[:, 1:] = m8[:, :, None].expand(b, f, n).reshape(b, f * n)
        tim = torch.ones(b, 1 + f * n, dtype=torch.uint8, device=video.device)
        tim[:, 1:] = m8[:, None, :].expand(b, n, f).reshape(b, n * f)
        return nat, tim

    def forward(self, video, mask=None):
        """mask: None, or a (b, f) bool tensor on video's device, True = valid frame (see the module docstring); anything
        else raises ValueError.
        An autograd graph (_xformer_autograd.TimeSformerFunction) is built when grad mode is on, the module is in
        training mode or `video` requires grad, and something (a parameter or `video`) requires grad.  Its forward runs the
        same kernels in the same order as the no-graph path (the output is bit-identical while dropout is not active); training
        with a dropout probability > 0 needs dropout_seed (module docstring).  Otherwise the no-graph path runs, launch for
        launch as an inference-only module would.  With dropout active the forward always goes through
        TimeSformerFunction, under no_grad too, and adds 1 to dropout_step."""
        if not self.use_rotary_emb:
            ps = self.patch_size
            X.check_table_rows("TimeSformer", self.pos_emb.weight, 1, video.shape[1], (video.shape[-2] // ps) * (video.shape[-1] // ps))
        if not video.is_cuda:
            raise _lib.HiddenPoseHipError("TimeSformer.forward needs a tensor on a HIP device; there is no CPU path")
        masks = (None, None)
        if mask is not None:
            ps = self.patch_size
            masks = self._key_masks(mask, video, (video.shape[-2] // ps) * (video.shape[-1] // ps))
        params = _xa.timesformer_params(self)
        graph, drop = _xa.training_gate(self, video, params, self.attn_dropout, self.ff_dropout, "TimeSformer", "attn_dropout",
                                        "ff_dropout")
        if graph:
            aprec, bprec = X.attention_precisions(self, self.dim_head, training=True)
            with torch.cuda.device(video.device):
                out = _xa.TimeSformerFunction.apply(video.contiguous().float(), self, X.PREC[self.linear_precision], aprec, bprec,
                                                    *masks, drop, *params)
            if drop is not None:
                self.dropout_step += 1
            return out
        with torch.no_grad():
            return self._forward_nograd(video, *masks)

    def _forward_nograd(self, video, mask_nat=None, mask_time=None):
        video = video.contiguous().float()
        b, f, c, H, W = video.shape
        ps, heads, dh = self.patch_size, self.heads, self.dim_head
        hp, wp = H // ps, W // ps
        n = hp * wp
        prec = X.PREC[self.linear_precision]
        aprec, _ = X.attention_precisions(self, dh, training=False)
        dev = video.device
        with torch.cuda.device(dev):
            if self.use_rotary_emb:
                _, x = X.embed_tokens(video, ps, self.to_patch_embedding.weight, self.to_patch_embedding.bias, self.cls_token)
                sin_s, cos_s = self.image_rot_emb.tables(hp, wp, dev)
                sin_t, cos_t = self._frame_tables(f, dev)
            else:   # the learned table goes into the token matrix once; every attention then runs without rotation
                _, x = X.assemble_tokens(video, ps, self.to_patch_embedding.weight, self.to_patch_embedding.bias, self.cls_token,
                                         self.pos_emb.weight)
                sin_s = cos_s = sin_t = cos_t = None
            ntok, dim = x.shape[1:]
            rows = b * ntok
            for time_attn, spatial_attn, ff in self.layers:
                unwrap = (lambda m: m.fn) if self.shift_tokens else (lambda m: m)
                # ---- time attention: groups = the f tokens of one patch position ('b (f n) d -> (b n) f d')
                a = unwrap(time_attn.fn)
                h = X.layernorm(x.view(rows, dim), time_attn.norm).view(b, ntok, dim)
                if self.shift_tokens:
                    h = _token_shift(h, f)
                att = X.attention(X.time_perm(h, f, n).view(rows, dim), a.to_qkv, b, ntok, heads, dh, 1, f, n, a.scale, sin_t, cos_t, prec,
                                  key_mask=mask_time, mask_patch_queries=True)
                X.linear(X.time_unperm(att, f, n).view(rows, heads * dh), a.to_out[0].weight, a.to_out[0].bias, prec, residual=x.view(rows, dim))
                # ---- spatial attention: groups = the n patches of one frame
                a = unwrap(spatial_attn.fn)
                h = X.layernorm(x.view(rows, dim), spatial_attn.norm).view(b, ntok, dim)
                if self.shift_tokens:
                    h = _token_shift(h, f)
                att = X.attention(h.view(rows, dim), a.to_qkv, b, ntok, heads, dh, 1, n, f, a.scale, sin_s, cos_s, prec,
                                  key_mask=mask_nat, mask_patch_queries=False, attention_precision=aprec)
                X.linear(att.view(rows, heads * dh), a.to_out[0].weight, a.to_out[0].bias, prec, residual=x.view(rows, dim))
                # ---- feed-forward
                m = unwrap(ff.fn)
                h = X.layernorm(x.view(rows, dim), ff.norm).view(b, ntok, dim)
                if self.shift_tokens:
                    h = _token_shift(h, f)
                X.geglu_ff(x.view(rows, dim), h.view(rows, dim), m.net[0], m.net[3], prec)
            cls = X.layernorm(x.view(rows, dim), self.to_out[0], rows=b, rows_per_batch=1, batch_stride_rows=ntok)
            return X.linear(cls, self.to_out[1].weight, self.to_out[1].bias)
