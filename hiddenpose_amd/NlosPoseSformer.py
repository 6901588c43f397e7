"""NlosPoseSformer: divided space-time transformer head with joint tokens and axial RoPE.

Drop-in for models/NlosPoseSformer.py `NlosPoseSformer(**kwargs)` (:11-151): same constructor
keywords, same state_dict keys (including the time-attention weights that the reference allocates
but never runs, :66,:133-134), `forward(video (b, f, c, H, W)) -> (b, num_joints, 4, out_dim/4)`.
All arithmetic runs in libhiddenpose_hip.so (csrc/sformer_kernels.hip, csrc/sformer_backward.hip + the
fp32 MFMA GEMM and its convolution gradients); autograd trains it through _xformer_autograd.SformerFunction.

Dropout (`attn_dropout` / `ff_dropout`, the reference's keywords) is opt-in by seed, because the HIP path cannot draw from
torch's global generator: set `dropout_seed` to an int.  It is then ACTIVE while the module is in training mode and one of the
two probabilities is > 0: every nn.Dropout of the reference's forward is a site whose keep mask is a pure function of
(dropout_seed, dropout_step, site, element index, p) (Philox4x32-10, hp_dropout_forward), each forward draws its masks and then
adds 1 to `dropout_step` (also under torch.no_grad(), as torch's dropout follows the training flag alone), setting
`dropout_step` back replays the same masks, and the backward regenerates them: no mask is stored.  Neither attribute is part
of the state_dict.  With `dropout_seed` None nothing changes: a training forward with a probability > 0 is refused, the
no-grad path ignores dropout.  In eval mode nothing is drawn, with or without a seed.  Sites per layer: the spatial attention's
to_out (attn_dropout), then the feed-forward's hidden activation after the GEGLU (ff_dropout).

`rotary_emb=False` (:55-60, :113-119) is the learned-position variant: the module owns `pose_emb = nn.Embedding(num_frames *
num_patches + 1, dim)` (the reference's spelling, default initialisation; the checkpoint key is `pose_emb.weight`) and neither
rotary module.  The table's first ntok rows are added to the token matrix, joint tokens included, once before the first layer,
in the pass that assembles [joints | patch embedding] (hp_tokens_assemble_forward / _backward); every attention
then runs without rotation (rot_dim 0: the joint queries see K0 = K), at every attention precision.  The table has
num_frames * num_patches + 1 rows and the joint tokens take num_joints of them, so a clip fits only while num_joints + f n <=
num_frames n + 1: a longer one (a full clip, with the default 24 joints) raises IndexError before anything is launched, as the
reference's lookup does.  A shorter clip uses the table's prefix and leaves an exactly zero gradient in the rows behind it.
The precisions and dropout compose with it unchanged (the table add is not a dropout site); a frozen table gets no gradient.
"""
from __future__ import annotations

from math import log, pi

import torch
from torch import nn

from . import _lib
from . import _xformer as _xf
from . import _xformer_autograd as _xa


class RotaryEmbedding(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.register_buffer("inv_freqs", 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim)))


class AxialRotaryEmbedding(nn.Module):
    """:219-247.  tables(): (hp*wp, dim) sin / cos with every frequency duplicated pairwise."""

    def __init__(self, dim, max_freq=10):
        super().__init__()
        self.dim = dim
        self.register_buffer("scales", torch.logspace(0.0, log(max_freq / 2) / log(2), dim // 4, base=2))

    def tables(self, h, w, device):
        sc = self.scales.to(device=device, dtype=torch.float32)
        hs = torch.linspace(-1.0, 1.0, steps=h, device=device).unsqueeze(-1) * sc.unsqueeze(0) * pi
        ws = torch.linspace(-1.0, 1.0, steps=w, device=device).unsqueeze(-1) * sc.unsqueeze(0) * pi
        ang = torch.cat((hs[:, None, :].expand(h, w, -1), ws[None, :, :].expand(h, w, -1)), dim=-1)
        ang = ang.reshape(h * w, -1).repeat_interleave(2, dim=-1).contiguous()
        return ang.sin().contiguous(), ang.cos().contiguous()


class _PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.fn = fn
        self.norm = nn.LayerNorm(dim)


class _Attention(nn.Module):
    def __init__(self, dim, dim_head, heads):
        super().__init__()
        self.heads, self.dim_head, self.scale = heads, dim_head, dim_head ** -0.5
        inner = dim_head * heads
        self.to_qkv = nn.Linear(dim, inner * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Identity())


class _FeedForward(nn.Module):
    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, dim * mult * 2), nn.Identity(), nn.Identity(), nn.Linear(dim * mult, dim))


class NlosPoseSformer(nn.Module):
    # arithmetic of the transformer-layer Linear GEMMs: "fp32" (exact, default) or the bf16 matrix-core modes of
    # hp_conv_desc.precision; attention, LayerNorm, GEGLU, patch embedding and the output head stay fp32
    linear_precision = "fp32"
    # patch-token attention: "fp32" (exact-fp32 MFMA, default), "bf16" or "fp16" (16-bit matrix cores, fp32 soft-max; dim_head 32 or 64)
    attention_precision = "fp32"
    # attention backward: "fp32" (exact, default; needs attention_precision "fp32") or "bf16" / "fp16": the patch queries'
    # part of the backward on the 16-bit matrix cores (dim_head 32 or 64; the joint queries stay exact fp32), after a forward
    # at either attention_precision
    attention_backward_precision = "fp32"
    # None: no dropout (training with attn_dropout / ff_dropout > 0 is refused); an int: seeded dropout (module docstring)
    dropout_seed = None

    def __init__(self, *, dim, num_frames, num_joints=24, image_size=224, patch_size=16, channels=2, depth=12, heads=8,
                 dim_head=64, attn_dropout=0.0, ff_dropout=0.0, rotary_emb=True, out_dim=64 * 2 * 3, batch_size=2):
        super().__init__()
        assert image_size % patch_size == 0, "Image dimensions must be divisible by the patch size."
        _lib.lib()
        self.heads, self.dim_head, self.patch_size, self.num_joints = heads, dim_head, patch_size, num_joints
        self.attn_dropout, self.ff_dropout = attn_dropout, ff_dropout
        self.dropout_step = 0   # training forwards drawn so far with dropout active (plain attribute, not in the state_dict)
        patch_dim = channels * patch_size ** 2
        self.to_patch_embedding = nn.Linear(patch_dim, dim)
        self.joints_token = nn.Parameter(torch.zeros(1, num_joints, dim))
        nn.init.trunc_normal_(self.joints_token, std=0.02)
        self.use_rotary_emb = rotary_emb
        if rotary_emb:
            self.frame_rot_emb = RotaryEmbedding(dim_head)
            self.image_rot_emb = AxialRotaryEmbedding(dim_head)
        else:   # :59-60, the reference's spelling (it is the checkpoint key)
            self.pose_emb = nn.Embedding(num_frames * (image_size // patch_size) ** 2 + 1, dim)
        self.layers = nn.ModuleList([
            nn.ModuleList([_PreNorm(dim, _Attention(dim, dim_head, heads)), _PreNorm(dim, _Attention(dim, dim_head, heads)),
                           _PreNorm(dim, _FeedForward(dim))]) for _ in range(depth)])
        self.to_out = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, out_dim))

    def position_table(self):
        """The learned position table (num_frames * num_patches + 1, dim) of the rotary_emb=False variant, else None."""
        return None if self.use_rotary_emb else self.pose_emb.weight

    def forward(self, video, mask=None):
        """An autograd graph is built when grad mode is on, the module is in training mode or `video` requires grad, and
        something (a parameter or `video`) requires grad.  Its forward runs the same kernels in the same order as the
        no-graph path (the output is bit-identical while dropout is not active) and keeps what backward needs; backward needs
        either attention_precision "fp32" or a 16-bit attention_backward_precision.  Otherwise (eval mode on a plain input, or
        no_grad) the no-graph path runs, launch for launch as an inference-only module would.  With dropout active (module
        docstring) the forward always goes through SformerFunction, under no_grad too, and adds 1 to dropout_step."""
        assert mask is None, "frame masks are ignored by the reference's attention (:177-179) and not supported"
        if not self.use_rotary_emb:
            ps = self.patch_size
            _xf.check_table_rows("NlosPoseSformer", self.pose_emb.weight, self.num_joints, video.shape[1],
                                 (video.shape[-2] // ps) * (video.shape[-1] // ps))
        if not video.is_cuda:
            raise _lib.HiddenPoseHipError("NlosPoseSformer.forward needs a tensor on a HIP device; there is no CPU path")
        params = _xa.trainable_params(self)
        graph, drop = _xa.training_gate(self, video, params, self.attn_dropout, self.ff_dropout, "NlosPoseSformer", "attn_dropout",
                                        "ff_dropout")
        if graph:
            aprec, bprec = _xf.attention_precisions(self, self.dim_head, training=True)
            with torch.cuda.device(video.device):
                out = _xa.SformerFunction.apply(video.contiguous().float(), self, _xf.PREC[self.linear_precision], aprec, bprec, drop,
                                                *params)
            if drop is not None:
                self.dropout_step += 1
            return out
        with torch.no_grad():
            return self._forward_nograd(video)

    def _forward_nograd(self, video):
        L = _lib.lib()
        video = video.contiguous().float()
        b, f, c, H, W = video.shape
        ps, nj, heads, dh = self.patch_size, self.num_joints, self.heads, self.dim_head
        hp, wp = H // ps, W // ps
        n = hp * wp
        dev = video.device
        st = _lib.current_stream_handle(dev)
        prec = _xf.PREC[self.linear_precision]
        aprec, _ = _xf.attention_precisions(self, dh, training=False)
        with torch.cuda.device(dev):
            if self.use_rotary_emb:
                _, x = _xf.embed_tokens(video, ps, self.to_patch_embedding.weight, self.to_patch_embedding.bias, self.joints_token)
                sin_t, cos_t = self.image_rot_emb.tables(hp, wp, dev)
                rot_dim = sin_t.shape[-1]
            else:   # the learned table goes into the token matrix once; the attention then runs without rotation
                _, x = _xf.assemble_tokens(video, ps, self.to_patch_embedding.weight, self.to_patch_embedding.bias, self.joints_token,
                                           self.pose_emb.weight)
                sin_t, cos_t, rot_dim = None, None, 0
            ntok, dim = x.shape[1:]
            rows = b * ntok
            inner = heads * dh
            h = torch.empty_like(x)
            q = torch.empty(b, heads, ntok, dh, dtype=torch.float32, device=dev)
            k = torch.empty_like(q)
            k0 = torch.empty_like(q)
            v = torch.empty_like(q)
            att = torch.empty(b, ntok, inner, dtype=torch.float32, device=dev)
            aws = _xf.attention_workspace(b, heads, dh, dev)
            for _time_attn, spatial, ff in self.layers:
                a = spatial.fn
                _lib.check(L.hp_layernorm_forward(x.data_ptr(), h.data_ptr(), rows, dim, spatial.norm.weight.data_ptr(),
                                                  spatial.norm.bias.data_ptr(), spatial.norm.eps, 0, 0, st), "hp_layernorm_forward")
                qkv = _xf.linear(h.view(rows, dim), a.to_qkv.weight, None, prec)
                _lib.check(L.hp_sformer_qkv_prepare(qkv.data_ptr(), q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), b, ntok, heads, dh,
                                                    nj, n, a.scale, _lib.ptr(sin_t), _lib.ptr(cos_t), rot_dim, st),
                           "hp_sformer_qkv_prepare")
                _xf.attention_forward(q, k, k0, v, att, None, b, heads, dh, ntok, nj, n, f, aws, precision=aprec)
                _xf.linear(att.view(rows, inner), a.to_out[0].weight, a.to_out[0].bias, prec, residual=x.view(rows, dim))
                _lib.check(L.hp_layernorm_forward(x.data_ptr(), h.data_ptr(), rows, dim, ff.norm.weight.data_ptr(),
                                                  ff.norm.bias.data_ptr(), ff.norm.eps, 0, 0, st), "hp_layernorm_forward")
                # feed-forward: Linear -> GEGLU (in the GEMM's epilogue) -> Linear + residual
                _xf.geglu_ff(x.view(rows, dim), h.view(rows, dim), ff.fn.net[0], ff.fn.net[3], prec)
            jt = _xf.layernorm(x, self.to_out[0], rows=b * nj, rows_per_batch=nj, batch_stride_rows=ntok)
            out = _xf.linear(jt, self.to_out[1].weight, self.to_out[1].bias)
        return out.view(b, nj, 4, -1)
