"""TokenPose-L: keypoint tokens + patch tokens through three stacked vanilla transformers, heat-map MLP head.

Drop-in for models/tokenpose.py `TokenPose_L_base(**kwargs)` (:66-227) and `TokenPose_L(cfg)` (:30-63):
same constructor keywords, same state_dict keys, `forward(feature (b, c, H, W)) -> (b, num_keypoints, h_hm, w_hm)`.
Patchify 'b c (h p1)(w p2) -> b (h w)(p1 p2 c)' -> Linear -> [keypoint tokens | patches] (+ position embedding;
'sine-full' re-adds it to the patch tokens before every layer but the first, :311-313) -> 3 x Transformer(depth) of
{x += MHA(LN(x)); x += W2 gelu(W1 LN(x))} -> concat of the keypoint tokens of the three stages -> LayerNorm + Linear
(+ LayerNorm + Linear) -> heat-maps.  All arithmetic in libhiddenpose_hip.so (_xformer.py); trainable through
_xformer_autograd.TokenPoseFunction (a HIP backward).  `mask` is not supported.

`attention_precision` / `attention_backward_precision` ("fp32" default, "bf16", "fp16"; NlosPoseSformer's attributes and
rules) run the all-to-all attention on the 16-bit matrix cores, forward and backward: every token is a patch query here (no
class queries, one group).  dim // heads must be 32 or 64: the reference's TokenPose-L geometry (8 heads of 24) is refused with
a 16-bit precision and runs as before otherwise.

Dropout (`dropout` / `emb_dropout`, the reference's keywords) is opt-in by seed, because the HIP path cannot draw from
torch's global generator: set `dropout_seed` to an int.  It is then ACTIVE while the module is in training mode and one of the
two probabilities is > 0: every nn.Dropout of the reference's forward is a site whose keep mask is a pure function of
(dropout_seed, dropout_step, site, element index, p) (Philox4x32-10, hp_dropout_forward), each forward draws its masks and then
adds 1 to `dropout_step` (also under torch.no_grad(), as torch's dropout follows the training flag alone), setting
`dropout_step` back replays the same masks, and the backward regenerates them: no mask is stored.  Neither attribute is part
of the state_dict.  With `dropout_seed` None nothing changes: a training forward with a probability > 0 is refused, the
no-grad path ignores dropout.  In eval mode nothing is drawn, with or without a seed.  Sites: 0 the token matrix after the position
embedding (emb_dropout); then per layer, counted through the three stages: the attention's to_out, the hidden activation after
the GELU, the feed-forward's output (all `dropout`)."""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _lib
from . import _xformer as X
from . import _xformer_autograd as _xa


class _Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


class _PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class _FeedForward(nn.Module):
    def __init__(self, dim, hidden_dim):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim), nn.Identity(), nn.Identity(), nn.Linear(hidden_dim, dim), nn.Identity())


class _Attention(nn.Module):
    def __init__(self, dim, heads=8, scale_with_head=False):
        super().__init__()
        self.heads = heads
        self.scale = (dim // heads) ** -0.5 if scale_with_head else dim ** -0.5
        self.to_qkv = nn.Linear(dim, dim * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(dim, dim), nn.Identity())


class Transformer(nn.Module):
    def __init__(self, dim, depth, heads, mlp_dim, dropout=0.0, num_keypoints=None, all_attn=False, scale_with_head=False):
        super().__init__()
        self.all_attn, self.num_keypoints = all_attn, num_keypoints
        self.layers = nn.ModuleList([
            nn.ModuleList([_Residual(_PreNorm(dim, _Attention(dim, heads, scale_with_head))),
                           _Residual(_PreNorm(dim, _FeedForward(dim, mlp_dim)))]) for _ in range(depth)])

    def run(self, x, pos, prec, aprec=0):
        """x (b, ntok, dim) -> new tensor (the input is kept: the three stages' keypoint tokens are concatenated)."""
        b, ntok, dim = x.shape
        rows = b * ntok
        x = x.clone()
        for idx, (attn, ff) in enumerate(self.layers):
            if idx > 0 and self.all_attn:
                X.add_position_embedding(x, pos, self.num_keypoints, "sine-full")
            a = attn.fn.fn
            dh = dim // a.heads
            h = X.layernorm(x.view(rows, dim), attn.fn.norm)
            # all-to-all attention = one group of ntok tokens, no class tokens, no rotary embedding
            att = X.attention(h, a.to_qkv, b, ntok, a.heads, dh, 0, ntok, 1, a.scale, None, None, prec, attention_precision=aprec)
            X.linear(att.view(rows, dim), a.to_out[0].weight, a.to_out[0].bias, prec, residual=x.view(rows, dim))
            h = X.layernorm(x.view(rows, dim), ff.fn.norm)
            X.gelu_ff(x.view(rows, dim), h, ff.fn.fn.net[0], ff.fn.fn.net[3], prec)
        return x


class TokenPose_L_base(nn.Module):
    linear_precision = "fp32"
    # the attention, forward / backward: "fp32" (exact, default), "bf16" or "fp16" (see the module docstring)
    attention_precision = "fp32"
    attention_backward_precision = "fp32"
    # None: no dropout (training with dropout / emb_dropout > 0 is refused); an int: seeded dropout (module docstring)
    dropout_seed = None

    def __init__(self, *, feature_size, patch_size, num_keypoints, dim, depth, heads, mlp_dim, apply_init=False,
                 hidden_heatmap_dim=64 * 6, heatmap_dim=64 * 48, heatmap_size=(64, 48), channels=3, dropout=0.0, emb_dropout=0.0,
                 pos_embedding_type="learnable"):
        super().__init__()
        assert feature_size[0] % patch_size[0] == 0 and feature_size[1] % patch_size[1] == 0
        assert patch_size[0] == patch_size[1], "square patches (hp_sformer_patchify)"
        assert pos_embedding_type in ("sine", "learnable", "sine-full")
        _lib.lib()
        h, w = feature_size[0] // patch_size[0], feature_size[1] // patch_size[1]
        self.num_patches = h * w
        self.patch_size, self.heatmap_size, self.num_keypoints = list(patch_size), list(heatmap_size), num_keypoints
        self.pos_embedding_type = pos_embedding_type
        self.dropout, self.emb_dropout = dropout, emb_dropout
        self.dropout_step = 0   # training forwards drawn so far with dropout active (plain attribute, not in the state_dict)
        self.all_attn = pos_embedding_type == "sine-full"
        self.keypoint_token = nn.Parameter(torch.zeros(1, num_keypoints, dim))
        if pos_embedding_type == "learnable":
            self.pos_embedding = nn.Parameter(torch.zeros(1, self.num_patches + num_keypoints, dim))
            nn.init.trunc_normal_(self.pos_embedding, std=0.02)
        else:
            self.pos_embedding = nn.Parameter(self._sine_embedding(h, w, dim), requires_grad=False)
        self.patch_to_embedding = nn.Linear(channels * patch_size[0] * patch_size[1], dim)
        mk = lambda: Transformer(dim, depth, heads, mlp_dim, dropout, num_keypoints=num_keypoints, all_attn=self.all_attn,
                                 scale_with_head=True)
        self.transformer1, self.transformer2, self.transformer3 = mk(), mk(), mk()
        self.dim_head = dim // heads
        # (:111-118; the reference's first branch needs an undefined name and a configuration it never takes)
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim * 3), nn.Linear(dim * 3, heatmap_dim))
        nn.init.trunc_normal_(self.keypoint_token, std=0.02)

    @staticmethod
    def _sine_embedding(h, w, d_model, temperature=10000, scale=2 * math.pi):
        """:146-170 (constant table, built on the host once)."""
        area = torch.ones(1, h, w)
        y_embed, x_embed = area.cumsum(1, dtype=torch.float32), area.cumsum(2, dtype=torch.float32)
        half = d_model // 2
        eps = 1e-6
        y_embed = y_embed / (y_embed[:, -1:, :] + eps) * scale
        x_embed = x_embed / (x_embed[:, :, -1:] + eps) * scale
        dim_t = torch.arange(half, dtype=torch.float32)
        dim_t = temperature ** (2 * (dim_t // 2) / half)
        pos_x, pos_y = x_embed[:, :, :, None] / dim_t, y_embed[:, :, :, None] / dim_t
        pos_x = torch.stack((pos_x[:, :, :, 0::2].sin(), pos_x[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos_y = torch.stack((pos_y[:, :, :, 0::2].sin(), pos_y[:, :, :, 1::2].cos()), dim=4).flatten(3)
        return torch.cat((pos_y, pos_x), dim=3).permute(0, 3, 1, 2).flatten(2).permute(0, 2, 1).contiguous()

    def forward(self, feature, mask=None):
        """An autograd graph (_xformer_autograd.TokenPoseFunction) is built when grad mode is on, the module is in training
        mode or `feature` requires grad, and something (a parameter or `feature`) requires grad.  Its forward runs the same
        kernels in the same order as the no-graph path (the output is bit-identical while dropout is not active); training with
        a dropout probability > 0 needs dropout_seed (module docstring).  Otherwise the no-graph path runs, launch for launch
        as an inference-only module would.  With dropout active the forward always goes through TokenPoseFunction, under
        no_grad too, and adds 1 to dropout_step."""
        assert mask is None, "masks are not supported"
        if not feature.is_cuda:
            raise _lib.HiddenPoseHipError("TokenPose.forward needs a tensor on a HIP device; there is no CPU path")
        params = _xa.tokenpose_params(self)
        graph, drop = _xa.training_gate(self, feature, params, self.dropout, self.emb_dropout, "TokenPose", "dropout", "emb_dropout")
        if graph:
            aprec, bprec = X.attention_precisions(self, self.dim_head, training=True)
            with torch.cuda.device(feature.device):
                out = _xa.TokenPoseFunction.apply(feature.contiguous().float(), self, X.PREC[self.linear_precision], aprec, bprec,
                                                  drop, *params)
            if drop is not None:
                self.dropout_step += 1
            return out
        with torch.no_grad():
            return self._forward_nograd(feature)

    def _forward_nograd(self, feature):
        feature = feature.contiguous().float()
        b, c, H, W = feature.shape
        nk, dim = self.num_keypoints, self.keypoint_token.shape[-1]
        prec = X.PREC[self.linear_precision]
        aprec, _ = X.attention_precisions(self, self.dim_head, training=False)
        dev = feature.device
        with torch.cuda.device(dev):
            pos = self.pos_embedding
            _, x = X.embed_tokens(feature.view(b, 1, c, H, W), self.patch_size[0], self.patch_to_embedding.weight,
                                  self.patch_to_embedding.bias, self.keypoint_token)
            x = X.add_position_embedding(x, pos, nk, self.pos_embedding_type)
            x1 = self.transformer1.run(x, pos, prec, aprec)
            x2 = self.transformer2.run(x1, pos, prec, aprec)
            x3 = self.transformer3.run(x2, pos, prec, aprec)
            cat = torch.cat((x1[:, :nk], x2[:, :nk], x3[:, :nk]), dim=2).contiguous().view(b * nk, 3 * dim)
            y = X.layernorm(cat, self.mlp_head[0])
            y = X.linear(y, self.mlp_head[1].weight, self.mlp_head[1].bias)
        return y.view(b, nk, self.heatmap_size[0], self.heatmap_size[1])


class TokenPose_L(nn.Module):
    """models/tokenpose.py:30-63: the same network configured from a yacs-style node (cfg.MODEL.*)."""

    def __init__(self, cfg, **kwargs):
        super().__init__()
        m = cfg.MODEL
        self.transformer = TokenPose_L_base(
            feature_size=[m.IMAGE_SIZE[1] // 4, m.IMAGE_SIZE[0] // 4], patch_size=[m.PATCH_SIZE[1], m.PATCH_SIZE[0]],
            num_keypoints=m.NUM_JOINTS, dim=m.DIM, channels=m.BASE_CHANNEL, depth=m.TRANSFORMER_DEPTH, heads=m.TRANSFORMER_HEADS,
            mlp_dim=m.DIM * m.TRANSFORMER_MLP_RATIO, apply_init=getattr(m, "INIT", False), hidden_heatmap_dim=m.HIDDEN_HEATMAP_DIM,
            heatmap_dim=m.HEATMAP_SIZE[1] * m.HEATMAP_SIZE[0], heatmap_size=[m.HEATMAP_SIZE[1], m.HEATMAP_SIZE[0]],
            pos_embedding_type=m.POS_EMBEDDING_TYPE)

    def forward(self, x):
        return self.transformer(x)
