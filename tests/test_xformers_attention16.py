"""TimeSformer and TokenPose-L with the bf16 / fp16 MFMA attention (attention_precision / attention_backward_precision), and
the C entries under them: hp_sformer_attention_masked_p, hp_sformer_attention_lse_masked_p,
hp_sformer_attention_backward_masked_p (csrc/sformer_masked.hip, csrc/sformer_backward16.hip: k_attn16_bwd_joint_kv_masked).

Op bars are those of tests/test_attention16_train.py (OP_BAR 1e-2 / 1.5e-3, LSE_BAR 5e-4 / 5e-5) for everything a patch query
touches and those of tests/test_frame_mask.py (1e-5, lse 1e-6) for the class query's exact-fp32 rows.  `emulate` with the exact
masked float64 gradients of `_masked_attn_ref(..., mask_patch_queries=False)` for the class query gives, over OP_LAYOUTS and
the five mask patterns, a worst patch-row error of 3.9 - 4.4e-3 (bf16) and 4.8 - 5.4e-4 (fp16): 0.32 - 0.44 of the bars, and
the same for every mask pattern (the mask touches only the exact class query).

Module bars (MODULE_BAR): three times the worst error of a float64 emulation of the package's data flow, rounded up to one
digit, per (configuration, 16-bit type): (parameter gradients, input gradient, output).  The emulation (`emu_forward`) is the
oracle's float64 network with the frame mask of models/transformer.py:208-253 and, for the spatial attention's patch queries
(TokenPose: every query), Q, K, V and P rounded to the 16-bit type in the forward and `emulate`'s rule in the backward; the time
attention and the class queries are exact.  Errors are taken against the committed float64 reference goldens with
`golden_compare`'s statistic (TokenPose at dim 64 / 2 heads: against the oracle's float64 autograd).  The emulated values are
the table EMULATED below, the bars MODULE_BAR; test_module_bars_follow_the_rounding_model recomputes the former on the CPU and
checks the rule.  Worst over the six configurations: parameters 6.9e-3 (bf16) / 6.8e-4 (fp16), input gradient 8.1e-3 / 1.1e-3,
output 1.9e-3 / 2.3e-4, all on TokenPose (every query is rounded); TimeSformer 1.6e-3 / 1.6e-4, 2.5e-3 / 3.2e-4, 3.2e-4 / 3.3e-5.
The run with the fp32 forward and the fp16 backward (ts_plain: 8.1e-5, 1.9e-4, output exact) is held to the fp16 bars.

The SGD drift bar: see SGD_DRIFT_BAR."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_head64 as H64
import test_xformers_train as XT
from hiddenpose_amd import _lib
from hiddenpose_amd import testing as hpt
from oracle import nlospose_oracle as O
from test_attention16_train import LSE_BAR, OP_BAR, _inputs, emulate
from test_frame_mask import _grad_err, _masked_attn_ref, _pattern
from test_head64 import golden_compare, loss_weights
from util import rel_l2

HP_ERR_BAD_ARG, HP_ERR_UNSUPPORTED = -1, -2   # include/hiddenpose_hip.h
PREC = {"fp32": (0, None), "bf16": (1, torch.bfloat16), "fp16": (4, torch.float16)}
PATTERNS = ("prefix", "scattered", "one", "none", "all")
# B, heads, dh, nj, n, frames: tile tails below, at and past 32 / 128 keys, more than one 128-query block, nj 1 and 24
OP_LAYOUTS = [(1, 2, 32, 1, 17, 3), (2, 2, 32, 1, 33, 4), (1, 2, 32, 1, 100, 2), (1, 2, 32, 1, 300, 2), (1, 2, 64, 1, 17, 4),
              (2, 2, 64, 1, 33, 2), (1, 2, 64, 1, 100, 3), (1, 1, 64, 1, 300, 2), (1, 2, 32, 24, 33, 3)]
_lid = lambda c: "B%d_h%d_dh%d_nj%d_n%d_f%d" % c   # noqa: E731


# ------------------------------------------------------------------------------------------------ the rounding model (float64)

class _PatchAttention(torch.autograd.Function):
    """softmax(q k^T) v for one group's queries.  hf: Q, K, V and P rounded to that type in the forward (the 16-bit patch
    kernels); hb: the backward by the rule of test_attention16_train.emulate's `block` (operands of the five products, P and dS
    before their second product).  None: exact."""

    @staticmethod
    def forward(ctx, q, k, v, hf, hb):
        r = (lambda t: t.float().to(hf).double()) if hf is not None else (lambda t: t)
        ctx.save_for_backward(q, k, v)
        ctx.hb = hb
        return r(torch.softmax(r(q) @ r(k).transpose(-1, -2), -1)) @ r(v)

    @staticmethod
    def backward(ctx, g):
        q, k, v = ctx.saved_tensors
        hb = ctx.hb
        r = (lambda t: t.float().to(hb).double()) if hb is not None else (lambda t: t)
        q, k, v, g = r(q), r(k), r(v), r(g)
        p = torch.softmax(q @ k.transpose(-1, -2), -1)
        delta = (g * (p @ v)).sum(-1, keepdim=True)
        ds = p * (g @ v.transpose(-1, -2) - delta)
        p, ds = r(p), r(ds)
        return ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ g, None, None


def _emu_attention(x, sd, p, heads, groups, sin, cos, time, mask, hf, hb):
    """oracle._grouped_attention with the frame mask (b, f) bool or None (the class query leaves the tokens of padded frames
    out, the time attention's patch queries too; the spatial attention's patch queries do not) and the spatial attention's patch
    queries through _PatchAttention."""
    B, Ntok, _ = x.shape
    neg = -torch.finfo(x.dtype).max
    qkv = F.linear(x, sd[p + "to_qkv.weight"])
    inner = qkv.shape[-1] // 3
    dh = inner // heads
    q, k, v = (t.reshape(B, Ntok, heads, dh).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
    q = q * dh ** -0.5
    cq, pq, ck, pk, cv, pv = q[:, :, :1], q[:, :, 1:], k[:, :, :1], k[:, :, 1:], v[:, :, :1], v[:, :, 1:]
    per = (Ntok - 1) // groups
    f = per if time else groups
    s = cq @ k.transpose(-1, -2)
    if mask is not None:
        km = torch.cat((torch.ones(B, 1, dtype=torch.bool), mask[:, :, None].expand(B, f, (Ntok - 1) // f).reshape(B, -1)), 1)
        s = s.masked_fill(~km[:, None, None, :], neg)
    cout = torch.softmax(s, -1) @ v
    if time:
        re = lambda t: t.reshape(B, heads, f, groups, dh).transpose(2, 3)          # noqa: E731  (B, h, n, f, d)
    else:
        re = lambda t: t.reshape(B, heads, groups, per, dh)                         # noqa: E731  (B, h, f, n, d)
    pq, pk, pv = re(pq), re(pk), re(pv)
    rd = sin.shape[-1]
    rot = lambda t: torch.cat((t[..., :rd] * cos + O._rotate_every_two(t[..., :rd]) * sin, t[..., rd:]), dim=-1)   # noqa: E731
    pq, pk = rot(pq), rot(pk)
    kk = torch.cat((ck[:, :, None].expand(-1, -1, groups, -1, -1), pk), dim=3)
    vv = torch.cat((cv[:, :, None].expand(-1, -1, groups, -1, -1), pv), dim=3)
    if time:
        s = pq @ kk.transpose(-1, -2)
        if mask is not None:
            kg = torch.cat((torch.ones(B, 1, dtype=torch.bool), mask), 1)            # (B, 1 + f)
            s = s.masked_fill(~kg[:, None, None, None, :], neg)
        pout = (torch.softmax(s, -1) @ vv).transpose(2, 3)
    else:
        pout = _PatchAttention.apply(pq, kk, vv, hf, hb)
    out = torch.cat((cout, pout.reshape(B, heads, Ntok - 1, dh)), dim=2).permute(0, 2, 1, 3).reshape(B, Ntok, inner)
    return F.linear(out, sd[p + "to_out.0.weight"], sd[p + "to_out.0.bias"])


def emu_timesformer(video, sd, kw, mask=None, hf=None, hb=None):
    """oracle.timesformer (float64) with a frame mask and the rounding of the 16-bit spatial attention."""
    b, f, c, H, W = video.shape
    ps, heads, shift = kw["patch_size"], kw["heads"], kw.get("shift_tokens", False)
    hp, wp = H // ps, W // ps
    n = hp * wp
    t = video.reshape(b, f, c, hp, ps, wp, ps).permute(0, 1, 3, 5, 4, 6, 2).reshape(b, f * n, ps * ps * c)
    tok = F.linear(t, sd["to_patch_embedding.weight"], sd["to_patch_embedding.bias"])
    x = torch.cat((sd["cls_token"].expand(b, -1, -1), tok), dim=1)
    sin_s, cos_s = O.axial_rotary_tables(hp, wp, sd["image_rot_emb.scales"])
    fr = torch.arange(f, dtype=torch.float32)[:, None] * sd["frame_rot_emb.inv_freqs"][None, :]
    fr = torch.cat((fr, fr), dim=-1)
    sin_t, cos_t = fr.sin(), fr.cos()
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    fn = "fn.fn." if shift else "fn."
    sh = (lambda h: O._token_shift(h, f)) if shift else (lambda h: h)
    for i in range(depth):
        lp = f"layers.{i}."
        h = sh(F.layer_norm(x, x.shape[-1:], sd[lp + "0.norm.weight"], sd[lp + "0.norm.bias"]))
        x = x + _emu_attention(h, sd, lp + "0." + fn, heads, n, sin_t, cos_t, True, mask, None, None)
        h = sh(F.layer_norm(x, x.shape[-1:], sd[lp + "1.norm.weight"], sd[lp + "1.norm.bias"]))
        x = x + _emu_attention(h, sd, lp + "1." + fn, heads, f, sin_s, cos_s, False, mask, hf, hb)
        h = sh(F.layer_norm(x, x.shape[-1:], sd[lp + "2.norm.weight"], sd[lp + "2.norm.bias"]))
        h = F.linear(h, sd[lp + "2." + fn + "net.0.weight"], sd[lp + "2." + fn + "net.0.bias"])
        a, gates = h.chunk(2, dim=-1)
        x = x + F.linear(a * F.gelu(gates), sd[lp + "2." + fn + "net.3.weight"], sd[lp + "2." + fn + "net.3.bias"])
    cls = F.layer_norm(x[:, 0], x.shape[-1:], sd["to_out.0.weight"], sd["to_out.0.bias"])
    return F.linear(cls, sd["to_out.1.weight"], sd["to_out.1.bias"])


def emu_tokenpose(feature, sd, kw, hf=None, hb=None):
    """oracle.tokenpose_base (float64) with every query of the all-to-all attention through _PatchAttention."""
    b, c, H, W = feature.shape
    ps, heads, nk = kw["patch_size"][0], kw["heads"], kw["num_keypoints"]
    hp, wp = H // ps, W // ps
    x = feature.reshape(b, c, hp, ps, wp, ps).permute(0, 2, 4, 3, 5, 1).reshape(b, hp * wp, ps * ps * c)
    x = F.linear(x, sd["patch_to_embedding.weight"], sd["patch_to_embedding.bias"])
    n = x.shape[1]
    pos = sd["pos_embedding"]
    kt = sd["keypoint_token"].expand(b, -1, -1)
    sine = kw["pos_embedding_type"] in ("sine", "sine-full")
    x = torch.cat((kt, x + pos[:, :n]), dim=1) if sine else torch.cat((kt, x), dim=1) + pos[:, :n + nk]
    outs = []
    for tp in ("transformer1.", "transformer2.", "transformer3."):
        depth = 1 + max(int(k[len(tp):].split(".")[1]) for k in sd if k.startswith(tp + "layers."))
        for i in range(depth):
            lp = f"{tp}layers.{i}."
            if i > 0 and kw["pos_embedding_type"] == "sine-full":
                x = torch.cat((x[:, :nk], x[:, nk:] + pos), dim=1)
            h = F.layer_norm(x, x.shape[-1:], sd[lp + "0.fn.norm.weight"], sd[lp + "0.fn.norm.bias"])
            B, N, D = h.shape
            dh = D // heads
            q, k, v = (t.reshape(B, N, heads, dh).permute(0, 2, 1, 3) for t in F.linear(h, sd[lp + "0.fn.fn.to_qkv.weight"]).chunk(3, dim=-1))
            att = _PatchAttention.apply(q * dh ** -0.5, k, v, hf, hb).permute(0, 2, 1, 3).reshape(B, N, D)
            x = x + F.linear(att, sd[lp + "0.fn.fn.to_out.0.weight"], sd[lp + "0.fn.fn.to_out.0.bias"])
            h = F.layer_norm(x, x.shape[-1:], sd[lp + "1.fn.norm.weight"], sd[lp + "1.fn.norm.bias"])
            h = F.gelu(F.linear(h, sd[lp + "1.fn.fn.net.0.weight"], sd[lp + "1.fn.fn.net.0.bias"]))
            x = x + F.linear(h, sd[lp + "1.fn.fn.net.3.weight"], sd[lp + "1.fn.fn.net.3.bias"])
        outs.append(x)
    cat = torch.cat([o[:, :nk] for o in outs], dim=2)
    y = F.layer_norm(cat, cat.shape[-1:], sd["mlp_head.0.weight"], sd["mlp_head.0.bias"])
    y = F.linear(y, sd["mlp_head.1.weight"], sd["mlp_head.1.bias"])
    return y.reshape(b, nk, kw["heatmap_size"][0], kw["heatmap_size"][1])


def emu_forward(kind, kw, x, sd, mask=None, hf=None, hb=None):
    return emu_timesformer(x, sd, kw, mask, hf, hb) if kind == "ts" else emu_tokenpose(x, sd, kw, hf, hb)


def emu_grads(kind, kw, m, x, mask=None, hf=None, hb=None):
    """float64 autograd of the emulation: ({parameter name: grad or None}, input grad, output)."""
    names = dict(m.named_parameters())
    sd = {k: v.detach().double().requires_grad_(k in names and names[k].requires_grad) for k, v in m.state_dict().items()}
    xd = x.detach().double().requires_grad_(True)
    y = emu_forward(kind, kw, xd, sd, mask, hf, hb)
    (y * loss_weights(y.shape)).sum().backward()
    return {k: sd[k].grad for k in names}, xd.grad, y.detach()


TP32 = dict(feature_size=[16, 24], patch_size=[4, 4], num_keypoints=5, dim=64, depth=1, heads=2, mlp_dim=128, heatmap_dim=48,
            heatmap_size=[8, 6], channels=3, pos_embedding_type="learnable", hidden_heatmap_dim=64)   # dim // heads = 32
CONFIGS = ("ts_plain", "ts_shift", "ts_shift32", "ts_masked64", "tp_learnable", "tp_dh32")


def module_case(cfg, golden):
    """(kind, kw, module on the CPU, input, frame mask or None, golden archive or None, golden key)"""
    if cfg in ("ts_plain", "ts_shift", "tp_learnable"):
        kind, kw, m, x = H64.build(cfg)
        return kind, kw, m, x, None, golden("head64.npz"), cfg
    if cfg == "ts_shift32":
        m, x = XT.build("ts", "shift")
        return "ts", XT.TS["shift"], m, x, None, golden("xformer_grads.npz"), "ts_shift"
    if cfg == "ts_masked64":
        from test_frame_mask import _module

        g = golden("frame_mask.npz")
        kw, m, x, mask = _module(g, "dh64")
        return "ts", kw, m, x, mask, g, "dh64"
    from hiddenpose_amd.tokenpose import TokenPose_L_base

    m = TokenPose_L_base(**TP32)
    hpt.fill_module(m, "tokenpose.")
    x = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(79))
    return "tp", TP32, m, x, None, None, None


_REFS = {}


def reference(cfg, golden):
    """(compare(grads, xgrad, y) -> (worst parameter, input, output) errors, names without a gradient); computed once."""
    if cfg not in _REFS:
        kind, kw, m, x, mask, g, key = module_case(cfg, golden)
        if g is not None:
            ref_y = g[f"{key}_y"] if f"{key}_y" in g else emu_grads(kind, kw, m, x, mask)[2]

            def compare(grads, xgrad, y):
                e_in = rel_l2(xgrad, g[f"{key}_input"])
                e_p = golden_compare(g, key, grads, torch.as_tensor(g[f"{key}_input"]), float("inf"))   # parameters alone
                return e_p, e_in, rel_l2(y, ref_y)
            none = sorted(g[f"{key}_none"].tolist())
        else:
            rg, rx, ry = H64.oracle_grads(kind, kw, m, x)

            def compare(grads, xgrad, y):
                e_p = max(rel_l2(grads[k], rg[k]) for k in rg if rg[k] is not None)
                return e_p, rel_l2(xgrad, rx), rel_l2(y, ry)
            none = sorted(k for k, v in rg.items() if v is None)
        _REFS[cfg] = (compare, none)
    return _REFS[cfg]


# emulated (worst parameter gradient, input gradient, output) errors, same 16-bit type forward and backward, and the bars: three
# times those, rounded up to one digit.  test_module_bars_follow_the_rounding_model recomputes the left column on the CPU.
EMULATED = {
    ("ts_plain", "bf16"): (1.09e-03, 2.52e-03, 3.20e-04),
    ("ts_plain", "fp16"): (1.60e-04, 3.23e-04, 2.38e-05),
    ("ts_shift", "bf16"): (7.36e-04, 1.57e-03, 2.64e-04),
    ("ts_shift", "fp16"): (1.20e-04, 2.01e-04, 3.33e-05),
    ("ts_shift32", "bf16"): (3.70e-04, 8.78e-04, 1.03e-04),
    ("ts_shift32", "fp16"): (6.63e-05, 1.11e-04, 1.65e-05),
    ("ts_masked64", "bf16"): (1.62e-03, 2.24e-03, 2.23e-04),
    ("ts_masked64", "fp16"): (1.49e-04, 2.83e-04, 2.82e-05),
    ("tp_learnable", "bf16"): (3.49e-03, 6.29e-03, 1.69e-03),
    ("tp_learnable", "fp16"): (5.48e-04, 8.33e-04, 2.14e-04),
    ("tp_dh32", "bf16"): (6.85e-03, 8.13e-03, 1.86e-03),
    ("tp_dh32", "fp16"): (6.78e-04, 1.09e-03, 2.26e-04),
}
MODULE_BAR = {
    ("ts_plain", "bf16"): (4e-03, 8e-03, 1e-03),
    ("ts_plain", "fp16"): (5e-04, 1e-03, 8e-05),
    ("ts_shift", "bf16"): (3e-03, 5e-03, 8e-04),
    ("ts_shift", "fp16"): (4e-04, 7e-04, 1e-04),
    ("ts_shift32", "bf16"): (2e-03, 3e-03, 4e-04),
    ("ts_shift32", "fp16"): (2e-04, 4e-04, 5e-05),
    ("ts_masked64", "bf16"): (5e-03, 7e-03, 7e-04),
    ("ts_masked64", "fp16"): (5e-04, 9e-04, 9e-05),
    ("tp_learnable", "bf16"): (2e-02, 2e-02, 6e-03),
    ("tp_learnable", "fp16"): (2e-03, 3e-03, 7e-04),
    ("tp_dh32", "bf16"): (3e-02, 3e-02, 6e-03),
    ("tp_dh32", "fp16"): (3e-03, 4e-03, 7e-04),
}
MIXED = ("ts_plain", "fp32", "fp16")   # one run with the fp32 forward and the fp16 backward: held to the (fp16, fp16) bars
# Five SGD steps in fp16: the drift of the worst parameter from the float64 trajectory is at most the exact-fp32 path's own drift
# (held to FP32_SGD_BAR by tests/test_head64_modules.py on the same modules, loss and loop) plus the drift the 16-bit rounding adds
# (emulated in float64; three times that).  The bar is their sum rounded up to one digit, and never above ten times the fp16
# parameter-gradient bar (the cap of test_attention16_train.SGD_DRIFT_BAR).
FP32_SGD_BAR = 1e-4
SGD_DRIFT_EMULATED = {"ts_plain": 3.73e-06, "tp_learnable": 2.32e-04}
SGD_DRIFT_BAR = {"ts_plain": 2e-4, "tp_learnable": 8e-4}


def _one_digit_up(v):
    e = 10.0 ** np.floor(np.log10(v))
    return float(np.ceil(v / e - 1e-9) * e)


# ----------------------------------------------------------------------------------------------------------------- CPU

def _host_call(L, name, dh, nj, n, groups, prec, key_mask=True, mpq=0, B=1, heads=2):
    """One new entry on HOST buffers that are never dereferenced: every check below fails before the first device call."""
    ntok = nj + n * groups
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    km = p if key_mask else None
    if name == "hp_sformer_attention_masked_p":
        return L.hp_sformer_attention_masked_p(p, p, p, p, p, B, heads, dh, ntok, nj, n, groups, km, mpq, prec, p, None)
    if name == "hp_sformer_attention_lse_masked_p":
        return L.hp_sformer_attention_lse_masked_p(p, p, p, p, p, p, B, heads, dh, ntok, nj, n, groups, km, mpq, prec, p, None)
    nb = L.hp_sformer_attention_backward_masked_p_workspace_bytes(B, heads, dh, ntok, nj, groups, prec)
    return L.hp_sformer_attention_backward_masked_p(p, p, p, p, p, p, p, p, p, p, p, B, heads, dh, ntok, nj, n, groups, km, mpq, prec, p,
                                                    nb, None)


ENTRIES = ["hp_sformer_attention_masked_p", "hp_sformer_attention_lse_masked_p", "hp_sformer_attention_backward_masked_p"]


@pytest.mark.parametrize("name", ENTRIES)
def test_new_entries_check_their_arguments_without_a_device(name):
    L = _lib.lib()
    err = lambda: L.hp_last_error_string().decode()   # noqa: E731
    for prec in (0, 1, 4):
        assert _host_call(L, name, 32, 1, 8, 4, prec, key_mask=False) == HP_ERR_BAD_ARG
        assert "key_mask" in err()
        assert _host_call(L, name, 32, 0, 8, 4, prec) == HP_ERR_UNSUPPORTED
        assert "num_joints 0" in err()
    assert _host_call(L, name, 48, 1, 8, 4, 4) == HP_ERR_UNSUPPORTED
    assert "dim_head 48" in err() and "(32, 64)" in err() and name in err()
    assert _host_call(L, name, 24, 1, 8, 4, 1) == HP_ERR_UNSUPPORTED and "(32, 64)" in err()
    assert _host_call(L, name, 32, 1, 8, 4, 1, mpq=1) == HP_ERR_UNSUPPORTED
    assert "mask_patch_queries" in err() and name in err()
    assert _host_call(L, name, 64, 1, 8, 4, 4, mpq=1) == HP_ERR_UNSUPPORTED
    assert _host_call(L, name, 32, 1, 8, 4, 2) not in (0, HP_ERR_UNSUPPORTED) and "precision 2" in err()
    assert _host_call(L, name, 32, 1, 8, 4, 7) != 0 and "precision 7" in err()
    assert _host_call(L, name, 32, 33, 8, 4, 1) == HP_ERR_BAD_ARG      # num_joints > 32


def test_new_workspace_query_equals_the_unmasked_one():
    L = _lib.lib()
    for (B, heads, dh, ntok, nj, frames) in [(2, 4, 32, 1 + 6 * 16, 1, 16), (4, 8, 64, 1 + 8 * 64, 1, 64), (1, 2, 32, 24 + 3 * 50, 24, 50)]:
        for prec in (0, 1, 4):
            ref = L.hp_sformer_attention_backward_p_workspace_bytes(B, heads, dh, ntok, nj, frames, prec)
            assert ref > 0 and L.hp_sformer_attention_backward_masked_p_workspace_bytes(B, heads, dh, ntok, nj, frames, prec) == ref


def _masked_float64(Q, K, K0, V, dO, nj, n, f, km):
    """Exact float64 (out, lse, dQ, dK, dK0, dV) of the attention whose class queries apply km."""
    B, heads, ntok, dh = Q.shape
    Qd, Kd, K0d, Vd = (t.double().detach().clone().requires_grad_(True) for t in (Q, K, K0, V))
    ref, ref_lse = _masked_attn_ref(Qd, Kd, K0d, Vd, nj, n, f, km, False)
    gd = dO.double().view(B, ntok, heads, dh).permute(0, 2, 1, 3)
    (ref * gd).sum().backward()
    return ref.detach(), ref_lse.detach(), Qd.grad, Kd.grad, K0d.grad, Vd.grad


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", OP_LAYOUTS, ids=_lid)
def test_rounding_model_of_the_masked_op_stays_under_two_thirds_of_the_bar(layout, prec):
    """emulate() rounds the patch queries' operands, keeps the class query exact and knows no mask; the entries mask the class
    query alone.  Model of their result: the exact masked float64 gradients plus the patch queries' rounding error
    emulate(half) - emulate(None), in which the (unmasked) class query cancels."""
    B, heads, dh, nj, n, f = layout
    Q, K, K0, V, dO = _inputs(layout)
    g = dO.view(B, -1, heads, dh).permute(0, 2, 1, 3)
    exact = emulate(Q, K, K0, V, g, nj, n, f, None)
    em = emulate(Q, K, K0, V, g, nj, n, f, PREC[prec][1])
    worst = {}
    for pat in PATTERNS:
        km = _pattern(pat, B, nj, n, f)
        ref = _masked_float64(Q, K, K0, V, dO, nj, n, f, km)[2:]
        # the patch queries' rounded part (em - exact is their rounding error alone: the class query is exact in both) on top of
        # the exact masked gradients
        model = [r + (a - b) for r, a, b in zip(ref, em, exact)]
        scale = float(dO.double().norm())
        errs = [_grad_err(a, r, scale) for i, (a, r) in enumerate(zip(model, ref)) if i != 2]
        errs += [_grad_err(a[:, :, nj:], r[:, :, nj:], scale) for i, (a, r) in enumerate(zip(model, ref)) if i != 2]
        assert float((model[2] - ref[2]).abs().max()) < 1e-12     # dK0: the class query alone
        worst[pat] = max(errs)
    print(prec, layout, {k: "%.2e" % e for k, e in worst.items()})
    assert max(worst.values()) < OP_BAR[prec] * 2 / 3


def _emulated_errors(cfg, fwd, bwd, golden):
    kind, kw, m, x, mask, _, _ = module_case(cfg, golden)
    compare, _ = reference(cfg, golden)
    return compare(*emu_grads(kind, kw, m, x, mask, PREC[fwd][1], PREC[bwd][1]))


@pytest.mark.parametrize("cfg", CONFIGS)
def test_module_bars_follow_the_rounding_model(cfg, golden):
    compare, _ = reference(cfg, golden)
    kind, kw, m, x, mask, _, _ = module_case(cfg, golden)
    exact = compare(*emu_grads(kind, kw, m, x, mask))
    print(f"{cfg}: the exact emulation against its reference: parameters {exact[0]:.1e}, input {exact[1]:.1e}, output {exact[2]:.1e}")
    assert max(exact) < 1e-6, "the emulation without rounding is not the reference network"   # (goldens: float32-built tables)
    for prec in ("bf16", "fp16"):
        emu = _emulated_errors(cfg, prec, prec, golden)
        bar = MODULE_BAR[(cfg, prec)]
        print(f"{cfg} {prec}: emulated (parameters, input, output) " + " ".join(f"{e:.2e}" for e in emu) + " | recorded "
              + " ".join(f"{e:.2e}" for e in EMULATED[(cfg, prec)]) + " | bars " + " ".join(f"{b:.0e}" for b in bar))
        for e, rec, b in zip(emu, EMULATED[(cfg, prec)], bar):
            assert abs(e - rec) <= 0.05 * rec, "the recorded emulated value is stale"
            assert b == pytest.approx(_one_digit_up(3 * rec), rel=1e-9), "bar = 3 x emulated, rounded up to one digit"
    if cfg == MIXED[0]:
        emu = _emulated_errors(cfg, MIXED[1], MIXED[2], golden)
        print(f"{cfg} forward {MIXED[1]} backward {MIXED[2]}: emulated " + " ".join(f"{e:.2e}" for e in emu))
        assert all(3 * e <= b for e, b in zip(emu, MODULE_BAR[(cfg, MIXED[2])]))


def _sgd_emulated(cfg, golden, half, steps=5):
    """`steps` float64 SGD steps (lr 0.005, momentum 0.9; the loss of test_head64_modules.test_sgd_steps_track_the_oracle) of the
    emulation -> parameters."""
    kind, kw, m, x, mask, _, _ = module_case(cfg, golden)
    names = dict(m.named_parameters())
    p = {k: v.detach().double() for k, v in m.state_dict().items()}
    with torch.no_grad():
        R = loss_weights(emu_forward(kind, kw, x.double(), p).shape) * 0.01
    buf = {}
    for _ in range(steps):
        sd = {k: t.clone().requires_grad_(k in names and names[k].requires_grad) for k, t in p.items()}
        y = emu_forward(kind, kw, x.double(), sd, mask, half, half)
        ((y ** 2).sum() * 0.01 + (y * R).sum()).backward()
        for k, t in sd.items():
            if t.grad is None:
                continue
            buf[k] = t.grad if k not in buf else 0.9 * buf[k] + t.grad
            p[k] = p[k] - 0.005 * buf[k]
    return {k: p[k] for k in names}


_SGD_REF = {}


def sgd_reference(cfg, golden):
    if cfg not in _SGD_REF:
        _SGD_REF[cfg] = _sgd_emulated(cfg, golden, None)
    return _SGD_REF[cfg]


@pytest.mark.parametrize("cfg", ["ts_plain", "tp_learnable"])
def test_sgd_drift_bar_follows_the_rounding_model(cfg, golden):
    ref = sgd_reference(cfg, golden)
    got = _sgd_emulated(cfg, golden, torch.float16)
    drift = max(rel_l2(got[k], ref[k]) for k in ref)
    print(f"{cfg}: emulated fp16 drift of the worst parameter after 5 SGD steps {drift:.2e}; recorded {SGD_DRIFT_EMULATED[cfg]:.2e}; "
          f"bar {SGD_DRIFT_BAR[cfg]:.0e}")
    assert abs(drift - SGD_DRIFT_EMULATED[cfg]) <= 0.05 * SGD_DRIFT_EMULATED[cfg], "the recorded emulated value is stale"
    assert SGD_DRIFT_BAR[cfg] == pytest.approx(_one_digit_up(FP32_SGD_BAR + 3 * SGD_DRIFT_EMULATED[cfg]), rel=1e-9)
    assert SGD_DRIFT_BAR[cfg] <= 10 * MODULE_BAR[(cfg, "fp16")][0]   # the cap of test_attention16_train.SGD_DRIFT_BAR


# ----------------------------------------------------------------------------------------------------------------- GPU

def _ws_fwd(L, B, heads, dh, dev):
    return torch.empty(int(L.hp_sformer_attention_workspace_bytes(B, heads, dh)) // 4 + 1, device=dev)


def _forward(L, q, k, k0, v, layout, prec, km, mpq, out, lse):
    """hp_sformer_attention_lse_masked_p (lse given) / hp_sformer_attention_masked_p; km None: hp_sformer_attention_lse_p /
    hp_sformer_attention."""
    B, heads, dh, nj, n, f = layout
    ntok = nj + f * n
    st = _lib.current_stream_handle(q.device)
    ws = _ws_fwd(L, B, heads, dh, q.device)
    a = (q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr())
    d = (B, heads, dh, ntok, nj, n, f)
    if km is None and lse is None:
        _lib.check(L.hp_sformer_attention(*a, *d, prec, ws.data_ptr(), st), "hp_sformer_attention")
    elif km is None:
        _lib.check(L.hp_sformer_attention_lse_p(*a, lse.data_ptr(), *d, prec, ws.data_ptr(), st), "hp_sformer_attention_lse_p")
    elif lse is None:
        _lib.check(L.hp_sformer_attention_masked_p(*a, *d, km.data_ptr(), mpq, prec, ws.data_ptr(), st), "hp_sformer_attention_masked_p")
    else:
        _lib.check(L.hp_sformer_attention_lse_masked_p(*a, lse.data_ptr(), *d, km.data_ptr(), mpq, prec, ws.data_ptr(), st),
                   "hp_sformer_attention_lse_masked_p")


def _backward(L, q, k, k0, v, out, do, lse, layout, prec, km, mpq, grads):
    B, heads, dh, nj, n, f = layout
    ntok = nj + f * n
    st = _lib.current_stream_handle(q.device)
    a = (q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(), *(t.data_ptr() for t in grads))
    d = (B, heads, dh, ntok, nj, n, f)
    if km is None:
        nb = L.hp_sformer_attention_backward_p_workspace_bytes(*d[:4], nj, f, prec)
        ws = torch.empty(nb // 4 + 1, device=q.device)
        _lib.check(L.hp_sformer_attention_backward_p(*a, *d, prec, ws.data_ptr(), nb, st), "hp_sformer_attention_backward_p")
    else:
        nb = L.hp_sformer_attention_backward_masked_p_workspace_bytes(*d[:4], nj, f, prec)
        ws = torch.empty(nb // 4 + 1, device=q.device)
        _lib.check(L.hp_sformer_attention_backward_masked_p(*a, *d, km.data_ptr(), mpq, prec, ws.data_ptr(), nb, st),
                   "hp_sformer_attention_backward_masked_p")


def _run(L, dev, layout, tensors, prec, km_bool, mpq=0):
    """[out, lse, dQ, dK, dK0, dV, out of the inference entry] of the _masked_p entries (km_bool None: of the unmasked _p entries)."""
    B, heads, dh, nj, n, f = layout
    ntok = nj + f * n
    q, k, k0, v, do = tensors
    km = None if km_bool is None else km_bool.to(dev).to(torch.uint8).contiguous()
    out, out_inf = torch.empty(B, ntok, heads * dh, device=dev), torch.empty(B, ntok, heads * dh, device=dev)
    lse = torch.empty(B, heads, ntok, device=dev)
    grads = [torch.empty_like(q) for _ in range(4)]
    _forward(L, q, k, k0, v, layout, prec, km, mpq, out, lse)
    _forward(L, q, k, k0, v, layout, prec, km, mpq, out_inf, None)
    _backward(L, q, k, k0, v, out, do, lse, layout, prec, km, mpq, grads)
    return [out, lse, *grads, out_inf]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", OP_LAYOUTS, ids=_lid)
def test_masked_16bit_attention_vs_float64(layout):
    B, heads, dh, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + f * n
    Q, K, K0, V, dO = _inputs(layout)
    tensors = [t.to(dev).contiguous() for t in (Q, K, K0, V, dO)]
    for pat in PATTERNS:
        km = _pattern(pat, B, nj, n, f)
        ref = _masked_float64(*(t.to(dev) for t in (Q, K, K0, V, dO)), nj, n, f, km.to(dev))
        ref_out = ref[0].permute(0, 2, 1, 3).reshape(B, ntok, -1)
        scale = float(dO.double().norm())
        dead = ~km.to(dev)
        dead[:, :nj] = False
        for prec in ("bf16", "fp16"):
            r = _run(L, dev, layout, tensors, PREC[prec][0], km)
            torch.cuda.synchronize()
            e = {"out": rel_l2(r[0], ref_out), "lse": rel_l2(r[1], ref[1])}
            e.update({nm: _grad_err(a, t, scale) for nm, a, t in zip(("dQ", "dK", "dK0", "dV"), r[2:6], ref[2:6])})
            e.update({nm + " patch": _grad_err(a[:, :, nj:], t[:, :, nj:], scale) for nm, a, t in zip(("dQ", "dK", "dV"), (r[2], r[3], r[5]),
                                                                                                       (ref[2], ref[3], ref[5]))})
            x = {"out cls": rel_l2(r[0][:, :nj], ref_out[:, :nj]), "lse cls": rel_l2(r[1][:, :, :nj], ref[1][:, :, :nj]),
                 "dQ cls": _grad_err(r[2][:, :, :nj], ref[2][:, :, :nj], scale), "dK0": e["dK0"]}
            print(layout, prec, pat, " ".join(f"{a} {b:.2e}" for a, b in e.items()), "| exact part", " ".join(f"{a} {b:.2e}" for a, b in x.items()))
            assert e.pop("lse") < LSE_BAR[prec], (prec, pat)
            assert max(e.values()) < OP_BAR[prec], (prec, pat, e)
            assert x.pop("lse cls") < 1e-6 and max(x.values()) < 1e-5, (prec, pat, x)
            if bool(dead.any()):   # a masked key gets exactly zero from the class queries
                assert float(r[4][dead[:, None, :].expand(B, heads, ntok)].abs().max()) == 0.0, (prec, pat)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", OP_LAYOUTS, ids=_lid)
def test_bit_equalities(layout):
    B, heads, dh, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + f * n
    tensors = [t.to(dev).contiguous() for t in _inputs(layout, seed=12)]
    names = ("out", "lse", "dQ", "dK", "dK0", "dV", "out (inference entry)")
    km = _pattern("scattered", B, nj, n, f)
    # precision FP32 is the masked entries, both values of mask_patch_queries
    import test_frame_mask as FM
    for mpq in (0, 1):
        got = _run(L, dev, layout, tensors, 0, km, mpq)
        old = FM._run_masked(L, dev, layout, tensors, km, mpq)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, old)), ("fp32", mpq)
    ones = torch.ones(B, ntok, dtype=torch.bool)
    for prec in ("bf16", "fp16"):
        p = PREC[prec][0]
        plain = _run(L, dev, layout, tensors, p, None)
        got = _run(L, dev, layout, tensors, p, ones)
        torch.cuda.synchronize()
        same = {nm: bool(torch.equal(a, b)) for nm, a, b in zip(names, got, plain)}
        assert all(same.values()), (prec, "all-true mask against the unmasked _p entries", same)
        r1 = _run(L, dev, layout, tensors, p, km)
        r2 = _run(L, dev, layout, tensors, p, km)
        torch.cuda.synchronize()
        assert torch.equal(r1[0], r1[6]), (prec, "the inference entry's out differs from the lse entry's")
        assert all(torch.equal(a, b) for a, b in zip(r1, r2)), (prec, "two calls differ")
        assert not torch.equal(r1[0][:, :nj], plain[0][:, :nj]), "the mask did not reach the class queries"


GUARD = 64 * 1024                                  # floats either side (256 KB), as tests/test_head64.py
SENT = float.fromhex("0x1.5a5a5ap+100")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", [(2, 3, 32, 24, 37, 3), (1, 2, 64, 7, 300, 2)], ids=_lid)
def test_new_entries_write_only_their_outputs_and_read_only_their_mask(layout, prec):
    """The pattern of test_frame_mask.test_masked_entries_write_only_their_outputs_and_read_only_their_mask: outputs between
    sentinel-filled guards; key_mask is the last B * ntok bytes of its allocation behind a guard filled with 0 or 0xff."""
    B, heads, dh, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + f * n
    tensors = [t.to(dev).contiguous() for t in _inputs(layout, seed=13)]
    q, k, k0, v, do = tensors
    km_bool = _pattern("scattered", B, nj, n, f)
    p = PREC[prec][0]

    def guarded(shape):
        cnt = int(np.prod(shape))
        buf = torch.full((GUARD + cnt + GUARD,), SENT, device=dev)
        return buf, buf[GUARD:GUARD + cnt].view(shape)

    def intact(buf, t):
        return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + t.numel():] == SENT).all())

    names = ["out", "lse", "dQ", "dK", "dK0", "dV"]
    shapes = [(B, ntok, heads * dh), (B, heads, ntok)] + [(B, heads, ntok, dh)] * 4
    results = []
    for fill in (0, 255):
        mbuf = torch.full((4 * GUARD + B * ntok,), fill, dtype=torch.uint8, device=dev)
        km = mbuf[4 * GUARD:].view(B, ntok)
        km.copy_(km_bool.to(dev).to(torch.uint8))
        bufs = [guarded(s) for s in shapes]
        _forward(L, q, k, k0, v, layout, p, km, 0, bufs[0][1], bufs[1][1])
        _backward(L, q, k, k0, v, bufs[0][1], do, bufs[1][1], layout, p, km, 0, [b[1] for b in bufs[2:]])
        ibuf, inf = guarded(shapes[0])
        _forward(L, q, k, k0, v, layout, p, km, 0, inf, None)
        torch.cuda.synchronize()
        for name, (buf, t) in zip(names + ["out (inference entry)"], bufs + [(ibuf, inf)]):
            assert intact(buf, t), f"{name} was written outside its tensor"
            assert not bool((t == SENT).any()), f"{name} has unwritten elements"
            assert bool(torch.isfinite(t).all()), name
        assert bool((mbuf[:4 * GUARD] == fill).all())
        results.append([b[1].clone() for b in bufs])
    own = _run(L, dev, layout, tensors, p, km_bool)
    for res in results:
        for name, a, b in zip(names, res, own):
            assert torch.equal(a, b), (name, "depends on the bytes in front of key_mask")


def _train_run(m, x, mask):
    m.zero_grad(set_to_none=True)
    xc = x.detach().clone().requires_grad_(True)
    y = m.train()(xc) if mask is None else m.train()(xc, mask=mask)
    assert y.grad_fn is not None
    (y.double() * loss_weights(y.shape).to(y.device)).sum().backward()
    return y.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}, xc.grad.detach()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
def test_modules_vs_reference(cfg, golden):
    kind, kw, m, x, mask, _, _ = module_case(cfg, golden)
    compare, none = reference(cfg, golden)
    m, x = m.cuda(), x.cuda()
    mask = None if mask is None else mask.cuda()
    call = (lambda mod: mod(x)) if mask is None else (lambda mod: mod(x, mask=mask))
    y32 = call(m.eval())
    y_a, g_a, x_a = _train_run(m, x, mask)                      # a module that never touched the attributes
    m.attention_precision = m.attention_backward_precision = "fp32"
    y_b, g_b, x_b = _train_run(m, x, mask)
    assert torch.equal(y_a, y32) and torch.equal(y_b, y_a) and torch.equal(x_b, x_a)
    linear_w = {name + ".weight" for name, mod in m.named_modules() if isinstance(mod, torch.nn.Linear)}
    for k in g_a:   # (the Linear weight gradients' split reduction meets in fp32 atomics: test_frame_mask compares them at 1e-5)
        if g_a[k] is None or k in linear_w:
            assert g_a[k] is None and g_b[k] is None or rel_l2(g_b[k], g_a[k]) < 1e-5, k
        else:
            assert torch.equal(g_b[k], g_a[k]), k
    runs = [("bf16", "bf16"), ("fp16", "fp16")] + ([MIXED[1:]] if cfg == MIXED[0] else [])
    for fwd, bwd in runs:
        m.attention_precision, m.attention_backward_precision = fwd, bwd
        y0 = call(m.eval())
        assert y0.grad_fn is None
        y, grads, xg = _train_run(m, x, mask)
        assert torch.equal(y, y0), "graph-mode output differs from the no-graph output"
        if fwd != "fp32":
            assert not torch.equal(y0, y32), "attention_precision is ignored"
        else:
            assert torch.equal(y0, y32)
            assert not torch.equal(xg, x_a), "attention_backward_precision is ignored"
        e_p, e_in, e_y = compare(grads, xg, y)
        bar = MODULE_BAR[(cfg, bwd)]
        emu = EMULATED[(cfg, bwd)]
        print(f"{cfg} forward {fwd} backward {bwd}: parameters {e_p:.2e} input {e_in:.2e} output {e_y:.2e} | emulated "
              + " ".join(f"{v:.1e}" for v in emu) + " | bars " + " ".join(f"{v:.0e}" for v in bar))
        assert e_p < bar[0] and e_in < bar[1] and e_y < bar[2], (fwd, bwd, e_p, e_in, e_y)
        assert sorted(k for k, v in grads.items() if v is None) == none


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["ts_plain", "tp_learnable"])
def test_sgd_steps_track_the_oracle(cfg, golden):
    """Five SGD steps in fp16 (forward and backward): the loss decreases and the parameters stay within SGD_DRIFT_BAR of the
    float64 trajectory."""
    kind, kw, m, x, _, _, _ = module_case(cfg, golden)
    ref = sgd_reference(cfg, golden)
    m = m.cuda().train()
    m.attention_precision = m.attention_backward_precision = "fp16"
    xc = x.cuda()
    with torch.no_grad():
        R = loss_weights(m(xc).shape) * 0.01
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.005, momentum=0.9)
    losses = []
    for _ in range(5):
        y = m(xc)
        loss = (y.double() ** 2).sum() * 0.01 + (y * R.float().cuda()).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    errs = {k: rel_l2(p, ref[k]) for k, p in m.named_parameters()}
    print(f"{cfg}: losses {losses}; worst parameter rel-L2 after 5 steps {max(errs.values()):.2e} (bar {SGD_DRIFT_BAR[cfg]:.0e})")
    assert losses[-1] < losses[0]
    assert max(errs.values()) < SGD_DRIFT_BAR[cfg]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ts", "tp"])
def test_refusals(kind):
    from hiddenpose_amd.tokenpose import TokenPose_L_base
    from hiddenpose_amd.transformer import TimeSformer

    if kind == "ts":
        _, kw, m, x = H64.build("ts_plain")
        small = [TimeSformer(**kw | dict(dim_head=dh)) for dh in (16, 24)]
    else:
        _, kw, m, x = H64.build("tp_learnable")
        small = [TokenPose_L_base(**kw | dict(dim=dim, heads=heads)) for dim, heads in ((64, 4), (192, 8))]   # 16, and TokenPose-L's 24
    x = x.cuda()
    for bad in small:
        bad = bad.cuda()
        assert bad.eval()(x).shape[0] == 2            # runs as before with the defaults
        for attr in ("attention_precision", "attention_backward_precision"):
            bad = bad.train()
            setattr(bad, attr, "fp16")
            with pytest.raises(_lib.HiddenPoseHipError, match="dim_head 32 and 64"):
                bad(x)
            setattr(bad, attr, "fp32")
        bad.attention_precision = "bf16"
        with pytest.raises(_lib.HiddenPoseHipError, match="dim_head 32 and 64"):
            bad.eval()(x)
    m = m.cuda().train()
    for attr in ("attention_precision", "attention_backward_precision"):
        setattr(m, attr, "fp8")
        with pytest.raises(_lib.HiddenPoseHipError, match=attr):
            m(x)
        setattr(m, attr, "fp32")
    m.attention_precision = "fp8"
    with pytest.raises(_lib.HiddenPoseHipError, match="attention_precision"):
        m.eval()(x)
    m.attention_precision = "fp16"                    # a 16-bit forward with the default backward refuses at backward()
    y = m.train()(x)
    with pytest.raises(_lib.HiddenPoseHipError, match="fp32"):
        y.sum().backward()
    assert m.eval()(x).grad_fn is None                # ... and infers
