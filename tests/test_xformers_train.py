"""TimeSformer and TokenPose-L training paths (hiddenpose_amd/_xformer_autograd.py TimeSformerFunction / TokenPoseFunction,
csrc/sformer_backward.hip hp_gelu_backward / hp_sformer_attention_backward_grouped): the oracle's float64 autograd pinned to
the reference's gradients (CPU), the two new kernels against float64 autograd, and the modules' gradients against the
reference goldens and the oracle (GPU).  Bars are those tests/test_sformer_train.py uses for the same quantities."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hiddenpose_amd import _lib
from hiddenpose_amd import _xformer_autograd as xa
from hiddenpose_amd import testing as hpt
from oracle import nlospose_oracle as O
from test_sformer_train import _attn_ref
from test_xformers import TP, TS, _tp, _ts
from util import rel_l2

HP_ERR_UNSUPPORTED = -2   # include/hiddenpose_hip.h
CASES = [("ts", t) for t in TS] + [("tp", t) for t in TP]


def build(kind, tag):
    return (_ts if kind == "ts" else _tp)(tag)


def loss_weights(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(78), dtype=torch.float64)


def oracle_forward(kind, kw, x, sd):
    if kind == "ts":
        return O.timesformer(x, sd, patch_size=kw["patch_size"], heads=kw["heads"], shift_tokens=kw.get("shift_tokens", False))
    return O.tokenpose_base(x, sd, patch_size=kw["patch_size"][0], heads=kw["heads"], num_keypoints=kw["num_keypoints"],
                            heatmap_size=kw["heatmap_size"], pos_embedding_type=kw["pos_embedding_type"])


def oracle_grads(kind, kw, m, x, device="cpu", R=None):
    """float64 autograd of the oracle: ({parameter name: grad or None}, input grad, output).  A parameter the module keeps
    frozen (requires_grad False) stays frozen."""
    names = dict(m.named_parameters())
    sd = {k: v.detach().to(device, torch.float64).requires_grad_(k in names and names[k].requires_grad) for k, v in m.state_dict().items()}
    xd = x.detach().to(device, torch.float64).requires_grad_(True)
    with torch.device(device):
        y = oracle_forward(kind, kw, xd, sd)
    R = loss_weights(y.shape) if R is None else R
    (y * R.to(device)).sum().backward()
    return {k: sd[k].grad for k in names}, xd.grad, y


def golden_compare(g, key, grads, xgrad, tol):
    worst = rel_l2(xgrad, g[f"{key}_input"])
    assert worst < tol, ("input", worst)
    for k, gr in grads.items():
        if gr is None:
            continue
        gr = gr.detach().cpu().double()
        if f"{key}/{k}" in g:
            e = rel_l2(gr, g[f"{key}/{k}"])
        else:
            idx = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).choice(gr.numel(), size=min(64, gr.numel()),
                                                                                  replace=False).astype(np.int64))
            ref_l2 = float(g[f"{key}/{k}/l2"])
            e = max(abs(float(gr.norm()) - ref_l2) / ref_l2, rel_l2(gr.reshape(-1)[idx], g[f"{key}/{k}/val"]))
        worst = max(worst, e)
        assert e < tol, (k, e)
    return worst


# ----------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("kind,tag", CASES, ids=lambda c: str(c))
def test_oracle_autograd_matches_reference_gradients(kind, tag, golden):
    m, x = build(kind, tag)
    kw = (TS if kind == "ts" else TP)[tag]
    grads, xgrad, _ = oracle_grads(kind, kw, m, x)
    g = golden("xformer_grads.npz")
    key = f"{kind}_{tag}"
    worst = golden_compare(g, key, grads, xgrad, 1e-6)
    print(f"{key}: worst rel-L2 {worst:.2e}")
    assert sorted(k for k, v in grads.items() if v is None) == sorted(g[f"{key}_none"].tolist())


@pytest.mark.parametrize("kind,tag", CASES, ids=lambda c: str(c))
def test_function_takes_every_parameter(kind, tag, golden):
    """The tensors the training path hands to autograd are the module's parameters; the ones without a reference gradient
    are exactly the frozen ones."""
    m, _ = build(kind, tag)
    ps = xa.timesformer_params(m) if kind == "ts" else xa.tokenpose_params(m)
    assert {id(p) for p in ps} == {id(p) for p in m.parameters()} and len(ps) == len(list(m.parameters()))
    frozen = sorted(k for k, p in m.named_parameters() if not p.requires_grad)
    assert frozen == sorted(golden("xformer_grads.npz")[f"{kind}_{tag}_none"].tolist())


# ----------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_gelu_backward_vs_float64():
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(6)
    u, dy = torch.randn(517, 300, generator=g) * 3, torch.randn(517, 300, generator=g)
    uc, dyc = u.to(dev), dy.to(dev)
    du = torch.empty_like(dyc)
    L = _lib.lib()
    _lib.check(L.hp_gelu_backward(uc.data_ptr(), dyc.data_ptr(), du.data_ptr(), u.numel(), _lib.current_stream_handle(dev)), "gelu_bwd")
    ud = u.double().requires_grad_(True)
    (F.gelu(ud) * dy.double()).sum().backward()
    e = rel_l2(du, ud.grad)
    print(f"gelu backward rel-L2 {e:.2e}")
    assert e < 1e-6
    alias = xa.gelu_backward(uc, dyc.clone())   # du written over dy
    assert torch.equal(alias, du)


GROUPED_CASES = [  # B, heads, dh, nj, n, groups
    (1, 2, 16, 1, 16, 37), (2, 1, 24, 0, 2, 300), (1, 2, 32, 24, 3, 50), (2, 2, 32, 1, 17, 29), (1, 2, 24, 24, 64, 5),
    (1, 3, 16, 0, 64, 7), (2, 2, 32, 0, 16, 40), (1, 2, 16, 24, 17, 11), (1, 2, 32, 1, 2, 130), (1, 2, 24, 1, 3, 100),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GROUPED_CASES, ids=lambda c: "B%d_h%d_dh%d_nj%d_n%d_g%d" % c)
def test_grouped_attention_backward_vs_float64(case):
    B, heads, dh, nj, n, groups = case
    L = _lib.lib()
    dev = torch.device("cuda")
    st = _lib.current_stream_handle(dev)
    ntok = nj + groups * n
    g = torch.Generator().manual_seed(12)
    Q, K, K0, V = (torch.randn(B, heads, ntok, dh, generator=g) * (dh ** -0.25) for _ in range(4))
    K[:, :, :nj] = K0[:, :, :nj]
    dO = torch.randn(B, ntok, heads * dh, generator=g)
    q, k, k0, v, do = (t.to(dev).contiguous() for t in (Q, K, K0, V, dO))
    out = torch.empty(B, ntok, heads * dh, device=dev)
    lse = torch.empty(B, heads, ntok, device=dev)
    ws = torch.empty(int(L.hp_sformer_attention_workspace_bytes(B, heads, dh)) // 4 + 1, device=dev)
    _lib.check(L.hp_sformer_attention_lse(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, heads,
                                          dh, ntok, nj, n, groups, ws.data_ptr(), st), "lse")
    r1 = xa.attention_backward_grouped(q, k, k0, v, out, do, lse, B, heads, dh, ntok, nj, n, groups)
    r2 = xa.attention_backward_grouped(q, k, k0, v, out, do, lse, B, heads, dh, ntok, nj, n, groups)
    rg = xa.attention_backward(q, k, k0, v, out, do, lse, B, heads, dh, ntok, nj, n, groups)
    torch.cuda.synchronize()
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    Qd, Kd, K0d, Vd = (t.to(dev, torch.float64).requires_grad_(True) for t in (Q, K, K0, V))
    ref, _ = _attn_ref(Qd, Kd, K0d, Vd, nj, n, groups)
    (ref * dO.to(dev, torch.float64).view(B, ntok, heads, dh).permute(0, 2, 1, 3)).sum().backward()
    errs = [rel_l2(a, t.grad) for a, t in zip(r1, (Qd, Kd, K0d, Vd)) if t.grad is not None]
    same = [bool(torch.equal(a, b)) for a, b in zip(r1, rg)]
    print(case, ["%.2e" % e for e in errs], "bit-equal to the generic entry (dQ, dK, dK0, dV):", same)
    assert max(errs) < 1e-5
    if nj == 0:
        assert float(r1[2].abs().max()) == 0.0


@pytest.mark.gpu
def test_grouped_attention_backward_refuses_unsupported():
    L = _lib.lib()
    dev = torch.device("cuda")
    buf = torch.zeros(1 << 16, device=dev)
    p = buf.data_ptr()
    for dh, n in ((32, 65), (64, 16)):
        ntok = 1 + 4 * n
        nb = L.hp_sformer_attention_backward_grouped_workspace_bytes(1, 1, dh, ntok, 1, 4)
        ws = torch.empty(int(nb) // 4 + 1, device=dev)
        rc = L.hp_sformer_attention_backward_grouped(p, p, p, p, p, p, p, p, p, p, p, 1, 1, dh, ntok, 1, n, 4, ws.data_ptr(), nb,
                                                     _lib.current_stream_handle(dev))
        assert rc == HP_ERR_UNSUPPORTED, (dh, n, rc)
        assert b"not built" in L.hp_last_error_string()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,tag", CASES, ids=lambda c: str(c))
def test_module_gradients_vs_reference_golden(kind, tag, golden):
    m, x = build(kind, tag)
    m = m.cuda().train()
    xc = x.cuda().requires_grad_(True)
    y = m(xc)
    (y * loss_weights(y.shape).float().cuda()).sum().backward()
    key = f"{kind}_{tag}"
    g = golden("xformer_grads.npz")
    grads = {k: p.grad for k, p in m.named_parameters()}
    worst = golden_compare(g, key, grads, xc.grad, 1e-4)
    print(f"{key}: worst gradient rel-L2 {worst:.2e}")
    assert sorted(k for k, gr in grads.items() if gr is None) == sorted(g[f"{key}_none"].tolist())


TS_CFG = dict(dim=256, num_frames=16, num_classes=10, image_size=128, patch_size=4, channels=1, depth=2, heads=8, dim_head=32)
TP_CFG = dict(feature_size=[64, 64], patch_size=[4, 4], num_keypoints=16, dim=192, depth=2, heads=8, mlp_dim=576, heatmap_dim=4096,
              heatmap_size=[64, 64], channels=128, pos_embedding_type="sine-full", hidden_heatmap_dim=384)


def _two_samples(shape, seed):
    """Batch 2: uniform noise, and a smooth moving blob (different content)."""
    x = torch.rand(shape, generator=torch.Generator().manual_seed(seed))
    H, W = shape[-2:]
    yy, xx = torch.linspace(-1, 1, H).view(H, 1), torch.linspace(-1, 1, W).view(1, W)
    lead = int(np.prod(shape[1:-2]))
    ff = torch.arange(float(lead)).view(*shape[1:-2], 1, 1) / lead
    x[1] = torch.exp(-((yy - 0.3 * ff) ** 2 + (xx + 0.4 - ff) ** 2) / 0.05)
    return x


def _config_geometry(kind, m, kw, x, out_shape):
    R = loss_weights(out_shape)
    ref, ref_x, _ = oracle_grads(kind, kw, m, x, device="cuda", R=R)
    ref = {k: (g.cpu() if g is not None else None) for k, g in ref.items()}
    ref_x = ref_x.cpu()
    torch.cuda.empty_cache()
    m = m.cuda().train()
    xc = x.cuda().requires_grad_(True)
    y = m(xc)
    (y * R.float().cuda()).sum().backward()
    errs = {k: rel_l2(p.grad, ref[k]) for k, p in m.named_parameters() if ref[k] is not None}
    assert all((p.grad is None) == (ref[k] is None) for k, p in m.named_parameters())
    worst = max(errs, key=errs.get)
    ev = [rel_l2(xc.grad[b], ref_x[b]) for b in range(2)]
    cross = rel_l2(xc.grad[1], ref_x[0])
    print(f"{kind} config geometry, batch 2: worst parameter gradient {worst} {errs[worst]:.2e}; input gradient per sample "
          f"{ev[0]:.2e} {ev[1]:.2e}, sample 1 against sample 0's reference {cross:.2e}")
    assert errs[worst] < 1e-3 and max(ev) < 1e-3
    assert cross > 100 * max(ev)


@pytest.mark.gpu
def test_timesformer_config_geometry_batch2_vs_oracle():
    """TimeSformer at dim 256, 16 frames of 128 x 128, patch 4, 1 channel, 8 heads of 32 (time attention: 1024 groups of 16
    frames per (b, head)); depth cut from 8 to 2 to keep the float64 oracle's autograd within the test's time."""
    from hiddenpose_amd.transformer import TimeSformer

    m = TimeSformer(**TS_CFG)
    hpt.fill_module(m, "timesformer.")
    with torch.no_grad():
        m.cls_token.copy_(hpt.fill_value("timesformer.cls_token", m.cls_token.shape))
    _config_geometry("ts", m, TS_CFG, _two_samples((2, 16, 1, 128, 128), 56), (2, 72))


@pytest.mark.gpu
def test_tokenpose_l_config_geometry_batch2_vs_oracle():
    """TokenPose-L as models/token_config.py configures it (the geometry of test_tokenpose_l_config_geometry_vs_oracle)."""
    from hiddenpose_amd.tokenpose import TokenPose_L_base

    m = TokenPose_L_base(**TP_CFG)
    hpt.fill_module(m, "tokenpose.")
    _config_geometry("tp", m, TP_CFG, _two_samples((2, 128, 64, 64), 57), (2, 16, 64, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("lin", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["ts", "tp"])
def test_graph_mode_output_equals_no_graph_output(kind, lin):
    if kind == "ts":
        m, x = build("ts", "shift")
    else:
        m, x = build("tp", "sinefull")
    m = m.cuda()
    m.linear_precision = lin
    x = x.cuda()
    with torch.no_grad():
        y0 = m(x)
    y1 = m.train()(x)
    assert y1.grad_fn is not None and torch.equal(y0, y1)
    y2 = m.eval()(x)
    assert y2.grad_fn is None and torch.equal(y0, y2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,tag", [("ts", "shift"), ("tp", "learnable")])
def test_sgd_steps_track_the_oracle(kind, tag):
    m, x = build(kind, tag)
    kw = (TS if kind == "ts" else TP)[tag]
    ref_p = {k: p.detach().double() for k, p in m.named_parameters()}
    bufs = {k: t.detach().double() for k, t in m.named_buffers()}
    m = m.cuda().train()
    xc = x.cuda()
    y = m(xc)
    R = loss_weights(y.shape) * 0.01
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.005, momentum=0.9)
    ref_buf = {}
    losses = []
    for _ in range(5):
        y = m(xc)
        loss = (y.double() ** 2).sum() * 0.01 + (y * R.float().cuda()).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        sd = {k: t.clone().requires_grad_(True) for k, t in ref_p.items()}
        yr = oracle_forward(kind, kw, x.double(), sd | bufs)
        ((yr ** 2).sum() * 0.01 + (yr * R).sum()).backward()
        for k, t in sd.items():   # torch.optim.SGD with momentum 0.9, in float64
            if t.grad is None:
                continue
            ref_buf[k] = t.grad if k not in ref_buf else 0.9 * ref_buf[k] + t.grad
            ref_p[k] = ref_p[k] - 0.005 * ref_buf[k]
    errs = {k: rel_l2(p, ref_p[k]) for k, p in m.named_parameters()}
    print(f"{kind}_{tag}: losses {losses}; worst parameter rel-L2 after 5 steps {max(errs.values()):.2e}")
    assert max(errs.values()) < 1e-4
    assert losses[-1] < losses[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,attr", [("ts", "attn_dropout"), ("ts", "ff_dropout"), ("tp", "dropout"), ("tp", "emb_dropout")])
def test_refusals(kind, attr):
    m, x = build(kind, "plain" if kind == "ts" else "learnable")
    m = m.cuda().train()
    setattr(m, attr, 0.1)
    with pytest.raises(_lib.HiddenPoseHipError, match="dropout"):
        m(x.cuda())
    with torch.no_grad():
        y = m(x.cuda())   # the no-graph path runs as before
    assert y.grad_fn is None
