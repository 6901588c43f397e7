"""NlosPoseSformer training path (hiddenpose_amd/_xformer_autograd.py, csrc/sformer_backward.hip): the oracle's float64
autograd pinned to the reference's gradients (CPU), every backward kernel against float64 autograd of its formula, and the
module's gradients against the reference goldens and the oracle (GPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hiddenpose_amd import _lib
from hiddenpose_amd import _xformer_autograd as xa
from hiddenpose_amd import testing as hpt
from hiddenpose_amd.NlosPoseSformer import NlosPoseSformer
from oracle import nlospose_oracle as O
from util import rel_l2

CFGS = {
    "small": dict(dim=64, num_frames=4, num_joints=24, image_size=32, patch_size=8, channels=1, depth=2, heads=4,
                  dim_head=16, out_dim=128),
    "mid": dict(dim=128, num_frames=3, num_joints=24, image_size=64, patch_size=4, channels=1, depth=2, heads=4,
                dim_head=32, out_dim=512),
}
CFG5 = dict(dim=256, num_frames=16, num_joints=24, image_size=128, patch_size=4, channels=1, depth=8, heads=8, dim_head=32,
            out_dim=512)


def build(tag):
    kw = CFGS[tag]
    m = NlosPoseSformer(**kw)
    hpt.fill_module(m, "sformer.")
    video = torch.rand(2, kw["num_frames"], kw["channels"], kw["image_size"], kw["image_size"],
                       generator=torch.Generator().manual_seed(77))
    return kw, m, video


def loss_weights(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(78), dtype=torch.float64)


def oracle_grads(m, video, kw, device="cpu", R=None):
    """float64 autograd of oracle.nlospose_sformer: ({parameter name: grad or None}, video grad, output)."""
    sd = {k: v.detach().to(device, torch.float64).requires_grad_(True) for k, v in m.state_dict().items()}
    v = video.detach().to(device, torch.float64).requires_grad_(True)
    with torch.device(device):   # the oracle's rotary tables are built with factory calls
        y = O.nlospose_sformer(v, {"sformer." + k: t for k, t in sd.items()}, patch_size=kw["patch_size"], heads=kw["heads"])
    R = loss_weights(y.shape) if R is None else R
    (y * R.to(device)).sum().backward()
    names = dict(m.named_parameters())
    return {k: sd[k].grad for k in names}, v.grad, y


def golden_compare(g, tag, grads, vgrad, tol):
    assert rel_l2(vgrad, g[f"{tag}_video"]) < tol
    worst = 0.0
    for k, gr in grads.items():
        if gr is None:
            continue
        gr = gr.detach().cpu().double()
        if f"{tag}/{k}" in g:
            e = rel_l2(gr, g[f"{tag}/{k}"])
        else:
            idx = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).choice(gr.numel(), size=min(64, gr.numel()),
                                                                                  replace=False).astype(np.int64))
            ref_l2 = float(g[f"{tag}/{k}/l2"])
            e = max(abs(float(gr.norm()) - ref_l2) / ref_l2, rel_l2(gr.reshape(-1)[idx], g[f"{tag}/{k}/val"]))
        worst = max(worst, e)
        assert e < tol, (k, e)
    return worst


# ----------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("tag", list(CFGS))
def test_oracle_autograd_matches_reference_gradients(tag, golden):
    kw, m, video = build(tag)
    grads, vgrad, _ = oracle_grads(m, video, kw)
    g = golden("sformer_grads.npz")
    golden_compare(g, tag, grads, vgrad, 1e-6)
    assert sorted(k for k, v in grads.items() if v is None) == sorted(g[f"{tag}_none"].tolist())


@pytest.mark.parametrize("tag", list(CFGS))
def test_trained_parameter_set_is_the_reference_one(tag, golden):
    """The parameters the training path hands to autograd are exactly those the reference gives a gradient."""
    _, m, _ = build(tag)
    ids = {id(p) for p in xa.trainable_params(m)}
    untrained = sorted(k for k, p in m.named_parameters() if id(p) not in ids)
    assert untrained == sorted(golden("sformer_grads.npz")[f"{tag}_none"].tolist())
    assert len(ids) == len(xa.trainable_params(m))


# ----------------------------------------------------------------------------------------------------------------- GPU

def _attn_ref(Q, K, K0, V, nj, n, f):
    """float64 attention of models/NlosPoseSformer.py:284-319 on prepared Q (scaled, rotated), K (rotated), K0, V."""
    B, h, ntok, dh = Q.shape
    outs = []
    lses = []
    if nj:
        s = Q[:, :, :nj] @ K0.transpose(-1, -2)
        outs.append(torch.softmax(s, -1) @ V)
        lses.append(torch.logsumexp(s, -1))
    pq = Q[:, :, nj:].reshape(B, h, f, n, dh)
    pk = K[:, :, nj:].reshape(B, h, f, n, dh)
    pv = V[:, :, nj:].reshape(B, h, f, n, dh)
    kk = torch.cat((K[:, :, None, :nj].expand(-1, -1, f, -1, -1), pk), 3)
    vv = torch.cat((V[:, :, None, :nj].expand(-1, -1, f, -1, -1), pv), 3)
    s = pq @ kk.transpose(-1, -2)
    outs.append((torch.softmax(s, -1) @ vv).reshape(B, h, f * n, dh))
    lses.append(torch.logsumexp(s, -1).reshape(B, h, f * n))
    return torch.cat(outs, 2), torch.cat(lses, 2)


ATTN_CASES = [  # B, heads, dh, nj, n, f
    (1, 2, 16, 24, 64, 2), (1, 2, 24, 24, 64, 2), (1, 2, 32, 24, 64, 2), (1, 8, 32, 24, 1024, 2), (1, 2, 32, 24, 100, 3),
    (1, 2, 32, 0, 100, 3), (2, 2, 24, 7, 50, 2), (2, 3, 16, 32, 33, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "B%d_h%d_dh%d_nj%d_n%d_f%d" % c)
def test_attention_backward_vs_float64(case):
    B, heads, dh, nj, n, f = case
    L = _lib.lib()
    dev = torch.device("cuda")
    st = _lib.current_stream_handle(dev)
    ntok = nj + f * n
    g = torch.Generator().manual_seed(11)
    Q, K, K0, V = (torch.randn(B, heads, ntok, dh, generator=g) * (dh ** -0.25) for _ in range(4))
    K[:, :, :nj] = K0[:, :, :nj]   # the joint rows of K carry no RoPE
    dO = torch.randn(B, ntok, heads * dh, generator=g)
    q, k, k0, v, do = (t.to(dev).contiguous() for t in (Q, K, K0, V, dO))
    out = torch.empty(B, ntok, heads * dh, device=dev)
    out2 = torch.empty_like(out)
    lse = torch.empty(B, heads, ntok, device=dev)
    ws = torch.empty(int(L.hp_sformer_attention_workspace_bytes(B, heads, dh)) // 4 + 1, device=dev)
    _lib.check(L.hp_sformer_attention_lse(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, heads,
                                          dh, ntok, nj, n, f, ws.data_ptr(), st), "lse")
    _lib.check(L.hp_sformer_attention(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out2.data_ptr(), B, heads, dh, ntok, nj, n,
                                      f, 0, ws.data_ptr(), st), "attention")
    assert torch.equal(out, out2)
    r1 = xa.attention_backward(q, k, k0, v, out, do, lse, B, heads, dh, ntok, nj, n, f)
    r2 = xa.attention_backward(q, k, k0, v, out, do, lse, B, heads, dh, ntok, nj, n, f)
    torch.cuda.synchronize()
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    Qd, Kd, K0d, Vd = (t.to(dev, torch.float64).requires_grad_(True) for t in (Q, K, K0, V))
    ref, ref_lse = _attn_ref(Qd, Kd, K0d, Vd, nj, n, f)
    assert rel_l2(out, ref.detach().permute(0, 2, 1, 3).reshape(B, ntok, -1)) < 1e-5
    assert rel_l2(lse, ref_lse.detach()) < 1e-6
    (ref * dO.to(dev, torch.float64).view(B, ntok, heads, dh).permute(0, 2, 1, 3)).sum().backward()
    errs = [rel_l2(a, t.grad) for a, t in zip(r1, (Qd, Kd, K0d, Vd)) if t.grad is not None]
    print(case, ["%.2e" % e for e in errs])
    assert max(errs) < 1e-5
    if nj == 0:
        assert float(r1[2].abs().max()) == 0.0


def _f64(*ts):
    return [t.detach().double().requires_grad_(True) for t in ts]


@pytest.mark.gpu
@pytest.mark.parametrize("rpb", [0, 24])
def test_layernorm_backward_vs_float64(rpb):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    B, ntok, dim = 3, 150, 96
    x = torch.randn(B, ntok, dim, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(dim, generator=g), 0.1 * torch.randn(dim, generator=g)
    rows = B * rpb if rpb else B * ntok
    dy = torch.randn(rows, dim, generator=g)
    dx0 = torch.randn(B, ntok, dim, generator=g)
    norm = torch.nn.LayerNorm(dim).to(dev)
    norm.weight.data.copy_(gamma)
    dx = dx0.to(dev).clone()
    dg, db = xa.layernorm_backward(x.to(dev), dy.to(dev), dx, norm.weight, 1e-5, rows, dim, rpb, ntok if rpb else 0)
    xd, gd, bd = _f64(x, gamma, beta)
    xs = xd[:, :rpb] if rpb else xd
    y = F.layer_norm(xs, (dim,), gd, bd, 1e-5).reshape(rows, dim)
    (y * dy.double()).sum().backward()
    assert rel_l2(dx - dx0.to(dev), xd.grad) < 1e-5
    assert rel_l2(dg, gd.grad) < 1e-5 and rel_l2(db, bd.grad) < 1e-5
    if rpb:
        assert torch.equal(dx[:, rpb:], dx0[:, rpb:].to(dev))   # rows the head does not read keep their gradient


@pytest.mark.gpu
def test_geglu_qkv_prepare_unpatchify_backward_vs_float64():
    dev = torch.device("cuda")
    L = _lib.lib()
    st = _lib.current_stream_handle(dev)
    g = torch.Generator().manual_seed(4)
    # GEGLU
    u, dgg = torch.randn(300, 256, generator=g) * 2, torch.randn(300, 128, generator=g)
    du = xa.geglu_backward(u.to(dev), dgg.to(dev))
    (ud,) = _f64(u)
    a, t = ud.chunk(2, -1)
    ((a * F.gelu(t)) * dgg.double()).sum().backward()
    assert rel_l2(du, ud.grad) < 1e-6
    # qkv split + scale + axial RoPE
    B, heads, dh, nj, hp, wp, f = 2, 3, 32, 24, 4, 5, 2
    n = hp * wp
    ntok = nj + f * n
    m = NlosPoseSformer(dim=64, num_frames=f, dim_head=dh, heads=heads)
    sin_t, cos_t = m.image_rot_emb.tables(hp, wp, dev)
    rd = sin_t.shape[-1]
    qkv = torch.randn(B, ntok, 3 * heads * dh, generator=g)
    grads = [torch.randn(B, heads, ntok, dh, generator=g) for _ in range(4)]
    dqkv = torch.empty(B, ntok, 3 * heads * dh, device=dev)
    gd = [t.to(dev) for t in grads]
    _lib.check(L.hp_sformer_qkv_prepare_backward(gd[0].data_ptr(), gd[1].data_ptr(), gd[2].data_ptr(), gd[3].data_ptr(), dqkv.data_ptr(), B,
                                                 ntok, heads, dh, nj, n, dh ** -0.5, sin_t.data_ptr(), cos_t.data_ptr(), rd, st), "prep")
    (qd,) = _f64(qkv)
    q, k, v = (t.reshape(B, ntok, heads, dh).permute(0, 2, 1, 3) for t in qd.chunk(3, -1))
    q = q * dh ** -0.5
    sn, cs = sin_t.cpu().double(), cos_t.cpu().double()
    rot = lambda t: torch.cat((t[..., :rd] * cs + O._rotate_every_two(t[..., :rd]) * sn, t[..., rd:]), -1)
    Qr = torch.cat((q[:, :, :nj], rot(q[:, :, nj:].reshape(B, heads, f, n, dh)).reshape(B, heads, f * n, dh)), 2)
    Kr = torch.cat((k[:, :, :nj], rot(k[:, :, nj:].reshape(B, heads, f, n, dh)).reshape(B, heads, f * n, dh)), 2)
    sum(((a * b.double()).sum() for a, b in zip((Qr, Kr, k, v), grads))).backward()
    assert rel_l2(dqkv, qd.grad) < 1e-6
    # unpatchify
    video = torch.rand(2, 3, 2, 16, 24, generator=g)
    dtok = torch.randn(2 * 3 * 4 * 6, 4 * 4 * 2, generator=g)
    dv = torch.empty(2, 3, 2, 16, 24, device=dev)
    dtd = dtok.to(dev)
    _lib.check(L.hp_sformer_unpatchify(dtd.data_ptr(), dv.data_ptr(), 2, 3, 2, 16, 24, 4, st), "unpatchify")
    (vd,) = _f64(video)
    tok = vd.reshape(2, 3, 2, 4, 4, 6, 4).permute(0, 1, 3, 5, 4, 6, 2).reshape(-1, 32)
    (tok * dtok.double()).sum().backward()
    assert torch.equal(dv.cpu(), vd.grad.float())


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", [(16, 256), (64, 768), (256, 1024), (1024, 256), (256, 2048), (2048, 64), (256, 16)])
def test_linear_backward_vs_float64(K, N):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(K + N)
    M = 517
    x, w, dy = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(M, N, generator=g)
    ref_dx, ref_dw, ref_db = dy.double() @ w.double(), dy.double().t() @ x.double(), dy.double().sum(0)
    for prec, tol in ((0, 1e-6), (2, 1e-5), (1, 1e-2)):
        dx, dw, db = xa.linear_backward(x.to(dev), dy.to(dev), w.to(dev), prec)
        e = (rel_l2(dx, ref_dx), rel_l2(dw, ref_dw), rel_l2(db, ref_db))
        assert max(e) < tol, (prec, e)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CFGS))
def test_module_gradients_vs_reference_golden(tag, golden):
    kw, m, video = build(tag)
    m = m.cuda().train()
    v = video.cuda().requires_grad_(True)
    y = m(v)
    (y * loss_weights(y.shape).float().cuda()).sum().backward()
    g = golden("sformer_grads.npz")
    grads = {k: p.grad for k, p in m.named_parameters()}
    worst = golden_compare(g, tag, grads, v.grad, 1e-4)
    print(f"{tag}: worst gradient rel-L2 {worst:.2e}")
    none = sorted(k for k, gr in grads.items() if gr is None)
    assert none == sorted(g[f"{tag}_none"].tolist())
    assert all(k.split(".")[2] == "0" for k in none)
    assert float(m.joints_token.grad.abs().max()) > 0


@pytest.mark.gpu
def test_module_gradients_config5_batch2_vs_oracle():
    m = NlosPoseSformer(**CFG5)
    hpt.fill_module(m, "sformer.")
    video = torch.rand(2, 16, 1, 128, 128, generator=torch.Generator().manual_seed(55))
    yy, xx = torch.linspace(-1, 1, 128).view(1, 1, 128, 1), torch.linspace(-1, 1, 128).view(1, 1, 1, 128)
    ff = torch.arange(16.0).view(16, 1, 1, 1) / 16
    video[1] = torch.exp(-((yy - 0.3 * ff) ** 2 + (xx + 0.4 - ff) ** 2) / 0.05)
    R = loss_weights((2, 24, 4, 128))
    ref, ref_v, _ = oracle_grads(m, video, CFG5, device="cuda", R=R)
    ref = {k: (g.cpu() if g is not None else None) for k, g in ref.items()}
    ref_v = ref_v.cpu()
    torch.cuda.empty_cache()
    m = m.cuda().train()
    v = video.cuda().requires_grad_(True)
    y = m(v)
    (y * R.float().cuda()).sum().backward()
    errs = {k: rel_l2(p.grad, ref[k]) for k, p in m.named_parameters() if ref[k] is not None}
    worst = max(errs, key=errs.get)
    ev = [rel_l2(v.grad[b], ref_v[b]) for b in range(2)]
    cross = rel_l2(v.grad[1], ref_v[0])
    print(f"config 5, batch 2: worst parameter gradient {worst} {errs[worst]:.2e}; video gradient per sample {ev[0]:.2e} {ev[1]:.2e}, "
          f"sample 1 against sample 0's reference {cross:.2e}")
    assert errs[worst] < 1e-3 and max(ev) < 1e-3
    assert cross > 100 * max(ev)


@pytest.mark.gpu
@pytest.mark.parametrize("lin,att", [("fp32", "fp32"), ("bf16", "fp16")])
def test_graph_mode_output_equals_no_graph_output(lin, att):
    m = NlosPoseSformer(**CFG5 | dict(depth=2, num_frames=4))
    hpt.fill_module(m, "sformer.")
    m = m.cuda()
    m.linear_precision, m.attention_precision = lin, att
    video = torch.rand(2, 4, 1, 128, 128, generator=torch.Generator().manual_seed(9)).cuda()
    with torch.no_grad():
        y0 = m(video)
    y1 = m.train()(video)
    assert y1.grad_fn is not None and torch.equal(y0, y1)
    y2 = m.eval()(video)   # eval mode on an input without grad: no graph
    assert y2.grad_fn is None and torch.equal(y0, y2)


@pytest.mark.gpu
def test_sgd_steps_track_the_oracle():
    kw, m, video = build("small")
    ref_m = NlosPoseSformer(**kw)
    ref_m.load_state_dict(m.state_dict())
    m = m.cuda().train()
    vid = video.cuda()
    R = loss_weights((2, 24, 4, 32)) * 0.01
    opt = torch.optim.SGD(m.parameters(), lr=0.005, momentum=0.9)
    ref_p = {k: p.detach().double() for k, p in ref_m.named_parameters()}
    ref_buf = {}
    losses = []
    for _ in range(5):
        y = m(vid)
        loss = (y.double() ** 2).sum() * 0.01 + (y * R.float().cuda()).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        sd = {k: t.clone().requires_grad_(True) for k, t in ref_p.items()}
        bufs = {k: t.double() for k, t in ref_m.named_buffers()}
        yr = O.nlospose_sformer(video.double(), {"sformer." + k: t for k, t in (sd | bufs).items()},
                                patch_size=kw["patch_size"], heads=kw["heads"])
        ((yr ** 2).sum() * 0.01 + (yr * R).sum()).backward()
        for k, t in sd.items():   # torch.optim.SGD with momentum 0.9, in float64
            if t.grad is None:
                continue
            ref_buf[k] = t.grad if k not in ref_buf else 0.9 * ref_buf[k] + t.grad
            ref_p[k] = ref_p[k] - 0.005 * ref_buf[k]
    errs = {k: rel_l2(p, ref_p[k]) for k, p in m.named_parameters()}
    print(f"losses {losses}; worst parameter rel-L2 after 5 steps {max(errs.values()):.2e}")
    assert max(errs.values()) < 1e-4
    assert losses[-1] < losses[0]


@pytest.mark.gpu
def test_refusals():
    kw, m, video = build("mid")
    m = m.cuda().train()
    m.attention_precision = "fp16"
    y = m(video.cuda())
    with pytest.raises(_lib.HiddenPoseHipError, match="fp32"):
        y.sum().backward()
    m.attention_precision = "fp32"
    m.attn_dropout = 0.1
    with pytest.raises(_lib.HiddenPoseHipError, match="dropout"):
        m(video.cuda())
    with torch.no_grad():
        m(video.cuda())   # the no-graph path runs as before
