"""The three transformer heads built at dim_head 64 (for TokenPose: dim // heads = 64) on the device: against the reference
goldens of tests/golden/head64.npz, against the float64 oracle at the config-5 geometry, graph mode against the no-graph path,
five SGD steps, and the refusals.  Bars are those of test_sformer.py / test_sformer_train.py / test_xformers_train.py."""
import pytest
import torch

from hiddenpose_amd import _lib
from hiddenpose_amd import _xformer_autograd as xa
from hiddenpose_amd import testing as hpt
from hiddenpose_amd.NlosPoseSformer import NlosPoseSformer
from test_head64 import CASES, build, golden_compare, loss_weights, oracle_forward, oracle_grads
from test_sformer_train import CFG5
from util import rel_l2


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CASES))
def test_module_forward_and_gradients_vs_reference_golden(key, golden):
    kind, kw, m, x = build(key)
    g = golden("head64.npz")
    m = m.cuda()
    y0 = m.eval()(x.cuda())
    assert y0.grad_fn is None
    e = rel_l2(y0, g[f"{key}_y"])
    m = m.train()
    xc = x.cuda().requires_grad_(True)
    y = m(xc)
    assert torch.equal(y, y0)
    (y * loss_weights(y.shape).float().cuda()).sum().backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    worst = golden_compare(g, key, grads, xc.grad, 1e-4)
    print(f"{key}: forward rel-L2 {e:.2e}, worst gradient rel-L2 {worst:.2e}")
    assert e < 1e-4
    assert sorted(k for k, gr in grads.items() if gr is None) == sorted(g[f"{key}_none"].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("key,lin,att", [("sf", "fp32", "fp32"), ("sf", "bf16", "fp16"), ("ts_plain", "fp32", None), ("ts_shift", "bf16", None),
                                         ("tp_learnable", "fp32", None), ("tp_learnable", "bf16", None)])
def test_graph_mode_output_equals_no_graph_output(key, lin, att):
    _, _, m, x = build(key)
    m = m.cuda()
    m.linear_precision = lin
    if att is not None:
        m.attention_precision = att
    x = x.cuda()
    with torch.no_grad():
        y0 = m(x)
    y1 = m.train()(x)
    assert y1.grad_fn is not None and torch.equal(y0, y1)
    y2 = m.eval()(x)   # eval mode on an input without grad: no graph
    assert y2.grad_fn is None and torch.equal(y0, y2)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CASES))
def test_sgd_steps_track_the_oracle(key):
    kind, kw, m, x = build(key)
    ref_p = {k: p.detach().double() for k, p in m.named_parameters()}
    bufs = {k: t.detach().double() for k, t in m.named_buffers()}
    m = m.cuda().train()
    xc = x.cuda()
    with torch.no_grad():
        R = loss_weights(m(xc).shape) * 0.01
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
    print(f"{key}: losses {losses}; worst parameter rel-L2 after 5 steps {max(errs.values()):.2e}")
    assert max(errs.values()) < 1e-4
    assert losses[-1] < losses[0]


@pytest.mark.gpu
def test_config5_geometry_4_heads_of_64_batch2_vs_oracle():
    """BASELINE config 5's geometry at the same inner width as its 8 x 32: 4 heads of 64, depth 2, batch 2.  Forward and
    gradients against the oracle's float64 autograd < 1e-3, each sample's video gradient far from the other sample's
    reference; forward with bf16 Linear layers and fp16 attention < 3e-2."""
    kw = CFG5 | dict(heads=4, dim_head=64, depth=2)
    m = NlosPoseSformer(**kw)
    hpt.fill_module(m, "sformer.")
    video = torch.rand(2, 16, 1, 128, 128, generator=torch.Generator().manual_seed(55))
    yy, xx = torch.linspace(-1, 1, 128).view(1, 1, 128, 1), torch.linspace(-1, 1, 128).view(1, 1, 1, 128)
    ff = torch.arange(16.0).view(16, 1, 1, 1) / 16
    video[1] = torch.exp(-((yy - 0.3 * ff) ** 2 + (xx + 0.4 - ff) ** 2) / 0.05)
    R = loss_weights((2, 24, 4, 128))
    ref, ref_v, ref_y = oracle_grads("sf", kw, m, video, device="cuda", R=R)
    ref = {k: (g.cpu() if g is not None else None) for k, g in ref.items()}
    ref_v, ref_y = ref_v.cpu(), ref_y.cpu()
    torch.cuda.empty_cache()
    m = m.cuda().train()
    v = video.cuda().requires_grad_(True)
    y = m(v)
    ef = rel_l2(y, ref_y)
    (y * R.float().cuda()).sum().backward()
    errs = {k: rel_l2(p.grad, ref[k]) for k, p in m.named_parameters() if ref[k] is not None}
    worst = max(errs, key=errs.get)
    ev = [rel_l2(v.grad[b], ref_v[b]) for b in range(2)]
    cross = rel_l2(v.grad[1], ref_v[0])
    m.linear_precision, m.attention_precision = "bf16", "fp16"
    with torch.no_grad():
        e16 = rel_l2(m(video.cuda()), ref_y)
    print(f"config 5 at 4 x 64, depth 2, batch 2: forward {ef:.2e}; worst parameter gradient {worst} {errs[worst]:.2e}; video gradient "
          f"per sample {ev[0]:.2e} {ev[1]:.2e}, sample 1 against sample 0's reference {cross:.2e}; bf16 Linear + fp16 attention "
          f"forward {e16:.2e}")
    assert ef < 1e-3
    assert errs[worst] < 1e-3 and max(ev) < 1e-3
    assert cross > 100 * max(ev)
    assert e16 < 3e-2


@pytest.mark.gpu
def test_refusals_and_the_time_attention_entry():
    kind, kw, m, x = build("sf")
    # a width that is not built: the error names the built set
    bad = NlosPoseSformer(**kw | dict(dim_head=48)).cuda()
    with pytest.raises(_lib.HiddenPoseHipError, match=r"not built \(16, 24, 32, 64\)"):
        with torch.no_grad():
            bad(x.cuda())
    with pytest.raises(_lib.HiddenPoseHipError, match=r"not built \(16, 24, 32, 64\)"):
        bad.train()(x.cuda())
    bad.attention_precision = "fp16"
    with pytest.raises(_lib.HiddenPoseHipError, match="dim_head 32 and 64"):
        with torch.no_grad():
            bad(x.cuda())
    # fp16 attention at 64 runs forward and still refuses to train
    m = m.cuda().train()
    m.attention_precision = "fp16"
    y = m(x.cuda())
    with pytest.raises(_lib.HiddenPoseHipError, match="fp32"):
        y.sum().backward()
    m.attention_precision = "fp32"
    m.attn_dropout = 0.1
    with pytest.raises(_lib.HiddenPoseHipError, match="dropout"):
        m(x.cuda())
    # TimeSformer at 64 trains through the generic backward entry: the grouped one is never called at this width
    _, _, ts, xv = build("ts_plain")
    ts = ts.cuda().train()
    calls = []
    grouped, generic = xa.attention_backward_grouped, xa.attention_backward
    xa.attention_backward_grouped = lambda *a: calls.append("grouped") or grouped(*a)
    xa.attention_backward = lambda *a: calls.append("generic") or generic(*a)
    try:
        assert xa.TIME_ATTENTION_BACKWARD == "grouped"
        ts(xv.cuda()).sum().backward()
    finally:
        xa.attention_backward_grouped, xa.attention_backward = grouped, generic
    assert calls and set(calls) == {"generic"}, calls
    assert all(p.grad is not None for p in ts.parameters())
