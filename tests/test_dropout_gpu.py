"""Seeded dropout of the transformer heads on the GPU (csrc/dropout_kernels.hip, the _dropout activation backwards of
csrc/sformer_backward.hip, hiddenpose_amd/_xformer_autograd.py and the three modules).

The C entries are compared BIT FOR BIT with the NumPy model of tests/dropout_ref.py (the mask is a pure function of
(seed, stream, element, p), the arithmetic one or two float32 roundings); the sublayer helpers with float64 autograd of their
formula under the kernels' own masks (bar 1e-5 rel-L2, the bar tests/test_xformers_train.py holds the attention backward to);
the modules with the reference's gradients under the same masks (tests/golden/dropout_grads.npz, tol 1e-4 as the p = 0
golden tests of tests/test_sformer_train.py and tests/test_xformers_train.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_ref as D
import test_sformer_train as SFT
import test_xformers_train as XFT
from hiddenpose_amd import _lib
from hiddenpose_amd import _xformer_autograd as xa
from test_sformer_train import _attn_ref
from test_xformers import _tp, _ts
from util import rel_l2

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 5, 1023, 4096, 4099, 70001)
FIRSTS = (0, 1, 2, 3, (1 << 34) + 1)
SEEDS = (0x9E3779B97F4A7C15, 0x0123456789ABCDEF)
STREAM = (3 << 20) | 5
GUARD = 16
SENTINEL = -12345.5
M64 = (1 << 64) - 1


def _dev():
    return torch.device("cuda")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- 1: the mask

@pytest.mark.parametrize("seed", SEEDS, ids=lambda s: "%x" % s)
def test_mask_is_the_models_bit_exact(seed):
    dev = _dev()
    for p in (0.0, 0.1, 0.5, 1.0):
        for first in FIRSTS:
            for n in NS:
                buf = torch.full((n + 2 * GUARD,), 7, dtype=torch.uint8, device=dev)
                _lib.check(_lib.lib().hp_dropout_mask(buf.data_ptr() + GUARD, n, first, p, seed, STREAM, _lib.current_stream_handle(dev)),
                           "hp_dropout_mask")
                got = buf.cpu().numpy()
                ref = D.keep_mask(n, first, p, seed, STREAM).astype(np.uint8)
                assert np.array_equal(got[GUARD:GUARD + n], ref), (p, first, n)
                assert (got[:GUARD] == 7).all() and (got[GUARD + n:] == 7).all(), (p, first, n)
    assert torch.equal(xa.dropout_mask(4099, 2, 0.5, seed, STREAM, dev).cpu(),
                       torch.from_numpy(D.keep_mask(4099, 2, 0.5, seed, STREAM).astype(np.uint8)))


# ---------------------------------------------------------------------------------------------------- 2: the forward

_INPUTS = {}


def _inputs(n):
    """x and addend of n values (made once per n and left unchanged)."""
    if n not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + n)
        _INPUTS[n] = (torch.randn(n, generator=g) * 3, torch.randn(n, generator=g))
    return _INPUTS[n]


def _placed(values, off, dev):
    """A sentinel-filled buffer with `values` at GUARD + off floats from its (256-byte aligned) start."""
    buf = torch.full((values.numel() + 2 * GUARD + 4,), SENTINEL, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[GUARD + off: GUARD + off + values.numel()] = values.to(dev)
    return buf


def _run_forward(n, first, with_addend, offs, alias, p=0.1, seed=SEEDS[0]):
    """alias: None, "x" (y = x) or "addend" (y = addend).  Returns nothing; asserts bit equality and untouched guards."""
    dev = _dev()
    ox, oa, oy = offs
    x, a = _inputs(n)
    bx = _placed(x, ox, dev)
    ba = _placed(a, oa, dev) if with_addend else None
    if alias == "x":
        by, oy = bx, ox
    elif alias == "addend":
        by, oy = ba, oa
    else:
        by = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.float32, device=dev)
    addr = lambda b, o: b.data_ptr() + 4 * (GUARD + o)
    _lib.check(_lib.lib().hp_dropout_forward(addr(bx, ox), addr(ba, oa) if with_addend else None, addr(by, oy), n, first, p, seed, STREAM,
                                             _lib.current_stream_handle(dev)), "hp_dropout_forward")
    got = by.cpu().numpy()
    ref = D.dropout(x.numpy(), a.numpy() if with_addend else None, first, p, seed, STREAM)
    what = (n, first, with_addend, offs, alias)
    assert np.array_equal(_bits(got[GUARD + oy: GUARD + oy + n]), _bits(ref)), what
    assert (got[:GUARD + oy] == SENTINEL).all() and (got[GUARD + oy + n:] == SENTINEL).all(), what
    if alias is None:   # the inputs are read only
        assert np.array_equal(_bits(bx.cpu().numpy()[GUARD + ox: GUARD + ox + n]), _bits(x.numpy())), what


OFFSETS = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2), (3, 0, 1), (1, 0, 0)]


@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: "x%d_a%d_y%d" % o)
def test_forward_is_the_models_bit_exact(offs):
    for first in FIRSTS:
        for n in NS:
            for with_addend in (False, True):
                _run_forward(n, first, with_addend, offs, None)


@pytest.mark.parametrize("alias", ["x", "addend"])
def test_forward_in_place(alias):
    for first in FIRSTS:
        for n in NS:
            for offs in ((0, 0, 0), (1, 2, 0), (3, 1, 0)):
                _run_forward(n, first, True, offs, alias)
                if alias == "x":
                    _run_forward(n, first, False, offs, alias)


def test_forward_ends_of_p():
    for p in (0.0, 1.0, 0.5):
        for first in (0, 3):
            _run_forward(4099, first, True, (0, 1, 2), None, p=p)
            _run_forward(4099, first, False, (2, 0, 0), None, p=p)


# ------------------------------------------------------------------------------------------------------- 3: slicing

def test_slices_equal_one_call():
    dev = _dev()
    n, first, p, seed = 70001, 5, 0.1, SEEDS[1]
    x, a = (t.to(dev) for t in _inputs(n))
    L, st = _lib.lib(), _lib.current_stream_handle(dev)
    whole, parts = torch.empty_like(x), torch.empty_like(x)
    _lib.check(L.hp_dropout_forward(x.data_ptr(), a.data_ptr(), whole.data_ptr(), n, first, p, seed, STREAM, st), "whole")
    cuts = (0, 1023, 1023 + 4099, n)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _lib.check(L.hp_dropout_forward(x.data_ptr() + 4 * lo, a.data_ptr() + 4 * lo, parts.data_ptr() + 4 * lo, hi - lo, first + lo, p, seed,
                                        STREAM, st), "slice")
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))
    assert np.array_equal(_bits(whole.cpu().numpy()), _bits(D.dropout(x.cpu().numpy(), a.cpu().numpy(), first, p, seed, STREAM)))


# ------------------------------------------------------------------------------------------------- 4: fused siblings

@pytest.mark.parametrize("rows,hid", [(300, 128), (37, 192), (5, 7)])
def test_geglu_backward_dropout_equals_two_passes(rows, hid):
    dev = _dev()
    g = torch.Generator().manual_seed(rows)
    u, dg = (torch.randn(rows, 2 * hid, generator=g) * 2).to(dev), torch.randn(rows, hid, generator=g).to(dev)
    drop = (SEEDS[0], 3, 0.2)
    fused = xa.geglu_backward(u, dg, drop, 5)
    two = xa.geglu_backward(u, xa.dropout(dg, drop, 5, out=torch.empty_like(dg)))
    assert torch.equal(fused.view(torch.int32), two.view(torch.int32))
    assert not torch.equal(fused, xa.geglu_backward(u, dg))
    # a du that is not 16-byte aligned takes the element path: the same bits
    L = _lib.lib()
    buf = torch.empty(rows * 2 * hid + 1, device=dev)
    _lib.check(L.hp_geglu_backward_dropout(u.data_ptr(), dg.data_ptr(), buf.data_ptr() + 4, rows, hid, 0.2, SEEDS[0] & M64,
                                           xa.dropout_stream(3, 5), _lib.current_stream_handle(dev)), "geglu_bwd_dropout")
    assert torch.equal(buf[1:].view(torch.int32), two.reshape(-1).view(torch.int32))


@pytest.mark.parametrize("n", [300 * 128, 4099])
def test_gelu_backward_dropout_equals_two_passes(n):
    dev = _dev()
    g = torch.Generator().manual_seed(n)
    u, dy = (torch.randn(n, generator=g) * 3).to(dev), torch.randn(n, generator=g).to(dev)
    drop = (SEEDS[1], 3, 0.2)
    fused = xa.gelu_backward(u, dy.clone(), drop, 8)
    two = xa.gelu_backward(u, xa.dropout(dy, drop, 8, out=torch.empty_like(dy)))
    assert torch.equal(fused.view(torch.int32), two.view(torch.int32))
    assert not torch.equal(fused, xa.gelu_backward(u, dy.clone()))


# ------------------------------------------------------------------------------------------------ 5: sublayer helpers

def _mask64(shape, p, drop, site, dev):
    """The site's keep mask from hp_dropout_mask, times 1 / (1 - p), float64 on the CPU."""
    n = int(np.prod(shape))
    m = xa.dropout_mask(n, 0, p, drop[0], xa.dropout_stream(drop[1], site), dev)
    return m.cpu().double().view(shape) / (1.0 - p)


def _f64(*ts):
    return [t.detach().cpu().double().requires_grad_(True) for t in ts]


def _report(what, pairs):
    errs = {k: rel_l2(a, b) for k, (a, b) in pairs.items()}
    print(what, {k: "%.2e" % e for k, e in errs.items()})
    assert max(errs.values()) < 1e-5, errs


@pytest.mark.parametrize("p", [0.1, 0.2])
def test_prenorm_attention_with_dropout_vs_float64(p):
    """nj = 1 class token, two groups of 25 tokens, 2 heads of 16, no rotary tables."""
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    b, nj, n, groups, heads, dh, dim = 2, 1, 25, 2, 2, 16, 64
    ntok, inner = nj + n * groups, heads * dh
    x = torch.randn(b, ntok, dim, generator=g)
    ln_w, ln_b = 1 + 0.1 * torch.randn(dim, generator=g), 0.1 * torch.randn(dim, generator=g)
    wqkv, wo = torch.randn(3 * inner, dim, generator=g) / dim ** 0.5, torch.randn(dim, inner, generator=g) / inner ** 0.5
    bo = 0.1 * torch.randn(dim, generator=g)
    dy = torch.randn(b, ntok, dim, generator=g)
    drop, site, scale, eps = (SEEDS[0], 3, p), 4, dh ** -0.5, 1e-5
    ps = [t.to(dev) for t in (ln_w, ln_b, wqkv, wo, bo)]
    x1, saved = xa.prenorm_attention_forward(x.to(dev), ps, eps, scale, heads, dh, nj, n, groups, None, None, 0, drop=drop, site=site)
    dx = dy.to(dev).clone()
    grads = xa.prenorm_attention_backward(dx, saved, ps, eps, scale, heads, dh, nj, n, groups, None, None, 0, drop=drop, site=site)
    xd, lwd, lbd, wqd, wod, bod = _f64(x, ln_w, ln_b, wqkv, wo, bo)
    h = F.layer_norm(xd, (dim,), lwd, lbd, eps)
    q, k, v = ((h @ wqd.t()).chunk(3, -1)[i].reshape(b, ntok, heads, dh).permute(0, 2, 1, 3) for i in range(3))
    att, _ = _attn_ref(q * scale, k, k, v, nj, n, groups)
    lin = att.permute(0, 2, 1, 3).reshape(b, ntok, inner) @ wod.t() + bod
    mask = _mask64((b, ntok, dim), p, drop, site, dev)
    ref = xd + lin * mask
    (ref * dy.double()).sum().backward()
    assert 0 < float((mask == 0).double().mean()) < 2 * p
    _report(f"prenorm attention p {p}:", {"y": (x1, ref.detach()), "dx": (dx, xd.grad), "ln_w": (grads[0], lwd.grad), "ln_b": (grads[1], lbd.grad),
                                         "wqkv": (grads[2], wqd.grad), "wo": (grads[3], wod.grad), "bo": (grads[4], bod.grad)})


def _ff_setup(hidden_out):
    g = torch.Generator().manual_seed(22)
    b, ntok, dim = 2, 50, 64
    hid = 4 * dim
    x = torch.randn(b, ntok, dim, generator=g)
    ln_w, ln_b = 1 + 0.1 * torch.randn(dim, generator=g), 0.1 * torch.randn(dim, generator=g)
    w1, b1 = torch.randn(hidden_out, dim, generator=g) / dim ** 0.5, 0.1 * torch.randn(hidden_out, generator=g)
    w2, b2 = torch.randn(dim, hid, generator=g) / hid ** 0.5, 0.1 * torch.randn(dim, generator=g)
    dy = torch.randn(b, ntok, dim, generator=g)
    return b, ntok, dim, hid, x, [ln_w, ln_b, w1, b1, w2, b2], dy


NAMES = ("ln_w", "ln_b", "w1", "b1", "w2", "b2")


@pytest.mark.parametrize("p", [0.1, 0.2])
def test_geglu_ff_with_dropout_vs_float64(p):
    dev = _dev()
    b, ntok, dim, hid, x, params, dy = _ff_setup(2 * 256)
    drop, site, eps = (SEEDS[1], 3, p), 2, 1e-5
    ps = [t.to(dev) for t in params]
    x1, saved = xa.geglu_ff_forward(x.to(dev), ps, eps, 0, drop=drop, site=site)
    dx = dy.to(dev).clone()
    grads = xa.geglu_ff_backward(dx, saved, ps, eps, 0, drop=drop, site=site)
    xd, *pd = _f64(x, *params)
    a, t = (F.layer_norm(xd, (dim,), pd[0], pd[1], eps) @ pd[2].t() + pd[3]).chunk(2, -1)
    ref = xd + (a * F.gelu(t) * _mask64((b, ntok, hid), p, drop, site, dev)) @ pd[4].t() + pd[5]
    (ref * dy.double()).sum().backward()
    _report(f"GEGLU feed-forward p {p}:", {"y": (x1, ref.detach()), "dx": (dx, xd.grad)} | {k: (gr, t.grad) for k, gr, t in zip(NAMES, grads, pd)})


@pytest.mark.parametrize("p", [0.1, 0.2])
def test_gelu_ff_with_dropout_vs_float64(p):
    dev = _dev()
    b, ntok, dim, hid, x, params, dy = _ff_setup(256)
    drop, site, eps = (SEEDS[1], 3, p), 2, 1e-5
    ps = [t.to(dev) for t in params]
    x1, saved = xa.gelu_ff_forward(x.to(dev), ps, eps, 0, drop=drop, site=site)
    dx = dy.to(dev).clone()
    grads = xa.gelu_ff_backward(dx, saved, ps, eps, 0, drop=drop, site=site)
    xd, *pd = _f64(x, *params)
    a = F.gelu(F.layer_norm(xd, (dim,), pd[0], pd[1], eps) @ pd[2].t() + pd[3]) * _mask64((b, ntok, hid), p, drop, site, dev)
    ref = xd + (a @ pd[4].t() + pd[5]) * _mask64((b, ntok, dim), p, drop, site + 1, dev)
    (ref * dy.double()).sum().backward()
    _report(f"GELU feed-forward p {p}:", {"y": (x1, ref.detach()), "dx": (dx, xd.grad)} | {k: (gr, t.grad) for k, gr, t in zip(NAMES, grads, pd)})


# --------------------------------------------------------------------------------- 6: modules against the reference

SEED, STEP = 1234, 3    # tests/golden/make_dropout_goldens.py
# key -> (builder -> (module, input), {dropout attribute: p}, golden_compare)
MODULES = {
    "sf_small": (lambda: SFT.build("small")[1:], dict(attn_dropout=0.1, ff_dropout=0.2), SFT.golden_compare),
    "ts_plain": (lambda: _ts("plain"), dict(attn_dropout=0.1, ff_dropout=0.2), XFT.golden_compare),
    "ts_plain_ff": (lambda: _ts("plain"), dict(attn_dropout=0.0, ff_dropout=0.2), XFT.golden_compare),
    "tp_learnable": (lambda: _tp("learnable"), dict(dropout=0.1, emb_dropout=0.2), XFT.golden_compare),
    "tp_sinefull": (lambda: _tp("sinefull"), dict(dropout=0.1, emb_dropout=0.2), XFT.golden_compare),
}


def _module(key, seed=SEED, step=STEP, probs=None):
    build, attrs, _ = MODULES[key]
    m, x = build()
    for k, v in (attrs if probs is None else probs).items():
        setattr(m, k, v)
    m.dropout_seed, m.dropout_step = seed, step
    return m.cuda().train(), x.cuda()


@pytest.mark.parametrize("key", list(MODULES))
def test_module_with_dropout_vs_reference_golden(key, golden):
    """(ts_plain_ff is 7e: a site with p = 0 keeps its index, so its neighbours' masks are those of the reference's call order.)"""
    m, x = _module(key)
    x.requires_grad_(True)
    y = m(x)
    (y * SFT.loss_weights(y.shape).float().cuda()).sum().backward()
    g = golden("dropout_grads.npz")
    ey = rel_l2(y.detach(), g[f"{key}_y"])
    grads = {k: p.grad for k, p in m.named_parameters()}
    worst = MODULES[key][2](g, key, grads, x.grad, 1e-4)
    print(f"{key}: output rel-L2 {ey:.2e}, worst gradient rel-L2 {max(worst, rel_l2(x.grad, g[f'{key}_input'])):.2e}")
    assert ey < 1e-4
    assert sorted(k for k, gr in grads.items() if gr is None) == sorted(g[f"{key}_none"].tolist())
    assert m.dropout_step == STEP + 1


# ------------------------------------------------------------------------------------------------------ 7: semantics

SEM = ["sf_small", "ts_plain", "tp_sinefull"]
ZERO = {"sf_small": dict(attn_dropout=0.0, ff_dropout=0.0), "ts_plain": dict(attn_dropout=0.0, ff_dropout=0.0),
        "tp_sinefull": dict(dropout=0.0, emb_dropout=0.0)}


@pytest.mark.parametrize("key", SEM)
def test_eval_mode_draws_nothing(key):
    """7a: a seed and p > 0 in eval mode give the bits of p = 0, on the no-graph path and on the graph path."""
    m, x = _module(key)
    m0, _ = _module(key, probs=ZERO[key])
    m.eval(), m0.eval()
    y0 = m0(x)
    y = m(x)
    assert y.grad_fn is None and torch.equal(y, y0)
    yg = m(x.clone().requires_grad_(True))
    assert yg.grad_fn is not None and torch.equal(yg, y0)
    assert m.dropout_step == STEP


@pytest.mark.parametrize("key", SEM)
def test_step_replays_and_advances(key):
    """7b, 7c: the same dropout_step gives the same bits; every training forward adds exactly 1, under no_grad too, where the
    output is a dropped one."""
    m, x = _module(key)
    m0, _ = _module(key, probs=ZERO[key])
    y0 = m0(x)
    assert m0.dropout_step == STEP      # not active: nothing drawn, nothing counted
    y1 = m(x)
    assert m.dropout_step == STEP + 1
    m.dropout_step = STEP
    y2 = m(x)
    assert torch.equal(y1, y2) and m.dropout_step == STEP + 1
    y3 = m(x)
    assert not torch.equal(y1, y3) and m.dropout_step == STEP + 2
    with torch.no_grad():
        y4 = m(x)
    assert m.dropout_step == STEP + 3 and y4.grad_fn is None
    assert not torch.equal(y4, y0) and not torch.equal(y1, y0)
    m.dropout_step = STEP
    with torch.no_grad():
        assert torch.equal(m(x), y1)      # the no-grad forward at step 3 draws step 3's masks
    assert "dropout_step" not in m.state_dict() and "dropout_seed" not in m.state_dict()


@pytest.mark.parametrize("key", SEM)
def test_without_a_seed_nothing_changes(key):
    """7d: today's refusal (type and the word "dropout") and today's no-grad path."""
    m, x = _module(key, seed=None)
    m0, _ = _module(key, seed=None, probs=ZERO[key])
    with pytest.raises(_lib.HiddenPoseHipError, match="dropout"):
        m(x)
    with torch.no_grad():
        y = m(x)
        y0 = m0(x)
    assert y.grad_fn is None and torch.equal(y, y0) and m.dropout_step == STEP
    assert torch.equal(m0(x), y0)     # p = 0: the graph path's bits are the no-graph path's
