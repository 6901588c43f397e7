"""Mixed-precision training of NlosPoseSformer's attention (csrc/sformer_backward16.hip, hp_sformer_attention_lse_p,
hp_sformer_attention_backward_p, NlosPoseSformer.attention_backward_precision): the rounding model that justifies the bars
(CPU, float64), the two entries against float64, reproducibility and containment, and the module's gradients against the
reference goldens and the oracle (GPU).

Bars.  The 16-bit backward rounds the operands of the five products (Q, K, V, dO, and P and dS before their second
product) to bf16 / fp16 for the PATCH queries and keeps the joint queries exact.  `emulate` below does exactly that in
float64; over layouts with dh 32 / 64, nj 0 / 1 / 24 / 32, n 17 .. 1024 it gives dQ 3.5 - 4.4e-3, dK 3.8 - 4.3e-3, dV 2.9 - 3.6e-3
(bf16) and 4.3 - 5.5e-4, 4.9 - 5.4e-4, 3.5 - 4.4e-4 (fp16).  The op bars are the ones the 16-bit attention forward is held to
(tests/test_head64.py): 1e-2 and 1.5e-3, 2.3 x / 2.7 x over the emulated worst.  The module bars are three times the emulated
module errors (joint queries exact): parameters 4e-3 (bf16) / 5e-4 (fp16), video gradient 1.5e-2 / 2e-3."""
import numpy as np
import pytest
import torch

import test_head64 as H64
import test_sformer_train as ST
from hiddenpose_amd import _lib
from hiddenpose_amd import testing as hpt
from hiddenpose_amd.NlosPoseSformer import NlosPoseSformer
from test_sformer_train import _attn_ref
from util import rel_l2

HP_ERR_UNSUPPORTED = -2   # include/hiddenpose_hip.h
PREC = {"fp32": (0, None), "bf16": (1, torch.bfloat16), "fp16": (4, torch.float16)}
OP_BAR = {"bf16": 1e-2, "fp16": 1.5e-3}
LSE_BAR = {"bf16": 5e-4, "fp16": 5e-5}
PARAM_BAR = {"bf16": 4e-3, "fp16": 5e-4}
VIDEO_BAR = {"bf16": 1.5e-2, "fp16": 2e-3}
# emulated module errors (worst parameter, video gradient) with the joint queries exact, same 16-bit type forward and backward
EMULATED = {("mid", "bf16"): (2.0e-4, 1.1e-3), ("mid", "fp16"): (3.3e-5, 1.7e-4), ("sf", "bf16"): (1.2e-3, 5.0e-3),
            ("sf", "fp16"): (1.4e-4, 6.2e-4)}

# B, heads, dh, nj, n, frames: dh 32 / 64; nj 0 / 1 / 24 / 32; ragged n 17, 33, 100, 300 and n = 1024; 1 - 4 frames
LAYOUTS = [(1, 2, 32, 24, 64, 2), (1, 4, 32, 24, 1024, 2), (1, 2, 32, 24, 100, 3), (1, 2, 32, 0, 100, 3), (2, 2, 32, 32, 33, 4),
           (1, 2, 32, 1, 17, 1), (1, 2, 32, 24, 300, 2), (2, 3, 64, 32, 33, 2), (1, 2, 64, 24, 300, 3), (1, 2, 64, 1, 17, 4),
           (1, 2, 64, 0, 300, 1), (1, 2, 64, 24, 1024, 2), (1, 2, 64, 24, 100, 3)]


def _ids(c):
    return "B%d_h%d_dh%d_nj%d_n%d_f%d" % c


def _inputs(layout, seed=11):
    """As tests/test_sformer_train.py::test_attention_backward_vs_float64 makes them."""
    B, heads, dh, nj, n, f = layout
    ntok = nj + f * n
    g = torch.Generator().manual_seed(seed)
    Q, K, K0, V = (torch.randn(B, heads, ntok, dh, generator=g) * (dh ** -0.25) for _ in range(4))
    K[:, :, :nj] = K0[:, :, :nj]   # the joint rows of K carry no RoPE
    dO = torch.randn(B, ntok, heads * dh, generator=g)
    return Q, K, K0, V, dO


def emulate(Q, K, K0, V, dO, nj, n, f, half):
    """float64 attention backward (dQ, dK, dK0, dV) of models/NlosPoseSformer.py:284-319 on prepared Q, K, K0, V and dO
    (B, heads, ntok, dh).  half = torch.bfloat16 / torch.float16: the operands of the patch queries' five products, and P
    and dS before their second product, are rounded to that type (everything else float64); the joint queries stay exact.
    half = None: the exact formula."""
    rnd = (lambda t: t.float().to(half).double()) if half is not None else (lambda t: t)
    Qd, Kd, K0d, Vd, Gd = (t.double() for t in (Q, K, K0, V, dO))
    dq, dk, dk0, dv = (torch.zeros_like(Qd) for _ in range(4))
    ntok = Qd.shape[2]

    def block(q, k, v, g, r):
        q, k, v, g = r(q), r(k), r(v), r(g)
        p = torch.softmax(q @ k.transpose(-1, -2), -1)
        delta = (g * (p @ v)).sum(-1, keepdim=True)
        ds = p * (g @ v.transpose(-1, -2) - delta)
        p, ds = r(p), r(ds)
        return ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ g

    if nj:
        a, b_, c = block(Qd[:, :, :nj], K0d, Vd, Gd[:, :, :nj], lambda t: t)
        dq[:, :, :nj] += a
        dk0 += b_
        dv += c
    for fr in range(f):
        qi = torch.arange(nj + fr * n, nj + (fr + 1) * n, device=Q.device)
        ki = torch.cat((torch.arange(nj, device=Q.device), qi))
        a, b_, c = block(Qd[:, :, qi], Kd[:, :, ki], Vd[:, :, ki], Gd[:, :, qi], rnd)
        dq[:, :, qi] += a
        dk[:, :, ki] += b_
        dv[:, :, ki] += c
    assert dq.shape[2] == ntok
    return dq, dk, dk0, dv


def _heads_first(dO, heads):
    B, ntok, inner = dO.shape
    return dO.view(B, ntok, heads, inner // heads).permute(0, 2, 1, 3)


# ----------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", [(1, 2, 32, 24, 64, 2), (2, 3, 64, 32, 33, 2), (1, 2, 64, 1, 17, 4)], ids=_ids)
def test_rounding_model_stays_under_two_thirds_of_the_op_bar(layout, prec):
    B, heads, dh, nj, n, f = layout
    Q, K, K0, V, dO = _inputs(layout)
    g = _heads_first(dO, heads)
    ref = emulate(Q, K, K0, V, g, nj, n, f, None)
    em = emulate(Q, K, K0, V, g, nj, n, f, PREC[prec][1])
    errs = {nm: rel_l2(a[:, :, nj:], b[:, :, nj:]) for nm, a, b in zip(("dQ", "dK", "dK0", "dV"), em, ref) if nm != "dK0"}
    print(prec, layout, {k: "%.2e" % e for k, e in errs.items()})
    assert max(errs.values()) < OP_BAR[prec] * 2 / 3
    if nj:   # the joint queries are not rounded
        assert rel_l2(em[2], ref[2]) < 1e-12 and rel_l2(em[0][:, :, :nj], ref[0][:, :, :nj]) < 1e-12


# ----------------------------------------------------------------------------------------------------------------- GPU

def _ws_fwd(L, B, heads, dh, dev):
    return torch.empty(int(L.hp_sformer_attention_workspace_bytes(B, heads, dh)) // 4 + 1, device=dev)


def _forward_p(L, q, k, k0, v, layout, prec, out, lse):
    B, heads, dh, nj, n, f = layout
    ntok = nj + f * n
    ws = _ws_fwd(L, B, heads, dh, q.device)
    return L.hp_sformer_attention_lse_p(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, heads,
                                        dh, ntok, nj, n, f, prec, ws.data_ptr(), _lib.current_stream_handle(q.device))


def _backward_p(L, q, k, k0, v, out, do, lse, layout, prec, grads=None, ws=None):
    B, heads, dh, nj, n, f = layout
    ntok = nj + f * n
    grads = grads if grads is not None else [torch.empty_like(q) for _ in range(4)]
    nb = L.hp_sformer_attention_backward_p_workspace_bytes(B, heads, dh, ntok, nj, f, prec)
    ws = ws if ws is not None else torch.empty(nb // 4 + 1, device=q.device)
    rc = L.hp_sformer_attention_backward_p(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), do.data_ptr(),
                                           lse.data_ptr(), *(t.data_ptr() for t in grads), B, heads, dh, ntok, nj, n, f, prec,
                                           ws.data_ptr(), nb, _lib.current_stream_handle(q.device))
    return rc, grads


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_forward_with_lse(layout, prec):
    B, heads, dh, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    st = _lib.current_stream_handle(dev)
    ntok = nj + f * n
    Q, K, K0, V, _ = _inputs(layout)
    q, k, k0, v = (t.to(dev).contiguous() for t in (Q, K, K0, V))
    p = PREC[prec][0]
    out, out0, out32 = (torch.empty(B, ntok, heads * dh, device=dev) for _ in range(3))
    lse, lse32 = (torch.full((B, heads, ntok), float("nan"), device=dev) for _ in range(2))
    _lib.check(_forward_p(L, q, k, k0, v, layout, p, out, lse), "lse_p")
    ws = _ws_fwd(L, B, heads, dh, dev)
    _lib.check(L.hp_sformer_attention(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out0.data_ptr(), B, heads, dh, ntok, nj, n, f,
                                      p, ws.data_ptr(), st), "attention")
    _lib.check(L.hp_sformer_attention_lse(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out32.data_ptr(), lse32.data_ptr(), B,
                                          heads, dh, ntok, nj, n, f, ws.data_ptr(), st), "lse")
    torch.cuda.synchronize()
    assert torch.equal(out, out0)
    assert torch.equal(lse[:, :, :nj], lse32[:, :, :nj])
    _, ref_lse = _attn_ref(*(t.to(dev, torch.float64) for t in (Q, K, K0, V)), nj, n, f)
    e = rel_l2(lse[:, :, nj:], ref_lse[:, :, nj:])
    print(f"{prec} {layout}: lse of the patch rows rel-L2 {e:.2e}")
    assert e < LSE_BAR[prec]


@pytest.mark.gpu
@pytest.mark.parametrize("fwd,prec", [("bf16", "bf16"), ("fp16", "fp16")])
@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_backward_vs_float64(layout, fwd, prec):
    _backward_case(layout, fwd, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_backward_after_the_fp32_forward_vs_float64(prec):
    _backward_case((1, 2, 32, 24, 100, 3), "fp32", prec)
    _backward_case((1, 2, 64, 24, 300, 3), "fp32", prec)


def _backward_case(layout, fwd, prec):
    B, heads, dh, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + f * n
    Q, K, K0, V, dO = _inputs(layout)
    q, k, k0, v, do = (t.to(dev).contiguous() for t in (Q, K, K0, V, dO))
    out = torch.empty(B, ntok, heads * dh, device=dev)
    lse = torch.empty(B, heads, ntok, device=dev)
    _lib.check(_forward_p(L, q, k, k0, v, layout, PREC[fwd][0], out, lse), "lse_p")
    rc, r1 = _backward_p(L, q, k, k0, v, out, do, lse, layout, PREC[prec][0])
    _lib.check(rc, "backward_p")
    rc, r2 = _backward_p(L, q, k, k0, v, out, do, lse, layout, PREC[prec][0])
    _lib.check(rc, "backward_p")
    torch.cuda.synchronize()
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    Qd, Kd, K0d, Vd = (t.to(dev, torch.float64).requires_grad_(True) for t in (Q, K, K0, V))
    ref, _ = _attn_ref(Qd, Kd, K0d, Vd, nj, n, f)
    gd = _heads_first(dO.to(dev, torch.float64), heads)
    (ref * gd).sum().backward()
    dq, dk, dk0, dv = r1
    e = {"dQ": rel_l2(dq[:, :, nj:], Qd.grad[:, :, nj:]), "dK": rel_l2(dk[:, :, nj:], Kd.grad[:, :, nj:]),
         "dV": rel_l2(dv[:, :, nj:], Vd.grad[:, :, nj:])}
    with torch.no_grad():
        em = emulate(Qd, Kd, K0d, Vd, gd, nj, n, f, PREC[prec][1])
    ee = {"dQ": rel_l2(em[0][:, :, nj:], Qd.grad[:, :, nj:]), "dK": rel_l2(em[1][:, :, nj:], Kd.grad[:, :, nj:]),
          "dV": rel_l2(em[3][:, :, nj:], Vd.grad[:, :, nj:])}
    exact = {}
    if nj:
        exact = {"dK0": rel_l2(dk0, K0d.grad), "dQ joint": rel_l2(dq[:, :, :nj], Qd.grad[:, :, :nj])}
        e["dK whole"], e["dV whole"] = rel_l2(dk, Kd.grad), rel_l2(dv, Vd.grad)
    print(f"forward {fwd}, backward {prec}, {layout}: measured " + " ".join(f"{a} {x:.2e}" for a, x in e.items()) + " | emulated "
          + " ".join(f"{a} {x:.2e}" for a, x in ee.items()) + " | measured / emulated "
          + " ".join(f"{a} {e[a] / ee[a]:.2f}" for a in ee) + " | exact part " + " ".join(f"{a} {x:.2e}" for a, x in exact.items()))
    assert max(e.values()) < OP_BAR[prec]
    if nj:
        assert max(exact.values()) < 1e-5
    else:
        assert float(dk0.abs().max()) == 0.0


GUARD = 64 * 1024                                  # floats either side (256 KB)
SENT = float.fromhex("0x1.5a5a5ap+100")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", [(2, 3, 32, 24, 37, 3), (1, 2, 64, 7, 300, 2)], ids=_ids)
def test_new_entries_write_only_their_outputs(layout, prec):
    """out, lse, dQ, dK, dK0, dV between two sentinel-filled guard regions (the pattern of tests/test_head64.py): the guards
    stay bit for bit, every output element is written."""
    B, heads, dh, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + f * n
    Q, K, K0, V, dO = _inputs(layout, seed=13)
    q, k, k0, v, do = (t.to(dev).contiguous() for t in (Q, K, K0, V, dO))

    def guarded(shape):
        cnt = int(np.prod(shape))
        buf = torch.full((GUARD + cnt + GUARD,), SENT, device=dev)
        return buf, buf[GUARD:GUARD + cnt].view(shape)

    def intact(buf, t):
        return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + t.numel():] == SENT).all())

    names = ["out", "lse", "dQ", "dK", "dK0", "dV"]
    shapes = [(B, ntok, heads * dh), (B, heads, ntok)] + [(B, heads, ntok, dh)] * 4
    bufs = [guarded(s) for s in shapes]
    out, lse = bufs[0][1], bufs[1][1]
    _lib.check(_forward_p(L, q, k, k0, v, layout, PREC[prec][0], out, lse), "lse_p")
    rc, _ = _backward_p(L, q, k, k0, v, out, do, lse, layout, PREC[prec][0], [b[1] for b in bufs[2:]])
    _lib.check(rc, "backward_p")
    torch.cuda.synchronize()
    for name, (buf, t) in zip(names, bufs):
        assert intact(buf, t), f"{name} was written outside its tensor"
        assert not bool((t == SENT).any()), f"{name} has unwritten elements"
        assert bool(torch.isfinite(t).all()), name


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [(1, 2, 32, 24, 100, 3), (2, 2, 64, 7, 50, 2)], ids=_ids)
def test_fp32_results_keep_their_bits(layout):
    """precision = FP32 through both new entries equals the old entries bitwise; the fp32 backward's results are the same
    whether or not 16-bit calls ran in between on the same stream and workspace."""
    B, heads, dh, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    st = _lib.current_stream_handle(dev)
    ntok = nj + f * n
    Q, K, K0, V, dO = _inputs(layout)
    q, k, k0, v, do = (t.to(dev).contiguous() for t in (Q, K, K0, V, dO))
    out, out_p = (torch.empty(B, ntok, heads * dh, device=dev) for _ in range(2))
    lse, lse_p = (torch.empty(B, heads, ntok, device=dev) for _ in range(2))
    ws = _ws_fwd(L, B, heads, dh, dev)
    _lib.check(L.hp_sformer_attention_lse(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, heads,
                                          dh, ntok, nj, n, f, ws.data_ptr(), st), "lse")
    _lib.check(_forward_p(L, q, k, k0, v, layout, 0, out_p, lse_p), "lse_p")
    assert torch.equal(out, out_p) and torch.equal(lse, lse_p)
    nb = L.hp_sformer_attention_backward_p_workspace_bytes(B, heads, dh, ntok, nj, f, 0)
    assert nb == L.hp_sformer_attention_backward_workspace_bytes(B, heads, dh, ntok, nj, f)
    bws = torch.empty(nb // 4 + 1, device=dev)
    old = [torch.empty_like(q) for _ in range(4)]
    _lib.check(L.hp_sformer_attention_backward(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), do.data_ptr(),
                                               lse.data_ptr(), *(t.data_ptr() for t in old), B, heads, dh, ntok, nj, n, f, bws.data_ptr(),
                                               nb, st), "backward")
    old = [t.clone() for t in old]
    rc, new = _backward_p(L, q, k, k0, v, out, do, lse, layout, 0, ws=bws)
    _lib.check(rc, "backward_p fp32")
    for a, b in zip(old, new):
        assert torch.equal(a, b)
    for p in (1, 4):   # 16-bit calls on the same workspace and stream, then the fp32 backward again
        rc, _ = _backward_p(L, q, k, k0, v, out, do, lse, layout, p, ws=bws)
        _lib.check(rc, "backward_p 16-bit")
    rc, again = _backward_p(L, q, k, k0, v, out, do, lse, layout, 0, ws=bws)
    _lib.check(rc, "backward_p fp32")
    torch.cuda.synchronize()
    for a, b in zip(old, again):
        assert torch.equal(a, b)


def _module_case(tag):
    """(kw, module on the CPU, video, golden file, golden key)"""
    if tag == "mid":
        kw, m, video = ST.build("mid")
        return kw, m, video, "sformer_grads.npz", "mid"
    _, kw, m, video = H64.build("sf")
    return kw, m, video, "head64.npz", "sf"


@pytest.mark.gpu
@pytest.mark.parametrize("fwd,bwd", [("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "bf16"), ("fp16", "fp16")])
@pytest.mark.parametrize("tag", ["mid", "sf"])
def test_module_gradients_vs_reference_golden(tag, fwd, bwd, golden):
    kw, m, video, gfile, key = _module_case(tag)
    m = m.cuda().train()
    m.attention_precision, m.attention_backward_precision = fwd, bwd
    v = video.cuda().requires_grad_(True)
    y = m(v)
    (y * ST.loss_weights(y.shape).float().cuda()).sum().backward()
    g = golden(gfile)
    grads = {k: p.grad for k, p in m.named_parameters()}
    if tag == "mid":
        ev = rel_l2(v.grad, g["mid_video"])
        worst = ST.golden_compare(g, "mid", grads, v.grad, VIDEO_BAR[bwd])
    else:
        ev = rel_l2(v.grad, g["sf_input"])
        H64.golden_compare(g, "sf", grads, v.grad, VIDEO_BAR[bwd])
        worst = H64.golden_compare(g, "sf", grads, torch.as_tensor(g["sf_input"]), VIDEO_BAR[bwd])   # parameters alone
    emu = EMULATED.get((tag, bwd)) if fwd == bwd else None
    print(f"{tag} forward {fwd} backward {bwd}: worst parameter gradient {worst:.2e}, video gradient {ev:.2e}"
          + (f"; emulated {emu[0]:.1e} / {emu[1]:.1e}: measured / emulated {worst / emu[0]:.2f} / {ev / emu[1]:.2f}" if emu else ""))
    assert worst < PARAM_BAR[bwd] and ev < VIDEO_BAR[bwd]
    assert sorted(k for k, gr in grads.items() if gr is None) == sorted(g[f"{key}_none"].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("heads,dim_head", [(8, 32), (4, 64)])
def test_config5_geometry_batch2_vs_oracle(heads, dim_head):
    """BASELINE config 5's geometry (n = 1024, 16 frames), depth 2, batch 2, against the oracle's float64 autograd on the
    device: the inputs and the pattern of test_sformer_train.test_module_gradients_config5_batch2_vs_oracle."""
    kw = ST.CFG5 | dict(heads=heads, dim_head=dim_head, depth=2)
    m = NlosPoseSformer(**kw)
    hpt.fill_module(m, "sformer.")
    video = torch.rand(2, 16, 1, 128, 128, generator=torch.Generator().manual_seed(55))
    yy, xx = torch.linspace(-1, 1, 128).view(1, 1, 128, 1), torch.linspace(-1, 1, 128).view(1, 1, 1, 128)
    ff = torch.arange(16.0).view(16, 1, 1, 1) / 16
    video[1] = torch.exp(-((yy - 0.3 * ff) ** 2 + (xx + 0.4 - ff) ** 2) / 0.05)
    R = ST.loss_weights((2, 24, 4, 128))
    ref, ref_v, _ = ST.oracle_grads(m, video, kw, device="cuda", R=R)
    ref = {k: (g.cpu() if g is not None else None) for k, g in ref.items()}
    ref_v = ref_v.cpu()
    torch.cuda.empty_cache()
    m = m.cuda().train()
    failures = []
    for prec in ("fp16", "bf16"):
        m.attention_precision = m.attention_backward_precision = prec
        m.zero_grad(set_to_none=True)
        v = video.cuda().requires_grad_(True)
        y = m(v)
        (y * R.float().cuda()).sum().backward()
        errs = {k: rel_l2(p.grad, ref[k]) for k, p in m.named_parameters() if ref[k] is not None}
        worst = max(errs, key=errs.get)
        ev = [rel_l2(v.grad[b], ref_v[b]) for b in range(2)]
        cross = rel_l2(v.grad[1], ref_v[0])
        print(f"config 5 at {heads} x {dim_head}, depth 2, batch 2, {prec} forward and backward: worst parameter gradient {worst} "
              f"{errs[worst]:.2e}; video gradient per sample {ev[0]:.2e} {ev[1]:.2e}, sample 1 against sample 0's reference {cross:.2e}")
        if not (errs[worst] < PARAM_BAR[prec] and max(ev) < VIDEO_BAR[prec] and cross > 100 * max(ev)):
            failures.append((prec, worst, errs[worst], ev, cross))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("lin,att", [("fp32", "fp32"), ("bf16", "fp16")])
@pytest.mark.parametrize("tag", ["mid", "sf"])
@pytest.mark.parametrize("bwd", ["bf16", "fp16"])
def test_graph_mode_output_equals_no_graph_output(tag, lin, att, bwd):
    _, m, video, _, _ = _module_case(tag)
    m = m.cuda()
    m.linear_precision, m.attention_precision, m.attention_backward_precision = lin, att, bwd
    video = video.cuda()
    with torch.no_grad():
        y0 = m(video)
    y1 = m.train()(video)
    assert y1.grad_fn is not None and torch.equal(y0, y1)
    y2 = m.eval()(video)
    assert y2.grad_fn is None and torch.equal(y0, y2)


SGD_DRIFT_BAR = 3e-4   # 3 x the measured 9.4e-5, rounded up to one digit (and below the 5e-3 cap)


@pytest.mark.gpu
def test_sgd_steps_track_the_oracle():
    """Five SGD steps of `mid` with fp16 attention forward and backward (the loop of test_sformer_train's test of the same
    name).  Measured on an MI355X: the worst parameter is 9.4e-5 from the float64 oracle's trajectory.  The bar is three times
    that rounded up to one digit, and never above 5e-3 (ten times the fp16 parameter-gradient bar: a larger drift in five
    steps of lr 0.005 is a bug, not noise)."""
    from oracle import nlospose_oracle as O

    kw, m, video = ST.build("mid")
    ref_m = NlosPoseSformer(**kw)
    ref_m.load_state_dict(m.state_dict())
    m = m.cuda().train()
    m.attention_precision = m.attention_backward_precision = "fp16"
    vid = video.cuda()
    R = ST.loss_weights((2, 24, 4, 128)) * 0.01
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
    assert losses[-1] < losses[0]
    assert max(errs.values()) < SGD_DRIFT_BAR


@pytest.mark.gpu
def test_refusals():
    kw, m, video = ST.build("mid")
    vid = video.cuda()
    for dh in (16, 24):   # a 16-bit backward at a width it is not built for: refused at forward
        bad = NlosPoseSformer(**kw | dict(dim_head=dh)).cuda().train()
        bad.attention_backward_precision = "fp16"
        with pytest.raises(_lib.HiddenPoseHipError, match="dim_head 32 and 64"):
            bad(vid)
    m = m.cuda().train()
    m.attention_backward_precision = "fp8"
    with pytest.raises(_lib.HiddenPoseHipError, match="attention_backward_precision"):
        m(vid)
    m.attention_backward_precision = "bf16"
    m.attn_dropout = 0.1
    with pytest.raises(_lib.HiddenPoseHipError, match="dropout"):
        m(vid)
    m.attn_dropout = 0.0
    m.attention_backward_precision = "fp32"   # the default: a 16-bit forward still refuses at backward
    m.attention_precision = "fp16"
    y = m(vid)
    with pytest.raises(_lib.HiddenPoseHipError, match="fp32"):
        y.sum().backward()
    # the C entries: dh 48 is not built and the message names the built set; an unknown precision is refused
    L = _lib.lib()
    layout = (1, 2, 48, 24, 64, 2)
    Q, K, K0, V, dO = _inputs(layout)
    q, k, k0, v, do = (t.cuda().contiguous() for t in (Q, K, K0, V, dO))
    out, lse = torch.zeros_like(do), torch.zeros(1, 2, 24 + 128, device="cuda")
    rc, _ = _backward_p(L, q, k, k0, v, out, do, lse, layout, 4)
    assert rc == HP_ERR_UNSUPPORTED and b"(32, 64)" in L.hp_last_error_string()
    assert _forward_p(L, q, k, k0, v, layout, 1, out, lse) == HP_ERR_UNSUPPORTED and b"32 and 64" in L.hp_last_error_string()
    layout = (1, 2, 32, 24, 64, 2)
    Q, K, K0, V, dO = _inputs(layout)
    q, k, k0, v, do = (t.cuda().contiguous() for t in (Q, K, K0, V, dO))
    out = torch.zeros_like(do)
    rc, _ = _backward_p(L, q, k, k0, v, out, do, lse, layout, 2)
    assert rc != 0 and b"precision" in L.hp_last_error_string()
    assert _forward_p(L, q, k, k0, v, layout, 2, out, lse) != 0 and b"precision" in L.hp_last_error_string()
