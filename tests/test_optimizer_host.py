"""CPU-side checks of the optimizer stage (hp_optim_adam_multi / hp_optim_sgd_multi, HipAdam / HipSGD): every refusal of the
C entries returns a status and a message with no device present, the Python refusals, the selection in `get_optimizer`, and
the float64 model of the update rules that the GPU tests compare against."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import optim_ref as R
from hiddenpose_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000      # a non-null address that is never dereferenced: every check below comes before any device call
WS = 1 << 16


def adam_recs(n=(8,), **over):
    recs = (_lib.OptimAdamRec * len(n))()
    for r, k in zip(recs, n):
        r.p, r.g, r.m, r.v, r.n, r.lr_over_bc1, r.inv_sqrt_bc2 = FAKE, FAKE, FAKE, FAKE, k, 1e-3, 1.0
        for key, val in over.items():
            setattr(r, key, val)
    return recs


def sgd_recs(n=(8,), **over):
    recs = (_lib.OptimSgdRec * len(n))()
    for r, k in zip(recs, n):
        r.p, r.g, r.buf, r.n, r.first_step = FAKE, FAKE, FAKE, k, 1
        for key, val in over.items():
            setattr(r, key, val)
    return recs


def adam(hip_lib, recs, count=None, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, ws=FAKE, ws_bytes=WS):
    return hip_lib.hp_optim_adam_multi(C.addressof(recs) if recs is not None else None, len(recs) if count is None else count,
                                       b1, b2, eps, wd, ws, ws_bytes, None)


def sgd(hip_lib, recs, count=None, lr=1e-3, mu=0.9, damp=0.0, wd=0.0, nesterov=0, ws=FAKE, ws_bytes=WS):
    return hip_lib.hp_optim_sgd_multi(C.addressof(recs) if recs is not None else None, len(recs) if count is None else count,
                                      lr, mu, damp, wd, nesterov, ws, ws_bytes, None)


def refused(hip_lib, rc, *words):
    msg = hip_lib.hp_last_error_string()
    assert rc == -1, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_record_layout_matches_the_header():
    assert C.sizeof(_lib.OptimAdamRec) == 48 and _lib.OptimAdamRec.n.offset == 32 and _lib.OptimAdamRec.inv_sqrt_bc2.offset == 44
    assert C.sizeof(_lib.OptimSgdRec) == 40 and _lib.OptimSgdRec.n.offset == 24 and _lib.OptimSgdRec.first_step.offset == 32


def test_workspace_query(hip_lib):
    for q, rec in ((hip_lib.hp_optim_adam_multi_workspace_bytes, 48), (hip_lib.hp_optim_sgd_multi_workspace_bytes, 40)):
        assert q(-1) == 0
        for count in (0, 1, 3, 255, 1000):
            assert q(count) >= count * rec + (count + 1) * 4 and q(count) % 16 == 0


def test_adam_argument_checks_come_before_any_device_call(hip_lib):
    L = hip_lib
    refused(L, adam(L, None, count=2), "null record table")
    refused(L, adam(L, adam_recs(), ws=None), "null workspace")
    for field in ("p", "g", "m", "v"):
        refused(L, adam(L, adam_recs(**{field: None})), "null pointer")
    refused(L, adam(L, adam_recs(), count=-1), "count")
    refused(L, adam(L, adam_recs(n=(8, -3))), "n -3")
    refused(L, adam(L, adam_recs(n=(8, 8, 8)), ws_bytes=L.hp_optim_adam_multi_workspace_bytes(3) - 1), "workspace too small")
    refused(L, adam(L, adam_recs(), b1=1.0), "beta1")
    refused(L, adam(L, adam_recs(), b1=-0.1), "beta1")
    refused(L, adam(L, adam_recs(), b2=1.0), "beta2")
    refused(L, adam(L, adam_recs(), b2=float("nan")), "beta2")
    refused(L, adam(L, adam_recs(), eps=-1e-8), "eps")
    refused(L, adam(L, adam_recs(), wd=-1e-2), "weight_decay")
    refused(L, adam(L, adam_recs(lr_over_bc1=-1e-3)), "lr")
    refused(L, adam(L, adam_recs(inv_sqrt_bc2=0.0)), "inv_sqrt_bc2")
    # nothing to do: success without a launch (no device is touched, so this passes without one)
    assert adam(L, adam_recs(), count=0) == 0
    assert adam(L, None, count=0, ws=None, ws_bytes=0) == 0
    assert adam(L, adam_recs(n=(0, 0)), ws=None, ws_bytes=0) == 0


def test_sgd_argument_checks_come_before_any_device_call(hip_lib):
    L = hip_lib
    refused(L, sgd(L, None, count=2), "null record table")
    refused(L, sgd(L, sgd_recs(), ws=None), "null workspace")
    for field in ("p", "g", "buf"):
        refused(L, sgd(L, sgd_recs(**{field: None})), "null pointer")
    refused(L, sgd(L, sgd_recs(), count=-1), "count")
    refused(L, sgd(L, sgd_recs(n=(8, -3))), "n -3")
    refused(L, sgd(L, sgd_recs(n=(8, 8, 8)), ws_bytes=L.hp_optim_sgd_multi_workspace_bytes(3) - 1), "workspace too small")
    refused(L, sgd(L, sgd_recs(), lr=-1e-3), "lr")
    refused(L, sgd(L, sgd_recs(), wd=-1e-2), "weight_decay")
    refused(L, sgd(L, sgd_recs(), mu=-0.5), "momentum")
    refused(L, sgd(L, sgd_recs(), mu=0.0, nesterov=1), "nesterov")
    refused(L, sgd(L, sgd_recs(), damp=0.1, nesterov=1), "nesterov")
    assert sgd(L, sgd_recs(), count=0) == 0
    assert sgd(L, None, count=0, ws=None, ws_bytes=0) == 0
    assert sgd(L, sgd_recs(n=(0, 0)), ws=None, ws_bytes=0) == 0


def test_python_refusals():
    from hiddenpose_amd.optimizer import HipAdam, HipSGD

    w = torch.nn.Parameter(torch.zeros(4))
    for kw in ({"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True}, {"fused": True},
               {"foreach": True}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            HipAdam([w], **kw)
    for kw in ({"maximize": True}, {"differentiable": True}, {"foreach": True}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            HipSGD([w], lr=0.1, **kw)
    for make in (lambda ps: HipAdam(ps), lambda ps: HipSGD(ps, lr=0.1, momentum=0.9)):
        cpu = torch.nn.Parameter(torch.zeros(4))
        cpu.grad = torch.ones(4)
        with pytest.raises(_lib.HiddenPoseHipError, match="no CPU path"):
            make([cpu]).step()
        half = torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))
        half.grad = torch.ones(4, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="bfloat16"):
            make([half]).step()
        sparse = torch.nn.Parameter(torch.zeros(4, 2))
        sparse.grad = torch.zeros(4, 2).to_sparse()
        with pytest.raises(ValueError, match="sparse"):
            make([sparse]).step()
        none = torch.nn.Parameter(torch.zeros(4))     # no gradient anywhere: nothing to do, nothing refused
        make([none]).step()
    # an option that arrives through a loaded state_dict is refused at the step
    opt = HipAdam([w])
    opt.param_groups[0]["amsgrad"] = True
    w.grad = torch.ones(4)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()


def test_get_optimizer_selection_and_stage_sets():
    from hiddenpose_amd import hip_ops
    from hiddenpose_amd.config import make_cfg
    from hiddenpose_amd.optimizer import HipAdam, HipSGD, get_optimizer

    assert os.environ.get("HP_OPTIMIZER_IMPL", "") in ("", "0"), "this test describes the default environment"
    model = torch.nn.Linear(3, 2)
    cfg = make_cfg(32, 32).clone()
    opt = get_optimizer(cfg, model)
    assert type(opt) is torch.optim.Adam and opt.defaults["lr"] == cfg.TRAIN.LR
    cfg.TRAIN.OPTIMIZER = "sgd"
    assert type(get_optimizer(cfg, model)) is torch.optim.SGD
    cfg.TRAIN.OPTIMIZER = "adam_hip"
    opt = get_optimizer(cfg, model)
    assert type(opt) is HipAdam and isinstance(opt, torch.optim.Adam) and opt.defaults["lr"] == cfg.TRAIN.LR
    assert set(opt.param_groups[0]) == set(torch.optim.Adam(model.parameters(), foreach=False).param_groups[0])
    cfg.TRAIN.OPTIMIZER = "sgd_hip"
    opt = get_optimizer(cfg, model)
    assert type(opt) is HipSGD and opt.defaults["momentum"] == 0.9
    assert hip_ops.ATEN_STAGES == {"Adam"} and "Adam" not in hip_ops.HIP_STAGES


def test_environment_switch_selects_the_hip_classes():
    code = ("import torch\n"
            "from hiddenpose_amd import hip_ops\n"
            "from hiddenpose_amd.config import make_cfg\n"
            "from hiddenpose_amd.optimizer import get_optimizer\n"
            "cfg = make_cfg(32, 32).clone()\n"
            "m = torch.nn.Linear(3, 2)\n"
            "a = type(get_optimizer(cfg, m)).__name__\n"
            "cfg.TRAIN.OPTIMIZER = 'sgd'\n"
            "s = type(get_optimizer(cfg, m)).__name__\n"
            "print(a, s, sorted(hip_ops.ATEN_STAGES), 'Adam' in hip_ops.HIP_STAGES)\n")
    for value, expect in (("hip", "HipAdam HipSGD [] True"), ("0", "Adam SGD ['Adam'] False")):
        env = dict(os.environ, HP_OPTIMIZER_IMPL=value, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().splitlines()[-1] == expect, (value, r.stdout)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_float64_model_agrees_with_torch_in_float64(wd):
    """The model of optim_ref against torch.optim.Adam / SGD (foreach=False) on float64 CPU tensors: 10 steps, lr times 0.2 after
    step 5, one parameter without a gradient on steps 3-4.  Both run in float64 and differ at most in association order, a
    few 1e-16 per operation; the bar is 1e-12, on |a - b| relative to the tensor's largest magnitude."""
    sizes = tuple(R.SIZES[:8])

    def run64(make):
        ps = [torch.nn.Parameter(p.double()) for p in R.params0(sizes)]
        opt = make(ps)
        for s in range(1, R.STEPS + 1):
            lr, gs = R.schedule(s, sizes)
            opt.param_groups[0]["lr"] = lr
            for p, g in zip(ps, gs):
                p.grad = None if g is None else g.double()
            opt.step()
        return ps, opt

    def close(a, b, what):
        err = float((a.detach() - b).abs().max() / b.abs().max().clamp_min(1e-300))
        assert err <= 1e-12, (what, err)

    ps, opt = run64(lambda ps: torch.optim.Adam(ps, lr=R.LR, betas=R.BETAS, eps=R.EPS, weight_decay=wd, foreach=False))
    p64, s64 = R.run_model64("adam", sizes, weight_decay=wd)
    for i, p in enumerate(ps):
        close(p, p64[i], ("adam p", i))
        close(opt.state[p]["exp_avg"], s64["exp_avg"][i], ("adam m", i))
        close(opt.state[p]["exp_avg_sq"], s64["exp_avg_sq"][i], ("adam v", i))
    assert float(opt.state[ps[R.NONE_PARAM]]["step"]) == R.STEPS - len(R.NONE_STEPS)
    for mu, nest, damp in ((0.0, False, 0.0), (0.9, False, 0.0), (0.9, True, 0.0), (0.8, False, 0.3)):
        ps, opt = run64(lambda ps: torch.optim.SGD(ps, lr=R.LR, momentum=mu, dampening=damp, nesterov=nest, weight_decay=wd,
                                                   foreach=False))
        p64, s64 = R.run_model64("sgd", sizes, momentum=mu, dampening=damp, nesterov=nest, weight_decay=wd)
        for i, p in enumerate(ps):
            close(p, p64[i], ("sgd p", mu, nest, i))
            if mu:
                close(opt.state[p]["momentum_buffer"], s64["momentum_buffer"][i], ("sgd buf", mu, nest, i))
