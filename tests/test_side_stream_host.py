"""Host logic of the side-stream weight gradients (hiddenpose_amd/_side_stream.py) on CPU tensors: which uses of a parameter
`release` keeps on the main stream, that a graph leaves the weak set with its ctx, and which parameters are `adoptable`.  The
stream half (`stream` / `launch` / `join`) needs a device: tests/test_conv_gpu.py, tests/test_dconv_gpu.py."""
import gc

import pytest
import torch

from hiddenpose_amd import _lib
from hiddenpose_amd import _side_stream as S
from hiddenpose_amd import hip_ops as ops

MAIN = []   # what release() answered, in backward order


class _Use(torch.autograd.Function):
    """y = x * w (+ b), registered and released the way the HIP Functions do it."""

    @staticmethod
    def forward(ctx, x, w, b=None):
        ctx.save_for_backward(x, w)
        ctx.b = b
        S.register(ctx, {1: w, 2: b})
        return x * w if b is None else x * w + b

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        main = S.release(ctx, w, ctx.b)        # always; the switch only decides what becomes of the answer
        MAIN.append(main or not ops._WGRAD_ASYNC)
        return g * w, g * x, (g if ctx.b is not None else None)


@pytest.fixture(autouse=True)
def _fresh():
    MAIN.clear()
    prev = ops.set_wgrad_async(True)
    yield
    ops.set_wgrad_async(prev)


def _param(v=2.0, requires_grad=True):
    return torch.nn.Parameter(torch.full((3,), v), requires_grad=requires_grad)


def _idle(p):
    return len(p._hp_uses) == 0 and not p._hp_shared


def test_one_use_takes_the_side_stream():
    w, x = _param(), torch.ones(3, requires_grad=True)
    y = _Use.apply(x, w)
    assert len(w._hp_uses) == 1
    y.sum().backward()
    assert MAIN == [False] and _idle(w)


def test_two_uses_in_one_graph_stay_on_the_main_stream():
    w, x = _param(), torch.ones(3, requires_grad=True)
    _Use.apply(_Use.apply(x, w), w).sum().backward()
    assert MAIN == [True, True] and _idle(w)      # the second release sees ONE live use: the sticky mark keeps it on main
    _Use.apply(x, w).sum().backward()             # and the mark does not outlive the pass
    assert MAIN == [True, True, False] and _idle(w)


def test_two_graphs_differentiated_by_one_backward_stay_on_the_main_stream():
    w, x = _param(), torch.ones(3, requires_grad=True)
    a, b = _Use.apply(x, w), _Use.apply(x * 2, w)
    (a.sum() + b.sum()).backward()
    assert MAIN == [True, True] and _idle(w)
    assert torch.equal(w.grad, torch.full((3,), 3.0))


def test_a_graph_dropped_without_a_backward_leaves_the_set():
    w, x = _param(), torch.ones(3, requires_grad=True)
    y = _Use.apply(x, w)
    assert len(w._hp_uses) == 1
    del y
    gc.collect()
    assert len(w._hp_uses) == 0
    _Use.apply(x, w).sum().backward()
    assert MAIN == [False] and _idle(w)


def test_a_stale_shared_mark_is_cleared_by_the_next_registration():
    w, x = _param(), torch.ones(3, requires_grad=True)
    _Use.apply(x, w).sum().backward()
    w._hp_shared = True      # what a graph discarded between the releases of its two uses leaves behind
    MAIN.clear()
    _Use.apply(x, w).sum().backward()
    assert MAIN == [False] and _idle(w)           # not even one step on the main stream


def test_no_grad_and_frozen_parameters_register_nothing():
    w, x = _param(), torch.ones(3, requires_grad=True)
    with torch.no_grad():
        _Use.apply(x, w)
    assert not getattr(w, "_hp_uses", ())
    frozen, b = _param(requires_grad=False), _param(0.5)
    y = _Use.apply(x, frozen, b)
    assert not hasattr(frozen, "_hp_uses") and len(b._hp_uses) == 1
    y.sum().backward()
    assert MAIN == [True] and _idle(b)            # the frozen weight's gradient is dropped by autograd at once: main stream


def test_a_second_backward_over_a_retained_graph_stays_on_the_main_stream():
    w, x = _param(), torch.ones(3, requires_grad=True)
    y = _Use.apply(x, w).sum()
    y.backward(retain_graph=True)
    y.backward()                                  # w.grad is summed by autograd: this use is no longer registered
    assert MAIN == [False, True] and _idle(w)


def test_a_bias_shared_by_two_layers_keeps_both_on_the_main_stream():
    w1, w2, b, x = _param(2.0), _param(3.0), _param(0.5), torch.ones(3, requires_grad=True)
    _Use.apply(_Use.apply(x, w1, b), w2, b).sum().backward()
    assert MAIN == [True, True] and _idle(b) and _idle(w1) and _idle(w2)
    MAIN.clear()
    _Use.apply(x, w1, b).sum().backward()         # each of them alone is free again
    assert MAIN == [False]


@pytest.mark.parametrize("at_backward", [False, True])
def test_release_runs_whatever_the_switch_says(at_backward):
    """The switch toggled between a forward and its backward: the use is released all the same, so the next step is not
    pinned to the main stream by a count that nobody took back."""
    w, x = _param(), torch.ones(3, requires_grad=True)
    ops.set_wgrad_async(not at_backward)
    y = _Use.apply(x, w)
    assert len(w._hp_uses) == 1                   # registering does not ask the switch either
    ops.set_wgrad_async(at_backward)
    y.sum().backward()
    assert MAIN == [not at_backward] and _idle(w)
    ops.set_wgrad_async(True)
    _Use.apply(x, w).sum().backward()
    assert MAIN == [not at_backward, False] and _idle(w)


def test_adoptable():
    leaf = _param()
    assert S.adoptable([leaf], False) and S.adoptable([leaf], True)
    assert not S.adoptable([leaf * 1.0], False) and not S.adoptable([leaf * 1.0], True)      # not a leaf
    assert not S.adoptable([leaf, leaf * 1.0], True)
    hooked = _param()
    hooked.register_hook(lambda g: g)                                                        # receives the gradient
    assert not S.adoptable([hooked], False) and not S.adoptable([hooked], True)
    hooked.grad = torch.zeros(3)
    assert not S.adoptable([hooked], True)
    post = _param()
    post.register_post_accumulate_grad_hook(lambda p: None)                                  # may read .grad
    assert not S.adoptable([post], False) and not S.adoptable([post], True)
    post.grad = torch.zeros(3)      # pre-allocated (a bucket view): the caller accumulates on the side stream itself
    assert S.adoptable([post], True) and not S.adoptable([post], False)
    acc = _param()
    acc.grad = torch.zeros(3)
    assert S.adoptable([acc], True) and not S.adoptable([acc], False)


def test_the_listener_list_and_the_join_are_the_modules_own():
    assert ops._side_grad_listeners is S.listeners and ops.join_side_streams is S.join


@pytest.mark.parametrize("value,want", [(None, 7), ("", 0), ("abc", 0), ("0", 0), ("1", 1), (" 12xy", 12), ("-3", -3), ("2.9", 2)])
def test_environment_switches_read_like_atoi(monkeypatch, value, want):
    monkeypatch.delenv("HP_TEST_SWITCH", raising=False)
    if value is not None:
        monkeypatch.setenv("HP_TEST_SWITCH", value)
    assert _lib.env_int("HP_TEST_SWITCH", 7) == want
    assert _lib.env_flag("HP_TEST_SWITCH", True) == (want != 0)
