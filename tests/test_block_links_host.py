"""Host logic of the links between the regressor's conv + BatchNorm units (hiddenpose_amd/_block_links.py) on CPU tensors, with
toy Functions that give and take the way hip_ops' nodes do.  What the links carry on a device: tests/test_conv_gpu.py."""
import gc
import weakref

import pytest
import torch

from hiddenpose_amd import _block_links as K


# ---------------------------------------------------------------- GradLink
LAST = []   # what take() answered for `last`, in backward order


class _Conv(torch.autograd.Function):
    """y = c x, one of the readers of a block input: the last one to run adds what the others parked."""

    @staticmethod
    def forward(ctx, x, c, link):
        ctx.c, ctx.link = c, link
        return x * c

    @staticmethod
    def backward(ctx, dy):
        addend, mask, last = ctx.link.take()
        LAST.append(last)
        dx = dy * ctx.c
        if addend is not None:
            dx = dx + (addend if mask is None else addend * mask)
        if not last:
            ctx.link.park(dx)
            dx = None
        return dx, None, None


class _OutIdentity(torch.autograd.Function):
    """y = relu(o + x), x the block input: parks its raw dy and the sign mask instead of returning a gradient for x."""

    @staticmethod
    def forward(ctx, o, x, link):
        y = torch.relu(o + x)
        ctx.mask, ctx.link = (y > 0).float(), link
        return y

    @staticmethod
    def backward(ctx, dy):
        ctx.link.park(dy, ctx.mask)
        return dy * ctx.mask, None, None


@pytest.fixture(autouse=True)
def _fresh():
    LAST.clear()


@pytest.mark.parametrize("first", [2.0, 3.0])
def test_two_takers_in_either_order(first):
    x = torch.ones(4, requires_grad=True)
    link = K.GradLink(2)
    second = 5.0 - first
    a = _Conv.apply(x, first, link)          # recorded first: its backward runs last
    b = _Conv.apply(x, second, link)
    (a + b).sum().backward()
    assert LAST == [False, True]
    assert torch.equal(x.grad, torch.full((4,), 5.0))
    with pytest.raises(RuntimeError, match="already consumed"):
        link.take()


def test_one_taker_adds_the_masked_gradient_parked_by_the_output_unit():
    x = torch.tensor([1.0, -3.0, 2.0, -0.5], requires_grad=True)
    link = K.GradLink(1)
    y = _OutIdentity.apply(_Conv.apply(x, 2.0, link), x, link)      # 3 x, negative where x is
    (y * torch.tensor([1.0, 10.0, 100.0, 1000.0])).sum().backward()
    assert LAST == [True]
    assert torch.equal(x.grad, torch.tensor([3.0, 0.0, 300.0, 0.0]))
    with pytest.raises(RuntimeError, match="already consumed"):
        link.take()


def test_a_parked_gradient_comes_back_exactly_once():
    link = K.GradLink(2)
    g, m = torch.ones(2), torch.zeros(2)
    link.park(g, m)
    addend, mask, last = link.take()
    assert addend is g and mask is m and not last
    assert link.take() == (None, None, True)                        # nothing parked in between: nothing to add
    link = K.GradLink(1)
    assert link.take() == (None, None, True)


def test_a_second_backward_over_the_same_graph_raises():
    x = torch.ones(4, requires_grad=True)
    y = _Conv.apply(x, 2.0, K.GradLink(1)).sum()
    y.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed"):
        y.backward()


# ---------------------------------------------------------------- BnLink
TOOK = []   # what take_sums() answered in the producer's backward


class _Producer(torch.autograd.Function):
    """y = 2 x; its backward may skip a pass if `link` holds sums that belong to the gradient it receives."""

    @staticmethod
    def forward(ctx, x, link):
        ctx.link = link
        return x * 2

    @staticmethod
    def backward(ctx, dy):
        TOOK.append(ctx.link.take_sums(dy))
        return dy.contiguous() * 2, None


class _Consumer(torch.autograd.Function):
    """y = 3 x; its backward takes the producer's sums from the dx it writes."""

    @staticmethod
    def forward(ctx, x, link):
        ctx.link = link
        return x * 3

    @staticmethod
    def backward(ctx, dy):
        dx = dy * 3
        ctx.link.give_sums("sums of this dx", dx)
        return dx, None


def _chain(tap):
    TOOK.clear()
    x = torch.ones(1000, requires_grad=True)
    link = K.BnLink()
    ya = _Producer.apply(x, link)
    if tap == "hook":
        ya.register_hook(lambda g: g * 2)
    elif tap == "hook_in_place":
        ya.register_hook(lambda g: g.mul_(2))
    extra = (ya * 5).sum() if tap == "before" else 0
    yb = _Consumer.apply(ya, link)
    if tap == "after":
        extra = (ya * 5).sum()
    (yb.sum() + extra).backward()
    assert link.sums is None and link._dx is None          # cleared whatever the answer was
    return x.grad


def test_one_consumer_the_sums_are_taken():
    assert torch.equal(_chain(None), torch.full((1000,), 6.0))
    assert TOOK == ["sums of this dx"]


@pytest.mark.parametrize("tap", ["before", "after"])
def test_a_second_consumer_the_sums_are_refused(tap):
    """Recorded before the consumer the tap's gradient arrives second (and is summed out of place: the link holds dx), recorded
    after it arrives first (and dx is summed into it): either way the producer receives another object."""
    assert torch.equal(_chain(tap), torch.full((1000,), 16.0))
    assert TOOK == [None]


def test_a_hook_that_returns_a_new_tensor_the_sums_are_refused():
    assert torch.equal(_chain("hook"), torch.full((1000,), 12.0))
    assert TOOK == [None]


def test_a_hook_that_edits_in_place_the_sums_are_refused_on_the_version():
    seen = []

    class _Watch(K.BnLink):     # the same object arrives, at another version
        __slots__ = ()

        def take_sums(self, dy):
            seen.append((dy is self._dx, dy._version, self._version))
            return super().take_sums(dy)

    TOOK.clear()
    x = torch.ones(1000, requires_grad=True)
    link = _Watch()
    ya = _Producer.apply(x, link)
    ya.register_hook(lambda g: g.mul_(2))
    _Consumer.apply(ya, link).sum().backward()
    assert seen == [(True, 1, 0)] and TOOK == [None]
    assert torch.equal(x.grad, torch.full((1000,), 12.0))
    assert torch.equal(_chain("hook_in_place"), torch.full((1000,), 12.0)) and TOOK == [None]


def test_sums_nobody_gave_are_not_taken():
    link = K.BnLink()
    assert link.take_sums(torch.ones(2)) is None


# ---------------------------------------------------------------- the offer from block to block
class _Out(torch.autograd.Function):
    """A block's output unit: its ctx keeps the link, as the producer of a BnLink does."""

    @staticmethod
    def forward(ctx, x, link):
        ctx.link = link
        link.src = (x.detach(),)
        return x * 2

    @staticmethod
    def backward(ctx, dy):
        return dy * 2, None


def test_the_offer_is_taken_by_the_block_whose_input_is_that_tensor_once():
    link = K.BnLink()
    y = _Out.apply(torch.ones(3, requires_grad=True), link)
    K.offer(y, link)
    assert K.take_offer(torch.relu(y)) is None and K.take_offer(y * 1.0) is None and K.take_offer(y.detach()) is None
    assert K.take_offer(y) is link
    assert K.take_offer(y) is None
    K.offer(y, None)                                  # no link (hand-over off): nothing to find
    assert K.take_offer(y) is None


def test_the_offer_does_not_keep_its_tensor_alive():
    link = K.BnLink()
    gc.collect()
    gc.disable()                                      # reference counts alone must free it: no cycle through the link
    try:
        y = _Out.apply(torch.ones(3, requires_grad=True), link)
        K.offer(y, link)
        ref = weakref.ref(y)
        del y
        assert ref() is None
    finally:
        gc.enable()


# ---------------------------------------------------------------- ResLink
@pytest.mark.parametrize("what", ["affine", "short", "mask", "done"])
def test_each_hand_over_of_a_reslink_reads_and_clears(what):
    link = K.ResLink()
    assert link.take(what) is None                    # never given
    v = object()
    link.give(what, v)
    for other in {"affine", "short", "mask", "done"} - {what}:
        assert link.take(other) is None
    assert link.take(what) is v
    assert link.take(what) is None
    with pytest.raises(AttributeError):
        link.give("dz", v)                            # no such hand-over
