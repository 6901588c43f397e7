"""Hand-overs between the autograd nodes of the regressor's conv + BatchNorm units: the state, without the library.

hip_ops' nodes skip passes that autograd would issue by handing tensors to one another.  Each hand-over is a give / take pair on
one of the links below; a take reads AND clears, and a take of something never given returns None.  Nothing here imports the
library: tests/test_block_links_host.py drives the links with toy Functions on CPU tensors."""


class GradLink:
    """Sums the gradient of a tensor that is used twice inside a Bottleneck (the block input: conv1 + identity shortcut, or
    conv1 + shortcut convolution) in the data-gradient GEMM that runs last, instead of by autograd's accumulation pass.
    `takers`: how many convolutions read the tensor and `take()` in their backward (2 with a shortcut convolution, 1 with an
    identity shortcut).  Whoever runs before the last taker parks its contribution."""
    __slots__ = ("_g", "_mask", "_left")

    def __init__(self, takers: int):
        self._g = self._mask = None
        self._left = takers

    def park(self, g, mask=None) -> None:     # mask: byte mask that gates g (identity shortcut: g is the block's raw dy)
        self._g, self._mask = g, mask

    def take(self):
        """One taker runs its backward: (addend, mask, last); the last one's data gradient is the complete gradient.  The
        link is consumed by ONE backward pass over the graph; a second pass (retain_graph=True, torch.autograd.grad twice)
        would silently drop the parked partial sums, so it raises instead."""
        if self._left <= 0:
            raise RuntimeError("hiddenpose_amd: a Bottleneck's fused gradient link was already consumed -- a second backward "
                               "pass over the same graph (retain_graph=True) is not supported; run the forward again")
        self._left -= 1
        g, mask = self._g, self._mask
        self._g = self._mask = None
        return g, mask, self._left == 0


class ResLink:
    """Joins the shortcut unit (downsample conv + BatchNorm) of a Bottleneck to the output unit that adds it as the residual.
    affine  forward, shortcut -> output unit: (mean, rstd, gamma, beta).  The shortcut hands on its RAW convolution output and
            the output unit applies both BatchNorms in one pass.
    short   forward -> the output unit's backward: (z, mean, rstd, gamma, train) of the shortcut, so that that backward can
            run both BatchNorm backwards in one pair of passes;
    done    backward, output unit -> shortcut: the (dz, dgamma, dbeta) it then leaves for the shortcut.
    mask    backward, output unit -> shortcut, where it does not: the byte mask of the block output.  The output unit hands on
            its raw dy, and the shortcut's BatchNorm backward applies the mask while it reads dy."""
    __slots__ = ("affine", "short", "mask", "done")

    def __init__(self):
        self.affine = self.short = self.mask = self.done = None

    def give(self, what: str, v) -> None:
        setattr(self, what, v)

    def take(self, what: str):
        v = getattr(self, what)
        setattr(self, what, None)
        return v


class BnLink:
    """Joins a conv + BatchNorm (+ ReLU) unit (the producer) to the ONE convolution that consumes its output.  The consumer's
    data gradient dx IS the producer's incoming gradient, so the consumer's data-gradient kernel also takes the producer's
    two BatchNorm-backward sums and the producer skips its reduction pass.  `src`: what that kernel needs of the producer
    (z, mean, rstd, gamma, beta, relu, byte mask or None), set by the producer's forward.

    That the output has ONE consumer is the caller's wiring, so the sums count only for the gradient they were taken from: the
    link holds dx itself (the producer's live dy for exactly that span: no lifetime is extended) and `take_sums` hands them out
    only if the producer's incoming gradient is that very object at the recorded version.  A second consumer or a hook that
    returns a new tensor makes autograd pass another object, a hook that edits in place bumps the version; the producer then
    runs its own reduction.  (data_ptr() does not tell: with nobody holding dx autograd sums a second gradient INTO it.)"""
    __slots__ = ("src", "sums", "_dx", "_version")

    def __init__(self):
        self.src = self.sums = self._dx = self._version = None

    def give_sums(self, sums, dx) -> None:
        self.sums, self._dx, self._version = sums, dx, dx._version

    def take_sums(self, dy):
        """From the producer's backward, with its incoming gradient as autograd passed it (before any .contiguous())."""
        sums, dx = self.sums, self._dx
        self.sums = self._dx = None
        return sums if (dx is not None and dy is dx and dy._version == self._version) else None


# A Bottleneck's OUTPUT unit (bn3 + identity shortcut + ReLU) is consumed by the next block's conv1 and identity shortcut.  Its
# gradient is complete in the epilogue of that conv1's data gradient (it adds the parked shortcut gradient), so conv1 of the NEXT
# block is the consumer of this unit's BnLink.  The two forwards do not see each other (blocks sit in an nn.Sequential): the
# offer travels on the output tensor object and only a block whose input IS that object finds it.  No cycle: the link does not
# reference the tensor that carries it.
def offer(y, link) -> None:
    if link is not None:
        y._hp_bn_offer = link


def take_offer(x):
    link = getattr(x, "_hp_bn_offer", None)
    if link is not None:
        del x._hp_bn_offer
    return link
