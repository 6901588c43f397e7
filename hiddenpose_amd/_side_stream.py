"""Weight gradients on a second HIP stream: the mechanism.  hip_ops keeps the policy (the switches, and which gradients gain).

A weight gradient has no reader before the optimizer, so its kernel may run on a side stream next to the rest of backward and
be joined when the backward pass ends.  That is safe only where nothing reads the gradient on the main stream before the join:

* `register` / `release`: a parameter used more than once among the graphs being differentiated has its gradients SUMMED by
  autograd on the main stream.  Every Function adds its `ctx` to the weak set `p._hp_uses` in `forward` and takes it out in
  `backward`.  A ctx lives exactly as long as its graph, so a graph that is dropped without a backward leaves the set by itself:
  there is no forward epoch to open and nothing to prune.
* `adoptable`: hooks and gradients that are not a leaf's.
* `stream` / `launch` / `join`: the stream, the hand-over and the end-of-backward join.

Two ownership rules keep the allocator out of the exchange (no block is owned by, or recorded on, the side stream):
1. The caller allocates the outputs on the MAIN stream before `launch` (written on the side stream, read and freed on the main
   one after the join).
2. A gradient that goes back to autograd must not be referenced by `keep`, nor by anything that outlives the caller's frame:
   autograd adopts a gradient as `.grad` only while nobody else references it and would otherwise clone it -- on the main
   stream, before the side stream has written it.  A gradient that was summed into `.grad` on the side stream dies with the
   call and MUST be in `keep`: its block was allocated on the main stream.
"""
from __future__ import annotations

import collections
import weakref

import torch

from ._lib import env_int

_PRIO = env_int("HP_WGRAD_PRIO", 0)
_HOLD_DEPTH = env_int("HP_WGRAD_HOLD", 4)
_streams = {}        # device -> side stream
_held = {}           # device -> deque of (event recorded behind a side-stream kernel, the operands it reads)
_joined_task = [-1]
# callables (parameter, side_stream) run after a weight gradient was ACCUMULATED into `.grad` on the side stream
listeners = []


def register(ctx, params) -> None:
    """From `Function.forward`.  params: {position among forward's inputs: parameter or None}.  `ctx.needs_input_grad` is what
    says whether the caller will differentiate (grad mode is always off inside `forward`); under no_grad, or for a frozen
    parameter, nothing registers."""
    for i, p in params.items():
        if p is None or not ctx.needs_input_grad[i]:
            continue
        uses = getattr(p, "_hp_uses", None)
        if uses is None:
            uses = p._hp_uses = weakref.WeakSet()
        if not uses:
            p._hp_shared = False    # a mark left behind by a graph that was discarded half-way through its uses
        uses.add(ctx)


def release(ctx, *params) -> bool:
    """From `backward`, always (a switch may only decide what the caller does with the answer).  True = these gradients stay on
    the main stream: one of the parameters has more than one live use, or this use is not registered (a frozen parameter, whose
    gradient autograd drops at once; a second backward over a retained graph; a tensor that saved-tensor hooks replaced).  The
    sticky mark `_hp_shared` keeps the LAST of several uses on the main stream too: it sees one live use, its own."""
    main = False
    for p in params:
        if p is None:
            continue
        uses = getattr(p, "_hp_uses", ())
        if len(uses) > 1:
            p._hp_shared = True
        if ctx not in uses or getattr(p, "_hp_shared", False):
            main = True
        if uses:
            uses.discard(ctx)
            if not uses:
                p._hp_shared = False
    return main


def adoptable(params, allow_accumulate: bool) -> bool:
    """True if nothing reads these gradients on the main stream before the join: leaves whose gradient autograd merely adopts
    as `.grad`.  A tensor hook receives the gradient and a post-accumulate hook may read it.  With `allow_accumulate` a leaf that
    already holds a `.grad` passes, hook or not: the caller then sums into it on the side stream and hands autograd nothing."""
    for p in params:
        if not p.is_leaf or getattr(p, "_backward_hooks", None):
            return False
        if not (allow_accumulate and p.grad is not None) and (p.grad is not None or getattr(p, "_post_accumulate_grad_hooks", None)):
            return False
    return True


def stream(device):
    """The side stream of `device`, or None outside a backward pass: `join` is queued as an end-of-backward callback of the
    pass, once per graph task."""
    task = torch._C._current_graph_task_id()
    if task == -1:
        return None
    s = _streams.get(device)
    if s is None:
        # Same priority as the training stream.  HIP offers two levels on this device (priority_range() = (0, -1)); giving the
        # training stream -- backward's critical path -- the high one, or the weight gradients the high one, measured 455.5 /
        # 455.2 ms against 456.6 (HP_MAIN_PRIO in bench.py, HP_WGRAD_PRIO here: A/B hooks): inside the noise
        s = _streams[device] = torch.cuda.Stream(device, priority=_PRIO)
    if _joined_task[0] != task:
        _joined_task[0] = task
        torch.autograd.Variable._execution_engine.queue_callback(join)
    return s


def launch(device, side, fn, keep) -> None:
    """Runs fn(stream handle) with `side` current, behind everything queued on the main stream so far, and keeps `keep` (the
    operands) alive until the main stream has waited for it.

    The operands stay referenced here -- NOT handed to the allocator with record_stream(): a record_stream'ed block is reusable
    only once the HOST has seen its event complete, and in a training loop the host runs a whole step ahead of the device, so
    those blocks were never reusable in time, the pool grew until allocation failed and every step paid for the allocator's
    free-everything-and-synchronize path (measured: 1.2 s instead of 0.47 s per headline step with no host synchronisation
    between steps).  Instead the MAIN stream waits for the weight gradient of `_HOLD_DEPTH` launches ago (a device-side wait,
    normally already satisfied: the side stream runs one or two kernels behind) and only then is the reference dropped, so the
    block returns to the allocator as an ordinary main-stream block, in stream order, and at most `_HOLD_DEPTH` launches'
    operands are held beyond their autograd lifetime."""
    main = torch.cuda.current_stream(device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        fn(side.cuda_stream)
    ev = torch.cuda.Event()
    ev.record(side)
    q = _held.setdefault(device, collections.deque())
    q.append((ev, keep))
    while len(q) > _HOLD_DEPTH:
        ev0, _ = q.popleft()
        main.wait_event(ev0)     # whatever reuses those blocks on the main stream is ordered behind the kernel that read them


def join() -> None:
    """The current stream of every device waits for the weight gradients queued on its side stream.  Runs by itself
    when the backward pass that queued them ends, i.e. before `backward()` returns to the caller."""
    for dev, s in _streams.items():
        torch.cuda.current_stream(dev).wait_stream(s)
        q = _held.get(dev)
        if q:
            q.clear()            # everything queued so far is ordered before whatever the main stream does next
