"""Training loops of the transformer heads on their own losses.

Counterparts of utils/train_2d_heatmap.py:8-44 (TokenPose-style (b, n, h, w) heat-maps on `JointsMSELoss`),
utils/train_3d_heatmap.py:8-43 (3-D heat-maps on `L2JointLocationLoss`) and utils/train_simdr.py:8-69 ((b, n, 3, bins)
coordinate classifiers on `NMTNORMCritierion`), with the reference's positional signatures.  Per batch: forward, loss,
zero_grad, backward, step.  As in train_epoch.py the reference's per-step `loss.item()` prints are not reproduced: the loss is
accumulated on the device and read back once per 100 iterations, so a loop never stalls the GPU.  `writer` may be None.
Each loop returns the per-step losses of the epoch as one device tensor (no read-back happens for it).
"""
from __future__ import annotations

import time

import torch


class _Window:
    """Running 100-iteration mean of the loss, kept on the device."""

    def __init__(self, device, writer, tag="loss"):
        self.sum = torch.zeros((), dtype=torch.float32, device=device)
        self.writer, self.tag, self.t0 = writer, tag, time.time()

    def add(self, loss, global_iter_num):
        self.sum += loss
        if global_iter_num % 100 == 0:
            mean100 = float(self.sum) / 100.0        # the only read-back of the loop
            self.sum.zero_()
            now = time.time()
            print(f"global iter is {global_iter_num}, loss is {mean100}, iter100 time is {now - self.t0}")
            self.t0 = now
            if self.writer is not None:
                self.writer.add_scalar(self.tag, mean100, global_iter_num)


def _step(loss, optimizer):
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach()


def _device(model):
    return next(model.parameters()).device


def train_2d_heatmap(cfg, train_loader, model, criterion, optimizer, epoch, result_dir, writer):
    """utils/train_2d_heatmap.py:8-44.  The model's output is (b, n, h, w) (TokenPose) or (b, n, h * w), reshaped with
    h = cfg.DATASET.HEATMAP_SIZE[0] as the reference does (:26); target (b, n, >= 2) holds (mu_x, mu_y) in heat-map pixels and
    may stay on the host (the criterion moves the b * n * 2 coordinates, never a map)."""
    model.train()
    device = _device(model)
    window = _Window(device, writer)
    losses = []
    for step, (input, target) in enumerate(train_loader):
        global_iter_num = epoch * len(train_loader) + step + 1
        output = model(torch.as_tensor(input).to(device))
        if output.dim() == 3:
            h = cfg.DATASET.HEATMAP_SIZE[0]
            output = output.reshape(output.shape[0], output.shape[1], h, output.shape[2] // h)
        target = torch.as_tensor(target)
        loss = criterion(output, target[:, :, :2], None, writer, global_iter_num)
        losses.append(_step(loss, optimizer))
        window.add(losses[-1], global_iter_num)
    return torch.stack(losses) if losses else torch.zeros(0, device=device)


def train_3d_heatmap(cfg, train_loader, model, criterion, optimizer, epoch, final_output_dir, writer):
    """utils/train_3d_heatmap.py:8-43: (b, n, d, h, w) heat-maps on L2JointLocationLoss; target (b, n, 3) in heat-map voxels,
    every joint visible."""
    model.train()
    device = _device(model)
    window = _Window(device, writer)
    losses = []
    for step, (input, target) in enumerate(train_loader):
        global_iter_num = epoch * len(train_loader) + step + 1
        output = model(torch.as_tensor(input).to(device))
        target = torch.as_tensor(target)
        gt = target.reshape(target.shape[0], -1).to(device=device, dtype=torch.float32)
        loss = criterion(output, gt, torch.ones_like(gt), writer, global_iter_num)
        losses.append(_step(loss, optimizer))
        window.add(losses[-1], global_iter_num)
    return torch.stack(losses) if losses else torch.zeros(0, device=device)


def train_simdr(cfg, train_loader, model, criterion, optimizer, epoch, output_dir, writer):
    """utils/train_simdr.py:8-69 as its commented line :50 states it: criterion(output[:, :, 0], output[:, :, 1],
    output[:, :, 2], target, weight) on a (b, n, 3, bins) output, with weights of ones.  (The reference's live body, an
    nn.MSELoss against tens scattered into a zero tensor, is a debugging leftover and is not reproduced.)  The three
    predictions are views of the packed output: nothing is copied."""
    model.train()
    device = _device(model)
    window = _Window(device, writer)
    losses = []
    for step, (input, target) in enumerate(train_loader):
        global_iter_num = epoch * len(train_loader) + step + 1
        output = model(torch.as_tensor(input).to(device))
        target = torch.as_tensor(target).to(device=device, dtype=torch.float32)
        loss = criterion(output[:, :, 0], output[:, :, 1], output[:, :, 2], target, None)
        losses.append(_step(loss, optimizer))
        window.add(losses[-1], global_iter_num)
    return torch.stack(losses) if losses else torch.zeros(0, device=device)
