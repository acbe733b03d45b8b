"""Classifier alignment, the "+CA" variant of InfLoRA_OPT (reference core/model/InfLoRA_opt.py:371-456), on the fp32 MFMA kernels of csrc/ca.hip.

After every task a Gaussian per class is stored over the backbone features of the task's training set (`_create_distribution`, :371-397); from
task 1 on all heads seen so far are re-trained on rows drawn from those Gaussians (`_compact_classifier`, :399-456): 5 epochs, 256 rows per class,
SGD(lr 0.01, momentum 0.9, weight decay 5e-4) under CosineAnnealingLR(T_max = 5), the mean of a class of task t scaled by
0.9 + 0.1 (t + 1) / (task_idx + 1), the rows of an epoch shuffled and consumed 256 at a time, cross-entropy over all heads.

Kept from the reference: the constants, torch.cov's unbiased estimate in fp32 storage plus 1e-4 I, `MultivariateNormal.sample` as mean + L z with L
the fp32 Cholesky factor, the shuffle by a CPU `torch.randperm`, the per-epoch schedule, one optimizer state per alignment.
Different by design: means, covariances and factors live on the device; a class is factored ONCE, when its Gaussian is created (the reference
re-factors every class in every epoch, and the covariance never changes); the heads are trained as one flat [classes, feat_dim] matrix without
autograd -- SGD is element-wise, so this is the reference's per-parameter optimizer over the concatenated logits; the normals come from
`torch.randn` on the device (the reference's stream cannot be matched anyway: the seed governs both).
"""
import os

import numpy as np
import torch

from .. import ops

EPOCHS, NUM_SAMPLE, LR, MOMENTUM, WEIGHT_DECAY = 5, 256, 0.01, 0.9, 5e-4          # InfLoRA_opt.py:402-406
COV_EPS = 1e-4                                                                    # InfLoRA_opt.py:397


def _cholesky(A):
    """torch.linalg.cholesky on the device in fp32 -- what MultivariateNormal(mean, cov) computes at InfLoRA_opt.py:425.  Where the device solver is
    unavailable (or CLHIP_SOLVE=host) the factor is taken on the host in fp64, the fallback shape of ranpac._solve."""
    if os.environ.get("CLHIP_SOLVE", "device") != "host":
        try:
            return torch.linalg.cholesky(A)
        except RuntimeError as e:
            if "positive-definite" in str(e):
                raise
    return torch.from_numpy(np.linalg.cholesky(A.double().cpu().numpy())).to(A)


def epoch_lrs():
    """the learning rate of every epoch under torch's CosineAnnealingLR(T_max = EPOCHS), read off the scheduler itself (InfLoRA_opt.py:412-413, :456)"""
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=LR, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer=opt, T_max=EPOCHS)
    lrs = []
    for _ in range(EPOCHS):
        lrs.append(float(opt.param_groups[0]["lr"]))
        opt.step()
        sched.step()
    return lrs


class ClassAligner:
    """The alignment without a backbone.  `add_task(features, labels, class_lo, n_classes)` is `_create_distribution` on given features [N, feat_dim]
    (rows in loader order), `align(heads, task_idx, inc_cls_num)` is `_compact_classifier`.  State: means [classes, D], covs and chols
    [classes, D, D], fp32 on `device`."""

    def __init__(self, feat_dim, device):
        self.feat_dim, self.device = int(feat_dim), torch.device(device)
        D = self.feat_dim
        self.means = torch.zeros(0, D, device=self.device)
        self.covs = torch.zeros(0, D, D, device=self.device)
        self.chols = torch.zeros(0, D, D, device=self.device)

    @torch.no_grad()
    def add_task(self, features, labels, class_lo, n_classes):
        feats = features.detach().to(self.device, torch.float32).contiguous()
        local = labels.detach().to(self.device, torch.int64) - int(class_lo)
        if feats.shape[1] != self.feat_dim or local.numel() != feats.shape[0]:
            raise ValueError(f"features {tuple(feats.shape)} / labels {tuple(local.shape)} do not fit feat_dim {self.feat_dim}")
        if int(class_lo) != self.means.shape[0]:
            raise ValueError(f"classes are added in order: {self.means.shape[0]} stored, class_lo {class_lo}")
        if local.numel() == 0 or int(local.min()) < 0 or int(local.max()) >= int(n_classes):
            raise ValueError(f"labels outside [{class_lo}, {int(class_lo) + int(n_classes)})")
        order = torch.argsort(local, stable=True)                     # the rows of a class keep the loader's order (InfLoRA_opt.py:378-382)
        counts = torch.bincount(local, minlength=int(n_classes))
        offsets = torch.zeros(int(n_classes) + 1, dtype=torch.int32, device=self.device)
        offsets[1:] = torch.cumsum(counts, 0)
        mean, cov = ops.class_moments(feats[order], offsets, COV_EPS)
        chol = _cholesky(cov)
        self.means = torch.cat((self.means, mean))
        self.covs = torch.cat((self.covs, cov))
        self.chols = torch.cat((self.chols, chol))
        return mean, cov

    @torch.no_grad()
    def align(self, heads, task_idx, inc_cls_num, normal_fn=None, perm_fn=None):
        """`heads`: the linear heads of tasks 0 .. task_idx; their weights and biases are replaced by the aligned ones.
        `normal_fn(epoch, shape)` -> standard normals [classes * 256, D], class-major; `perm_fn(epoch, n)` -> the shuffle of the epoch's rows."""
        C, S, D = (int(task_idx) + 1) * int(inc_cls_num), NUM_SAMPLE, self.feat_dim
        outs = [h.weight.shape[0] for h in heads]
        if C != self.means.shape[0] or sum(outs) != C:
            raise ValueError(f"{C} classes up to task {task_idx}, {self.means.shape[0]} Gaussians stored, heads of {outs}")
        if normal_fn is None:
            normal_fn = lambda ep, shape: torch.randn(shape, device=self.device)
        if perm_fn is None:
            perm_fn = lambda ep, n: torch.randperm(n)                 # InfLoRA_opt.py:435: the CPU generator
        W = torch.cat([h.weight.detach().to(self.device, torch.float32) for h in heads]).contiguous()
        b = torch.cat([h.bias.detach().to(self.device, torch.float32) for h in heads]).contiguous()
        mom_w, mom_b = torch.zeros_like(W), torch.zeros_like(b)
        task_id = torch.arange(C, device=self.device) // int(inc_cls_num)
        scale = (0.9 + (task_id + 1).double() / (int(task_idx) + 1) * 0.1).float()          # InfLoRA_opt.py:419-422
        ws = None
        for ep, lr in enumerate(epoch_lrs()):
            z = normal_fn(ep, (C * S, D)).to(self.device, torch.float32)
            perm = torch.as_tensor(perm_fn(ep, C * S)).to(self.device, torch.int64)
            dest = torch.empty_like(perm)
            dest[perm] = torch.arange(C * S, device=self.device)      # inputs[sf_indexes] (:436): row perm[r] of the draws becomes row r
            X, y = ops.ca_sample(self.means, scale, self.chols, z, dest, 0)
            for it in range(C):                                       # InfLoRA_opt.py:439-454
                ws = ops.head_sgd_step(X[it * S:(it + 1) * S], y[it * S:(it + 1) * S], W, b, mom_w, mom_b, lr, MOMENTUM, WEIGHT_DECAY, ws)
        lo = 0
        for h, n in zip(heads, outs):
            h.weight.copy_(W[lo:lo + n])
            h.bias.copy_(b[lo:lo + n])
            lo += n
        return W, b
