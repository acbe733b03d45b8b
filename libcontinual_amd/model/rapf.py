"""RAPF plugin (reference core/model/rapf.py) on the CLIP backbone: a frozen CLIP tower, one trainable `Linear(E, E, bias=False)` adapter on the image
features, replay of draws from per-class Gaussians from task 1 on, a hinge loss on "hard pairs" (old / new classes whose text features are close), and after
each task a mix of the new adapter with the old one in the old one's singular basis.

Hot loop (observe / backward / step) = HIP: one no-grad executor forward plus `visual.proj` gives the image rows; clhip_rapf_draw writes the replay and edge
draws behind them into the step's row matrix; clhip_rapf_step_fwd forms the adapter output, the normalisation, the CLIP logits, cross entropy, hinge and the
gradient at the adapter's output; the loss's backward is clhip_rapf_step_bwd into `adapter.weight.grad` (csrc/rapf.hip).  Adam and MultiStepLR are the
trainer's.  Per-task host logic stays in torch where the reference runs it: the hard pairs (`cdist(new, old) < threshold`, rapf.py:181-192), the shuffle of the
old classes (:264-266), `shrink_cov` (:26-36) and `mix_matrix` (:212-225).

Different by design:
  * the text tower is frozen, so the normalised text features are computed ONCE per task (the reference re-encodes them in every forward, :128-129);
  * a class's covariance never changes after `after_task`, so it is factored there, once (`class_align._cholesky`); the reference calls
    `torch.linalg.cholesky` on every sampled class in every step (:41) -- that is where its step time goes.  `shrinkage: true` is deterministic and is
    applied once, to the matrix that is factored; `class_covs` keeps the unshrunk estimate the reference stores;
  * mean and covariance come from clhip_class_moments (same formula as :204-205, unbiased + 1e-4 I);
  * the edge and text rows are normalised once, not twice (:343-347 is the identity on unit vectors, in value and in Jacobian);
  * the adapter's width is the backbone's embedding width, not the literal 512 of :84;
  * randomness: the shuffle of the old classes and the normals go through `class_order_fn(task_idx, classes)` and `normal_fn(shape)`; the defaults are a
    `random.Random(seed)` owned by the method and `torch.randn` on the device.  The reference draws both from the global generators that `seed_everything`
    seeds, whose streams also feed everything else in the process: they cannot be matched, the seed governs both.
Not built, because the reference computes it and never reads it: `old_adapter(memory_data)` (:157-159), `class_edge_distance` (:206-208) and
`sample_after_adapt_feature` (:281).

Evaluation: `inference` returns (softmax probabilities, accuracy) as :365-377 does.  The trainer's per-task evaluation (`testing_per_task: true`, the default
of the headers and of the reference's RAPF configs) reads only the accuracy.  Its merged evaluation compares `output` with the labels as predictions
(trainer.py:653; reference core/trainer.py:699-702): with the reference's return value that comparison is between a [B, C] matrix and [B] labels and cannot
work there either, so `before_task` refuses `testing_per_task: false` when it is told of it (kwarg `testing_per_task`), and nothing is invented.

`cuda_graph_safe = False`: the host picks the replay classes of a step from `batch_id`.
"""
import copy
import random

import torch
import torch.nn as nn

from .. import ops
from ..utils import device_svd
from .backbone.clip import CLIP
from .backbone.clip_tokenizer import tokenize
from .class_align import COV_EPS, _cholesky

MARGIN = 0.1                                                              # rapf.py:348


def shrink_cov(cov):
    """rapf.py:26-36 (alpha1 = alpha2 = 1)"""
    diag_mean = torch.mean(torch.diagonal(cov))
    off = cov.clone()
    off.fill_diagonal_(0.0)
    mask = off != 0.0
    off_mean = (off * mask).sum() / mask.sum()
    iden = torch.eye(cov.shape[0], device=cov.device, dtype=cov.dtype)
    return cov + diag_mean * iden + off_mean * (1 - iden)


def hard_pairs(text_features, prev_cls_num, threshold):
    """[P, 2] int64 (old class, new class) with |t_new - t_old| < threshold, old-major and new-minor: the order of torch.nonzero over the [old, new] distance
    table of rapf.py:181-192; the new class carries its label (the reference's offset init + (task - 1) * inc is prev_cls_num)"""
    t = text_features.float()
    idx = torch.nonzero(torch.cdist(t[:prev_cls_num], t[prev_cls_num:]) < threshold)
    idx[:, 1] += prev_cls_num
    return idx


def replay_classes(order, batch_id, inc_cls_num):
    """rapf.py:312-315: two classes of the shuffled old-class list per batch, four when inc_cls_num == 5, walking the list with the batch index"""
    k = 4 if inc_cls_num == 5 else 2
    return [order[(batch_id * k + i) % len(order)] for i in range(k)]


def mix_matrix(weight_new, weight_old, mix_bias):
    """rapf.py:212-225 in fp64: P = U^T W_new against S V of the old weight, mask = min(|P - S V| / max + mix_bias, 1), U (P mask + S V (1 - mask)).  A sign flip
    of a singular pair flips a row of P and of S V together and a column of U: the result does not depend on it."""
    U, S, Vh = device_svd(weight_old.detach().double(), full_matrices=True)
    U, SV = torch.from_numpy(U), torch.from_numpy(S[:, None] * Vh)
    P = U.T @ weight_new.detach().double().cpu()
    dist = (P - SV).abs()
    mask = torch.clamp(dist / dist.max() + mix_bias, max=1)
    return U @ (P * mask + SV * (1 - mask))


class RAPF(nn.Module):
    cuda_graph_safe = False

    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        if kwargs.get("fp16", False):
            raise NotImplementedError("fp16: true runs the adapter stage in half precision (rapf.py:83, :136-143); the adapter stage is fp32 here")
        if not isinstance(backbone, CLIP):
            raise NotImplementedError(f"RAPF needs this project's CLIP backbone (backbone.name: clip), got {type(backbone).__name__}")
        if int(kwargs.get("n_gpu", 1) or 1) > 1:
            raise NotImplementedError("n_gpu > 1 with the CLIP backbone: data parallelism is not built on this backbone")
        self.backbone, self.device, self.kwargs = backbone, device, kwargs
        self.init_cls_num, self.inc_cls_num = kwargs["init_cls_num"], kwargs["inc_cls_num"]
        self.beta, self.shrinkage, self.threshold, self.mix_bias = kwargs["beta"], bool(kwargs["shrinkage"]), kwargs["threshold"], kwargs["mix_bias"]
        self.prompt_template = kwargs["prompt_template"]
        self.seed = kwargs.get("seed", 0)
        self._testing_per_task = kwargs.get("testing_per_task", True)
        self._class_tokens, self._bpe_path = kwargs.get("class_tokens"), kwargs.get("bpe_path")
        if self._class_tokens is not None:
            self._class_tokens = torch.as_tensor(self._class_tokens, dtype=torch.int64)
            if self._class_tokens.dim() != 2:
                raise ValueError(f"class_tokens must be [classes, context length] in label order, got {tuple(self._class_tokens.shape)}")
        E = backbone.visual.output_dim
        self.embed_dim = E
        for p in backbone.parameters():                                  # the tower is frozen (get_parameters returns the adapter only, rapf.py:289-290)
            p.requires_grad_(False)
        self.adapter = nn.Linear(E, E, bias=False)
        self.old_adapter = None
        self.classes_names = None                                        # label -> name: the train loader's cls_map (reference trainer.py:280-281)
        self.current_class_names = []
        self.class_name_features = None                                  # [classes so far, E], normalised, fp32, on the device
        self.hard_pairs = None
        self.class_means = torch.zeros(0, E, device=device)
        self.class_covs = torch.zeros(0, E, E, device=device)
        self.class_chols = torch.zeros(0, E, E, device=device)
        self.prev_cls_num = self.accu_cls_num = 0
        self.task_id = -1
        self.random_class_order_list = None
        self._rng = random.Random(self.seed)
        self.class_order_fn = None                                       # (task_idx, classes) -> shuffled list; None: self._rng.shuffle
        self.normal_fn = None                                            # (shape) -> standard normals on the device; None: torch.randn
        self._scale = self._pos = self._neg = self._projT = None
        self.last_step = None

    def set_class_names(self, cls_map):
        self.classes_names = cls_map

    def get_parameters(self, config):
        return self.adapter.parameters()

    # ------------------------------------------------------------------------------------------ the frozen tower
    @torch.no_grad()
    def image_features(self, x):
        """un-normalised image features [B, E]: the input rounded through fp16 as rapf.py:127 does, the executor forward, visual.proj"""
        x = x.to(self.device)
        x = x.to(torch.float16).to(torch.float32)
        was = self.backbone.training
        self.backbone.eval()
        try:
            feat = self.backbone.visual.features(x, None, False)
            if self._projT is None or self._projT.device != feat.device:
                self._projT = self.backbone.visual.proj.detach().float().t().contiguous()
            return ops.linear(feat.float(), self._projT)
        finally:
            self.backbone.train(was)

    # ------------------------------------------------------------------------------------------ hooks
    @torch.no_grad()
    def before_task(self, task_idx, buffer, train_loader, test_loaders):
        if not self._testing_per_task:
            raise NotImplementedError("testing_per_task: false reads inference()'s first value as predictions; RAPF returns probabilities there, as the reference "
                                      "does (rapf.py:365-377), and the reference's merged evaluation cannot compare them with the labels either")
        self.task_id = task_idx
        self.accu_cls_num = self.init_cls_num if task_idx == 0 else self.accu_cls_num + self.inc_cls_num
        if self._class_tokens is not None:
            if self._class_tokens.shape[0] < self.accu_cls_num:
                raise ValueError(f"class_tokens has {self._class_tokens.shape[0]} rows; task {task_idx} needs {self.accu_cls_num}")
            tokens = self._class_tokens[: self.accu_cls_num]
        else:
            if self.classes_names is None:
                raise ValueError("RAPF needs the class names: the trainer hands the train loader's cls_map to set_class_names(); without names give "
                                 "classifier.kwargs.class_tokens")
            self.current_class_names += [self.classes_names[i] for i in range(self.prev_cls_num, self.accu_cls_num)]      # rapf.py:170
            tokens = tokenize([self.prompt_template.format(c) for c in self.current_class_names], self.backbone.context_length, self._bpe_path)
        self.class_name_features = self.backbone.text_features(tokens.to(self.device))       # once per task: the text tower is frozen
        self._scale = float(self.backbone.logit_scale.exp())
        self.hard_pairs, self._pos, self._neg = None, None, None
        if task_idx > 0:
            self.old_adapter = copy.deepcopy(self.adapter)
            self.hard_pairs = hard_pairs(self.class_name_features, self.prev_cls_num, self.threshold).cpu()
            n = int(20 * self.beta)
            if self.hard_pairs.shape[0] > 0:
                self._pos = self.hard_pairs[:, 0].repeat_interleave(n).to(self.device)
                self._neg = self.hard_pairs[:, 1].repeat_interleave(n).to(self.device)
            classes = list(range(self.prev_cls_num))                     # rapf.py:264-266
            if self.class_order_fn is not None:
                classes = [int(c) for c in self.class_order_fn(task_idx, classes)]
                if sorted(classes) != list(range(self.prev_cls_num)):
                    raise ValueError("class_order_fn must return a permutation of the old classes")
            else:
                self._rng.shuffle(classes)
            self.random_class_order_list = classes

    def _normals(self, shape):
        if self.normal_fn is not None:
            return self.normal_fn(shape).to(self.device, torch.float32).contiguous()
        return torch.randn(shape, device=self.device)

    def observe(self, data):
        y = data["label"].to(self.device)
        feats = self.image_features(data["image"])
        B, E = feats.shape
        cls, cnt, labels = [], [], y
        if self.task_id > 0:
            cls = replay_classes(self.random_class_order_list, int(data["batch_id"]), self.inc_cls_num)
            cnt = [int(10 * self.beta)] * len(cls)
            labels = torch.cat([y, torch.tensor(cls, dtype=torch.int64).repeat_interleave(cnt[0]).to(self.device, non_blocking=True)])
            if self._pos is not None:
                cls = cls + self.hard_pairs[:, 0].tolist()
                cnt = cnt + [int(20 * self.beta)] * self.hard_pairs.shape[0]
        n_draw = sum(cnt)
        if n_draw:
            X = torch.empty(B + n_draw, E, device=self.device, dtype=torch.float32)
            X[:B] = feats
            ops.rapf_draw(self.class_means, self.class_chols, self._normals((n_draw, E)), X, B, cls, cnt)      # replay and edge groups in one call
        else:
            X = feats
        loss, st = ops.rapf_loss(self.adapter.weight, X, self.class_name_features, self._scale, labels, self._pos, self._neg, B, MARGIN)
        self.last_step = st
        aux = ops.LossAux()
        aux.pred, aux.correct, aux.batch = st.pred, st.correct, B
        return st.pred, aux.acc(), loss

    @torch.no_grad()
    def inference(self, data, task_id=None):
        y = data["label"].to(self.device)
        st = ops.rapf_step_fwd(self.image_features(data["image"]), self.adapter.weight.detach(), self.class_name_features, self._scale)
        prob = torch.softmax(st.logits, dim=-1)
        return prob, (prob.argmax(dim=1) == y).sum().item() / y.size(0)

    @torch.no_grad()
    def after_task(self, task_idx, buffer, train_loader, test_loaders):
        feats, labels = [], []
        for batch in train_loader:
            feats.append(self.image_features(batch["image"]))
            labels.append(batch["label"].to(self.device))
        self.add_class_statistics(torch.cat(feats), torch.cat(labels))
        if self.old_adapter is not None:
            mixed = mix_matrix(self.adapter.weight, self.old_adapter.weight, self.mix_bias)
            self.adapter.weight.copy_(mixed.to(self.adapter.weight))
        self.prev_cls_num = self.accu_cls_num

    @torch.no_grad()
    def add_class_statistics(self, feats, labels):
        """analyze_mean_cov (rapf.py:198-210) for the classes of `labels`, in ascending label order, which must continue the stored ones"""
        feats = feats.to(self.device, torch.float32).contiguous()
        labels = labels.to(self.device, torch.int64)
        lo = self.class_means.shape[0]
        local = labels - lo
        n_cls = int(local.max()) + 1 if local.numel() else 0
        counts = torch.bincount(local.clamp(min=0), minlength=max(n_cls, 1))
        if n_cls < 1 or int(local.min()) < 0 or int(counts.min()) < 2:
            raise ValueError(f"classes are added in label order behind the {lo} stored ones, at least two rows each")
        order = torch.argsort(local, stable=True)
        offsets = torch.zeros(n_cls + 1, dtype=torch.int32, device=self.device)
        offsets[1:] = torch.cumsum(counts, 0)
        mean, cov = ops.class_moments(feats[order], offsets, COV_EPS)
        factored = torch.stack([shrink_cov(c) for c in cov]) if self.shrinkage else cov
        self.class_means = torch.cat((self.class_means, mean))
        self.class_covs = torch.cat((self.class_covs, cov))
        self.class_chols = torch.cat((self.class_chols, _cholesky(factored)))
        return mean, cov
