"""InfLoRA_OPT plugin (reference core/model/InfLoRA_opt.py:46-460, ViT and CLIP branches) on the HIP ViT executor.

Same constructor kwargs, hooks and quirks: every task re-zeroes all `lora_B`, fixes
`lora_A` from the SVD of the (DualGPM-projected) input Gram, trains all `lora_B*` + the task's head
(`get_parameters` returns ALL network parameters; frozen ones keep `grad None` and are skipped by the optimizer),
labels offset by the known classes, CE on the current task's head only; after the task the LoRA branch is merged into
the qkv weight and the DualGPM bases are updated.

Hot loop (observe / backward / step) = HIP: effective-qkv refresh, one backbone forward, head + CE, one backbone
backward producing the 24 dB matrices through the rank-r shortcut.  Per-task host logic (SVD of 768x768 Grams,
DualGPM thresholds) stays on the host in torch / numpy exactly where the reference runs it (InfLoRA_opt.py:251-369);
the Gram itself (X^T X per layer, transformer.py:241-244) is accumulated on the device by the executor.
Classifier alignment (`use_ca: true`, InfLoRA_opt.py:285-288, :371-456): after every task a Gaussian per class over the backbone features, from
task 1 on all heads so far re-trained on draws from them -- class_align.ClassAligner on the kernels of csrc/ca.hip.  Two quirks of the reference
are guards here: with any dataset but cifar100 its loss branch is an empty `pass` (:445-447) and the first step fails on an undefined `loss`; and
both functions index classes as if init_cls_num == inc_cls_num (:377-381, :418-419).  The feature width is `embd_dim`, not the reference's literal 768.
The CLIP branch (`backbone: clip`, `visual_only: true`; InfLoRA_opt.py:60-66, :74-85, :123-128, :137-138, :166-171, :229-235): LoRA on k and v of the visual
tower only, a frozen text tower, CE on logit_scale * cos(image, text) against the text features of the running task's classes (training) or of all classes
so far (inference).  There is no classifier_pool; the trainable parameters are the visual lora_B only.  The text tower is frozen, so `update_fc` computes
the normalised text features of both class sets ONCE per task and keeps them (the reference recomputes identical values every step); a step is one executor
forward in CLIP mode plus csrc/clip.hip.  Class names come from `train_loader.dataset.get_class_names()` through backbone/clip_tokenizer.py, or, without
the merges file, from the kwarg `class_tokens` ([total classes, 77] int64 in label order).
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..utils import device_svd
from .backbone.clip import CLIP
from .backbone.clip_tokenizer import tokenize
from .backbone.vit import MultiHeadAttention_LoRA, ViTZoo
from .class_align import ClassAligner
from .heads import HipLinear


class SiNet(nn.Module):
    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        self._cur_task_id = -1
        self.backbone = backbone
        self.device = device
        self.is_clip = isinstance(backbone, CLIP)
        if self.is_clip:
            self.prompt_template = kwargs["prompt_template"]
            self.accm_class_names, self.curr_class_names = [], []
            self.accm_text_tokens = self.curr_text_tokens = None
            self.accm_text_features = self.curr_text_features = None      # normalised, fp32, on the device: fixed for the task (frozen text tower)
            self._class_tokens, self._bpe_path = kwargs.get("class_tokens"), kwargs.get("bpe_path")
            self._task_sizes = [kwargs["init_cls_num"]] + [kwargs["inc_cls_num"]] * (kwargs["task_num"] - 1)
            self._scale = None
            if self._class_tokens is not None:
                self._class_tokens = torch.as_tensor(self._class_tokens, dtype=torch.int64)
                if self._class_tokens.dim() != 2 or self._class_tokens.shape[0] < sum(self._task_sizes):
                    raise ValueError(f"class_tokens must be [>= {sum(self._task_sizes)} classes, context length] in label order, got {tuple(self._class_tokens.shape)}")
            return
        if not isinstance(backbone, ViTZoo):
            raise NotImplementedError("only the ViT and CLIP backbones are on the hot path (SURVEY.md section 8)")
        self.classifier_pool = nn.ModuleList(
            [HipLinear(kwargs["embd_dim"], kwargs["init_cls_num"], bias=True)] +
            [HipLinear(kwargs["embd_dim"], kwargs["inc_cls_num"], bias=True) for _ in range(kwargs["task_num"] - 1)])

    @torch.no_grad()
    def update_fc(self, train_loader):
        self._cur_task_id += 1
        if not self.is_clip:
            return
        t = self._cur_task_id
        if self._class_tokens is not None:
            known = sum(self._task_sizes[:t])
            curr, accm = self._class_tokens[known:known + self._task_sizes[t]], self._class_tokens[:known + self._task_sizes[t]]
        else:                                                            # InfLoRA_opt.py:76-85
            self.curr_class_names = list(train_loader.dataset.get_class_names())
            self.accm_class_names += self.curr_class_names
            curr = tokenize([self.prompt_template.format(c) for c in self.curr_class_names], self.backbone.context_length, self._bpe_path)
            accm = tokenize([self.prompt_template.format(c) for c in self.accm_class_names], self.backbone.context_length, self._bpe_path)
        self.curr_text_tokens, self.accm_text_tokens = curr.to(self.device), accm.to(self.device)
        self.curr_text_features = self.backbone.text_features(self.curr_text_tokens)
        self.accm_text_features = self.backbone.text_features(self.accm_text_tokens)
        self._scale = float(self.backbone.logit_scale.exp())             # frozen: read once per task, not once per step

    def get_feature(self, x):
        if self.is_clip:
            raise NotImplementedError("get_feature on the CLIP backbone is `assert 0` in the reference (InfLoRA_opt.py:88-94)")
        return self.backbone(x)

    def fc_only(self, x):
        if self.is_clip:
            raise NotImplementedError("fc_only on the CLIP backbone is `assert 0` in the reference (InfLoRA_opt.py:96-105)")
        return torch.cat([fc(x) for fc in self.classifier_pool[: self._cur_task_id + 1]], dim=1)

    def forward(self, x, inference=False):
        if self.is_clip:                                                 # InfLoRA_opt.py:123-128
            txt = self.accm_text_features if inference else self.curr_text_features
            return self.backbone.image_logits(x, txt, self._scale)[0]
        features = self.backbone(x)
        heads = self.classifier_pool[: self._cur_task_id + 1] if inference else [self.classifier_pool[self._cur_task_id]]
        return torch.cat([fc(features) for fc in heads], dim=1)

    def update_input_matrix(self, x):
        with torch.no_grad():
            if self.is_clip:                                             # (InfLoRA_opt.py:137-138 also runs the text tower, whose Grams nobody reads)
                self.backbone.visual.features(x, None, True)
            else:
                self.backbone(x, get_input_matrix=True)


class InfLoRA_OPT(nn.Module):
    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        self.device = device
        self.init_cls_num = kwargs["init_cls_num"]
        self.inc_cls_num = kwargs["inc_cls_num"]
        self.task_num = kwargs["task_num"]
        self.lame = kwargs["lame"]
        self.lamb = kwargs["lamb"]
        self._known_classes = 0
        self.feature_list = []
        self.project_type = []
        self._dataset = kwargs.get("dataset")
        self._use_class_alignment = bool(kwargs.get("use_ca", False))
        self._aligner = None
        if self._use_class_alignment:
            if self._dataset != "cifar100":
                raise NotImplementedError(f"use_ca with dataset {self._dataset!r}: the reference sets _logit_norm = 0.1 for every dataset but cifar100 and that "
                                          "branch of _compact_classifier is an empty `pass` (InfLoRA_opt.py:158, :445-447): its first step fails on an "
                                          "undefined `loss`")
            if self.init_cls_num != self.inc_cls_num:
                raise NotImplementedError(f"use_ca with init_cls_num {self.init_cls_num} != inc_cls_num {self.inc_cls_num}: _create_distribution and "
                                          "_compact_classifier index classes as if the two were equal (InfLoRA_opt.py:377-381, :418-419)")
            self._aligner = ClassAligner(kwargs["embd_dim"], device)
        self._is_clip = isinstance(backbone, CLIP)
        if self._is_clip:
            if not kwargs.get("visual_only", False):
                raise NotImplementedError("visual_only: false trains LoRA on the text tower too (InfLoRA_opt.py:170-171, :236-241): that needs a causal attention "
                                          "forward / backward in the executor, which is not built")
            if self._use_class_alignment:
                raise NotImplementedError("use_ca with the CLIP backbone: the reference's get_feature / fc_only are `assert 0` there (InfLoRA_opt.py:88-105)")
            if getattr(backbone, "lora_rank", 0) <= 0:
                raise NotImplementedError("the CLIP backbone was built without lora_rank (or with 0): the reference's block default (transformer.py:1293) gives a "
                                          "rank-0 LoRA, and InfLoRA_opt.py:256-257 has no row of lora_A to fill; set backbone.kwargs.lora_rank")
            if int(kwargs.get("n_gpu", 1) or 1) > 1:
                raise NotImplementedError("n_gpu > 1 with the CLIP backbone: data parallelism is not built on this backbone")
        self._network = SiNet(backbone, device, **kwargs).to(self.device)
        if self._is_clip:                                                # InfLoRA_opt.py:167-169: the visual tower's modules only
            self.visual_only = True
            self.attention_modules = [m for n, m in self._network.named_modules() if isinstance(m, MultiHeadAttention_LoRA) and "visual" in n]
        else:
            self.attention_modules = [m for m in self._network.modules() if isinstance(m, MultiHeadAttention_LoRA)]

    def observe(self, data):
        x, y = data["image"].to(self.device), data["label"].to(self.device) - self._known_classes
        logits = self._network(x)
        aux = ops.LossAux()
        loss = ops.classify_loss(logits, y, aux=aux)
        self._last_aux = aux
        return aux.pred, aux.acc(), loss

    def inference(self, data):
        x, y = data["image"].to(self.device), data["label"].to(self.device)
        with torch.no_grad():
            logits = self._network(x, inference=True)
        pred, correct = ops.predict(logits, y)
        return pred, correct.item() / y.size(0)

    @torch.no_grad()
    def before_task(self, task_idx, buffer, train_loader, test_loaders):
        if self._is_clip and torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError("n_gpu > 1 with the CLIP backbone: data parallelism is not built on this backbone")
        if task_idx == 1:
            self._known_classes = self.init_cls_num
        elif task_idx > 1:
            self._known_classes += self.inc_cls_num
        self._network.update_fc(train_loader)
        for module in self.attention_modules:
            module.init_param()
        for name, param in self._network.named_parameters():
            param.requires_grad_(False)
            if self._is_clip:                                            # InfLoRA_opt.py:229-235
                param.requires_grad_("visual" in name and "lora_B" in name)
            elif f"classifier_pool.{task_idx}." in name or "lora_B" in name:
                param.requires_grad_(True)
        for batch in train_loader:
            self._network.update_input_matrix(x=batch["image"].to(self.device))
        for i, module in enumerate(self.attention_modules):
            assert module.n_cur_matrix > 0
            cur_matrix = module.cur_matrix
            if task_idx > 0:
                assert self.project_type[i] in ("remove", "retain")
                feature_mat = torch.as_tensor(self.feature_list[i] @ self.feature_list[i].T, dtype=cur_matrix.dtype)
                cur_matrix = cur_matrix - feature_mat @ cur_matrix if self.project_type[i] == "remove" else feature_mat @ cur_matrix
            U = torch.from_numpy(device_svd(cur_matrix, full_matrices=False)[0]).to(cur_matrix.dtype)      # fp64 on the GPU (utils.device_svd)
            A = (U[:, : module.lora_rank].T / math.sqrt(3)).to(module.lora_A_k.weight)
            module.lora_A_k.weight.copy_(A)          # in-place on the Parameter (not .data): bumps its version, which the
            module.lora_A_v.weight.copy_(A)          # executor watches to refresh its [A_k; A_v] copy
            module.reset_input_matrix()

    def after_task(self, task_idx, buffer, train_loader, test_loaders):
        for module in self.attention_modules:
            module.merge_weight()
        self._update_feature(task_idx, train_loader, None)
        if self._use_class_alignment:                                       # InfLoRA_opt.py:285-288
            self._create_distribution(train_loader, test_loaders[0].dataset.trfms)
            if task_idx > 0:
                self._compact_classifier(task_idx)

    # the reference's attribute names (InfLoRA_opt.py:159-160, :385-390), as views of the aligner's state
    @property
    def _class_means(self):
        return self._aligner.means if self._aligner is not None and self._aligner.means.shape[0] else None

    @property
    def _class_covs(self):
        return self._aligner.covs if self._aligner is not None and self._aligner.covs.shape[0] else None

    @torch.no_grad()
    def _create_distribution(self, train_loader, test_trfms):
        """InfLoRA_opt.py:371-397: eval forward of the task's training set under the test transforms, then mean and covariance per class.  Features are
        collected batch by batch (the reference keeps the task's images resident and forwards one class at a time)."""
        from .ranpac import _eval_view
        self._network.eval()
        feats, labels = [], []
        for batch in _eval_view(train_loader, test_trfms, self.device):
            feats.append(self._network.get_feature(batch["image"].to(self.device)).float())
            labels.append(batch["label"].to(self.device))
        self._aligner.add_task(torch.cat(feats, dim=0), torch.cat(labels, dim=0), self._known_classes, self.inc_cls_num)

    def _compact_classifier(self, task_idx):
        """InfLoRA_opt.py:399-456"""
        heads = self._network.classifier_pool[: task_idx + 1]
        for param in heads.parameters():
            param.requires_grad_(True)
        self._aligner.align(list(heads), task_idx, self.inc_cls_num)

    @torch.no_grad()
    def _update_feature(self, task_idx, train_loader, test_trfms):
        """DualGPM update of the per-layer bases (InfLoRA_opt.py:290-369), host side as in the reference"""
        for batch in train_loader:
            self._network.update_input_matrix(x=batch["image"].to(self.device))
        threshold = (self.lame - self.lamb) * task_idx / self.task_num + self.lamb
        for i, module in enumerate(self.attention_modules):
            activation = module.cur_matrix.numpy().astype(np.float64)
            if task_idx == 0:
                U, S, _ = device_svd(activation, full_matrices=False)
                ratio = (S ** 2) / (S ** 2).sum()
                r = max(np.sum(np.cumsum(ratio) < threshold), 1)
                assert r < activation.shape[0] / 2
                self.feature_list.append(U[:, :r])
                self.project_type.append("remove")
            else:
                _, S, _ = device_svd(activation, full_matrices=False)
                total = (S ** 2).sum()
                fm = self.feature_list[i] @ self.feature_list[i].T
                if self.project_type[i] == "remove":
                    U, S, _ = device_svd(activation - fm @ activation, full_matrices=False)
                    ratio = (S ** 2) / total
                    acc = (total - (S ** 2).sum()) / total
                    if acc < threshold:
                        r = np.sum(np.cumsum(ratio) + acc < threshold) + 1
                        Ui = np.hstack((self.feature_list[i], U[:, :r]))
                        self.feature_list[i] = Ui[:, : min(Ui.shape[0], Ui.shape[1])]
                else:
                    U, S, _ = device_svd(fm @ activation, full_matrices=False)
                    ratio = (S ** 2) / total
                    acc = (S ** 2).sum() / total
                    if acc >= 1 - threshold:
                        r = np.sum(acc - np.cumsum(ratio) >= 1 - threshold) + 1
                        af = self.feature_list[i] - U[:, :r] @ U[:, :r].T @ self.feature_list[i]
                        U, _, _ = device_svd(af, full_matrices=True)
                        self.feature_list[i] = U[:, : self.feature_list[i].shape[1] - r]
            module.reset_input_matrix()
        for i in range(len(self.feature_list)):
            f = self.feature_list[i]
            if self.project_type[i] == "remove" and f.shape[1] > f.shape[0] / 2:
                U, _, _ = device_svd(f, full_matrices=True)
                self.feature_list[i] = U[:, f.shape[1]:]
                self.project_type[i] = "retain"
            elif self.project_type[i] == "retain":
                assert f.shape[1] <= f.shape[0] / 2

    def get_parameters(self, config):
        return self._network.parameters()
