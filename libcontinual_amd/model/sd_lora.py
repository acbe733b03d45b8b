"""SD-LoRA plugin (reference core/model/sd_lora.py:24-210) on the HIP ViT executor.

Same constructor kwargs and hooks.  The backbone's attention layers are `MultiHeadAttention_SDLoRA` (backbone/vit.py): per task one low-rank term on q
and v; the terms of finished tasks stay as unit-Frobenius-norm directions, and one trainable scalar per task -- the same parameters in all blocks --
scales each of them.  Within a task A and B of the current term, every magnitude and the head train (sd_lora.py:129-136).  One growing linear head
(old rows copied, sd_lora.py:35-54); the loss is CE over the logits of the current task's classes with shifted labels, predictions are taken
over all logits (sd_lora.py:86-91).

Hot loop = HIP: per step one refresh of the q / v rows of the effective qkv copies (clhip_sdlora_refresh), the backbone forward, head + CE
(clhip_linear_fwd, clhip_ce_window), and one backbone backward that runs clhip_sdlora_grad per layer (csrc/sdlora.hip).  The norms of the past
terms are constant within a task: `before_task` computes their reciprocals once, on the device.

`knowledge_dist[0] = True` (SD-LoRA-KD, sd_lora.py:145-207) raises: the reference's merge loop cannot run as written (see the message below).
Graph capture of the step and data-parallel runs are not covered.
"""
import copy

import torch
import torch.nn as nn

from .. import ops
from .backbone.vit import MultiHeadAttention_SDLoRA, ViTZoo
from .heads import HipLinear


class Model(nn.Module):
    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        if not isinstance(backbone, ViTZoo):
            raise NotImplementedError("only the ViT backbone is on the hot path (SURVEY.md section 8)")
        self._cur_task_id = -1
        self.backbone = backbone
        self.device = device
        self.embed_dim = kwargs["embd_dim"]
        self.init_cls_num = kwargs["init_cls_num"]
        self.inc_cls_num = kwargs["inc_cls_num"]

    def update_fc(self):
        self._cur_task_id += 1
        classifier = HipLinear(self.embed_dim, self.init_cls_num + self.inc_cls_num * self._cur_task_id, bias=True)
        nn.init.kaiming_uniform_(classifier.weight, nonlinearity="linear")
        nn.init.constant_(classifier.bias, 0)
        if self._cur_task_id > 0:
            nb_output = self.classifier.out_features
            classifier.weight.data[:nb_output] = copy.deepcopy(self.classifier.weight.data)
            classifier.bias.data[:nb_output] = copy.deepcopy(self.classifier.bias.data)
            del self.classifier
        self.classifier = classifier

    def forward(self, x, inference=False):
        return self.classifier(self.backbone(x))


class SD_LoRA(nn.Module):
    cuda_graph_safe = False     # not audited for trainer.GraphedStep

    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        self.device = device
        self.init_cls_num = kwargs["init_cls_num"]
        self.inc_cls_num = kwargs["inc_cls_num"]
        self.task_num = kwargs["task_num"]
        self.init_mag = kwargs["init_mag"]
        self.rank_reduction = kwargs["rank_reduction"]
        self.knowledge_dist = kwargs["knowledge_dist"]
        self._known_classes = 0
        if self.knowledge_dist[0]:
            raise NotImplementedError(
                "knowledge_dist[0] = True: the reference's merge cannot run as written.  Its loop `for ii in range(prev_dirs.shape[1])` adds "
                "`alphas.solution[i]` with the stale `i == task_idx` left over from the loop above it, one past the end of the task_idx solutions "
                "(sd_lora.py:187, :204), and the zero-norm fallback of the v directions appends a q product (sd_lora.py:172)")
        self._network = Model(backbone, device, **kwargs)
        self.attention_modules = [module for module in self._network.modules() if isinstance(module, MultiHeadAttention_SDLoRA)]
        if not self.attention_modules:
            raise ValueError("SD_LoRA needs a backbone built with attn_layer: MultiHeadAttention_SDLoRA")

    def observe(self, data):
        x, y = data["image"].to(self.device), data["label"].to(self.device)
        logits = self._network(x)
        aux = ops.LossAux()
        loss = ops.classify_loss(logits, y, lo=self._known_classes, aux=aux)       # CE on logits[:, known:] with y - known; argmax over all logits
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
        self._network.update_fc()
        if self.rank_reduction[0]:
            if task_idx == self.rank_reduction[1]:
                for module in self.attention_modules:
                    module.lora_rank = self.rank_reduction[3]
            elif task_idx == self.rank_reduction[2]:
                for module in self.attention_modules:
                    module.lora_rank = self.rank_reduction[4]
        self._network = self._network.to(self.device)
        # all blocks share the same magnitudes, re-created at init_mag for every task (sd_lora.py:122)
        mag = nn.ParameterList([nn.Parameter(torch.full((1,), float(self.init_mag), device=self.device)) for _ in range(task_idx + 1)])
        for module in self.attention_modules:
            module.mag_lora = mag
            module.init_param()
        self._network.backbone.feat.sdlora_update_inv()
        for name, param in self._network.named_parameters():
            param.requires_grad_(False)
            if "classifier" in name or f"list.{task_idx}" in name or ("mag" in name and "assimilated" not in name):     # sd_lora.py:132-134
                param.requires_grad_(True)

    @torch.no_grad()
    def after_task(self, task_idx, buffer, train_loader, test_loaders):
        self._known_classes += self.init_cls_num if task_idx == 0 else self.inc_cls_num

    def get_parameters(self, config):
        return self._network.parameters()
