"""DualPrompt plugin (reference core/model/dualprompt.py:46-128) on the HIP ViT executor.

Same constructor kwargs and hooks.  The backbone (a frozen ViT) gets a `DualPromptPool` (backbone/vit.py; prompt.py:231-337) of 10 E-prompts per layer -- the
pool size is hard-coded in the reference (dualprompt.py:69) -- : per step the device runs the query forward (no prefix, no gradient) -> one selection launch
for the five prompted layers (csrc/dual.hip: the shared G-prompts of blocks 0-1, row `task_idx` of the E-prompts of blocks 2-4, and the key loss) -> the
forward whose blocks 0-4 attend over [prefix | tokens] (the prefix form of csrc/attn.hip inside csrc/vit_plan.hip, with a prefix length per layer) -> head +
masked CE (clhip_linear_fwd, clhip_ce_window) -> ONE backbone backward that also fills the prefix gradients -> the selection backward.  The trainer's default
branch drives it (observe, then loss.backward()).

The head is regrown in `before_task` as a fresh Linear of the new width with the old rows copied in (dualprompt.py:79-86), so the generator is consumed as
in the reference.  The loss is the key loss, sum over the batch and the three E-layers of 1 - cos(q, e_k[task_idx]) (prompt.py:286), plus the mean CE over
the logits [last_out_dim, out_dim) (the reference fills the columns below with -inf, :99); `dw_k` is all ones (:91, :100).  Predictions are taken over the
masked logits in `observe` and over all grown logits in `inference`, where every sample takes the E-prompt whose key is closest to its query among ALL 10 keys,
those no task has trained yet included (prompt.py:294-296).

What the reference cannot run raises at construction (backbone/vit.py, DualPromptPool): odd prompt lengths, task_num > 10, key_dim != the backbone width.
Graph capture of the step and data-parallel runs are not covered.
"""
import torch
import torch.nn as nn

from .. import ops
from .backbone.vit import ViTZoo
from .heads import HipLinear, widened

POOL_SIZE = 10      # dualprompt.py:69


class Model(nn.Module):
    """prompted backbone + head (dualprompt.py:46-61)"""

    def __init__(self, backbone, feat_dim, num_class):
        super().__init__()
        self.backbone, self.feat_dim, self.num_class = backbone, feat_dim, num_class
        self.classifier = HipLinear(feat_dim, num_class)

    def forward(self, x, train=True):
        if train:
            feat, loss = self.backbone(x, train=True)
            return self.classifier(feat), loss
        return self.classifier(self.backbone(x, train=False))


class DualPrompt(nn.Module):
    cuda_graph_safe = False     # not audited for trainer.GraphedStep

    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        if not isinstance(backbone, ViTZoo):
            raise NotImplementedError("only the ViT backbone is on the hot path (SURVEY.md section 8)")
        self.device, self.kwargs = device, kwargs
        self.backbone, self.feat_dim, self.num_class = backbone, kwargs["feat_dim"], kwargs["num_class"]
        self.classifier = nn.Linear(self.feat_dim, self.num_class)       # Finetune's head (finetune.py:10): unused by the method, drawn first as there
        self.network = Model(backbone, self.feat_dim, kwargs["init_cls_num"])
        backbone.create_prompt("dual", n_tasks=kwargs["task_num"], prompt_param=[POOL_SIZE, kwargs["e_prompt_length"], kwargs["g_prompt_length"]])
        self.task_idx, self.last_out_dim, self.out_dim = 0, 0, kwargs["init_cls_num"]

    def before_task(self, task_idx, buffer, train_loader, test_loaders):
        self.task_idx = task_idx
        self.network.backbone.task_id = task_idx
        self.out_dim = self.kwargs["init_cls_num"] + task_idx * self.kwargs["inc_cls_num"]
        self.network.classifier = widened(self.network.classifier.cpu(), self.out_dim)
        self.network.to(self.device)

    def observe(self, data):
        x, y = data["image"].to(self.device), data["label"].to(self.device)
        logits, key_loss = self.network(x, train=True)
        aux = ops.LossAux()
        lo, hi = self.last_out_dim, self.out_dim
        loss = ops.classify_loss(logits, y, lo=lo, hi=hi, pred_lo=lo, pred_hi=hi, aux=aux) + key_loss.reshape(())
        self._last_aux, self._last_key_loss = aux, key_loss.detach()
        return aux.pred, aux.acc(), loss

    def after_task(self, task_idx, buffer, train_loader, test_loaders):
        self.last_out_dim = self.out_dim

    def inference(self, data):
        x, y = data["image"].to(self.device), data["label"].to(self.device)
        with torch.no_grad():
            logits = self.network(x, train=False)
        pred, correct = ops.predict(logits, y)
        return pred, correct.item() / x.size(0)

    def get_parameters(self, config):
        return list(self.network.backbone.prompt.parameters()) + list(self.network.classifier.parameters())
