"""CODA-Prompt plugin (reference core/model/codaprompt.py:39-121) on the HIP ViT executor.

Same constructor kwargs and hooks.  The backbone (a frozen ViT) gets a `CodaPromptPool` (backbone/vit.py; prompt.py:37-223): per step the device runs the
query forward (no prefix, no gradient) -> one assembly launch for the five prompted layers (csrc/coda.hip) -> the forward whose blocks 0-4 attend over
[prefix | tokens] (the prefix form of csrc/attn.hip inside csrc/vit_plan.hip) -> head + masked CE (clhip_linear_fwd, clhip_ce_window) -> ONE backbone backward that
also fills the prefix gradients -> the assembly backward.  The trainer's default branch drives it (observe, then loss.backward()).

The head is regrown in `before_task` as a fresh Linear of the new width with the old rows copied in (codaprompt.py:72-78), so the generator is consumed as
in the reference.  The loss is CE over the logits [last_out_dim, out_dim) (the reference fills the columns below with -inf, :92); `dw_k` is all ones (:84,
:93).  Predictions are taken over the masked logits in `observe` and over all grown logits in `inference`.

`mu > 0` raises: the reference's ortho_penalty calls .cuda() (prompt.py:222-223) and its shipped config sets mu 0.0, so the penalty is never evaluated.
Graph capture of the step and data-parallel runs are not covered.
"""
import torch
import torch.nn as nn

from .. import ops
from .backbone.vit import ViTZoo
from .heads import HipLinear, widened


class Model(nn.Module):
    """prompted backbone + head (codaprompt.py:39-54)"""

    def __init__(self, backbone, feat_dim, num_class):
        super().__init__()
        self.backbone, self.feat_dim, self.num_class = backbone, feat_dim, num_class
        self.classifier = HipLinear(feat_dim, num_class)

    def forward(self, x, train=True):
        if train:
            feat, loss = self.backbone(x, train=True)
            return self.classifier(feat), loss
        return self.classifier(self.backbone(x, train=False))


class CodaPrompt(nn.Module):
    cuda_graph_safe = False     # not audited for trainer.GraphedStep

    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        if not isinstance(backbone, ViTZoo):
            raise NotImplementedError("only the ViT backbone is on the hot path (SURVEY.md section 8)")
        if kwargs["mu"] > 0:
            raise NotImplementedError("mu > 0: the orthogonality penalty is not built (the reference's ortho_penalty calls .cuda(), prompt.py:222-223, and "
                                      "config/codaprompt.yaml sets mu: 0.0)")
        self.device, self.kwargs = device, kwargs
        self.backbone, self.feat_dim, self.num_class = backbone, kwargs["feat_dim"], kwargs["num_class"]
        self.classifier = nn.Linear(self.feat_dim, self.num_class)       # Finetune's head (finetune.py:10): unused by the method, drawn first as there
        self.network = Model(backbone, self.feat_dim, kwargs["init_cls_num"])
        backbone.create_prompt("coda", n_tasks=kwargs["task_num"], prompt_param=[kwargs["pool_size"], kwargs["prompt_length"], kwargs["mu"]])
        self.task_idx, self.last_out_dim, self.out_dim = 0, 0, kwargs["init_cls_num"]

    def before_task(self, task_idx, buffer, train_loader, test_loaders):
        self.task_idx = task_idx
        self.network.backbone.task_id = task_idx
        # The reference never calls prompt.process_task_count() (no file under core/ does), so task_count stays 0: components [0, pool / task_num) are
        # used and trained in every task.  Restated as it is; `self.network.backbone.prompt.process_task_count()` here (for task_idx > 0) would move the
        # window -- the kernels take (s, f) as arguments.
        self.out_dim = self.kwargs["init_cls_num"] + task_idx * self.kwargs["inc_cls_num"]
        self.network.classifier = widened(self.network.classifier.cpu(), self.out_dim)
        self.network.to(self.device)

    def observe(self, data):
        x, y = data["image"].to(self.device), data["label"].to(self.device)
        logits, _ = self.network(x, train=True)                          # (the prompt loss is identically 0 at mu = 0)
        aux = ops.LossAux()
        lo, hi = self.last_out_dim, self.out_dim
        loss = ops.classify_loss(logits, y, lo=lo, hi=hi, pred_lo=lo, pred_hi=hi, aux=aux)
        self._last_aux = aux
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
