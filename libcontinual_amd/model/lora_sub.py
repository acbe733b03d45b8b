"""LoRA-Sub-DRS plugin (reference core/model/lora_sub.py:27-432) on the HIP ViT executor.

Same constructor kwargs, hooks and `get_optimizer(lr, weight_decay)`.  The backbone's attention layers are `MultiHeadAttention_LoRA_Sub` (backbone/vit.py):
one rank-r LoRA term on k and v per task, A and B both trained, finished terms summed into the buffers `prev_{k,v}_weight`.  One linear head per task; the
loss is CE over the current head with shifted labels plus `lambada` times the augmented triplet loss of the normalised features against the batch and
the prototypes of all finished classes (lora_sub.py:293-311).  From task 1 on every LoRA update is multiplied by a per-layer transform
T = V_k V_k^T / |V_k V_k^T|_F, V_k the leading singular vectors of the Gram mean of the attention input under the weights W - prev that reach 0.99 of the
spectrum (lora_sub.py:159-191).  Inference is nearest normalised prototype (lora_sub.py:313-331).

Hot loop = HIP: per step one refresh of the k / v rows (clhip_vit_lora_refresh_ab), the backbone forward, head + CE (clhip_linear_fwd, clhip_ce_window),
the triplet loss and its feature gradient in two launches (clhip_atl), one backbone backward that runs clhip_lora_grad_ab per layer, and the optimizer's
step: clhip_proj_adam_multi for the 4 * depth factors, clhip_adam_step for the head (csrc/lorasub.hip).

`before_task`: the Gram pass runs through the executor's resident Gram buffer; the reference keeps four copies of a layer's Gram (one per factor) and
decomposes each -- the four are the same matrix, so this does `depth` fp64 SVDs (utils.device_svd: on the GPU, CLHIP_SVD=host on the host) and keeps one
T per layer on the device.  `after_task`: the reference makes one full pass over the train loader PER CLASS, each with fresh random crops, and averages
the class's features; here ONE pass feeds per-class sums on the device -- the same estimator (a mean over one augmented view per image) at a tenth of
the cost, not the same random draws.  Graph capture of the step and data-parallel runs are not covered.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..utils import device_svd
from .backbone.vit import MultiHeadAttention_LoRA_Sub, ViTZoo
from .heads import HipLinear


class _AtlFn(torch.autograd.Function):
    """weight * AugmentedTripletLoss(f / |f|, y, protos) as one scalar; the kernel hands back the feature gradient with the weight already in it"""

    @staticmethod
    def forward(ctx, feats, labels, protos, margin, weight):
        loss, df = ops.atl(feats.detach(), labels, protos, margin, weight)
        ctx.save_for_backward(df)
        ctx.mark_non_differentiable(loss)
        return loss * weight, loss

    @staticmethod
    def backward(ctx, dl, _):
        (df,) = ctx.saved_tensors
        return df * dl, None, None, None, None


class Model(nn.Module):
    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        if not isinstance(backbone, ViTZoo):
            raise NotImplementedError("only the ViT backbone is on the hot path (SURVEY.md section 8)")
        self._cur_task_id = -1
        self.backbone = backbone
        self.device = device
        self.classifier_pool = nn.ModuleList([HipLinear(kwargs["embd_dim"], kwargs["init_cls_num"], bias=True)] +
                                             [HipLinear(kwargs["embd_dim"], kwargs["inc_cls_num"], bias=True) for _ in range(kwargs["task_num"] - 1)])

    def update_fc(self):
        self._cur_task_id += 1

    def update_input_matrix(self, x):
        self.backbone(x, get_input_matrix=True)

    def extract_features(self, x):
        return self.backbone(x)

    def forward(self, x):
        features = self.backbone(x)
        return {"logits": self.classifier_pool[self._cur_task_id](features), "features": features}


class ProjectedAdam:
    """the reference's Adam (lora_sub.py:70-233) with the `torch.optim.Optimizer` surface the trainer and the schedulers use: `param_groups` = the LoRA
    factors (svd: True) and the current head, each with its learning rate.  step(): one clhip_proj_adam_multi call for all factors (their Adam update
    multiplied by the layer's transform; plain Adam while there is none), clhip_adam_step for the head tensors.
    The reference's update is lr sqrt(bc2) / bc1 * m / (sqrt(v) + eps) (lora_sub.py:224-232); the kernels evaluate clhip_adam_step's lr / bc1 * m / (sqrt(v) /
    sqrt(bc2) + eps'), which is the same expression at eps' = eps / sqrt(bc2): that is the eps every step hands them.  The difference is not academic: the
    k-side gradients of a LoRA factor reach 1e-7, where eps decides the size of the first steps."""
    capture_safe = False

    def __init__(self, factors, head, transforms, dim, rank, lr, fc_lrate, weight_decay, betas=(0.9, 0.999), eps=1e-8):
        assert len(factors) % 4 == 0
        self.param_groups = [dict(params=list(factors), svd=True, thres=0.99, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps),
                             dict(params=list(head), svd=False, lr=fc_lrate, weight_decay=weight_decay, betas=betas, eps=eps)]
        self.transforms, self.dim, self.rank = transforms, dim, rank               # transforms: [layers, D, D] fp32 on the device, or None
        self.state = {}
        self._step = 0
        self._table = self._table_key = self._tt = self._ws = None

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    def state_dict(self):
        return {"step": self._step, "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    @torch.no_grad()
    def step(self, closure=None):
        self._step += 1
        fg, hg = self.param_groups
        fac = fg["params"]
        eps_of = lambda g: g["eps"] / math.sqrt(1.0 - g["betas"][1] ** self._step)
        for p in fac:
            if p.grad is None:
                raise RuntimeError("ProjectedAdam.step: a LoRA factor has no gradient (all of them come out of one backward)")
            if p not in self.state:
                self.state[p] = (torch.zeros_like(p), torch.zeros_like(p))
        rows = [(p, p.grad.contiguous(), *self.state[p]) for p in fac]
        key = tuple(t.data_ptr() for row in rows for t in row)
        if key != self._table_key:                                                  # (the gradients live in one buffer the backbone reuses: built once)
            self._table, self._table_key = ops.proj_adam_table(rows), key
        if self.transforms is not None and self._tt is None:
            self._tt = torch.tensor([t.data_ptr() for t in self.transforms], dtype=torch.int64).to(self.transforms.device)
            self._ws = torch.empty(len(fac) * self.dim * self.rank, device=self.transforms.device)
        ops.proj_adam_multi(self._table, self._tt, self._ws, self.dim, self.rank, fg["lr"], fg["betas"][0], fg["betas"][1], eps_of(fg), fg["weight_decay"],
                            self._step)
        for p in hg["params"]:
            if p.grad is None:
                continue
            if p not in self.state:
                self.state[p] = (torch.zeros_like(p), torch.zeros_like(p))
            m, v = self.state[p]
            ops.adam_step(p, p.grad.contiguous(), m, v, hg["lr"], hg["betas"][0], hg["betas"][1], eps_of(hg), hg["weight_decay"], 1.0, self._step)
        return None


class LoRAsub_DRS(nn.Module):
    cuda_graph_safe = False     # not audited for trainer.GraphedStep

    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        self.device = device
        self.init_cls_num = kwargs["init_cls_num"]
        self.inc_cls_num = kwargs["inc_cls_num"]
        self.task_num = kwargs["task_num"]
        self.fc_lrate = kwargs["fc_lrate"]
        self.margin_inter = kwargs["margin_inter"]
        self.lambada = kwargs["lambada"]
        self._known_classes = 0
        self._total_classes = 0
        self._cur_task = 0
        self._network = Model(backbone, device, **kwargs)
        self.attention_modules = [module for module in self._network.modules() if isinstance(module, MultiHeadAttention_LoRA_Sub)]
        if not self.attention_modules:
            raise ValueError("LoRAsub_DRS needs a backbone built with attn_layer: MultiHeadAttention_LoRA_Sub")
        self._protos = None               # [classes so far, D] fp32 on the device, un-normalised
        self.transforms = None            # [depth, D, D] fp32 on the device, from task 1 on
        self.reserved_basis = []          # k per layer of the running task
        self.last_atl = None

    def observe(self, data):
        x, y = data["image"].to(self.device), data["label"].to(self.device) - self._known_classes
        out = self._network(x)
        aux = ops.LossAux()
        ce = ops.classify_loss(out["logits"], y, aux=aux)
        term, self.last_atl = _AtlFn.apply(out["features"], y, self._protos, float(self.margin_inter), float(self.lambada))
        self._last_aux = aux
        return aux.pred, aux.acc(), ce + term.reshape(ce.shape)

    def inference(self, data):
        x, y = data["image"].to(self.device), data["label"].to(self.device)
        if self._protos is None:
            raise RuntimeError("LoRAsub_DRS.inference before the first after_task: there are no prototypes yet")
        with torch.no_grad():
            f = self._network.extract_features(x).float()
            f = f / (f.norm(dim=1, keepdim=True) + 1e-8)                           # lora_sub.py:318 (the + 1e-8, then the kernels)
            pred = ops.ncm_classify(f, ops.l2_normalize_rows(self._protos))
        return pred, (pred == y).sum().item() / y.size(0)

    @torch.no_grad()
    def before_task(self, task_idx, buffer, train_loader, test_loaders):
        self._known_classes = self._total_classes
        self._total_classes += self.init_cls_num if task_idx == 0 else self.inc_cls_num
        self._network.update_fc()
        self._network = self._network.to(self.device)
        for module in self.attention_modules:
            module.init_param()
        for name, param in self._network.named_parameters():
            param.requires_grad_(f"classifier_pool.{self._cur_task}." in name or "lora" in name)
        self.transforms, self.reserved_basis = None, []
        if task_idx == 0:
            return
        # the Gram pass on W - prev, without the LoRA term (transformer.py:407-413), into the executor's resident buffer
        for module in self.attention_modules:
            module.apply_lora, module.subtract = False, True
        for batch in train_loader:
            self._network.update_input_matrix(batch["image"].to(self.device))
        T = []
        for i, module in enumerate(self.attention_modules):
            module.apply_lora, module.subtract = True, False
            G = module.cur_matrix.double()
            _, S, Vh = device_svd(G, full_matrices=True)                           # fp64; one per layer: the four factors share G
            ratio = np.cumsum(S) / S.sum()
            k = int(np.nonzero(ratio >= 0.99)[0][0]) + 1
            V = torch.from_numpy(np.ascontiguousarray(Vh[:k].T))
            t = V @ V.T
            T.append((t / torch.linalg.norm(t)).float())
            self.reserved_basis.append(k)
            print(f"layer {i}: reserving basis {k}/{len(S)}; cond: {S[0] / S[-1]}, ratio:{ratio[k - 1]}")
            module.reset_input_matrix()
        self.transforms = torch.stack(T).to(self.device)

    @torch.no_grad()
    def after_task(self, task_idx, buffer, train_loader, test_loaders):
        for module in self.attention_modules:
            module.save_weight()
        n_new = self._total_classes - self._known_classes
        D = self._network.backbone.feat.embed_dim
        sums = torch.zeros(n_new, D, device=self.device)
        counts = torch.zeros(n_new, device=self.device)
        for batch in train_loader:                                                  # one pass, the loader's train transforms (see the module docstring)
            x, y = batch["image"].to(self.device), batch["label"].to(self.device) - self._known_classes
            f = self._network.extract_features(x).float()
            keep = (y >= 0) & (y < n_new)
            hot = torch.nn.functional.one_hot(y[keep], n_new).float()                # (a product, not index_add_: no atomics, two runs agree bit for bit)
            sums += hot.T @ f[keep]
            counts += hot.sum(0)
        assert bool((counts > 0).all()), "a class of the task has no training image"
        means = sums / counts[:, None]
        self._protos = means if self._protos is None else torch.cat([self._protos, means])
        self._known_classes += self.init_cls_num if task_idx == 0 else self.inc_cls_num
        self._cur_task += 1

    def get_parameters(self, config):
        return self._network.parameters()

    def get_optimizer(self, lr, weight_decay):
        fac = [w for m in self.attention_modules for w in (m.lora_A_k.weight, m.lora_B_k.weight, m.lora_A_v.weight, m.lora_B_v.weight)]
        head = self._network.classifier_pool[self._cur_task]
        return ProjectedAdam(fac, [head.weight, head.bias], self.transforms if self._cur_task > 0 else None, fac[0].shape[1], fac[0].shape[0], lr,
                             self.fc_lrate, weight_decay)
