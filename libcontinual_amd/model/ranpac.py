"""RanPAC plugin (reference core/model/ranpac.py:30-269) on the HIP ViT executor and the fp32 MFMA kernels of csrc/rp.hip.

A frozen pre-trained ViT, a fixed random projection `W_rand` [feat_dim, M] with a ReLU, and a ridge-regression head that is solved, not trained:
after every task the projected features of the task's training set update two running sums, G = H^T H [M, M] and Q = H^T Y [M, classes], the ridge
parameter is picked out of 10^-8 .. 10^8 on a 20 % hold-out of the task, and Wo = solve(G + ridge I, Q)^T becomes the head (ranpac.py:214-266).
Without first-session training there is no per-step backward: `observe` returns a zero loss that requires grad, so the trainer's backward / step are
no-ops (ranpac.py:184-186).

Kept from the reference: constructor kwargs, hook order, the fresh cosine head at every `before_task` (so a validation between `before_task` and
`after_task` scores with a random cosine head), `W_rand` drawn on the CPU from the global generator (a seed reproduces the reference's matrix), Q growing
by `inc_cls_num` columns per task, the loader's dataset switched to the test transforms for the feature pass, `int(0.8 N)` rows in loader order as
the fitting part of the ridge search, numpy's first-minimum rule, `weight.data = Wo[:classes]`.
Different by design: features, H, G, Q and the solves live on the device in fp32 (the reference moves everything to the CPU after the forward);
G and Q are formed as G_val + G_rest / Q_val + Q_rest instead of a third pass over all rows.
First-session training (`first_session_training: true`, the reference's shipped setting; ranpac.py:176-199): task 0 is trained with SGD on the
cross-entropy of the cosine head's logits, and what moves are the head and the AdaptFormer adapters of the backbone (`ffn_adapt: true` on
`vit_pt_imnet_in21k_adapter`; forward, input gradient and parameter gradients in csrc/adapter.hip inside the ViT executor, dropout in training mode).
From `after_task(0)` on the backbone runs in eval mode and every later task only solves the ridge head, on features the trained adapters take part
in.  The reference's adapters start as the identity (`up_proj` is zero-initialised), so without that session -- or on a backbone built without
`ffn_adapt`, where the switch raises -- the network is exactly the plain ViT-B/16.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

RIDGES = 10.0 ** np.arange(-8, 9)          # ranpac.py:253
_H_BYTES = 256 << 20                       # H is built in row chunks of at most this size


def _solve(A, Qm):
    """torch.linalg.solve on the device in fp32 -- the reference's factorisation (ranpac.py:259, :265), there on the CPU.  Where the device solver is
    unavailable (or CLHIP_SOLVE=host) the system is solved on the host in fp64, as CLHIP_SVD=host does for the SVDs (utils.device_svd)."""
    if os.environ.get("CLHIP_SOLVE", "device") != "host":
        try:
            return torch.linalg.solve(A, Qm)
        except RuntimeError as e:
            if "singular" in str(e):
                raise
    return torch.from_numpy(np.linalg.solve(A.double().cpu().numpy(), Qm.double().cpu().numpy())).to(A)


class RPClassifier:
    """The classifier without a backbone: `update(features, labels, n_classes)` is ranpac.py:246-266 for one task on given features [N, feat_dim]
    (rows in loader order), `logits(features)` the use_RP branch of ranpac.py:53-61.  State: W_rand, G, Q (fp32, on `device`), Wo, ridge."""

    def __init__(self, feat_dim, M, device, w_rand=None):
        self.feat_dim, self.M, self.device = int(feat_dim), int(M), torch.device(device)
        if w_rand is None:
            w_rand = torch.randn(self.feat_dim, self.M)              # ranpac.py:221: on the CPU, from the global generator
        assert tuple(w_rand.shape) == (self.feat_dim, self.M)
        self.W_rand = w_rand.to(self.device, torch.float32).contiguous()
        self.G = torch.zeros(self.M, self.M, device=self.device)
        self.Q = torch.zeros(self.M, 0, device=self.device)
        self.Wo, self.ridge, self.losses = None, None, None

    def _rows(self):
        return max(1, _H_BYTES // (4 * self.M))

    def _accumulate(self, feats, labels, G, Qm):
        for s in range(0, feats.shape[0], self._rows()):
            H = ops.rp_project(feats[s:s + self._rows()], self.W_rand, relu=True)
            ops.rp_gram_accum(H, G)
            ops.rp_label_sum(H, labels[s:s + self._rows()], Qm)

    def _predict(self, feats, Wo):
        return torch.cat([ops.rp_classify(feats[s:s + self._rows()], self.W_rand, Wo) for s in range(0, feats.shape[0], self._rows())])

    @torch.no_grad()
    def update(self, features, labels, n_classes):
        feats = features.detach().to(self.device, torch.float32).contiguous()
        labels = labels.detach().to(self.device, torch.int64).contiguous()
        N, C = feats.shape[0], int(n_classes)
        if self.Q.shape[1] < C:                                       # ranpac.py:222, :226
            self.Q = torch.cat((self.Q, torch.zeros(self.M, C - self.Q.shape[1], device=self.device)), dim=1).contiguous()
        nv = int(N * 0.8)                                             # ranpac.py:254
        G_val, Q_val = torch.zeros_like(self.G), torch.zeros_like(self.Q)
        G_rest, Q_rest = torch.zeros_like(self.G), torch.zeros_like(self.Q)
        if nv:
            self._accumulate(feats[:nv], labels[:nv], G_val, Q_val)
        self._accumulate(feats[nv:], labels[nv:], G_rest, Q_rest)
        Y_rest = F.one_hot(labels[nv:], C).double()
        losses = []
        for ridge in RIDGES:                                          # ranpac.py:258-261
            A = G_val.clone()
            A.diagonal().add_(float(ridge))
            Wo = _solve(A, Q_val).T.contiguous()
            losses.append((self._predict(feats[nv:], Wo).double() - Y_rest).pow(2).mean())
        del A
        self.losses = torch.stack(losses).cpu().numpy()
        self.ridge = float(RIDGES[np.argmin(self.losses)])            # first minimum (ranpac.py:262)
        self.G += G_val
        self.G += G_rest
        self.Q += Q_val
        self.Q += Q_rest
        del G_val, G_rest
        A = self.G.clone()
        A.diagonal().add_(self.ridge)
        self.Wo = _solve(A, self.Q).T.contiguous()                    # ranpac.py:265: [classes, M]
        return self.Wo

    @torch.no_grad()
    def logits(self, features, sigma=None):
        feats = features.detach().to(self.device, torch.float32).contiguous()
        return ops.rp_classify(feats, self.W_rand, self.Wo, sigma)


class CosineLinear(nn.Module):
    """ranpac.py:30-63: a cosine head until `use_RP` is set, then sigma * relu(x W_rand) weight^T with weight = Wo"""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.sigma = nn.Parameter(torch.empty(1))
        self.reset_parameters()
        self.use_RP = False
        self.W_rand = None

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.weight.size(1))
        self.weight.data.uniform_(-stdv, stdv)
        self.sigma.data.fill_(1)

    def forward(self, x):
        if not self.use_RP:
            return ops.sigma_scale(ops.cosine_linear(x, self.weight), self.sigma)
        if self.W_rand is None:
            raise RuntimeError("use_RP is set without W_rand (ranpac.py:57)")
        return ops.rp_classify(x, self.W_rand, self.weight, self.sigma)


class Network(nn.Module):
    """ranpac.py:65-138, the ViT branch"""

    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        self._cur_task_id = -1
        self.backbone = backbone
        self.device = device
        self.classifier = None
        self.feature_dim = backbone.feat_dim

    def update_classifer(self, num_classes, train_loader=None):
        self._cur_task_id += 1
        self.classifier = CosineLinear(self.feature_dim, num_classes).to(self.device)       # fresh at every task (ranpac.py:105-106)

    def get_feature(self, x):
        return self.backbone(x)

    def forward(self, x, inference=False):
        return self.classifier(self.backbone(x))


def _eval_view(train_loader, test_trfms, device):
    """ranpac.py:234: the task's training images under the TEST transforms, in the train loader's order.  A torch DataLoader reads
    `dataset.trfms` per sample; the GPU batch loader compiled its plan from the transforms it was built with, so it gets the plan of the new ones
    (or, where the augment kernels have none for them, a host loader takes over)."""
    from ..data.dataset import make_loader
    from ..data.gpu_loader import GpuBatchLoader
    train_loader.dataset.trfms = test_trfms
    if isinstance(train_loader, GpuBatchLoader):
        return make_loader(train_loader.dataset, train_loader.batch_size, train_loader.shuffle, train_loader.num_workers, device, train_loader.drop_last)
    return train_loader


class RanPAC(nn.Module):
    cuda_graph_safe = False        # later tasks: the step is a no-op; the first session: the host draws a dropout seed and re-arms the executor per forward
    reduces_own_gradients = True   # parallel.attach then hands a data-parallel reducer to the plugin, whose setter below refuses it
    _grad_reducer = None

    def __init__(self, backbone, device, **kwargs):
        super().__init__()
        fst = bool(kwargs.get("first_session_training", False))
        adapters = getattr(getattr(backbone, "feat", None), "adapter_tensors", lambda: [])()
        if fst and not adapters:
            raise NotImplementedError("RanPAC: `first_session_training: true` trains the AdaptFormer adapters of the backbone, and this backbone has none; "
                                      "build it with the backbone kwarg `ffn_adapt: true`, or set first_session_training: false")
        self._network = Network(backbone, device, **kwargs)
        self.device = device
        self.first_session_training = fst
        self.init_cls_num, self.inc_cls_num = kwargs["init_cls_num"], kwargs["inc_cls_num"]
        self.total_cls_num, self.task_num = kwargs["total_cls_num"], kwargs["task_num"]
        self.M = kwargs["M"]
        self._known_classes = 0
        self._classes_seen_so_far = 0
        self._skip_train = False
        self.rp = None
        for p in self._network.backbone.parameters():      # the frozen pre-trained network: nothing of it ever reaches the optimizer ...
            p.requires_grad_(False)
        if fst:
            for p in adapters:                              # ... but the adapters, in the first session (vision_transformer_adapter.py:461-466)
                p.requires_grad_(True)
        self._network.to(self.device)

    # a data-parallel run would leave every rank with the G / Q of its own shard of the task
    @property
    def grad_reducer(self):
        return self._grad_reducer

    @grad_reducer.setter
    def grad_reducer(self, reducer):
        if reducer is not None:
            raise NotImplementedError("RanPAC keeps G and Q per process: data parallelism (n_gpu > 1) is not supported")
        self._grad_reducer = None

    @property
    def backbone(self):
        return self._network.backbone

    def before_task(self, task_idx, buffer, train_loader, test_loaders):
        if task_idx == 0:
            self._classes_seen_so_far = self.init_cls_num
        else:
            self._classes_seen_so_far += self.inc_cls_num
        self._network.update_classifer(self._classes_seen_so_far, train_loader)
        self._skip_train = not (task_idx == 0 and self.first_session_training)              # ranpac.py:176-180
        if self.first_session_training:
            for p in self._network.backbone.feat.adapter_tensors():                         # after the first session the whole backbone is frozen
                p.requires_grad_(task_idx == 0)

    def observe(self, data):
        if self._skip_train:
            return None, 0., torch.tensor(0., device=self.device, requires_grad=True)        # ranpac.py:184-186
        x, y = data["image"].to(self.device), data["label"].to(self.device) - self._known_classes                     # ranpac.py:188-199
        logits = self._network(x)
        aux = ops.LossAux()                                 # cross-entropy, its gradient, the predictions and the correct count: one launch
        loss = ops.classify_loss(logits, y, aux=aux)
        return aux.pred, aux.acc(), loss

    def inference(self, data):
        x, y = data["image"].to(self.device), data["label"].to(self.device)
        with torch.no_grad():
            logits = self._network(x, True)
        pred, correct = ops.predict(logits, y)
        return pred, correct.item() / y.size(0)

    def after_task(self, task_idx, buffer, train_loader, test_loaders):
        self._known_classes = self._classes_seen_so_far
        if task_idx == 0:
            self.rp = RPClassifier(self._network.classifier.in_features, self.M, self.device)
        self.update_rp_classifier(train_loader, test_loaders[0].dataset.trfms)

    @torch.no_grad()
    def collect_features(self, train_loader, test_trfms):
        """ranpac.py:233-244: eval forward of the task's training set under the test transforms; features stay on the device"""
        self._network.eval()
        feats, labels = [], []
        for batch in _eval_view(train_loader, test_trfms, self.device):
            feats.append(self._network.get_feature(batch["image"].to(self.device)).float())
            labels.append(batch["label"].to(self.device))
        return torch.cat(feats, dim=0), torch.cat(labels, dim=0)

    @torch.no_grad()
    def update_rp_classifier(self, train_loader, test_trfms):
        feats, labels = self.collect_features(train_loader, test_trfms)
        self.last_features = (feats, labels)                # (kept for diagnostics and tests: [N, feat_dim] and [N])
        head = self._network.classifier
        head.use_RP = True
        head.W_rand = self.rp.W_rand
        Wo = self.rp.update(feats, labels, self._classes_seen_so_far)
        print(f"Optimal lambda: {self.rp.ridge}")
        head.weight.data = Wo[:head.weight.shape[0], :].contiguous()

    @property
    def W_rand(self):
        return self.rp.W_rand

    @property
    def G(self):
        return self.rp.G

    @property
    def Q(self):
        return self.rp.Q

    def get_parameters(self, config):
        return list(self._network.parameters())             # ranpac.py:268-269; the backbone's are frozen and never get a gradient
