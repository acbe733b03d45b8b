"""Write tests/golden/ca_tiny.npz by running the REFERENCE's own classifier alignment (core/model/InfLoRA_opt.py:371-456) on the CPU, imported through
oracle.ref_shim.

Build-container only (needs the reference tree).  The reference's `InfLoRA_OPT` gets a stand-in network whose `get_feature` returns the given
768-wide rows and whose `classifier_pool` / `fc_only` are real `nn.Linear` heads, so its own `_create_distribution` and `_compact_classifier` run
unchanged, in its own fp32, for two tasks of two classes on the seeded inputs of tests/ca_ref.py.  Two names are replaced during the run by functions
that return ca_ref's seeded arrays -- `torch.distributions.multivariate_normal._standard_normal` (the normals of every `MultivariateNormal.sample`)
and `torch.randperm` (the shuffle of every epoch) -- so nothing large needs storing and the fp64 restatement sees the same draws.

    python tools/gen_ca_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import ca_ref as CA  # noqa: E402


class _Set:
    def __init__(self, feats, labels):
        self.feats, self.labels, self.trfms = torch.from_numpy(feats), torch.from_numpy(labels), "train"


class _Loader:
    """the slice of the DataLoader interface the plugin touches: `.dataset.trfms` and iteration over {"image", "label"} batches, in row order"""

    def __init__(self, feats, labels, batch=16):
        self.dataset, self.batch = _Set(feats, labels), batch

    def __iter__(self):
        for s in range(0, len(self.dataset.labels), self.batch):
            yield {"image": self.dataset.feats[s:s + self.batch], "label": self.dataset.labels[s:s + self.batch]}


class _Net(nn.Module):
    """what `_create_distribution` / `_compact_classifier` ask of SiNet: features, the heads and the logits over the heads so far"""

    def __init__(self):
        super().__init__()
        self._cur_task_id = -1
        self.classifier_pool = nn.ModuleList([nn.Linear(CA.D, CA.CLS, bias=True) for _ in range(CA.TASKS)])
        with torch.no_grad():
            for fc, (w, b) in zip(self.classifier_pool, CA.init_heads()):
                fc.weight.copy_(torch.from_numpy(w))
                fc.bias.copy_(torch.from_numpy(b))

    def get_feature(self, x):
        return x

    def fc_only(self, x):
        return torch.cat([fc(x) for fc in self.classifier_pool[: self._cur_task_id + 1]], dim=1)

    def flat(self):
        return (torch.cat([fc.weight.detach() for fc in self.classifier_pool]).numpy().copy(),
                torch.cat([fc.bias.detach() for fc in self.classifier_pool]).numpy().copy())


def main():
    if torch.get_default_dtype() != torch.float32:
        raise RuntimeError("the reference aligns in fp32 (InfLoRA_opt.py:425, :431): do not change the default dtype")
    os.environ.setdefault("PYTHONHASHSEED", "0")
    ref_shim.install_vit_standins()
    ref = ref_shim.load("core.model.InfLoRA_opt")
    mvn = torch.distributions.multivariate_normal

    model = ref.InfLoRA_OPT.__new__(ref.InfLoRA_OPT)       # its __init__ wants a ViTZoo; the two functions under test read the attributes below
    nn.Module.__init__(model)
    model.device, model.init_cls_num, model.inc_cls_num = "cpu", CA.CLS, CA.CLS
    model._known_classes, model._class_means, model._class_covs, model._logit_norm = 0, None, None, None
    model._network = _Net()
    W0, b0 = model._network.flat()

    for t in range(CA.TASKS):
        model._known_classes = t * CA.CLS
        model._network._cur_task_id = t
        f, l = CA.task_rows(t, "train")
        counts = np.bincount(l - t * CA.CLS, minlength=CA.CLS)
        assert counts.min() >= 2, counts
        loader = _Loader(f, l)
        model._create_distribution(loader, "test")
        assert loader.dataset.trfms == "test"                # InfLoRA_opt.py:375
        if t > 0:
            C, calls, epochs = (t + 1) * CA.CLS, [0], [0]

            def seeded_normal(shape, dtype, device):
                ep, cls = divmod(calls[0], C)
                calls[0] += 1
                assert tuple(shape) == (CA.NUM_SAMPLE, CA.D) and dtype == torch.float32
                return torch.from_numpy(CA.normals(ep, cls))

            def seeded_perm(n):
                epochs[0] += 1
                return torch.from_numpy(CA.permutation(epochs[0] - 1, n))

            real_normal, real_perm = mvn._standard_normal, torch.randperm
            mvn._standard_normal, torch.randperm = seeded_normal, seeded_perm
            try:
                model._compact_classifier(t)
            finally:
                mvn._standard_normal, torch.randperm = real_normal, real_perm
            assert calls[0] == CA.EPOCHS * C and epochs[0] == CA.EPOCHS
    W, b = model._network.flat()
    means, covs = model._class_means.numpy(), model._class_covs.numpy()
    assert means.dtype == covs.dtype == W.dtype == np.float32 and means.shape == (CA.TASKS * CA.CLS, CA.D)
    held = np.concatenate([CA.task_rows(t, "held")[0] for t in range(CA.TASKS)])
    with torch.no_grad():
        logits = model._network.fc_only(torch.from_numpy(held)).numpy()

    # the conditions the tests put on these inputs, checked where the seeds are chosen (change the inputs' scale, never a cap)
    r64 = CA.run_fixture()
    kappa = [float(np.linalg.cond(covs[c].astype(np.float64))) for c in range(covs.shape[0])]
    moved = max(np.abs(W.astype(np.float64) - W0).max(), np.abs(b.astype(np.float64) - b0).max())
    dev_ref = max(np.abs(W - r64["W"]).max(), np.abs(b - r64["b"]).max())
    gap = CA.top2_gap(logits)
    out_rule = gap <= 8 * dev_ref * np.abs(held.astype(np.float64)).sum(1)
    agree = np.argmax(logits, 1) == np.argmax(r64["logits"], 1)
    print(f"kappa(cov) per class: {', '.join(f'{k:.3e}' for k in kappa)} (cap 1e4)")
    print(f"max |heads_after - heads_before| {moved:.4e}; dev_ref = max |reference fp32 heads - ca_ref fp64 heads| {dev_ref:.4e} = {dev_ref / moved:.3e} of it "
          f"(cap 2.5e-4)")
    print(f"held-out rows: {len(held)}, left out by the top-2 gap rule {out_rule.mean():.4f} (cap 0.02), reference arg-max equals the fp64 one on the "
          f"others: {bool(agree[~out_rule].all())}; means off fp64 by {np.abs(means - r64['means']).max():.2e}, covariances by "
          f"{np.abs(covs - r64['covs']).max():.2e}")
    assert max(kappa) <= 1e4 and dev_ref <= 2.5e-4 * moved and out_rule.mean() <= 0.02 and agree[~out_rule].all()

    out = {"means": means, "cov_diag": np.stack([np.diag(c) for c in covs]), "cov_corner": covs[:, :16, -16:].copy(),
           "cov_sum": covs.astype(np.float64).sum((1, 2)), "W_before": W0, "b_before": b0, "W_after": W, "b_after": b, "held_logits": logits,
           "dev_ref": np.float64(dev_ref)}
    path = os.path.join(ROOT, "tests", "golden", "ca_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
