"""Write tests/golden/ranpac_tiny.npz by running the REFERENCE's own RanPAC (core/model/ranpac.py) on the CPU, imported through oracle.ref_shim.

Build-container only (needs the reference tree).  The backbone is a stand-in subclass of the reference's `ViT_in21k_adapter` whose `feat` flattens a
given feature vector, so the plugin's own code -- hooks, classifier, Gram / label sums, ridge search, solves -- runs unchanged on the seeded features
of tests/ranpac_ref.py.  The reference one-hots its labels to fp32 and therefore runs in its own fp32; a float64 default dtype is refused.

    python tools/gen_ranpac_golden.py
"""
import contextlib
import io
import os
import re
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import ranpac_ref as R  # noqa: E402


class _Set:
    def __init__(self, feats, labels):
        self.feats, self.labels, self.trfms = torch.from_numpy(feats), torch.from_numpy(labels), "train"


class _Loader:
    """the slice of the DataLoader interface the plugin touches: `.dataset.trfms` and iteration over {"image", "label"} batches, in row order"""

    def __init__(self, feats, labels, batch=32):
        self.dataset, self.batch = _Set(feats, labels), batch

    def __iter__(self):
        for s in range(0, len(self.dataset.labels), self.batch):
            yield {"image": self.dataset.feats[s:s + self.batch], "label": self.dataset.labels[s:s + self.batch]}


def main():
    if torch.get_default_dtype() != torch.float32:
        raise RuntimeError("the reference runs RanPAC in fp32 (labels are one-hot fp32, ranpac.py:246): do not change the default dtype")
    ref_shim.install_vit_standins()
    ref = ref_shim.load("core.model.ranpac")

    class Standin(ref.ViT_in21k_adapter):
        def __init__(self, feat_dim):
            nn.Module.__init__(self)
            self.feat_dim, self.prompt, self.task_id = feat_dim, None, None
            self.feat = nn.Flatten()

    model = ref.RanPAC(Standin(R.D), "cpu", first_session_training=False, init_cls_num=R.CLS, inc_cls_num=R.CLS, total_cls_num=R.TASKS * R.CLS,
                       task_num=R.TASKS, M=R.M)
    out = {}
    test_feats, test_labels = [], []
    fp64 = None
    for t in range(R.TASKS):
        ftr, ltr = R.task_rows(t, "train")
        fte, lte = R.task_rows(t, "test")
        test_feats.append(fte)
        test_labels.append(lte)
        train, tests = _Loader(ftr, ltr), [_Loader(f, l) for f, l in zip(test_feats, test_labels)]
        model.before_task(t, None, train, tests)
        if t == 0:
            torch.manual_seed(R.W_SEED)              # W_rand is the next draw from the global generator (ranpac.py:221)
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            model.after_task(t, None, train, tests)
        ridge = float(re.search(r"Optimal lambda: ([0-9.e+-]+)", log.getvalue()).group(1))
        assert train.dataset.trfms == tests[0].dataset.trfms          # ranpac.py:234
        if t == 0:
            out["W_rand"] = model.W_rand.numpy().copy()
            fp64 = R.Ridge64(out["W_rand"])
        X, Y = np.concatenate(test_feats), np.concatenate(test_labels)
        logits, acc = model.inference({"image": torch.from_numpy(X), "label": torch.from_numpy(Y)})
        logits = logits.detach().numpy()
        assert logits.dtype == np.float32 and model.G.dtype == torch.float32
        G = model.G.numpy()
        out.update({f"train_feats_{t}": ftr, f"train_labels_{t}": ltr, f"test_feats_{t}": fte, f"test_labels_{t}": lte,
                    f"ridge_exp_{t}": np.int64(round(np.log10(ridge))), f"Q_{t}": model.Q.numpy().copy(),
                    f"G_diag_{t}": np.diag(G).copy(), f"G_corner_{t}": G[:16, -16:].copy(), f"G_sum_{t}": np.float64(G.astype(np.float64).sum()),
                    f"Wo_{t}": model._network.classifier.weight.detach().numpy().copy(), f"logits_{t}": logits, f"acc_{t}": np.float64(acc)})
        # the conditions tests/test_ranpac_cpu.py puts on these inputs, checked where the seeds are chosen
        fp64.fit(ftr, ltr, (t + 1) * R.CLS)
        srt = np.sort(fp64.losses)
        l64 = fp64.logits(X)
        dev = np.abs(l64 - logits).max()
        near = float(np.mean(R.top2_gap(l64) < 2 * dev))
        print(f"task {t}: ridge 1e{fp64.ridge_exp} (reference 1e{int(out[f'ridge_exp_{t}'])}), second-best / best hold-out loss {srt[1] / srt[0]:.3f}, "
              f"accuracy {acc:.4f}, reference fp32 logits off fp64 by {dev:.2e}, near-tie rows {near:.4f}")
        assert fp64.ridge_exp == int(out[f"ridge_exp_{t}"]) and srt[1] >= 1.05 * srt[0] and 0.6 <= acc <= 0.97 and near <= 0.02
    path = os.path.join(ROOT, "tests", "golden", "ranpac_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
