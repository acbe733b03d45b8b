"""fp64 restatement of RanPAC's classifier (reference core/model/ranpac.py:214-266 and :49-63), the seeded inputs of its tests and their bounds.

Test infrastructure shared by tests/test_ranpac_cpu.py, tests/test_ranpac_kernels_gpu.py, tests/test_ranpac_gpu.py and tools/gen_ranpac_golden.py.
Hand-written from the lines cited; nothing here is reference code.
"""
import numpy as np

from oracle import detrand

RIDGES = 10.0 ** np.arange(-8, 9)                  # ranpac.py:253
U32 = 2.0 ** -24                                   # unit roundoff of fp32, round to nearest

# the tiny fixture (tests/golden/ranpac_tiny.npz): 3 tasks of 4 classes, feature width 24, projection width 144, 120 training and 60 test rows per task
TASKS, CLS, D, M, N_TRAIN, N_TEST = 3, 4, 24, 144, 120, 60
SEP, NOISE = 0.55, 1.0                             # class-mean spread against per-row noise: chosen for an accuracy of 0.6 .. 0.97 (the golden records it)
W_SEED = 1993


# ------------------------------------------------------------------------------------------------ seeded inputs
def _gauss(tag, shape):
    """roughly normal, exactly reproducible: the centred sum of four detrand uniforms (variance 4/3 -> scaled to 1)"""
    s = sum(detrand.uniform(f"{tag}/{i}", shape).astype(np.float64) for i in range(4))
    return (s * np.sqrt(3.0 / 4.0)).astype(np.float32)


def class_means():
    return (SEP * _gauss("ranpac/means", (TASKS * CLS, D))).astype(np.float32)


def task_rows(task, split):
    """(features fp32 [n, D], labels int64 [n]) of one task; `split` = "train" | "test".  Row order is the loader order."""
    n = N_TRAIN if split == "train" else N_TEST
    labels = task * CLS + detrand.randint(f"ranpac/{split}/labels/{task}", (n,), 0, CLS)
    feats = class_means()[labels] + NOISE * _gauss(f"ranpac/{split}/noise/{task}", (n, D))
    return feats.astype(np.float32), labels.astype(np.int64)


# ------------------------------------------------------------------------------------------------ the restatement (fp64)
def project(feats, W, relu=True):
    h = np.asarray(feats, np.float64) @ np.asarray(W, np.float64)
    return np.maximum(h, 0.0) if relu else h


def onehot(labels, C):
    y = np.zeros((len(labels), C))
    y[np.arange(len(labels)), np.asarray(labels)] = 1.0
    return y


class Ridge64:
    """state W, G, Q; `fit(features, labels, n_classes)` = one after_task (ranpac.py:216-266), `logits` = the use_RP head (ranpac.py:53-61)"""

    def __init__(self, W):
        self.W = np.asarray(W, np.float64)
        m = self.W.shape[1]
        self.G, self.Q = np.zeros((m, m)), np.zeros((m, 0))
        self.Wo = self.ridge_exp = self.losses = None

    def fit(self, feats, labels, n_classes):
        m = self.W.shape[1]
        if self.Q.shape[1] < n_classes:
            self.Q = np.concatenate([self.Q, np.zeros((m, n_classes - self.Q.shape[1]))], axis=1)
        H, Y = project(feats, self.W), onehot(labels, n_classes)
        self.Q = self.Q + H.T @ Y
        self.G = self.G + H.T @ H
        nv = int(H.shape[0] * 0.8)
        Qv, Gv = H[:nv].T @ Y[:nv], H[:nv].T @ H[:nv]
        losses = []
        for r in RIDGES:
            Wo = np.linalg.solve(Gv + r * np.eye(m), Qv).T
            losses.append(np.mean((H[nv:] @ Wo.T - Y[nv:]) ** 2))
        self.losses = np.asarray(losses)
        k = int(np.argmin(self.losses))
        self.ridge_exp = k - 8
        self.Wo = np.linalg.solve(self.G + RIDGES[k] * np.eye(m), self.Q).T
        return self.Wo

    def logits(self, feats, sigma=1.0):
        return sigma * (project(feats, self.W) @ self.Wo.T)


def top2_gap(logits):
    s = np.sort(np.asarray(logits, np.float64), axis=1)
    return s[:, -1] - s[:, -2]


# ------------------------------------------------------------------------------------------------ bounds
def chain_bound(K, abs_products_sum, extra=0):
    """|error| of a K-long fp32 fmaf chain (what the f32-input MFMA computes) against the exact sum: every partial sum is rounded once and is at most
    sum |a_i b_i| in magnitude, so the error is at most K * 2^-24 * sum |a_i b_i| to first order.  `extra` counts further roundings of values bounded by
    the same sum (the add of an accumulating call, a final scale)."""
    return (K + extra) * U32 * np.asarray(abs_products_sum, np.float64)


def solve_rel_tol(A, n_rows):
    """relative error allowed between an fp32 and an fp64 solution of A X = Q whose A and Q were themselves SUMMED in fp32 over n_rows rows:
    kappa_2(A) * (dim + n_rows) * 2^-24 -- Higham's forward bound for Gaussian elimination (dim * u * kappa, growth factor taken as 1) plus the operand
    perturbation of an n_rows-long fp32 sum (n_rows * u) carried through the same condition number."""
    return float(np.linalg.cond(A)) * (A.shape[0] + n_rows) * U32
