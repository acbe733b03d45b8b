"""fp64 restatement of InfLoRA_OPT's classifier alignment (reference core/model/InfLoRA_opt.py:371-456), the seeded inputs of its tests and their bounds.

Test infrastructure shared by tests/test_class_align_cpu.py, tests/test_class_align_kernels_gpu.py, tests/test_class_align_gpu.py and
tools/gen_ca_golden.py.  Hand-written from the lines cited; nothing here is reference code.
"""
import numpy as np

from oracle import detrand
from ranpac_ref import U32, _gauss, chain_bound, top2_gap  # noqa: F401  (re-exported for the tests)

EPOCHS, NUM_SAMPLE, LR, MOMENTUM, WEIGHT_DECAY, COV_EPS = 5, 256, 0.01, 0.9, 5e-4, 1e-4          # InfLoRA_opt.py:402-406, :397

# the tiny fixture (tests/golden/ca_tiny.npz): 2 tasks of 2 classes, 48 training rows per task (about 24 per class), 32 held-out rows per task.
# The width is 768 because the reference hard-codes it (InfLoRA_opt.py:386-397).
TASKS, CLS, D, N_TRAIN, N_HELD = 2, 2, 768, 48, 32
# class-mean spread against per-row noise.  With 24 rows of noise sigma in 768 dimensions the largest eigenvalue of the sample covariance is about
# sigma^2 * (sqrt(768 / 23) + 1)^2 = 46 sigma^2 and the smallest is the 1e-4 added to the diagonal: sigma = 0.1 keeps kappa near 5e3 (<= 1e4, the
# condition tools/gen_ca_golden.py asserts), so the fp32 Cholesky of the reference itself is safe.
SEP, NOISE = 0.5, 0.1


# ------------------------------------------------------------------------------------------------ seeded inputs
def class_means():
    return (SEP * _gauss("ca/means", (TASKS * CLS, D))).astype(np.float32)


def task_rows(task, split):
    """(features fp32 [n, D], labels int64 [n]) of one task; `split` = "train" | "held".  Row order is the loader order."""
    n = N_TRAIN if split == "train" else N_HELD
    labels = task * CLS + detrand.randint(f"ca/{split}/labels/{task}", (n,), 0, CLS)
    feats = class_means()[labels] + NOISE * _gauss(f"ca/{split}/noise/{task}", (n, D))
    return feats.astype(np.float32), labels.astype(np.int64)


def init_heads():
    """[(weight fp32 [CLS, D], bias fp32 [CLS])] per task, in nn.Linear's range"""
    k = 1.0 / np.sqrt(D)
    return [(detrand.uniform(f"ca/head/w/{t}", (CLS, D), -k, k), detrand.uniform(f"ca/head/b/{t}", (CLS,), -k, k)) for t in range(TASKS)]


def normals(epoch, cls, shape=(NUM_SAMPLE, D)):
    """the standard normals of one MultivariateNormal.sample call: epoch `epoch`, class `cls` (InfLoRA_opt.py:427)"""
    return _gauss(f"ca/z/{epoch}/{cls}", shape)


def normals_epoch(epoch, n_classes):
    return np.concatenate([normals(epoch, c) for c in range(n_classes)])


def permutation(epoch, n):
    """the shuffle of one epoch (InfLoRA_opt.py:435)"""
    return np.argsort(detrand.uniform(f"ca/perm/{epoch}", (n,)), kind="stable").astype(np.int64)


# ------------------------------------------------------------------------------------------------ the restatement (fp64)
def moments(feats, labels, class_lo, n_classes, eps=COV_EPS):
    """(means [n_classes, D], covs [n_classes, D, D]): InfLoRA_opt.py:392-397"""
    feats, labels = np.asarray(feats, np.float64), np.asarray(labels)
    means, covs = [], []
    for c in range(n_classes):
        x = feats[labels == class_lo + c]
        m = x.mean(0)
        xc = x - m
        means.append(m)
        covs.append(xc.T @ xc / (x.shape[0] - 1) + eps * np.eye(feats.shape[1]))
    return np.stack(means), np.stack(covs)


def mean_scale(n_classes, inc_cls_num, task_idx):
    task_id = np.arange(n_classes) // inc_cls_num
    return 0.9 + (task_id + 1) / (task_idx + 1) * 0.1                 # InfLoRA_opt.py:419-422


def sample(means, scale, chols, z, perm, class_lo=0):
    """(X, labels) after the shuffle: row r is draw perm[r] of the class-major stack scale * mean + z L^T (InfLoRA_opt.py:418-437)"""
    C = means.shape[0]
    S = z.shape[0] // C
    z = np.asarray(z, np.float64).reshape(C, S, -1)
    X = np.concatenate([scale[c] * means[c] + z[c] @ np.asarray(chols[c], np.float64).T for c in range(C)])
    labels = class_lo + np.repeat(np.arange(C), S)
    return X[perm], labels[perm]


def cosine_lr(epoch):
    return 0.5 * LR * (1.0 + np.cos(np.pi * epoch / EPOCHS))          # CosineAnnealingLR(T_max = EPOCHS), eta_min 0 (InfLoRA_opt.py:413)


def align(means, covs, W, b, task_idx, inc_cls_num, normal_fn=normals_epoch, perm_fn=permutation):
    """InfLoRA_opt.py:399-456 on the flat heads W [C, D], b [C]; returns the aligned (W, b)"""
    W, b = np.array(W, np.float64), np.array(b, np.float64)
    C = (task_idx + 1) * inc_cls_num
    chols = np.stack([np.linalg.cholesky(np.asarray(covs[c], np.float64)) for c in range(C)])
    scale = mean_scale(C, inc_cls_num, task_idx)
    mW, mb = np.zeros_like(W), np.zeros_like(b)
    for ep in range(EPOCHS):
        X, y = sample(np.asarray(means[:C], np.float64), scale, chols, normal_fn(ep, C), perm_fn(ep, C * NUM_SAMPLE))
        lr = cosine_lr(ep)
        for it in range(C):
            x, t = X[it * NUM_SAMPLE:(it + 1) * NUM_SAMPLE], y[it * NUM_SAMPLE:(it + 1) * NUM_SAMPLE]
            logits = x @ W.T + b
            p = np.exp(logits - logits.max(1, keepdims=True))
            p /= p.sum(1, keepdims=True)
            p[np.arange(len(t)), t] -= 1.0
            p /= len(t)                                               # d mean-CE / d logits
            gW, gb = p.T @ x + WEIGHT_DECAY * W, p.sum(0) + WEIGHT_DECAY * b
            mW, mb = MOMENTUM * mW + gW, MOMENTUM * mb + gb           # torch.optim.SGD: buf = momentum * buf + (grad + wd * p)
            W, b = W - lr * mW, b - lr * mb
    return W, b


def run_fixture():
    """the whole two-task run in fp64 on the seeded inputs: dict with means, covs, heads_before / heads_after (flat W, b) and the held-out logits"""
    heads = init_heads()
    W0, b0 = np.concatenate([h[0] for h in heads]).astype(np.float64), np.concatenate([h[1] for h in heads]).astype(np.float64)
    means, covs = [], []
    for t in range(TASKS):
        f, l = task_rows(t, "train")
        m, c = moments(f, l, t * CLS, CLS)
        means.append(m)
        covs.append(c)
    means, covs = np.concatenate(means), np.concatenate(covs)
    W, b = align(means, covs, W0, b0, TASKS - 1, CLS)
    held = np.concatenate([task_rows(t, "held")[0] for t in range(TASKS)]).astype(np.float64)
    return {"means": means, "covs": covs, "W0": W0, "b0": b0, "W": W, "b": b, "held": held, "logits": held @ W.T + b}


# ------------------------------------------------------------------------------------------------ bounds
def mean_bound(x):
    """|fp32 mean - exact mean| per column of the rows x [n, D]: n - 1 adds and one division, every partial at most sum |x|"""
    x = np.abs(np.asarray(x, np.float64))
    return (x.shape[0] + 1) * U32 * x.sum(0) / x.shape[0]


def cov_bound(x, eps=COV_EPS):
    """|fp32 covariance - exact| per element for the rows x [n, D] of one class: the n-long chain of products of centred values (each centred value,
    the division and the eps add are the 4 extra roundings), over n - 1, plus the second-order term of the mean's own error: the first-order terms
    cancel because the exactly centred columns sum to zero.  On the diagonal eps itself is rounded twice -- once as an fp32 constant, once in the
    add, whose result is at most cov + eps -- and where a class varies little in a column (cov_ii << eps) those 2 * 2^-24 * eps are all there is:
    the chain term scales with cov_ii alone.  The fp32 storage of the reference's fp64 result carries the same term."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    xc = np.abs(x - x.mean(0))
    d = mean_bound(x)
    return chain_bound(n, xc.T @ xc, extra=4) / (n - 1) + n * np.outer(d, d) / (n - 1) + 2 * U32 * eps * np.eye(x.shape[1])


def sample_bound(mean, scale, chol, z):
    """|fp32 draw - exact| for the rows z [S, D] of one class: element j is a (j + 1)-long chain; the scaled mean and its add are 2 more roundings"""
    L = np.abs(np.tril(np.asarray(chol, np.float64)))
    mag = np.abs(scale * np.asarray(mean, np.float64))[None, :] + np.abs(np.asarray(z, np.float64)) @ L.T
    return (np.arange(L.shape[0]) + 1 + 2)[None, :] * U32 * mag
