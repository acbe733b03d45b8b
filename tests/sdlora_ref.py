"""Plain-torch fp64 restatement of SD-LoRA in the effective-weight form the HIP path uses (csrc/sdlora.hip):

    W_eff[q rows] = W[q rows] + sum_i c_i B_i A_i,  c_T = m_T,  c_i = m_i / (|B_i|_F |A_i|_F) for i < T, or 0 when a norm is 0

(v rows likewise, k rows untouched).  tests/test_sdlora_cpu.py holds it to tests/golden/sdlora_tiny.npz (fp64 runs of the reference's own classes) at
1e-10; the GPU tests compare the kernels and the method with it.
"""
import torch
import torch.nn.functional as F

from oracle import vit as ov

LISTS = ("lora_A_q_list", "lora_B_q_list", "lora_A_v_list", "lora_B_v_list")
CFG = dict(img=32, patch=8, dim=64, depth=2, heads=2, mlp=256)          # the method part of the fixture
LR, MOM, INC = 0.05, 0.9, 3


def inv_norms(A, B):
    """[T + 1]: 1 / (|B_i| |A_i|) of the past terms (0 where a norm is 0), 1 for the last"""
    out = []
    for a, b in zip(A[:-1], B[:-1]):
        n = torch.linalg.vector_norm(a.detach()) * torch.linalg.vector_norm(b.detach())
        out.append(1.0 / n if float(n) != 0.0 else torch.zeros((), dtype=a.dtype))
    return torch.stack(out + [torch.ones((), dtype=A[0].dtype)])


def delta(A, B, mag, inv):
    """sum_i mag_i inv_i B_i A_i, terms in order"""
    d = 0.0
    for i in range(len(A)):
        d = d + mag[i] * inv[i] * (B[i] @ A[i])
    return d


def effective_qkv(W, Aq, Bq, Av, Bv, mag, inv_q=None, inv_v=None):
    inv_q = inv_norms(Aq, Bq) if inv_q is None else inv_q
    inv_v = inv_norms(Av, Bv) if inv_v is None else inv_v
    q, k, v = W.chunk(3, dim=0)
    return torch.cat([q + delta(Aq, Bq, mag, inv_q), k, v + delta(Av, Bv, mag, inv_v)], dim=0)


def attention(x, P, prefix, heads, W_eff):
    """MultiHeadAttention_SDLoRA.forward with the branch folded into the weight"""
    Q = dict(P)
    Q[prefix + "attn.qkv.weight"] = W_eff
    return ov.attention(Q, prefix, x, heads)


def grads(X, dqkv, Aq, Bq, Av, Bv, mag, inv_q, inv_v):
    """the five results of clhip_sdlora_grad for one layer: dA_q, dB_q, dA_v, dB_v [of the last term], dmag row [T + 1]"""
    D = X.shape[1]
    out, dm = [], torch.zeros(len(mag), dtype=X.dtype)
    for A, B, inv, dY in ((Aq, Bq, inv_q, dqkv[:, :D]), (Av, Bv, inv_v, dqkv[:, 2 * D:])):
        for i in range(len(A)):
            S = dY.T @ (X @ A[i].T)
            dm[i] += inv[i] * (S * B[i]).sum()
        out += [mag[-1] * ((dY @ B[-1]).T @ X), mag[-1] * S]
    return out[0], out[1], out[2], out[3], dm


def grads_bounded(X64, dY64, host, mag, inv, q, v):
    """clhip_sdlora_grad's five results with their error bounds (the rule and the numbers of tests/test_sdlora_kernels_gpu.py, which imports this; the
    executor's test applies the same).  host = [A_q terms, B_q terms, A_v terms, B_v terms] (fp32 masters), mag [T + 1], inv [2, T + 1]; q rounds a factor to the
    compute dtype where the MFMA products read it, v = 2^-8 in the bf16 mode, else 0.  -> ([dA_q, dB_q, dA_v, dB_v, dmag], the same five bounds)"""
    U = 2.0 ** -24
    M, D = X64.shape
    m64, inv64, T1 = mag.double(), inv.double(), len(host[0])
    mT = m64[-1]
    want_dm, e_dm = torch.zeros(T1, dtype=torch.float64), torch.zeros(T1, dtype=torch.float64)
    want, bound = [None] * 5, [None] * 5
    for w, dYw in ((0, dY64[:, :D]), (1, dY64[:, 2 * D:])):
        A, B = host[2 * w], host[2 * w + 1]
        for i in range(T1):
            A16, Bi = q(A[i]).double(), B[i].double()
            P = X64 @ A16.T
            eP = D * U * (X64.abs() @ A16.abs().T) + 2 * v * P.abs()
            S = dYw.T @ P
            eS = dYw.abs().T @ eP + (M + 2) * U * (dYw.abs().T @ P.abs())
            term = inv64[w, i] * (S * Bi).sum()
            want_dm[i] += term
            e_dm[i] += inv64[w, i].abs() * ((eS * Bi.abs()).sum() + (D * A[i].shape[0] + 3) * U * (S.abs() * Bi.abs()).sum()) + 2 * U * term.abs()
        want[2 * w + 1] = mT * S                                                                       # (S of the last term)
        bound[2 * w + 1] = mT.abs() * eS + U * want[2 * w + 1].abs()
        B16 = q(B[-1]).double()
        Uw = dYw @ B16
        eU = D * U * (dYw.abs() @ B16.abs()) + 2 * v * Uw.abs()
        want[2 * w] = mT * (Uw.T @ X64)
        bound[2 * w] = mT.abs() * (eU.T @ X64.abs() + (M + 2) * U * (Uw.abs().T @ X64.abs())) + U * want[2 * w].abs()
    want[4], bound[4] = want_dm, e_dm + U * want_dm.abs()
    return want, bound


# ------------------------------------------------------------------------------------------------- the method on the tiny ViT
class Method:
    """SD_LoRA on a dict of fp64 tensors: the state `before_task` leaves is loaded from the fixture (its random draws are the reference's)"""

    def __init__(self, P, dtype=torch.float64):
        self.P = {k: v.to(dtype) for k, v in P.items()}          # `feat.*` backbone weights
        self.known = 0
        self.past = []                                            # per finished task: {name: tensor} of its frozen factors
        self.dtype = dtype

    def start_task(self, t, init):
        """init: {parameter name under `_network.`: value} of everything trainable in task t"""
        self.t = t
        self.train = {k: torch.as_tensor(v).to(self.dtype).clone().requires_grad_(True) for k, v in init.items()}
        self.mom = {k: None for k in self.train}

    def factors(self, blk, which):
        pre = f"backbone.feat.transformer.blocks.{blk}.attn."
        A = [p[pre + f"lora_A_{which}_list.{i}.weight"] for i, p in enumerate(self.past)] + [self.train[pre + f"lora_A_{which}_list.{self.t}.weight"]]
        B = [p[pre + f"lora_B_{which}_list.{i}.weight"] for i, p in enumerate(self.past)] + [self.train[pre + f"lora_B_{which}_list.{self.t}.weight"]]
        return A, B

    def mags(self):
        return [self.train[f"backbone.feat.transformer.blocks.0.attn.mag_lora.{i}"].reshape(()) for i in range(self.t + 1)]

    def logits(self, x):
        Q = dict(self.P)
        mag = self.mags()
        for b in range(CFG["depth"]):
            Aq, Bq = self.factors(b, "q")
            Av, Bv = self.factors(b, "v")
            Q[f"feat.transformer.blocks.{b}.attn.qkv.weight"] = effective_qkv(self.P[f"feat.transformer.blocks.{b}.attn.qkv.weight"], Aq, Bq, Av, Bv, mag)
        feat = ov.cls_features(Q, x, CFG)
        return F.linear(feat, self.train["classifier.weight"], self.train["classifier.bias"])

    def step(self, x, y):
        logits = self.logits(x)
        loss = F.cross_entropy(logits[:, self.known:], y - self.known)
        g = torch.autograd.grad(loss, list(self.train.values()))
        with torch.no_grad():
            for (k, p), gk in zip(self.train.items(), g):
                self.mom[k] = gk.clone() if self.mom[k] is None else MOM * self.mom[k] + gk          # torch.optim.SGD
                p -= LR * self.mom[k]
        return loss.detach(), logits.detach().argmax(1)

    def end_task(self):
        self.past.append({k: v.detach().clone() for k, v in self.train.items() if "_list." in k})
        self.known += INC


def trainable_names(t, depth=CFG["depth"]):
    """what sd_lora.py:130-136 leaves trainable in task t (named_parameters lists the shared magnitudes under the first block only)"""
    names = ["classifier.weight", "classifier.bias"]
    for b in range(depth):
        names += [f"backbone.feat.transformer.blocks.{b}.attn.{n}.{t}.weight" for n in LISTS]
    names += [f"backbone.feat.transformer.blocks.0.attn.mag_lora.{i}" for i in range(t + 1)]
    return sorted(names)
