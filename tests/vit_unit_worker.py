"""Child process of tests/test_vit_plan_units_gpu.py (a helper, not a test): ONE form of the ViT executor (csrc/vit_plan.hip), its CLHIP_<NAME> switches set by
the parent in this process's environment (WGRAD_STREAM, ATTN_GENERIC and the GEMM route switches are cached at their first use).
usage: python vit_unit_worker.py DTYPE CASE_ID[,CASE_ID...] [capture]
The C API is driven through _lib directly, so the layouts and flags are this file's own choice.  For every case (vit_plan_ref.CASES), in the order given:
  step 0 at the mode's first batch, no Gram buffer (h1 aliases the LN2 scratch unless LoRA / SD-LoRA keep it); step 1 at the other batch (the layout changes) with a
  Gram buffer of zeros; then a non-saving forward with the same, now non-zero, Gram buffer (the ping-pong layout and the contiguous h1 region): its feat must be
  bitwise the saving forward's and the Gram is judged as an accumulation.
Every step allocates exactly clhip_vit_workspace_bytes (asserted equal to the parent commit's recorded total) plus a 4 KB guard, fills workspace, guard, tap and
every output the kernels are documented to overwrite (the LoRA-Sub factor gradients and their scratch among them) with 0xFF bytes (NaN in both types), the
accumulated lora_B gradients with a known value, reads every stored
tensor once and judges it with vit_plan_ref.judge.  With `capture` the backward runs under torch.cuda.graph capture and one replay.  After step 0 the refusals
are tried: each must return an error, set clhip_last_error and launch nothing.
Prints `RATIOS {case: {"s<step> <link>": worst err / bound}}`, `INFO {case: {...}}`, `BITS {case: {"s<step>": sha1 of the tap and of the parameter gradients}}`,
`SECONDS {case: s}`, a `FAIL ...` line per link outside its bound; exit status 1 when there is one."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                              # noqa: E402

import vit_plan_ref as VP                 # noqa: E402
import vit_refs as VR                     # noqa: E402
from libcontinual_amd import _lib         # noqa: E402
from libcontinual_amd._lib import call    # noqa: E402

DEV = "cuda:0"
TD = {"bf16": torch.bfloat16, "f32": torch.float32}
CODE = {"bf16": _lib.BF16, "f32": _lib.F32}
GUARD = 4096
SEED_WORD = 0x1234567887654321


def st():
    return torch.cuda.current_stream().cuda_stream


def al(v):
    return (v + 255) // 256 * 256


def nan_f32(*shape):
    """an fp32 tensor of 0xFF bytes (a NaN)"""
    n = 1
    for s in shape:
        n *= s
    return torch.full((4 * n,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32).reshape(shape)


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def grads(**members):
    """a clhip_vit_grads: a tensor gives its pointer, a list of tensors a pointer table (kept alive by the structure), None stays NULL"""
    g = _lib.VitGrads()
    for k, v in members.items():
        if v is not None:
            setattr(g, k, ptrs(v) if isinstance(v, list) else v.data_ptr())
    return g


def cpu64(t):
    return t.double().cpu()


class Exec:
    """one executor with its parameters, shadow and device tables (everything the C side points to stays alive here)"""

    def __init__(self, c, P, dt):
        self.c, self.P, self.dt, self.e = c, P, dt, 2 if dt == "bf16" else 4
        lib = _lib.lib()
        desc = _lib.VitDesc(c["img"], c["patch"], c["dim"], c["depth"], c["heads"], c["mlp"], c["lora_rank"], VP.BLOCK_EPS, c["adapter_dim"], VP.ADAPTER_SCALE)
        self.h = lib.clhip_vit_create(C.byref(desc), CODE[dt])
        assert self.h, lib.clhip_last_error()
        self.keep = []
        d = lambda t: self._own(t.float().contiguous().to(DEV))
        self.layers = (_lib.VitLayerParams * c["depth"])()
        for l, L in enumerate(P["layers"]):
            lp = self.layers[l]
            for k in ("qkv_w", "qkv_b", "proj_w", "proj_b", "ln1_w", "ln1_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ln2_w", "ln2_b"):
                setattr(lp, k, d(L[k]).data_ptr())
            if c["lora_rank"]:
                for k in ("lora_a_k", "lora_b_k", "lora_a_v", "lora_b_v"):
                    setattr(lp, k, d(L[k]).data_ptr())
            if c["adapter_dim"]:
                for k, t in zip(("ad_down_w", "ad_down_b", "ad_up_w", "ad_up_b"), L["adapter"]):
                    setattr(lp, k, d(t).data_ptr())
        self.params = _lib.VitParams(d(P["cls"]).data_ptr(), d(P["pos"]).data_ptr(), d(P["pe_w"]).data_ptr(), d(P["pe_b"]).data_ptr(), d(P["norm_w"]).data_ptr(),
                                     d(P["norm_b"]).data_ptr(), self.layers)
        self.prompt = d(P["prompt"])
        self.shadow = torch.zeros(lib.clhip_vit_shadow_bytes(self.h), dtype=torch.uint8, device=DEV)
        if c["sd"]:
            self.set_sdlora()
        call("clhip_vit_prep_weights", self.h, C.byref(self.params), self.shadow.data_ptr(), 1 if c["lora_rank"] else 0, 0, st())
        if c["sd"]:
            call("clhip_vit_sdlora_refresh", self.h, C.byref(self.params), self.shadow.data_ptr(), st())
        self.seed = torch.tensor([SEED_WORD], dtype=torch.int64, device=DEV)

    def _own(self, t):
        self.keep.append(t)
        return t

    def set_sdlora(self):
        P, T = self.P, len(VP.SD_RANKS)
        if not hasattr(self, "sd_tab"):
            fac = [[[self._own(t.float().contiguous().to(DEV)) for t in row] for row in L["sd"]] for L in P["layers"]]
            self.sd_tab = torch.tensor([[[t.data_ptr() for t in row] for row in lay] for lay in fac], dtype=torch.int64).to(DEV)
            self.sd_mag = P["sd_mag"].float().to(DEV)
            self.sd_inv = torch.stack([L["sd_inv"] for L in P["layers"]]).float().contiguous().to(DEV)
            self.sd_ranks = (C.c_int * T)(*VP.SD_RANKS)
        call("clhip_vit_set_sdlora", self.h, T, self.sd_ranks, self.sd_tab.data_ptr(), self.sd_mag.data_ptr(), self.sd_inv.data_ptr())

    def weights(self):
        """the compute-dtype weight copies, read from the shadow at clhip_vit_create's offsets"""
        c, e = self.c, self.e
        D, H, Kp = c["dim"], c["mlp"], c["Kp"]
        off = [0]

        def take(r, k):
            t = self.shadow[off[0]:off[0] + r * k * e].view(TD[self.dt]).reshape(r, k)
            off[0] += al(r * k * e)
            return cpu64(t)
        pe = take(D, Kp)
        wf, wb = [], []
        for _ in range(c["depth"]):
            f, b = {}, {}
            for n, r, k in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", H, D), ("fc2", D, H)):
                f[n] = take(r, k)
                b[n] = take(k, r)
            if c["lora_rank"]:
                take(32, D)
            wf.append(f), wb.append(b)
        assert off[0] == self.shadow.numel()
        return pe, wf, wb

    def read(self, ws, layer, which, shape):
        out = nan_f32(*shape)
        call("clhip_vit_read_act", self.h, ws.data_ptr(), layer, which, out.data_ptr(), st())
        return cpu64(out)


def refused(name, outs, *args):
    """the call must fail, leave clhip_last_error set and launch nothing: the 0xFF-filled outputs stay as they are"""
    lib = _lib.lib()
    rc = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    assert rc != 0 and lib.clhip_last_error(), (name, rc)
    for t in outs:
        assert bool((t.view(torch.uint8) == 0xFF).all()), (name, "wrote into an output")


def run_case(geo, mode, dt, capture):
    c = VP.mode_cfg(geo, mode)
    P = VP.trained_like(geo, mode, 4321 + len(geo) + 7 * len(mode))
    ex = Exec(c, P, dt)
    lib, h, e = _lib.lib(), ex.h, ex.e
    D, depth, Hh, R_ = c["dim"], c["depth"], c["heads"], c["adapter_dim"]
    pe_wf, wf, wb = ex.weights()
    steps = VP.batches_of(mode) if len(VP.batches_of(mode)) == 2 else VP.batches_of(mode) * 2
    ratios, info, bits = {}, {}, {}
    lora_acc = [torch.full((D, VP.LORA_RANK), 0.25, device=DEV) for _ in range(2 * depth)] if c["lora_rank"] else None
    gram = torch.zeros(depth, D, D, device=DEV)
    feat_saved = None
    for i, (B, npr) in enumerate(steps):
        w = VP.wants(c, npr)
        N = npr + 1 + c["np"]
        M = B * N
        flags = 1 | (2 if i == 1 else 0)
        need = lib.clhip_vit_workspace_bytes(h, B, npr, flags)
        key = f"{geo}-{mode}-{dt}-b{B}-p{npr}-f{flags}"
        assert need == VP.WS_TOTALS[key], (key, need, VP.WS_TOTALS[key])          # the read access costs no workspace: the parent commit's totals
        ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        X = VP.step_inputs(c, B, npr, 77, dt)
        img, dfeat = X["img"].to(DEV), X["dfeat"].to(DEV)
        pk = [None if t is None else t.to(DEV).to(TD[dt]) for t in X["pk"]]
        pv = [None if t is None else t.to(DEV).to(TD[dt]) for t in X["pv"]]
        if c["prefix"]:
            call("clhip_vit_set_prefix", h, (C.c_int * depth)(*c["Lp"]), ptrs(pk), ptrs(pv))
        if c["p"] > 0:
            call("clhip_vit_set_adapter_dropout", h, ex.seed.data_ptr(), c["p"])
            for l in range(depth):
                m = torch.empty(M, R_, dtype=torch.uint8, device=DEV)
                call("clhip_adapter_dropout_mask", ex.seed.data_ptr(), l, M, R_, c["p"], m.data_ptr(), st())
                X["mask"][l] = m.cpu()
        feat = nan_f32(B, D)
        gram0 = gram.clone() if i == 1 else None
        call("clhip_vit_forward", h, C.byref(ex.params), ex.shadow.data_ptr(), ws.data_ptr(), img.data_ptr(), B, ex.prompt.data_ptr() if npr else None, npr, 1,
             gram.data_ptr() if i == 1 else None, feat.data_ptr(), st())
        tm, total = VP.tap_map(c, M)
        assert lib.clhip_vit_tap_floats(h) == total, (lib.clhip_vit_tap_floats(h), total)
        tapbuf = nan_f32(total)
        call("clhip_vit_set_tap", h, tapbuf.data_ptr(), total)
        dprompt = nan_f32(npr, D) if w["dprompt"] else None
        d_ad = [nan_f32(*s) for _ in range(depth) for s in ((R_, D), (R_,), (D, R_), (D,))] if w["adapter"] else None
        rT = VP.SD_RANKS[-1]
        d_sd = [nan_f32(*s) for _ in range(depth) for s in ((rT, D), (D, rT), (rT, D), (D, rT))] if w["sd"] else None
        d_rows, d_mag = (nan_f32(depth, len(VP.SD_RANKS)), nan_f32(len(VP.SD_RANKS))) if w["sd"] else (None, None)
        dpk = [None if not lp else nan_f32(B * lp, D) for lp in c["Lp"]] if w["prefix"] else None
        dpv = [None if not lp else nan_f32(B * lp, D) for lp in c["Lp"]] if w["prefix"] else None
        rk = VP.LORA_RANK
        d_ab = [nan_f32(*s) for _ in range(depth) for s in ((rk, D), (D, rk), (rk, D), (D, rk))] if w["ab"] else None      # written, not accumulated into
        ab_ws = torch.full((lib.clhip_lora_grad_ab_ws_bytes(M, D),), 0xFF, dtype=torch.uint8, device=DEV) if w["ab"] else None
        lora0 = [cpu64(t) for t in lora_acc] if w["lora"] else None
        common = (h, C.byref(ex.params), ex.shadow.data_ptr(), ws.data_ptr(), dfeat.data_ptr())
        G = grads(dprompt_tokens=dprompt, d_lora_b=lora_acc if w["lora"] else None, d_adapter=d_ad, d_sd=d_sd, d_mag_rows=d_rows, d_mag=d_mag, d_ab=d_ab, ab_ws=ab_ws,
                  dpk=dpk, dpv=dpv)

        def backward(stream):
            call("clhip_vit_backward", *common, C.byref(G), stream)
        if capture:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                backward(st())
            graph.replay()
        else:
            backward(st())
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xFF).all()), "the guard behind the workspace was written"
        side, low = C.c_int(-1), C.c_int(-1)
        call("clhip_vit_last_backward_info", h, C.byref(side), C.byref(low))
        info[f"s{i}"] = dict(side=side.value, lowest=low.value, B=B, n_prompt=npr)
        ratios[f"s{i} lowest_layer_run"] = 0.0 if low.value == VP.lowest_layer(c, npr) else float("inf")
        if low.value != VP.lowest_layer(c, npr):
            print(f"FAIL {geo}-{mode} step {i} lowest_layer_run: {low.value}, the rule says {VP.lowest_layer(c, npr)}", flush=True)
        # ---- one read of every stored tensor
        R = dict(B=B, N=N, M=M, n_prompt=npr, dt=dt, img=X["img"].double(), dfeat=X["dfeat"].double(), mask=X["mask"], pk=X["pk"], pv=X["pv"], pe_wf=pe_wf, wf=wf, wb=wb)
        view = lambda off, r, k: cpu64(ws[off:off + r * k * e].view(TD[dt]).reshape(r, k))
        R["patches"] = view(0, B * c["np"], c["Kp"])
        R["pe_out"] = view(al(B * c["np"] * c["Kp"] * e), B * c["np"], D)
        own_h1 = bool(c["lora_rank"] or c["sd"] or i == 1)
        R["x"] = [ex.read(ws, l, 0, (M, D)) for l in range(depth + 1)]
        R["qkv"] = [ex.read(ws, l, 1, (M, 3 * D)) for l in range(depth)]
        R["attn_o"] = [ex.read(ws, l, 2, (M, D)) for l in range(depth)]
        R["x_mid"] = [ex.read(ws, l, 3, (M, D)) for l in range(depth)]
        R["hpre"] = [ex.read(ws, l, 4, (M, c["mlp"])) for l in range(depth)]
        R["h1"] = [ex.read(ws, l, 5, (M, D)) if own_h1 else None for l in range(depth)]
        R["lse"] = [ex.read(ws, l, 6, (B, Hh, N)) for l in range(depth)]
        R["st1"] = [ex.read(ws, l, 7, (2, M)) for l in range(depth)]
        R["st2"] = [ex.read(ws, l, 8, (2, M)) for l in range(depth)]
        R["ad_hd"] = [ex.read(ws, l, 9, (M, R_)) if R_ else None for l in range(depth)]
        R["feat"] = cpu64(feat)
        R["gram0"], R["gram"] = (cpu64(gram0), cpu64(gram)) if i == 1 else (None, None)
        tcpu = tapbuf.cpu()
        R["tap"] = {}
        for k, (off, n, cols) in tm.items():
            t = tcpu[off:off + n]
            if bool(torch.isnan(t).all()):                                       # an untouched slot: still the 0xFF fill
                assert bool((t.view(torch.int32) == -1).all()), k
                continue
            R["tap"][k] = t.double().reshape(-1, cols)
        R["dprompt"] = cpu64(dprompt) if w["dprompt"] else None
        R["d_lora_b0"] = [(lora0[2 * l], lora0[2 * l + 1]) for l in range(depth)] if w["lora"] else None
        R["d_lora_b"] = [(cpu64(lora_acc[2 * l]), cpu64(lora_acc[2 * l + 1])) if w["lora"] else None for l in range(depth)]
        R["d_adapter"] = [tuple(cpu64(t) for t in d_ad[4 * l:4 * l + 4]) if w["adapter"] else None for l in range(depth)]
        R["d_sd"] = [tuple(cpu64(t) for t in d_sd[4 * l:4 * l + 4]) if w["sd"] else None for l in range(depth)]
        R["d_ab"] = [tuple(cpu64(t) for t in d_ab[4 * l:4 * l + 4]) if w["ab"] else None for l in range(depth)]
        if w["sd"]:
            R["d_mag_rows"], R["d_mag"] = cpu64(d_rows), cpu64(d_mag)
        R["dpk"] = [cpu64(t) if (t is not None and l >= low.value) else None for l, t in enumerate(dpk)] if w["prefix"] else [None] * depth
        R["dpv"] = [cpu64(t) if (t is not None and l >= low.value) else None for l, t in enumerate(dpv)] if w["prefix"] else [None] * depth
        if w["prefix"]:                                                          # layers the backward did not run keep their fill
            for l in range(low.value):
                assert dpk[l] is None or bool(torch.isnan(dpk[l]).all())
        V = VP.judge(c, P, R)
        for k, v in V.worst_by_link().items():
            ratios[f"s{i} {k}"] = v
        for k, v in V.failures().items():
            print(f"FAIL {geo}-{mode} step {i} {k}: {v:.4g}", flush=True)
        leaves = [t for ts in (lora_acc if w["lora"] else None, d_ad, d_sd, [d_rows, d_mag] if w["sd"] else None, d_ab, dpk, dpv, [dprompt]) if ts for t in ts if t is not None]
        sha = lambda ts: hashlib.sha1(b"".join(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in ts)).hexdigest()
        bits[f"s{i}"] = dict(tap=sha([tapbuf]), leaves=sha(leaves) if leaves else "")
        call("clhip_vit_set_tap", h, None, 0)
        if i == 0:
            refusals(ex, c, ws, X, dfeat, B, npr, own_h1, pk, pv)
        if mode == "prefix" and npr > 0:
            # the same saved forward again, now with the prompt gradient: the chain runs to layer 0 and the prefix gradients of the layers above stay bitwise
            dp2, dpk2, dpv2 = nan_f32(npr, D), [None if t is None else nan_f32(*t.shape) for t in dpk], [None if t is None else nan_f32(*t.shape) for t in dpv]
            call("clhip_vit_backward", *common, C.byref(grads(dprompt_tokens=dp2, dpk=dpk2, dpv=dpv2)), st())
            torch.cuda.synchronize()
            call("clhip_vit_last_backward_info", h, C.byref(side), C.byref(low))
            assert low.value == 0 and info[f"s{i}"]["lowest"] == (1 if depth > 1 else 0)
            assert bool(torch.isfinite(dp2).all())
            for l in range(1, depth):
                assert torch.equal(dpk[l], dpk2[l]) and torch.equal(dpv[l], dpv2[l]), l
            info[f"s{i}"]["lowest_with_dprompt"] = low.value
        if i == 1:
            feat_saved, ws1, B1, npr1, img1, M1 = feat.clone(), ws, B, npr, img, M
    # ---- the non-saving forward: ping-pong activations, the contiguous h1 region, the Gram accumulated onto what step 1 left
    need = lib.clhip_vit_workspace_bytes(h, B1, npr1, 2)
    assert need == VP.WS_TOTALS[f"{geo}-{mode}-{dt}-b{B1}-p{npr1}-f2"]
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    if c["p"] > 0:
        call("clhip_vit_set_adapter_dropout", h, ex.seed.data_ptr(), c["p"])
    feat2, gram1 = nan_f32(B1, D), cpu64(gram)
    call("clhip_vit_forward", h, C.byref(ex.params), ex.shadow.data_ptr(), ws.data_ptr(), img1.data_ptr(), B1, ex.prompt.data_ptr() if npr1 else None, npr1, 0,
         gram.data_ptr(), feat2.data_ptr(), st())
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xFF).all()), "the guard behind the workspace was written"
    assert torch.equal(feat2, feat_saved), "the non-saving forward's feat differs from the saving forward's"
    worst = 0.0
    for l in range(depth):
        h1 = ex.read(ws, l, 5, (M1, D))
        ref = gram1[l] + VR.gram_ref(h1)
        rel = VR.GRAM_BATCHED if (depth > 1 and dt == "bf16") else VR.GRAM
        worst = max(worst, VR.err_ratio(cpu64(gram[l]), ref, rel * float(ref.abs().max())))
    ratios["nosave gram"] = worst
    if not worst <= 1.0:
        print(f"FAIL {geo}-{mode} non-saving forward gram: {worst:.4g}", flush=True)
    out = nan_f32(M1, D)
    refused("clhip_vit_read_act", [out], h, ws.data_ptr(), 0, 0, out.data_ptr(), st())                       # x_in is one of two ping-pong buffers there
    refused("clhip_vit_backward", [out], h, C.byref(ex.params), ex.shadow.data_ptr(), ws.data_ptr(), out.data_ptr(), None, st())           # a backward after a non-saving forward
    lib.clhip_vit_destroy(h)
    return ratios, info, bits


def refusals(ex, c, ws, X, dfeat, B, npr, own_h1, pk, pv):
    """after a saved forward: every call below must be refused with nothing launched (their outputs keep the 0xFF fill)"""
    h, D, depth = ex.h, c["dim"], c["depth"]
    M = B * (npr + 1 + c["np"])
    base = (h, C.byref(ex.params), ex.shadow.data_ptr(), ws.data_ptr(), dfeat.data_ptr())
    out = nan_f32(M, D)
    big = [nan_f32(B * 8, D) for _ in range(depth)]
    if not own_h1:
        refused("clhip_vit_read_act", [out], h, ws.data_ptr(), 0, 5, out.data_ptr(), st())               # h1 == ln_out: whatever LN2 left there
    if not c["adapter_dim"]:
        refused("clhip_vit_read_act", [out], h, ws.data_ptr(), 0, 9, out.data_ptr(), st())
        d_ad = [nan_f32(D, 16) for _ in range(4 * depth)]
        refused("clhip_vit_backward", d_ad, *base, C.byref(grads(d_adapter=d_ad)), st())                  # d_adapter on an executor without adapters
    if npr == 0:
        refused("clhip_vit_backward", [out], *base, C.byref(grads(dprompt_tokens=out)), st())             # dprompt when n_prompt == 0
    if c["prefix"]:
        refused("clhip_vit_backward", [out], *base, None, st())                                           # dpk missing after a prefixed forward
        refused("clhip_vit_backward", big, *base, C.byref(grads(dpk=big)), st())                          # dpk without dpv
    else:
        refused("clhip_vit_backward", big, *base, C.byref(grads(dpk=big, dpv=big)), st())                 # dpk given after a plain forward
    if c["lora_rank"]:
        rk = c["lora_rank"]
        d_ab = [nan_f32(*s) for _ in range(depth) for s in ((rk, D), (D, rk), (rk, D), (D, rk))]
        d_b = [nan_f32(D, rk) for _ in range(2 * depth)]
        ab_ws = torch.full((_lib.lib().clhip_lora_grad_ab_ws_bytes(M, D),), 0xFF, dtype=torch.uint8, device=DEV)
        refused("clhip_vit_backward", d_ab + d_b + [ab_ws], *base, C.byref(grads(d_ab=d_ab, ab_ws=ab_ws, d_lora_b=d_b)), st())     # d_ab together with d_lora_b
        refused("clhip_vit_backward", d_ab, *base, C.byref(grads(d_ab=d_ab)), st())                       # d_ab without ab_ws
    feat = nan_f32(B, D)
    n_big = 256 - c["np"]                                                                                 # n_prompt + 1 + np = 257 tokens
    assert _lib.lib().clhip_vit_workspace_bytes(h, B, n_big, 1) == 0
    refused("clhip_vit_forward", [feat], h, C.byref(ex.params), ex.shadow.data_ptr(), ws.data_ptr(), X["img"].to(DEV).data_ptr(), B, ex.prompt.data_ptr(), n_big, 1,
            None, feat.data_ptr(), st())
    if c["sd"]:
        rT, T = VP.SD_RANKS[-1], len(VP.SD_RANKS)
        d_sd = [nan_f32(*s) for _ in range(depth) for s in ((rT, D), (D, rT), (rT, D), (D, rT))]
        rows, mag = nan_f32(depth, T), nan_f32(T)
        d_b = [nan_f32(D, rT) for _ in range(2 * depth)]
        refused("clhip_vit_backward", d_sd + d_b + [rows, mag], *base, C.byref(grads(d_sd=d_sd, d_mag_rows=rows, d_mag=mag, d_lora_b=d_b)), st())   # d_sd together with d_lora_b
        refused("clhip_vit_backward", d_sd + [rows], *base, C.byref(grads(d_sd=d_sd, d_mag_rows=rows)), st())                                       # d_sd without d_mag
        ex.set_sdlora()                                                                                   # a backward after clhip_vit_set_sdlora changed the term set
        refused("clhip_vit_backward", d_sd + [rows, mag], *base, C.byref(grads(d_sd=d_sd, d_mag_rows=rows, d_mag=mag)), st())


def gemm_routes(c, dt):
    """the kernel family clhip_gemm_nt_route reports for every GEMM shape of the case at both batches: {"MxNxK": [family, ...]}"""
    out = {}
    D, H = c["dim"], c["mlp"]
    for B, npr in VP.BATCHES:
        M = B * (npr + 1 + c["np"])
        for N_, K in ((3 * D, D), (D, D), (H, D), (D, H), (D, 3 * D)):
            buf = (C.c_int * 16)()
            n = _lib.lib().clhip_gemm_nt_route(M, N_, K, K, K, N_, 0, 0, CODE[dt], buf, 4)
            out[f"{M}x{N_}x{K}"] = [buf[4 * j] for j in range(max(n, 0))]
    return out


def main():
    dt = sys.argv[1]
    cases = [cs for cs in VP.CASES if VP.case_id(cs) in sys.argv[2].split(",")]
    capture = len(sys.argv) > 3 and sys.argv[3] == "capture"
    assert cases
    R, I, Bt, S, Rt = {}, {}, {}, {}, {}
    for geo, mode in cases:
        t0 = time.time()
        cid = VP.case_id((geo, mode))
        R[cid], I[cid], Bt[cid] = run_case(geo, mode, dt, capture)
        Rt[cid] = gemm_routes(VP.mode_cfg(geo, mode), dt)
        S[cid] = round(time.time() - t0, 2)
    print("RATIOS " + json.dumps(R))
    print("INFO " + json.dumps(I))
    print("BITS " + json.dumps(Bt))
    print("ROUTES " + json.dumps(Rt))
    print("SECONDS " + json.dumps(S))
    sys.exit(1 if any(not v <= 1.0 for r in R.values() for v in r.values()) else 0)


if __name__ == "__main__":
    main()
