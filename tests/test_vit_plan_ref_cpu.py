"""The authority of tests/vit_plan_ref.py without a GPU: fed the intermediates of an independent fp64 autograd ViT (written here from nn.functional calls; it
shares no code with the helper's closed forms) the judge's chained references reproduce every link to 1e-12 on every case and mode; fed the storage-precision
emulator every link stays inside its bound in bf16 and fp32; each seeded wiring fault breaks its own link by more than 2x and no other; and the tap's slot map
and the "which slots a backward writes" rule agree with the emulator."""
import math

import pytest
import torch
import torch.nn.functional as F

import vit_plan_ref as VP

_CACHE = {}


def _setup(geo, mode):
    if (geo, mode) not in _CACHE:
        _CACHE[(geo, mode)] = (VP.mode_cfg(geo, mode), VP.trained_like(geo, mode, 4321 + len(geo) + 7 * len(mode)))
    return _CACHE[(geo, mode)]


def _gram0(c, on):
    return torch.full((c["depth"], c["dim"], c["dim"]), 0.5) if on else None


# ------------------------------------------------------------------------------------------------ an independent autograd ViT (the exact chain)
def autograd_step(c, P, X, gram0):
    """the dict of vit_plan_ref.emulate from torch autograd in fp64, no rounding anywhere"""
    B, n_prompt = X["B"], X["n_prompt"]
    D, Hh, depth, p_ = c["dim"], c["heads"], c["depth"], c["patch"]
    hd, N = D // Hh, n_prompt + 1 + c["np"]
    M, Pp = B * N, max(n_prompt, 1)
    w = VP.wants(c, n_prompt)
    dd = lambda t: t.double()
    leaf = lambda t: t.double().clone().requires_grad_(True)
    keep = []

    def hold(t):
        if not t.requires_grad:                            # (the tokens of a forward without prompt tokens: a leaf)
            t.requires_grad_(True)
        t.retain_grad()
        keep.append(t)
        return t
    img = dd(X["img"])
    prompt = leaf(P["prompt"][:n_prompt]) if n_prompt else None
    pe = F.conv2d(img, dd(P["pe_w"]).reshape(D, 3, p_, p_), dd(P["pe_b"]), stride=p_)          # [B, D, g, g]
    pe_out = pe.flatten(2).transpose(1, 2)                                                     # [B, np, D]
    tok = torch.cat([(dd(P["cls"]) + dd(P["pos"])[0]).expand(B, 1, D), pe_out + dd(P["pos"])[1:]], 1)
    if n_prompt:
        tok = torch.cat([prompt.unsqueeze(0).expand(B, -1, -1), tok], 1)
    R = dict(B=B, N=N, M=M, n_prompt=n_prompt, dt=None, img=img, dfeat=dd(X["dfeat"]), mask=X["mask"], pk=X["pk"], pv=X["pv"], pe_wf=dd(P["pe_w"]), wf=[], wb=[])
    R["patches"] = F.unfold(img, p_, stride=p_).transpose(1, 2).reshape(B * c["np"], -1)
    R["pe_out"] = pe_out.reshape(-1, D).detach()
    for k in ("h1", "st1", "st2", "qkv", "lse", "attn_o", "x_mid", "hpre", "ad_hd"):
        R[k] = [None] * depth
    x = [hold(tok.reshape(M, D))]
    T = dict(lora=[], ad=[], sd=[], pk=[], pv=[], mag=leaf(P["sd_mag"]) if c["sd"] else None)
    nodes = []
    for l, L in enumerate(P["layers"]):
        Wq = dd(L["qkv_w"])
        if c["lora_rank"]:
            ak, bk, av, bv = [leaf(L[k]) for k in ("lora_a_k", "lora_b_k", "lora_a_v", "lora_b_v")]
            T["lora"].append((ak, bk, av, bv))
            Wq = torch.cat([Wq[:D], Wq[D:2 * D] + bk @ ak, Wq[2 * D:] + bv @ av])
        if c["sd"]:
            last = [leaf(L["sd"][k][-1]) for k in range(4)]                                   # A_q, B_q, A_v, B_v of the current term
            T["sd"].append(last)
            inv = dd(L["sd_inv"])
            term = lambda k, i: last[k] if i == len(VP.SD_RANKS) - 1 else dd(L["sd"][k][i])
            dq_ = sum(T["mag"][i] * inv[0, i] * (term(1, i) @ term(0, i)) for i in range(len(VP.SD_RANKS)))
            dv_ = sum(T["mag"][i] * inv[1, i] * (term(3, i) @ term(2, i)) for i in range(len(VP.SD_RANKS)))
            Wq = torch.cat([Wq[:D] + dq_, Wq[D:2 * D], Wq[2 * D:] + dv_])
        wfl = dict(qkv=Wq.detach(), proj=dd(L["proj_w"]), fc1=dd(L["fc1_w"]), fc2=dd(L["fc2_w"]))
        R["wf"].append(wfl)
        R["wb"].append({k: v.T for k, v in wfl.items()})
        xin = x[l]
        h1 = hold(F.layer_norm(xin, (D,), dd(L["ln1_w"]), dd(L["ln1_b"]), VP.BLOCK_EPS))
        mu, var = xin.mean(1), xin.var(1, unbiased=False)
        R["st1"][l] = torch.stack([mu, 1 / torch.sqrt(var + VP.BLOCK_EPS)]).detach()
        qkv = hold(F.linear(h1, Wq, dd(L["qkv_b"])))
        q_, k_, v_ = [t.reshape(B, N, Hh, hd).transpose(1, 2) for t in qkv.split(D, dim=1)]
        Lp = c["Lp"][l]
        if Lp:
            pk, pv = leaf(X["pk"][l]), leaf(X["pv"][l])
            T["pk"].append(pk), T["pv"].append(pv)
            k_ = torch.cat([pk.reshape(B, Lp, Hh, hd).transpose(1, 2), k_], 2)
            v_ = torch.cat([pv.reshape(B, Lp, Hh, hd).transpose(1, 2), v_], 2)
        else:
            T["pk"].append(None), T["pv"].append(None)
        sc = (q_ @ k_.transpose(-1, -2)) / math.sqrt(hd)
        R["lse"][l] = torch.logsumexp(sc, -1).detach()
        o = hold((F.softmax(sc, -1) @ v_).transpose(1, 2).reshape(M, D))
        xm = hold(xin + F.linear(o, dd(L["proj_w"]), dd(L["proj_b"])))
        ln2 = hold(F.layer_norm(xm, (D,), dd(L["ln2_w"]), dd(L["ln2_b"]), VP.BLOCK_EPS))
        R["st2"][l] = torch.stack([xm.mean(1), 1 / torch.sqrt(xm.var(1, unbiased=False) + VP.BLOCK_EPS)]).detach()
        pre = hold(F.linear(ln2, dd(L["fc1_w"]), dd(L["fc1_b"])))
        pl = pre.detach().clone().requires_grad_(True)
        F.gelu(pl).sum().backward()
        R["hpre"][l] = pl.grad
        res = hold(xm.clone())                                                                 # the residual path of x_mid, on its own node
        xo = res + F.linear(F.gelu(pre), dd(L["fc2_w"]), dd(L["fc2_b"]))
        a_pre = a_in = None
        if c["adapter_dim"]:
            ad = [leaf(t) for t in L["adapter"]]
            T["ad"].append(ad)
            a_in = hold(xm.clone())
            a_pre = hold(F.linear(a_in, ad[0], ad[1]))
            hdn = F.relu(a_pre)
            if c["p"] > 0:
                hdn = hdn * X["mask"][l].double() / (1 - c["p"])
            R["ad_hd"][l] = hdn.detach()
            xo = xo + VP.ADAPTER_SCALE * F.linear(hdn, ad[2], ad[3])
        x.append(hold(xo))
        nodes.append(dict(h1=h1, qkv=qkv, o=o, xm=xm, ln2=ln2, pre=pre, res=res, a_in=a_in, a_pre=a_pre))
        R["h1"][l] = h1.detach() if (c["lora_rank"] or c["sd"] or gram0 is not None) else None
        R["qkv"][l], R["attn_o"][l], R["x_mid"][l] = qkv.detach(), o.detach(), xm.detach()
    y = F.layer_norm(x[depth].reshape(B, N, D), (D,), dd(P["norm_w"]), dd(P["norm_b"]), 1e-6)
    feat = y[:, :Pp].mean(1)
    feat.backward(dd(X["dfeat"]))
    R["x"], R["feat"] = [t.detach() for t in x], feat.detach()
    R["gram0"] = gram0
    R["gram"] = None if gram0 is None else torch.stack([gram0[l].double() + nodes[l]["h1"].detach().T @ nodes[l]["h1"].detach() for l in range(depth)])
    lowest = VP.lowest_layer(c, n_prompt)
    R["lowest"] = lowest
    tap = {(-1, "g0"): x[depth].grad}
    for l in range(depth - 1, lowest - 1, -1):
        n = nodes[l]
        tap[(l, "dbig")], tap[(l, "dfc1")], tap[(l, "g_ln2")] = n["pre"].grad, n["ln2"].grad, n["xm"].grad
        tap[(l, "dproj")], tap[(l, "dqkv")] = n["o"].grad, n["qkv"].grad
        if c["adapter_dim"]:
            tap[(l, "ad_dh")], tap[(l, "ad_gx")] = n["a_pre"].grad, n["res"].grad + n["a_in"].grad
        if l == lowest and not w["dprompt"]:
            break
        tap[(l, "dqin")], tap[(l, "g_ln1")] = n["h1"].grad, x[l].grad
    R["tap"] = tap
    R["d_lora_b0"] = [(torch.zeros(D, VP.LORA_RANK, dtype=torch.float64),) * 2] * depth
    R["d_lora_b"] = [tuple(t.grad for t in T["lora"][l][1::2]) if w["lora"] else None for l in range(depth)]
    R["d_ab"] = [tuple(t.grad for t in T["lora"][l]) if w["ab"] else None for l in range(depth)]
    R["d_adapter"] = [tuple(t.grad for t in T["ad"][l]) if w["adapter"] else None for l in range(depth)]
    R["d_sd"] = [tuple(t.grad for t in T["sd"][l]) if w["sd"] else None for l in range(depth)]
    R["dpk"] = [T["pk"][l].grad if (w["prefix"] and T["pk"][l] is not None and l >= lowest) else None for l in range(depth)]
    R["dpv"] = [T["pv"][l].grad if (w["prefix"] and T["pv"][l] is not None and l >= lowest) else None for l in range(depth)]
    R["dprompt"] = prompt.grad if w["dprompt"] else None
    if w["sd"]:
        R["d_mag"] = T["mag"].grad
    return R


@pytest.mark.parametrize("case", VP.CASES, ids=VP.case_id)
def test_exact_chain(case):
    c, P = _setup(*case)
    for i, (B, npr) in enumerate(VP.batches_of(c["mode"])):
        X = VP.step_inputs(c, B, npr, 77, None)
        R = autograd_step(c, P, X, _gram0(c, i == 1 or len(VP.batches_of(c["mode"])) == 1))
        if c["sd"]:                                        # the per-layer rows are the executor's scratch: the exact chain only has their sum
            rows = VP.emulate(c, P, X, None)["d_mag_rows"]
            assert float((rows.sum(0) - R["d_mag"]).abs().max()) <= 1e-12 * float(R["d_mag"].abs().max())
            R["d_mag_rows"] = rows
        V = VP.judge(c, P, R)
        bad = {k: v for k, v in V.rel.items() if not v <= 1e-12}
        assert not bad, bad
        assert not [k for k in V if "written" in k[1]]
        assert len(V) >= 20 * c["depth"]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", VP.CASES, ids=VP.case_id)
def test_honest_chain(case, dt):
    c, P = _setup(*case)
    old = None
    for i, (B, npr) in enumerate(VP.batches_of(c["mode"])):
        X = VP.step_inputs(c, B, npr, 77, dt)
        R = VP.emulate(c, P, X, dt, gram0=_gram0(c, i == 1), grads0=old)
        V = VP.judge(c, P, R)
        print(f"[ratio] {VP.case_id(case)} b{B} {dt} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(V.worst_by_link().items())))
        V.check(VP.case_id(case))
        old = dict(d_lora_b=R["d_lora_b"]) if c["lora_rank"] else None          # the second step accumulates onto the first one's lora_B gradients


# the link each fault belongs to, at layer FAULT_LAYER of the t64 case of its mode
EXPECT = dict(stale_h1={"d_lora_b k", "d_lora_b v"}, ln1_st2={"g_ln1"}, lost_plus={"g_ln2"}, swap_twice={"g_ln2"}, dqkv_late={"d_lora_b k", "d_lora_b v"},
              ad_wgrad_post_swap={"d_adapter dWu", "d_adapter dbu"}, gram_from_ln2={"gram"})


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("fault", VP.FAULTS)
def test_seeded_fault_is_caught_at_its_link(fault, dt):
    c, P = _setup("t64", VP.FAULT_MODE[fault])
    B, npr = (3, 0) if fault == "break_high" else (5, 4)
    X = VP.step_inputs(c, B, npr, 77, dt)
    V = VP.judge(c, P, VP.emulate(c, P, X, dt, fault=fault, gram0=_gram0(c, True)))
    over = {k: v for k, v in V.items() if not v <= 1.0}
    print(f"[fault] {fault} {dt}: " + ", ".join(f"layer {k[0]} {k[1]} {v:.3g}" for k, v in sorted(over.items())))
    if fault == "break_high":                              # the lowest layer's launches never ran (nor the qkv dgrad and LN1 backward above it): slots untouched
        low = VP.lowest_layer(c, npr)
        assert over and all(k[1].endswith("not written") and (k[0] == low or (k[0] == low + 1 and k[1][:4] in ("dqin", "g_ln"))) for k in over), over
        assert {k[1] for k in over if k[0] == low} >= {"dbig not written", "dqkv not written"}
    else:
        assert set(over) == {(VP.FAULT_LAYER, k) for k in EXPECT[fault]}, over           # its own link(s), and no link upstream or downstream of it
        assert all(v > 2.0 for v in over.values()), over
    with pytest.raises(AssertionError, match=r"unit \d+ \w+"):
        V.check(fault)


@pytest.mark.parametrize("geo,mode,B,npr,lowest", [("t64", "prefix", 3, 0, 1), ("t64", "prefix_prompt", 5, 4, 0), ("t64", "lora", 3, 0, 0), ("d1", "prefix", 3, 0, 0),
                                                   ("d1", "lora", 5, 4, 0), ("t64", "adapter", 5, 4, 0), ("t64", "lora_ab", 3, 0, 0)])
def test_tap_slot_map_and_written_rule(geo, mode, B, npr, lowest):
    c, P = _setup(geo, mode)
    assert VP.lowest_layer(c, npr) == lowest
    R = VP.emulate(c, P, VP.step_inputs(c, B, npr, 77, "f32"), "f32")
    assert set(R["tap"]) == VP.written_slots(c, npr)
    M, D, Rr = R["M"], c["dim"], c["adapter_dim"]
    tm, total = VP.tap_map(c, M)
    stride = M * (c["mlp"] + 8 * D) + (M * (Rr + D) if Rr else 0)               # include/clhip.h, clhip_vit_set_tap
    assert total == M * D + c["depth"] * stride
    spans = sorted((o, o + n) for o, n, _ in tm.values())
    assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    for k, t in R["tap"].items():
        assert t.numel() == tm[k][1] and t.shape[1] == tm[k][2], k
    for l in range(c["depth"]):
        assert tm[(l, "dbig")][0] == M * D + l * stride


def test_workspace_totals_are_the_recorded_ones():
    """clhip_vit_workspace_bytes is host code: every (case, type, batch, prompt tokens, flags) of the tests gives the total recorded before the read access and
    the tap were added (tests/golden/vit_ws_totals.json); they cost no workspace"""
    import ctypes as C

    from libcontinual_amd import _lib
    lib = _lib.lib()
    seen = 0
    for geo, mode in VP.CASES:
        c = VP.mode_cfg(geo, mode)
        for dt, code in (("bf16", _lib.BF16), ("f32", _lib.F32)):
            desc = _lib.VitDesc(c["img"], c["patch"], c["dim"], c["depth"], c["heads"], c["mlp"], c["lora_rank"], VP.BLOCK_EPS, c["adapter_dim"], VP.ADAPTER_SCALE)
            h = lib.clhip_vit_create(C.byref(desc), code)
            assert h
            if c["sd"]:                                    # (the pointers are only stored)
                dummy = (C.c_char * 64)()
                assert lib.clhip_vit_set_sdlora(h, len(VP.SD_RANKS), (C.c_int * len(VP.SD_RANKS))(*VP.SD_RANKS), dummy, dummy, dummy) == 0
            for B, npr in VP.batches_of(mode):
                for flags in (1, 2, 3):
                    key = f"{geo}-{mode}-{dt}-b{B}-p{npr}-f{flags}"
                    assert lib.clhip_vit_workspace_bytes(h, B, npr, flags) == VP.WS_TOTALS[key]
                    if mode == "lora_ab":                  # the layout depends on the descriptor alone, and that is the LoRA case's
                        assert VP.WS_TOTALS[key] == VP.WS_TOTALS[key.replace("lora_ab", "lora")]
                    seen += 1
            assert lib.clhip_vit_tap_floats(h) == 0        # no saved forward yet
            lib.clhip_vit_destroy(h)
    assert seen == len(VP.WS_TOTALS)
