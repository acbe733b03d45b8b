"""The ImageNet stem on the MI355X (csrc/stem7.hip, the CLHIP_UNIT_MAXPOOL unit of csrc/plan.hip): the 7x7 / s2 convolution, its weight gradient
and the fused BatchNorm + ReLU + max-pool kernels against fp64 torch, then ResNet-18/34 with both ImageNet stems against the fp64 restatement of
tests/imagenet_stem_common.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import libcontinual_amd.model as M                     # noqa: E402
from libcontinual_amd import _lib                      # noqa: E402
from libcontinual_amd._lib import call                 # noqa: E402

import imagenet_stem_common as C                       # noqa: E402

DEV = "cuda"
DT = {"bf16": (_lib.BF16, torch.bfloat16), "f32": (_lib.F32, torch.float32)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rb(t, dtype):
    return t.to(torch.bfloat16).double() if dtype == "bf16" else t.double()


def _nhwc8(x, tdt):
    N, Cc, H, W = x.shape
    y = torch.zeros(N, H, W, 8, dtype=torch.float32)
    y[..., :Cc] = x.permute(0, 2, 3, 1)
    return y.to(tdt).to(DEV).contiguous()


def _w7(w, tdt):
    K = w.shape[0]
    y = torch.zeros(K, 7, 7, 8, dtype=torch.float32)
    y[..., :3] = w.permute(0, 2, 3, 1)
    return y.to(tdt).to(DEV).contiguous()


def _relmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("N,H", [(1, 224), (3, 57), (10, 64)])
def test_stem7_forward_and_bn_sums(dtype, N, H):
    code, tdt = DT[dtype]
    K = 64
    x = C.det_images(f"s7f/x/{N}/{H}", N, H)
    w = torch.from_numpy(np.asarray(C.detrand.uniform(f"s7f/w/{N}/{H}", (K, 3, 7, 7), -0.1, 0.1)))
    Ho = (H - 1) // 2 + 1
    z = torch.empty(N, Ho, Ho, K, dtype=tdt, device=DEV)
    rep = 4
    acc = torch.zeros(rep * 2 * K, dtype=torch.float64, device=DEV)
    xd, wd = _nhwc8(x, tdt), _w7(w, tdt)                 # (held: a temporary's memory could be reused before the launch reads it)
    call("clhip_conv_fwd_acc", xd.data_ptr(), wd.data_ptr(), z.data_ptr(), acc.data_ptr(), rep, N, H, H, 8, K, 7, 2, 3, code, _stream())
    ref = F.conv2d(_rb(x, dtype), _rb(w, dtype), stride=2, padding=3).permute(0, 2, 3, 1)
    tol = 2.0 ** -7 if dtype == "bf16" else 1e-5
    assert _relmax(z.cpu(), ref) <= tol
    s = acc.view(rep, 2, K).sum(0).cpu()
    r1, r2 = ref.reshape(-1, K).sum(0), (ref.reshape(-1, K) ** 2).sum(0)
    assert float((s[0] - r1).abs().max()) <= 1e-4 * float(ref.abs().sum(dim=(0, 1, 2)).max())
    assert float(((s[1] - r2).abs() / r2).max()) <= (1e-3 if dtype == "bf16" else 1e-5)
    # the no-statistics form (eval) gives the same z
    z2 = torch.empty_like(z)
    call("clhip_conv_fwd", xd.data_ptr(), wd.data_ptr(), z2.data_ptr(), None, N, H, H, 8, K, 7, 2, 3, code, _stream())
    assert torch.equal(z, z2)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("N,H", [(1, 224), (3, 57), (10, 64)])
def test_stem7_weight_gradient_deterministic(dtype, N, H):
    code, tdt = DT[dtype]
    K = 64
    Ho = (H - 1) // 2 + 1
    x = C.det_images(f"s7w/x/{N}/{H}", N, H)
    dz = torch.from_numpy(np.asarray(C.detrand.uniform(f"s7w/dz/{N}/{H}", (N, Ho, Ho, K), -1.0, 1.0)))
    L = _lib.lib()
    wsb = int(L.clhip_conv_wgrad_ws_bytes(N, H, H, 8, 3, K, 7, 2, 3, code))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    xd, dzd = _nhwc8(x, tdt), dz.to(tdt).to(DEV).contiguous()
    outs = []
    for _ in range(2):
        dw = torch.zeros(K * 49 * 3, dtype=torch.float32, device=DEV)
        call("clhip_conv_wgrad", xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, H, H, 8, 3, K, 7, 2, 3, code, _stream())
        outs.append(dw.cpu())
    assert torch.equal(outs[0], outs[1])                 # partial blocks + fixed-order reduce: bit-reproducible
    ref = torch.nn.grad.conv2d_weight(_rb(x, dtype), (K, 3, 7, 7), _rb(dz, dtype).permute(0, 3, 1, 2), stride=2, padding=3)
    got = outs[0].view(K, 7, 7, 3).permute(0, 3, 1, 2)
    assert _relmax(got, ref) <= (2.0 ** -7 if dtype == "bf16" else 1e-5)
    # 7x7 stays illegal for a wider input and for the input gradient
    dx = torch.zeros(N, H, H, 16, dtype=tdt, device=DEV)
    with pytest.raises(_lib.ClhipError):
        call("clhip_conv_dgrad", dzd.data_ptr(), xd.data_ptr(), dx.data_ptr(), 0, N, H, H, 16, K, 7, 2, 3, code, _stream())


def _pool_case(N, H, Cc, ties, tag):
    if ties:      # few levels: equal z -> bit-equal BN outputs, so windows hold exact ties (zeros after the ReLU among them)
        z = torch.from_numpy(np.asarray(C.detrand.randint(tag, (N, H, H, Cc), -2, 3))).float()
    else:
        z = torch.from_numpy(np.asarray(C.detrand.uniform(tag, (N, H, H, Cc), -3.0, 3.0)))
    gamma = torch.from_numpy(np.asarray(C.detrand.uniform(tag + "/g", (Cc,), 0.5, 1.5)))
    beta = torch.from_numpy(np.asarray(C.detrand.uniform(tag + "/b", (Cc,), -0.2, 0.2)))
    if ties:
        gamma, beta = torch.ones(Cc), torch.zeros(Cc)
    return z, gamma, beta


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("H,ties", [(112, False), (57, False), (57, True), (112, True)])
def test_bn_relu_maxpool_forward_backward(dtype, H, ties):
    code, tdt = DT[dtype]
    N, Cc = 2, 64
    z, gamma, beta = _pool_case(N, H, Cc, ties, f"pool/{H}/{int(ties)}")
    zq = _rb(z, dtype)                                    # what the kernel reads
    Hp = int(_lib.lib().clhip_maxpool_out_dim(H))
    assert Hp == (H - 1) // 2 + 1
    zd = zq.to(tdt).to(DEV).contiguous()
    acc = torch.zeros(2 * Cc, dtype=torch.float64)
    acc[:Cc], acc[Cc:] = zq.reshape(-1, Cc).sum(0), (zq.reshape(-1, Cc) ** 2).sum(0)
    acc = acc.to(DEV)
    g_, b_ = gamma.float().to(DEV), beta.float().to(DEV)
    rm, rv = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
    mean, invstd = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
    y = torch.empty(N, Hp, Hp, Cc, dtype=tdt, device=DEV)
    am = torch.empty(N, Hp, Hp, Cc, dtype=torch.uint8, device=DEV)
    call("clhip_bn_relu_maxpool_fwd", zd.data_ptr(), acc.data_ptr(), 1, g_.data_ptr(), b_.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5,
         mean.data_ptr(), invstd.data_ptr(), y.data_ptr(), am.data_ptr(), N, H, H, Cc, 1, code, _stream())
    # fp64 reference on the same (rounded) z
    zc = zq.permute(0, 3, 1, 2).clone()
    m64 = zc.mean(dim=(0, 2, 3))
    v64 = zc.var(dim=(0, 2, 3), unbiased=False)
    h = ((zc - m64.view(1, -1, 1, 1)) / torch.sqrt(v64.view(1, -1, 1, 1) + 1e-5) * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1))
    h.requires_grad_(True)
    yr, idx = F.max_pool2d(F.relu(h), 3, 2, 1, return_indices=True)
    assert _relmax(y.cpu().permute(0, 3, 1, 2), yr.detach()) <= (2.0 ** -7 if dtype == "bf16" else 1e-5)
    # window position of torch's argmax
    hp = torch.arange(Hp).view(1, 1, -1, 1)
    ky, kx = idx // H - (2 * hp - 1), idx % H - (2 * hp.transpose(2, 3) - 1)
    pos = (ky * 3 + kx).permute(0, 2, 3, 1)
    got = am.cpu().long()
    if ties or dtype == "f32":
        if ties:
            assert torch.equal(got, pos)
        else:
            assert float((got == pos).double().mean()) > 0.9999
    assert int(got.max()) <= 8
    assert torch.allclose(mean.cpu().double(), m64, atol=1e-5) and torch.allclose(rm.cpu().double(), 0.1 * m64, atol=1e-5)
    assert torch.allclose(rv.cpu().double(), 0.9 + 0.1 * v64 * (N * H * H) / (N * H * H - 1), rtol=1e-4)
    # eval form: running statistics
    ye = torch.empty_like(y)
    call("clhip_bn_relu_maxpool_fwd", zd.data_ptr(), None, 1, g_.data_ptr(), b_.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.0, 1e-5,
         None, None, ye.data_ptr(), None, N, H, H, Cc, 0, code, _stream())
    he = (zc - rm.cpu().double().view(1, -1, 1, 1)) / torch.sqrt(rv.cpu().double().view(1, -1, 1, 1) + 1e-5) * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
    assert _relmax(ye.cpu().permute(0, 3, 1, 2), F.max_pool2d(F.relu(he), 3, 2, 1)) <= (2.0 ** -7 if dtype == "bf16" else 1e-5)
    # backward: gather form, ReLU mask, BatchNorm-backward sums
    dy = torch.from_numpy(np.asarray(C.detrand.uniform(f"pool/dy/{H}/{int(ties)}", (N, Hp, Hp, Cc), -1.0, 1.0)))
    dyq = _rb(dy, dtype)
    yr.backward(dyq.permute(0, 3, 1, 2))
    gref = h.grad.permute(0, 2, 3, 1)
    g = torch.empty(N, H, H, Cc, dtype=tdt, device=DEV)
    accb = torch.zeros(2 * 2 * Cc, dtype=torch.float64, device=DEV)
    dyd = dyq.to(tdt).to(DEV).contiguous()
    outs = []
    for _ in range(2):
        accb.zero_()
        call("clhip_maxpool_bwd_bn_reduce", dyd.data_ptr(), am.data_ptr(), zd.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
             g_.data_ptr(), b_.data_ptr(), g.data_ptr(), accb.data_ptr(), 2, N, H, H, Cc, code, _stream())
        outs.append((g.cpu().clone(), accb.cpu().clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    gg = outs[0][0].double()
    if ties or dtype == "f32":
        assert _relmax(gg, gref) <= (2.0 ** -8 if dtype == "bf16" else 1e-6)
    s = outs[0][1].view(2, 2, Cc).sum(0)
    xhat = (zq - m64) / torch.sqrt(v64 + 1e-5)
    r1, r2 = gg.reshape(-1, Cc).sum(0), (gg * xhat).reshape(-1, Cc).sum(0)
    scale = float(gg.abs().reshape(-1, Cc).sum(0).max())
    assert float((s[0] - r1).abs().max()) <= 1e-5 * scale and float((s[1] - r2).abs().max()) <= 1e-4 * scale


# ------------------------------------------------------------------------------------------------------------ backbone
def _backbone(arch, stem, dtype, P, B):
    bb = getattr(M, arch)(args=C.ARGS[stem], dtype=dtype)
    sd = bb.state_dict()
    sd.update(P)
    sd.update(B)
    bb.load_state_dict(sd)
    return bb.to(DEV)


def _oracle(arch, stem, P, B, x, cw, round_stem=False):
    Pg = {k: v.double().requires_grad_(True) for k, v in P.items()}
    Bo = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in B.items()}
    out = C.forward(arch, stem, Pg, Bo, x.double(), True, round_stem)
    (out["features"] * cw.double()).sum().backward()
    return out, Pg, Bo


def _relnorm(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


CASES = [("resnet18", "imagenet7", 224), ("resnet34", "imagenet7", 224), ("resnet18", "imagenet3", 64)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch,stem,size", CASES)
def test_backbone_vs_fp64(arch, stem, size, dtype):
    """f32 at B = 4: features and fmaps <= 2e-4, gradients per layer <= 2e-2 and whole <= 1e-2 (test_parity_gpu's bar).  bf16 at B = 8, against the
    yardstick of test_backbone_vs_oracle_random_init -- the fp64 forward / backward on bf16-rounded conv weights and input -- extended by the stem's
    own storage sites: its z and pooled activation (and their gradients) rounded to bf16 as the bf16 mode stores them.  The CIFAR backbones that
    test was written for have no such full-resolution tensors in front of layer1; here they are 112 x 112 (64 x 64) maps whose rounding the plain
    yardstick does not see.  Against it: whole gradient <= 1.45 x, per-layer median <= 1.5 x, worst layer <= 1.7 x, as there; features <= 3 x the
    yardstick's own feature deviation in max norm and fmaps <= 3 x its relative L2 norm."""
    B_ = 4 if dtype == "f32" else 8
    P, Bf = C.det_state(arch, stem, "bb")
    x = C.det_images(f"bb/x/{arch}/{stem}", B_, size)
    cw = torch.from_numpy(np.asarray(C.detrand.uniform(f"bb/cw/{arch}/{stem}", (B_, 512), -1.0, 1.0)))
    ref, Pg, Bo = _oracle(arch, stem, P, Bf, x, cw)
    bb = _backbone(arch, stem, dtype, P, Bf)
    assert bb.stem == stem and bb._units[0].k == (7 if stem == "imagenet7" else 3)
    bb.train()
    out = bb(x.to(DEV))
    f = out["features"]
    (f * cw.to(DEV)).sum().backward()
    fm = out["fmaps"]
    assert [tuple(t.shape[2:]) for t in fm] == [tuple(t.shape[2:]) for t in ref["fmaps"]]
    if dtype == "f32":
        ftol = 2e-4
        for a, b in zip(fm, ref["fmaps"]):
            assert _relmax(a.cpu(), b.detach()) < 2e-4
    else:
        rb = lambda t: t.to(torch.bfloat16).float()
        yref, Py, _ = _oracle(arch, stem, {k: (rb(v) if v.dim() == 4 else v) for k, v in P.items()}, Bf, rb(x), cw, round_stem=True)
        ftol = 3 * _relmax(yref["features"].detach(), ref["features"].detach())
        for a, b, c in zip(fm, ref["fmaps"], yref["fmaps"]):
            assert _relnorm(a.cpu().double(), b.detach()) <= 3 * _relnorm(c.detach(), b.detach())
    assert _relmax(f.detach().cpu(), ref["features"].detach()) < ftol
    rels, a_all, b_all = {}, [], []
    named = dict(bb.named_parameters())
    for n in P:
        a, b = named[n].grad.cpu().double().reshape(-1), Pg[n].grad.reshape(-1)
        rels[n] = _relnorm(a, b)
        a_all.append(a)
        b_all.append(b)
    assert named["fc.weight"].grad is None
    whole = _relnorm(torch.cat(a_all), torch.cat(b_all))
    if dtype == "f32":
        assert max(rels.values()) < 2e-2 and whole < 1e-2, (max(rels.values()), whole)
    else:
        yard = {n: _relnorm(Py[n].grad.reshape(-1), Pg[n].grad.reshape(-1)) for n in rels}
        yard_whole = _relnorm(torch.cat([Py[n].grad.reshape(-1) for n in rels]), torch.cat(b_all))
        med, ymed = float(np.median(list(rels.values()))), float(np.median(list(yard.values())))
        print(f"{arch} {stem} bf16: whole {whole:.3f} / yardstick {yard_whole:.3f} = {whole / yard_whole:.3f}; median {med:.3f} / {ymed:.3f}")
        assert whole <= 1.45 * yard_whole, (whole, yard_whole)
        assert med <= 1.5 * ymed, (med, ymed)
        assert max(rels.values()) <= 1.7 * max(yard.values()), (max(rels.values()), max(yard.values()))
    # running statistics (one training forward, momentum 0.1)
    sd = bb.state_dict()
    for k, v in Bo.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            # (bf16: the batch statistics of the deep layers carry the activations' bf16 deviation, a few 1e-3 of the 0.1-weighted update)
            assert torch.allclose(sd[k].cpu().double(), v, rtol=1e-2 if dtype == "bf16" else 1e-4, atol=1e-2 if dtype == "bf16" else 1e-5), k
        elif k.endswith("num_batches_tracked"):
            assert int(sd[k]) == 1, k
    # eval-mode features (the running statistics just updated)
    bb.eval()
    with torch.no_grad():
        fe = bb(x.to(DEV))["features"]
    Be = {k: v.clone() for k, v in Bo.items()}
    fe_ref = C.forward(arch, stem, {k: v.detach() for k, v in Pg.items()}, Be, x.double(), False)["features"]
    assert _relmax(fe.cpu(), fe_ref) < ftol


def test_backbone_step_bit_reproducible():
    """two bf16 224 x 224 forward + backward passes at batch 10 on the same weights: the same bits (no atomics on any gradient of the stem)"""
    P, Bf = C.det_state("resnet18", "imagenet7", "rep")
    x = C.det_images("rep/x", 10, 224).to(DEV)
    cw = torch.from_numpy(np.asarray(C.detrand.uniform("rep/cw", (10, 512), -1.0, 1.0))).to(DEV)
    res = []
    for _ in range(2):
        bb = _backbone("resnet18", "imagenet7", "bf16", P, Bf)
        bb.train()
        f = bb(x)["features"]
        (f * cw).sum().backward()
        res.append((f.detach().cpu(), torch.cat([p.grad.reshape(-1) for n, p in bb.named_parameters() if not n.startswith("fc.")]).cpu()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_teacher_forward_matches_training_forward():
    """training = 2 (a batch-statistics forward no backward follows, ops.TeacherPass) writes no argmax and gives the training forward's features"""
    from libcontinual_amd.model.backbone.resnet import no_backward_follows
    P, Bf = C.det_state("resnet18", "imagenet7", "teacher")
    x = C.det_images("teacher/x", 4, 224).to(DEV)
    a = _backbone("resnet18", "imagenet7", "bf16", P, Bf)
    b = _backbone("resnet18", "imagenet7", "bf16", P, Bf)
    a.train()
    b.train()
    for p in b.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        fa = a(x)["features"]
        with no_backward_follows():
            fb = b(x)["features"]
    assert torch.equal(fa, fb)


def test_stem7_f32_weight_gradient_eight_real_channels():
    """Creal = 8 (49 x 8 = 392 entries per output channel, more than a workgroup's 256 threads): every entry is written in every split"""
    N, H, K = 2, 57, 32
    Ho = (H - 1) // 2 + 1
    x = torch.from_numpy(np.asarray(C.detrand.uniform("s7w8/x", (N, 8, H, H), -2.0, 2.0)))
    dz = torch.from_numpy(np.asarray(C.detrand.uniform("s7w8/dz", (N, Ho, Ho, K), -1.0, 1.0)))
    for dtype in ("f32", "bf16"):
        code, tdt = DT[dtype]
        xd = x.permute(0, 2, 3, 1).to(tdt).to(DEV).contiguous()
        dzd = dz.to(tdt).to(DEV).contiguous()
        ws = torch.full((int(_lib.lib().clhip_conv_wgrad_ws_bytes(N, H, H, 8, 8, K, 7, 2, 3, code)),), 0x7f, dtype=torch.uint8, device=DEV)   # (no zero scratch)
        dw = torch.zeros(K * 49 * 8, dtype=torch.float32, device=DEV)
        call("clhip_conv_wgrad", xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, H, H, 8, 8, K, 7, 2, 3, code, _stream())
        ref = torch.nn.grad.conv2d_weight(_rb(x, dtype), (K, 8, 7, 7), _rb(dz, dtype).permute(0, 3, 1, 2), stride=2, padding=3)
        assert _relmax(dw.cpu().view(K, 7, 7, 8).permute(0, 3, 1, 2), ref) <= (2.0 ** -7 if dtype == "bf16" else 1e-5), dtype


def test_plan_refuses_a_7x7_unit_without_the_max_pool():
    """the 7x7 / s2 unit is legal only as the max-pool stem (CLHIP_UNIT_MAXPOOL); without the bit plan creation fails"""
    L = _lib.lib()
    for bits, ok in ((1, False), (1 | 16, True)):
        d = (_lib.UnitDesc * 1)()
        d[0].cin, d[0].cout, d[0].ksize, d[0].stride, d[0].pad, d[0].src, d[0].res, d[0].relu = 3, 64, 7, 2, 3, 0, -1, bits
        d[0].w_off, d[0].gamma_off, d[0].beta_off, d[0].rm_off, d[0].rv_off = 0, 64 * 49 * 3, 64 * 49 * 3 + 64, 0, 64
        p = L.clhip_plan_create_ex(d, 1, 2, 64, 64, 3, _lib.BF16, 0)
        assert bool(p) == ok, L.clhip_last_error()
        if p:
            L.clhip_plan_destroy(p)


@pytest.mark.parametrize("stem,size", [("imagenet7", 224), ("imagenet3", 64)])
def test_backbone_golden(golden, stem, size):
    """fixture = the REFERENCE's own resnet18 in fp64 (tools/gen_imagenet_golden.py): the tolerances of test_parity_gpu.py::test_backbone_golden"""
    from oracle import fixtures as fx
    want = golden(f"backbone_resnet18_{stem}")
    P, Bf = C.det_state("resnet18", stem, "golden")
    x = C.det_images(f"golden/{stem}/x", 4, size)
    cw = torch.from_numpy(np.asarray(C.detrand.uniform(f"golden/{stem}/cw", (4, 512), -1.0, 1.0))).to(DEV)
    for dtype in ("f32", "bf16"):
        bb = _backbone("resnet18", stem, dtype, P, Bf)
        bb.train()
        f = bb(x.to(DEV))["features"]
        (f * cw).sum().backward()
        named = dict(bb.named_parameters())
        names = [str(n) for n in want["grad_names"]]
        _, rows = fx.summarize({n: named[n].grad.cpu() for n in names})
        sd = bb.state_dict()
        _, brows = fx.summarize({str(n): sd[str(n)].cpu() for n in want["buf_names"]})
        bb.eval()
        with torch.no_grad():
            fe = bb(x.to(DEV))["features"]
        if dtype == "f32":
            assert _relmax(f.detach().cpu(), torch.from_numpy(want["features_train"])) < 1e-4
            assert _relmax(fe.cpu(), torch.from_numpy(want["features_eval"])) < 1e-4
            g = named["conv1.0.weight"].grad.cpu().double()
            assert _relnorm(g, torch.from_numpy(want["grad_stem"]).double()) < 0.1
            fx.assert_summary_close(rows, want["grad_rows"], 2e-2, what="grads")
            assert _relmax(torch.from_numpy(brows[:, :3]), torch.from_numpy(want["buf_rows"][:, :3])) < 1e-4
        else:
            assert _relmax(f.detach().cpu(), torch.from_numpy(want["features_train"])) < 5e-2
            assert _relmax(fe.cpu(), torch.from_numpy(want["features_eval"])) < 2.5e-2


def test_backbone_at_a_batch_above_64_vs_fp64():
    """batch 72 (above the stage-level / fusion thresholds that depend on N) on the 64 x 64 stem, f32: the B = 4 bars"""
    P, Bf = C.det_state("resnet18", "imagenet3", "b72")
    x = C.det_images("b72/x", 72, 64)
    cw = torch.from_numpy(np.asarray(C.detrand.uniform("b72/cw", (72, 512), -1.0, 1.0)))
    ref, Pg, _ = _oracle("resnet18", "imagenet3", P, Bf, x, cw)
    bb = _backbone("resnet18", "imagenet3", "f32", P, Bf)
    bb.train()
    f = bb(x.to(DEV))["features"]
    (f * cw.to(DEV)).sum().backward()
    assert _relmax(f.detach().cpu(), ref["features"].detach()) < 2e-4
    named = dict(bb.named_parameters())
    rels = {n: _relnorm(named[n].grad.cpu().double().reshape(-1), Pg[n].grad.reshape(-1)) for n in P}
    whole = _relnorm(torch.cat([named[n].grad.cpu().double().reshape(-1) for n in P]), torch.cat([Pg[n].grad.reshape(-1) for n in P]))
    assert max(rels.values()) < 2e-2 and whole < 1e-2, (max(rels.values()), whole)


def test_a_replayed_step_is_the_same_step(monkeypatch):
    """LwF / ResNet-18 with the 7 x 7 max-pool stem, batch 10, 224 x 224 (the imagenet-r setting): eight steps of which six are HIP-graph replays
    against eight eager steps.  (WA declares itself not graph-safe and stays eager; LwF is the graph-safe method on this backbone.)  The BatchNorm
    sums are fp64 atomics, so the bar is test_graph_step_gpu's: 1e-5 of the parameters."""
    from libcontinual_amd import optim
    from libcontinual_amd import trainer as T

    def batches(n):
        out = []
        for i in range(n):
            g = torch.Generator().manual_seed(300 + i)
            out.append({"image": torch.randn(10, 3, 224, 224, generator=g).cuda(), "label": torch.randint(0, 20, (10,), generator=g).cuda()})
        return out
    out = []
    for mode in ("0", "1"):
        monkeypatch.setenv("CLHIP_CUDA_GRAPH", mode)
        torch.manual_seed(9)
        bb = M.resnet18(args=C.ARGS["imagenet7"], dtype="bf16")
        m = M.LWF(bb, 512, 200, device="cuda", init_cls_num=20, inc_cls_num=20).to("cuda")
        m.before_task(0, None, None, None)
        m.train()
        o = optim.SGD(m.get_parameters({}), lr=0.02, momentum=0.9, weight_decay=5e-4)
        T.train_steps(m, o, batches(8), None, "LWF", None, "cuda")
        torch.cuda.synchronize()
        out.append((m.backbone.flat_parameters()[0].clone(), bb._stats.clone(), getattr(m, "_graphed_step", None)))
    (p0, s0, g0), (p1, s1, g1) = out
    assert g0 is None and g1 is not None and len(g1.graphs) == 1
    assert float((p0 - p1).abs().max()) <= 1e-5 * float(p0.abs().max())
    assert float((s0 - s1).abs().max()) <= 1e-5 * float(s0.abs().max())


def test_reference_yaml_trains_end_to_end(tmp_path):
    """the reference's config/zz_WA/wa-resnet18-imagenetr-b20-20-10.yaml (verbatim: tests/golden/) through libcontinual_amd.config and the Trainer, on
    a tree of differently sized PNGs; only the scale keys are overridden (data root, 2 tasks x 4 classes x 12 images, 8 classes, a buffer of 16, one
    epoch): dataset, image size, backbone and classifier stay as shipped"""
    import os
    from PIL import Image
    from libcontinual_amd.config import Config
    from libcontinual_amd.data import transforms as TR
    from libcontinual_amd.trainer import Trainer
    root = tmp_path / "imagenet-r"
    rng = np.random.default_rng(0)
    for mode, n in (("train", 12), ("test", 4)):
        for c in range(8):
            d = root / mode / f"n{c:03d}"
            d.mkdir(parents=True)
            for k in range(n):
                h, w = int(rng.integers(180, 300)), int(rng.integers(180, 300))
                img = np.clip(rng.normal(40 + 25 * c, 30, (h, w, 3)), 0, 255).astype(np.uint8)
                Image.fromarray(img).save(d / f"{k}.png")
    cfg = Config(os.path.join(os.path.dirname(__file__), "golden", "wa-resnet18-imagenetr-b20-20-10.yaml")).get_config_dict()
    assert cfg["dataset"] == "imagenet-r" and cfg["image_size"] == 224 and cfg["backbone"]["name"] == "resnet18" and cfg["classifier"]["name"] == "WA"
    cfg.update(data_root=str(root), init_cls_num=4, inc_cls_num=4, task_num=2, total_cls_num=8, init_epoch=1, epoch=1, num_workers=0, save_path="",
               testing_times=1, seed=3)
    cfg["classifier"]["kwargs"].update(num_class=8, init_cls_num=4)
    cfg["backbone"]["kwargs"]["num_classes"] = 8
    cfg["buffer"]["kwargs"]["buffer_size"] = 16
    logs = []
    tr = Trainer(0, cfg, log=lambda *a, **k: logs.append(" ".join(map(str, a))))
    assert tr.model.backbone.stem == "imagenet7" and tr.model.backbone._units[0].k == 7
    kinds = [type(t).__name__ for t in tr.train_loader.get_loader(0).dataset.trfms.transforms]
    assert kinds == ["RandomResizedCrop", "RandomHorizontalFlip", "ColorJitter", "ToTensor", "Normalize"]
    tkinds = [type(t).__name__ for t in tr.test_loader.get_loader(0)[0].dataset.trfms.transforms]
    assert tkinds == ["Resize", "CenterCrop", "ToTensor", "Normalize"]
    assert torch.allclose(tr.train_loader.get_loader(0).dataset.trfms.transforms[-1].mean.flatten(), torch.tensor(TR.IMAGENET_R_MEAN))
    out = tr.train_loop()
    acc = out["acc_table"]
    assert acc.shape == (2, 2) and np.isfinite(acc).all()
    assert logs and not any("nan" in ln.lower() or "inf " in ln.lower() for ln in logs)       # the logged losses / accuracies are finite
    assert len(tr.buffer.labels) > 0
