"""csrc/ca.hip against fp64 numpy: clhip_class_moments and clhip_ca_sample.

Widths: 24 (below one tile), 130 (ragged, and a pitch that is no multiple of 4: the element-load path), 768 (the production width: 6 tiles a side).
Moments: three classes of 2, 21 and 48 rows -- the smallest legal class, a count that is no multiple of the K block of 16, and one that is.
Sampler: 5 and 256 rows per class (one ragged row tile, two full ones), 3 classes, a shuffle across the classes, class_lo = 7, unequal scales.
Bounds are derived (tests/ca_ref.py mean_bound / cov_bound / sample_bound, on ranpac_ref.chain_bound), never fitted; every test prints its largest
error-to-bound ratio.
"""
import numpy as np
import pytest
import torch

import ca_ref as CA
from oracle import detrand

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DS = (24, 130, 768)
COUNTS = (2, 21, 48)


def _ops():
    from libcontinual_amd import ops
    return ops


def _ratio(got, ref, bound):
    err = np.abs(got.double().cpu().numpy() - ref)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max())


def _rows(d):
    """rows of the three classes back to back: class centres of spread 0.5 plus unit-range noise"""
    n = sum(COUNTS)
    centre = np.repeat(0.5 * detrand.uniform(f"ca/k/centre/{d}", (len(COUNTS), d)), COUNTS, axis=0)
    return (centre + detrand.uniform(f"ca/k/rows/{d}", (n, d))).astype(np.float32)


def _offsets():
    return torch.tensor(np.concatenate([[0], np.cumsum(COUNTS)]), dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("d", DS)
def test_class_moments(d):
    ops = _ops()
    x = _rows(d)
    labels = np.repeat(np.arange(len(COUNTS)), COUNTS)
    ref_mean, ref_cov = CA.moments(x, labels, 0, len(COUNTS), eps=1e-4)
    F = torch.from_numpy(x).to(DEV)
    mean, cov = ops.class_moments(F, _offsets(), 1e-4)
    assert mean.shape == (3, d) and cov.shape == (3, d, d) and mean.dtype == cov.dtype == torch.float32
    worst_m = worst_c = 0.0
    lo = 0
    for c, n in enumerate(COUNTS):
        xc = x[lo:lo + n]
        lo += n
        worst_m = max(worst_m, _ratio(mean[c], ref_mean[c], CA.mean_bound(xc)))
        worst_c = max(worst_c, _ratio(cov[c], ref_cov[c], CA.cov_bound(xc)))
        assert torch.equal(cov[c], cov[c].T)                          # bit for bit
        assert float(cov[c].diagonal().min()) >= 1e-4 * (1 - 2 ** -20)
    print(f"clhip_class_moments D={d}: largest error / bound, mean {worst_m:.4f}, covariance {worst_c:.4f}")
    assert worst_m <= 1.0 and worst_c <= 1.0, (d, worst_m, worst_c)
    mean2, cov2 = ops.class_moments(F, _offsets(), 1e-4)
    assert torch.equal(mean, mean2) and torch.equal(cov, cov2)        # a repeated run is bit-identical


def test_class_moments_unaligned_base_takes_the_element_path():
    """a pitch that is a multiple of 4 behind a base pointer that is not 16-byte aligned: same bits as the aligned call"""
    ops = _ops()
    d = 24
    F = torch.from_numpy(_rows(d)).to(DEV)
    Fo = torch.empty(F.numel() + 1, device=DEV)
    Fo[1:].copy_(F.reshape(-1))
    Fv = Fo[1:].view(F.shape)
    assert Fv.data_ptr() % 16 == 4 and Fv.is_contiguous()
    m0, c0 = ops.class_moments(F, _offsets(), 1e-4)
    m1, c1 = ops.class_moments(Fv, _offsets(), 1e-4)
    assert torch.equal(m0, m1) and torch.equal(c0, c1)


@pytest.mark.parametrize("offs", [(0, 2, 3, 71), (0, 30, 21, 71), (0, 2, 23, 70), (1, 3, 24, 71)])
def test_class_moments_rejects_bad_offsets(offs):
    """a class of one row, offsets that go back, offsets that do not end at N or do not start at 0: CLHIP_EINVAL, outputs untouched, device usable"""
    from libcontinual_amd import _lib
    ops = _ops()
    d = 24
    F = torch.from_numpy(_rows(d)).to(DEV)
    o = torch.tensor(offs, dtype=torch.int32, device=DEV)
    mean, cov = torch.full((3, d), 7.0, device=DEV), torch.full((3, d, d), 7.0, device=DEV)
    rc = _lib.lib().clhip_class_moments(F.data_ptr(), o.data_ptr(), mean.data_ptr(), cov.data_ptr(), F.shape[0], d, 3, 1e-4,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and b"invalid argument" in _lib.lib().clhip_last_error()
    assert bool((mean == 7.0).all()) and bool((cov == 7.0).all())
    with pytest.raises(_lib.ClhipError):
        ops.class_moments(F, o, 1e-4)
    m, _ = ops.class_moments(F, _offsets(), 1e-4)                     # the next legal call works
    assert bool(torch.isfinite(m).all())


def _sampler_inputs(d, s, c=3):
    mean = detrand.uniform(f"ca/k/mean/{d}", (c, d))
    scale = np.asarray([0.9, 0.95, 1.0], np.float32)[:c]
    chol = np.tril(0.2 * detrand.uniform(f"ca/k/chol/{d}", (c, d, d)))
    idx = np.arange(d)
    chol[:, idx, idx] = 0.5 + np.abs(chol[:, idx, idx])
    z = CA._gauss(f"ca/k/z/{d}/{s}", (c * s, d))
    dest = np.argsort(detrand.uniform(f"ca/k/dest/{d}/{s}", (c * s,)), kind="stable").astype(np.int64)
    return mean, scale, chol.astype(np.float32), z, dest


@pytest.mark.parametrize("s", [5, 256])
@pytest.mark.parametrize("d", DS)
def test_ca_sample(d, s):
    ops = _ops()
    mean, scale, chol, z, dest = _sampler_inputs(d, s)
    c = mean.shape[0]
    assert not np.array_equal(dest, np.arange(c * s)) and len({int(v) // s for v in dest[:s]}) > 1      # the shuffle crosses the classes
    dev = lambda a: torch.from_numpy(a).to(DEV)
    X, labels = ops.ca_sample(dev(mean), dev(scale), dev(chol), dev(z), dev(dest), 7)
    assert X.shape == (c * s, d) and X.dtype == torch.float32 and labels.dtype == torch.int64
    worst = 0.0
    for k in range(c):
        zk = z[k * s:(k + 1) * s]
        ref = scale[k].astype(np.float64) * mean[k].astype(np.float64) + zk.astype(np.float64) @ np.tril(chol[k]).astype(np.float64).T
        worst = max(worst, _ratio(X[dev(dest[k * s:(k + 1) * s])], ref, CA.sample_bound(mean[k], scale[k].astype(np.float64), chol[k], zk)))
        assert bool((labels[dev(dest[k * s:(k + 1) * s])] == 7 + k).all())   # labels land on the permuted rows
    print(f"clhip_ca_sample D={d} S={s}: largest error / bound {worst:.4f}")
    assert worst <= 1.0, (d, s, worst)
    # the strict upper triangle of chol is never read: NaN there changes no bit
    poisoned = chol.copy()
    poisoned[:, np.triu_indices(d, 1)[0], np.triu_indices(d, 1)[1]] = np.nan
    X2, labels2 = ops.ca_sample(dev(mean), dev(scale), dev(poisoned), dev(z), dev(dest), 7)
    assert torch.equal(X, X2) and torch.equal(labels, labels2)


def test_ca_sample_rejects_a_repeated_destination():
    from libcontinual_amd import _lib
    ops = _ops()
    d, s = 24, 5
    mean, scale, chol, z, dest = _sampler_inputs(d, s)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    for bad in (np.where(np.arange(15) == 3, dest[4], dest), np.where(np.arange(15) == 0, 15, dest), np.where(np.arange(15) == 0, -1, dest)):
        X, labels = torch.full((15, d), 7.0, device=DEV), torch.zeros(15, dtype=torch.int64, device=DEV)
        keep = (dev(mean), dev(scale), dev(chol), dev(z), dev(bad.astype(np.int64)))
        rc = _lib.lib().clhip_ca_sample(*[t.data_ptr() for t in keep], X.data_ptr(), labels.data_ptr(), 3, s, d, 7, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == -1 and b"permutation" in _lib.lib().clhip_last_error(), (rc, bad)
        assert bool((X == 7.0).all())
    with pytest.raises(_lib.ClhipError):
        ops.ca_sample(dev(mean), dev(scale), dev(chol), dev(z), dev(np.zeros(15, np.int64)), 0)
    X, _ = ops.ca_sample(dev(mean), dev(scale), dev(chol), dev(z), dev(dest), 0)       # the next legal call works
    assert bool(torch.isfinite(X).all())
