"""CPU: the references of tests/elem_ref.py against torch itself -- the bit-level dynamic-threshold quantile within 2 ulp of
torch.quantile on every input the GPU test uses (1 ulp is what a lerp contracted to an FMA can differ by, 2 is the margin), and
the embedding references against torch's own fp32 expressions."""
import math

import numpy as np
import pytest
import torch

import elem_ref as R
from gpu_util import rnd


@pytest.mark.parametrize("C,L,Cp", R.DYN_SHAPES)
def test_quantile_reference_within_2ulp_of_torch_quantile(C, L, Cp):
    x, pred = R.dyn_inputs(C, L, Cp)
    qs = R.DYN_QS + ([R.Q_INTEGRAL] if C * L == 2052 else [])
    worst = 0.0
    for q in qs:
        for cs, co in R.DYN_COEF:
            for b in range(4):
                v = R.magnitudes(x[b], pred[b], cs, co)
                got = float(R.quantile_lerp(v, q))
                want = torch.quantile(torch.from_numpy(v), torch.tensor(q, dtype=torch.float32)).item()
                ulp = float(np.spacing(np.float32(abs(want)))) if want else float(np.spacing(np.float32(0)))
                worst = max(worst, abs(got - want) / ulp)
                assert abs(got - want) <= 2 * ulp, (q, cs, co, b, got, want)
    print(f"\nDYNREF N={C * L} worst |ref - torch.quantile| = {worst:.2f} ulp")


def test_quantile_reference_edges():
    # the rank chosen to be integral is integral in fp32, so floor == ceil and the result is an order statistic itself
    rank = np.float32(R.Q_INTEGRAL) * np.float32(2051)
    assert rank == np.float32(1000.0)
    v = np.arange(2052, dtype=np.float32)[::-1].copy()
    assert R.quantile_lerp(v, R.Q_INTEGRAL) == np.float32(1000.0) and R.quantile_lerp(v, 1.0) == np.float32(2051.0)
    # the inputs are what their names say: a floor at exactly 1, heavy ties, all-equal values
    x, pred = R.dyn_inputs(22, 32, 32)
    for cs, co in R.DYN_COEF:
        assert float(R.magnitudes(x[1], pred[1], cs, co).max()) < 1.0
        assert float(R.dyn_scale_ref(x, pred, cs, co, 1.0)[1]) == 1.0
    ties = R.magnitudes(x[2], pred[2], 0.5, 0.25)
    assert np.unique(ties).size < ties.size // 4
    assert np.unique(R.magnitudes(x[3], pred[3], 0.31, 0.095)).size == 1
    s = R.dyn_scale_ref(x, pred, [c[0] for c in R.DYN_COEF], [c[1] for c in R.DYN_COEF], 0.9)
    assert s.dtype == torch.float32 and s.shape == (4,) and float(s[0]) > 1.0 and float(s[3]) == 2.5
    # q near 0 at the smallest N interpolates between the two smallest values
    assert R.quantile_lerp(np.array([4.0, 1.0, 3.0, 2.0], dtype=np.float32), 0.001) == np.float32(1.0) + np.float32(np.float32(0.001) * np.float32(3.0))


def test_embedding_references_agree_with_torch_fp32():
    seq, w, b = rnd(3, 12, seed=1), rnd(32, seed=2), rnd(32, seed=3)
    f = R.inv_freq(64)
    assert f.shape == (32,) and float(f[0]) == 1.0
    both = R.cond_embed_ref(seq, w, b, f, 64, False)
    h = seq.view(3, 12, 1) * w + b
    assert (both[:, :, :32] - torch.nn.functional.gelu(h).double()).abs().max() < 1e-6
    ang = torch.arange(12).float().view(12, 1) * f
    assert (both[0, :, 32:64] - ang.sin().double()).abs().max() < 1e-6 and (both[0, :, 64:] - ang.cos().double()).abs().max() < 1e-6
    add = R.cond_embed_ref(seq, w, b, f, 64, True)
    assert add.shape == (3, 12, 32) and torch.equal(add, both[:, :, :32] + both[:, :, 32:64])
    t, tw = torch.linspace(-1.7, 0.55, 7), rnd(32, seed=5)
    te = R.time_embed_ref(t, tw, 80)
    fr = t.view(7, 1) * tw.view(1, 32) * 2 * math.pi
    assert (te[:, 1:33] - fr.sin().double()).abs().max() < 2e-6 and (te[:, 33:65] - fr.cos().double()).abs().max() < 2e-6
    assert torch.equal(te[:, 0], t.double()) and float(te[:, 65:].abs().max()) == 0.0
