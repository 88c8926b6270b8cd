"""Host: the builder of the ReLU-edge inputs (helpers.bn_mask_edge_inputs) that tests/test_bn_forward_gpu.py holds the kernels'
ReLU masks against.  It must (a) give a reference that is EXACT and (b) really sit where a multiply + add and one fma disagree:
otherwise the GPU test's bit-for-bit assertions would pass for a kernel that lost its explicit fma."""
from fractions import Fraction

import numpy as np
import pytest

from helpers import bf16_exact, bn_mask_edge_inputs, muladd32_mask


@pytest.mark.parametrize("bf16", [False, True], ids=["f32-ulps", "bf16-ulps"])
def test_edge_inputs_are_exact_and_split_fma_from_mul_add(bf16):
    d = bn_mask_edge_inputs(7, 64, 4096, bf16=bf16)
    y, sc, sh, exact = d["y"], d["sc"], d["sh"], d["exact"]
    assert y.dtype == np.float32 and y.shape == (4096, 64) and d["dz"].dtype == np.float32
    assert float(np.abs(d["dz"]).min()) >= 0.5 and float(np.abs(d["dz"]).max()) <= 1.5 and (d["dz"] < 0).any() and (d["dz"] > 0).any()
    # the float64 value is the exact one: rational arithmetic on a sample (all 7 steps of every channel are in the first rows)
    rng = np.random.default_rng(0)
    for i, j in zip(rng.integers(0, 4096, 3000), rng.integers(0, 64, 3000)):
        f = Fraction(float(y[i, j])) * Fraction(float(sc[j])) + Fraction(float(sh[j]))
        assert Fraction(float(exact[i, j])) == f, (i, j)
    # rounding the exact value to float32 (what one fma returns) keeps it clear of the subnormals, so its sign is the exact sign
    nz = np.abs(exact[exact != 0.0])
    assert float(nz.min()) > 2.0 ** -100
    assert np.array_equal(exact.astype(np.float32) > 0, d["mask"])
    # every element is y0 stepped by at most 3 ulps of its format
    y0 = (-sh.astype(np.float64) / sc.astype(np.float64)).astype(np.float32) if not bf16 else None
    if bf16:
        assert np.array_equal(bf16_exact(y), y)
        steps = (y.view(np.int32).astype(np.int64) >> 16)
        assert int((steps.max(0) - steps.min(0)).max()) <= 6
    else:
        assert int(np.abs(y.view(np.int32).astype(np.int64) - y0.view(np.int32).astype(np.int64)[None, :]).max()) <= 3
    wrong = muladd32_mask(y, sc, sh) != d["mask"]
    zeros = int((exact == 0.0).sum())
    print("%s: mul + add disagrees with the exact sign on %d of %d elements (%.2f %%), exact zeros %d, positive %.1f %%"
          % ("bf16 steps" if bf16 else "f32 steps", int(wrong.sum()), wrong.size, 100.0 * wrong.mean(), zeros, 100.0 * d["mask"].mean()))
    assert wrong.mean() >= 0.03          # measured 6.4 % (float32 steps) / 7.1 % (bfloat16 steps): the floor guards a degenerate builder
    assert 0.3 <= d["mask"].mean() <= 0.7
