"""CPU checks of the L2+LAB oracle (tests/_oracles_l2lab.py): the conditions
the GPU tests of tests/test_gpu_ncc_l2lab.py rely on."""

import pytest
import torch

import _oracles as O
import _oracles_l2lab as L
from dsin_amd.ops import reference as ref


@pytest.mark.parametrize("case", L.L2_CPU_CASES, ids=str)
def test_l2lab_cases_are_decided(case):
    """At least 90% of the patches of every case are decided on the CPU's
    bf16 operands (rgb_to_lab_ref rounded), so the exact-agreement GPU test
    is not vacuous."""
    d = L.l2_cpu_reference(*case)
    share = float(d["decided"].double().mean())
    print(f"l2lab {case}: e32 {d['e32']:.3e} decided "
          f"{int(d['decided'].sum())}/{d['decided'].numel()}")
    assert share >= 0.9


def test_lab64_matches_rgb_to_lab_ref():
    """The fp64 LAB helper is rgb_to_lab_ref to fp32 accuracy. Both
    piecewise functions are continuous, so a value that the two precisions
    put on different sides of a threshold moves nothing. The fp32 path
    rounds the linear RGB (up to 7.7e5 at 300), then X, Y, Z, the cube roots
    (up to 92) and the products with 116, 500 and 200; the largest
    intermediate is 500*92, and each of fewer than 16 roundings moves the
    result by at most one unit roundoff of that."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 16, 24, generator=g) * 255
    x[:, 0, :6] = torch.tensor([0.0, 0.04045, -3.0, 255.0, 300.0, 1e-3])
    want = ref.rgb_to_lab_ref(x)
    got = L.lab64(x)
    assert got.dtype == torch.float64 and got.shape == want.shape
    err = float((got - want.double()).abs().max())
    print(f"lab64 vs rgb_to_lab_ref: max err {err:.3e}")
    assert err <= 16 * O.U32 * 500 * 92


@pytest.mark.parametrize("case", L.L2_CPU_CASES, ids=str)
def test_l2lab_oracle_argmin_is_ncc_search_ref(case):
    """The oracle's argmin equals ncc_search_ref(l2lab=True) on decided
    patches. The CPU path keeps its LAB operands in fp32, so the oracle is
    given those same unrounded operands here: then only the fp32 arithmetic
    of the CPU path separates the two, which is what b allows for."""
    h, w, ph, pw, use_mask, noise = case
    x, y_dec, y_orig = L.lab_case(h, w, ph, pw, noise)
    d = L.l2_decide(ref.rgb_to_lab_ref(x), ref.rgb_to_lab_ref(y_dec), ph, pw,
                    use_mask)
    y_syn, rows, cols = ref.ncc_search_ref(x, y_dec, y_orig, ph, pw, use_mask,
                                           l2lab=True)
    L.l2_check(d, rows, cols, f"cpu fp32 {case}")
    # and how often the bf16 rounding of the operands moves the winner
    b = L.l2_cpu_reference(*case)
    same = (rows == b["rows"]) & (cols == b["cols"])
    print(f"l2lab {case}: bf16-operand argmin equals the fp32 path's on "
          f"{int(same.sum())}/{same.numel()} patches")
