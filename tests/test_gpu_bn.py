"""GPU tests of the fused batch-norm(+residual)(+activation) kernels
(csrc/bn.hip, ops/bn.py) against the fp64 oracle of tests/_oracles.py.

Inputs are generated on the CPU and rounded to bf16, the type the kernels
read; the oracle gets exactly those values. Bounds (O.bn_bounds), with e32
the max error of the unrounded fp32 CPU result:

  out, dx (bf16 stores)     2^-8*|ref| + 4*e32 + 1e-6, elementwise
  dgamma, dbeta (fp32 sums) 4*e32 + depth*2^-24*sum|t_i|, per channel
  running_mean / _var       4*e32 + momentum*depth*2^-24*(...)

depth is the longest chain of additions one summand passes through in
bn_stats_part / bn_bwd_part and the sum of the S slices (O.bn_depth): the
thread's own elements, 6 shuffle steps, 4 waves, S slices.

The kernel takes the activation gradient from the sign of the stored
output, the oracle from the fp64 pre-activation; dy is zero wherever the
pre-activation is within 1e-3 of zero (under 1% of the elements, asserted
in tests/test_oracles.py), so neither side's rounding decides a branch.

Shapes (B, C, H, W) and what they reach:
  (2, 32, 20, 24)   the baseline: S=1, no tail, aligned planes
  (3, 5, 7, 9)      HW=63: a tail of 7, odd planes not 16-byte aligned
  (2, 3, 1, 5)      HW < 8: tail only
  (2, 3, 65, 67)    HW=4355: S=2, a grid-stride second pass, a tail of 3
  (1, 2, 220, 300)  HW=66000: S=32
  (2, 8, 20, 24)    input mean shifted by 8 standard deviations
"""

import pytest
import torch

import _oracles as O
from dsin_amd.ops.bn import batch_norm_act

pytestmark = pytest.mark.gpu

_IDS, _CASES = O.bn_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run_gpu(case, dev):
    c = case["x"].shape[1]
    bn = torch.nn.BatchNorm2d(c, eps=case["eps"],
                              momentum=case["momentum"]).to(dev)
    with torch.no_grad():
        bn.weight.copy_(case["gamma"])
        bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["rmean"])
        bn.running_var.copy_(case["rvar"])
    x = case["x"].to(dev, torch.bfloat16).requires_grad_(True)
    res = None
    if case["res"] is not None:
        res = case["res"].to(dev, torch.bfloat16).requires_grad_(True)
    out = batch_norm_act(x, bn, training=case["training"], act=case["act"],
                         residual=res)
    assert out.dtype == torch.bfloat16
    out.backward(case["dy"].to(dev, torch.bfloat16))
    got = dict(out=out.detach(), dx=x.grad, dgamma=bn.weight.grad,
               dbeta=bn.bias.grad, running_mean=bn.running_mean,
               running_var=bn.running_var)
    got = {k: v.detach().double().cpu() for k, v in got.items()}
    got["dres"] = res.grad.cpu() if res is not None else None
    got["nbt"] = int(bn.num_batches_tracked)
    return got


@pytest.mark.parametrize("kw", _CASES, ids=_IDS)
def test_bn_matches_fp64(dev, kw):
    case = O.bn_case(**kw)
    r64, r32 = O.bn_case_oracle(case)
    bounds = O.bn_bounds(case, r64, r32)
    got = _run_gpu(case, dev)
    worst = {}
    for k, (bound, e32) in bounds.items():
        err = (got[k] - r64[k]).abs()
        worst[k] = float((err / bound).max())
        print(f"bn {kw} {k}: max err {float(err.max()):.3e} e32 {e32:.3e} "
              f"min bound {float(bound.min()):.3e} worst err/bound "
              f"{worst[k]:.3f}")
    for k in bounds:
        assert worst[k] <= 1.0, (k, worst[k])
    if case["training"]:
        # matching the oracle, which applies the momentum update once, also
        # shows that a batch of B > 1 images advances the statistics once
        assert got["nbt"] == 1
    else:
        assert got["nbt"] == 0
        assert torch.equal(got["running_mean"], case["rmean"].double())
        assert torch.equal(got["running_var"], case["rvar"].double())
    if case["res"] is not None:
        # the gradient reaching the residual is dy after its bf16 rounding
        assert got["dres"].dtype == torch.bfloat16
        assert torch.equal(got["dres"], case["dy"].to(torch.bfloat16))


def test_bn_two_calls_advance_running_stats_twice(dev):
    """Second call on the same module: the statistics and the batch counter
    advance once per call (oracle applied twice)."""
    case = O.bn_case((3, 5, 7, 9), act=0)
    r64a, _ = O.bn_case_oracle(case)
    second = dict(case, rmean=r64a["running_mean"], rvar=r64a["running_var"])
    r64b, r32b = O.bn_case_oracle(second)
    bounds = O.bn_bounds(second, r64b, r32b)
    c = case["x"].shape[1]
    bn = torch.nn.BatchNorm2d(c).to(dev)
    with torch.no_grad():
        bn.weight.copy_(case["gamma"])
        bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["rmean"])
        bn.running_var.copy_(case["rvar"])
    x = case["x"].to(dev, torch.bfloat16)
    for _ in range(2):
        batch_norm_act(x, bn, training=True, act=0)
    assert int(bn.num_batches_tracked) == 2
    for k, buf in (("running_mean", bn.running_mean),
                   ("running_var", bn.running_var)):
        err = (buf.double().cpu() - r64b[k]).abs()
        # two updates: twice the one-update bound
        assert bool((err <= 2 * bounds[k][0]).all()), k


# ----------------------------------------- against torch's batch_norm
# The older checks, kept as they were.

def test_bn_act_matches_torch(dev):
    from dsin_amd.ops.bn import batch_norm_act
    torch.manual_seed(0)
    bn1 = torch.nn.BatchNorm2d(32, eps=1e-5, momentum=0.1).to(dev)
    bn2 = torch.nn.BatchNorm2d(32, eps=1e-5, momentum=0.1).to(dev)
    with torch.no_grad():
        bn2.weight.copy_(bn1.weight)
        bn2.bias.copy_(bn1.bias)
        g = torch.rand(32, device=dev) + 0.5
        bn1.weight.copy_(g); bn2.weight.copy_(g)
        b = torch.randn(32, device=dev) * 0.3
        bn1.bias.copy_(b); bn2.bias.copy_(b)
    x = (torch.randn(2, 32, 20, 24, device=dev) * 2 + 1).to(torch.bfloat16)
    x1 = x.clone().requires_grad_(True)
    y1 = batch_norm_act(x1, bn1, training=True, act=1)
    x2 = x.float().clone().requires_grad_(True)
    y2 = torch.relu(torch.nn.functional.batch_norm(
        x2, bn2.running_mean, bn2.running_var, bn2.weight, bn2.bias, True,
        0.1, 1e-5))
    torch.testing.assert_close(y1.float(), y2, rtol=0.05, atol=0.05)
    torch.testing.assert_close(bn1.running_mean, bn2.running_mean,
                               rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(bn1.running_var, bn2.running_var,
                               rtol=1e-2, atol=1e-2)
    gr = torch.randn_like(y2)
    y1.backward(gr.to(y1.dtype))
    y2.backward(gr)
    torch.testing.assert_close(x1.grad.float(), x2.grad, rtol=0.1, atol=0.1)
    torch.testing.assert_close(bn1.weight.grad, bn2.weight.grad,
                               rtol=0.05, atol=0.3)
    torch.testing.assert_close(bn1.bias.grad, bn2.bias.grad,
                               rtol=0.05, atol=0.3)


def test_bn_eval_mode(dev):
    from dsin_amd.ops.bn import batch_norm_act
    torch.manual_seed(1)
    bn = torch.nn.BatchNorm2d(16).to(dev)
    with torch.no_grad():
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2)
    x = torch.randn(1, 16, 8, 12, device=dev).to(torch.bfloat16)
    y = batch_norm_act(x, bn, training=False, act=0)
    yr = torch.nn.functional.batch_norm(
        x.float(), bn.running_mean, bn.running_var, bn.weight, bn.bias,
        False, 0.1, bn.eps)
    torch.testing.assert_close(y.float(), yr, rtol=0.05, atol=0.05)
