"""CPU tests of tests/_oracles.py: the conditions the GPU kernel tests rely
on, checked on the reference alone (none of these needs a GPU)."""

import pytest
import torch

import _oracles as O
from dsin_amd import ops
from dsin_amd.ops import reference as ref


# ------------------------------------------------------------------- NCC

@pytest.mark.parametrize("case", O.NCC_CASES, ids=str)
def test_ncc_cases_are_decided(case):
    """At least 90% of the patches have a top-2 gap in the fp64 map above
    bound = 4*e32 + 1e-5, so the exact-agreement GPU test is not vacuous."""
    d = O.ncc_reference(*case)
    share = float(d["decided"].float().mean())
    print(f"ncc {case}: e32 {d['e32']:.2e} bound {d['bound']:.2e} min gap "
          f"{float(d['gaps'].min()):.2e} decided {share:.3f}")
    assert share >= 0.9


@pytest.mark.parametrize("case", O.NCC_CASES, ids=str)
def test_ncc_search_ref_agrees_with_fp64_map(case):
    """The CPU path of the op lands on the fp64 argmax. ncc_search_ref keeps
    its operands in fp32 where the kernel (and the oracle) round them to
    bf16, which moves every score by up to delta = max|map64 - map64 of the
    unrounded operands|; so the locations must be equal wherever the gap
    exceeds bound + 2*delta, and on every patch the location it picks scores
    within 2*delta + bound of the oracle's maximum."""
    h, w, ph, pw, use_mask, noise = case
    d = O.ncc_reference(*case)
    _, rows, cols = ref.ncc_search_ref(d["x"], d["y_dec"], d["y_orig"], ph, pw,
                                       use_mask)
    unrounded = O.ncc_map(d["x"], d["y_dec"], ph, pw, use_mask, torch.float64,
                          round_bf16=False)
    delta = float((unrounded - d["m64"]).abs().max())
    tol = d["bound"] + 2 * delta
    same = (rows == d["rows"]) & (cols == d["cols"])
    sure = d["gaps"] > tol
    score = d["m64"][torch.arange(rows.numel()), rows, cols]
    print(f"ncc ref {case}: delta {delta:.2e} agree {int(same.sum())}/"
          f"{same.numel()} sure {int(sure.sum())}")
    assert bool(same[sure].all())
    assert bool((score >= d["vmax"] - tol).all())


def test_ncc_map_matches_reference_mask_and_formula():
    """The oracle's inline location prior equals the dense mask of the
    reference for even patch sizes."""
    h, w, ph, pw = 24, 80, 6, 10
    x, y_dec, _ = O.ncc_case(h, w, 3, 8)
    with_mask = O.ncc_map(x, y_dec, ph, pw, True, torch.float64)
    without = O.ncc_map(x, y_dec, ph, pw, False, torch.float64)
    mask = ref.gaussian_mask_value(w // pw, ph, pw, h, w, "cpu", torch.float64)
    torch.testing.assert_close(with_mask, without * mask, rtol=1e-12,
                               atol=1e-14)


@pytest.mark.parametrize("ph,pw", [(c[2], c[3]) for c in O.NCC_V1_CASES])
def test_ncc_v1_cases_fit_64k_of_lds(ph, pw):
    assert pw % 8 != 0 and O.ncc_v1_lds_bytes(ph, pw) < 65536


@pytest.mark.parametrize("tie", O.NCC_TIE_CASES, ids=str)
def test_ncc_tie_cases_have_a_unique_first_maximum(tie):
    """Every periodic copy of a patch's own location scores the maximum, and
    no other location comes near it."""
    ty, tx, ny, nx, ph, pw = tie
    y = O.ncc_tie_case(ty, tx, ny, nx)
    m = O.ncc_map(y, y, ph, pw, False, torch.float64)
    gw = y.shape[2] // pw
    margin = 1.0
    for p in range(m.shape[0]):
        gr, gc = divmod(p, gw)
        copies = torch.zeros_like(m[p], dtype=torch.bool)
        copies[(gr * ph) % ty::ty, (gc * pw) % tx::tx] = True
        assert copies.sum() > 1
        assert bool((m[p][copies] > 1 - 1e-9).all())
        margin = min(margin, 1.0 - float(m[p][~copies].max()))
    print(f"tie {tie}: margin to any non-copy {margin:.3f}")
    assert margin > 0.5


@pytest.mark.parametrize("use_mask", [False, True])
def test_ncc_flat_case_has_decided_patches(use_mask):
    d = O.ncc_flat_case(use_mask)
    assert int(d["decided"].sum()) >= 27  # 90% of the 30 textured patches


def _bad_ncc_inputs():
    x = torch.rand(3, 24, 80) * 255
    return [
        ("tile", (x, x, x, 5, 10, False)),
        ("tile", (x, x, x, 6, 9, False)),
        ("share one shape", (x, x[:, :, :70].contiguous(), x, 6, 10, False)),
        ("share one shape", (x, x, x[:, :18].contiguous(), 6, 10, False)),
        ("even patch sizes", (x, x, x, 3, 10, True)),
        ("even patch sizes", (x, x, x, 6, 5, True)),
    ]


@pytest.mark.parametrize("match,args", _bad_ncc_inputs())
def test_ncc_search_rejects_bad_inputs_on_cpu(match, args):
    with pytest.raises(ValueError, match=match):
        ops.ncc_search(*args)


def test_ncc_search_accepts_odd_patches_without_mask_on_cpu():
    x, y_dec, y_orig = O.ncc_case(21, 45, 1, 8)
    y_syn, rows, cols = ops.ncc_search(x, y_dec, y_orig, 7, 15, False)
    assert y_syn.shape == x.shape and rows.numel() == 9


# ------------------------------------------------------------ batch norm

_BN_IDS, _BN_CASES = O.bn_cases()


@pytest.mark.parametrize("kw", _BN_CASES, ids=_BN_IDS)
def test_bn_cases_mask_few_elements_and_bounds_hold_for_emulation(kw):
    """Under 1% of the elements sit within 1e-3 of the activation's kink
    (their dy is zeroed). An emulation of the kernel's arithmetic, the fp32
    result rounded to bf16, stays inside the bounds the GPU test uses."""
    case = O.bn_case(**kw)
    assert case["masked"] < 0.01
    r64, r32 = O.bn_case_oracle(case)
    bounds = O.bn_bounds(case, r64, r32)
    for k in ("out", "dx"):
        emu = r32[k].to(torch.bfloat16).double()
        slack = (bounds[k][0] - (emu - r64[k]).abs()).min()
        assert float(slack) >= 0, (k, float(slack))
    for k in ("dgamma", "dbeta", "running_mean", "running_var"):
        if k in bounds:
            assert bool(((r32[k].double() - r64[k]).abs()
                         <= bounds[k][0]).all()), k
    print(f"bn {kw}: masked {case['masked']:.4f}")


def test_bn_oracle_matches_torch_batch_norm():
    case = O.bn_case((3, 5, 7, 9), act=0)
    r64, _ = O.bn_case_oracle(case)
    x = case["x"].double().requires_grad_(True)
    g = case["gamma"].double().requires_grad_(True)
    b = case["beta"].double().requires_grad_(True)
    rm, rv = case["rmean"].double().clone(), case["rvar"].double().clone()
    out = torch.nn.functional.batch_norm(x, rm, rv, g, b, True, 0.1, 1e-5)
    dx, dg, db = torch.autograd.grad(out, (x, g, b), case["dy"].double())
    for got, want in ((r64["out"], out.detach()), (r64["dx"], dx),
                      (r64["dgamma"], dg), (r64["dbeta"], db),
                      (r64["running_mean"], rm), (r64["running_var"], rv)):
        torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-10)


# ------------------------------------------------------------- pointwise

def test_quantizer_symbols_are_decided_on_99_percent():
    """Wherever the two smallest distances differ by more than 1e-6
    relative, fp32 and fp64 pick the same center; that holds for at least
    99% of the elements of the inputs the GPU test uses."""
    for L in (6, 16):
        x, centers, _ = O.quantizer_inputs(3 * 7 * 11 * 13, L, seed=L)
        r = O.quantize_oracle(x, centers, 1.0, torch.ones_like(x),
                              torch.float64)
        assert float((r["relgap"] > 1e-6).float().mean()) >= 0.99


@pytest.mark.parametrize("use_wd", [False, True])
def test_fused_adam_cpu_branch_matches_fp64_oracle(use_wd):
    """The class's CPU branch stays within the bound the GPU kernel is held
    to (tests/test_gpu_pointwise.py)."""
    for sizes in O.ADAM_SMALL_SIZES:
        O.run_adam_case(sizes, use_wd, torch.device("cpu"))


def test_heatmap_clamp_edge_share_is_small():
    for dtype in (torch.float32, torch.bfloat16):
        b, edge = O.heatmap_inputs(dtype)
        assert float(edge.float().mean()) < 0.01
