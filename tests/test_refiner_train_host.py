"""CPU only: the references of tests/refiner_train_ref.py agree with one another, and the bounds of tests/test_gpu_refiner_train.py hide no lost term."""
import pytest
import torch

from conftest import load_golden
import refiner_train_ref as R


@pytest.mark.parametrize("tag", R.TAGS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_hand_written_chain_equals_autograd(tag, kind):
    """The backward the kernels implement, restated by hand in f64, against torch autograd through the oracle in f64: 1e-10 relative on every tensor.
    The key third of in_proj_bias is mathematically zero (a shift of every key cancels in the softmax); both give rounding noise there."""
    ref, got = R.autograd_grads(tag, kind), R.chain(tag, kind)
    assert abs(got["loss"] - ref["loss"]) < 1e-12 * abs(ref["loss"])
    a, b = R.split_thirds(ref["grads"]), R.split_thirds(got["grads"])
    assert sorted(a) == sorted(b) and len(ref["grads"]) == 18
    for k in a:
        if k == R.ZERO_REFERENCE:
            assert float(a[k].norm()) < 1e-15 and float(b[k].norm()) < 1e-15, k
        else:
            assert R.rel_l2(b[k], a[k]) < 1e-10, (k, R.rel_l2(b[k], a[k]))
            lo, hi = (3e-4, 1.4e-1) if (tag, kind) == ("full", "prob") else (1e-4, 1.0)       # no tensor of the fixture has a vanishing gradient
            assert lo < float(a[k].norm()) < hi, (k, float(a[k].norm()))


@pytest.mark.parametrize("tag", R.TAGS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_f64_reference_reproduces_g9b(tag, kind):
    g = load_golden("g9b_refiner_train")
    ref = R.autograd_grads(tag, kind)
    want = float(g[f"{tag}.{kind}.ex_loss"])
    assert abs(ref["loss"] - want) < 2e-6 * want, (ref["loss"], want)          # G9b is the reference module in f32
    assert ref["window_preds"].shape[0] == (18 if tag == "full" else 6)
    assert R.rel_l2(ref["window_preds"], g[f"{tag}.{kind}.window_preds"]) < 1e-5


def test_f32_chain_is_far_inside_the_bounds():
    """the same chain in f32: its error is what an exact-f32 implementation would show, orders below the 16-bit bounds"""
    err, bound = R.branch_error(R.chain("full", "prob", torch.float32)["grads"], "full", "prob"), R.branch_bounds("full", "prob")
    for k in err:
        assert err[k] < 0.05 * bound[k], (k, err[k], bound[k])


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_fault_exceeds_a_bound(fault):
    """Each lost term moves at least one tensor beyond the bound the GPU test uses for it (3 x the bf16-autocast error): the bounds hide none of them."""
    bound = R.branch_bounds("full", "prob")
    err = R.branch_error(R.chain("full", "prob", fault=fault)["grads"], "full", "prob")
    over = {k: err[k] / bound[k] for k in err if err[k] > bound[k]}
    assert over, (fault, max(err[k] / bound[k] for k in err))


def test_branch_bounds_are_what_the_issue_measured():
    b = R.branch_bounds("full", "prob")
    rel = {k: v / 3.0 for k, v in b.items() if k != R.ZERO_REFERENCE}
    assert 5e-4 < min(rel.values()) and max(rel.values()) < 3e-2, (min(rel.values()), max(rel.values()))
    assert b[R.ZERO_REFERENCE] / 3.0 < 1e-5


def test_attention_cases_reach_every_tile_edge():
    """From the tile constants: Nq and Nk each reach one below, equal to and one above a wave's rows, a streamed tile and a workgroup's rows, and more
    than two tiles.  (The dQ kernel owns queries and streams keys; the dK/dV kernel owns keys and streams queries.)"""
    for axis in (1, 2):
        have = {c[axis] for c in R.ATTN_CASES}
        for edge in (R.WAVE_ROWS, R.ST, R.WT):
            assert {edge - 1, edge, edge + 1} <= have, (axis, edge, sorted(have))
        assert any(n > 2 * R.ST for n in have) and 1 in have
    kinds = {c[4] for c in R.ATTN_CASES}
    assert {"randn", "peaked", "ldq", "ldout"} <= kinds
    assert (1, 96, 3136, 1, "randn") in R.ATTN_CASES and (1, 36, 36, 8, "randn") in R.ATTN_CASES


def test_attention_rounding_model_and_checker():
    """The rounding model is a bf16-sized distance from the reference; the model itself passes the checker, a lost delta, ln 2 or lse does not."""
    case = (2, 70, 45, 2, "randn")
    ops = R.attn_inputs(case)
    ref, model = R.attn_backward(*ops, 2, lambda x: x), R.attn_backward(*ops, 2, R.bf16_round)
    for name in R.GRADS:
        e = float(R.slab_error(model[name], ref[name]).max())
        assert 1e-4 < e < 2e-2, (name, e)
    R.attn_check("model", model, ref, model, audit=False)
    for name, factor in (("dk", 1.0 / R.LN2), ("dq", 96 ** 0.5)):
        bad = dict(model)
        bad[name] = model[name] * factor
        with pytest.raises(AssertionError):
            R.attn_check("fault", bad, ref, model, audit=False)
    # the base-2 log-sum-exp of the model stays inside the bound of the LSE test (tests/test_gpu_vit_train.py:241)
    assert float((model["lse"] - ref["lse"]).abs().max()) / R.LOG2E < R.lse_bound(ref["lse"])


def test_descent_reference_decreases():
    """the f64 losses the GPU descent check's docstring quotes"""
    losses = R.sgd_losses(R.SGD_LR)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert all(abs(a - b) < 5e-6 for a, b in zip(losses, R.SGD_F64)), losses
    assert min(a - b for a, b in zip(losses, losses[1:])) > 1e-3                # margin: 16-bit noise on the loss is ~1e-4
