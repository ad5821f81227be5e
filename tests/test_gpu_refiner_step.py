"""GPU: the refiner's training step -- SparseRefiner.loss_and_grads into caller-owned buffers, the direct weight gradients inside the chain, RefinerArena,
the two fused AdamW segments, LocalRefineTrainLoop and the runner switch.  Fixtures, f64 autograd and bounds: tests/refiner_train_ref.py (by import); the AdamW
trajectories through the oracle: tests/refiner_wgrad_ref.py.  No bound here comes from GPU output."""
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import maxdiff, within

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import refiner_train_ref as R  # noqa: E402
import refiner_wgrad_ref as W  # noqa: E402
from refiner_train_ref import RI  # noqa: E402
from ucod_dpl_amd.engine.config import CfgNode  # noqa: E402
from ucod_dpl_amd.engine.runner.loop_CORAL import LocalRefineTrainLoop, RefinerArena  # noqa: E402
from ucod_dpl_amd.models.UDLR import SparseRefiner  # noqa: E402

DEV = torch.device("cuda", 0)
WEIGHTS = ("attn.attn.in_proj_weight", "attn.attn.out_proj.weight", "attn.mlp.0.weight", "attn.mlp.2.weight")      # what the six direct products write


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def make_module(**keys):
    torch.manual_seed(RI.SEED)
    return RI.perturb_(SparseRefiner.from_config(CfgNode(dict(window_size=3, threshold=0.0015, **keys)))).train().to(DEV)


def batch(tag="full", kind="prob"):
    l, h, preds = RI.make_inputs(tag == "partial")
    return l.to(DEV), h.to(DEV), preds.to(DEV), RI.make_h_targets(kind).to(DEV)


def buffers(m, n=18):
    params = [p for _, p in m.HRE.CSF.named_parameters()] + [m.GE.fuser[0].weight, m.GE.fuser[0].bias, m.GE.fuser[2].weight, m.GE.fuser[2].bias]
    return [torch.full_like(p.detach(), float("nan")) for p in params[:n]]


def make_loop(m=None, direct=True, cot=None, lr=W.ADAMW_LR, preds=None):
    cfg = CfgNode(dict(model_cfg=dict(window_length=6),
                       train_cfg=dict(dist_train=False, lr0=lr, step_lr_size=2, step_lr_gamma=0.95, max_epoch=1, start_epoch=0, refiner_direct_wgrad=direct,
                                      save_cfg=dict(save_interval=1, start_save=0))))
    runner = SimpleNamespace(refiner=make_module() if m is None else m, model=lambda x: (preds,), device=DEV, train_dataloader=[], save_checkpoint=lambda e: None)
    return LocalRefineTrainLoop(cfg, runner, outputs_cotangent=cot)


def mean_cotangent(outputs, opt):
    return torch.ones_like(outputs) / outputs.numel()                                # d outputs.mean() / d outputs


# ================================================================================================ loss_and_grads
@pytest.mark.parametrize("tag", R.TAGS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_loss_and_grads_is_bit_equal_to_autograd(tag, kind):
    """direct_wgrad off: the buffers hold the bits of .grad after ex_loss.backward(), and outputs / ex_loss are the forward's"""
    m = make_module()
    out_a, ex_a, _ = m(*batch(tag, kind))
    ex_a.backward()
    m2 = make_module()
    bufs = buffers(m2)
    out, ex, opt = m2.loss_and_grads(*batch(tag, kind), bufs)
    assert opt["grads_written"] == (True, False) and not ex.requires_grad
    assert torch.equal(bits(out), bits(out_a)) and torch.equal(bits(ex), bits(ex_a))
    for (k, p), b in zip(m.HRE.CSF.named_parameters(), bufs):
        assert b.shape == p.shape and torch.equal(bits(b), bits(p.grad)), k
    assert all(p.grad is None for p in m2.parameters())                              # no autograd graph was involved


@pytest.mark.parametrize("tag", R.TAGS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_direct_wgrad_gradients_within_the_branch_bounds(tag, kind):
    """direct_wgrad on: every tensor within R.branch_bounds (3 x the bf16-autocast oracle's error) of f64 autograd; the tensors no weight-gradient product
    writes are the bits of the other route"""
    m, m0 = make_module(direct_wgrad=True), make_module()
    assert m.direct_wgrad and not m0.direct_wgrad
    bufs, bufs0 = buffers(m), buffers(m0)
    _, ex, _ = m.loss_and_grads(*batch(tag, kind), bufs)
    _, ex0, _ = m0.loss_and_grads(*batch(tag, kind), bufs0)
    assert torch.equal(bits(ex), bits(ex0))
    names = [k for k, _ in m.HRE.CSF.named_parameters()]
    for k, b, b0 in zip(names, bufs, bufs0):
        assert not bool(torch.isnan(b).any()), k
        if k not in WEIGHTS:
            assert torch.equal(bits(b), bits(b0)), k
    err, bound = R.branch_error({k: b.cpu() for k, b in zip(names, bufs)}, tag, kind), R.branch_bounds(tag, kind)
    for k in err:
        print(f"direct {tag}.{kind} {k}: {err[k]:.3e} (bound {bound[k]:.3e}, ratio to the autocast error {3 * err[k] / bound[k]:.2f})")
    for k in err:
        within(f"refiner_step:direct_grad:{k}", err[k], bound[k])


def test_outputs_cotangent_is_the_refiner_function_backward():
    """with an outputs_cotangent the 22 buffers hold the bits of .grad after (ex_loss + outputs.mean()).backward() through _RefinerFunction (train_outputs)"""
    m = make_module(train_outputs=True)
    out_a, ex_a, _ = m(*batch())
    (ex_a + out_a.mean()).backward()
    assert m.csf_backward_calls == 1
    m2 = make_module()
    bufs = buffers(m2, 22)
    out, ex, opt = m2.loss_and_grads(*batch(), bufs, outputs_cotangent=mean_cotangent)
    assert opt["grads_written"] == (True, True) and m2.csf_backward_calls == 1
    assert torch.equal(bits(out), bits(out_a)) and torch.equal(bits(ex), bits(ex_a))
    params = [p for _, p in m.HRE.CSF.named_parameters()] + [m.GE.fuser[0].weight, m.GE.fuser[0].bias, m.GE.fuser[2].weight, m.GE.fuser[2].bias]
    for i, (p, b) in enumerate(zip(params, bufs)):
        assert torch.equal(bits(b), bits(p.grad)), i
    with pytest.raises(ValueError):
        m2.loss_and_grads(*batch(), bufs[:18], outputs_cotangent=mean_cotangent)
    with pytest.raises(ValueError):
        m2.loss_and_grads(*batch(), bufs[:5])
    # no window and no cotangent: 0, and no buffer is touched; no window with a cotangent: the fuser buffers alone
    l, h, preds, ht = batch()
    nan = buffers(m2, 22)
    _, ex, opt = m2.loss_and_grads(l, h, torch.full_like(preds, 14.0), ht, nan)
    assert ex == 0 and isinstance(ex, int) and opt["grads_written"] == (False, False) and all(bool(torch.isnan(b).all()) for b in nan)
    _, ex, opt = m2.loss_and_grads(l, h, torch.full_like(preds, 14.0), ht, nan, outputs_cotangent=mean_cotangent)
    assert ex == 0 and opt["grads_written"] == (False, True) and all(bool(torch.isnan(b).all()) for b in nan[:18]) and not any(bool(torch.isnan(b).any()) for b in nan[18:])


# ================================================================================================ the optimizer step
def test_one_step_matches_adamw_in_f64_and_ex_loss_leaves_ge_alone():
    loop = make_loop()
    A, m = loop.arena, loop.refiner
    l, h, preds, ht = batch()
    p0 = A.p.clone()
    last = loop.refine_step(l, h, preds, ht)
    assert last["stepped"] and last["windows"] == int(R.fixture("full", "prob")["mask"].sum()) and float(last["ex_loss"]) > 0
    n = A.n_csf
    ref = p0[:n].double().cpu().requires_grad_(True)
    ref.grad = A.g[:n].double().cpu()
    torch.optim.AdamW([ref], lr=W.ADAMW_LR).step()
    d = maxdiff(A.p[:n].cpu(), ref.detach())
    print(f"one AdamW step against f64 on the same gradients: max |dp| {d:.2e} (moved by up to {float((A.p[:n] - p0[:n]).abs().max()):.2e})")
    within("refiner_step:adamw_vs_f64", d, 1e-6)                                    # tests/test_gpu_kernels.py::test_adamw_ema_matches_torch_optimizer
    assert float((A.p[:n] - p0[:n]).abs().min()) >= 0 and float((A.p[:n] != p0[:n]).float().mean()) > 0.99
    loop.refine_step(l, h, preds, ht)
    # ex_loss alone: GE.* bit-unchanged, their moments zero, their step count 0
    assert torch.equal(bits(A.p[n:]), bits(p0[n:])) and not bool(A.m[n:].any()) and not bool(A.v[n:].any())
    assert loop.optimizers["csf"].t == 2 and loop.optimizers["fuser"].t == 0
    for k, p in m.named_parameters():                                                # the parameters ARE the arena
        assert p.data_ptr() == A.p[A.offsets[A.names.index(k)]:].data_ptr(), k


def test_outputs_cotangent_moves_all_22_parameters():
    loop = make_loop(cot=mean_cotangent)
    A = loop.arena
    p0 = A.p.clone()
    loop.refine_step(*batch())
    for name, off, n in zip(A.names, A.offsets, A.sizes):
        moved = float((A.p[off:off + n] != p0[off:off + n]).float().mean())
        assert (moved == 0) if name == "GE.alpha" else (moved > 0.9), (name, moved)
    assert loop.optimizers["csf"].t == 1 and loop.optimizers["fuser"].t == 1


def test_prepared_operands_are_invalidated_by_a_step():
    """the stale-operand trap: the in-place HIP update changes neither data_ptr nor _version, so the module would go on multiplying by the old bf16 weights"""
    loop = make_loop()
    m = loop.refiner
    l, h, preds, ht = batch()
    with torch.no_grad():
        before, _, _ = m.eval()(l, h, preds)
    m.train()
    loop.refine_step(l, h, preds, ht)
    fresh = make_module()
    fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    with torch.no_grad():
        got, _, _ = m.eval()(l, h, preds)
        want, _, _ = fresh.eval()(l, h, preds)
    assert torch.equal(bits(got), bits(want))
    assert not torch.equal(bits(got), bits(before))                                  # (and the step was large enough to show)


def test_no_window_batch_takes_no_step():
    loop = make_loop()
    A = loop.arena
    l, h, preds, ht = batch()
    A.g.fill_(7.0)
    state = [t.clone() for t in (A.p, A.g, A.m, A.v)]
    kept = loop.refiner._prepare(DEV)
    last = loop.refine_step(l, h, torch.full_like(preds, 14.0), ht)
    assert last == dict(ex_loss=0, windows=0, stepped=False) and loop.refiner._prepared is kept
    for a, b in zip(state, (A.p, A.g, A.m, A.v)):
        assert torch.equal(bits(a), bits(b))
    assert loop.optimizers["csf"].t == 0 and loop.optimizers["fuser"].t == 0


def test_three_steps_twice_give_identical_bits():
    runs = []
    for _ in range(2):
        loop = make_loop(cot=mean_cotangent)
        losses = [bits(loop.refine_step(*batch())["ex_loss"]).clone() for _ in range(3)]
        runs.append((losses, loop.arena.p.clone(), loop.arena.m.clone(), loop.arena.v.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(bits(a), bits(b))


def test_five_adamw_steps_follow_the_f64_oracle():
    """ex_loss over five steps at the config's lr0 against the same five torch.optim.AdamW steps in f64 through the CPU oracle: the largest relative distance
    is at most 3 x that of the oracle under bf16 autocast run through the same steps (the project's 16-bit convention)."""
    f64, ac = W.adamw_losses("f64"), W.adamw_losses("autocast")
    loop = make_loop()
    l, h, preds, ht = batch()
    got = [float(loop.refine_step(l, h, preds, ht)["ex_loss"]) for _ in range(5)]
    dev, dev_ac = W.loss_deviation(got, f64), W.loss_deviation(ac, f64)
    print(f"ex_loss over five AdamW steps: GPU {got} | f64 {f64} | autocast {ac} | deviation {dev:.3e} vs autocast {dev_ac:.3e}: ratio {dev / dev_ac:.2f} (bound 3)")
    assert all(b < a for a, b in zip(got, got[1:])), got
    within("refiner_step:five_steps_deviation", dev, 3.0 * dev_ac)


# ================================================================================================ loop and runner
def test_loop_step_takes_preds_from_the_frozen_baseline_and_schedules_per_epoch():
    l, h, preds, ht = batch()
    loop = make_loop(preds=preds)
    same = make_loop()
    b = dict(features=l, h_inputs=h, h_targets=ht)
    out = loop.step(b)
    ref = same.refine_step(l, h, preds, ht)
    assert out["stepped"] and torch.equal(bits(out["ex_loss"]), bits(ref["ex_loss"])) and torch.equal(bits(loop.arena.p), bits(same.arena.p))
    with pytest.raises(KeyError, match="h_targets"):
        loop.step(dict(features=l, h_inputs=h))
    loop.runner.train_dataloader = [b, b]
    loop._max_epoch = 2
    loop.run()
    assert loop.global_step == 5 and loop.optimizers["csf"].t == 5 and loop._cur_epoch == 2
    assert loop.optimizers["csf"].param_groups[0]["lr"] == pytest.approx(W.ADAMW_LR * 0.95)     # StepLR(2, 0.95) stepped once per epoch, twice


def test_runner_raises_with_the_shipped_config_and_trains_with_the_switch(tmp_path):
    from safetensors.torch import load_file
    from conftest import ROOT
    from ucod_dpl_amd.engine.runner import create_runner, LocalRefineRunner
    cfg = CfgNode(CfgNode.load_with_base(os.path.join(ROOT, "configs", "uscod", "CORAL_dinov2.py")))
    cfg.log_cfg.log_path = str(tmp_path)
    cfg.train_cfg.checkpoint = os.path.join(ROOT, "tests", "golden", "weights", "UCOD_DPL_dinov2.safetensors")
    cfg.model_cfg.window_length = 6
    l, m, h = RI.coral_inputs()
    ht = RI.make_h_targets("prob")[:9]
    b = dict(pseudo_label=None, label_tensor=None, features=l, img_path=["x"], m_inputs=m, h_inputs=h, index=[0], h_targets=ht)
    runner = create_runner(cfg, train_dataloader=[b, b])
    assert isinstance(runner, LocalRefineRunner)
    with pytest.raises(NotImplementedError):
        runner.launch_train()
    assert isinstance(runner.optimizer, torch.optim.AdamW)
    cfg.train_cfg.refiner_train_loop = True
    cfg.train_cfg.max_epoch = 1
    cfg.train_cfg.save_cfg.save_interval = 1
    before = {k: v.detach().clone() for k, v in runner.refiner.state_dict().items()}
    last = runner.launch_train()
    loop = runner.trainloop
    assert loop.global_step == 2 and loop.refiner.direct_wgrad and loop.require_m_patches
    path = os.path.join(str(tmp_path), "refiner_ckp", "epoch1.pth", "model.safetensors")
    saved = load_file(path)
    assert sorted(saved) == sorted(before) and all(saved[k].shape == before[k].shape for k in before)
    fresh = SparseRefiner.from_config(cfg.model_cfg)
    fresh.load_state_dict(saved, strict=True)
    runner.load_refiner_checkpoint(os.path.dirname(path))
    if last["stepped"]:
        assert loop.optimizers["csf"].t >= 1 and any(not torch.equal(saved[k], before[k].cpu()) for k in before)
    for k, v in runner.refiner.state_dict().items():
        assert torch.equal(v.cpu(), saved[k]), k
