"""CPU: the checkers of the direct weight-gradient kernel and of the refiner's optimizer step (tests/refiner_wgrad_ref.py) are shown to catch what they
are there for, and the host side of the step -- the split rule the library exports, the arena's layout, the segment-skip rule, the StepLR schedule -- is
checked against torch on the CPU."""
import pytest
import torch

import refiner_wgrad_ref as W
from ucod_dpl_amd.engine.config import CfgNode


# ================================================================================================ the split of the token axis
SIZES = [(M, N, K) for (N, K) in ((64, 64), (128, 192), (256, 128), (768, 768), (1536, 768), (3072, 768), (768, 3072))
         for M in (1, 63, 64, 65, 127, 128, 129, 300, 895, 896, 897, 3136, 56448, 56449)]


def test_library_nsplit_is_the_documented_rule():
    from ucod_dpl_amd import native
    lib = native.load()
    for M, N, K in SIZES:
        n, chunk = W.nsplit_rule(M, N, K)
        assert lib.ucod_wgrad_bf16_det_nsplit(M, N, K) == n, (M, N, K)
        assert lib.ucod_wgrad_bf16_det_workspace_bytes(M, N, K) == (0 if n == 1 else n * N * K * 4)
    assert W.nsplit_rule(56448, 768, 768)[0] * 36 in range(240, 513)             # fills the 256 CUs at 768 x 768 ...
    assert W.nsplit_rule(56448, 3072, 768)[0] in (1, 2) and W.nsplit_rule(56448, 768, 3072)[0] in (1, 2)      # ... and stays at 1-2 at 3072 x 768
    for bad in ((0, 64, 64), (5, 96, 64), (5, 64, 100), (5, 0, 64)):
        assert lib.ucod_wgrad_bf16_det_nsplit(*bad) == 0 and lib.ucod_wgrad_bf16_det_workspace_bytes(*bad) == 0
    assert lib.ucod_wgrad_bf16_det(None, 64, None, 64, None, 64, 8, 64, 64, 0, None, 0, None) == -1


def test_chunking_partitions_the_rows():
    for M, N, K in SIZES:
        n, chunk = W.nsplit_rule(M, N, K)
        c2, ranges = W.chunking(M, n)
        assert c2 == chunk and chunk % W.SLAB == 0                               # the chunk size follows from nsplit alone
        assert ranges[0][0] == 0 and ranges[-1][1] == M and all(a < b for a, b in ranges)           # no empty chunk
        assert all(r0[1] == r1[0] for r0, r1 in zip(ranges, ranges[1:])) and all(b - a == chunk for a, b in ranges[:-1])
        assert W.chain_length(M, n) == chunk // 16 + n + 1


# ================================================================================================ exact cases and the bound
CASES = [(200, 128, 192, False, True), (200, 128, 192, True, True), (130, 64, 64, True, False), (65, 256, 128, False, False), (300, 256, 128, True, False)]


@pytest.mark.parametrize("M,N,K,accumulate,wide", CASES)
def test_exact_cases_hold_bit_for_bit_in_any_order(M, N, K, accumulate, wide):
    case = W.make_case(M, N, K, "exact", accumulate, wide)
    n, _ = W.nsplit_rule(M, N, K)
    assert W.check(case, W.emulate(case, n).float(), n) is None
    # f32 arithmetic, the chunks in another order and the rows one at a time: the same bits
    dy, x = case["dy"].float(), case["x"].float()
    acc = case["base"].clone() if accumulate else torch.zeros(N, K)
    for m in reversed(range(M)):
        acc += torch.outer(dy[m], x[m])
    assert W.check(case, acc, n) is None
    assert float((case["ref"] != 0).double().mean()) > 0.9                       # not a degenerate case


@pytest.mark.parametrize("M,N,K,accumulate,wide", CASES)
def test_bound_is_derived_and_small(M, N, K, accumulate, wide):
    case = W.make_case(M, N, K, "random", accumulate, wide)
    n, chunk = W.nsplit_rule(M, N, K)
    assert W.check(case, W.emulate(case, n), n) is None
    lim = W.bound(case, n)
    c = chunk // 16 + n + 1
    mag = case["dy"].double().abs().t() @ case["x"].double().abs() + (case["base"].double().abs() if accumulate else 0)
    assert torch.allclose(lim, c * 2.0 ** -24 * mag, rtol=1e-4, atol=0)
    assert float((lim / case["ref"].abs().clamp_min(1e-3)).median()) < 1e-3     # far below the values it guards


@pytest.mark.parametrize("kind", ("exact", "random"))
@pytest.mark.parametrize("fault", W.FAULTS)
def test_every_injected_fault_is_caught(fault, kind):
    hit = 0
    for M, N, K, accumulate, wide in CASES:
        if (fault == "no_accumulate" and not accumulate) or (fault == "tail_past_M" and M % W.SLAB == 0):
            continue
        case = W.make_case(M, N, K, kind, accumulate, wide)
        n, _ = W.nsplit_rule(M, N, K)
        assert W.check(case, W.emulate(case, n, fault=fault), n) is not None, (fault, kind, M, N, K)
        hit += 1
    assert hit >= 2


# ================================================================================================ the arena
def make_refiner():
    from ucod_dpl_amd.models.UDLR import SparseRefiner
    torch.manual_seed(3)
    return SparseRefiner.from_config(CfgNode(dict(window_size=3, threshold=0.0015)))


def test_arena_layout_and_state_dict():
    from ucod_dpl_amd.engine.runner.loop_CORAL import RefinerArena
    m = make_refiner()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m._prepared = "stale"
    A = RefinerArena(m)
    assert m._prepared is None
    layout = W.arena_layout(m)
    assert [n for n, _, _ in layout] == A.names and [o for _, o, _ in layout] == A.offsets and [s for _, _, s in layout] == A.sizes
    assert A.n == sum(s for _, _, s in layout) and A.n_csf == sum(s for _, _, s in layout[:18]) and A.n_fuser == 64 + 64 + 64 + 1 and A.names[-1] == "GE.alpha"
    assert all(t.shape == (A.n,) and t.dtype == torch.float32 for t in (A.p, A.g, A.m, A.v))
    params = dict(m.named_parameters())
    for (name, off, n), gv in zip(layout, A.grad_views):
        assert params[name].data_ptr() == A.p[off:off + n].data_ptr() and gv.data_ptr() == A.g[off:off + n].data_ptr() and gv.shape == params[name].shape
    after = m.state_dict()
    assert list(after) == list(before) and all(after[k].shape == before[k].shape and torch.equal(after[k], before[k]) for k in before)
    # loading a checkpoint writes into the arena; the arena's segments are the two optimizers' parameters
    m.load_state_dict({k: v + 1 for k, v in before.items()}, strict=True)
    assert torch.equal(A.p[:4], (before[A.names[0]] + 1).reshape(-1)[:4]) and float(A.p[-1]) == float(before["GE.alpha"]) + 1
    assert A.segment(A.p, "csf").numel() == A.n_csf and A.segment(A.p, "fuser").data_ptr() == A.p[A.n_csf:].data_ptr()


# ================================================================================================ the segment rule and the schedule
def host_loop(monkeypatch, lr=1e-2, step_size=2, gamma=0.5):
    from types import SimpleNamespace
    from ucod_dpl_amd import ops
    from ucod_dpl_amd.engine.runner.loop_CORAL import LocalRefineTrainLoop
    monkeypatch.setattr(ops, "adamw_ema", W.adamw_cpu)
    cfg = CfgNode(dict(model_cfg=dict(window_length=6),
                       train_cfg=dict(dist_train=False, lr0=lr, step_lr_size=step_size, step_lr_gamma=gamma, max_epoch=5, start_epoch=0,
                                      save_cfg=dict(save_interval=100, start_save=0))))
    runner = SimpleNamespace(refiner=make_refiner(), model=None, device=torch.device("cpu"), train_dataloader=[], save_checkpoint=lambda e: None)
    return LocalRefineTrainLoop(cfg, runner)


def test_segments_follow_adamw_grad_is_none_rule(monkeypatch):
    """a segment that received no gradient is not touched -- no decay, no moment update, no count -- exactly torch.optim.AdamW with .grad None"""
    loop = host_loop(monkeypatch)
    A, m = loop.arena, loop.refiner
    assert loop.refiner.direct_wgrad is True
    ref = {k: v.detach().clone().requires_grad_(True) for k, v in m.named_parameters()}
    opt = torch.optim.AdamW(list(ref.values()), lr=1e-2)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    g = torch.Generator().manual_seed(5)
    pattern = [(True, False), (True, False), (True, True), (False, False), (False, True), (True, True)]
    for epoch, (csf, fuser) in enumerate(pattern):
        A.g.copy_(torch.randn(A.n, generator=g) * 0.1)
        m._prepared = "fresh"
        for name, gv in zip(A.names, A.grad_views):
            seg = csf if name.startswith("HRE.CSF.") else (fuser if name != "GE.alpha" else False)
            ref[name].grad = gv.detach().clone() if seg else None
        stepped = loop.apply_updates(csf, fuser)
        opt.step()
        assert stepped == (csf or fuser) and (m._prepared is None) == stepped       # the stale-operand trap: invalidated exactly when a segment moved
        for s in loop.lr_schedulers.values():
            s.step()
        sched.step()
        for k in ("csf", "fuser"):
            assert loop.optimizers[k].param_groups[0]["lr"] == pytest.approx(sched.get_last_lr()[0], rel=1e-12), epoch
        for name, p in m.named_parameters():
            assert torch.allclose(p.detach(), ref[name].detach(), rtol=0, atol=2e-7), (epoch, name)
    assert loop.optimizers["csf"].t == 4 and loop.optimizers["fuser"].t == 3
    assert opt.state[ref["HRE.CSF.mask_dec.bias"]]["step"] == 4 and opt.state[ref["GE.fuser.0.bias"]]["step"] == 3 and ref["GE.alpha"] not in opt.state
    assert float(m.GE.alpha.detach()) == 0.5


def test_step_needs_h_targets(monkeypatch):
    loop = host_loop(monkeypatch)
    with pytest.raises(KeyError, match="h_targets"):
        loop.step(dict(features=torch.zeros(1, 768, 6, 6), h_inputs=torch.zeros(1, 9, 768, 6, 6)))


def test_adamw_reference_descends():
    """the f64 AdamW trajectory the GPU test follows: strictly decreasing, and the bf16-autocast oracle stays close to it"""
    f64, ac = W.adamw_losses("f64"), W.adamw_losses("autocast")
    assert all(b < a for a, b in zip(f64, f64[1:])), f64
    assert 0 < W.loss_deviation(ac, f64) < 2e-2, (ac, f64)
