"""CPU: what makes the per-head attention-backward tests of tests/test_gpu_attention_bwd.py legitimate, and what they can see.

1. attn_bwd_ref.reference (closed formulas, f64) against f64 torch autograd of softmax attention, a spiked key included.
2. Coverage: attn_bwd_ref.walk restates every decision of the launch and the two kernels of csrc/attention_bwd.hip; enumerated over N = 1..1500 and a grid
   of (B, heads) it gives the reachable classes, and attn_bwd_ref.CASES reaches every value of every axis, every (dQ walk, dK/dV walk) pair, every
   (grid class, one / many row blocks) pair and every (dead waves, partly dead last wave) pair.
3. The yardstick: over all CASES and both input kinds the rounding model's distance to the reference is neither zero nor broken: in (0, 1e-2) per slab for the
   roundings the kernel header documents, and no further above that than the forward's own probability rounding can reach.
4. Checker sensitivity: eleven faults a tile-walk, grid-decode or scaling error would cause, injected into the model at 100, 256 and 1374 tokens.  check()
   rejects ten of them everywhere, by at least 3 x the bound (ratio 6.1 against F = 2: the last key dropped from dQ at 1374 tokens on random operands).  The
   eleventh, a zero-filled out-of-range key counted in the row sums, cannot move a gradient by one bf16 rounding; that is asserted instead.
5. The record of the gap: which of those faults the old bar (one relative L2 < 1.5e-2 per gradient over the whole tensor) accepts.
"""
import pytest
import torch

import attn_bwd_ref as R

SENS_CASES = ((1, 100, 1), (2, 256, 2), (1, 1374, 2))
FILL = 5.0                       # what the GPU tests pre-fill dqkv with


# ================================================================================================ 1. reference against autograd
def _autograd(qs, k, v, do, heads):
    q = (R.heads_of(qs, heads) / R.C_Q).requires_grad_(True)             # the unscaled q the gradient refers to
    kk, vv = R.heads_of(k, heads).requires_grad_(True), R.heads_of(v, heads).requires_grad_(True)
    s = q @ kk.transpose(2, 3) * R.HD ** -0.5
    o = torch.softmax(s, -1) @ vv
    dO = R.heads_of(do, heads)
    dq, dk, dv = torch.autograd.grad((o * dO).sum(), (q, kk, vv))
    return {"out": o.detach(), "lse": torch.logsumexp(s, -1).detach() / R.LN2, "delta": (o.detach() * dO).sum(-1), "dq": dq, "dk": dk, "dv": dv}


@pytest.mark.parametrize("case,kind,spike", [((2, 70, 3), "randn", False), ((1, 100, 1), "edges", False), ((2, 45, 2), "randn", True)])
def test_reference_equals_f64_autograd(case, kind, spike):
    qs, k, v, do = R.inputs(case, kind)
    if spike:                                                             # one key that takes nearly all of every row's probability
        k = k.clone()
        k[:, 17] = (k[:, 17].float() * 6).to(torch.bfloat16)
    ref, auto = R.reference(qs, k, v, do, case[2]), _autograd(qs, k, v, do, case[2])
    for name, a in auto.items():
        err = float((ref[name] - a).norm() / a.norm())
        assert err < 1e-10, (name, err)


# ================================================================================================ 2. coverage
def _reachable():
    return {R.walk(N, B, heads) for N in range(1, 1501) for B in (1, 2, 3, 4) for heads in (1, 2, 3, 4, 6, 8, 12, 16, 24)}


PAIRS = (("dq", "dkv"), ("grid", "nb"), ("dead_waves", "last_wave_partial"))


def test_cases_reach_every_walk_class():
    reach = _reachable()
    have = {R.walk(N, B, heads) for B, N, heads in R.CASES}
    assert have <= reach
    for axis in R.Walk._fields:
        want, got = {getattr(w, axis) for w in reach}, {getattr(w, axis) for w in have}
        print(f"{axis}: reachable {sorted(want, key=str)}")
        assert want == got, (axis, sorted(want - got, key=str))
    for a, b in PAIRS:
        want, got = {(getattr(w, a), getattr(w, b)) for w in reach}, {(getattr(w, a), getattr(w, b)) for w in have}
        print(f"({a}, {b}): {len(want)} reachable pairs, {len(got)} reached")
        for p in sorted(want, key=str):
            print("   ", p, "<-", [c for c in R.CASES if (getattr(R.walk(c[1], c[0], c[2]), a), getattr(R.walk(c[1], c[0], c[2]), b)) == p])
        assert want == got, ((a, b), sorted(want - got, key=str))


def test_walk_classes_are_what_the_kernel_source_says():
    """walk() on hand-worked shapes: a slip in the restatement would let CASES 'cover' classes that do not exist."""
    w = R.walk(1370, 1, 2)                    # nt 22, remainder 26: 21 full tiles, TAIL on buffer 1 with its second block skipped; last workgroup has 90 rows
    assert w == R.Walk(("odd", "skipped"), ("odd", "skipped"), 1, True, "many", "lt8")
    w = R.walk(165, 1, 1)                     # nt 3, remainder 37
    assert (w.dq, w.dkv, w.dead_waves, w.last_wave_partial) == (("even", "masked"), ("even", "processed"), 2, True)
    w = R.walk(64, 1, 8)                      # one full tile and nothing else
    assert w == R.Walk(("odd", "none"), ("zero", "processed"), 2, False, "one", "eq8")
    assert R.walk(7, 3, 3).grid == "gt8_partial" and R.walk(7, 2, 12).grid == "gt8_full"
    old = {R.walk(N, B, h) for B, N, h in R.CASES[:4]}                   # what the suite ran before: the record behind the issue
    assert {w.dq[1] for w in old} == {"skipped"} and {w.dkv[1] for w in old} == {"skipped"} and {w.grid for w in old} == {"lt8"}


# ================================================================================================ 3. the yardstick
def _forward_rounding_reach(case, kind, ref):
    """First-order worst case of what the forward's probability rounding (attn_bwd_ref.forward_out) can add to a slab's relative error.  Each probability is
    off by at most 2^-9 relative, so delta_i moves by at most 2^-9 a_i with a_i = sum_j P_ij |dO_i . V_j|; dS_ij moves by P_ij times that, hence
    dQ_i by 2^-9 a_i * 0.125 |(P K)_i| and dK_j by ln 2 * 2^-9 sum_i P_ij a_i |Q_i|.  dV does not see delta."""
    qs, k, v, do = (R.heads_of(t, case[2]) for t in R.inputs(case, kind))
    P = torch.exp2(qs @ k.transpose(2, 3) - ref["lse"].unsqueeze(-1))
    a = (P * (do @ v.transpose(2, 3)).abs()).sum(-1, keepdim=True)
    dq = 2.0 ** -9 * 0.125 * (a * (P @ k)).flatten(2).norm(dim=2) / ref["dq"].flatten(2).norm(dim=2)
    dk = 2.0 ** -9 * R.LN2 * ((P * a).transpose(2, 3) @ qs.abs()).flatten(2).norm(dim=2) / ref["dk"].flatten(2).norm(dim=2)
    return {"dq": dq, "dk": dk, "dv": torch.zeros_like(dq)}


def test_model_error_is_neither_zero_nor_broken():
    """Over all CASES and both kinds.  The model of the roundings the header of attention_bwd.hip documents stays in the band (0, 1e-2) per slab.  The model
    check() uses adds the rounding inside the forward, which on peaked rows with a large dO is the largest single term (one slab of (2, 70, 12) "edges"
    reaches 1.03e-2 in dQ, in the model and on the GPU alike): it stays above 0 and below that band plus the first-order reach of the added rounding."""
    lo, hi, lo_f, hi_f = float("inf"), 0.0, float("inf"), 0.0
    for case in R.CASES:
        for kind in R.KINDS:
            ref, model = R.expected(case, kind)
            header = R.rounding_model(*R.inputs(case, kind), case[2], forward=False)
            reach = _forward_rounding_reach(case, kind, ref)
            for name in R.GRADS:
                e, ef = R.slab_error(header[name], ref[name]), R.slab_error(model[name], ref[name])
                lo, hi, lo_f, hi_f = min(lo, float(e.min())), max(hi, float(e.max())), min(lo_f, float(ef.min())), max(hi_f, float(ef.max()))
                assert 0 < float(e.min()) and float(e.max()) < 1e-2, (case, kind, name, float(e.min()), float(e.max()))
                assert 0 < float(ef.min()) and bool((ef < 1e-2 + reach[name]).all()), (case, kind, name, ef, reach[name])
            assert torch.equal(header["dv"], model["dv"])
    print(f"model slab error over {len(R.CASES)} cases x {len(R.KINDS)} kinds: header roundings {lo:.3e} .. {hi:.3e}, with the forward's {lo_f:.3e} .. {hi_f:.3e}")


# ================================================================================================ 4. faults
def _at(stage, fn):
    def hook(s, x):
        if s != stage:
            return x
        x = x.clone()
        fn(x)
        return x
    return hook


def _set(stage, value):
    return lambda s, x: value if s == stage else x


def _swap(out):
    out = {k: t.clone() for k, t in out.items()}
    for name in R.GRADS:
        out[name][0, 0], out[name][-1, -1] = out[name][-1, -1].clone(), out[name][0, 0].clone()
    return out


def _fill_row(out):
    out = dict(out)
    out["dk"] = out["dk"].clone()
    out["dk"][-1, -1, -1] = FILL
    return out


def faults(case):
    """{name: (hook or None, post-edit or None)}: each is applied to the LAST (image, head) slab unless it says otherwise."""
    B, N, heads = case
    t0 = (N - 1) // R.ST * R.ST
    halved = lambda x: x[-1, -1, :, t0].mul_(0.5)                               # noqa: E731
    f = {
        "last key dropped from dQ": (_at("ds_for_dq", lambda x: x[-1, -1, :, N - 1].zero_()), None),
        "last query dropped from dK": (_at("ds_for_dk", lambda x: x[-1, -1, N - 1].zero_()), None),
        "last query dropped from dV": (_at("p_for_dv", lambda x: x[-1, -1, N - 1].zero_()), None),
        "P of the last tile's first key halved": (_at("p", halved), None),
        "last row of dK left at its fill": (None, _fill_row),
        "dK without ln 2": (_set("dk_scale", 1.0), None),
        "dQ without 0.125": (_set("dq_scale", 1.0), None),
    }
    if t0 + 32 < N:                                                              # (1374 = 21 * 64 + 30: that block holds no key)
        f["key (last tile + 32) dropped from dQ"] = (_at("ds_for_dq", lambda x: x[-1, -1, :, t0 + 32].zero_()), None)
    if B * heads > 1:
        f["first and last slabs swapped"] = (None, _swap)
    if heads > 1:
        f["delta from the neighbouring head"] = (lambda s, x: x.roll(1, dims=1) if s == "delta" else x, None)
    return f


def _phantom_zero_key(s, x):
    """An out-of-range key that reads as zeros (S = 0) counted in the row sums: L' = log2(2^L + 2^0).  Its K and V rows are zero, so all it can do to a
    gradient is rescale the row's P and dS by 2^L / (2^L + 1)."""
    return torch.log2(torch.exp2(x) + 1.0) if s == "lse" else x


def _faulty(case, kind, hook, post):
    out = R.rounding_model(*R.inputs(case, kind), case[2], hook) if hook else R.expected(case, kind)[1]
    return post(out) if post else out


def _old_bar_accepts(got, ref):
    """test_gpu_vit_train.py::test_attention_backward: one relative L2 per gradient over the whole tensor"""
    return all(float((got[n] - ref[n]).norm() / ref[n].norm()) < 1.5e-2 for n in R.GRADS)


# which faults the old global bar lets through -- a record, computed on the CPU.  Random operands spread a row's probability over all keys, so at 256 and
# 1374 tokens one lost or halved key among them moves the whole-tensor norm by well under 1.5e-2.
_HALVED, _LASTKEY = "P of the last tile's first key halved", "last key dropped from dQ"
OLD_BAR_ACCEPTS = {
    ((1, 100, 1), "randn"): set(),
    ((1, 100, 1), "edges"): set(),
    ((2, 256, 2), "randn"): {_HALVED, _LASTKEY},
    ((2, 256, 2), "edges"): {_HALVED},
    ((1, 1374, 2), "randn"): {_HALVED, _LASTKEY},
    ((1, 1374, 2), "edges"): set(),
}


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", SENS_CASES)
def test_check_rejects_every_injected_fault(case, kind):
    ref, model = R.expected(case, kind)
    assert max(R.check("model", model, ref, model, audit=False).values()) == 1.0          # the unfaulted model passes, at ratio 1 by construction
    accepted_by_old = set()
    for name, (hook, post) in faults(case).items():
        bad = _faulty(case, kind, hook, post)
        r = R.ratios(bad, ref, model)
        print(f"{case} {kind:6s} {name:40s} worst ratio {max(r.values()):10.1f}   old bar {'accepts' if _old_bar_accepts(bad, ref) else 'rejects'}")
        with pytest.raises(AssertionError):
            R.check(name, bad, ref, model, audit=False)
        if _old_bar_accepts(bad, ref):
            accepted_by_old.add(name)
    assert accepted_by_old == OLD_BAR_ACCEPTS[case, kind], (case, kind, sorted(accepted_by_old))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", SENS_CASES)
def test_a_zero_key_counted_in_the_row_sums_is_below_one_rounding(case, kind):
    """The eleventh fault is arithmetically invisible, so it is recorded, not rejected.  A zero-filled out-of-range key has S = 0 against a row sum 2^L in the
    hundreds or thousands, and its zero K and V rows add nothing to any product: all it does is scale the row's P and dS by 2^L / (2^L + 1), less than one
    bf16 unit in the last place (2^-8) on the worst row at 100 tokens and ten times less at 1374.  No checker with F > 1 can tell that from another draw of
    the roundings, and none should: asserted, check() accepts it (measured ratios 1.00 .. 1.31)."""
    ref, model = R.expected(case, kind)
    rescale = float((1.0 / (torch.exp2(ref["lse"]) + 1.0)).max())
    bad = _faulty(case, kind, _phantom_zero_key, None)
    r = R.check("phantom", bad, ref, model, audit=False)
    print(f"{case} {kind:6s} largest relative change of a row {rescale:.2e}; worst ratio {max(r.values()):.2f}")
    assert rescale < 2.0 ** -8
