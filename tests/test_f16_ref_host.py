"""CPU: the acceptance rule of tests/f16_ref.py (error against the f64 reference at most F times the rounding model's, in relative L2 and in the worst row)
rejects subtly wrong attention outputs -- each fault below is simulated on the CPU and must be refused with the factor F the GPU tests use -- and takes
the model itself, also in the forms a correct kernel may differ by (f32 scores, probabilities formed against a trailing maximum)."""
import pytest
import torch

import f16_ref as R

SHAPES = [(1, 65, 3), (2, 257, 2), (1, 1370, 2)]
F16 = torch.float16


@pytest.fixture(scope="module")
def case():
    cache = {}

    def get(fam, B, tok, heads, dt=F16):
        key = (fam, B, tok, heads, dt)
        if key not in cache:
            x = {"r": R.family_r, "s": R.family_s}[fam](B, tok, heads, dt)
            cache[key] = (x, R.attention_ref(x, B, tok, heads, 1.0), R.attention_model(x, B, tok, heads, 1.0))
        return cache[key]
    return get


def _with_keys(x, B, tok, heads, keys):
    """f64 attention of every query over an edited key set: keys(k, v) -> (k', v') on [B, heads, tok, 64]."""
    q, k, v = R.heads_of(x, B, tok, heads)
    k, v = keys(k, v)
    o = R.softmax_v_model(torch.matmul(q, k.transpose(2, 3)), v, x.dtype, x.dtype)
    return o.transpose(1, 2).reshape(B * tok, heads * 64)


def test_factors_are_in_the_range_the_rule_needs():
    assert 1.0 < R.F_L2 <= R.F <= 4.0


@pytest.mark.parametrize("B,tok,heads", SHAPES)
@pytest.mark.parametrize("fam", ["r", "s"])
def test_the_model_passes_with_room_to_spare(case, fam, B, tok, heads):
    x, ref, model = case(fam, B, tok, heads)
    assert R.accepts(model, ref, model)[0]
    # f32 scores (the MFMA accumulator) and P formed against a maximum that trails the true one by 2^8, the far end of the deferred max
    s32 = R.scores(x, B, tok, heads, 1.0).float().double()
    _, _, v = R.heads_of(x, B, tok, heads)
    alt = R.softmax_v_model(s32, v, F16, F16, lag=8.0).transpose(1, 2).reshape(B * tok, heads * 64)
    ok, r2, rm = R.accepts(alt, ref, model)
    assert ok and r2 < 1.05 and rm < 1.25, (r2, rm)          # (a power of two moves nothing but the subnormal boundary)


@pytest.mark.parametrize("B,tok,heads", SHAPES)
@pytest.mark.parametrize("dt", [F16, torch.bfloat16])
def test_a_deferred_maximum_is_accepted(case, dt, B, tok, heads):
    """attn_fwd_v5_kernel / attn_fwd_v6_kernel form P against a running maximum that trails the true one by a NON-integer power of two: the heaviest key's P is
    no longer exactly 1 and is rounded like the others.  A correct kernel of that kind -- every row trailing by the same delta, the worst case -- costs up to
    1.6 x the model in relative L2 and 2 x in the worst row here; the rule must take it.  (Measured on the GPU: 1.26 / 2.79, only rows whose first key block
    does not hold the maximum trail.)"""
    x, ref, model = case("r", B, tok, heads, dt)
    s = R.scores(x, B, tok, heads, 1.0)
    _, _, v = R.heads_of(x, B, tok, heads)
    worst = 0.0
    for lag in (0.5, 3.3, 7.7):
        alt = R.softmax_v_model(s, v, dt, dt, lag=lag).transpose(1, 2).reshape(B * tok, heads * 64)
        ok, r2, rm = R.accepts(alt, ref, model)
        assert ok, (lag, r2, rm)
        worst = max(worst, r2)
    assert worst > 1.3                                       # ... and the effect is real: the model's exact P = 1 is worth that much
    # closer to the kernels: the running maximum is the first 32-key block's until a later key beats it by more than 2^8 (then it is rescaled to the true one)
    first, top = s[..., :32].amax(-1, keepdim=True), s.amax(-1, keepdim=True)
    lag = torch.where(top - first > 8.0, torch.zeros_like(top), top - first)
    p = torch.exp2(s - top + lag)
    alt = (torch.matmul(p.float().to(dt).double(), v) / p.sum(-1, keepdim=True)).float().to(dt).double().transpose(1, 2).reshape(B * tok, heads * 64)
    ok, r2, rm = R.accepts(alt, ref, model)
    assert ok and 1.05 < r2 < 1.3, (r2, rm)                  # 1.10 - 1.22 here; the GPU measures 1.10 - 1.25 on the same inputs


@pytest.mark.parametrize("B,tok,heads", SHAPES)
def test_family_s_scores_are_all_far_below_zero(B, tok, heads):
    for dt in (F16, torch.bfloat16):
        for pre in (True, False):
            s = R.scores(R.family_s(B, tok, heads, dt, pre), B, tok, heads, 1.0 if pre else R.C_PRE)
            assert float(s.max()) < -20.0, (dt, pre, float(s.max()))


@pytest.mark.parametrize("B,tok,heads", SHAPES)
def test_bf16_sized_probability_error_is_refused_on_fp16_operands(case, B, tok, heads):
    x, ref, model = case("r", B, tok, heads)
    bad = R.attention_model(x, B, tok, heads, 1.0, p_dtype=torch.bfloat16, out_dtype=torch.bfloat16)
    ok, r2, _ = R.accepts(bad, ref, model)
    assert not ok and r2 > 7.0, r2                           # the bf16 model on fp16 operands: 8 x the fp16 model, beyond any F the rule allows
    # bf16 probabilities alone (the output still rounded to fp16) sit at 3.6 - 4.0 x: F = 4 alone would take them at some shapes, F_L2 must not
    bad = R.attention_model(x, B, tok, heads, 1.0, p_dtype=torch.bfloat16)
    ok, r2, _ = R.accepts(bad, ref, model)
    assert not ok and r2 > 1.5 * R.F_L2, r2
    # ... while the same output IS what the bf16 build's bound takes
    xb, refb, modelb = case("r", B, tok, heads, torch.bfloat16)
    assert R.accepts(modelb, refb, modelb)[0]


@pytest.mark.parametrize("dominant", [0, 333])
def test_flushed_subnormal_probabilities_are_refused(dominant):
    x = R.family_p(dominant)
    ref, model = R.attention_ref(x, 1, R.P_TOK, 1, 1.0), R.attention_model(x, 1, R.P_TOK, 1, 1.0)
    p = torch.exp2(R.scores(x, 1, R.P_TOK, 1, 1.0))
    sub = (p.float().half().float() < 2.0 ** -14).float().mean().item()
    assert sub > 0.99 * (R.P_TOK - 1) / R.P_TOK                # every probability but the dominant key's is an fp16 subnormal
    assert R.rel_l2(model, ref) < 5e-4                        # kept, the subnormals cost their six bits: 2.6e-4
    bad = R.attention_model(x, 1, R.P_TOK, 1, 1.0, flush_subnormal_p=True)
    assert R.rel_l2(bad, ref) > 0.5                           # flushed: 0.67
    assert not R.accepts(bad, ref, model)[0]


@pytest.mark.parametrize("B,tok,heads", SHAPES)
def test_a_padded_zero_key_counted_as_real_is_refused(case, B, tok, heads):
    """K / V rows past the last token read as zero: such a key has score 0.  On family R its weight is 2^-15 (hidden); on family S it carries the row."""
    pad = lambda k, v: (torch.cat((k, torch.zeros_like(k[:, :, :1])), 2), torch.cat((v, torch.zeros_like(v[:, :, :1])), 2))
    x, ref, model = case("s", B, tok, heads)
    bad = _with_keys(x, B, tok, heads, pad)
    assert R.rel_l2(bad, ref) > 0.99 and not R.accepts(bad, ref, model)[0]
    # the same fault on family R with bf16 operands from 129 tokens on: the rule (and every bar of the product tests) takes it -- which is why family S exists
    if tok >= 129:
        xr, refr, modelr = case("r", B, tok, heads, torch.bfloat16)
        assert R.accepts(_with_keys(xr, B, tok, heads, pad), refr, modelr)[0]


@pytest.mark.parametrize("B,tok,heads", SHAPES)
@pytest.mark.parametrize("fam", ["r", "s"])
def test_a_dropped_last_key_is_refused(case, fam, B, tok, heads):
    x, ref, model = case(fam, B, tok, heads)
    bad = _with_keys(x, B, tok, heads, lambda k, v: (k[:, :, :-1], v[:, :, :-1]))
    assert not R.accepts(bad, ref, model)[0]


@pytest.mark.parametrize("B,tok,heads", SHAPES)
def test_exchanged_heads_and_a_repeated_row_are_refused(case, B, tok, heads):
    x, ref, model = case("r", B, tok, heads)
    swapped = model.clone()
    swapped[:, :64], swapped[:, 64:128] = model[:, 64:128], model[:, :64]
    assert not R.accepts(swapped, ref, model)[0]
    row = model.clone()
    row[tok - 1] = model[tok - 2]                             # one output row replaced by its neighbour
    ok, r2, rm = R.accepts(row, ref, model)
    assert not ok and rm > R.F, (r2, rm)                     # (a single row among 1370 moves the L2 norm little: the row bound is what sees it)
