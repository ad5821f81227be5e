"""GPU: ucod_attention_fwd_lse + ucod_attention_bwd (csrc/attention_bwd.hip: attn_bwd_dq_kernel / attn_bwd_dkv_kernel) at every tile-walk case, per (image, head)
slab against f64, through the C ABI only.

attn_bwd_ref.py holds the reference, the rounding model the tolerances come from, the restatement of the tile walk and the case list; test_attn_bwd_host.py
shows on the CPU that the list reaches every case and that the checker rejects a lost boundary key or query, a wrong slab, a wrong scale.  Here:

  test_backward_matches_f64_per_head            out / lse / delta / dQ / dK / dV of every case, both input kinds; rows and columns around the outputs untouched
  test_each_head_equals_its_own_single_pair_call  the grid decode, descriptor bases and per-image ranges, bit for bit
  test_repeat_launches_are_bitwise_equal        the header's "no atomics (bitwise reproducible)"
  test_refusals                                 every argument set the entry rejects before launching
"""
import functools

import pytest
import torch

import attn_bwd_ref as R
from conftest import within

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402

DEV = "cuda"
AUG = N.LORA_AUG
EINVAL = -1
PAD = 128                        # sentinel rows (dqkv) / floats (delta) in front of and behind the views the kernels write
FILL_BF16, FILL_F32 = 5.0, -7.25


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _launch(qs, k, v, do, heads, aug):
    """fwd_lse then bwd on [B, N, D] operands; dqkv and delta are views into larger sentinel-filled buffers.  Everything comes back on the CPU, untouched:
    out [B, N, D] bf16, lse / delta [B, heads, N] f32, dqkv [B, N, ld] bf16, and whether every sentinel survived."""
    B, T, D = qs.shape
    ld = 3 * D + (AUG if aug else 0)
    lib = N.load()
    qkv = torch.cat((qs, k, v), -1).reshape(B * T, 3 * D).contiguous().to(DEV)
    dos = do.reshape(B * T, D).contiguous().to(DEV)
    out = torch.empty(B * T, D, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, heads, T, device=DEV)
    N.check(lib.ucod_attention_fwd_lse(N.ptr(qkv), N.ptr(out), N.ptr(lse), B, T, heads, N.stream()), "fwd_lse")
    big = torch.full((B * T + 2 * PAD, ld), FILL_BF16, dtype=torch.bfloat16, device=DEV)
    bigd = torch.full((B * heads * T + 2 * PAD,), FILL_F32, device=DEV)
    dqkv, delta = big[PAD:PAD + B * T], bigd[PAD:PAD + B * heads * T]
    N.check(lib.ucod_attention_bwd(N.ptr(qkv), N.ptr(out), N.ptr(dos), N.ptr(lse), N.ptr(delta), N.ptr(dqkv), ld, B, T, heads, N.stream()), "bwd")
    torch.cuda.synchronize()
    big, bigd = big.cpu(), bigd.cpu()
    fill16, fill32 = _bits(torch.tensor(FILL_BF16, dtype=torch.bfloat16)), _bits(torch.tensor(FILL_F32))
    untouched = {
        "dqkv rows in front": bool((_bits(big[:PAD]) == fill16).all()), "dqkv rows behind": bool((_bits(big[PAD + B * T:]) == fill16).all()),
        "aug columns": bool((_bits(big[PAD:PAD + B * T, 3 * D:]) == fill16).all()),
        "delta in front": bool((_bits(bigd[:PAD]) == fill32).all()), "delta behind": bool((_bits(bigd[PAD + B * heads * T:]) == fill32).all()),
    }
    return {"out": out.cpu().reshape(B, T, D), "lse": lse.cpu(), "delta": bigd[PAD:PAD + B * heads * T].reshape(B, heads, T).clone(),
            "dqkv": big[PAD:PAD + B * T].reshape(B, T, ld).clone(), "untouched": untouched}


@functools.lru_cache(maxsize=None)
def gpu(case, kind, aug=True):
    """one launch per (case, kind, leading dimension), shared by the tests"""
    return _launch(*R.inputs(case, kind), case[2], aug)


def _slabs(g, heads):
    """the launch's results as attn_bwd_ref lays them out: [B, heads, N, 64] / [B, heads, N]"""
    D = heads * R.HD
    d = g["dqkv"]
    return {"out": R.heads_of(g["out"], heads), "lse": g["lse"].double(), "delta": g["delta"].double(),
            "dq": R.heads_of(d[..., :D], heads), "dk": R.heads_of(d[..., D:2 * D], heads), "dv": R.heads_of(d[..., 2 * D:3 * D], heads)}


_ID = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c)          # noqa: E731
PLAIN_LD = ((1, 100, 1), (3, 140, 3))          # additionally with ld_dqkv = 3D: no aug columns between the rows
RUNS = [(c, k, True) for c in R.CASES for k in R.KINDS] + [(c, "edges", False) for c in PLAIN_LD]


@pytest.mark.parametrize("case,kind,aug", RUNS, ids=[f"{_ID(c)}-{k}-{'aug' if a else 'ld3D'}" for c, k, a in RUNS])
def test_backward_matches_f64_per_head(case, kind, aug):
    """Measured (profiles/attention_bwd_tests.txt): kernel error / model error at most 1.08 over all cases, 1.00 in most -- the model's f64 sums and the kernel's
    f32 sums round to the same bf16 in over 99 % of the elements."""
    B, T, heads = case
    tag = f"{_ID(case)}:{kind}:{'aug' if aug else 'ld3D'}"
    qs, k, v, do = R.inputs(case, kind)
    ref, model = R.expected(case, kind)
    g = gpu(case, kind, aug)
    got = _slabs(g, heads)
    assert all(g["untouched"].values()), g["untouched"]                   # sentinel rows, sentinel floats and the aug columns: bit-identical
    assert bool(torch.isfinite(g["dqkv"][..., :3 * heads * R.HD].float()).all())
    # out: the bar tests/test_gpu_kernels.py holds this forward kernel to, here per slab
    within(f"attn_bwd:{tag}:out_slab_rel_l2", float(R.slab_error(got["out"], ref["out"]).max()), 4e-3)
    # lse (base 2): the bar of test_gpu_vit_train.py::test_attention_backward, in natural-log units
    ln = ref["lse"] * R.LN2
    within(f"attn_bwd:{tag}:lse_maxdiff", float((got["lse"] * R.LN2 - ln).abs().max()), 2e-3 * max(1.0, float(ln.abs().max())))
    # delta: the f32 sum of the 64 products dO * (the GPU's own bf16 out), each exact in f32
    prod = R.heads_of(do, heads) * got["out"]
    excess = (got["delta"] - prod.sum(-1)).abs() - 64 * 2.0 ** -24 * prod.abs().sum(-1)
    assert float(excess.max()) <= 0, (tag, "delta", float(excess.max()))
    r = R.check(tag, got, ref, model)
    print("\nRATIO " + tag + "  " + "  ".join(f"{n}:{b}={r[n, b]:.3f}" for n in R.GRADS for b in ("slab", "row")))


# ------------------------------------------------------------------------------------------------ one pair at a time
@pytest.mark.parametrize("case", [(3, 40, 3), (2, 70, 12), (2, 300, 12)], ids=_ID)
def test_each_head_equals_its_own_single_pair_call(case):
    """Every (image, head) slab of the batched call is bitwise the B = 1, heads = 1 call on that slab's own columns: the arithmetic of a pair does not
    depend on its neighbours (same tile walk, same summation order, no atomics), so this pins decode(), the descriptor bases and the per-image ranges with
    no tolerance."""
    B, T, heads = case
    qs, k, v, do = R.inputs(case, "edges")
    batched = gpu(case, "edges")
    D = heads * R.HD
    for b in range(B):
        for h in range(heads):
            col = slice(h * R.HD, (h + 1) * R.HD)
            one = _launch(*(t[b:b + 1, :, col].contiguous() for t in (qs, k, v, do)), 1, True)
            assert all(one["untouched"].values()), (b, h, one["untouched"])
            pairs = {"out": (batched["out"][b, :, col], one["out"][0]), "lse": (batched["lse"][b, h], one["lse"][0, 0]),
                     "delta": (batched["delta"][b, h], one["delta"][0, 0])}
            for i, name in enumerate(R.GRADS):
                pairs[name] = (batched["dqkv"][b, :, i * D + h * R.HD:i * D + (h + 1) * R.HD], one["dqkv"][0, :, i * R.HD:(i + 1) * R.HD])
            for name, (x, y) in pairs.items():
                assert torch.equal(_bits(x.contiguous()), _bits(y.contiguous())), (b, h, name)


# ------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("case", [(2, 300, 12), (1, 1374, 2)], ids=_ID)
def test_repeat_launches_are_bitwise_equal(case):
    """attention_bwd.hip: 'Two kernels, no atomics (bitwise reproducible)' -- three launches into fresh sentinel-filled buffers, delta included"""
    ops = R.inputs(case, "edges")
    first = _launch(*ops, case[2], True)
    for _ in range(2):
        again = _launch(*ops, case[2], True)
        for name in ("out", "lse", "delta", "dqkv"):
            assert torch.equal(_bits(first[name]), _bits(again[name])), name


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """every argument set ucod_attention_bwd rejects before it launches anything returns UCOD_EINVAL, and leaves the buffers alone"""
    B, T, heads = 1, 8, 1
    D = heads * R.HD
    lib = N.load()
    qkv = torch.zeros(B * T, 3 * D, dtype=torch.bfloat16, device=DEV)
    out, dout = (torch.zeros(B * T, D, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    lse = torch.zeros(B, heads, T, device=DEV)
    delta = torch.full((B, heads, T), FILL_F32, device=DEV)
    dqkv = torch.full((B * T, 3 * D + AUG), FILL_BF16, dtype=torch.bfloat16, device=DEV)
    good = [N.ptr(qkv), N.ptr(out), N.ptr(dout), N.ptr(lse), N.ptr(delta), N.ptr(dqkv), 3 * D + AUG, B, T, heads, N.stream()]

    def call(**change):
        a = list(good)
        for i, val in change.items():
            a[int(i[1:])] = val
        return lib.ucod_attention_bwd(*a)

    assert call(_6=3 * D - 8) == EINVAL                                 # ld_dqkv < 3D
    assert call(_6=3 * D + 4) == EINVAL                                 # ld_dqkv not a multiple of 8
    for i in range(6):                                                  # each NULL pointer in turn
        assert call(**{f"_{i}": None}) == EINVAL, i
    assert call(_6=1 << 30, _8=1) == EINVAL                             # tok * ld_dqkv * 2 bytes = 2 GiB: past the 32-bit byte offsets of the stores
    for i in (7, 8, 9):                                                 # B, tok, heads of 0
        assert call(**{f"_{i}": 0}) == EINVAL, i
    torch.cuda.synchronize()
    assert bool((dqkv == FILL_BF16).all()) and bool((delta == FILL_F32).all())
    assert call() == 0                                                  # and the unchanged set is accepted
    torch.cuda.synchronize()
