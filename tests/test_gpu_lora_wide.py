"""GPU: the wide forms of the LoRA row kernels (include/ucod_dpl.h: UCOD_LORA_WIDE, the _wide entry points) -- the MLP input's gradient kernel at
8192 < N1 <= UCOD_LORA_WIDE_MAX_N1 (five vectors per thread, one rank per pass), the output projection's forward at 4096 < K <= UCOD_LORA_WIDE_MAX_K (blocks of 512
threads), and grad_s / both grad_x forms / the packs with their width guard lifted -- against f64 on the same bf16-rounded operands, with canaries around every
output, each run twice and bit-identical.  DINOv3 ViT-H+/16 is N1 = 10240, K = 5120, D = 1280.

Bars are the narrow forms' (tests/test_gpu_lora_mlp_pair.py, test_gpu_lora_out.py, test_gpu_lora_swiglu_out.py), taken over unchanged: t 1e-2, dA (from the t the
kernel wrote) and dB 2e-4, cotangent 1e-2, relative to max(1, |ref|max); u 1e-2, f32 stream row 2e-5, fp16 row 2e-5 + 2^-11.

The gradient cases reach every instantiation the wide launch can select (tests/test_lora_wide_host.py restates the dispatch): N1 = 8448 is the first width past the
old limit (33 of the fifth vector's 256 lanes live), 10240 the ceiling; D = 128 / 768 / 1280 and 1536 are 1, 2 and 3 column pairs per thread; r = 1, 2, 3, 8 passes;
37 rows end inside a 4-row group, 1029 are one group above the 256-block cap; both module counts.  At N1 <= 8192 / K <= 4096 every wide entry point is the narrow
one bit for bit.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as TF

from conftest import maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402
from oracle import vit as OV  # noqa: E402
from test_gpu_lora_targets import Guarded, FlatGuarded, drop_arg  # noqa: E402
from test_gpu_lora_mlp_pair import operands, gate_rows, run_grad, SCALING, SEED, LAYER  # noqa: E402
import test_gpu_lora_out as TO  # noqa: E402
import test_gpu_lora_swiglu_out as TS  # noqa: E402
from lora_wide_cases import WIDE_GRAD_CASES, WIDE_FWD_SHAPES, WIDE_FWD_RANKS, WIDE_OUT_GRAD_SHAPES, WIDE_OUT_GRAD_RANKS, MAX_N1, MAX_K  # noqa: E402

DEV = "cuda"
AUG, W = N.LORA_AUG, N.LORA_OUT_W
EINVAL, ENOMEM = -1, -2


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def mlp_fns(lib, modules, wide=True):
    names = ("ucod_lora_mlp_pair_grad_workspace_bytes", "ucod_lora_mlp_pair_grad") if modules == 2 else ("ucod_lora_mlp_grad_workspace_bytes", "ucod_lora_mlp_grad")
    return tuple(getattr(lib, n + ("_wide" if wide else "")) for n in names)


def run_grad_wide(o, M, N1, D, r, p_drop, modules=2):
    """tests/test_gpu_lora_mlp_pair.py::run_grad through the wide entry points"""
    wsf, fn = mlp_fns(N.load(), modules)
    wsb = wsf(N1, D)
    if N1 > 8192:
        assert wsb == 256 * (modules * D + N1) * 4               # one rank per pass: [modules][D] | [N1] per block, 256 blocks
    ws = FlatGuarded(wsb // 4)
    t, grad = Guarded(M, AUG, torch.bfloat16), Guarded(1, r * (modules * D + N1), torch.float32)
    rc = fn(N.ptr(o["dpre"]), N.ptr(o["h_aug"]), N.ptr(o["flat"]), r, SCALING, grad.ptr(), t.ptr(), ws.ptr(), wsb, M, N1, D, drop_arg(p_drop, SEED, LAYER), N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert t.guards_intact() and grad.guards_intact() and ws.guards_intact(), "wrote outside its outputs"
    return t.payload.clone(), grad.payload.clone().reshape(-1)


# ------------------------------------------------------------------------------------------------ 1. the MLP input's gradient kernel, N1 > 8192
@pytest.mark.parametrize("modules", [2, 1])
@pytest.mark.parametrize("N1,D,r,M,p_drop", WIDE_GRAD_CASES)
def test_lora_mlp_grad_wide(N1, D, r, M, p_drop, modules):
    o = operands(M, N1, D, r, p_drop, modules=modules)
    runs = [run_grad_wide(o, M, N1, D, r, p_drop, modules) for _ in range(2)]
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16)) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    t_out, grad = runs[0][0].float().cpu(), runs[0][1].cpu()
    assert bool(torch.isfinite(t_out).all()) and bool(torch.isfinite(grad).all()), "left elements unwritten"
    assert float(t_out[:, modules * r:].abs().max()) == 0.0     # the unused aug columns
    e_t = maxdiff(t_out[:, :modules * r], o["t_ref"]) / max(1.0, o["t_ref"].abs().max().item())
    gA, gB = grad[:modules * r * D].reshape(modules, r, D), grad[modules * r * D:].reshape(N1, r)
    e_a = 0.0
    for p in range(modules):                                     # dA_p = t_p^T drop_p(h), from the bf16 t the kernel wrote, under mask p
        dA_ref = (t_out[:, p * r:(p + 1) * r].double().to(DEV).t() @ o["hd"][p]).cpu()
        e_a = max(e_a, maxdiff(gA[p], dA_ref) / max(1.0, dA_ref.abs().max().item()))
        assert float(gA[p].abs().max()) > 0
    e_b = maxdiff(gB, o["dB_ref"]) / max(1.0, o["dB_ref"].abs().max().item())
    print(f"lora_mlp_grad_wide, {modules} module(s) {(M, N1, D, r)} p={p_drop}: t {e_t:.2e} (bar 1e-2) dA {e_a:.2e} (2e-4) dB {e_b:.2e} (2e-4)")
    assert e_t < 1e-2 and e_a < 2e-4 and e_b < 2e-4, (e_t, e_a, e_b)
    # the columns past 8192 are in t: the sum over the first 8192 alone is far away
    d64, b64 = o["dpre"].double(), o["flat"][modules * r * D:].reshape(N1, r).double()
    gd = gate_rows(N1).to(DEV) if modules == 2 else torch.ones(N1, dtype=torch.bool, device=DEV)
    first = (torch.arange(N1, device=DEV) < 8192) & gd
    short = (SCALING * d64[:, first] @ b64[first]).cpu()
    assert maxdiff(t_out[:, :r], short) / max(1.0, o["t_ref"].abs().max().item()) > 3e-2
    assert float(gB[8192:].abs().max()) > 0 and float(gB[N1 - 8:].abs().max()) > 0          # ... and so are their rows of dB, the last vector's included


def test_an_untargeted_module_of_the_wide_pair_has_exact_zero_gradients():
    N1, D, r, M, p_drop = MAX_N1, 768, 3, 37, 0.05
    both = run_grad_wide(operands(M, N1, D, r, p_drop), M, N1, D, r, p_drop)
    gate = gate_rows(N1).to(DEV)
    for p, live in enumerate(((True, False), (False, True))):     # p: the live module
        t, grad = run_grad_wide(operands(M, N1, D, r, p_drop, live), M, N1, D, r, p_drop)
        gA, gB = grad[:2 * r * D].reshape(2, r, D), grad[2 * r * D:].reshape(N1, r)
        mine, dead = (gate, ~gate) if p == 0 else (~gate, gate)
        assert float(gA[1 - p].abs().max()) == 0.0 and float(gB[dead].abs().max()) == 0.0 and float(t[:, (1 - p) * r:(2 - p) * r].float().abs().max()) == 0.0
        bA, bB = both[1][:2 * r * D].reshape(2, r, D), both[1][2 * r * D:].reshape(N1, r)
        assert torch.equal(gA[p], bA[p]) and torch.equal(gB[mine], bB[mine]), "the live module's gradients depend on its partner"
        assert torch.equal(t[:, p * r:(p + 1) * r].view(torch.int16), both[0][:, p * r:(p + 1) * r].view(torch.int16)) and float(gA[p].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2. the output projection's forward, K > 4096
@functools.lru_cache(maxsize=2)
def fwd_operands(M, K, D, p_drop):
    """bf16-rounded operands of one shape for every rank (A, B: the first r of 8 ranks), computed once, never modified"""
    g = torch.Generator().manual_seed(M + K + D)
    A = torch.randn(W, K, generator=g) / math.sqrt(K)
    Bo = torch.randn(D, W, generator=g) * 0.3
    lam = torch.rand(D, generator=g) + 0.5
    x_in = torch.randn(M, K, generator=g).bfloat16()
    x0 = torch.randn(M, D, generator=g) * 2
    mask = OV.lora_dropout_mask(TO.SEED, TO.KEY, 0, M, K, p_drop).double().reshape(M, K) if p_drop > 0 else None
    xd = x_in.double() if mask is None else x_in.double() * mask
    return dict(A=A, B=Bo, lam=lam, x_in=x_in, x0=x0, u_all=xd @ A.double().t(), u_nomask=x_in.double() @ A.double().t())


@pytest.mark.parametrize("h16", [False, True])
@pytest.mark.parametrize("r", WIDE_FWD_RANKS)
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("M,K,D", WIDE_FWD_SHAPES)
def test_lora_out_fwd_wide(M, K, D, p_drop, r, h16):
    o = fwd_operands(M, K, D, p_drop)
    lib = N.load()
    A, Bo = o["A"][:r].contiguous(), o["B"][:, :r].contiguous()
    flat = torch.cat((A.reshape(-1), Bo.reshape(-1))).to(DEV)
    x0 = o["x0"].half() if h16 else o["x0"]
    u_ref = o["u_all"][:, :r]
    x_ref = x0.double() + o["lam"].double() * (2.0 * u_ref @ Bo.double().t())
    xin, lam = o["x_in"].to(DEV), o["lam"].to(DEV)
    runs = []
    for _ in range(2):
        xs, u = TO.Guarded(M, D, x0.dtype, fill=x0.to(DEV)), Guarded(M, W, torch.float32)
        rc = lib.ucod_lora_out_fwd_wide(N.ptr(xin), N.ptr(flat), r, 2.0, N.ptr(lam), xs.ptr(), int(h16), u.ptr(), M, K, D, drop_arg(p_drop, TO.SEED, TO.KEY), N.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert xs.guards_intact() and u.guards_intact(), "wrote outside its outputs"
        runs.append((xs.payload.clone(), u.payload.clone()))
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    xg, ug = runs[0][0].double().cpu(), runs[0][1].cpu()
    assert bool(torch.isfinite(ug).all()) and bool(torch.isfinite(xg).all()), "left elements unwritten"
    if r < W:
        assert float(ug[:, r:].abs().max()) == 0.0               # the columns beyond the rank
    e_u = maxdiff(ug[:, :r], u_ref) / max(1.0, u_ref.abs().max().item())
    e_x = maxdiff(xg, x_ref) / max(1.0, x_ref.abs().max().item())
    bar_x = 2e-5 + (2.0 ** -11 if h16 else 0.0)
    print(f"lora_out_fwd_wide {(M, K, D, r)} p={p_drop} h16={h16}: u {e_u:.2e} (bar 1e-2), stream {e_x:.2e} (bar {bar_x:.2e})")
    assert e_u < 1e-2 and e_x < bar_x, (e_u, e_x)
    assert maxdiff(xg, x0.double()) > 0.1                        # the update is there
    short = (o["x_in"][:, :4096].double() @ A[:, :4096].double().t())
    assert p_drop > 0 or maxdiff(ug[:, :r], short) > 0.05        # ... with the columns past 4096 in it
    if p_drop > 0:                                               # ... and under the mask
        assert maxdiff(ug[:, :r], o["u_nomask"][:, :r]) > 0.05
    xs = TO.Guarded(M, D, x0.dtype, fill=x0.to(DEV))             # the no-grad form (u not stored) gives the same stream, bit for bit
    assert lib.ucod_lora_out_fwd_wide(N.ptr(xin), N.ptr(flat), r, 2.0, N.ptr(lam), xs.ptr(), int(h16), None, M, K, D, drop_arg(p_drop, TO.SEED, TO.KEY), N.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(xs.payload), bits(runs[0][0])) and xs.guards_intact()


# ------------------------------------------------------------------------------------------------ 3. grad_s and both grad_x forms, K > 4096
def run_out_grads(o, pre, cot0, act, flags, r, M, K, D, p_drop, wide=True):
    """ucod_lora_out_grad_s(_wide), then ucod_lora_out_grad_x_ex(flags) on ``pre`` and a copy of ``cot0``, with canaries -> (t, grad, cotangent)"""
    lib = N.load()
    wsb = (lib.ucod_lora_out_grad_workspace_bytes_wide if wide else lib.ucod_lora_out_grad_workspace_bytes)(r, K, D)
    assert wsb == max(512 * D * r, 256 * r * K) * 4
    gs = lib.ucod_lora_out_grad_s_wide if wide else lib.ucod_lora_out_grad_s
    ws = FlatGuarded(wsb // 4)
    t, grad, cot = Guarded(M, W, torch.float32), Guarded(1, r * (K + D), torch.float32), TO.Guarded(M, cot0.shape[1], torch.bfloat16, fill=cot0)
    rc = gs(N.ptr(o["s_dev"]), N.ptr(o["u_dev"]), N.ptr(o["flat"]), r, o["scaling"], grad.ptr(), t.ptr(), ws.ptr(), wsb, M, K, D, N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(grad.payload.reshape(-1)[:r * K]).all()), "grad_s wrote into the A part"
    rc = lib.ucod_lora_out_grad_x_ex(N.ptr(pre), act, flags, cot.ptr(), t.ptr(), N.ptr(o["flat"]), r, grad.ptr(), ws.ptr(), wsb, M, K, D,
                                     drop_arg(p_drop, TO.SEED, TO.KEY), N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert t.guards_intact() and grad.guards_intact() and cot.guards_intact() and ws.guards_intact(), "wrote outside its outputs"
    return t.payload.clone(), grad.payload.clone(), cot.payload.clone()


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("r", WIDE_OUT_GRAD_RANKS)
@pytest.mark.parametrize("M,K,D,K0", WIDE_OUT_GRAD_SHAPES)
def test_lora_out_grad_swiglu_wide(M, K, D, K0, r, p_drop):
    """tests/test_gpu_lora_swiglu_out.py::test_lora_out_grad_swiglu past K = 4096: padded units (hidden 4200 in 4224) give exact zeros and leave dpre untouched"""
    o = dict(TS.operands(M, K, D, K0, r, p_drop))
    o["s_dev"], o["u_dev"] = o["s"].to(DEV), o["u"].to(DEV)
    pre, cot0 = TS.interleave(o["x1"], o["x2"]).to(DEV), o["cot"].to(DEV)
    runs = [run_out_grads(o, pre, cot0, N.LORA_OUT_ACT_SWIGLU, N.LORA_OUT_SWIGLU | N.LORA_WIDE, r, M, K, D, p_drop) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(bits(a), bits(b)), "two runs differ"
    t_out, grad, cot_out = runs[0][0].cpu(), runs[0][1].cpu().reshape(-1), runs[0][2].double().cpu()
    assert bool(torch.isfinite(t_out).all()) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(cot_out).all()), "left elements unwritten"
    if r < W:
        assert float(t_out[:, r:].abs().max()) == 0.0
    tk = t_out[:, :r].double()
    t_ref = o["scaling"] * o["s"].double() @ o["B"]
    dB_ref = o["scaling"] * o["s"].double().t() @ o["u"][:, :r].double()
    dA_ref, d1, d2 = TS.branch_grads(o, tk)                     # (dA from the t the kernel wrote)
    c1, c2 = TS.deinterleave(o["cot"].double())
    cot_ref = TS.interleave(c1 + d1, c2 + d2)
    gA, gB = grad[:r * K].reshape(r, K), grad[r * K:].reshape(D, r)
    e_t = maxdiff(tk, t_ref) / max(1.0, t_ref.abs().max().item())
    e_a = maxdiff(gA, dA_ref) / max(1.0, dA_ref.abs().max().item())
    e_b = maxdiff(gB, dB_ref) / max(1.0, dB_ref.abs().max().item())
    e_c = maxdiff(cot_out, cot_ref) / max(1.0, cot_ref.abs().max().item())
    print(f"lora_out_grad swiglu wide {(M, K, D, r)} p={p_drop}: t {e_t:.2e} (bar 1e-2) dA {e_a:.2e} (2e-4) dB {e_b:.2e} (2e-4) dpre {e_c:.2e} (1e-2)")
    assert e_t < 1e-2 and e_a < 2e-4 and e_b < 2e-4 and e_c < 1e-2, (e_t, e_a, e_b, e_c)
    assert float(gA[:, 4096:K0].abs().max()) > 0 and float(gB.abs().max()) > 0 and maxdiff(cot_out, o["cot"].double()) > 0.05
    if K0 < K:                                                   # padded units: dA exactly zero, dpre untouched bit for bit
        assert float(gA[:, K0:].abs().max()) == 0.0
        got1, got2 = TS.deinterleave(runs[0][2].cpu())
        assert torch.equal(bits(got1[:, K0:]), bits(TS.deinterleave(o["cot"])[0][:, K0:])) and torch.equal(bits(got2[:, K0:]), bits(TS.deinterleave(o["cot"])[1][:, K0:]))
    x1 = o["x1"].double()                                        # teeth: dA from silu(x1) alone is far from what the kernel gave
    assert maxdiff(gA, tk.t() @ (TF.silu(x1) * o["mask"])) / max(1.0, dA_ref.abs().max().item()) > 1e-2


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("r", WIDE_OUT_GRAD_RANKS)
@pytest.mark.parametrize("M,K,D,K0", WIDE_OUT_GRAD_SHAPES)
def test_lora_out_grad_gelu_wide(M, K, D, K0, r, p_drop):
    """tests/test_gpu_lora_out.py::test_lora_out_grad (the GELU form: the plain MLP's fc2 / down_proj) past K = 4096"""
    o = dict(TO.operands(M, K, D, r, p_drop))
    g = torch.Generator().manual_seed(K + r)
    u = torch.full((M, W), 55.0)                                 # columns beyond the rank are never read
    u[:, :r] = torch.randn(M, r, generator=g)
    o["s_dev"], o["u_dev"] = o["s"].to(DEV), u.to(DEV)
    x = o["x_in"].double()
    xa = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    da = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    runs = [run_out_grads(o, o["x_in"].to(DEV), o["cot"].to(DEV), N.LORA_OUT_ACT_GELU, N.LORA_WIDE, r, M, K, D, p_drop) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(bits(a), bits(b)), "two runs differ"
    t_out, grad, cot_out = runs[0][0].cpu(), runs[0][1].cpu().reshape(-1), runs[0][2].double().cpu()
    assert bool(torch.isfinite(t_out).all()) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(cot_out).all()), "left elements unwritten"
    tk = t_out[:, :r].double()
    t_ref = o["scaling"] * o["s"].double() @ o["B"]
    dB_ref = o["scaling"] * o["s"].double().t() @ u[:, :r].double()
    dA_ref = tk.t() @ (xa * o["mask"])
    cot_ref = o["cot"].double() + da * o["mask"] * (tk @ o["A"])
    gA, gB = grad[:r * K].reshape(r, K), grad[r * K:].reshape(D, r)
    e_t = maxdiff(tk, t_ref) / max(1.0, t_ref.abs().max().item())
    e_a = maxdiff(gA, dA_ref) / max(1.0, dA_ref.abs().max().item())
    e_b = maxdiff(gB, dB_ref) / max(1.0, dB_ref.abs().max().item())
    e_c = maxdiff(cot_out, cot_ref) / max(1.0, cot_ref.abs().max().item())
    print(f"lora_out_grad gelu wide {(M, K, D, r)} p={p_drop}: t {e_t:.2e} (bar 1e-2) dA {e_a:.2e} (2e-4) dB {e_b:.2e} (2e-4) cotangent {e_c:.2e} (1e-2)")
    assert e_t < 1e-2 and e_a < 2e-4 and e_b < 2e-4 and e_c < 1e-2, (e_t, e_a, e_b, e_c)
    assert float(gA[:, 4096:].abs().max()) > 0 and float(gB.abs().max()) > 0 and maxdiff(cot_out[:, 4096:], o["cot"].double()[:, 4096:]) > 0.05


# ------------------------------------------------------------------------------------------------ 4. the packs
@pytest.mark.parametrize("modules", [2, 1])
@pytest.mark.parametrize("N1,D,r", [(8448, 128, 3), (MAX_N1, 1280, 8)])
def test_pack_wide(N1, D, r, modules):
    g = torch.Generator().manual_seed(N1 + r)
    flat = torch.randn(modules * r * D + N1 * r, generator=g)
    Bm = flat[modules * r * D:].reshape(N1, r)
    w = Guarded(N1, D + AUG, torch.bfloat16)
    w.payload.copy_(torch.randn(N1, D + AUG, generator=g).bfloat16())
    before = w.payload.clone()
    fl = flat.to(DEV)
    lib = N.load()
    assert (lib.ucod_lora_mlp_pair_pack_wide if modules == 2 else lib.ucod_lora_mlp_pack_wide)(N.ptr(fl), r, SCALING, w.ptr(), N1, D, N.stream()) == 0
    torch.cuda.synchronize()
    assert w.guards_intact() and torch.equal(w.payload[:, :D].view(torch.int16), before[:, :D].view(torch.int16)), "touched the weight or its surroundings"
    want = torch.zeros(N1, AUG, dtype=torch.bfloat16)
    gate = gate_rows(N1) if modules == 2 else torch.ones(N1, dtype=torch.bool)
    want[gate, :r] = (SCALING * Bm[gate]).bfloat16()
    if modules == 2:
        want[~gate, r:2 * r] = (SCALING * Bm[~gate]).bfloat16()
    assert torch.equal(w.payload[:, D:].cpu().view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------ 5. at narrow widths the wide entry points are the narrow ones
@pytest.mark.parametrize("modules", [2, 1])
@pytest.mark.parametrize("N1,D,r,M,p_drop", [(8192, 128, 3, 37, 0.0), (8192, 1536, 2, 1029, 0.05), (1024, 768, 2, 37, 0.05)])
def test_narrow_mlp_grad_through_the_wide_entry_point_is_bit_identical(N1, D, r, M, p_drop, modules):
    lib = N.load()
    assert mlp_fns(lib, modules)[0](N1, D) == mlp_fns(lib, modules, False)[0](N1, D) > 0
    o = operands(M, N1, D, r, p_drop, modules=modules)
    (t0, g0), (t1, g1) = run_grad(o, M, N1, D, r, p_drop, modules), run_grad_wide(o, M, N1, D, r, p_drop, modules)
    assert torch.equal(bits(t0), bits(t1)) and torch.equal(g0, g1)


@pytest.mark.parametrize("h16", [False, True])
@pytest.mark.parametrize("M,K,D,r,p_drop", [(111, 4096, 1536, 8, 0.5), (111, 3072, 768, 2, 0.0), (111, 512, 128, 2, 0.5)])
def test_narrow_out_kernels_through_the_wide_entry_points_are_bit_identical(M, K, D, r, p_drop, h16):
    lib = N.load()
    o = dict(TO.operands(M, K, D, r, p_drop))
    assert lib.ucod_lora_out_grad_workspace_bytes_wide(r, K, D) == lib.ucod_lora_out_grad_workspace_bytes(r, K, D) > 0
    x0 = o["x0"].half() if h16 else o["x0"]
    xin, lam = o["x_in"].to(DEV), o["lam"].to(DEV)
    got = []
    for fn in (lib.ucod_lora_out_fwd, lib.ucod_lora_out_fwd_wide):
        xs, u = TO.Guarded(M, D, x0.dtype, fill=x0.to(DEV)), Guarded(M, W, torch.float32)
        assert fn(N.ptr(xin), N.ptr(o["flat"]), r, 2.0, N.ptr(lam), xs.ptr(), int(h16), u.ptr(), M, K, D, drop_arg(p_drop, TO.SEED, TO.KEY), N.stream()) == 0
        torch.cuda.synchronize()
        got.append((xs.payload.clone(), u.payload.clone()))
    assert torch.equal(bits(got[0][0]), bits(got[1][0])) and torch.equal(got[0][1], got[1][1])
    if h16:
        return
    u = torch.full((M, W), 55.0)
    u[:, :r] = torch.randn(M, r, generator=torch.Generator().manual_seed(K + r))
    o["s_dev"], o["u_dev"] = o["s"].to(DEV), u.to(DEV)
    narrow = run_out_grads(o, xin, o["cot"].to(DEV), N.LORA_OUT_ACT_GELU, 0, r, M, K, D, p_drop, wide=False)
    wide = run_out_grads(o, xin, o["cot"].to(DEV), N.LORA_OUT_ACT_GELU, N.LORA_WIDE, r, M, K, D, p_drop)
    for a, b in zip(narrow, wide):
        assert torch.equal(bits(a), bits(b))


def test_narrow_pack_through_the_wide_entry_point_is_bit_identical():
    N1, D, r = 8192, 256, 3
    lib = N.load()
    flat = torch.randn(2 * r * D + N1 * r, generator=torch.Generator().manual_seed(5)).to(DEV)
    for narrow, wide in ((lib.ucod_lora_mlp_pack, lib.ucod_lora_mlp_pack_wide), (lib.ucod_lora_mlp_pair_pack, lib.ucod_lora_mlp_pair_pack_wide)):
        a, b = (torch.full((N1, D + AUG), 3.0, dtype=torch.bfloat16, device=DEV) for _ in range(2))
        assert narrow(N.ptr(flat), r, SCALING, N.ptr(a), N1, D, N.stream()) == 0 and wide(N.ptr(flat), r, SCALING, N.ptr(b), N1, D, N.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(bits(a), bits(b)) and bool((b[:, :D] == 3.0).all())


# ------------------------------------------------------------------------------------------------ 6. refusals write nothing
def test_wide_refusals_write_nothing():
    M, N1, D, K, r = 37, MAX_N1, 128, 5120, 2
    lib, P, st = N.load(), N.ptr, N.stream()
    o = operands(M, N1, D, r, 0.0)
    wsb = max(lib.ucod_lora_mlp_pair_grad_workspace_bytes_wide(N1, D), lib.ucod_lora_out_grad_workspace_bytes_wide(r, K, D))
    ws = torch.full((wsb // 4,), 3.0, device=DEV)
    t, grad = torch.full((M, AUG), 3.0, dtype=torch.bfloat16, device=DEV), torch.full((9 * (2 * 1664 + MAX_N1 + 128 + MAX_K + 128),), 3.0, device=DEV)
    w_aug = torch.full((MAX_N1 + 128, D + AUG), 3.0, dtype=torch.bfloat16, device=DEV)
    xs, u, cot = torch.full((M, 1664), 3.0, device=DEV), torch.full((M, W), 3.0, device=DEV), torch.full((M, 2 * (MAX_K + 128)), 3.0, dtype=torch.bfloat16, device=DEV)
    xin = torch.zeros(M, 2 * (MAX_K + 128), dtype=torch.bfloat16, device=DEV)

    def mg(fn=lib.ucod_lora_mlp_pair_grad_wide, dpre=P(o["dpre"]), h=P(o["h_aug"]), lora=P(o["flat"]), rr=r, g=P(grad), tt=P(t), w=P(ws), wb=wsb, n1=N1, d=D):
        return fn(dpre, h, lora, rr, SCALING, g, tt, w, wb, M, n1, d, None, st)

    def pk(fn=lib.ucod_lora_mlp_pair_pack_wide, lora=P(o["flat"]), wp=P(w_aug), rr=r, n1=N1):
        return fn(lora, rr, SCALING, wp, n1, D, st)

    def fwd(xp=P(xin), a=P(o["flat"]), sp=P(xs), rr=r, k=K, d=D):
        return lib.ucod_lora_out_fwd_wide(xp, a, rr, 2.0, None, sp, 0, P(u), M, k, d, None, st)

    def gs(sp=P(xin), up=P(u), rr=r, k=K, d=D, wb=wsb):
        return lib.ucod_lora_out_grad_s_wide(sp, up, P(o["flat"]), rr, 2.0, P(grad), P(u), P(ws), wb, M, k, d, st)

    def gx(xp=P(xin), cp=P(cot), act=N.LORA_OUT_ACT_GELU, fl=N.LORA_WIDE, rr=r, k=K, d=D, wb=wsb):
        return lib.ucod_lora_out_grad_x_ex(xp, act, fl, cp, P(u), P(o["flat"]), rr, P(grad), P(ws), wb, M, k, d, None, st)

    need_m, need_o = lib.ucod_lora_mlp_pair_grad_workspace_bytes_wide(N1, D), lib.ucod_lora_out_grad_workspace_bytes_wide(r, K, D)
    calls = {"mlp past the ceiling": lambda: mg(n1=MAX_N1 + 128), "mlp single past the ceiling": lambda: mg(fn=lib.ucod_lora_mlp_grad_wide, n1=MAX_N1 + 128),
             "mlp N1 % 128": lambda: mg(n1=MAX_N1 - 64), "mlp rank 9": lambda: mg(rr=9), "mlp D = 1664": lambda: mg(d=1664), "mlp null dpre": lambda: mg(dpre=None),
             "mlp null h": lambda: mg(h=None), "mlp null lora": lambda: mg(lora=None), "mlp null grad": lambda: mg(g=None), "mlp null t": lambda: mg(tt=None),
             "mlp null workspace": lambda: mg(w=None), "mlp small workspace": lambda: mg(wb=need_m - 1),
             "pack past the ceiling": lambda: pk(n1=MAX_N1 + 128), "single pack past the ceiling": lambda: pk(fn=lib.ucod_lora_mlp_pack_wide, n1=MAX_N1 + 128),
             "pack rank 9": lambda: pk(rr=9), "pack null lora": lambda: pk(lora=None), "pack null weight": lambda: pk(wp=None),
             "fwd past the ceiling": lambda: fwd(k=MAX_K + 128), "fwd K % 128": lambda: fwd(k=K - 64), "fwd rank 9": lambda: fwd(rr=9), "fwd D = 1664": lambda: fwd(d=1664),
             "fwd null x": lambda: fwd(xp=None), "fwd null lora": lambda: fwd(a=None), "fwd null stream": lambda: fwd(sp=None),
             "grad_s past the ceiling": lambda: gs(k=MAX_K + 128), "grad_s rank 9": lambda: gs(rr=9), "grad_s D = 1664": lambda: gs(d=1664), "grad_s null s": lambda: gs(sp=None),
             "grad_s null u": lambda: gs(up=None), "grad_s small workspace": lambda: gs(wb=need_o - 1),
             "grad_x past the ceiling": lambda: gx(k=MAX_K + 128), "grad_x K = 5120 without the bit": lambda: gx(fl=0), "grad_x unknown bit beside 16": lambda: gx(fl=N.LORA_WIDE | 2),
             "grad_x unknown bit 8": lambda: gx(fl=N.LORA_WIDE | 8), "grad_x swiglu without its flag": lambda: gx(act=N.LORA_OUT_ACT_SWIGLU),
             "grad_x swiglu without the wide bit": lambda: gx(act=N.LORA_OUT_ACT_SWIGLU, fl=N.LORA_OUT_SWIGLU), "grad_x rank 9": lambda: gx(rr=9), "grad_x D = 1664": lambda: gx(d=1664),
             "grad_x K % 128": lambda: gx(k=K - 64), "grad_x null x": lambda: gx(xp=None), "grad_x null cot": lambda: gx(cp=None), "grad_x small workspace": lambda: gx(wb=need_o - 1)}
    for name, call in calls.items():
        assert call() == (ENOMEM if "small workspace" in name else EINVAL), name
    f16 = N.load("f16")
    assert f16.ucod_lora_mlp_pair_grad_wide(P(o["dpre"]), P(o["h_aug"]), P(o["flat"]), r, SCALING, P(grad), P(t), P(ws), wsb, M, N1, D, None, st) != 0
    assert f16.ucod_lora_out_fwd_wide(P(xin), P(o["flat"]), r, 2.0, None, P(xs), 0, P(u), M, K, D, None, st) != 0
    torch.cuda.synchronize()
    for a in (ws, t, grad, w_aug, xs, u, cot):
        assert bool((a.float() == 3.0).all()), "a refused call wrote to its outputs"
