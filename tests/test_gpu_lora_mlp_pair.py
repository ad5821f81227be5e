"""GPU: the kernels of LoRA on the gated MLP's input -- gate_proj and up_proj as a pair on the fused, 4-interleaved weights_in (include/ucod_dpl.h:
ucod_layernorm_lora_mlp_pair, ucod_lora_mlp_pair_pack, ucod_lora_mlp_pair_grad, ucod_layernorm_bwd_lora_mlp_pair) -- against f64 on the same 16-bit-rounded
operands, with canary regions around every output.

Bars are the single module's (tests/test_gpu_lora_targets.py): t 1e-2, dA and dB 2e-4 relative to max(1, |ref|max), dA computed from the bf16 t the kernel wrote;
LayerNorm output 2e-2, u 1e-2; LayerNorm backward 2e-5 (dx) and 1e-2 (s).  tests/test_dinov3_lora_mlp_in_host.py shows the distances a wrong block structure
produces to be of order 1: here a gate element multiplied by an up row of B, a shared mask or a live cross block would miss the references by as much.

The gradient kernel is one template for the pair and for the single module (ucod_lora_mlp_grad: every fc1 / up_proj adapter): its cases run for both module counts,
the single module on the same dpre, h2 and B_m with every row its own, against the same references and bars.
The cases reach every instantiation of its launch function: N1 = 1024 / 3072 / 6144 / 8192 are 1, 2, 3 (in the 4 form) and 4 vectors per thread,
D = 128 / 768 / 1536 are 1, 2, 3 column pairs per thread -- every pair of the two occurs; r = 1 (half a pass live), 2 (one pass), 3 (odd tail), 8 (four passes)
each occur with every vector count; 37 rows end inside a 4-row group, 2053 (N1 <= 4096) / 1029 rows are one group above the block-stride cap.
"""
import functools
import math

import pytest
import torch

from conftest import maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402
from oracle import vit as OV  # noqa: E402
from test_gpu_lora_targets import Guarded, FlatGuarded, drop_arg  # noqa: E402

DEV = "cuda"
AUG = N.LORA_AUG
EINVAL, ENOMEM = -1, -2
SCALING, SEED, LAYER = 2.0, 0xFEEDC0DE1234, 14


def gate_rows(N1):
    return (torch.arange(N1) % 8) < 4


# (N1, D, r, rows, p_drop): the twelve (vectors, column pairs) combinations, r = 1, 2, 3, 8 with every N1, both row counts and both dropout settings with every N1
GRAD_CASES = [(1024, 128, 1, 37, 0.0), (1024, 768, 2, 2053, 0.05), (1024, 1536, 3, 37, 0.05), (1024, 128, 8, 2053, 0.0),
              (3072, 128, 2, 2053, 0.05), (3072, 768, 3, 37, 0.0), (3072, 1536, 8, 37, 0.05), (3072, 768, 1, 2053, 0.0),
              (6144, 128, 3, 1029, 0.0), (6144, 768, 8, 37, 0.05), (6144, 1536, 1, 37, 0.0), (6144, 1536, 2, 1029, 0.05),
              (8192, 128, 8, 37, 0.0), (8192, 768, 1, 1029, 0.05), (8192, 1536, 2, 37, 0.05), (8192, 128, 3, 1029, 0.0)]


def test_the_cases_cover_every_dispatch_case():
    nvt = lambda n1: -(-(n1 // 8) // 256)  # noqa: E731
    npt = lambda d: -(-(d // 2) // 256)  # noqa: E731
    assert {(nvt(c[0]), npt(c[1])) for c in GRAD_CASES} == {(v, p) for v in (1, 2, 3, 4) for p in (1, 2, 3)}
    assert {(nvt(c[0]), c[2]) for c in GRAD_CASES} == {(v, r) for v in (1, 2, 3, 4) for r in (1, 2, 3, 8)}
    for n1 in (1024, 3072, 6144, 8192):
        cap = 256 if n1 > 4096 else 512                          # blocks of the kernel's grid; a block walks 4 rows at a time
        rows = {c[3] for c in GRAD_CASES if c[0] == n1}
        assert rows == {37, 4 * cap + 5} and {c[4] for c in GRAD_CASES if c[0] == n1} == {0.0, 0.05}


@functools.lru_cache(maxsize=4)
def operands(M, N1, D, r, p_drop, live=(True, True), modules=2):
    """bf16-rounded operands of one case and the f64 references that do not depend on the kernel's output (computed once, never modified).  ``live``: which of
    (gate_proj, up_proj) is targeted -- the other has A = 0 and its rows of B = 0.  ``modules`` = 1: the single module on the same dpre, h and B_m -- every row is
    module 0's, A is the pair's A_g, the flat layout [A_m | B_m]."""
    g = torch.Generator().manual_seed(M + N1 + D + r)
    A = torch.randn(2, r, D, generator=g)[:modules] / math.sqrt(D)
    Bm = torch.randn(N1, r, generator=g) * 0.05
    dpre = torch.randn(M, N1, generator=g).bfloat16()
    h = torch.randn(M, D, generator=g).bfloat16()
    gate = gate_rows(N1) if modules == 2 else torch.ones(N1, dtype=torch.bool)
    for p, on in enumerate(live[:modules]):
        if not on:
            A[p] = 0.0
            Bm[gate if p == 0 else ~gate] = 0.0
    hd, u = [], []
    for p in range(modules):
        mask = OV.lora_dropout_mask(SEED, LAYER, p, M, D, p_drop).double() if p_drop > 0 else torch.ones(M, D, dtype=torch.float64)
        hd.append((h.double() * mask).to(DEV))
        u.append((hd[p] @ A[p].double().to(DEV).t()).bfloat16())
    h_aug = torch.zeros(M, D + AUG, dtype=torch.bfloat16, device=DEV)
    h_aug[:, :D], h_aug[:, D:D + modules * r] = h.to(DEV), torch.cat(u, 1)
    d64, b64, gd = dpre.double().to(DEV), Bm.double().to(DEV), gate.to(DEV)
    t_ref = torch.cat([SCALING * d64[:, rows] @ b64[rows] for rows in (gd, ~gd)[:modules]], 1)          # [M, modules r]: columns p r + j
    dB_ref = SCALING * torch.where(gd[:, None], d64.t() @ u[0].double(), d64.t() @ u[-1].double())       # each row against u of its own module
    return dict(flat=torch.cat((A.reshape(-1), Bm.reshape(-1))).to(DEV), dpre=dpre.to(DEV), h_aug=h_aug, hd=hd, t_ref=t_ref.cpu(), dB_ref=dB_ref.cpu(), gate=gate)


def run_grad(o, M, N1, D, r, p_drop, modules=2):
    lib = N.load()
    wsf, fn = (lib.ucod_lora_mlp_pair_grad_workspace_bytes, lib.ucod_lora_mlp_pair_grad) if modules == 2 else (lib.ucod_lora_mlp_grad_workspace_bytes, lib.ucod_lora_mlp_grad)
    wsb = wsf(N1, D)
    assert wsb == (256 if N1 > 4096 else 512) * 2 * (modules * D + N1) * 4
    ws = FlatGuarded(wsb // 4)
    t, grad = Guarded(M, AUG, torch.bfloat16), Guarded(1, r * (modules * D + N1), torch.float32)
    rc = fn(N.ptr(o["dpre"]), N.ptr(o["h_aug"]), N.ptr(o["flat"]), r, SCALING, grad.ptr(), t.ptr(), ws.ptr(), wsb, M, N1, D, drop_arg(p_drop, SEED, LAYER), N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert t.guards_intact() and grad.guards_intact() and ws.guards_intact(), "wrote outside its outputs"
    return t.payload.clone(), grad.payload.clone().reshape(-1)


def grad_params():
    """every case for the pair (under the ids the cases have always had) and for the single module"""
    for modules in (2, 1):
        for case in GRAD_CASES:
            name = "-".join(str(v) for v in case)
            yield pytest.param(*case, modules, id=name if modules == 2 else name + "-single")


@pytest.mark.parametrize("N1,D,r,M,p_drop,modules", grad_params())
def test_lora_mlp_pair_grad(N1, D, r, M, p_drop, modules):
    o = operands(M, N1, D, r, p_drop, modules=modules)
    runs = [run_grad(o, M, N1, D, r, p_drop, modules) for _ in range(2)]
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
        if p_drop > 0 and modules == 2:                          # ... and not under the other module's mask
            other = (t_out[:, p * r:(p + 1) * r].double().to(DEV).t() @ o["hd"][1 - p]).cpu()
            assert maxdiff(gA[p], other) > 100 * 2e-4 * max(1.0, dA_ref.abs().max().item())
    e_b = maxdiff(gB, o["dB_ref"]) / max(1.0, o["dB_ref"].abs().max().item())
    print(f"lora_mlp_grad, {modules} module(s) {(M, N1, D, r)} p={p_drop}: t {e_t:.2e} dA {e_a:.2e} dB {e_b:.2e}")
    assert e_t < 1e-2 and e_a < 2e-4 and e_b < 2e-4, (e_t, e_a, e_b)
    assert float(gB.abs().max()) > 0
    if modules == 2:
        assert float(gB[o["gate"]].abs().max()) > 0 and float(gB[~o["gate"]].abs().max()) > 0


@pytest.mark.parametrize("N1,D,r,M,p_drop", [(3072, 768, 3, 37, 0.05), (8192, 128, 2, 41, 0.0)])
def test_an_untargeted_module_of_the_pair_has_exact_zero_gradients(N1, D, r, M, p_drop):
    both = run_grad(operands(M, N1, D, r, p_drop), M, N1, D, r, p_drop)
    gate = gate_rows(N1).to(DEV)
    for p, live in enumerate(((True, False), (False, True))):     # p: the live module
        t, grad = run_grad(operands(M, N1, D, r, p_drop, live), M, N1, D, r, p_drop)
        gA, gB = grad[:2 * r * D].reshape(2, r, D), grad[2 * r * D:].reshape(N1, r)
        mine, dead = (gate, ~gate) if p == 0 else (~gate, gate)
        assert float(gA[1 - p].abs().max()) == 0.0 and float(gB[dead].abs().max()) == 0.0 and float(t[:, (1 - p) * r:(2 - p) * r].float().abs().max()) == 0.0
        bA, bB = both[1][:2 * r * D].reshape(2, r, D), both[1][2 * r * D:].reshape(N1, r)
        assert torch.equal(gA[p], bA[p]) and torch.equal(gB[mine], bB[mine]), "the live module's gradients depend on its partner"
        assert torch.equal(t[:, p * r:(p + 1) * r].view(torch.int16), both[0][:, p * r:(p + 1) * r].view(torch.int16)) and float(gA[p].abs().max()) > 0


def test_refusals_write_nothing():
    M, N1, D, r = 37, 1024, 128, 2
    o = operands(M, N1, D, r, 0.0)
    lib = N.load()
    wsb = lib.ucod_lora_mlp_pair_grad_workspace_bytes(N1, D)
    ws = torch.full((wsb // 4,), 3.0, device=DEV)
    t, grad = torch.full((M, AUG), 3.0, dtype=torch.bfloat16, device=DEV), torch.full((9 * (2 * 1664 + 8320),), 3.0, device=DEV)
    P = N.ptr

    def call(dpre=P(o["dpre"]), h=P(o["h_aug"]), lora=P(o["flat"]), rr=r, g=P(grad), tt=P(t), w=P(ws), wb=wsb, n1=N1, d=D):
        return lib.ucod_lora_mlp_pair_grad(dpre, h, lora, rr, SCALING, g, tt, w, wb, M, n1, d, None, N.stream())

    assert lib.ucod_lora_mlp_pair_grad_workspace_bytes(8320, D) == 0 and lib.ucod_lora_mlp_pair_grad_workspace_bytes(N1, 1664) == 0
    assert call(n1=8320) == EINVAL and call(d=1664) == EINVAL and call(rr=9) == EINVAL and call(wb=wsb - 4) == ENOMEM
    assert call(dpre=None) == EINVAL and call(h=None) == EINVAL and call(lora=None) == EINVAL and call(g=None) == EINVAL and call(tt=None) == EINVAL and call(w=None) == EINVAL
    assert N.load("f16").ucod_lora_mlp_pair_grad(P(o["dpre"]), P(o["h_aug"]), P(o["flat"]), r, SCALING, P(grad), P(t), P(ws), wsb, M, N1, D, None, N.stream()) != 0
    torch.cuda.synchronize()
    assert bool((ws == 3.0).all()) and bool((t == 3.0).all()) and bool((grad == 3.0).all())


# ------------------------------------------------------------------------------------------------ LayerNorm + the two down-projections
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("x16", [False, True])
@pytest.mark.parametrize("M,D,r", [(37, 128, 2), (45, 768, 3)])           # the 2-column and the 4-column form
def test_layernorm_lora_mlp_pair(M, D, r, x16, p_drop):
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    if x16:
        x = x.half()
    gam, bet = torch.randn(D, generator=g), torch.randn(D, generator=g)
    A = torch.randn(2, r, D, generator=g) / math.sqrt(D)
    out = Guarded(M, D + AUG, torch.bfloat16)
    xs, gs, bs, As = x.to(DEV), gam.to(DEV), bet.to(DEV), A.to(DEV)
    rc = N.load().ucod_layernorm_lora_mlp_pair(N.ptr(xs), int(x16), N.ptr(gs), N.ptr(bs), N.ptr(As), r, out.ptr(), M, D, 1e-6, drop_arg(p_drop, SEED, LAYER), N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.guards_intact(), "wrote outside its output"
    got = out.payload.float().cpu()
    assert bool(torch.isfinite(got).all()), "left elements unwritten"
    h = OV.layer_norm(x.double(), gam.double(), bet.double(), 1e-6)
    assert maxdiff(got[:, :D], h) < 2e-2 * max(1.0, h.abs().max().item())
    masks = [OV.lora_dropout_mask(SEED, LAYER, p, M, D, p_drop).double() if p_drop > 0 else torch.ones(M, D, dtype=torch.float64) for p in range(2)]
    for p in range(2):                                           # h2_aug[:, D + p r + j] = <drop_p(LN2 x), A_p[j]>
        u = (h * masks[p]) @ A[p].double().t()
        assert maxdiff(got[:, D + p * r:D + (p + 1) * r], u) < 1e-2 * max(1.0, u.abs().max().item())
        if p_drop > 0:                                           # its own mask: the other module's, and no mask at all, are far away
            assert maxdiff(got[:, D + p * r:D + (p + 1) * r], (h * masks[1 - p]) @ A[p].double().t()) > 0.05
            assert maxdiff(got[:, D + p * r:D + (p + 1) * r], h @ A[p].double().t()) > 0.05
    assert float(got[:, D + 2 * r:].abs().max()) == 0.0
    assert p_drop == 0 or not torch.equal(masks[0], masks[1])


# ------------------------------------------------------------------------------------------------ LayerNorm-2 backward with the two terms
def ln_bwd_case(M, D, r, p_drop, flags, live=(True, True), seed_shift=0):
    g = torch.Generator().manual_seed(M * 3 + D + r + seed_shift)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    gam, dy, dres = torch.randn(D, generator=g), torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    if flags & 1:
        dy = dy.bfloat16()
    if flags & 2:
        x = x.half()
    sc = torch.rand(D, generator=g) + 0.5
    A = torch.randn(2, r, D, generator=g) / math.sqrt(D)
    t = torch.full((M, AUG), 55.0, dtype=torch.bfloat16)         # columns beyond 2 r are never read
    t[:, :2 * r] = torch.randn(M, 2 * r, generator=g).bfloat16()
    for p, on in enumerate(live):
        if not on:
            t[:, p * r:(p + 1) * r] = 0.0
    dx, s = Guarded(M, D, torch.float32), Guarded(M, D, torch.bfloat16)
    dys, xs, gs, scs, drs, ts, As = (v.to(DEV) for v in (dy, x, gam, sc, dres, t, A))
    rc = N.load().ucod_layernorm_bwd_lora_mlp_pair(N.ptr(dys), N.ptr(xs), flags, N.ptr(gs), N.ptr(drs), N.ptr(scs), dx.ptr(), s.ptr(), M, D, 1e-6, N.ptr(ts), AUG, N.ptr(As),
                                                   r, drop_arg(p_drop, SEED, LAYER), N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert dx.guards_intact() and s.guards_intact()
    masks = [OV.lora_dropout_mask(SEED, LAYER, p, M, D, p_drop).double() if p_drop > 0 else torch.ones(M, D, dtype=torch.float64) for p in range(2)]

    def ref(mask_of=(0, 1)):
        """the plain backward applied to dy + sum_p mask_{mask_of[p]} (t_p A_p), formed in f64"""
        xr = x.float().double().requires_grad_(True)
        dy2 = dy.double() + sum(masks[mask_of[p]] * (t[:, p * r:(p + 1) * r].double() @ A[p].double()) for p in range(2))
        (gx,) = torch.autograd.grad((OV.layer_norm(xr, gam.double(), torch.zeros(D).double(), 1e-6) * dy2).sum(), xr)
        return gx + dres.double()

    return dx.payload.cpu(), s.payload.float().cpu(), ref, sc.double(), masks


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("r", [2, 3])                             # the rank known at compile time, and the loop
@pytest.mark.parametrize("M,D", [(37, 128), (45, 768)])
def test_layernorm_bwd_lora_mlp_pair(M, D, r, p_drop, flags):
    dx, s, ref_of, sc, masks = ln_bwd_case(M, D, r, p_drop, flags)
    ref = ref_of()
    assert maxdiff(dx, ref) < 2e-5 * max(1.0, ref.abs().max().item())
    assert maxdiff(s, ref * sc) < 1e-2 * max(1.0, (ref * sc).abs().max().item())
    if p_drop > 0:                                               # two masks, each on its own module's term
        assert not torch.equal(masks[0], masks[1])
        for wrong in ((0, 0), (1, 1), (1, 0)):
            assert maxdiff(dx, ref_of(wrong)) > 1e-2


@pytest.mark.parametrize("D", [128, 768])
def test_forward_and_backward_imply_the_same_mask_per_module(D):
    """Module p alone (the other's A, u and t at zero): the forward's u_p is <mask_p * h, A_p> and the backward's term is mask_p * (t_p A_p) for the SAME p -- each
    meets the reference under mask p and misses the one under mask 1 - p.  Same seed and key in both kernels, as the passes give them."""
    M, r, p_drop = 37, 2, 0.3
    for p, live in enumerate(((True, False), (False, True))):
        dx, _, ref_of, _, masks = ln_bwd_case(M, D, r, p_drop, 0, live, seed_shift=p)
        right, wrong = ref_of((p, p)), ref_of((1 - p, 1 - p))       # (only module p's term is live: the pair (p, p) puts mask p on it)
        assert maxdiff(dx, right) < 2e-5 * max(1.0, right.abs().max().item()) and maxdiff(dx, wrong) > 1e-2
        g = torch.Generator().manual_seed(D + p)
        x, gam, bet = torch.randn(M, D, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
        A = torch.zeros(2, r, D)
        A[p] = torch.randn(r, D, generator=g) / math.sqrt(D)
        out = torch.zeros(M, D + AUG, dtype=torch.bfloat16, device=DEV)
        xs, gs, bs, As = x.to(DEV), gam.to(DEV), bet.to(DEV), A.to(DEV)
        assert N.load().ucod_layernorm_lora_mlp_pair(N.ptr(xs), 0, N.ptr(gs), N.ptr(bs), N.ptr(As), r, N.ptr(out), M, D, 1e-6, drop_arg(p_drop, SEED, LAYER), N.stream()) == 0
        torch.cuda.synchronize()
        h = OV.layer_norm(x.double(), gam.double(), bet.double(), 1e-6)
        u = out[:, D + p * r:D + (p + 1) * r].float().cpu()
        u_right, u_wrong = (h * masks[p]) @ A[p].double().t(), (h * masks[1 - p]) @ A[p].double().t()
        assert maxdiff(u, u_right) < 1e-2 * max(1.0, u_right.abs().max().item()) and maxdiff(u, u_wrong) > 0.05
        assert float(out[:, D + (1 - p) * r:D + (2 - p) * r].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the pack
@pytest.mark.parametrize("N1,D,r", [(768, 128, 2), (3072, 384, 3), (1024, 256, 8)])
def test_pair_pack_puts_each_row_in_its_own_modules_columns(N1, D, r):
    g = torch.Generator().manual_seed(N1 + r)
    flat = torch.randn(2 * r * D + N1 * r, generator=g)
    Bm = flat[2 * r * D:].reshape(N1, r)
    w = Guarded(N1, D + AUG, torch.bfloat16)
    w.payload.copy_(torch.randn(N1, D + AUG, generator=g).bfloat16())
    before = w.payload.clone()
    fl = flat.to(DEV)
    assert N.load().ucod_lora_mlp_pair_pack(N.ptr(fl), r, SCALING, w.ptr(), N1, D, N.stream()) == 0
    torch.cuda.synchronize()
    assert w.guards_intact() and torch.equal(w.payload[:, :D].view(torch.int16), before[:, :D].view(torch.int16)), "touched the weight or its surroundings"
    aug = w.payload[:, D:].cpu()
    want = torch.zeros(N1, AUG, dtype=torch.bfloat16)
    gate = gate_rows(N1)
    want[gate, :r], want[~gate, r:2 * r] = (SCALING * Bm[gate]).bfloat16(), (SCALING * Bm[~gate]).bfloat16()
    assert torch.equal(aug.view(torch.int16), want.view(torch.int16))           # exactly the model's bf16 values; every column outside a row's own [D + p r, D + p r + r) zero
    assert float(aug[gate, r:].float().abs().max()) == 0.0 and float(aug[~gate, :r].float().abs().max()) == 0.0 and float(aug[:, 2 * r:].float().abs().max()) == 0.0
