"""GPU: the LoRA row kernels of csrc/vit_train.hip at every dispatch case against f64, through the C ABI only.

lora_rows_ref.py holds the reference, the rounding model the bf16 bounds come from, the restatement of launch_ln_lora / launch_ln_bwd and the case lists;
test_lora_rows_host.py shows on the CPU that the lists reach every instantiation and that the checker rejects the faults these cases are there for.  Here:

   1  test_ln_lora_every_instantiation            y, every u_p against its own projection's mask, zeros behind; the refused widths
   2  test_ln_lora_row_walk                       the block-stride walk: one live row in a wave, the second trip past 16 384 rows
   3  test_ln_bwd_every_instantiation             12 widths x 10 (entry, flags) forms; dres / next_scale / dropout rotate; the refused width and flags
   4  test_rank_*                                 the unrolled ranks and the generic loop; the LDS request at 64 KiB and the refusal past the device's LDS
   5  test_ln_bwd_aliasing_and_null_outputs       "dx may alias dres or dy; either output may be NULL", bit for bit
   6  test_dropout_extremes                       floor(1024 p) = 0 is no dropout, bit for bit; the clamp at 1023
   7  test_forward_and_backward_imply_the_same_mask   2-wide and 4-wide lanes against the oracle mask, element for element
   8  test_key_grad_tokens                        exact, registers included; 9  test_lora_pack  exact, canaries kept; 10  test_lora_grad

Outputs sit between canary rows and start as NaN.  Measured ratios: profiles/lora_rows_tests.txt (a record; no bound is taken from it).
"""
import ctypes as C

import pytest
import torch

import lora_rows_ref as R

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402

DEV = "cuda"
AUG = N.LORA_AUG
EINVAL = -1
GUARD_ROWS = 16
CANARY = 1234.0


class Guarded:
    """[rows, cols] of ``dtype`` between GUARD_ROWS canary rows on either side; the payload starts as NaN (or ``fill``), so an element no store reached shows."""

    def __init__(self, rows, cols, dtype, fill=float("nan")):
        self.rows = rows
        self.buf = torch.full((rows + 2 * GUARD_ROWS, cols), CANARY, dtype=dtype, device=DEV)
        self.payload = self.buf[GUARD_ROWS:GUARD_ROWS + rows]
        self.payload.fill_(fill)

    def ptr(self):
        return self.payload.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD_ROWS] == CANARY).all()) and bool((self.buf[GUARD_ROWS + self.rows:] == CANARY).all())

    def untouched(self):
        return self.guards_intact() and bool(torch.isnan(self.payload).all())

    def cpu(self):
        return self.payload.cpu()


class FlatGuarded:
    """n bytes between two canary runs (the partials workspace: too large for whole guard rows)"""
    PAD = 4096

    def __init__(self, nbytes):
        self.n = (nbytes + 3) // 4
        self.buf = torch.full((self.n + 2 * self.PAD,), CANARY, dtype=torch.float32, device=DEV)

    def ptr(self):
        return self.buf[self.PAD:].data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.PAD] == CANARY).all()) and bool((self.buf[self.PAD + self.n:] == CANARY).all())


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _drop(p, layer=3):
    """the struct for (p, R.SEED, layer); None for p = None"""
    return None if p is None else N.LoraDropout(p, R.SEED, layer)


def _ref(d):
    return None if d is None else C.byref(d)


def _id(c):
    return "-".join(str(v) for v in c)


# ================================================================================================ launches
def run_fwd(case, drop="case", inputs=None):
    """-> (rc, Guarded y_aug [rows, D + 64]).  ``drop``: "case" = NULL for p = 0, the struct otherwise; or a p to force a struct."""
    i = inputs or R.fwd_inputs(case)
    n_proj, xh = R.LN_LORA_ENTRIES[case.entry]
    lib = N.load()
    x = i["x"].to(torch.float16 if xh else torch.float32).to(DEV)
    gam, bet, flat = i["gamma"].to(DEV), i["beta"].to(DEV), i["flat"].to(DEV)
    out = Guarded(case.rows, case.D + AUG, torch.bfloat16)
    d = _drop(case.p if case.p else None) if drop == "case" else _drop(drop)
    tail = (case.r, out.ptr(), case.rows, case.D, R.EPS, _ref(d), N.stream())
    if n_proj == 1:
        rc = lib.ucod_layernorm_lora_mlp(N.ptr(x), int(xh), N.ptr(gam), N.ptr(bet), N.ptr(flat), *tail)
    else:
        fn = lib.ucod_layernorm_lora_h16 if xh else lib.ucod_layernorm_lora
        rc = fn(N.ptr(x), N.ptr(gam), N.ptr(bet), N.ptr(flat), *tail)
    torch.cuda.synchronize()
    return rc, out


def check_fwd(tag, case, out, expected=None, rows=None):
    """y, u against (reference, model), zeros past NP r, guards; ``rows`` restricts the comparison (the row walk).  -> (ratio y, ratio u)"""
    n_proj, _ = R.LN_LORA_ENTRIES[case.entry]
    ref, model = expected or R.fwd_expected(case)
    got = out.cpu()
    assert out.guards_intact(), tag
    assert bool(torch.isfinite(got.float()).all()), (tag, "an element no store reached")
    nu = n_proj * case.r
    assert bool((_bits(got[:, case.D + nu:].contiguous()) == 0).all()), (tag, "columns past NP r")
    sel = slice(None) if rows is None else rows
    ry, _ = R.check_bf16(f"{tag}:y", got[:, :case.D][sel], ref["y"][sel], model["y"][sel])
    ru, _ = R.check_bf16(f"{tag}:u", got[:, case.D:case.D + nu][sel], ref["u"][sel], model["u"][sel])
    return ry, ru


def run_bwd(case, inputs=None, want=("dx", "s"), alias=None, p="case"):
    """-> (rc, Guarded dx or None, Guarded s or None).  alias: None, "dres" (dx = dres) or "dy" (dx = dy, f32 dy only)."""
    i = inputs or R.bwd_inputs(case)
    lora, _ = R.LN_BWD_ENTRIES[case.entry]
    lib = N.load()
    fl = case.flags or 0
    rows, D, r = case.rows, case.D, case.r
    dy = i["dy"].to(torch.bfloat16 if fl & 1 else torch.float32).to(DEV)
    x = i["x"].to(torch.float16 if fl & 2 else torch.float32).to(DEV)
    gam = i["gamma"].to(DEV)
    dres = i["dres"].to(DEV) if i["dres"] is not None else None
    scale = i["scale"].to(DEV) if i["scale"] is not None else None
    dx = Guarded(rows, D, torch.float32) if "dx" in want else None
    s = Guarded(rows, D, torch.bfloat16) if "s" in want else None
    dy_ptr, dres_ptr = N.ptr(dy), N.ptr(dres)
    if alias == "dres":
        dx.payload.copy_(dres)
        dres_ptr = dx.ptr()
    elif alias == "dy":
        assert not fl & 1
        dx.payload.copy_(dy)
        dy_ptr = dx.ptr()
    head = (dy_ptr, N.ptr(x)) + ((case.flags,) if case.flags is not None else ())
    body = (N.ptr(gam), dres_ptr, N.ptr(scale), dx.ptr() if dx else None, s.ptr() if s else None, rows, D, R.EPS)
    d = _drop(case.p if p == "case" else p)                                  # p = 0: a struct that says so, not NULL
    if lora == 0:
        fn = lib.ucod_layernorm_bwd if case.flags is None else lib.ucod_layernorm_bwd_ex
        rc = fn(*head, *body, N.stream())
    else:
        flat = i["flat"].to(DEV)
        if lora == 3:
            aug = torch.full((rows, 3 * D + AUG), R.T_FILL, dtype=torch.bfloat16)
            aug[:, 3 * D:3 * D + 3 * r] = i["t"].to(torch.bfloat16)
            aug = aug.to(DEV)
            fn = lib.ucod_layernorm_bwd_lora if case.flags is None else lib.ucod_layernorm_bwd_lora_ex
            rc = fn(*head, *body, N.ptr(aug), N.ptr(flat), r, _ref(d), N.stream())
        else:
            ldt = r + 5
            tb = torch.full((rows, ldt), R.T_FILL, dtype=torch.bfloat16)
            tb[:, :r] = i["t"].to(torch.bfloat16)
            tb = tb.to(DEV)
            rc = lib.ucod_layernorm_bwd_lora_mlp(*head, *body, N.ptr(tb), ldt, N.ptr(flat), r, _ref(d), N.stream())
    torch.cuda.synchronize()
    return rc, dx, s


def check_bwd(tag, case, dx, s, expected=None):
    ref, model = expected or R.bwd_expected(case)
    assert dx.guards_intact() and s.guards_intact(), tag
    wdx = R.check_f32(f"{tag}:dx", dx.cpu(), ref["dx"], R.DX_TOL)
    rs, _ = R.check_bf16(f"{tag}:s", s.cpu(), ref["s"], model["s"])
    return wdx, rs


# ================================================================================================ 1. ln_lora, every instantiation
@pytest.mark.parametrize("case", R.FWD_CASES, ids=_id)
def test_ln_lora_every_instantiation(case):
    assert R.ln_lora_instance(case.entry, case.D, case.r) is not None
    rc, out = run_fwd(case)
    assert rc == 0, rc
    tag = "fwd:" + _id(case)
    ry, ru = check_fwd(tag, case, out)
    print(f"\nRATIO {tag}  y={ry:.3f}  u={ru:.3f}")
    if case.p > 0 and case.rows >= 5:                                            # the projection really is dropped: the undropped one is far off
        i = R.fwd_inputs(case)
        ref, model = R.fwd_expected(case)
        plain = R.ln_lora(i["x"], i["gamma"], i["beta"], [a for a, _ in i["mats"]], None)["u"]
        n_proj = R.LN_LORA_ENTRIES[case.entry][0]
        got = out.cpu()[:, case.D:case.D + n_proj * case.r].double()
        for p in range(n_proj):
            c = slice(p * case.r, (p + 1) * case.r)
            assert float((got[:, c] - plain[:, c]).abs().max()) > 8 * float(R.bf16_row_bound(ref["u"][:, c], model["u"][:, c]).max()), (tag, p)


@pytest.mark.parametrize("D", R.LN_LORA_REFUSED_D)
def test_ln_lora_refuses_the_widths_it_has_no_kernel_for(D):
    for entry in R.LN_LORA_ENTRIES:
        case = R.FwdCase(entry, D, 5, 2, 0.0, "randn")
        assert R.ln_lora_instance(entry, D, 2) is None
        rc, out = run_fwd(case)
        assert rc == EINVAL and out.untouched(), (entry, rc)


# ================================================================================================ 2. the row walk
@pytest.mark.parametrize("case", R.WALK_CASES, ids=_id)
def test_ln_lora_row_walk(case):
    """at most 2048 blocks x 4 waves x 2 rows in flight: a second trip from 16 384 rows on, and an odd row count leaves a wave with one live row.  gamma = 1,
    beta = 0, so that every row of y -- compared or not -- has mean 0 and mean square 1 up to its bf16 rounding: |e_i| <= 2^-8 |y_i| gives
    |mean y| <= 2^-8 mean|y| <= 2^-8 and |mean y^2 - 1| <= 2 * 2^-8 + 2^-16 (plus eps / var and the f32 sums, < 1e-4).
    (The clamp of the dead row's load to rows - 1 only keeps that load inside x: the loaded values are never used, so no result here depends on it.)"""
    i = dict(R.fwd_inputs(case))
    i["gamma"], i["beta"] = torch.ones(case.D), torch.zeros(case.D)
    A = [a for a, _ in i["mats"]]
    args = (i["x"], i["gamma"], i["beta"], A, R.drop_of(case.p) if case.p else None)
    expected = (R.ln_lora(*args), R.ln_lora(*args, rnd=R.bf16_round))
    rc, out = run_fwd(case, inputs=i)
    assert rc == 0, rc
    tag = "walk:" + _id(case)
    ry, ru = check_fwd(tag, case, out, expected, rows=R.edge_rows(case.rows))
    print(f"\nRATIO {tag}  y={ry:.3f}  u={ru:.3f}  ({len(R.edge_rows(case.rows))} edge rows)")
    y = out.cpu()[:, :case.D].double()
    assert float(y.mean(1).abs().max()) <= 2.0 ** -8 + 1e-4, tag
    assert float(((y * y).mean(1) - 1).abs().max()) <= 2.0 ** -7 + 2.0 ** -16 + 1e-4, tag


# ================================================================================================ 3. ln_bwd, every instantiation
@pytest.mark.parametrize("case", R.BWD_CASES, ids=_id)
def test_ln_bwd_every_instantiation(case):
    assert R.ln_bwd_instance(case.entry, case.D, case.flags, case.r) is not None
    rc, dx, s = run_bwd(case)
    assert rc == 0, rc
    tag = "bwd:" + _id(case)
    wdx, rs = check_bwd(tag, case, dx, s)
    print(f"\nRATIO {tag}  dx/bound={wdx:.4f}  s={rs:.3f}")


def test_ln_bwd_refusals():
    """D = 1664 (13 x 128: no instantiation) and flags = 2 (fp16 x only with bf16 dy) return UCOD_EINVAL and write nothing"""
    for entry, flags in R.BWD_FORMS:
        case = R.BwdCase(entry, flags, 1664, 5, 2, True, True, 0.3, "randn")
        rc, dx, s = run_bwd(case)
        assert rc == EINVAL and dx.untouched() and s.untouched(), (entry, flags, rc)
    for entry in ("bwd_ex", "bwd_lora_ex", "bwd_lora_mlp"):
        case = R.BwdCase(entry, 2, 768, 5, 2, True, True, 0.3, "randn")
        rc, dx, s = run_bwd(case)
        assert rc == EINVAL and dx.untouched() and s.untouched(), (entry, rc)
    case = R.BwdCase("bwd_ex", 1, 768, 5, 2, True, True, None, "randn")           # the stream carries no error from the refusals
    rc, dx, s = run_bwd(case)
    assert rc == 0
    check_bwd("bwd:after-refusals", case, dx, s)


# ================================================================================================ 4. rank
@pytest.mark.parametrize("case", R.RANK_BWD_CASES, ids=_id)
def test_rank_ln_bwd(case):
    """ranks 1, 2, 4 take the unrolled branch of ln_bwd_kernel, every other rank the generic loop"""
    rc, dx, s = run_bwd(case)
    assert rc == 0, rc
    tag = "rank-bwd:" + _id(case)
    wdx, rs = check_bwd(tag, case, dx, s)
    print(f"\nRATIO {tag}  dx/bound={wdx:.4f}  s={rs:.3f}")


@pytest.mark.parametrize("case", R.RANK_FWD_CASES, ids=_id)
def test_rank_ln_lora(case):
    rc, out = run_fwd(case)
    assert rc == 0, rc
    tag = "rank-fwd:" + _id(case)
    ry, ru = check_fwd(tag, case, out)
    print(f"\nRATIO {tag}  y={ry:.3f}  u={ru:.3f}")


@pytest.mark.parametrize("D,r", R.LDS_CASES)
def test_rank_ln_lora_lds_boundary(D, r):
    """3 r D 4 bytes of staged A rows around 64 KiB (where the launch has to ask) and around one workgroup's LDS (where it has to refuse).  The contract:
    rc == 0 and correct; or rc != 0, nothing written, and the next valid call on the same stream returns 0 and is correct (no error left behind).
    ucod_layernorm_lora_fits says beforehand which of the two; on gfx950 it says what the restated table says."""
    lib = N.load()
    fits = lib.ucod_layernorm_lora_fits(D, r, 3)
    if lib.ucod_device_is_gfx950() == 1:
        assert (fits == 1) == (R.ln_lora_instance("lora", D, r) is not None), (D, r, fits)
    for entry in ("lora", "lora_h16"):
        case = R.FwdCase(entry, D, 5, r, 0.3, "randn")
        rc, out = run_fwd(case)
        tag = f"lds:{entry}:{D}-{r}"
        assert (rc == 0) == (fits == 1), (tag, rc, fits)
        if rc == 0:
            ry, ru = check_fwd(tag, case, out)
            print(f"\nRATIO {tag}  {3 * r * D * 4} bytes  y={ry:.3f}  u={ru:.3f}")
        else:
            assert rc == EINVAL and out.untouched(), (tag, rc)
            print(f"\nREFUSED {tag}  {3 * r * D * 4} bytes  rc={rc}")
        small = R.FwdCase(entry, D, 5, 2, 0.3, "randn")
        rc, out = run_fwd(small)
        assert rc == 0, (tag, "the next valid call", rc)
        check_fwd(tag + ":next", small, out)


def test_training_descriptor_and_engine_refuse_what_the_row_kernel_refuses():
    """a (D, r) whose A rows do not fit one workgroup's LDS is refused by the size helpers of the training passes and by the engine's constructor, so that a
    pass cannot fail half-way through its first layer"""
    lib = N.load()
    if lib.ucod_device_is_gfx950() != 1:
        pytest.skip("the (D, r) table is gfx950's")
    for D, heads, r, fits in ((768, 12, 17, True), (768, 12, 18, False), (1536, 24, 8, True), (1536, 24, 9, False), (1024, 16, 13, True), (1024, 16, 14, False)):
        t = N.VitTrainDesc()
        v = t.vit
        v.B, v.C, v.H, v.W, v.P, v.D, v.heads, v.F, v.L, v.Kpad, v.eps, v.attn_variant = 2, 3, 56, 56, 14, D, heads, 4 * D, 2, 640, 1e-6, 2
        t.lora_r, t.lora_scaling = r, 2.0
        assert lib.ucod_layernorm_lora_fits(D, r, 3) == int(fits), (D, r)
        assert (lib.ucod_vit_train_workspace_bytes(C.byref(t)) > 0) == fits, (D, r)
        assert (lib.ucod_vit_lora_infer_workspace_bytes(C.byref(t)) > 0) == fits, (D, r)
    assert lib.ucod_layernorm_lora_fits(768, 0, 3) == 0 and lib.ucod_layernorm_lora_fits(768, 2, 2) == 0 and lib.ucod_layernorm_lora_fits(768, 22, 3) == 0
    assert lib.ucod_layernorm_lora_fits(1536, 8, 1) == 1 and lib.ucod_layernorm_lora_fits(0, 2, 3) == 0
    from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict, ARCHS
    from ucod_dpl_amd.vit_engine import ViTLoRAEngine
    ARCHS["lora_rows_vit768"] = (768, 12, 1, 14, 70, True)
    sd = random_state_dict("lora_rows_vit768", seed=3)
    with pytest.raises(ValueError, match="do not fit"):
        ViTLoRAEngine(sd, heads=12, r=18, device=DEV)
    assert ViTLoRAEngine(sd, heads=12, r=17, device=DEV).r == 17


# ================================================================================================ 5. aliasing and null outputs
@pytest.mark.parametrize("D", [384, 1024])
@pytest.mark.parametrize("entry,flags", [("bwd", None), ("bwd_lora", None), ("bwd_ex", 1), ("bwd_lora_ex", 3)])
def test_ln_bwd_aliasing_and_null_outputs(entry, flags, D):
    """include/ucod_dpl.h: 'dx may alias dres or dy; either output may be NULL' -- each bitwise the unaliased two-output call"""
    case = R.BwdCase(entry, flags, D, 37, 2, True, True, 0.3, "randn")
    rc, dx0, s0 = run_bwd(case)
    assert rc == 0
    check_bwd(f"alias:{entry}:{flags}:{D}:base", case, dx0, s0)
    dx0, s0 = _bits(dx0.cpu()), _bits(s0.cpu())
    variants = [("dres", ("dx", "s")), (None, ("dx",)), (None, ("s",))] + ([("dy", ("dx", "s"))] if not (flags or 0) & 1 else [])
    for alias, want in variants:
        rc, dx, s = run_bwd(case, want=want, alias=alias)
        assert rc == 0, (alias, want, rc)
        if dx is not None:
            assert dx.guards_intact() and torch.equal(_bits(dx.cpu()), dx0), (alias, want, "dx")
        if s is not None:
            assert s.guards_intact() and torch.equal(_bits(s.cpu()), s0), (alias, want, "s")


# ================================================================================================ 6. dropout extremes
@pytest.mark.parametrize("D", [128, 256])
def test_dropout_extremes(D):
    """p = 0.0005: floor(1024 p) = 0, no dropout at all -- bit for bit the call without; p = 0.9995: the clamp at 1023, kept elements scaled by 1024"""
    assert R.drop_threshold(0.0005) == 0 and R.drop_threshold(0.9995) == 1023
    for entry in ("lora", "lora_mlp_h16"):
        base = R.FwdCase(entry, D, 37, 2, 0.0, "randn")
        _, off = run_fwd(base)
        rc, tiny = run_fwd(base, drop=0.0005)
        assert rc == 0 and torch.equal(_bits(off.cpu()), _bits(tiny.cpu())), entry
        top = R.FwdCase(entry, D, 37, 2, 0.9995, "randn")
        rc, out = run_fwd(top)
        assert rc == 0
        ry, ru = check_fwd(f"extreme-fwd:{entry}:{D}", top, out)
        ref, _ = R.fwd_expected(top)
        assert float(ref["u"].abs().max()) > 0                                   # some element survives: the check is not about zeros only
        print(f"\nRATIO extreme-fwd:{entry}:{D}  y={ry:.3f}  u={ru:.3f}")
    for entry, flags in (("bwd_lora", None), ("bwd_lora_ex", 3), ("bwd_lora_mlp", 1)):
        base = R.BwdCase(entry, flags, D, 37, 2, True, True, 0.0, "randn")
        _, dx0, s0 = run_bwd(base)
        rc, dx1, s1 = run_bwd(base, p=0.0005)
        assert rc == 0 and torch.equal(_bits(dx0.cpu()), _bits(dx1.cpu())) and torch.equal(_bits(s0.cpu()), _bits(s1.cpu())), entry
        check_bwd(f"extreme-bwd:{entry}:{D}:off", base, dx0, s0)
        top = base._replace(p=0.9995)
        rc, dx, s = run_bwd(top)
        assert rc == 0
        wdx, rs = check_bwd(f"extreme-bwd:{entry}:{D}", top, dx, s)
        print(f"\nRATIO extreme-bwd:{entry}:{D}  dx/bound={wdx:.4f}  s={rs:.3f}")


# ================================================================================================ 7. one mask, forward and backward, 2-wide and 4-wide lanes
def _probe_columns(D):
    fixed = [0, 1, 2, 3, 127, 128, 255, 256, D - 1]
    g = torch.Generator().manual_seed(D)
    rest = [c for c in torch.randperm(D, generator=g).tolist() if c not in fixed]
    return sorted(fixed + rest[:64 - len(fixed)])


@pytest.mark.parametrize("D", [384, 768])
def test_forward_and_backward_imply_the_same_mask(D):
    """ln_lora_kernel / ln_lora4_kernel index the mix by 2 / 4 columns per lane, ln_bwd_kernel by VW; all three fields must land on the oracle's elements.
    Forward: A_p[j] = e_(col j), so u[row, p r + j] = y[row, col j] * mask_p[row, col j].  Backward: gamma = 1, dy = 0, row i carries t = e_(p, j), so
    dy' = mask_p[i, col j] e_(col j): the row of dx is zero exactly where the element is dropped."""
    r, rows, p_drop = 16, 48, 0.3
    cols = _probe_columns(D)
    assert len(cols) == 64 and len(set(cols)) == 64
    oracle = [R.masks(R.drop_of(p_drop), rows, D, 3)[p] > 0 for p in range(3)]
    assert all(0.5 < float(m.double().mean()) < 0.9 for m in oracle)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(rows, D, generator=g) * 2 + 0.3
    for c0 in range(0, 64, r):
        grp = cols[c0:c0 + r]
        A = torch.zeros(r, D)
        A[torch.arange(r), torch.tensor(grp)] = 1.0
        flat = torch.cat([torch.cat((A.reshape(-1), torch.zeros(D * r))) for _ in range(3)])
        mats = [(A, torch.zeros(D, r))] * 3
        # forward
        case = R.FwdCase("lora", D, rows, r, p_drop, "randn")
        i = {"x": x, "gamma": torch.ones(D), "beta": torch.zeros(D), "flat": flat, "mats": mats}
        rc, out = run_fwd(case, inputs=i)
        assert rc == 0
        u = out.cpu()[:, D:D + 3 * r].float()
        y = R.ln_lora(x, i["gamma"], i["beta"], [A] * 3, None)["y"]
        assert float(y[:, grp].abs().min()) > 1e-6                               # no probed element of y is zero by itself
        for p in range(3):
            assert torch.equal(u[:, p * r:(p + 1) * r] != 0, oracle[p][:, grp]), ("forward", D, p, c0)
        args = (x, i["gamma"], i["beta"], [A] * 3, R.drop_of(p_drop))
        check_fwd(f"mask-fwd:{D}:{c0}", case, out, (R.ln_lora(*args), R.ln_lora(*args, rnd=R.bf16_round)))
        # backward: row i probes (p, j) = (i // r, i % r)
        t = torch.zeros(rows, 3 * r)
        t[torch.arange(rows), torch.arange(rows)] = 1.0
        bcase = R.BwdCase("bwd_lora", None, D, rows, r, False, False, p_drop, "randn")
        bi = {"x": x, "gamma": torch.ones(D), "dy": torch.zeros(rows, D), "dres": None, "scale": None, "t": t, "flat": flat, "mats": mats}
        rc, dx, s = run_bwd(bcase, inputs=bi)
        assert rc == 0
        kept = (dx.cpu() != 0).any(1)
        want = torch.stack([oracle[i_ // r][i_, grp[i_ % r]] for i_ in range(rows)])
        assert torch.equal(kept, want), ("backward", D, c0)
        bargs = (bi["dy"], x, bi["gamma"], None, None, t, [A] * 3, R.drop_of(p_drop))
        check_bwd(f"mask-bwd:{D}:{c0}", bcase, dx, s, (R.ln_bwd(*bargs), R.ln_bwd(*bargs, rnd_dx=R.f32_round, rnd_s=R.bf16_round)))


# ================================================================================================ 8. key_grad_tokens(_reg)
@pytest.mark.parametrize("n_reg", [0, 1, 4])
@pytest.mark.parametrize("D", [32, 96, 384])
def test_key_grad_tokens(D, n_reg):
    """exact: the K third is bf16(dkey^T) behind the CLS and register rows; the q / v thirds, the aug columns and those rows are zero bits"""
    lib = N.load()
    for B in (1, 3):
        for tok in (2 + n_reg, 26, 32, 33, 65, 257):
            g = torch.Generator().manual_seed(B * 1000 + tok + D)
            dkey = torch.randn(B, D, tok - 1 - n_reg, generator=g)
            dk = dkey.to(DEV)
            want = _bits(R.key_grad_tokens(dkey, tok, n_reg).reshape(B * tok, 3 * D + AUG))
            out = Guarded(B * tok, 3 * D + AUG, torch.bfloat16)
            assert lib.ucod_key_grad_tokens_reg(N.ptr(dk), out.ptr(), B, tok, D, n_reg, N.stream()) == 0
            torch.cuda.synchronize()
            assert out.guards_intact() and torch.equal(_bits(out.cpu()), want), (B, tok)
            if n_reg == 0:                                                       # the plain entry is the _reg one at n_reg = 0, bit for bit
                plain = Guarded(B * tok, 3 * D + AUG, torch.bfloat16)
                assert lib.ucod_key_grad_tokens(N.ptr(dk), plain.ptr(), B, tok, D, N.stream()) == 0
                torch.cuda.synchronize()
                assert plain.guards_intact() and torch.equal(_bits(plain.cpu()), want), (B, tok)


def test_key_grad_tokens_refusals():
    lib = N.load()
    D, tok = 96, 26
    dk = torch.zeros(3, D, tok - 1, device=DEV)
    out = Guarded(3 * tok, 3 * D + AUG, torch.bfloat16)
    bad = [(1, 2, D, 1), (1, 1, D, 0), (1, 5, D, 4), (1, tok, 48, 0), (1, tok, D + 16, 0), (65536, tok, D, 0), (1, tok, D, -1), (0, tok, D, 0)]
    for B, t, d, n_reg in bad:                                                   # tok < 2 + n_reg, D % 32 != 0, B = 65 536 (the grid's y limit), n_reg < 0
        assert lib.ucod_key_grad_tokens_reg(N.ptr(dk), out.ptr(), B, t, d, n_reg, N.stream()) == EINVAL, (B, t, d, n_reg)
    assert lib.ucod_key_grad_tokens(N.ptr(dk), out.ptr(), 1, 1, D, N.stream()) == EINVAL
    assert lib.ucod_key_grad_tokens_reg(None, out.ptr(), 1, tok, D, 0, N.stream()) == EINVAL
    assert lib.ucod_key_grad_tokens_reg(N.ptr(dk), None, 1, tok, D, 0, N.stream()) == EINVAL
    torch.cuda.synchronize()
    assert out.untouched()
    assert lib.ucod_key_grad_tokens_reg(N.ptr(dk), out.ptr(), 3, tok, D, 0, N.stream()) == 0
    torch.cuda.synchronize()
    assert out.guards_intact() and bool((_bits(out.cpu()) == 0).all())


# ================================================================================================ 9. lora_pack
@pytest.mark.parametrize("D", [128, 384, 1536])
@pytest.mark.parametrize("r", [1, 2, 3, 8, 21])
def test_lora_pack(r, D):
    """exact; zero_a_columns; either matrix NULL; the non-aug columns of both matrices keep their canary"""
    lib = N.load()
    g = torch.Generator().manual_seed(r * 31 + D)
    flat, mats = R.arena(r, D, g)
    fs = flat.to(DEV)
    scaling = float(torch.tensor(4.0 / 3.0, dtype=torch.float32))
    for zero_a, use_w, use_wt in ((0, True, True), (1, True, True), (0, True, False), (0, False, True), (1, False, True)):
        w = Guarded(3 * D, D + AUG, torch.bfloat16, fill=CANARY)
        wt = Guarded(D, 3 * D + AUG, torch.bfloat16, fill=CANARY)
        assert lib.ucod_lora_pack(N.ptr(fs), r, scaling, w.ptr() if use_w else None, wt.ptr() if use_wt else None, D, zero_a, N.stream()) == 0
        torch.cuda.synchronize()
        want_w, want_wt = R.lora_pack(mats, r, D, scaling, zero_a)
        gw, gwt = w.cpu(), wt.cpu()
        assert w.guards_intact() and wt.guards_intact()
        assert bool((gw[:, :D] == CANARY).all()) and bool((gwt[:, :3 * D] == CANARY).all()), "a non-aug column was written"
        if use_w:
            assert torch.equal(_bits(gw[:, D:].contiguous()), _bits(want_w)), (zero_a, "w_aug")
        else:
            assert bool((gw == CANARY).all())
        if use_wt:
            assert torch.equal(_bits(gwt[:, 3 * D:].contiguous()), _bits(want_wt)), (zero_a, "wt_aug")
        else:
            assert bool((gwt == CANARY).all())
    assert lib.ucod_lora_pack(N.ptr(fs), r, scaling, None, None, D, 0, N.stream()) == EINVAL
    assert lib.ucod_lora_pack(N.ptr(fs), 22, scaling, None, wt.ptr(), D, 0, N.stream()) == EINVAL


# ================================================================================================ 10. lora_grad
def _run_grad(case, i):
    lib = N.load()
    rows, D, r = case.rows, case.D, case.r
    d_aug = torch.full((rows, 3 * D + AUG), R.T_FILL, dtype=torch.bfloat16)
    d_aug[:, :3 * D] = i["dqkv"]
    h_aug = torch.zeros(rows, D + AUG, dtype=torch.bfloat16)
    h_aug[:, :D] = i["h"]
    h_aug[:, D:D + 3 * r] = i["u"]
    dq = Guarded(rows, 3 * D + AUG, torch.bfloat16)
    dq.payload.copy_(d_aug)
    hs, fs = h_aug.to(DEV), i["flat"].to(DEV)
    wsb = lib.ucod_lora_grad_workspace_bytes(D)
    ws = FlatGuarded(wsb)
    grad = Guarded(1, 6 * r * D, torch.float32)
    if case.accumulate:
        grad.payload.copy_(i["grad0"].reshape(1, -1))
    d = _drop(case.p if case.p else None)
    rc = lib.ucod_lora_grad(dq.ptr(), N.ptr(hs), N.ptr(fs), r, i["scaling"], grad.ptr(), int(case.accumulate), ws.ptr(), wsb, rows, D, _ref(d), N.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert dq.guards_intact() and grad.guards_intact() and ws.guards_intact(), "a guard was written"
    return dq.cpu(), grad.cpu().reshape(-1)


@pytest.mark.parametrize("case", R.GRAD_CASES, ids=_id)
def test_lora_grad(case):
    """t against f64 under the bf16 row bound; dA and dB under test_lora_grad's 2e-4 per row, from the bf16 t the kernel itself wrote (as that test does: the
    kernel documents that dA uses the value the dgrad GEMM will see); accumulate adds onto a known gradient; two runs are bitwise equal"""
    i = R.grad_inputs(case)
    rows, D, r = case.rows, case.D, case.r
    dq, grad = _run_grad(case, i)
    dq2, grad2 = _run_grad(case, i)
    assert torch.equal(_bits(dq), _bits(dq2)) and torch.equal(_bits(grad), _bits(grad2)), "two runs differ"
    tag = "grad:" + _id(case)
    assert torch.equal(_bits(dq[:, :3 * D].contiguous()), _bits(i["dqkv"])), "dqkv itself was written"
    assert bool((dq[:, 3 * D + 3 * r:] == R.T_FILL).all()), "aug columns past 3 r were written"
    B = [b for _, b in i["mats"]]
    t_got = dq[:, 3 * D:3 * D + 3 * r]
    rt, _ = R.check_bf16(f"{tag}:t", t_got, R.lora_t(i["dqkv"], B, i["scaling"]), R.lora_t(i["dqkv"], B, i["scaling"], rnd=R.bf16_round))
    dA, dB = R.lora_grads(i["dqkv"], i["h"], i["u"], t_got, i["scaling"], R.drop_of(case.p) if case.p else None)
    worst, off = 0.0, 0
    g0 = i["grad0"].double() if case.accumulate else torch.zeros(6 * r * D, dtype=torch.float64)
    for p in range(3):
        gA, gB = grad[off:off + r * D].reshape(r, D), grad[off + r * D:off + 2 * r * D].reshape(D, r)
        worst = max(worst, R.check_f32(f"{tag}:dA{p}", gA, dA[p] + g0[off:off + r * D].reshape(r, D), R.GRAD_TOL),
                    R.check_f32(f"{tag}:dB{p}", gB, dB[p] + g0[off + r * D:off + 2 * r * D].reshape(D, r), R.GRAD_TOL))
        off += 2 * r * D
    print(f"\nRATIO {tag}  t={rt:.3f}  grad/bound={worst:.4f}")
