"""GPU: LoRA ``bias="lora_only"`` (models/modules/full_model.py:53,66 hands ``bias`` to peft) -- the biases of the targeted modules trained by the backbone backward,
every call through the C ABI or the engine.

1-3  ucod_colsum_det alone: exact inputs against f64 column sums bit for bit, random 16-bit data under the bar tests/test_gpu_lora_out.py holds dA / dB to (the same
     kind of f32 sum over M rows of 16-bit values: 2e-4 max(1, |ref|max)), canaries around output and workspace, large values beyond column N, run twice; refusals;
4    whole passes against f64 autograd (tests/lora_bias_ref.py, whose measure tests/test_lora_bias_host.py shows to have teeth): five models x three target sets x
     dropout 0 / 0.05 x one / two streams.  Key map and LoRA gradients under the bars of the files that own those models (tests/test_gpu_lora_out.py,
     tests/test_gpu_lora_swiglu_out.py, tests/test_gpu_dinov3_lora.py); bias gradients under the project's LoRA-gradient bar, 4e-2 (5e-2 with dropout or at D = 256), on
     each layer's concatenated vector and on every tensor with at least 1e-3 of its norm; the last layer's non-key bias gradients exact zeros;
5    bias="none", and "lora_only" where no targeted module has a bias, against the engine built without the argument, bit for bit; the new backward tier with a NULL
     table against _lora_out_ex;
6    three steps of the runner: what moves, what keeps its bits, what the state dicts say of the last layer, two runs identical;
7    merging perturbed biases: the merged state dict on the f32-equivalent engine, merge_into on the folded default engine, the adapter folder.

No bar is taken from a run of this code.  Measured on MI355X: profiles/lora_bias_tests.txt."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, sub, maxdiff

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd import native as N  # noqa: E402
from ucod_dpl_amd.vit_engine import ViTEngine, SplitViTEngine, ViTLoRAEngine, normalize_state_dict, _prepare_mlp  # noqa: E402
from oracle import vit as OV  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import dinov3_lora_ref as RL  # noqa: E402
import registers_ref as RR  # noqa: E402
import lora_out_ref as RO  # noqa: E402
import lora_swiglu_out_ref as RS  # noqa: E402
import lora_bias_ref as RB  # noqa: E402

DEV = "cuda"
HALF, F32 = N.ROPE_ELEM_HALF, N.ROPE_ELEM_F32
CANARY, PAD = 1234.0, 4096


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


class Flat:
    """n f32 elements (NaN: an element no store reached shows) between two canary runs"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV)
        self.payload = self.buf[PAD:PAD + n]
        self.payload.fill_(float("nan"))

    def ptr(self):
        return self.payload.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[PAD + self.n:] == CANARY).all())


# ------------------------------------------------------------------------------------------------ 1-2. the kernel
# (M, N, ld, elem, scaled): one row; rows that are no multiple of the 16 row threads or of a slab, two slabs; 43 slabs and a pitch beyond N (the thirds of dqkv:
# ld = 3 D + 64); the widest buffer (64 column groups); f32 input; a power-of-two col_scale
CASES = [(1, 128, 128, HALF, False), (111, 384, 448, HALF, False), (2740, 2304, 2368, HALF, False), (111, 8192, 8192, HALF, False), (2740, 256, 256, F32, False),
         (1371, 1536, 1536, HALF, True)]
LEAK = 30000.0            # what columns N .. ld - 1 hold


def run_colsum(x, elem, M, n, ld, scale):
    lib = N.load()
    wsb = lib.ucod_colsum_det_workspace_bytes(M, n)
    assert wsb == min(128, -(-M // 64)) * n * 4
    outs = []
    for _ in range(2):
        out, ws = Flat(n), Flat(wsb // 4)
        assert lib.ucod_colsum_det(N.ptr(x), elem, M, n, ld, None if scale is None else N.ptr(scale), out.ptr(), ws.ptr(), wsb, N.stream()) == 0
        torch.cuda.synchronize()
        assert out.guards_intact() and ws.guards_intact(), "wrote outside its output or workspace"
        assert bool(torch.isfinite(out.payload).all()) and bool(torch.isfinite(ws.payload).all()), "left elements unwritten"
        outs.append(out.payload.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs differ"
    return outs[0].cpu()


@pytest.mark.parametrize("M,n,ld,elem,scaled", CASES)
def test_colsum_exact(M, n, ld, elem, scaled):
    """Integers in [-8, 8] times a power of two per column: every partial sum in any order is an f32 number (8 M < 2^24, asserted), so the result must be the f64
    column sums bit for bit whatever the order of the additions."""
    g = torch.Generator().manual_seed(M + n)
    assert 8 * M < 2 ** 24
    x = torch.randint(-8, 9, (M, n), generator=g).double() * torch.exp2(torch.randint(-6, 7, (n,), generator=g).double())
    scale = torch.exp2(torch.randint(-3, 4, (n,), generator=g).double()) if scaled else None
    dtype = torch.float32 if elem == F32 else torch.bfloat16
    buf = torch.full((M, ld), LEAK, dtype=dtype)
    buf[:, :n] = x.to(dtype)
    assert torch.equal(buf[:, :n].double(), x)                       # the inputs are exact in the element type
    ref = x.sum(0) * (scale if scaled else 1.0)
    assert torch.equal(ref.float().double(), ref)
    got = run_colsum(buf.to(DEV), elem, M, n, ld, None if scale is None else scale.float().to(DEV))
    assert torch.equal(got.double(), ref), f"{int((got.double() != ref).sum())} of {n} columns differ, worst {float((got.double() - ref).abs().max()):.3e}"
    assert float(ref.abs().max()) > 0


@pytest.mark.parametrize("M,n,ld,elem,scaled", CASES)
def test_colsum_random(M, n, ld, elem, scaled):
    """N(0, 1) rounded to the element type: |got - ref| <= 2e-4 max(1, |ref|max), the bar of dA / dB in tests/test_gpu_lora_out.py."""
    g = torch.Generator().manual_seed(M + n + 1)
    dtype = torch.float32 if elem == F32 else torch.bfloat16
    buf = torch.full((M, ld), LEAK, dtype=dtype)
    buf[:, :n] = torch.randn(M, n, generator=g).to(dtype)
    scale = (torch.rand(n, generator=g) + 0.5) if scaled else None
    ref = buf[:, :n].double().sum(0) * (scale.double() if scaled else 1.0)
    got = run_colsum(buf.to(DEV), elem, M, n, ld, None if scale is None else scale.to(DEV))
    err = maxdiff(got, ref) / max(1.0, ref.abs().max().item())
    print(f"colsum {(M, n, ld)} {'f32' if elem == F32 else 'bf16'} scaled={scaled}: {err:.2e} (bar 2e-4)")
    assert err <= 2e-4, err


def test_colsum_refusals_leave_outputs_untouched():
    M, n, ld = 111, 384, 448
    lib = N.load()
    x = torch.randn(M, ld, device=DEV).bfloat16()
    wsb = lib.ucod_colsum_det_workspace_bytes(M, n)
    out, ws = torch.full((n,), 3.0, device=DEV), torch.full((wsb // 4,), 3.0, device=DEV)
    ok = dict(x=N.ptr(x), elem=HALF, M=M, n=n, ld=ld, scale=None, out=N.ptr(out), ws=N.ptr(ws), wb=wsb)
    call = lambda **kw: lib.ucod_colsum_det(*[{**ok, **kw}[k] for k in ("x", "elem", "M", "n", "ld", "scale", "out", "ws", "wb")], N.stream())  # noqa: E731
    bad = {"null x": dict(x=None), "null out": dict(out=None), "null workspace": dict(ws=None), "M < 1": dict(M=0), "N % 8": dict(n=380), "ld < N": dict(ld=376),
           "misaligned ld": dict(ld=452), "small workspace": dict(wb=wsb - 4), "unknown elem": dict(elem=2)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name
    for M0, n0 in ((0, n), (M, 380), (M, 0)):
        assert lib.ucod_colsum_det_workspace_bytes(M0, n0) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((ws == 3.0).all()), "a refused call wrote to its outputs"
    assert call() == 0                                              # ... and the same arguments without a fault run
    torch.cuda.synchronize()
    assert maxdiff(out.cpu(), x[:, :n].double().sum(0).cpu()) <= 2e-4 * max(1.0, float(x[:, :n].double().sum(0).abs().max()))


# ------------------------------------------------------------------------------------------------ 4. whole passes vs f64 autograd
@functools.lru_cache(maxsize=None)
def model(tag):
    """One model of the five: state dict, geometry, inputs, engine arguments, its three target sets (q / k / v, the key alone, every module that is built), the LoRA
    matrices of each set, and the bars of the file that owns the model."""
    m = dict(tag=tag, eps=1e-6, patch=14, scale=2.0, r=2, alpha=4, kw={}, family="dinov2", z=None, grad_plain=(4e-2, 5e-2), D=128)
    if tag == "g8":
        sd = sub(load_golden("g8_dinov2_native"), "sd.")
        m.update(sd=sd, heads=2, L=3, inputs=RO.case_inputs(2, 128, 70), kw=dict(allow_out=True), sets=(("query", "key", "value"), ("key",), ("query", "key", "value", "fc1", "dense", "fc2")))
    elif tag == "d256":
        sd, heads, L, image, B = RO.d256_state_dict()
        m.update(sd=sd, heads=heads, L=L, D=256, inputs=RO.case_inputs(B, 256, image), kw=dict(allow_out=True), grad_plain=(5e-2, 5e-2),
                 sets=(("query", "key", "value"), ("key",), ("query", "key", "value", "fc1", "dense", "fc2")))
    elif tag == "swiglu":
        sd = RS.g24_state_dict("dinov2")
        m.update(sd=sd, heads=2, L=3, inputs=RO.case_inputs(2, 128, 70), kw=dict(allow_swiglu=True, allow_out=True, allow_swiglu_out=True), grad_plain=(4e-2, 4e-2),
                 sets=(("query", "key", "value"), ("key",), ("query", "key", "value", "weights_in", "dense", "weights_out")))
    elif tag == "reg":
        sd = RR.g21_state_dict("native")
        gen = torch.Generator().manual_seed(7)
        m.update(sd=sd, heads=2, L=3, inputs=(torch.randn(3, 3, 70, 70, generator=gen), torch.randn(3, 128, 5, 5, generator=gen)), kw=dict(allow_out=True),
                 sets=(("query", "key", "value"), ("key",), ("query", "key", "value", "fc1", "dense", "fc2")))
    else:
        assert tag == "g46"
        z = np.load(os.path.join(os.path.dirname(__file__), "golden", "g23_dinov3_lora_g46.npz"))
        sd = R3.g22_state_dict("g46")
        m.update(sd=sd, heads=R3.G22["g46"]["heads"], L=R3.G22_LAYERS, eps=1e-5, patch=16, scale=RL.G23_SCALE, r=RL.G23_R, alpha=RL.G23_ALPHA, family="dinov3", z=z,
                 inputs=(torch.from_numpy(z["x"]), torch.from_numpy(z["dkey"])), kw=dict(allow_rope=True, allow_out=True),
                 sets=(("q_proj", "k_proj", "v_proj"), ("k_proj",), ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")))      # (no MLP input module is built for DINOv3)
    m["tok"], m["lead"] = RB.geometry(m["inputs"][0], m["sd"])
    return m


def lora_of(m, targets):
    sd = m["sd"]
    if m["tag"] == "swiglu":
        return RS.lora_for(sd, targets)
    if m["tag"] == "g46":                                            # the golden's own q / k / v matrices (its bars belong to them), fresh ones for the output modules
        z = m["z"]
        qkv = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lora/") and any(f".{t}." in k for t in targets)}
        out = RO.lora_for(sd, tuple(t for t in targets if t in RO.OUT_NAMES), seed=5)
        return {**qkv, **out}
    return RO.lora_for(sd, targets)


def masks_for(m, targets, p_drop):
    L, tok, D = m["L"], m["tok"], m["D"]
    sd, lay = m["sd"], RB.layer_path(m["sd"])

    def masks_of(seed, images):
        if p_drop == 0:
            return None
        rows = images * tok
        qkv = RL.QKV if m["family"] == "dinov3" else ("query", "key", "value")
        mk = {(i, nm): OV.lora_dropout_mask(seed, i, pi, rows, D, p_drop) for i in range(L) for pi, nm in enumerate(qkv) if nm in targets}
        for nm in ("fc1", "weights_in"):
            if nm in targets:
                mk.update({(i, nm): OV.lora_dropout_mask(seed, L + i, 0, rows, D, p_drop) for i in range(L)})
        if m["tag"] == "swiglu":
            out = RS.out_masks(seed, L, rows, D, 344, p_drop)
        else:
            F = sd[lay + "0." + ("mlp.up_proj" if m["family"] == "dinov3" else "mlp.fc1") + ".weight"].shape[0]
            out = RO.out_masks(seed, L, rows, D, F, p_drop, RO.OUT_LEAVES[m["family"]])
        mk.update({k: v for k, v in out.items() if k[1] in targets})
        return mk
    return masks_of


def reference(m, targets, lora, masks_of, bounds, seeds):
    """(key, LoRA gradients, bias gradients, the bias gradients' term magnitudes) of the f64 restatement chunk by chunk (each chunk of a pass has its own masks);
    gradients add."""
    img, dkey = m["inputs"]
    full = {**m["sd"], **lora}
    keys, gl, gb, ga = [], None, None, None
    for (b0, b1), seed in zip(bounds, seeds):
        k, g, rows = RB.grads(img[b0:b1], full, m["heads"], dkey[b0:b1], m["scale"], targets, masks=masks_of(seed, b1 - b0), device=DEV)
        b = RB.bias_grads(rows, full, m["lead"])
        keys.append(k.cpu())
        gl = {n: v.cpu() for n, v in g.items()} if gl is None else {n: gl[n] + v.cpu() for n, v in g.items()}
        gb = {n: v.cpu() for n, v in b.items()} if gb is None else {n: gb[n] + v.cpu() for n, v in b.items()}
        ga = {n: v.cpu() for n, v in RB.abs_sums(rows).items()} if ga is None else {n: ga[n] + v.cpu() for n, v in RB.abs_sums(rows).items()}
    return torch.cat(keys, 0), gl, gb, ga


@functools.lru_cache(maxsize=None)
def reference_without_dropout(tag, targets):
    """(without dropout no mask depends on the chunks: one reference serves both stream counts)"""
    m = model(tag)
    B = m["inputs"][0].shape[0]
    return reference(m, targets, lora_of(m, targets), lambda seed, images: None, [(0, B)], [0])


def bias_engine(m, targets, lora, bias="lora_only", biases=None, **kw):
    eng = ViTLoRAEngine(m["sd"], heads=m["heads"], r=m["r"], lora_alpha=m["alpha"], eps=m["eps"], device=DEV, generator=torch.Generator().manual_seed(3),
                        target_modules=list(targets), bias=bias, **m["kw"], **kw)
    have = RB.bias_names(m["sd"], targets) if bias == "lora_only" else []
    assert sorted(eng.lora_state_dict()) == sorted(list(lora) + have)
    eng.load_lora_state_dict({**lora, **{k: m["sd"][k] for k in have}, **(biases or {})})
    return eng


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["qkv", "key", "all"])
@pytest.mark.parametrize("tag", ["g8", "d256", "swiglu", "reg", "g46"])
def test_passes_vs_f64_autograd(tag, which, p_drop, streams):
    m = model(tag)
    targets = m["sets"][which]
    sd, L, lay = m["sd"], m["L"], RB.layer_path(m["sd"])
    lora = lora_of(m, targets)
    img, dkey = m["inputs"]
    eng = bias_engine(m, targets, lora, lora_dropout=p_drop, seed=1234)
    eng.train_streams = streams
    key = eng.forward_train(img.to(DEV)).clone()
    eng.backward(dkey.to(DEV))
    eng.check_overflow(wait=True)
    if p_drop == 0:
        key_ref, gl, gb, ga = reference_without_dropout(tag, targets)
    else:
        key_ref, gl, gb, ga = reference(m, targets, lora, masks_for(m, targets, p_drop), list(eng._bounds), list(eng._chunk_seed))
    got = {k: v.cpu() for k, v in eng.lora_state_dict(grads=True).items()}
    assert sorted(got) == sorted(list(gl) + list(gb))
    # the key map and the LoRA gradients: the owning file's bars
    z = m["z"]
    if z is None:
        key_err, key_bar = maxdiff(key.cpu(), key_ref), 3e-2 * max(1.0, key_ref.abs().max().item())
    else:
        key_err, key_bar = rel_l2(key, key_ref), R3.engine_bound("bf16", z)
    plain = m["grad_plain"][p_drop > 0]
    lora_bar = (lambda k: RL.grad_bar(z, k, p_drop) if ("ebf/" + k) in z.files else plain) if z is not None else (lambda k: plain)
    errs = {k: rel_l2(got[k], ref) for k, ref in gl.items() if float(ref.abs().max()) != 0.0}
    for k, ref in gl.items():
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
    worst = max(errs, key=lambda k: errs[k] / lora_bar(k))
    # the bias gradients: the project's LoRA-gradient bar on each layer's vector and on every tensor that carries at least 1e-3 of it
    bias_bar = RB.BAR_LOOSE if (p_drop > 0 or m["D"] == 256) else RB.BAR
    berrs = RB.errors(got, gb, sd, scale=ga)          # (a layer whose only trained bias is the key's: a cancelled sum, judged at the scale of its terms)
    bworst = max(berrs, key=berrs.get) if berrs else None
    print(f"lora_bias {tag} {targets} p={p_drop} streams={streams}: key {key_err:.3e} (bar {key_bar:.2e}); worst LoRA gradient {errs[worst]:.3e} of bar {lora_bar(worst):.2e} "
          f"({worst}); bias gradients: worst layer vector {max([e for k, e in berrs.items() if k.startswith('layer')], default=0.0):.3e}, worst tensor "
          f"{max([e for k, e in berrs.items() if not k.startswith('layer')], default=0.0):.3e} ({bworst}) (bar {bias_bar:.0e})")
    assert key_err < key_bar, (key_err, key_bar)
    for k, e in errs.items():
        assert e < lora_bar(k), (k, e, lora_bar(k))
    for k, e in berrs.items():
        assert e < bias_bar, (k, e, bias_bar)
    trained = RB.bias_names(sd, targets)
    assert sorted(gb) == sorted(trained)
    for k in trained:                                               # the last layer: exact zeros everywhere but the key's, whose gradient is the largest there is
        if k.startswith(f"{lay}{L - 1}.") and RB.leaf_of(k) not in RB.KEY_LEAVES:
            assert float(gb[k].abs().max()) == 0.0 and float(got[k].abs().max()) == 0.0, k
    if any(RB.leaf_of(k) in RB.KEY_LEAVES for k in trained):
        assert f"layer {L - 1}" in berrs and float(got[next(k for k in trained if k.startswith(f"{lay}{L - 1}.") and RB.leaf_of(k) in RB.KEY_LEAVES)].abs().max()) > 0
    if tag == "g46":
        assert not any("k_proj.bias" in k for k in got) and eng.bias_off[1] is None
        assert (eng.bias_numel == 0) == (which == 1)
    if tag == "swiglu" and which == 2:                              # the padded columns of the weights_in bias: gradient exact zeros
        o = eng.bias_off[3]
        assert float(eng.lora_grad[:, o:o + 768].reshape(L, -1, 2, 4)[:, 86:].abs().max()) == 0.0
    for p, on in enumerate(eng.targets):                          # untargeted projections: parameters and gradients exactly zero, as ever
        if not on:
            for sl in eng._slices(p):
                assert float(eng.lora[:, sl].abs().max()) == 0.0 and float(eng.lora_grad[:, sl].abs().max()) == 0.0, p
    if p_drop == 0:                                                 # a second pass on the same engine (no mask depends on the step): bit-identical
        first = eng.lora_grad.clone()
        eng.forward_train(img.to(DEV))
        assert torch.equal(eng.backward(dkey.to(DEV)), first)


# ------------------------------------------------------------------------------------------------ 5. "none", and "lora_only" with no bias to train
@pytest.mark.parametrize("tag,which,bias", [("g8", 2, "none"), ("swiglu", 2, "none"), ("g46", 1, "none"), ("g46", 1, "lora_only")])
def test_nothing_to_train_is_the_engine_without_the_argument(tag, which, bias):
    m = model(tag)
    targets = m["sets"][which]
    lora = lora_of(m, targets)
    img, dkey = (t.to(DEV) for t in m["inputs"])
    out = []
    for kw in ({}, {"bias": bias}):
        eng = ViTLoRAEngine(m["sd"], heads=m["heads"], r=m["r"], lora_alpha=m["alpha"], eps=m["eps"], device=DEV, generator=torch.Generator().manual_seed(3),
                            target_modules=list(targets), lora_dropout=0.05, seed=5, **m["kw"], **kw)
        eng.load_lora_state_dict(lora)
        assert eng._bias_table(eng.lora_grad) is None and eng.bias_numel == 0 and eng.bias == kw.get("bias", "none")
        key = eng.forward_train(img).clone()
        out.append((eng.lora.numel(), eng.lora.clone(), key, eng.backward(dkey).clone(), eng.forward_nograd(img).clone(), sum(w.numel() for w in eng._tside_ws if w is not None)))
    for a, b in zip(*out):
        assert a == b if isinstance(a, int) else torch.equal(a, b)


def test_the_new_tier_with_a_null_table_is_lora_out_ex():
    """ucod_vit_backward_lora_bias / ucod_vit_train_workspace_bytes_lora_bias with bias_table_host = NULL against the _lora_out_ex forms: the same bytes, and from
    the same saved workspace the same gradients bit for bit.  With the table, every gradient in front of the biases is still the same."""
    m = model("g8")
    targets = m["sets"][2]
    lora = lora_of(m, targets)
    eng = bias_engine(m, targets, lora, lora_dropout=0.05, seed=1234)
    eng.train_streams = 1
    x, dkey = (t.to(DEV) for t in m["inputs"])
    eng.forward_train(x)
    seed = eng._chunk_seed[0]
    grad = eng.backward(dkey).clone()
    torch.cuda.synchronize()
    lib, P, st, B = eng.lib, N.ptr, N.stream(), x.shape[0]
    t = eng._train_desc(B, 70, 70, seed)
    base = eng.lora.shape[1] - eng.bias_numel
    results = {}
    for name in ("ex", "bias NULL", "bias table"):
        g = torch.full_like(eng.lora_grad, 7.0)
        T, TT, TM, keep = eng._tables(5, 5, g)
        TO, TB = eng._out_table(g), eng._bias_table(g)
        lead = (C.byref(t), eng.mlp, eng._out_flags)
        n_ex = lib.ucod_vit_train_workspace_bytes_lora_out_ex(*lead, TM, TO)
        assert lib.ucod_vit_train_workspace_bytes_lora_bias(*lead, TM, TO, None) == n_ex
        n_tb = lib.ucod_vit_train_workspace_bytes_lora_bias(*lead, TM, TO, TB)
        assert n_tb == eng._tside_ws[0].numel() > n_ex
        ws, k = torch.zeros(n_tb, dtype=torch.uint8, device=DEV), torch.empty(B, 128, 5, 5, device=DEV)
        assert lib.ucod_vit_forward_train_lora_out_ex(*lead, T, TT, TM, TO, P(x), P(k), P(ws), n_tb, st) == 0
        if name == "ex":
            assert lib.ucod_vit_backward_lora_out_ex(*lead, T, TT, TM, TO, P(dkey), P(ws), n_ex, st) == 0
        else:
            assert lib.ucod_vit_backward_lora_bias(*lead, T, TT, TM, TO, TB if name == "bias table" else None, P(dkey), P(ws), n_tb, st) == 0
        torch.cuda.synchronize()
        results[name] = g
    assert torch.equal(results["ex"], results["bias NULL"])
    assert bool((results["ex"][:, base:] == 7.0).all())             # without the table nothing writes the bias slots
    assert torch.equal(results["bias table"][:, :base], results["ex"][:, :base]) and torch.equal(results["bias table"], grad)
    # a workspace of the _lora_out_ex size is too small for the pass with the table
    T, TT, TM, keep = eng._tables(5, 5, eng.lora_grad)
    assert lib.ucod_vit_backward_lora_bias(C.byref(t), eng.mlp, eng._out_flags, T, TT, TM, eng._out_table(eng.lora_grad), eng._bias_table(eng.lora_grad), P(dkey),
                                           P(eng._tside_ws[0]), n_ex, st) == -2


# ------------------------------------------------------------------------------------------------ 6. the runner
def train_three_steps(tmp_path, tag):
    from safetensors.torch import save_file
    from ucod_dpl_amd.engine.config import CfgNode
    from ucod_dpl_amd.engine.runner import StandardRunner, TrainLoop
    from ucod_dpl_amd.models.modules.full_model import load_lora
    sd = model("g8")["sd"]
    weights = tmp_path / f"weights_{tag}"
    weights.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(weights / "model.safetensors"))
    (weights / "config.json").write_text(json.dumps({"model_type": "dinov2", "num_attention_heads": 2, "layer_norm_eps": 1e-6}))
    cfg = CfgNode(dict(
        model_cfg=dict(dim=128, feature_size=8, ema_weight=0.99, dis_use_features=False),
        lora_cfg=dict(r=2, lora_alpha=4, lora_dropout=0.05, target_modules=["query", "value", "dense"], allow_out=True, bias="lora_only"),
        train_cfg=dict(max_epoch=25, start_epoch=0, start_finetune=-5, lr0=6e-4, dis_lr0=1e-3, step_lr_size=2, dis_step_lr_size=2, deterministic=True,
                       step_lr_gamma=0.95, dis_step_lr_gamma=0.95, merge_alpha=0.5, merge_method="dis", dist_train=False, dis_epoch=1,
                       dis_intertrain=2, save_cfg=dict(save_mode="model", save_interval=5, start_save=-50)),
        val_cfg=dict(enable_val=False, val_interval=5, start_val=-50),
        dataset_cfg=dict(feature_extractor_cfg=dict(type="dinov2", backbone_type="huggingface", backbone="facebook/dinov2-base", backbone_weights=str(weights))),
        log_cfg=dict(log_interval=50, log_path=str(tmp_path / f"log_{tag}"), multi_rank=[0])))
    torch.manual_seed(3)
    runner = StandardRunner(cfg)
    loop = TrainLoop(cfg, runner)
    eng = load_lora(cfg.lora_cfg, sd, heads=2, device=DEV, generator=torch.Generator().manual_seed(1)).engine
    loop.attach_lora_backbone(eng)
    start = (eng.lora.clone(), loop.lora_engine_ema.lora.clone(), [[t.clone() for t in (row[N.QKV_B], row[N.FC1_B], row[N.PROJ_B], row[N.FC2_B])] for row in eng.layers])
    img = load_golden("g8_dinov2_native")["x"].to(DEV)
    pl = (torch.rand(2, 1, 16, 16, generator=torch.Generator().manual_seed(11)) > 0.5).float()
    for _ in range(3):
        loss = loop._process_batch_full(img, pl)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss))
    return eng, loop.lora_engine_ema, start


def test_training_moves_what_it_should(tmp_path):
    sd = model("g8")["sd"]
    eng, ema, (lora0, ema0, bias0) = train_three_steps(tmp_path, "a")
    D, L = 128, 3
    assert eng.bias == ema.bias == "lora_only" and tuple(o is not None for o in eng.bias_off) == (True, False, True, False, True, False)
    assert ema._bias_flat.data_ptr() != eng._bias_flat.data_ptr() and ema.layers[0][N.QKV_B].data_ptr() != eng.layers[0][N.QKV_B].data_ptr()
    for e, first in ((eng, lora0), (ema, ema0)):
        for j in (0, 2, 4):
            o = e.bias_off[j]
            assert bool((e.lora[:L - 1, o:o + D] != first[:L - 1, o:o + D]).any(dim=1).all()), j          # every layer below the last: moved (the student and the EMA copy)
            assert float(e.lora[L - 1, o:o + D].abs().max()) == 0.0, j                                      # the last layer's slot: an exact zero stays at zero
        for i, (row, (qkv_b, fc1_b, proj_b, fc2_b)) in enumerate(zip(e.layers, bias0)):
            # the engine's own bias vectors follow the arena (repack): targeted thirds below the last layer moved and equal the arena; the key third, fc1 and fc2 keep their bits
            assert torch.equal(row[N.QKV_B][D:2 * D], qkv_b[D:2 * D]) and torch.equal(row[N.FC1_B], fc1_b) and torch.equal(row[N.FC2_B], fc2_b), i
            for j, (now, was) in ((0, (row[N.QKV_B][:D], qkv_b[:D])), (2, (row[N.QKV_B][2 * D:], qkv_b[2 * D:])), (4, (row[N.PROJ_B], proj_b))):
                if i < L - 1:
                    assert not torch.equal(now, was) and torch.equal(now, e.lora[i, e.bias_off[j]:e.bias_off[j] + D]), (i, j)
                else:
                    assert torch.equal(now, was), (i, j)                                                    # (the last layer's Q bias feeds forward_with_cls_attention of a merged engine)
    assert not torch.equal(eng.lora, ema.lora)
    # every last-layer bias equals the checkpoint's in both dicts (no key is targeted here)
    lsd, merged = eng.lora_state_dict(), eng.merged_state_dict()
    for mod in ("attention.attention.query", "attention.attention.value", "attention.output.dense"):
        k = f"encoder.layer.{L - 1}.{mod}.bias"
        assert torch.equal(lsd[k].cpu(), sd[k]) and torch.equal(merged[k].cpu(), sd[k]), k
        k0 = f"encoder.layer.0.{mod}.bias"
        assert not torch.equal(lsd[k0].cpu(), sd[k0]) and torch.equal(merged[k0].cpu(), lsd[k0].cpu()), k0
    for k in ("encoder.layer.0.attention.attention.key.bias", "encoder.layer.0.mlp.fc1.bias", "encoder.layer.0.mlp.fc2.bias"):
        assert k not in lsd and merged[k] is sd[k], k
    # two runs from the same seed: identical arenas, student and teacher
    eng2, ema2, _ = train_three_steps(tmp_path, "b")
    assert torch.equal(eng2.lora, eng.lora) and torch.equal(ema2.lora, ema.lora)


# ------------------------------------------------------------------------------------------------ 7. merging, the adapter
SPLIT3_G8_BAR = 3e-6            # tests/test_gpu_lora_merge.py (tests/test_gpu_split.py::test_split_engine_against_reference_golden, terms=3 on this golden)
FOLDED_BAR = 3e-3               # tests/test_gpu_lora_merge.py: the folded fp16 default at D = 256


def test_merged_state_dict_carries_the_trained_biases(tmp_path):
    from safetensors.torch import load_file
    from ucod_dpl_amd.models.modules.full_model import load_lora_adapter, save_lora_adapter
    m = model("g8")
    sd, heads, targets = m["sd"], m["heads"], m["sets"][2]
    lora, moved = lora_of(m, targets), RB.perturbed_biases(m["sd"], m["sets"][2])
    eng = bias_engine(m, targets, lora, biases=moved)
    img = load_golden("g8_dinov2_native")["x"]
    full = {k: v.to(DEV, torch.float64) for k, v in {**sd, **lora, **moved}.items() if v.is_floating_point()}
    ref = RO.forward(img.to(DEV, torch.float64), full, heads, eng.scaling).cpu()
    merged = eng.merged_state_dict()
    assert sorted(merged) == sorted(sd)
    for k, v in moved.items():
        assert torch.equal(merged[k], v) and not torch.equal(v, sd[k]), k
    x = img.to(DEV)
    e_merged = rel_l2(SplitViTEngine(merged, heads=heads, device=DEV, terms=3)(x), ref)
    e_without = rel_l2(SplitViTEngine({**merged, **{k: sd[k] for k in moved}}, heads=heads, device=DEV, terms=3)(x), ref)
    print(f"merged with trained biases: split3 {e_merged:.2e} (bar {SPLIT3_G8_BAR:.0e}); with the biases left unmerged {e_without:.2e}")
    assert e_merged < SPLIT3_G8_BAR and e_without > 100 * SPLIT3_G8_BAR
    # the training engine itself runs the perturbed biases (repack carried them into its own bias vectors): its key map is the f64 one at bf16 accuracy
    k_train = eng.forward_train(x)
    assert maxdiff(k_train.cpu(), ref) < 3e-2 * max(1.0, ref.abs().max().item())
    # adapter folder -> a fresh engine: the same arena, the same bias vectors, the config says lora_only
    folder = save_lora_adapter(eng, str(tmp_path / "lora"))
    assert json.load(open(os.path.join(folder, "adapter_config.json")))["bias"] == "lora_only"
    tensors = load_file(os.path.join(folder, "adapter_model.safetensors"))
    pre = "base_model.model.ViT.encoder.layer."
    assert sorted(tensors) == sorted(pre + k[len("encoder.layer."):] for k in list(lora) + list(moved))
    other = bias_engine(m, targets, RO.lora_for(sd, targets, seed=99))
    assert not torch.equal(other.lora, eng.lora)
    load_lora_adapter(other, folder)
    assert torch.equal(other.lora, eng.lora) and torch.equal(other._bias_flat, eng._bias_flat)
    with pytest.raises(ValueError, match="bias is 'lora_only'"):
        load_lora_adapter(bias_engine(m, targets, lora, bias="none"), folder)


def test_merge_into_refreshes_biases_and_the_fold():
    """D = 256 (the LayerNorm fold exists): merge_into on the default folded engine against an engine rebuilt from merged_state_dict() under the rules of
    tests/test_gpu_lora_merge.py -- the plain tables bit for bit, the folded weights and column sums bit for bit, the folded biases within one f32 ulp plus
    1e-12 |q| sum |w beta| (f64 summation order)."""
    m = model("d256")
    sd, heads, targets = m["sd"], m["heads"], ("query", "value", "fc1", "dense")
    lora, moved = RO.lora_for(sd, targets), RB.perturbed_biases(sd, targets)
    eng = bias_engine(m, targets, lora, biases=moved)
    vit = ViTEngine(sd, heads=heads, device=DEV)
    assert vit.ln_fold
    x = m["inputs"][0].to(DEV)
    key_base = vit(x).clone()
    before = [[None if t is None else t.clone() for t in row] for row in vit.layers]
    ptrs = [None if t is None else t.data_ptr() for rows in (vit.layers, vit.fold_layers) for row in rows for t in row]
    assert eng.merge_into(vit) is vit
    torch.cuda.synchronize()
    assert ptrs == [None if t is None else t.data_ptr() for rows in (vit.layers, vit.fold_layers) for row in rows for t in row], "merge_into reallocated a tensor"
    merged = eng.merged_state_dict()
    fresh = ViTEngine(merged, heads=heads, device=DEV)
    same = lambda a, b: a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.element_size() == 2 else a, b.view(torch.int16) if b.element_size() == 2 else b)  # noqa: E731
    _, mc = _prepare_mlp(normalize_state_dict(merged))
    worst = 0.0
    for i in range(m["L"]):
        for s, (a, b) in enumerate(zip(vit.layers[i], fresh.layers[i])):
            assert (a is None and b is None) or same(a, b), (i, N.VIT_LAYER_SLOTS[s])
        for s, (a, b) in enumerate(zip(vit.fold_layers[i], fresh.fold_layers[i])):
            if a is not None and s not in (N.QKV_B, N.FC1_B):
                assert same(a, b), (i, N.VIT_LAYER_SLOTS[s])
        for slot_b, wname, bname in ((N.QKV_B, "qkv_w", "ln1_b"), (N.FC1_B, "fc1_w", "ln2_b")):
            got, want = vit.fold_layers[i][slot_b].cpu(), fresh.fold_layers[i][slot_b].cpu()
            q = vit.q_row_scale.cpu().double() if slot_b == N.QKV_B else torch.ones(got.numel(), dtype=torch.float64)
            ulp = (torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()).double()
            tol = ulp + 1e-12 * q * (mc["layers"][i][wname].double().abs() @ mc["layers"][i][bname].double().abs())
            err = (got.double() - want.double()).abs()
            worst = max(worst, float((err / ulp).max()))
            assert bool((err <= tol).all()), (i, N.VIT_LAYER_SLOTS[slot_b], float((err / tol).max()))
        # the trained biases are in the live vectors; the key third and fc2's keep their bits
        D = 256
        assert not torch.equal(vit.layers[i][N.QKV_B][:D], before[i][N.QKV_B][:D]) and torch.equal(vit.layers[i][N.QKV_B][D:2 * D], before[i][N.QKV_B][D:2 * D])
        assert not torch.equal(vit.layers[i][N.PROJ_B], before[i][N.PROJ_B]) and torch.equal(vit.layers[i][N.FC2_B], before[i][N.FC2_B])
    full = {k: v.to(DEV, torch.float64) for k, v in {**sd, **lora, **moved}.items() if v.is_floating_point()}
    ref = RO.forward(x.double(), full, heads, eng.scaling).cpu()
    k_live, k_fresh = vit(x), fresh(x)
    vit.check_overflow(wait=True)
    e_live, e_fresh = rel_l2(k_live, ref), rel_l2(k_fresh, ref)
    print(f"merge_into with trained biases, D = 256: live {e_live:.2e}, fresh {e_fresh:.2e} (bar {FOLDED_BAR:.0e}), live vs fresh {rel_l2(k_live, k_fresh):.2e}, "
          f"folded bias worst {worst:.2f} ulp, unrefreshed {rel_l2(key_base, ref):.2e}")
    assert e_live < FOLDED_BAR and e_fresh < FOLDED_BAR and rel_l2(key_base, ref) > 5 * e_live
