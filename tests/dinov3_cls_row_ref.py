"""Test helper: the CLS query's softmax row of the LAST layer of a DINOv3 ViT (``outputs.attentions[-1][:, :, 0, :]`` of transformers' eager DINOv3ViTModel), as
an f64 restatement on a flat HF-named state dict, with the faults a kernel or an engine can make on that row as switches.  It imports tests/dinov3_ref.py (the pass
itself, its table builder, ``rotate``) and changes nothing there.

In the last layer, as in every layer, only the PATCH tokens' q and k are rotated: the CLS query, the CLS key and the register keys are not.  So for one head, the
CLS query q, a patch's unrotated key k_j and its table row (c_j[0:32] | s_j[0:32]):

    score_j = scale * q . rotate(k_j) = scale * sum_{i<32} c_j[i] (q[i] k_j[i] + q[i+32] k_j[i+32]) + s_j[i] (q[i+32] k_j[i] - q[i] k_j[i+32])

``forward`` runs the pass and forms the row with ``dinov3_ref.rotate`` on the keys; ``cls_row`` is the regrouped right-hand side on the operands of
ucod_cls_attention_rope (q, k_lead, key_map, table) -- the sum the kernel takes, in another order of the same products: no rotated key is formed;
tests/test_dinov3_cls_row_host.py shows the two equal in f64.

Faults (all on the last layer's row alone: the layers below, and with them the key map, stay right):
    unrotated_keys    the patch keys enter the product as the key map holds them (what ucod_cls_attention_reg computes on a DINOv3 checkpoint)
    sin_sign          the sine's sign flipped
    swap_yx           the table's y and x blocks swapped
    rotate_lead       the CLS and register keys rotated too, key r by the row of patch r
    rotate_query      the CLS query rotated too, by the row of patch 0
    half_partner      the partner of column i taken 16 columns on, not 32
    table_row_shift   patch j reads the table row j + 1 (modulo hw)
    no_reg_keys       the register keys left out of the softmax's maximum and denominator (vacuous without register tokens: ``faults_for``)

``bkg_seg`` restates oracle/pseudo_label.py's function of that name without its resampler: the oracle resizes the grid to (up, up), the identity on a square grid
only, and the generator never resizes (up_size = grid).  tests/golden/make_golden_dinov3_cls_row.py checks it against the oracle's on the square golden and uses it on
the 4 x 6 one.

It runs in the dtype of the inputs (f64 as the reference).  Nothing under ucod_dpl_amd/ imports this file.

The engine rows of tests/test_gpu_dinov3_cls_row.py are dinov3_ref.ENGINE_ROWS, and ``engine_bound`` is dinov3_ref.engine_bound's rule applied to the figures a
G25 file stores for the ROW (transformers' own f32 / autocast runs against its f64 run).
"""
import torch

from oracle import vit as OV
import dinov3_ref as R3

FAULTS = ("unrotated_keys", "sin_sign", "swap_yx", "rotate_lead", "rotate_query", "half_partner", "table_row_shift", "no_reg_keys")
GOLDEN_NAME = "g25_dinov3_cls_row_{tag}.npz"
GENERATOR_TAGS = ("g66", "g46")                                  # the goldens that also store cos_row / mask / th for the whole generator


def faults_for(R):
    """the faults that change anything on a model with R register tokens"""
    return tuple(f for f in FAULTS if R > 0 or f != "no_reg_keys")


def table(gh, gw, theta=100.0, fault=None):
    """[n, 64] = (cos 32 | sin 32): the layout of vit_engine.rope_table, from dinov3_ref's own builder (in f32, as the model computes it)"""
    cos, sin = R3.cos_sin(gh, gw, theta, fault if fault in ("swap_yx", "sin_sign") else None)
    return torch.cat((cos, sin), 1)


def _half_rotate(v, c, s):
    """[..., 64] rotated by c, s [..., 32] (broadcast): out[i] = v[i] c[i] - v[i + 32] s[i], out[i + 32] = v[i + 32] c[i] + v[i] s[i]"""
    a, b = v[..., :32], v[..., 32:]
    return torch.cat((a * c - b * s, b * c + a * s), -1)


def cls_row(q, k_lead, key_map, tab, heads, scale=0.125, fault=None):
    """The kernel's operands -> (att [B, heads, hw], lead [B, heads, 1 + R]): q [B, D], k_lead [B, 1 + R, D], key_map [B, D, hw] (or [B, D, gh, gw]) unrotated,
    tab [hw, 64] or None (no rotation: ucod_cls_attention_reg's row).  Plain arithmetic in the operands' dtype, the regrouped formula of the header."""
    assert fault is None or fault in FAULTS
    B, D = q.shape
    key_map = key_map.reshape(B, D, -1)
    hw, R = key_map.shape[-1], k_lead.shape[1] - 1
    qh = q.reshape(B, heads, 64)
    kh = key_map.reshape(B, heads, 64, hw)
    kl = k_lead.reshape(B, 1 + R, heads, 64).permute(0, 2, 1, 3)                   # [B, heads, 1 + R, 64]
    if tab is None or fault == "unrotated_keys":
        s = torch.einsum("bhd,bhdj->bhj", qh, kh)
    else:
        tab = tab.to(q.dtype)
        if fault == "table_row_shift":
            tab = tab.roll(-1, 0)
        c, sn = tab[:, :32].t(), tab[:, 32:].t()                                   # [32, hw]
        step = 16 if fault == "half_partner" else 32
        if fault == "rotate_query":
            qh = _half_rotate(qh, tab[0, :32], tab[0, 32:])
        qa, qp = qh[..., :32, None], qh[..., step:step + 32, None]
        ka, kp = kh[:, :, :32], kh[:, :, step:step + 32]
        s = (c * (qa * ka + qp * kp) + sn * (qp * ka - qa * kp)).sum(2)
    if fault == "rotate_lead" and tab is not None:
        assert hw >= 1 + R
        kl = _half_rotate(kl, tab[:1 + R, :32].to(q.dtype), tab[:1 + R, 32:].to(q.dtype))
    sl = torch.einsum("bhd,bhrd->bhr", qh, kl)                                       # (a rotated query meets the CLS and register keys rotated as well)
    if fault == "no_reg_keys":
        sl = sl[..., :1]
    p = torch.softmax(torch.cat((sl, s), -1) * scale, -1)
    n_lead = sl.shape[-1]
    return p[..., n_lead:], p[..., :n_lead]


def forward(img, sd, heads, eps=1e-5, theta=100.0, patch=16, fault=None, operands=False):
    """(key [B, D, gh, gw] unrotated, att [B, heads, n], lead [B, heads, 1 + R]): DINOv3ViTModel up to the last layer's attention probabilities, row 0 -- the patch
    columns and the CLS / register columns.  Without a fault the row is formed as the model forms it (keys rotated by ``dinov3_ref.rotate``, one softmax over all
    tokens); with one, by ``cls_row`` with that fault.  ``operands``: return instead what ``cls_row`` takes -- (q [B, D], k_lead [B, 1 + R, D], key [B, D, n], table)."""
    assert fault is None or fault in FAULTS
    B, _, H, W = img.shape
    gh, gw = H // patch, W // patch
    n = gh * gw
    x = OV.patch_embed(img, sd["embeddings.patch_embeddings.weight"], sd["embeddings.patch_embeddings.bias"], patch)
    reg = sd["embeddings.register_tokens"]
    R = reg.shape[1]
    x = torch.cat((sd["embeddings.cls_token"].expand(B, -1, -1), reg.expand(B, -1, -1), x), 1)
    cos, sin = R3.cos_sin(gh, gw, theta)
    pre = "model.layer." if any(k.startswith("model.layer.") for k in sd) else "layer."
    L = 1 + max(int(k[len(pre):].split(".")[0]) for k in sd if k.startswith(pre))
    D = x.shape[-1]
    lin = lambda t, name: t @ sd[name + ".weight"].t() + (sd[name + ".bias"] if name + ".bias" in sd else 0)  # noqa: E731

    def rot(t):
        t = t.reshape(B, 1 + R + n, heads, 64)
        return torch.cat((t[:, :1 + R], R3.rotate(t[:, 1 + R:], cos, sin)), 1).reshape(B, -1, D)

    for i in range(L):
        p = f"{pre}{i}."
        h = OV.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        q, k = lin(h, p + "attention.q_proj"), lin(h, p + "attention.k_proj")
        if i == L - 1:
            key = k[:, 1 + R:].reshape(B, gh, gw, D).permute(0, 3, 1, 2)
            if operands:
                return q[:, 0], k[:, :1 + R], key.reshape(B, D, n), table(gh, gw, theta)
            if fault is not None:
                att, lead = cls_row(q[:, 0], k[:, :1 + R], key, table(gh, gw, theta, fault), heads, fault=fault)
                return key, att, lead
            qr = rot(q).reshape(B, -1, heads, 64)[:, 0]                              # [B, heads, 64]: the CLS query (rot leaves it as it is)
            kr = rot(k).reshape(B, -1, heads, 64)
            row = torch.softmax(torch.einsum("bhd,bthd->bht", qr, kr) * 0.125, -1)
            return key, row[..., 1 + R:], row[..., :1 + R]
        v = lin(h, p + "attention.v_proj")
        o = lin(OV.attention(rot(q), rot(k), v, heads), p + "attention.o_proj")
        x = o * sd[p + "layer_scale1.lambda1"] + x
        h = OV.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        if p + "mlp.gate_proj.weight" in sd:
            h = torch.nn.functional.silu(lin(h, p + "mlp.gate_proj")) * lin(h, p + "mlp.up_proj")
        else:
            h = OV.gelu_erf(lin(h, p + "mlp.up_proj"))
        x = lin(h, p + "mlp.down_proj") * sd[p + "layer_scale2.lambda1"] + x


def forward_f64(img, sd, heads, **kw):
    sdd = {k: v.to(torch.float64) for k, v in sd.items()}
    return forward(img.to(torch.float64), sdd, heads, **kw)


def last_layer_operands_f64(img, sd, heads, **kw):
    """(q [B, D], k_lead [B, 1 + R, D], key_map [B, D, n], table [n, 64]) in f64: what an exact engine would hand ucod_cls_attention_rope on this model"""
    sdd = {k: v.to(torch.float64) for k, v in sd.items()}
    return forward(img.to(torch.float64), sdd, heads, operands=True, **kw)


def bkg_seg(att, key_map, th_bkg, epsilon=1e-10):
    """oracle.pseudo_label.bkg_seg (apply_weights, up_size = grid) without its resampler, for any grid: att [B, heads, n] patch columns (the oracle drops the CLS
    column it is handed), key_map [B, D, gh, gw].  -> (bkg_mask [B, gh, gw], cos_row)."""
    B, nh, n = att.shape
    _, D, gh, gw = key_map.shape
    thr = att.reshape(B, -1).mean(1)
    Q = (att > thr[:, None, None]).sum(2) / n
    beta = torch.log((Q + epsilon).sum(1)[:, None] / (Q + epsilon))
    d = key_map.reshape(B, nh, 64, n).permute(0, 3, 1, 2) * beta[:, None, :, None]
    d = torch.nn.functional.normalize(d.reshape(B, n, D), dim=-1, p=2)
    ref = (att * beta[:, :, None]).sum(1).argmin(-1)
    row = torch.einsum("bc,bpc->bp", d[torch.arange(B), ref], d).reshape(B, gh, gw)
    return (row > th_bkg).float(), row


def engine_bound(precision, z):
    """dinov3_ref.engine_bound on a G25 file: 4 x err_f32 + 1e-7 (split3 / split2h / split2hf), ten times that (split2), 3 x err_f16ac (fp16 operands),
    3 x err_bf16ac (bf16) -- the figures being those of the ROW."""
    return R3.engine_bound(precision, z)


def widest_bound(tag, z, rows=None):
    """the widest bound of any engine row that runs on the golden ``tag`` (``rows``: among these precisions only)"""
    return max(engine_bound(p, z) for p, t in R3.ENGINE_ROWS if t == tag and (rows is None or p in rows))


# The golden script's condition is that every fault lies at least 10 x the widest engine bound of its golden away.  Measured (make_golden_dinov3_cls_row.py prints
# them), these pairs do not: the two faults that move the row by the attention mass of the CLS / register keys alone, on the models where that mass is small
# (register mass 0.2 % on r1 and d256; r0 has no register and a CLS mass of 0.5 %).  Distance, in units of the widest bound (fp16 operands: 3 x err_f16ac; on d256
# bf16: 3 x err_bf16ac):
#     g66 no_reg_keys 3.04e-2 = 8.7 x      r1 no_reg_keys 2.40e-3 = 0.72 x      d256 no_reg_keys 2.31e-3 = 0.09 x      r0 rotate_lead 2.91e-2 = 8.9 x
# For them the script asserts the condition against the widest bound of the f32-class rows (SPLIT_ROWS, at most 4e-5: met by 60 x and more), which run on every
# golden, and that each pair listed here does miss the full condition, so that the list cannot go stale.  The kernel test, whose bound is ~1e-6 at n_reg = 0, 1, 4,
# is what tells these two faults apart at the 16-bit rows' precision.
UNDER_TEN_WIDEST = (("g66", "no_reg_keys"), ("r1", "no_reg_keys"), ("d256", "no_reg_keys"), ("r0", "rotate_lead"))


def fault_floor(tag, fault, z):
    """what the distance of ``fault`` on the golden ``tag`` must reach: 10 x the widest bound (of the f32-class rows for the pairs of UNDER_TEN_WIDEST)"""
    return 10.0 * widest_bound(tag, z, R3.SPLIT_ROWS if (tag, fault) in UNDER_TEN_WIDEST else None)
