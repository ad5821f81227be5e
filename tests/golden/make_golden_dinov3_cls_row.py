"""G25: the CLS query's softmax row of the LAST layer of transformers' DINOv3ViTModel (eager attention, f64, CPU) on the G22 models -- the pin of the restatement
in tests/dinov3_cls_row_ref.py, of ucod_cls_attention_rope and of ``forward_with_cls_attention(img, allow_rope=True)``.

Weights and inputs are G22's (``dinov3_ref.g22_state_dict(tag)`` / ``g22_input(tag)``) and are NOT stored; the SHA-256 of the weights is, as in G22.  The model is
the f64 one with the f32 ``inv_freq`` buffer put back (make_golden_dinov3.py: the angles are f32 in the model and in every engine).  Stored per file, from
``model(x, output_attentions=True).attentions[-1][:, :, 0]``:

  att   f64 [B, heads, n]        the patch columns
  lead  f64 [B, heads, 1 + R]    the CLS and register columns
  err_f32 / err_f16ac / err_bf16ac   relative L2 of transformers' own f32 run and its runs under torch.autocast("cpu", float16 / bfloat16) of ``att`` against it
  fault_<name>                   the restatement with one fault of dinov3_cls_row_ref.FAULTS switched on (no_reg_keys only where R > 0)

and for the generator test, on g66 and g46: ``cos_row`` / ``mask`` (f64 [B, gh, gw]) of the background discovery on the f64 row and the f64 G22 key map, and the
threshold ``th`` they were made with -- 0.6 if background and foreground then each hold at least 10 % of the patches, otherwise the median of cos_row rounded to
0.05.  On the square grid they come from oracle.pseudo_label.bkg_seg (CLS column and CLS row in place, register columns and rows dropped); the oracle resizes to
(up, up), which is the identity on a square grid only, so on 4 x 6 they come from dinov3_cls_row_ref.bkg_seg, which this script checks against the oracle's on
the square one.

Asserted before anything is written, so that a toothless golden cannot be: the restatement within 1e-10; every fault at least 10 x the widest engine bound of the
golden away (dinov3_cls_row_ref.fault_floor: the four pairs of UNDER_TEN_WIDEST, listed there with their figures, against the f32-class rows' bound instead); at
least 95 % of cos_row further than 1e-5 from th.

    python tests/golden/make_golden_dinov3_cls_row.py      (needs transformers >= 5 with models/dinov3_vit; writes tests/golden/g25_dinov3_cls_row_<tag>.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/ (dinov3_ref, dinov3_cls_row_ref)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle)
from transformers import DINOv3ViTConfig, DINOv3ViTModel  # noqa: E402
from oracle import pseudo_label as OPL  # noqa: E402
import dinov3_ref as R3  # noqa: E402
import dinov3_cls_row_ref as C3  # noqa: E402


def hf_row(model, x, autocast=None):
    """attentions[-1][:, :, 0, :] -> [B, heads, tok]"""
    with torch.no_grad():
        if autocast is None:
            out = model(x, output_attentions=True)
        else:
            with torch.autocast("cpu", dtype=autocast):
                out = model(x, output_attentions=True)
    return out.attentions[-1][:, :, 0, :].detach()


def main():
    for tag, m in R3.G22.items():
        sd = R3.g22_state_dict(tag)
        gh, gw = m["grid"]
        R, nl = m["R"], 1 + m["R"]
        cfg = DINOv3ViTConfig(hidden_size=m["D"], num_hidden_layers=R3.G22_LAYERS, num_attention_heads=m["heads"], intermediate_size=m["F"], patch_size=16,
                              image_size=16 * gh, num_register_tokens=R, use_gated_mlp=m["gated"], hidden_act="silu" if m["gated"] else "gelu",
                              layer_norm_eps=1e-5, rope_theta=100.0, attn_implementation="eager")
        model = DINOv3ViTModel(cfg).eval()
        model.load_state_dict(sd, strict=True)
        x = R3.g22_input(tag)
        r32, r16, rb16 = hf_row(model, x)[..., nl:], hf_row(model, x, torch.float16)[..., nl:], hf_row(model, x, torch.bfloat16)[..., nl:]
        inv_freq = model.rope_embeddings.inv_freq.clone()
        model.double()
        model.rope_embeddings.inv_freq = inv_freq
        r64 = hf_row(model, x.double())
        assert r64.dtype == torch.float64 and r64.shape == (R3.G22_B, m["heads"], nl + gh * gw)
        att, lead = r64[..., nl:], r64[..., :nl]
        out = dict(att=att.numpy(), lead=lead.numpy(), seed=np.int64(R3.G22_SEED), gain=np.float64(R3.G22_GAIN), n_reg=np.int64(R),
                   sd_sha256=np.array(R3.weights_sha256(sd)), err_f32=np.float64(R3.rel_l2(r32, att)), err_f16ac=np.float64(R3.rel_l2(r16, att)),
                   err_bf16ac=np.float64(R3.rel_l2(rb16, att)))
        key, own_att, own_lead = C3.forward_f64(x, sd, m["heads"])
        own = max(R3.rel_l2(own_att, att), R3.rel_l2(own_lead, lead))
        assert own < 1e-10, own
        g22 = np.load(os.path.join(HERE, f"g22_dinov3_{tag}.npz"))
        assert R3.rel_l2(key, torch.from_numpy(g22["key"])) < 1e-10
        widest = C3.widest_bound(tag, out)
        for f in C3.faults_for(R):
            d = R3.rel_l2(C3.forward_f64(x, sd, m["heads"], fault=f)[1], att)
            assert d >= C3.fault_floor(tag, f, out), (tag, f, d, widest)
            assert ((tag, f) in C3.UNDER_TEN_WIDEST) == (d < 10 * widest), (tag, f, d, widest)
            out["fault_" + f] = np.float64(d)
        if tag in C3.GENERATOR_TAGS:
            key64 = torch.from_numpy(g22["key"])                                              # [B, D, gh, gw] f64
            own_mask, own_row = C3.bkg_seg(att, key64, 0.6)
            th = 0.6
            if not 0.1 <= float(own_mask.mean()) <= 0.9:
                th = round(float(own_row.median()) / 0.05) * 0.05
                own_mask, own_row = C3.bkg_seg(att, key64, th)
            if gh == gw:
                # the oracle takes the row with its CLS column and [B, tok, C] features with a CLS row (which it drops)
                feats = torch.cat((torch.zeros(R3.G22_B, 1, m["D"], dtype=torch.float64), key64.flatten(2).transpose(1, 2)), 1)
                mask, _, row = OPL.bkg_seg(torch.cat((lead[..., :1], att), -1), feats, (gh, gw), th, dim=64, apply_weights=True)
                assert torch.equal(mask, own_mask) and float((row - own_row).abs().max()) < 1e-14, "dinov3_cls_row_ref.bkg_seg is not the oracle's"
            else:
                mask, row = own_mask, own_row
            assert 0.1 <= float(mask.mean()) <= 0.9, (tag, th, float(mask.mean()))
            assert float(((row - th).abs() > 1e-5).double().mean()) >= 0.95
            out.update(cos_row=row.numpy(), mask=mask.numpy(), th=np.float64(th))
        path = os.path.join(HERE, C3.GOLDEN_NAME.format(tag=tag))
        np.savez_compressed(path, **out)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)  restatement {own:.1e}  widest bound {widest:.2e}  " +
              "  ".join(f"{k} {float(v):.2e}" for k, v in out.items() if k.startswith(("err_", "fault_"))) + (f"  th {out['th']}" if "th" in out else ""))


if __name__ == "__main__":
    main()
