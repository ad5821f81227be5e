#!/usr/bin/env python3
"""Generate tests/golden/g29_refiner_outputs_grad.npz: the REAL reference SparseRefiner in .train() on the G9 inputs (refiner_init, seed 9, perturb_;
tags full / partial, targets of kind prob), differentiated through `outputs`.

Run where the reference is present only:
    python tests/golden/make_golden_refiner_outputs.py
The import recipe (stubs of the absent third-party modules) is make_golden.py's, taken by importing it.  Only data is written.

For each tag and each of the two losses  "out": <G, outputs>  and  "both": <G, outputs> + ex_loss  (G = randn, seed G_SEED):
  * the four GE.fuser gradients, whole;
  * d loss / d window_preds, taken with retain_grad;
  * every 1-D HRE.CSF gradient, whole;
  * for every HRE.CSF gradient of more dimensions (the full matrices are tens of MB): its Frobenius norm and its inner product with a seeded randn of
    its shape (probe(name, shape)), as float64;
  * whether GE.alpha received a gradient (it does not: the forward never reads it);
and per tag the smallest |z| of the fuser's 64 pre-activations over all pixels in the reference's own f32 run, with the counts below 1e-5 and 1e-3 and the gates m_k = [z_k > 0] themselves (uint8).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

G_SEED = 29
LOSSES = ("out", "both")
TAGS = ("full", "partial")


def probe(index, shape):
    """the seeded randn a matrix gradient is projected on: index = the parameter's position in HRE.CSF.named_parameters()"""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(2900 + index), dtype=torch.float64)


def cotangent():
    return torch.randn(2, 1, 18, 18, generator=torch.Generator().manual_seed(G_SEED))


def main():
    import make_golden as MG                                           # stubs the absent modules at import, puts the reference on sys.path
    import refiner_init as RI
    from models.UDLR import SparseRefiner
    torch.manual_seed(RI.SEED)
    m = RI.perturb_(SparseRefiner.from_config(MG.CfgNode(dict(window_size=3, threshold=0.0015, dim=768)))).train()
    G = cotangent()
    out = {"G": G}
    ht = RI.make_h_targets("prob")
    for tag in TAGS:
        l, h, preds = RI.make_inputs(tag == "partial")
        for loss_kind in LOSSES:
            m.zero_grad(set_to_none=True)
            outputs, ex, opt = m(l, h, preds, ht)
            opt["window_preds"].retain_grad()
            loss = (outputs * G).sum() + (ex if loss_kind == "both" else 0.0)
            loss.backward()
            k = f"{tag}.{loss_kind}."
            out[k + "alpha_has_grad"] = torch.tensor(float(m.GE.alpha.grad is not None))
            out[k + "d_window_preds"] = opt["window_preds"].grad.clone()
            for name, p in m.GE.fuser.named_parameters():
                out[k + "GE.fuser." + name] = p.grad.clone()
            for i, (name, p) in enumerate(m.HRE.CSF.named_parameters()):
                g = p.grad.double()
                if g.dim() == 1:
                    out[k + "HRE.CSF." + name] = p.grad.clone()
                else:
                    out[k + "HRE.CSF." + name + ".norm"] = g.norm()
                    out[k + "HRE.CSF." + name + ".probe"] = (g * probe(i, g.shape)).sum()
        with torch.no_grad():                                          # the fuser's pre-activations in the reference's own f32 run
            _, _, opt = m(l, h, preds, ht)
            l1 = torch.nn.functional.interpolate(preds, size=opt["h_preds"].shape[-2:], mode="bilinear")
            y = l1 * opt["GE_w"] + opt["h_preds"] * (1 - opt["GE_w"])
            zs = torch.nn.functional.conv2d(y, m.GE.fuser[0].weight, m.GE.fuser[0].bias)
            z = zs.abs()
            out[tag + ".z_f32_min"] = z.min().double()
            out[tag + ".z_f32_below_1e-5"] = (z < 1e-5).sum().double()
            out[tag + ".z_f32_below_1e-3"] = (z < 1e-3).sum().double()
            out[tag + ".z_f32_gate"] = (zs > 0).to(torch.uint8)               # m_k of the f32 run, [B,64,h,w]
    MG.save("g29_refiner_outputs_grad", **out)


if __name__ == "__main__":
    main()
