"""The oracle's autocast emulation (oracle/vit.py::autocast_rounding: the roundings `accelerate launch --mixed_precision fp16` puts into the
reference's forward, scripts/launch_train_first_stage.sh:20) against torch's own autocast on the real HF Dinov2Model: the emulated forward must
sit much closer to the really-autocast forward than either sits to f32.  bench.py reports the emulated deviation at full size as the second
data point beside the f32 reference ("fp16-autocast reference vs bf16 build")."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vit as OV  # noqa: E402

transformers = pytest.importorskip("transformers")

# torch's CPU autocast forward of the model below, recorded on a CPU with native bf16 and fp16 arithmetic (AVX512-FP16 / AMX): there its 16-bit
# GEMMs run through oneDNN with f32 accumulation, the rounding points of the reference's GPU autocast.  A CPU without native fp16 takes another fp16
# GEMM path, and a 16-bit forward's rounding pattern follows any change of the f32 values before each rounding (a 1e-7 relative change of the input
# moves this fp16 forward by 0.4 of its deviation from f32), so the emulation is held to the recorded forward on every host and the live one is
# checked beside it.  The emulation keeps its values in f32 containers; its f32 GEMMs (MKL) pick a code path per CPU (AVX512 on some, AVX2 on
# others) and so sum in a different order, which moves the fp16 rounding pattern just as much.  It therefore runs in a child process on MKL's
# strict conditional-numerical-reproducibility branch (MKL_CBWR=AVX2,STRICT: the same bits on every x86 CPU with AVX2, any thread count; MKL
# takes the setting only before its first call).  Regenerate the recording: python tests/test_oracle_autocast.py capture
GOLDEN = os.path.join(ROOT, "tests", "golden", "g19_hf_autocast.npz")
KEY = {torch.bfloat16: "bf16", torch.float16: "f16"}
MKL_REPRODUCIBLE = {"MKL_CBWR": "AVX2,STRICT"}


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def _model_and_input():
    cfg = transformers.Dinov2Config(hidden_size=64, num_hidden_layers=3, num_attention_heads=2, mlp_ratio=4, image_size=70, patch_size=14,
                                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, layerscale_value=0.5,
                                    attn_implementation="eager")      # modeling_dinov2.py:153-179, the path SURVEY.md maps
    torch.manual_seed(0)
    model = transformers.Dinov2Model(cfg).eval()
    with torch.no_grad():
        for prm in model.parameters():                       # spread the weights so that the 16-bit roundings are visible above f32 noise
            prm.mul_(3.0)
    return cfg, model, torch.randn(2, 3, 70, 70)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_autocast_emulation_tracks_torch_autocast_on_hf_dinov2(dtype, tmp_path):
    _, model, x = _model_and_input()
    with torch.no_grad():
        ref32 = model(x).last_hidden_state
        try:
            with torch.autocast("cpu", dtype=dtype):
                live = model(x).last_hidden_state.float()
        except RuntimeError as e:                             # a CPU kernel this torch build lacks in that type
            pytest.skip(f"CPU autocast in {dtype} is not runnable here: {e}")
    out = tmp_path / "emulated.npz"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "emulate", KEY[dtype], str(out)], env=dict(os.environ, **MKL_REPRODUCIBLE),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    e = np.load(out)
    emu32, emu = torch.from_numpy(e["f32"]), torch.from_numpy(e["emulated"])
    g = np.load(GOLDEN)
    real = torch.from_numpy(g[KEY[dtype]])                   # torch's autocast forward with f32-accumulating 16-bit GEMMs (recorded)
    assert rel_l2(ref32, torch.from_numpy(g["f32"])) < 1e-5  # the same weights and input as the recorded run
    assert rel_l2(emu32, ref32) < 1e-5                        # the f32 restatement itself (G8 pins it too)
    d_real, d_emu, d_between = rel_l2(real, ref32), rel_l2(emu, ref32), rel_l2(emu, real)
    assert d_real > 1e-4 and d_emu > 1e-4                     # the roundings are visible
    assert 0.5 < d_emu / d_real < 2.0, (d_emu, d_real)        # same size of deviation from f32 ...
    assert d_between < 0.3 * d_real, (d_between, d_real)      # ... and mostly the SAME deviation (measured 0.13 bf16, 0.17 fp16)
    d_live = rel_l2(live, ref32)                              # torch's autocast on this host: the same size of deviation as the recorded one
    assert d_live > 1e-4 and 0.5 < d_live / d_real < 2.0, (d_live, d_real)


def emulate(name, path):
    """The oracle's f32 forward and its emulated autocast forward in `name`'s type, written to `path` (run in a child process; see MKL_REPRODUCIBLE)."""
    cfg, model, x = _model_and_input()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    dtype = {v: k for k, v in KEY.items()}[name]
    with torch.no_grad():
        emu32, _ = OV.dinov2_forward(x, sd, heads=2, patch=14, eps=cfg.layer_norm_eps)
        emu, _ = OV.dinov2_forward(x, sd, heads=2, patch=14, eps=cfg.layer_norm_eps, autocast=dtype)
    np.savez(path, f32=emu32.numpy(), emulated=emu.numpy())


def capture():
    """Writes GOLDEN from this host's torch autocast.  Run it on a CPU with native bf16 and fp16 arithmetic (AVX512-FP16 or AMX-FP16)."""
    assert torch.ops.mkldnn._is_mkldnn_fp16_supported() and torch.ops.mkldnn._is_mkldnn_bf16_supported(), "needs native bf16 and fp16 on this CPU"
    _, model, x = _model_and_input()
    out = {}
    with torch.no_grad():
        out["f32"] = model(x).last_hidden_state.numpy()
        for dtype, name in KEY.items():
            with torch.autocast("cpu", dtype=dtype):
                out[name] = model(x).last_hidden_state.float().numpy()
    np.savez_compressed(GOLDEN, **out)


if __name__ == "__main__":
    if sys.argv[1:2] == ["emulate"]:
        emulate(sys.argv[2], sys.argv[3])
    elif sys.argv[1:] == ["capture"]:
        capture()
    else:
        raise SystemExit("usage: test_oracle_autocast.py capture | emulate {bf16,f16} OUT.npz")
