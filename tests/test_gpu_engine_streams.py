"""GPU: the engines' side-stream fan-out and saturation guard (ucod_dpl_amd/vit_engine.py: _BackboneEngine._fan_out, _SaturationGuard).

An image's key map does not depend on which stream computes it: a pass fanned out over side streams equals, bit for bit, the same chunks run one after the other on
one stream.  The comparison is chunk for chunk, never against the whole-batch pass: a chunk may take another tile and statistics path than the full batch
(tests/test_gpu_lnfold.py allows 1e-3 there).  The shape -- D = 256, 4 heads, 3 layers, patch 14, 70 x 70 images (26 token rows each), batch 3 -- is the smallest that
has the LayerNorm fold, an uneven chunk split (1 + 2) and a truncated pass."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from ucod_dpl_amd.vit_engine import ViTEngine, ViTLoRAEngine  # noqa: E402
from ucod_dpl_amd.data.utils.feature_extractor import random_state_dict, ARCHS  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def small():
    ARCHS["streams_vit"] = (256, 4, 3, 14, 70, True)
    sd = random_state_dict("streams_vit", seed=4)
    g = torch.Generator().manual_seed(8)
    for k in sd:                                                # LayerNorm parameters away from (1, 0): the fold has something to carry
        if "norm" in k and k.endswith("weight"):
            sd[k] = 1 + 0.3 * torch.randn(sd[k].shape, generator=g)
        if "norm" in k and k.endswith("bias"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
    img = torch.randn(3, 3, 70, 70, generator=torch.Generator().manual_seed(9)).to(DEV)
    return sd, img


@pytest.mark.parametrize("n_layers", [None, 2])
def test_two_streams_equal_the_chunks_run_one_by_one(small, n_layers):
    sd, img = small
    eng = ViTEngine(sd, heads=4, device=DEV)
    assert eng.ln_fold and eng.streams == 1
    chunks = torch.cat((eng.forward(img[:1], n_layers=n_layers), eng.forward(img[1:3], n_layers=n_layers)))
    eng.streams = 2                                             # chunks of 1 and 2 images, each on its own side stream
    both = eng.forward(img, n_layers=n_layers)
    key, events = eng.forward_async(img)
    for e in events:
        torch.cuda.current_stream().wait_event(e)
    eng.check_overflow(wait=True)
    assert len(events) == 2 and tuple(both.shape) == (3, 256, 5, 5) and bool(torch.isfinite(both).all())
    assert torch.equal(both, chunks)
    if n_layers is None:
        assert torch.equal(key, chunks)


def lora_engine(sd, **kw):
    eng = ViTLoRAEngine(sd, heads=4, device=DEV, generator=torch.Generator().manual_seed(3), **kw)
    lsd = eng.lora_state_dict()
    g = torch.Generator().manual_seed(5)
    for k in lsd:
        if "lora_B" in k:                                       # lora_B starts at zero: give the LoRA branch something to add
            lsd[k] = 0.05 * torch.randn(lsd[k].shape, generator=g)
    eng.load_lora_state_dict(lsd)
    assert all(float(v.abs().max()) > 0.0 for k, v in eng.lora_state_dict().items() if "lora_B" in k)
    return eng


def test_lora_engine_two_train_streams_equal_the_chunks_run_one_by_one(small):
    sd, img = small
    one, two = lora_engine(sd), lora_engine(sd)
    assert two.train_streams == 2 and torch.equal(one.lora, two.lora)
    one.train_streams = 1
    for fwd in ("forward_train", "forward_nograd"):
        chunks = torch.cat((getattr(one, fwd)(img[:1]), getattr(one, fwd)(img[1:3])))
        both = getattr(two, fwd)(img)
        one.check_overflow(wait=True)
        two.check_overflow(wait=True)
        assert bool(torch.isfinite(both).all()) and torch.equal(both, chunks), fwd


def test_a_clone_for_ema_reports_its_own_saturation(small):
    """The clone made AFTER the student has run (and reported) a saturating pass holds a guard of its own: a saturating no-grad pass of the clone raises from the
    clone's check_overflow(wait=True), never from the student's.  The saturating model is that of test_gpu_parity_c2.py (the position embedding puts 1e5 into two
    channels of the CLS token and of a few patch tokens: beyond fp16's 65504 from the first layer on) at this file's shape."""
    _, img = small
    ARCHS["streams_massive_vit"] = (256, 4, 3, 14, 70, True)
    sd = random_state_dict("streams_massive_vit", seed=3)
    pos = sd["embeddings.position_embeddings"]
    for t in (0, 5, 17, 25):
        pos[0, t, 5] = 1.0e5
        pos[0, t, 200] = -0.75e5
    student = ViTLoRAEngine(sd, heads=4, device=DEV)
    assert student.resid16
    key = student.forward_nograd(img)
    assert bool(torch.isfinite(key).all())
    with pytest.raises(FloatingPointError):
        student.check_overflow(wait=True)                       # handed out once, and cleared
    student.check_overflow(wait=True)
    clone = student.clone_for_ema()
    assert clone._guard is not student._guard
    clone.forward_nograd(img)
    student.check_overflow(wait=True)                           # not the student's pass: no FloatingPointError
    student.forward_nograd(img, resid16=False)                  # (nor from the non-blocking poll inside a pass of the student's on the f32 stream)
    student.check_overflow(wait=True)
    with pytest.raises(FloatingPointError):
        clone.check_overflow(wait=True)
    clone.check_overflow(wait=True)
