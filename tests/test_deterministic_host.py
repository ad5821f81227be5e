"""CPU: the host side of the deterministic training step -- the `_det` entry points are declared, bound and exported with matching arity, the ABI number
stands, the summation-order contract is in the header, and the switch (train_cfg.deterministic / set_random_seed(seed, deterministic=...)) reaches TrainLoop."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

DET_ENTRY_POINTS = ("ucod_dba_wgrad_det", "ucod_conv_wgrad_f32_det", "ucod_dba_heads_fwd_det", "ucod_dba_bwd_det", "ucod_apm_bce_det", "ucod_disc_fwd_det",
                    "ucod_disc_bwd_det")


def header_text():
    return open(os.path.join(ROOT, "include", "ucod_dpl.h")).read()


def declarations():
    """{name: number of parameters} of every function the header declares (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(ucod_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else len(args.split(","))
    return out


def g18_cfg(**train_extra):
    """tests/test_gpu_train_step.py::_g18_cfg (that module needs a GPU to import)"""
    from ucod_dpl_amd.engine.config import CfgNode
    return CfgNode(dict(
        model_cfg=dict(dim=128, feature_size=12, ema_weight=0.99, dis_use_features=False),
        train_cfg=dict(max_epoch=6, start_epoch=0, start_finetune=-2, lr0=6e-4, dis_lr0=1e-3, step_lr_size=2, dis_step_lr_size=2, step_lr_gamma=0.95,
                       dis_step_lr_gamma=0.95, merge_alpha=0.5, merge_method="dis", dist_train=False, dis_epoch=1, dis_intertrain=2,
                       save_cfg=dict(save_mode="model", save_interval=5, start_save=1000), **train_extra),
        val_cfg=dict(enable_val=False, val_interval=5, start_val=1000),
        log_cfg=dict(log_interval=50, log_path="/tmp/ucod_g18", multi_rank=[0]),
    ))


def test_header_declares_every_det_symbol_and_its_workspace_helper():
    from ucod_dpl_amd import native
    decl = declarations()
    for name in DET_ENTRY_POINTS:
        for n in (name, name + "_workspace_bytes"):
            assert n in decl, n
            assert n in native.SIGNATURES, n
            res, args = native.SIGNATURES[n]
            assert len(args) == decl[n], (n, len(args), decl[n])
        assert native.SIGNATURES[name][0] is native.ci and native.SIGNATURES[name + "_workspace_bytes"][0] is native.sz
        # the explicit workspace: a pointer, then its size, in front of the trailing shape / stream arguments
        args = native.SIGNATURES[name][1]
        assert any(a is native.vp and b is native.sz for a, b in zip(args, args[1:])), name


def test_det_symbols_are_exported_and_refuse_bad_arguments_before_any_launch():
    from ucod_dpl_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = native.load()
    raw = ctypes.CDLL(native.LIB_PATH)
    for name in DET_ENTRY_POINTS:
        assert hasattr(raw, name) and hasattr(raw, name + "_workspace_bytes"), name
    # size helpers: 0 for an invalid shape, the documented layouts otherwise (no device needed)
    assert lib.ucod_dba_wgrad_det_workspace_bytes(0, 768, 1369, 0) == 0 and lib.ucod_dba_wgrad_det_workspace_bytes(2, 768, -1, 1) == 0
    for exact in (0, 1):
        nb = lib.ucod_dba_wgrad_det_workspace_bytes(32, 768, 1369, exact)
        assert nb > 0 and nb % (128 * 768 * 4) == 0 and (nb // (128 * 768 * 4)) % 32 == 0            # Q = B * nchunk planes of [128][C] f32
    assert lib.ucod_conv_wgrad_f32_det_workspace_bytes(2, 144, 36, 200) % (200 * 144 * 4) == 0 and lib.ucod_conv_wgrad_f32_det_workspace_bytes(2, 144, 36, 0) == 0
    assert lib.ucod_dba_heads_fwd_det_workspace_bytes(3, 1369) == 3 * 6 * 4 and lib.ucod_dba_heads_fwd_det_workspace_bytes(3, 0) == 0
    assert lib.ucod_dba_bwd_det_workspace_bytes(2, 100) == lib.ucod_dba_bwd_workspace_bytes(2, 100) + 2 * 258 * 4
    assert lib.ucod_dba_bwd_det_workspace_bytes(0, 100) == 0
    assert lib.ucod_apm_bce_det_workspace_bytes(5) == 5 * 3 * 4 and lib.ucod_apm_bce_det_workspace_bytes(0) == 0
    assert lib.ucod_disc_fwd_det_workspace_bytes(3, 12) == (2 * 64 + 1 * 32 + 1 * 16) * 8 and lib.ucod_disc_fwd_det_workspace_bytes(3, 3) == 0
    assert lib.ucod_disc_bwd_det_workspace_bytes(3, 12) == lib.ucod_disc_bwd_workspace_bytes(3, 12) + (3 * 8 * 9 + 3) * 4
    assert lib.ucod_disc_bwd_det_workspace_bytes(0, 12) == 0
    # null pointers: UCOD_EINVAL (-1) before anything is launched
    assert lib.ucod_dba_wgrad_det(None, None, None, 2, 48, 100, 0, None, 0, None) == -1
    assert lib.ucod_conv_wgrad_f32_det(None, None, None, 2, 48, 100, 20, 0, None, 0, None) == -1
    assert lib.ucod_dba_heads_fwd_det(None, 128, 0, None, None, None, None, None, None, None, None, 0, 2, 100, None) == -1
    assert lib.ucod_dba_bwd_det(None, 128, 0, None, None, None, None, None, None, 1.0, None, None, None, None, None, 0, 2, 100, None) == -1
    assert lib.ucod_apm_bce_det(None, None, None, None, None, None, 0.0, 1.0, None, None, None, None, None, None, 0, 2, 100, None) == -1
    assert lib.ucod_disc_fwd_det(None, None, None, None, 2, 12, 1, None, 0, None) == -1
    assert lib.ucod_disc_bwd_det(None, None, None, None, None, 0, None, 0, 2, 12, None) == -1


def test_abi_version_is_unchanged_and_the_header_states_the_order():
    text = header_text()
    assert re.search(r"^#define UCOD_ABI_VERSION 5$", text, flags=re.M)
    assert "(still 5) The deterministic training step" in text
    from ucod_dpl_amd import native
    assert native.ABI_VERSION == 5
    flat = " ".join(text.split())
    assert "q = b * nchunk + chunk" in flat and "ws[q][n][c]" in flat
    assert "ascending q" in flat and "(accumulate ? gW[n][c] : 0) + ws[0][n][c] + ws[1][n][c]" in flat


def test_train_loop_reads_the_build_only_key():
    from ucod_dpl_amd.engine.runner.loop_UCOD_DPL import TrainLoop
    assert TrainLoop(g18_cfg(), None).deterministic is False
    assert TrainLoop(g18_cfg(deterministic=True), None).deterministic is True
    assert TrainLoop(g18_cfg(deterministic=0), None).deterministic is False
    # no shipped config carries the key (tests/golden/g17_config_trees.json pins those trees)
    for dp, _, files in os.walk(os.path.join(ROOT, "configs")):
        for f in files:
            if f.endswith(".py"):
                assert "deterministic" not in open(os.path.join(dp, f)).read(), f


def test_set_random_seed_sets_the_default_only_when_asked():
    from ucod_dpl_amd.engine.utils import seed as S
    from ucod_dpl_amd.engine.runner.loop_UCOD_DPL import TrainLoop
    assert inspect.signature(S.set_random_seed).parameters["deterministic"].default is None
    try:
        assert S.set_random_seed(42) == 42 and S.deterministic_default() is False
        assert S.set_random_seed(7, deterministic=True) == 7 and S.deterministic_default() is True
        assert TrainLoop(g18_cfg(), None).deterministic is True                    # no key: the seed helper's default
        assert TrainLoop(g18_cfg(deterministic=False), None).deterministic is False   # the key wins
        assert S.set_random_seed(42) == 42 and S.deterministic_default() is True   # None leaves it alone
        assert S.set_random_seed(42, deterministic=False) == 42 and S.deterministic_default() is False
    finally:
        S.set_random_seed(42, deterministic=False)


@pytest.mark.parametrize("fn,extra", [("dba_wgrad", ()), ("dba_heads", ()), ("dba_bwd", ()), ("apm_bce", ()), ("disc_fwd", ()), ("disc_bwd", ())])
def test_ops_wrappers_default_to_the_atomic_forms(fn, extra):
    from ucod_dpl_amd import ops
    p = inspect.signature(getattr(ops, fn)).parameters
    assert p["deterministic"].default is False and p["ws"].default is None
    from ucod_dpl_amd.models.discriminator import Discriminator
    assert inspect.signature(Discriminator._conv_block_bwd).parameters["deterministic"].default is False
    assert inspect.signature(Discriminator.backward_features).parameters["deterministic"].default is False
