"""GPU: ucod_wgrad_bf16_det (csrc/wgrad.hip) at every dispatch case, at the smallest sizes where each exists: exact-arithmetic cases bit for bit, random
cases within the bound derived in tests/refiner_wgrad_ref.py against f64, two runs bit-identical, guard rows around dW and the workspace untouched, and every
UCOD_EINVAL condition refused with nothing written."""
import pytest
import torch

import refiner_wgrad_ref as W

pytestmark = pytest.mark.gpu

SHAPES = ((64, 64), (128, 192), (256, 128), (768, 768))
SENTINEL = -12345.5


def _boundary_M():
    """a row count of the 768 x 768 shape whose chunks are two slabs long and all full: one row less leaves the last chunk ragged, one row more moves the chunk size"""
    n, _ = W.nsplit_rule(1 << 20, 768, 768)
    return n * 2 * W.SLAB


MB = _boundary_M()
# (M, N, K, accumulate, wide)
CASES = [(M, N, K, False, False) for (N, K) in SHAPES for M in (1, 63, 64, 65)] + [
    (MB - 1, 768, 768, False, False), (MB, 768, 768, True, False), (MB + 1, 768, 768, False, False),      # below, at, above a chunk boundary
    (300, 256, 128, True, False),                                                                          # ragged last chunk, nsplit 5
    (200, 128, 192, False, True), (200, 128, 192, True, True), (40, 128, 192, True, True),                 # ld_dy > N (the V half), ld_x > K, ld_dw > K
    (130, 64, 64, True, False),
]


@pytest.fixture(scope="module")
def lib():
    from ucod_dpl_amd import native
    return native.load()


def test_case_list_reaches_every_dispatch_case(lib):
    ns = {c: lib.ucod_wgrad_bf16_det_nsplit(*c[:3]) for c in CASES}
    for c, n in ns.items():
        assert n == W.nsplit_rule(*c[:3])[0], c
        assert lib.ucod_wgrad_bf16_det_workspace_bytes(*c[:3]) == (0 if n == 1 else n * c[1] * c[2] * 4)
    assert any(n == 1 for n in ns.values()) and any(n >= 3 for n in ns.values()) and any(n == 2 for n in ns.values())
    chunk, ranges = W.chunking(MB, ns[(MB, 768, 768, True, False)])
    assert chunk == 2 * W.SLAB and ranges[-1][1] - ranges[-1][0] == chunk                                 # all chunks full at the boundary
    _, below = W.chunking(MB - 1, ns[(MB - 1, 768, 768, False, False)])
    assert below[-1][1] - below[-1][0] == chunk - 1
    chunk_above, above = W.chunking(MB + 1, ns[(MB + 1, 768, 768, False, False)])
    assert chunk_above > chunk and 0 < above[-1][1] - above[-1][0] < chunk_above                           # ragged
    assert lib.ucod_wgrad_bf16_det_nsplit(56448, 768, 768) * 36 in range(240, 513) and lib.ucod_wgrad_bf16_det_nsplit(56448, 3072, 768) in (1, 2)
    assert lib.ucod_wgrad_bf16_det_nsplit(56448, 768, 3072) in (1, 2)


def _run(case, lib, pad_k):
    """-> (dW [N, K] view, the whole guarded dW buffer, the guarded workspace or None, the workspace's byte count)"""
    from ucod_dpl_amd import ops
    M, N, K = case["M"], case["N"], case["K"]
    dyb, xb = case["dy_buf"].cuda(), case["x_buf"].cuda()
    dy, x = dyb[:M, case["col"]:case["col"] + N], xb[:M, :K]
    big = torch.full((N + 2, K + pad_k), SENTINEL, dtype=torch.float32, device="cuda")
    out = big[1:1 + N, :K]
    out.copy_(case["base"].cuda())
    nbytes = lib.ucod_wgrad_bf16_det_workspace_bytes(M, N, K)
    wsg = None
    if nbytes:
        wsg = torch.full((nbytes // 4 + 128,), SENTINEL, dtype=torch.float32, device="cuda")
        ws = wsg[64:64 + nbytes // 4].view(torch.uint8)
    ops.weight_grad_direct(dy, x, out=out, accumulate=case["accumulate"], ws=ws if nbytes else None)
    torch.cuda.synchronize()
    return out, big, wsg, nbytes


@pytest.mark.parametrize("kind", ("exact", "random"))
@pytest.mark.parametrize("M,N,K,accumulate,wide", CASES)
def test_wgrad_direct(lib, M, N, K, accumulate, wide, kind):
    case = W.make_case(M, N, K, kind, accumulate, wide)
    nsplit = lib.ucod_wgrad_bf16_det_nsplit(M, N, K)
    pad_k = 8 if wide else 0
    out, big, wsg, nbytes = _run(case, lib, pad_k)
    got = out.cpu().clone()
    msg = W.check(case, got, nsplit)
    print(f"wgrad {kind} M={M} N={N} K={K} nsplit={nsplit} acc={accumulate} wide={wide}: {msg or 'ok'}")
    assert msg is None, msg
    # guards: the rows above and below dW, the columns K .. ld_dw-1 of its own rows, the floats on both sides of the workspace
    assert bool((big[0] == SENTINEL).all()) and bool((big[-1] == SENTINEL).all()) and bool((big[1:-1, K:] == SENTINEL).all())
    if wsg is not None:
        assert bool((wsg[:64] == SENTINEL).all()) and bool((wsg[64 + nbytes // 4:] == SENTINEL).all())
    out2, _, _, _ = _run(case, lib, pad_k)
    assert torch.equal(out2.cpu(), got), "two runs differ"


def test_default_output_and_workspace(lib):
    from ucod_dpl_amd import ops
    case = W.make_case(200, 128, 192, "exact")
    got = ops.weight_grad_direct(case["dy"].cuda(), case["x"].cuda())
    assert got.dtype == torch.float32 and W.check(case, got, lib.ucod_wgrad_bf16_det_nsplit(200, 128, 192)) is None


def test_einval_conditions_write_nothing(lib):
    from ucod_dpl_amd import native as N
    M, Nn, K = 200, 128, 192
    dy = torch.ones(M, Nn + 8, dtype=torch.bfloat16, device="cuda")
    x = torch.ones(M, K + 8, dtype=torch.bfloat16, device="cuda")
    dw = torch.full((Nn, K + 8), SENTINEL, dtype=torch.float32, device="cuda")
    nbytes = lib.ucod_wgrad_bf16_det_workspace_bytes(M, Nn, K)
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), SENTINEL, dtype=torch.float32, device="cuda")
    st = N.stream()
    p = lambda t: t.data_ptr()                                                     # noqa: E731
    good = dict(dy=p(dy), ld_dy=Nn + 8, x=p(x), ld_x=K + 8, dw=p(dw), ld_dw=K + 8, M=M, N=Nn, K=K, ws=p(ws), ws_bytes=nbytes)
    bad = [dict(dy=None), dict(x=None), dict(dw=None), dict(ws=None), dict(M=0), dict(M=-1), dict(N=Nn - 32), dict(K=K + 32), dict(N=0), dict(K=0),
           dict(ld_dy=Nn - 4), dict(ld_x=K - 4), dict(ld_dw=K - 4), dict(ld_dy=Nn + 2), dict(ld_x=K + 6), dict(dy=p(dy) + 4), dict(x=p(x) + 2),
           dict(ws_bytes=nbytes - 4), dict(ws_bytes=0)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.ucod_wgrad_bf16_det(a["dy"], a["ld_dy"], a["x"], a["ld_x"], a["dw"], a["ld_dw"], a["M"], a["N"], a["K"], 0, a["ws"], a["ws_bytes"], st)
        assert rc == -1, change
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all()) and bool((ws == SENTINEL).all())
    assert lib.ucod_wgrad_bf16_det_nsplit(M, Nn - 32, K) == 0 and lib.ucod_wgrad_bf16_det_workspace_bytes(0, Nn, K) == 0
    a = good                                                                       # and the good call goes through
    assert lib.ucod_wgrad_bf16_det(a["dy"], a["ld_dy"], a["x"], a["ld_x"], a["dw"], a["ld_dw"], M, Nn, K, 0, a["ws"], nbytes, st) == 0
    torch.cuda.synchronize()
    assert bool((dw[:, :K] == M).all()) and bool((dw[:, K:] == SENTINEL).all())
