"""GPU tests of the 128 (n) x 512 (k) tile of the transposed-read weight-gradient kernel (csrc/gemm_tn_tr.hip): dW += dG^T X with X
stored as bf16 rows (dW_ih of the video encoder).  Conventions of tests/test_gpu_tn_slabs.py: inputs from a seeded generator, the
reference is the fp64 product of the same operands on the CPU, the bound is that file's for the split products (the arithmetic is
the same: dG hi * X + dG lo * X, fp32 accumulate), and a product whose slabs are stored and added in slab order gives the same bits
twice.  (The wide form of the slab kernel that was to be tested here as well was not kept: DESIGN.md section 3.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _tr_case(M, N, K, lda, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=g).to(torch.bfloat16)
    full = torch.randn(M, lda, generator=g)
    C0 = torch.randn(N, K, generator=g)
    return X, full, C0


def _launches(table, key):
    return table[key][0] if key in table else 0


# (2048, 128, 512): one tile, 8 slabs of 8 stages; (4096, 1024, 2048): 8 x 4 tiles, every wave's k quarter in another half image
# of X, dG a column block of a wider matrix as one direction's gate gradients are
@pytest.mark.parametrize('M,N,K,lda', [(2048, 128, 512, 128), (4096, 1024, 2048, 2048), (2048, 384, 1024, 384)])
def test_transposed_read_product_matches_fp64(M, N, K, lda):
    from stair_amd import ops
    X, full, C0 = _tr_case(M, N, K, lda, M + N + K)
    Xd, fd = X.to(DEV), full.to(DEV)
    dZ = fd[:, lda - N:]
    Cm = C0.to(DEV)
    with ops.kernel_accounting() as acct:
        ops.gemm_tn(dZ, Xd, Cm, M, N, K, rows_per_group=1, lda=lda)
    assert _launches(acct.table, 'gemm_tn_tr') == 1, sorted(acct.table)
    ref = C0.double() + full[:, lda - N:].double().t() @ X.double()
    tol = 4e-4 * max(1.0, (M / 1000) ** 0.5 * 3)
    err = float((Cm.cpu().double() - ref).abs().max())
    print('M %d N %d K %d: max error %.3g (bound %.3g)' % (M, N, K, err, tol))
    assert err < tol


def test_stored_slabs_of_the_video_encoder_product_give_the_same_bits_twice():
    """stair_lstm_bidir_bwd with slabs: dW_ih of both directions (M = 32 x 64, N = 4 Hh = 1024, K = 512, dG the direction's column
    block of the gate gradients) takes this kernel with its eight slabs stored and added in slab order: no atomics."""
    from stair_amd import ops
    n, L, I, Hh = 32, 64, 512, 256
    g = torch.Generator().manual_seed(77)
    seq_off = torch.arange(n + 1, dtype=torch.int32, device=DEV) * L
    x = torch.randn(n * L, I, generator=g).to(torch.bfloat16).to(DEV)
    d_out = torch.randn(n * L, 2 * Hh, generator=g).to(DEV)
    d_hn = torch.randn(n, 2 * Hh, generator=g).to(DEV)
    ws = []
    for _ in range(2):
        ws += [(torch.randn(4 * Hh, I, generator=g) * 0.05).to(DEV), (torch.randn(4 * Hh, Hh, generator=g) * 0.05).to(DEV),
               (torch.randn(4 * Hh, generator=g) * 0.05).to(DEV), (torch.randn(4 * Hh, generator=g) * 0.05).to(DEV)]
    out, h_n, gates0, cbuf = ops.lstm_bidir(x, seq_off, L, ws, save=True)
    runs = []
    for _ in range(2):
        with ops.kernel_accounting() as acct:
            grads = ops.lstm_bidir_bwd(x, seq_off, L, ws, out, gates0.clone(), cbuf, d_out, d_hn, slabs=True)
        assert _launches(acct.table, 'gemm_tn_tr') == 2, sorted(acct.table)
        assert _launches(acct.table, 'gemm_tn_x3tr') >= 2, sorted(acct.table)       # dW_hh (K = Hh = 256, shifted rows): the slab kernel as before
        runs.append([t.cpu() for t in grads])
    assert all(float(t.abs().max()) > 0 for t in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))


@pytest.mark.parametrize('M,N,K', [(2048, 256, 256), (2048, 192, 512)])
def test_shapes_off_the_tile_take_the_register_transposing_kernel(M, N, K):
    """K % 512 != 0 (a 256-column input) or N % 128 != 0: not this kernel's; the product is still right"""
    from stair_amd import ops
    X, full, C0 = _tr_case(M, N, K, N, M + N + K + 1)
    Cm = C0.to(DEV)
    with ops.kernel_accounting() as acct:
        ops.gemm_tn(full.to(DEV), X.to(DEV), Cm, M, N, K, rows_per_group=1)
    assert 'gemm_tn_tr' not in acct.table and any(k.startswith('gemm_tn_bf16x3') for k in acct.table), sorted(acct.table)
    ref = C0.double() + full.double().t() @ X.double()
    assert float((Cm.cpu().double() - ref).abs().max()) < 4e-4 * max(1.0, (M / 1000) ** 0.5 * 3)
