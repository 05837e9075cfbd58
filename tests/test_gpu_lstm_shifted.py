"""dW_hh of the bidirectional LSTM from shifted output rows (`-m gpu`): with the slab scratch, stair_lstm_bidir_bwd forms
dW_hh = dG^T Hprev by reading `out` one row before / behind each gate-gradient row under a 0 / 1 mask instead of copying h(t-1)
into hprev_ws (csrc/lstm.hip launch_lstm_bwd_weights, csrc/gemm_tn_x3tr.hip SHIFT).  The rows around `out` and all of hprev_ws are
NaN before the call: a masked row must count as an exact zero whatever it holds, and nothing outside `out` may be needed.  dw_hh
and both bias gradients are compared with an fp64 host product on explicitly shifted rows, to the tolerance
tests/test_gpu_lstm_coop.py uses for the same tensors."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
Hh = 256


def _weights(I, seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / np.sqrt(Hh)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * k).to(DEV)
    return [t for _ in range(2) for t in (u(4 * Hh, I), u(4 * Hh, Hh), u(4 * Hh), u(4 * Hh))]


@pytest.mark.parametrize('layout,n,lo,hi', [('ragged', 2100, 1, 8), ('padded', 300, 2, 10), ('uniform', 64, 64, 64), ('uniform', 37, 64, 64)])
def test_dw_hh_from_shifted_rows_matches_fp64_host_product(layout, n, lo, hi):
    from stair_amd import ops
    assert ops.get_matmul_mode() == 'bf16x3'
    I = 64
    g = torch.Generator().manual_seed(1000 + n)
    lens = torch.randint(lo, hi + 1, (n,), generator=g).tolist()
    if layout == 'padded':
        off = np.arange(n + 1) * hi
        seq_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    else:
        off = np.concatenate([[0], np.cumsum(lens)])
        seq_len = None
    rows = int(off[-1])
    assert rows >= 2048                                     # the slab kernel's range: below it the copy stays
    seq_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    x = torch.randn(rows, I, generator=g).to(DEV)
    d_out = torch.randn(rows, 2 * Hh, generator=g).to(DEV)
    d_hn = torch.randn(n, 2 * Hh, generator=g).to(DEV)
    ws = _weights(I, n)
    out, h_n, gates, cbuf = ops.lstm_bidir(x, seq_off, hi, ws, save=True, seq_len=seq_len)

    pad = 3
    around = torch.full((rows + 2 * pad, 2 * Hh), float('nan'), device=DEV)
    around[pad: pad + rows] = out
    out_in = around[pad: pad + rows]                        # `out` with NaN rows before its first and behind its last row
    hprev = torch.full((rows, 2 * Hh), float('nan'), device=DEV)
    grads = ops.lstm_bidir_bwd(x, seq_off, hi, ws, out_in, gates, cbuf, d_out, d_hn, seq_len=seq_len, slabs=True, hprev=hprev)
    torch.cuda.synchronize()
    # the copy was not made: apart from the two masks and the < 32 rows past the last whole stage, hprev_ws is untouched
    assert bool(hprev.view(-1)[2 * rows: (rows & ~31) * 2 * Hh].isnan().all())
    assert torch.equal(around[:pad].isnan(), torch.ones_like(around[:pad], dtype=torch.bool))

    dG = gates.double().cpu()                               # gate pre-activation gradients, written in place: [rows, 2 x 4Hh]
    o = out.double().cpu()
    hp = torch.zeros(2, rows, Hh, dtype=torch.float64)      # h of the previous step of each direction, explicitly shifted
    for s in range(n):
        b, L = int(off[s]), lens[s]
        hp[0, b + 1: b + L] = o[b: b + L - 1, :Hh]
        hp[1, b: b + L - 1] = o[b + 1: b + L, Hh:]
        if layout == 'padded':
            assert float(dG[b + L: int(off[s + 1])].abs().max() if L < hi else 0.0) == 0.0     # rows past the length: cleared
    for d in range(2):
        dg = dG[:, d * 4 * Hh: (d + 1) * 4 * Hh]
        ref_w = dg.t() @ hp[d]
        ref_b = dg.sum(0)
        for name, got, ref in (('dw_hh', grads[4 * d + 1], ref_w), ('db_ih', grads[4 * d + 2], ref_b), ('db_hh', grads[4 * d + 3], ref_b)):
            got = got.double().cpu()
            assert int(got.isnan().sum()) == 0, (name, d)
            scale = max(1.0, float(ref.abs().max()))
            err = float((got - ref).abs().max())
            print('%s dir %d (%s, %d rows): max error %.3g, bound %.3g' % (name, d, layout, rows, err, 1e-4 * scale))
            assert err < 1e-4 * scale, (name, d, err, scale)
