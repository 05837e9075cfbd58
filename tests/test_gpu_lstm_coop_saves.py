"""Training saves of the cooperative forward recurrence (csrc/lstm_coop.hip, lstm_rec_coop_kernel<true, NT>): the activated
gates that replace a row's xproj and the cell state in cbuf are not stored by the cell update that computes them but later in
the same loop iteration, behind the fetch of the next tile's slab (the gates wait in LDS, c in its registers, the row and the
predicate of the store in two more).  A store that went out with a stale row or predicate would land in another step's row or
behind a sequence's end, so the tests compare EVERY saved value with an fp64 explicit recurrence (stair_lstm_bidir_fwd through
the C ABI, Hh = 256, the tolerance tests/test_gpu_lstm_coop.py holds `out` to) and look at every row the kernel must not touch:

  * n = 33, lengths 1..5 (one tile per group; the second group's tile holds ONE live sequence, the first one sequences that end
    after a single step while their neighbours go on);
  * n = 1025, lengths 1..4, the launch capped to 32 workgroups (stair_lstm_coop_limit, as tests/test_gpu_lstm_coop.py caps it):
    two tiles per group, four groups per direction, each of which walks 4 or 5 of the 17 chunks; the last chunk has one sequence
    in tile A and an empty tile B;
  * both with padded storage: cbuf is filled with a sentinel before the launch and the rows behind a sequence's end must still
    hold it; the same rows of the xproj buffer are written by the input projection (every row of the storage), so they must hold
    what the inference launch -- which stores nothing into xproj -- leaves there, bit for bit;
  * the training launch's `out` and `h_n` equal the inference launch's bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
Hh = 256
I = 64
TOL = 2e-5                # tests/test_gpu_lstm_coop.py: out, gates and cbuf of the cooperative kernel
SENTINEL = -12345.0

CASES = {'one_tile': dict(n=33, hi=5, cap=-1), 'two_tiles_chunks': dict(n=1025, hi=4, cap=32)}


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / np.sqrt(Hh)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k
    return [t for _ in range(2) for t in (u(4 * Hh, I), u(4 * Hh, Hh), u(4 * Hh), u(4 * Hh))]


def _reference(x, lens, off, ws):
    """nn.LSTM's recurrence written out in fp64 on the host: out, h_n, the four activated gates [rows, dir, gate, Hh] and c."""
    n, rows = len(lens), x.shape[0]
    x = x.double()
    out = torch.zeros(rows, 2 * Hh, dtype=torch.float64)
    gates = torch.zeros(rows, 8 * Hh, dtype=torch.float64)
    cbuf = torch.zeros(rows, 2 * Hh, dtype=torch.float64)
    h_n = torch.zeros(n, 2 * Hh, dtype=torch.float64)
    lens_t, off_t = torch.tensor(lens), torch.tensor(off[:-1])
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = (w.double() for w in ws[4 * d: 4 * d + 4])
        pre = x @ w_ih.t() + b_ih + b_hh
        h = torch.zeros(n, Hh, dtype=torch.float64)
        c = torch.zeros(n, Hh, dtype=torch.float64)
        for t in range(max(lens)):
            live = torch.nonzero(lens_t > t).squeeze(1)
            r = off_t[live] + (t if d == 0 else lens_t[live] - 1 - t)
            a = pre[r] + h[live] @ w_hh.t()
            i, f, g, o = torch.sigmoid(a[:, :Hh]), torch.sigmoid(a[:, Hh: 2 * Hh]), torch.tanh(a[:, 2 * Hh: 3 * Hh]), torch.sigmoid(a[:, 3 * Hh:])
            c[live] = f * c[live] + i * g
            h[live] = o * torch.tanh(c[live])
            out[r, d * Hh: (d + 1) * Hh] = h[live]
            gates[r, d * 4 * Hh: (d + 1) * 4 * Hh] = torch.cat([i, f, g, o], 1)
            cbuf[r, d * Hh: (d + 1) * Hh] = c[live]
        h_n[:, d * Hh: (d + 1) * Hh] = h
    return dict(out=out, h_n=h_n, gates=gates, cbuf=cbuf)


@functools.lru_cache(maxsize=None)
def _case(name, padded):
    """Inputs (host), the fp64 reference and the row masks of one case; built once, never modified."""
    n, hi = CASES[name]['n'], CASES[name]['hi']
    g = torch.Generator().manual_seed(7 + n + int(padded))
    lens = torch.randint(1, hi + 1, (n,), generator=g).tolist()
    lens[0], lens[3], lens[n - 1] = 1, 1, hi          # sequences that end after one step; the lone sequence of the last tile runs longest
    off = (np.arange(n + 1) * hi) if padded else np.concatenate([[0], np.cumsum(lens)])
    rows = int(off[-1])
    x = torch.randn(rows, I, generator=g)
    ws = _weights(n)
    data = torch.zeros(rows, dtype=torch.bool)
    for s in range(n):
        data[int(off[s]): int(off[s]) + lens[s]] = True
    return dict(lens=lens, off=off, x=x, ws=ws, data=data, hi=hi, ref=_reference(x, lens, off, ws))


def _forward(case, padded, train, cap):
    """stair_lstm_bidir_fwd as ops.lstm_bidir calls it, with buffers the test owns: cbuf and xproj start as SENTINEL."""
    from stair_amd import ops
    from stair_amd._lib import LstmArgs, check, lib
    assert ops.get_matmul_mode() == 'bf16x3'
    x = case['x'].to(DEV)
    ws = [w.to(DEV) for w in case['ws']]
    rows, n = x.shape[0], len(case['lens'])
    seq_off = torch.tensor(case['off'], dtype=torch.int32, device=DEV)
    seq_len = torch.tensor(case['lens'], dtype=torch.int32, device=DEV) if padded else None
    out = torch.empty(rows, 2 * Hh, device=DEV)
    h_n = torch.empty(n, 2 * Hh, device=DEV)
    xproj = torch.full((rows, 8 * Hh), SENTINEL, device=DEV)
    cbuf = torch.full((rows, 2 * Hh), SENTINEL, device=DEV) if train else None
    bias_ws = torch.empty(8 * Hh, device=DEV)
    pack_ws = torch.empty(8 * Hh * Hh, device=DEV)
    coop_ws = torch.empty(int(lib.stair_lstm_coop_ws_bytes(n)), device=DEV, dtype=torch.uint8)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = LstmArgs()
    a.x, a.ldx, a.rows, a.n, a.max_len, a.I, a.Hh = x.data_ptr(), I, rows, n, case['hi'], I, Hh
    a.seq_off = seq_off.data_ptr()
    if padded:
        a.seq_len = seq_len.data_ptr()
    a.coop_ws, a.coop_ws_bytes, a.status = coop_ws.data_ptr(), coop_ws.numel(), status.data_ptr()
    for d in range(2):
        a.w_ih[d], a.w_hh[d] = ws[4 * d].data_ptr(), ws[4 * d + 1].data_ptr()
        a.b_ih[d], a.b_hh[d] = ws[4 * d + 2].data_ptr(), ws[4 * d + 3].data_ptr()
    a.xproj_ws, a.bias_ws, a.whh_pack_ws = xproj.data_ptr(), bias_ws.data_ptr(), pack_ws.data_ptr()
    a.out, a.ldo, a.h_n = out.data_ptr(), 2 * Hh, h_n.data_ptr()
    a.cbuf = cbuf.data_ptr() if train else None
    try:
        lib.stair_lstm_coop_limit(cap)
        with ops.kernel_accounting() as acct:
            check(lib.stair_lstm_bidir_fwd(C.byref(a), ops._stream()))
        torch.cuda.synchronize()
    finally:
        lib.stair_lstm_coop_limit(-1)
    assert 'lstm_rec_coop' in acct.table, sorted(acct.table)          # the cooperative kernel is what ran
    assert int(status.item()) == 0                                     # no hand-off timed out
    return dict(out=out.cpu(), h_n=h_n.cpu(), gates=xproj.cpu(), cbuf=cbuf.cpu() if train else None)


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('name', sorted(CASES))
def test_saved_gates_and_cells_match_fp64_recurrence_and_nothing_else_is_written(name, padded):
    case = _case(name, padded)
    got = _forward(case, padded, train=True, cap=CASES[name]['cap'])
    data, ref = case['data'], case['ref']
    for k in ('out', 'gates', 'cbuf'):
        err = float((got[k][data].double() - ref[k][data]).abs().max())
        print('%s %s padded=%s: max |%s - fp64| = %.3g (bound %.3g)' % (name, case['x'].shape, padded, k, err, TOL))
        assert err < TOL, (k, err)
    err = float((got['h_n'].double() - ref['h_n']).abs().max())
    print('%s padded=%s: max |h_n - fp64| = %.3g (bound %.3g)' % (name, padded, err, TOL))
    assert err < TOL, ('h_n', err)
    if padded:
        tail = ~data
        assert int(tail.sum()) > 0
        assert bool((got['cbuf'][tail] == SENTINEL).all())            # no cell state behind a sequence's end
        assert float(got['out'][tail].abs().max()) == 0.0             # rows past a length read as zero downstream
        plain = _forward(case, padded, train=False, cap=CASES[name]['cap'])
        assert bool((plain['gates'] != SENTINEL).all())               # the input projection writes every row of the storage
        assert torch.equal(got['gates'][tail], plain['gates'][tail])  # ... and no activated gate replaced one of those


def test_training_launch_leaves_out_and_h_n_of_the_inference_launch():
    case = _case('one_tile', False)
    train = _forward(case, False, train=True, cap=-1)
    infer = _forward(case, False, train=False, cap=-1)
    assert torch.equal(train['out'], infer['out'])
    assert torch.equal(train['h_n'], infer['h_n'])
