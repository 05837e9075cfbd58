"""Packed tiles of the fused tile operators (csrc/tile_mlp.hip, the PACK kernel forms; include/stair_hip.h stair_set_tile_pack): clips
of T <= 32 frames share a 64-row tile, P = 64 / T instances each.  Every case runs with packing on and off; the unpacked launch is
the reference, bit for bit, and the packed one is also compared with fp64 at the tolerance tests/test_gpu_building_blocks.py (or,
for the backward chains, tests/test_gpu_tile_fused.py) uses for the same operator.  `-m gpu`."""
import numpy as np
import pytest
import torch

from stair_amd import spec, synth
from stair_amd._lib import lib
from tile_helpers import (DEV, H, STORE_FIRST, _gen, _lin, d, i32, _perm, _close, _launch, _mlp_ref, _chain_ref, _fwd2, _tile_words,
                          _work_items)

pytestmark = pytest.mark.gpu
# (T, cnt): one tile / a full and a partial tile / three tiles / T no multiple of 8, 60 used rows / 63 used rows / P = 2 / unpacked
CASES = [(8, 1), (8, 9), (8, 17), (5, 13), (21, 4), (32, 3), (33, 3)]


@pytest.fixture(autouse=True)
def default_switch():
    yield
    lib.stair_set_tile_pack(-1)


def _both(run):
    """run() with packing on, then off: ({name: tensor} of each)"""
    out = {}
    for on in (1, 0):
        lib.stair_set_tile_pack(on)
        out[on] = {k: v.clone() for k, v in run().items()}
        torch.cuda.synchronize()
    lib.stair_set_tile_pack(-1)
    return out[1], out[0]


def _same(on, off, skip=()):
    for k in off:
        if k not in skip:
            assert torch.equal(on[k], off[k]), (k, float((on[k].double() - off[k].double()).abs().max()))


def _expected_bits(act, T, cnt, P):
    """save_bits of activation rows act [cnt, T, 512] (> 0) as a launch with P instances per tile writes them, and the mask of the
    bits that belong to rows that exist: word (tile, 64 w + c), byte j, bit e <-> row w + 8 j of the tile, column 8 c + e"""
    tiles = (cnt + P - 1) // P
    rows = torch.zeros(tiles * 64, H, dtype=torch.bool)
    exists = torch.zeros(tiles * 64, dtype=torch.bool)
    pos = (act > 0).reshape(cnt * T, H).cpu()
    for i in range(cnt):
        r0 = (i // P) * 64 + (i % P) * T
        rows[r0:r0 + T] = pos[i * T:(i + 1) * T]
        exists[r0:r0 + T] = True
    return _tile_words(rows.reshape(tiles, 64, H)), _tile_words(exists.reshape(tiles, 64, 1).expand(-1, -1, H))


# ---------------------------------------------------------------------------------------------
# forward operators
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,cnt', CASES)
def test_filter_shape(T, cnt):
    """2 layers + the sum over each instance's own frames (len < T included), saves and relu' bits"""
    from stair_amd import ops
    g = _gen(T, cnt, 1)
    n_src = cnt + 2
    x = torch.randn(n_src, T, H, generator=g)
    x_idx = torch.randint(0, n_src, (cnt,), generator=g, dtype=torch.int32)
    lens = [(T, max(1, T - 3), 1, max(1, T // 2))[i % 4] for i in range(cnt)]
    out_idx = _perm(cnt + 2, cnt, g)
    planes = [ops.pack_wfrag(d(_lin(i)[0])) for i in range(2)]
    xd, xi, oi, ln = d(x), d(x_idx), d(out_idx), i32(lens)

    def run():
        out = torch.full((cnt + 2, H), -3.0, device=DEV)
        sv = [torch.zeros(cnt, T, H, device=DEV) for _ in range(2)]
        bits = [torch.zeros(cnt, H, dtype=torch.int64, device=DEV) for _ in range(2)]
        _launch(cnt, T, [(planes[0], d(_lin(0)[1]), 1), (planes[1], d(_lin(1)[1]), 1)], tail=2, X=xd, x_gstride=T * H, x_idx=xi,
                out=out, out_gstride=H, out_idx=oi, len=ln, save=sv, save_bits=bits)
        return dict(out=out, s0=sv[0], s1=sv[1], b0=bits[0], b1=bits[1])
    on, off = _both(run)
    _same(on, off, skip=('b0', 'b1'))             # (the bits are indexed by tile: another layout when packed)
    acts = _mlp_ref(x[x_idx.long()], 2)
    for i in range(cnt):
        ref = acts[1][i][:lens[i]].sum(0)
        _close(on['out'][int(out_idx[i])], ref, 2e-5, ('sum', i))
    _close(on['s0'], acts[0], 1e-4, 's0'); _close(on['s1'], acts[1], 1e-4, 's1')
    untouched = torch.ones(cnt + 2, dtype=torch.bool); untouched[out_idx.long()] = False
    assert bool((on['out'].cpu()[untouched] == -3.0).all())
    P = lib.stair_tile_pack_factor(T)
    for res, p in ((on, P), (off, 1)):
        for l in range(2):
            want, real = _expected_bits(res['s%d' % l], T, cnt, p)
            tiles = want.shape[0]
            got = res['b%d' % l].cpu()
            assert torch.equal(got[:tiles] & real, want), (l, p)
            assert bool((got[tiles:] == 0).all())              # a packed launch writes the first ceil(cnt / P) tiles' words only
            if l == 0:
                assert torch.equal(got[:tiles] & ~real, torch.zeros_like(want))


@pytest.mark.parametrize('T,cnt,indexed', [pytest.param(T, cnt, True, id='%d-%d' % (T, cnt)) for T, cnt in CASES] +
                         [pytest.param(8, 9, False, id='8-9-no_out_idx'), pytest.param(21, 4, False, id='21-4-no_out_idx')])
def test_filterframe_shape(T, cnt, indexed):
    """3 layers, the sigmoid attention (with the per-instance keyword term `extra`) between the second and the third, rs_out, STORE
    (through out_idx, or without one: instance i into tile i of `out`)"""
    from stair_amd import ops
    g = _gen(T, cnt, 2)
    x = torch.randn(cnt, T, H, generator=g)
    vw = torch.randn(H, generator=g) / H ** 0.5; vb = torch.randn(1, generator=g); extra = torch.randn(cnt, generator=g)
    out_idx = _perm(cnt + 2, cnt, g) if indexed else torch.arange(cnt, dtype=torch.int32)
    layers = [(d(_lin(i)[0]), d(_lin(i)[1]), 'relu') for i in range(3)]
    xd, oi, mid = d(x), d(out_idx) if indexed else None, (d(vw), d(vb), d(extra))

    def run():
        out = torch.full((cnt + 2, T, H), -3.0, device=DEV)
        saves, rs = ops.tile_mlp(xd, layers, 'store', save=True, mid_rowdot=mid, out=out, out_idx=oi)
        return dict(out=out, s0=saves[0], s1=saves[1], s2=saves[2], rs=rs)
    on, off = _both(run)
    _same(on, off)
    f = _mlp_ref(x, 2)[1]
    a = torch.sigmoid(f @ vw.double() + extra.double().unsqueeze(1) + vb.double())
    w3, b3 = _lin(2)
    ref = torch.relu((a.unsqueeze(-1) * f) @ w3.double().t() + b3.double())
    _close(on['out'].cpu()[out_idx.long()], ref, 3e-5, 'out')
    _close(on['s1'], f, 1e-4, 'f')
    assert float((on['rs'].cpu().double() - a).abs().max()) < 1e-5
    untouched = torch.ones(cnt + 2, dtype=torch.bool); untouched[out_idx.long()] = False
    assert bool((on['out'].cpu()[untouched] == -3.0).all())


@pytest.mark.parametrize('T,cnt', CASES)
def test_localize_shape(T, cnt):
    """2 layers + cosine against each instance's own keyword rows: 0, 1 and 3 pairs in one launch"""
    from stair_amd import ops
    g = _gen(T, cnt, 3)
    n_src = cnt + 1
    x = torch.randn(n_src, T, H, generator=g)
    x_idx = torch.randint(0, n_src, (cnt,), generator=g, dtype=torch.int32)
    K = [(3, 0, 1)[i % 3] for i in range(cnt)]
    first = np.concatenate([[0], np.cumsum(K)])[:-1]
    kb = torch.randn(sum(K) + 1, H, generator=g)
    att_idx = _perm(sum(K) + 3, sum(K), g) if sum(K) else torch.zeros(0, dtype=torch.int32)
    layers = [(d(_lin(0)[0]), d(_lin(0)[1]), 'relu'), (d(_lin(1)[0]), d(_lin(1)[1]), None)]
    xd, xi, kbd, pf, pc, ai = d(x), d(x_idx), d(kb), i32(first), i32(K), d(att_idx) if sum(K) else torch.zeros(1, dtype=torch.int32, device=DEV)

    def run():
        att = torch.full((sum(K) + 3, T), -3.0, device=DEV)
        ops.tile_mlp(xd, layers, 'cosine', x_idx=xi, kb=kbd, pair_first=pf, pair_cnt=pc, att_idx=ai, att=att)
        return dict(att=att)
    on, off = _both(run)
    _same(on, off)
    f = _mlp_ref(x[x_idx.long()], 2, last_relu=False)[1]
    written = torch.zeros(sum(K) + 3, dtype=torch.bool)
    for i in range(cnt):
        for j in range(K[i]):
            k = kb[first[i] + j].double()
            ref = (torch.nn.functional.cosine_similarity(f[i], k.unsqueeze(0).expand(T, -1), dim=-1, eps=1e-8) + 1) * 0.49
            row = int(att_idx[first[i] + j])
            written[row] = True
            assert float((on['att'][row].cpu().double() - ref).abs().max()) < 2e-5, (i, j)
    assert bool((on['att'].cpu()[~written] == -3.0).all())


@pytest.mark.parametrize('T,cnt', CASES)
def test_hasitem_shape(T, cnt):
    """1 layer + sigmoid(w . row + b (+ extra of the row's instance)), one float per frame: out_gstride = T"""
    from stair_amd import ops
    g = _gen(T, cnt, 4)
    x = torch.randn(cnt, T, H, generator=g)
    vw = torch.randn(H, generator=g) / H ** 0.5; vb = torch.randn(1, generator=g); extra = torch.randn(cnt, generator=g)
    out_idx = _perm(cnt + 3, cnt, g)
    layers = [(d(_lin(0)[0]), d(_lin(0)[1]), 'relu')]
    xd, oi, vwd, vbd, ex = d(x), d(out_idx), d(vw), d(vb), d(extra)

    def run():
        att = torch.full((cnt + 3, T), -3.0, device=DEV)
        ops.tile_mlp(xd, layers, 'rowdot_sigmoid', out=att, out_idx=oi, out_gstride=T, vw=vwd, vb=vbd, extra=ex)
        return dict(att=att)
    on, off = _both(run)
    _same(on, off)
    f = _mlp_ref(x, 1)[0]
    ref = torch.sigmoid(f @ vw.double() + extra.double().unsqueeze(1) + vb.double())
    assert float((on['att'].cpu()[out_idx.long()].double() - ref).abs().max()) < 1e-5
    untouched = torch.ones(cnt + 3, dtype=torch.bool); untouched[out_idx.long()] = False
    assert bool((on['att'].cpu()[untouched] == -3.0).all())


@pytest.mark.parametrize('T,cnt', CASES)
def test_temporal_shape(T, cnt):
    """row-scaled input (scale rows shared through rs_idx), 1 layer, LayerNorm through out_idx"""
    from stair_amd import ops
    g = _gen(T, cnt, 5)
    n_src = cnt + 1
    x = torch.randn(n_src, T, H, generator=g)
    x_idx = torch.randint(0, n_src, (cnt,), generator=g, dtype=torch.int32)
    r = torch.rand(cnt + 1, T, generator=g)
    rs_idx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g); beta = 0.1 * torch.randn(H, generator=g)
    out_idx = _perm(cnt + 2, cnt, g)
    layers = [(d(_lin(0)[0]), d(_lin(0)[1]), 'relu')]
    xd, xi, rd, ri, oi, gd, bd = d(x), d(x_idx), d(r), d(rs_idx), d(out_idx), d(gamma), d(beta)

    def run():
        out = torch.full((cnt + 2, T, H), -3.0, device=DEV)
        saves, _ = ops.tile_mlp(xd, layers, 'layernorm', x_idx=xi, row_scale=rd, rs_idx=ri, save=True, out=out, out_idx=oi, gamma=gd, beta=bd, eps=1e-5)
        return dict(out=out, s0=saves[0])
    on, off = _both(run)
    _same(on, off)
    w, b = _lin(0)
    y = torch.relu((r[rs_idx.long()].double().unsqueeze(-1) * x[x_idx.long()].double()) @ w.double().t() + b.double())
    ref = torch.nn.functional.layer_norm(y, (H,), gamma.double(), beta.double(), 1e-5)
    assert float((on['out'].cpu()[out_idx.long()].double() - ref).abs().max()) < 5e-5
    _close(on['s0'], y, 1e-4, 'y')
    untouched = torch.ones(cnt + 2, dtype=torch.bool); untouched[out_idx.long()] = False
    assert bool((on['out'].cpu()[untouched] == -3.0).all())


@pytest.mark.parametrize('T,cnt', CASES)
def test_dropout_drops_the_same_elements(T, cnt):
    """nn.Dropout(0.25) behind both activations: element (instance * T + frame) * H + column draws its bit whatever tile it sits in"""
    p = 0.25
    g0 = _gen(T, cnt, 6)
    state = g0.get_state()

    def run():
        g = torch.Generator(); g.set_state(state)
        x, sv, bits = _fwd2(T, cnt, g, drop=(p, 11))
        run.x = x
        return dict(s0=sv[0], s1=sv[1])
    on, off = _both(run)
    _same(on, off)
    # fp64 with the kernel's own keep masks (a dropped element is an exact zero; the layers' ReLU zeros are zero either way)
    w0, b0 = _lin(0); w1, b1 = _lin(1)
    c0, c1 = (on['s0'].cpu() != 0).double(), (on['s1'].cpu() != 0).double()
    h0 = torch.relu(run.x.double() @ w0.double().t() + b0.double())
    kept0 = h0 * c0 / (1 - p)
    _close(on['s0'], kept0, 1e-4, 's0')
    h1 = torch.relu(kept0 @ w1.double().t() + b1.double())
    _close(on['s1'], h1 * c1 / (1 - p), 1e-4, 's1')
    # the masks are on, at about the rate asked for: of the clearly positive activations a quarter is dropped
    pos = h0 > 1e-3
    rate = 1.0 - float(c0[pos].mean())
    n = int(pos.sum())
    assert abs(rate - p) < 5 * (p * (1 - p) / n) ** 0.5 + 1e-3, (rate, n)


# ---------------------------------------------------------------------------------------------
# backward chains
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize('T,cnt,tail', [pytest.param(T, cnt, 6, id='%d-%d' % (T, cnt)) for T, cnt in CASES] +
                         [pytest.param(8, 9, 1, id='8-9-store'), pytest.param(21, 4, 1, id='21-4-store')])
def test_backward_chain_exclusive_with_first_touch_stores(T, cnt, tail):
    """KIND 3 fed by the bits of a forward launch with the same packing: dZ saves, read - add - write into targets of the instances' own,
    some marked STORE_FIRST (their targets hold a sentinel no result may depend on).  `store`: the same chain ending in STORE (tail 1),
    which writes dX over every target whatever it held and whatever its out_idx entry's STORE_FIRST bit says"""
    from stair_amd import ops
    g = _gen(T, cnt, 7)
    dy = torch.randn(cnt, T, H, generator=g)
    tgt = _perm(cnt + 2, cnt, g)
    first = [(i % 3) != 1 for i in range(cnt)]
    base = torch.randn(cnt + 2, T, H, generator=g)
    for i in range(cnt):
        if first[i]:
            base[int(tgt[i])] = float('nan')
    out_idx = i32([int(tgt[i]) | (STORE_FIRST if first[i] else 0) for i in range(cnt)])
    wT = [ops.pack_wfrag(d(_lin(i)[0]), transpose=True) for i in range(2)]
    dyd, based = d(dy), d(base)
    gstate = g.get_state()

    def run():
        gg = torch.Generator(); gg.set_state(gstate)
        _, sv, bits = _fwd2(T, cnt, gg)
        out = based.clone()
        gB, gA = torch.zeros(cnt, T, H, device=DEV), torch.zeros(cnt, T, H, device=DEV)
        _launch(cnt, T, [(wT[1], None, 3), (wT[0], None, 0)], tail=tail, X=dyd, x_gstride=T * H, in_bits=bits[1], in_scale=1.0, save_in=gB,
                act_bits=[bits[0]], act_scale=1.0, save=[gA], out=out, out_gstride=T * H, out_idx=out_idx, acc_exclusive=1)
        run.sv = sv
        return dict(out=out, gA=gA, gB=gB)
    on, off = _both(run)
    assert not bool(on['out'].cpu()[tgt.long()].isnan().any())
    got_on, got_off = on['out'].cpu()[tgt.long()], off['out'].cpu()[tgt.long()]
    assert torch.equal(got_on, got_off) and torch.equal(on['gA'], off['gA']) and torch.equal(on['gB'], off['gB'])
    rest = torch.ones(cnt + 2, dtype=torch.bool); rest[tgt.long()] = False
    assert torch.equal(on['out'].cpu()[rest], base[rest])
    dz2, dz1, dx = _chain_ref(dy, run.sv)
    _close(on['gB'], dz2, 3e-5, 'dZ2'); _close(on['gA'], dz1, 3e-5, 'dZ1')
    for i in range(cnt):
        ref = dx[i] if first[i] or tail == 1 else dx[i] + base[int(tgt[i])].double()
        _close(got_on[i], ref, 3e-5, ('dX', i))


@pytest.mark.parametrize('T,cnt', CASES)
def test_backward_chain_broadcast_input_and_atomic_pairs(T, cnt):
    """KIND 3 with Filter's input -- ONE gradient row per instance over its own frames (len) -- and float atomics into zeroed targets
    that exactly two instances share (two addends into zero commute: still bit for bit)"""
    from stair_amd import ops
    g = _gen(T, cnt, 8)
    rows = torch.randn(cnt + 1, H, generator=g)
    x_idx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    lens = [(T, max(1, T - 3), 1, max(1, T // 2))[i % 4] for i in range(cnt)]
    tgt = torch.tensor([i // 2 for i in range(cnt)], dtype=torch.int32)[torch.randperm(cnt, generator=g)]
    wT = [ops.pack_wfrag(d(_lin(i)[0]), transpose=True) for i in range(2)]
    rd, xi, ln, oi = d(rows), d(x_idx), i32(lens), d(tgt)
    gstate = g.get_state()

    def run():
        gg = torch.Generator(); gg.set_state(gstate)
        _, sv, bits = _fwd2(T, cnt, gg)
        out = torch.zeros((cnt + 1) // 2 + 1, T, H, device=DEV)
        gB, gA = torch.full((cnt, T, H), -3.0, device=DEV), torch.full((cnt, T, H), -3.0, device=DEV)
        _launch(cnt, T, [(wT[1], None, 3), (wT[0], None, 0)], tail=6, X=rd, x_gstride=H, x_idx=xi, x_broadcast=1, len=ln,
                in_bits=bits[1], in_scale=1.0, save_in=gB, act_bits=[bits[0]], act_scale=1.0, save=[gA],
                out=out, out_gstride=T * H, out_idx=oi, acc_exclusive=0)
        run.sv = sv
        return dict(out=out, gA=gA, gB=gB)
    on, off = _both(run)
    _same(on, off)
    dy = rows[x_idx.long()].unsqueeze(1).expand(-1, T, -1).clone()
    for i in range(cnt):
        dy[i, lens[i]:] = 0.0                       # a broadcast row fills the clip's own frames only
    dz2, dz1, dx = _chain_ref(dy, run.sv)
    _close(on['gB'], dz2, 3e-5, 'dZ2'); _close(on['gA'], dz1, 3e-5, 'dZ1')
    ref = torch.zeros((cnt + 1) // 2 + 1, T, H, dtype=torch.float64)
    ref.index_add_(0, tgt.long(), dx)
    _close(on['out'], ref, 3e-5, 'dX')


@pytest.mark.parametrize('T,cnt', CASES)
def test_backward_chain_float_masks_and_atomic_first_touch(T, cnt):
    """KIND 3 with the relu' masks as fp32 activations instead of bits -- the input's through in_mask_idx (mask tiles shared by
    instances), the layer's as act_mask [cnt, T, H] -- and the atomic ACCUMULATE branch where some instances store first (sentinel
    targets) and the others add into targets of their own (one add per address: bit for bit)"""
    from stair_amd import ops
    g = _gen(T, cnt, 10)
    dy = torch.randn(cnt + 1, T, H, generator=g)
    x_idx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    m_in = torch.randn(cnt + 1, T, H, generator=g)
    m_idx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    m_act = torch.randn(cnt, T, H, generator=g)
    tgt = _perm(cnt + 2, cnt, g)
    first = [(i % 3) != 1 for i in range(cnt)]
    base = torch.randn(cnt + 2, T, H, generator=g)
    for i in range(cnt):
        if first[i]:
            base[int(tgt[i])] = float('nan')
    out_idx = i32([int(tgt[i]) | (STORE_FIRST if first[i] else 0) for i in range(cnt)])
    wT = [ops.pack_wfrag(d(_lin(i)[0]), transpose=True) for i in range(2)]
    dyd, xi, mind, mi, mactd, based = d(dy), d(x_idx), d(m_in), d(m_idx), d(m_act), d(base)

    def run():
        out = based.clone()
        gB, gA = torch.zeros(cnt, T, H, device=DEV), torch.zeros(cnt, T, H, device=DEV)
        _launch(cnt, T, [(wT[1], None, 3), (wT[0], None, 0)], tail=6, X=dyd, x_gstride=T * H, x_idx=xi,
                in_mask=mind, in_mask_gstride=T * H, in_mask_idx=mi, in_scale=1.0, save_in=gB,
                act_mask=[mactd], act_scale=1.0, save=[gA], out=out, out_gstride=T * H, out_idx=out_idx, acc_exclusive=0)
        return dict(out=out, gA=gA, gB=gB)
    on, off = _both(run)
    got_on, got_off = on['out'].cpu()[tgt.long()], off['out'].cpu()[tgt.long()]
    assert not bool(got_on.isnan().any())
    assert torch.equal(got_on, got_off) and torch.equal(on['gA'], off['gA']) and torch.equal(on['gB'], off['gB'])
    rest = torch.ones(cnt + 2, dtype=torch.bool); rest[tgt.long()] = False
    assert torch.equal(on['out'].cpu()[rest], base[rest])
    dz2 = dy[x_idx.long()].double() * (m_in[m_idx.long()] > 0).double()
    dz1 = (dz2 @ _lin(1)[0].double()) * (m_act > 0).double()
    dx = dz1 @ _lin(0)[0].double()
    _close(on['gB'], dz2, 3e-5, 'dZ2'); _close(on['gA'], dz1, 3e-5, 'dZ1')
    for i in range(cnt):
        ref = dx[i] if first[i] else dx[i] + base[int(tgt[i])].double()
        _close(got_on[i], ref, 3e-5, ('dX', i))


@pytest.mark.parametrize('mode', ['exclusive', 'exclusive_mixed', 'all_first', 'atomic_mixed'])
@pytest.mark.parametrize('T,cnt', CASES)
def test_temporal_backward_chain(T, cnt, mode):
    """KIND 2: the LayerNorm adjoint in, the row-scale adjoint out.  dZ, d feat (exclusive targets) and d r (one add per address) bit for
    bit; d gamma / d beta are float sums over a TILE's rows, grouped differently when a tile holds several instances: within the bound
    of tests/test_gpu_tile_fused.py::test_fused_and_sequenced_paths_agree_forward_and_backward, 2e-4 of the tensor's largest entry
    (or of 1e-3 of the largest of the compared tensors).  The three branches of the ROWSCALE_ADJ tail: read - add - write (`exclusive`;
    `exclusive_mixed`: some instances store first instead, into sentinel targets), every instance of a tile stores (`all_first`),
    float atomics with some instances storing (`atomic_mixed`; targets of the instances' own, so one add per address).
    Two packed runs: everything bit for bit, except that d gamma / d beta of a launch of more than two tiles are left out -- outside a
    plan's backward pass they are float atomics, one per workgroup and column, and three addends do not commute bit for bit (as in
    the unpacked kernel).  Inside a plan they go through the fixed-point shadows; their reproducibility under packing is what
    test_training_step_is_reproducible_with_packing_and_queue checks, on a batch whose Temporal bucket spans more than two tiles."""
    from stair_amd import ops
    g = _gen(T, cnt, 9)
    first = [{'exclusive': False, 'all_first': True}.get(mode, (i % 3) != 1) for i in range(cnt)]
    feat = torch.randn(cnt + 1, T, H, generator=g)
    fidx = _perm(cnt + 1, cnt, g)
    rs = torch.rand(cnt + 2, T, generator=g)
    ridx = _perm(cnt + 2, cnt, g)
    w, b = _lin(0)
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g)
    dy = torch.randn(cnt + 1, T, H, generator=g)
    yidx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    F = feat.double().requires_grad_(True); R = rs.double().requires_grad_(True)
    G = gamma.double().requires_grad_(True); Bt = torch.zeros(H, dtype=torch.float64, requires_grad=True)
    z = (R[ridx.long()].unsqueeze(-1) * F[fidx.long()]) @ w.double().t() + b.double()
    z.retain_grad()
    a = torch.relu(z)
    y = torch.nn.functional.layer_norm(a, (H,), G, Bt, 1e-5)
    (y * dy[yidx.long()].double()).sum().backward()
    dfeat0 = torch.randn(cnt + 1, T, H, generator=g); drs0 = torch.randn(cnt + 2, T, generator=g)
    for i in range(cnt):
        if first[i]:
            dfeat0[int(fidx[i])] = float('nan')         # a target that is stored is not read
    ad, dyd, gd, wd, fd, rd = d(a.detach().float()), d(dy), d(gamma), d(w), d(feat), d(rs)
    yi, fi, ri = d(yidx), d(fidx), d(ridx)
    oi = i32([int(fidx[i]) | (STORE_FIRST if first[i] else 0) for i in range(cnt)])

    def run():
        dfeat, drs = d(dfeat0.clone()), d(drs0.clone())
        dgamma, dbeta = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
        dz = ops.tile_temporal_bwd(dyd, ad, gd, wd, fd, rd, dfeat, drs, dgamma, dbeta, dy_idx=yi, feat_idx=fi, rs_idx=ri, dfeat_idx=oi, exclusive=mode != 'atomic_mixed')
        return dict(dz=dz, dfeat=dfeat, drs=drs, dgamma=dgamma, dbeta=dbeta)
    on, off = _both(run)
    used = fidx.long()
    for res in (on, off):                           # (the one feature tile no instance uses keeps whatever it held)
        res['dfeat'] = res['dfeat'][used.to(DEV)]
    assert not bool(on['dfeat'].isnan().any())
    _same(on, off, skip=('dgamma', 'dbeta'))
    gmax = max(float(off['dgamma'].abs().max()), float(off['dbeta'].abs().max()))
    for k in ('dgamma', 'dbeta'):
        bound = 2e-4 * max(float(off[k].abs().max()), 1e-3 * gmax)
        assert float((on[k] - off[k]).abs().max()) < bound, k
    P = lib.stair_tile_pack_factor(T)
    # a second packed run.  Outside a plan's backward pass d gamma / d beta are added with float atomics, one per workgroup and
    # column (inside one they go through the fixed-point shadows): from zero, one or two addends give the same bits in any order
    lib.stair_set_tile_pack(1)
    again = run()
    again['dfeat'] = again['dfeat'][used.to(DEV)]
    lib.stair_set_tile_pack(-1)
    tiles = (cnt + P - 1) // P
    _same(again, on, skip=() if tiles <= 2 else ('dgamma', 'dbeta'))
    # fp64 autograd, at the tolerance of tests/test_gpu_tile_fused.py::test_temporal_backward_chain_matches_autograd
    _close(on['dz'], z.grad, 3e-5, 'dZ')
    for i in range(cnt):
        ref = F.grad[used[i]] if first[i] else F.grad[used[i]] + dfeat0[used[i]].double()
        _close(on['dfeat'][i], ref, 3e-5, ('dfeat', i))
    _close(on['drs'].cpu() - drs0, R.grad, 3e-5, 'drs')
    _close(on['dgamma'], G.grad, 3e-5, 'dgamma')
    _close(on['dbeta'], Bt.grad, 3e-5, 'dbeta')


@pytest.mark.parametrize('T,cnt,packed,unpacked', [(8, 17, 3, 17), (33, 3, 3, 3)])
def test_work_item_count(T, cnt, packed, unpacked):
    from stair_amd import ops
    x = torch.randn(cnt, T, H, device=DEV)
    out = torch.empty(cnt, T, H, device=DEV)
    layers = [(d(_lin(0)[0]), d(_lin(0)[1]), 'relu')]
    for on, want in ((1, packed), (0, unpacked)):
        lib.stair_set_tile_pack(on)
        _work_items()
        ops.tile_mlp(x, layers, 'store', out=out)
        assert _work_items() == want, (on, want)
        assert _work_items() == 0


# ---------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------
LINEAR_T8 = dict(spec.DEFAULT_CONFIG, video_size=128, answer_vocab_length=16, max_video_length=8, object_types=10)
CONV_T64 = dict(spec.DEFAULT_CONFIG, video_size=128, answer_vocab_length=16, max_video_length=64, object_types=10)
LN_GRADS = ('submodules.Temporal.layer_norm.weight', 'submodules.Temporal.layer_norm.bias')


def _model(config, seed=1):
    from stair_amd.module_net import VideoNMN
    m = VideoNMN(config)
    w = synth.make_weights(config, seed)
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    return m.to(DEV)


def _questions(config, T, frames=None):
    qs = synth.make_questions(config, 5, 12, forms=synth.ALL_FORMS, T=T)
    if frames:
        for i, q in enumerate(qs):
            q['video_features'] = torch.as_tensor(q['video_features'])[:frames[i % len(frames)]].clone()
    return qs


def _oracle_pass(config, qs, res, seed=1):
    """logits and parameter gradients of the oracle (mean CE over the batch), every module / decoder ReLU differentiated through the
    mask the HIP forward pass produced (tests/helpers.py::_ForcedMasks, as tests/test_gpu_bench_path.py::
    test_full_size_gradients_are_strict_given_the_same_relu_masks): in split-bf16 mode -- the only one the tile operators run in -- a
    pre-activation within rounding of zero may take the other side of its ReLU, which is a property of the comparison, not of packing.
    Must run between the HIP forward and backward passes (the backward pass reuses parts of the workspace)."""
    from helpers import _ForcedMasks
    names = [n for n, _ in spec.weight_table(config)]
    weights = synth.make_weights(config, seed)
    w = {k: torch.from_numpy(weights[k].copy()).requires_grad_(True) for k in names}
    logits = []
    for qi, q in enumerate(qs):
        fm = _ForcedMasks(res, qi, q['nmn_program_list'])
        lg = fm.forward(w, config, q, return_res_by_step=False, explicit_lstm=True)['logits']
        logits.append(lg.detach())
        ce = torch.nn.functional.cross_entropy(lg.unsqueeze(0), torch.tensor([q['answer']]))
        (ce / len(qs)).backward()
    return logits, {n: w[n].grad for n in names}


def _train_pass(config, qs, pack, oracle=False, switch_before_backward=None):
    """one training pass (forward + backward of the mean CE) on a fresh model: logits, gradients, tile work items"""
    model = _model(config)
    if pack is not None:
        model.set_option('tile_pack', pack)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    _work_items()
    res = model.forward_batch(qs, train=True)
    logits = res.logits.detach().cpu().clone()
    ref = _oracle_pass(config, qs, res) if oracle else None
    if switch_before_backward is not None:
        lib.stair_set_tile_pack(switch_before_backward)
    res.backward(torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV), 1.0 / len(qs))
    torch.cuda.synchronize()
    items = _work_items()
    lib.stair_set_tile_pack(-1)
    return dict(logits=logits, grads={n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}, items=items, oracle=ref)


_PASSES = {}


def _passes(name):
    """the packed (default) pass, with the oracle's, and the unpacked pass of a configuration: computed once, never changed"""
    if name not in _PASSES:
        config, qs = {'linear_t8': (LINEAR_T8, _questions(LINEAR_T8, 8)),
                      'conv_ragged': (CONV_T64, _questions(CONV_T64, 24, frames=[3, 17, 24]))}[name]
        _PASSES[name] = dict(config=config, qs=qs, on=_train_pass(config, qs, None, oracle=True), off=_train_pass(config, qs, 0))
    return _PASSES[name]


def _compare_passes(c):
    on, off = c['on'], c['off']
    assert torch.equal(on['logits'], off['logits'])
    gmax = max(float(g.abs().max()) for g in off['grads'].values())
    for n, g in off['grads'].items():
        if n in LN_GRADS:                       # float sums over a tile's rows ahead of the fixed-point shadows (see test_temporal_backward_chain)
            assert float((on['grads'][n] - g).abs().max()) < 2e-4 * max(float(g.abs().max()), 1e-3 * gmax), n
        else:
            assert torch.equal(on['grads'][n], g), (n, float((on['grads'][n] - g).abs().max()))
    assert any(float(off['grads'][n].abs().max()) > 0 for n in LN_GRADS)
    # the packed pass against the oracle: logits as tests/test_gpu_parity.py::test_appearance_feature_config_against_oracle,
    # gradients as tests/test_gpu_train.py::test_backward_on_odd_shapes
    ref_logits, ref_grads = on['oracle']
    for qi, lg in enumerate(ref_logits):
        assert float((on['logits'][qi] - lg).abs().max()) < 1e-4, qi
        assert int(torch.argmax(on['logits'][qi])) == int(torch.argmax(lg)), qi
    for n, ref in ref_grads.items():
        if ref is None:
            continue
        assert float((on['grads'][n] - ref).abs().max()) < 2e-4 * max(float(ref.abs().max()), 1e-3), n
    assert 0 < on['items'] < off['items'], (on['items'], off['items'])


def test_plan_linear_temporal_t8_packed_equals_unpacked():
    """max_video_length = 8 (Linear(T, T) Temporal nets), all 12 program forms, one training pass: P = 8"""
    _compare_passes(_passes('linear_t8'))


def test_plan_conv_temporal_ragged_clips_packed_equals_unpacked():
    """max_video_length = 64 (Conv1d Temporal nets), clips of 3, 17 and 24 frames: plan T = 24, P = 2, per-instance len"""
    c = _passes('conv_ragged')
    assert sorted({int(q['video_features'].shape[0]) for q in c['qs']}) == [3, 17, 24]
    _compare_passes(c)


def test_plan_keeps_its_packing_when_the_switch_moves_before_the_backward_pass():
    """the relu' bits are indexed by tile: the chains of a plan run with the packing of the forward pass that wrote them"""
    c = _passes('linear_t8')
    moved = _train_pass(c['config'], c['qs'], None, switch_before_backward=0)
    assert torch.equal(moved['logits'], c['on']['logits'])
    for n, g in c['on']['grads'].items():
        assert torch.equal(moved['grads'][n], g), n


def test_training_step_is_reproducible_with_packing_and_queue():
    """two Trainer.step calls from identical state (packing and work queue on, the defaults): the same weights, bit for bit.  This is
    also where the run-to-run reproducibility of Temporal's LayerNorm gradients under packing is checked (fixed-point shadows behind
    per-tile float sums): 240 questions, so that one (level, mode) of Temporal has more than 2 P = 16 instances -- more than two
    packed tiles, several workgroups adding into the same shadow"""
    from collections import Counter
    from stair_amd.train import Trainer
    config = LINEAR_T8
    qs = synth.make_questions(config, 5, 240, forms=synth.ALL_FORMS, T=8)
    same_bucket = Counter((q['form'], i, q['nmn_program_list'][i + 1]) for q in qs for i, t in enumerate(q['nmn_program_list']) if t == 'Temporal')
    assert max(same_bucket.values()) > 2 * lib.stair_tile_pack_factor(8), same_bucket.most_common(3)
    video = torch.stack([torch.as_tensor(q['video_features']) for q in qs]).to(DEV)
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV)
    args = ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], video, question,
            [q['question'].shape[0] for q in qs], torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV))
    after = []
    for _ in range(2):
        tr = Trainer(_model(config), dropout=0.0, lr=1e-3)
        _work_items()
        tr.step(*args)
        tr.check()
        torch.cuda.synchronize()
        assert _work_items() > 0
        after.append(tr.flat_p.clone())
    assert torch.equal(after[0], after[1])
    assert not torch.equal(after[0], Trainer(_model(config), dropout=0.0, lr=1e-3).flat_p)


def test_packed_forward_reads_no_uninitialised_workspace():
    """as tests/test_gpu_parity.py::test_forward_reads_no_uninitialised_workspace, at T = 8 (P = 8; 12 and 31 questions: full and
    partial last tiles; Linear-Temporal configurations take every clip at max_video_length)"""
    config = LINEAR_T8
    model = _model(config, 4)
    batches = [synth.make_questions(config, 31, 12, forms=synth.ALL_FORMS, T=8), synth.make_questions(config, 32, 31, forms=synth.ALL_FORMS, T=8)]
    for qs in batches:
        _work_items()
        ref = model.forward_batch(qs).logits.clone()
        packed_items = _work_items()
        for poison in (float('nan'), 1e30, -7.0):
            model._ws.fill_(poison)
            got = model.forward_batch(qs).logits
            assert torch.equal(got, ref), (poison, int(got.isnan().sum()))
        assert packed_items > 0
