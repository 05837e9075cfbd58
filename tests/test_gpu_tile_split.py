"""Segmented tiles of the fused tile operators (csrc/tile_mlp.hip, the SPLIT kernel forms; include/stair_hip.h stair_set_tile_split):
an instance of 64 < T <= 141 frames runs as ceil(T / 64) segments of 64 rows.  A row's result depends on no other row, so every
row-wise output of a segmented launch must equal, bit for bit, what the unsegmented kernel gives when each segment is launched as
an instance of its own (one launch per segment number over sliced views of the same buffers, packing off); it is also compared
with fp64 at the tolerance tests/test_gpu_building_blocks.py (forward operators) or tests/test_gpu_tile_fused.py (chains) uses for
the same operator.  Filter's sum over frames is the one tail that crosses segments: fp64, and bit-identical from run to run.
A segment behind its clip's end (ragged: 64 g >= len) is not computed and holds zeros wherever a live segment writes.  `-m gpu`."""
import numpy as np
import pytest
import torch

from stair_amd import spec, synth
from stair_amd._lib import lib, check
from tile_helpers import (DEV, H, STORE_FIRST, _gen, _lin, _planes, d, i32, _perm, _close, _launch, _fwd_layers, _mlp_ref, _chain_ref,
                          _fwd2, _tile_words, _work_items)

pytestmark = pytest.mark.gpu
# (T, cnt, lens): one live row in segment 1 / the same, several instances / a partial second segment / two full segments / three
# segments / the largest admitted T / ragged: a one-row segment (65), an exactly empty one (64), an empty one behind a short clip (30, 1)
CASES = [(65, 1, None), (65, 3, None), (100, 2, None), (128, 3, None), (129, 2, None), (141, 1, None), (100, 5, (100, 65, 64, 30, 1))]
IDS = ['65x1', '65x3', '100x2', '128x3', '129x2', '141x1', 'ragged100']
cases = pytest.mark.parametrize('T,cnt,lens', CASES, ids=IDS)


@pytest.fixture(autouse=True)
def default_switches():
    yield
    lib.stair_set_tile_split(-1)
    lib.stair_set_tile_pack(-1)
    lib.stair_set_tile_queue(-1)


def _segs(T):
    """(segment, first frame, rows) of a clip of T frames"""
    return [(s, 64 * s, min(64, T - 64 * s)) for s in range((T + 63) // 64)]


def _at(t, elems):
    """address of element `elems` of a float32 / int64 tensor"""
    return t.data_ptr() + elems * t.element_size()


def _exists_words(rows):
    """the bits of a tile's words that belong to its first `rows` rows: word (64 w + c), byte j, bit e <-> row w + 8 j, column 8 c + e
    (as _expected_bits of tests/test_gpu_tile_pack.py, one instance per tile)"""
    return _tile_words((torch.arange(64) < rows).reshape(1, 64, 1).expand(1, 64, H))[0]


def _bits_of(act_seg):
    """save_bits words [cnt, 512] of activation rows act_seg [cnt, rows <= 64, 512], as the kernel lays them out"""
    cnt, rows, _ = act_seg.shape
    pos = torch.zeros(cnt, 64, H, dtype=torch.bool)
    pos[:, :rows] = act_seg.cpu() > 0
    return _tile_words(pos)


def _live(lens, i, f0):
    return lens is None or f0 < lens[i]


def _zero_dead(t, T, lens, per_frame_dim=1):
    """expected values: zeros in the segments behind a clip's end (t: [cnt, T, ...] on the CPU, changed in place)"""
    if lens is not None:
        for i, ln in enumerate(lens):
            for _, f0, rows in _segs(T):
                if f0 >= ln:
                    t[i, f0:f0 + rows] = 0
    return t


def _check_bits(got, saved, T, cnt, lens, what):
    """got: save_bits [cnt * S, 512] of a segmented launch; saved: the activation it saved [cnt, T, 512]"""
    S = len(_segs(T))
    got = got.cpu().reshape(cnt, S, H)
    for s, f0, rows in _segs(T):
        real = _exists_words(rows)
        want = _bits_of(saved[:, f0:f0 + rows])
        assert torch.equal(got[:, s] & real, want), (what, s)
        for i in range(cnt):
            if not _live(lens, i, f0):
                assert bool((got[i, s] == 0).all()), (what, s, i)


# ---------------------------------------------------------------------------------------------
# forward operators: the segmented launch against one unsegmented launch per segment number
# ---------------------------------------------------------------------------------------------
def _per_segment(T, run_seg):
    """run_seg(s, f0, rows) for every segment, as today's kernel sees it: the segment switch off is not needed (rows <= 64), packing
    off so that a short last segment is one instance per tile as well"""
    lib.stair_set_tile_pack(0)
    for s, f0, rows in _segs(T):
        run_seg(s, f0, rows)
    lib.stair_set_tile_pack(-1)
    torch.cuda.synchronize()


@cases
def test_filterframe_shape(T, cnt, lens):
    """3 layers, the sigmoid attention (per-instance keyword term `extra`) between the second and the third, rs_out, every layer's
    save and relu' bits, STORE through x_idx / out_idx"""
    g = _gen(T, cnt, 2)
    S = len(_segs(T))
    x = torch.randn(cnt + 1, T, H, generator=g)
    x_idx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    vw = torch.randn(H, generator=g) / H ** 0.5; vb = torch.randn(1, generator=g); extra = torch.randn(cnt, generator=g)
    out_idx = _perm(cnt + 2, cnt, g)
    xd, xi, oi, vwd, vbd, exd = d(x), d(x_idx), d(out_idx), d(vw), d(vb), d(extra)
    ln = i32(lens) if lens else None
    layers = _fwd_layers(3)
    out = torch.full((cnt + 2, T, H), -3.0, device=DEV)
    sv = [torch.full((cnt, T, H), -3.0, device=DEV) for _ in range(3)]
    bits = [torch.full((cnt * S, H), -1, dtype=torch.int64, device=DEV) for _ in range(3)]
    rs = torch.full((cnt, T), -3.0, device=DEV)
    _launch(cnt, T, layers, tail=1, X=xd, x_gstride=T * H, x_idx=xi, mid_rowdot=1, vw=vwd, vb=vbd, extra=exd, rs_out=rs,
            save=sv, save_bits=bits, out=out, out_gstride=T * H, out_idx=oi, len=ln)
    torch.cuda.synchronize()
    r_out = torch.full((cnt + 2, T, H), -3.0, device=DEV)
    r_sv = [torch.zeros(cnt, T, H) for _ in range(3)]
    r_rs = torch.zeros(cnt, T)
    r_bits = [torch.zeros(cnt, S, H, dtype=torch.int64) for _ in range(3)]

    def run_seg(s, f0, rows):
        ssv = [torch.zeros(cnt, rows, H, device=DEV) for _ in range(3)]
        sb = [torch.zeros(cnt, H, dtype=torch.int64, device=DEV) for _ in range(3)]
        srs = torch.zeros(cnt, rows, device=DEV)
        _launch(cnt, rows, layers, tail=1, X=_at(xd, f0 * H), x_gstride=T * H, x_idx=xi, mid_rowdot=1, vw=vwd, vb=vbd, extra=exd, rs_out=srs,
                save=ssv, save_bits=sb, out=_at(r_out, f0 * H), out_gstride=T * H, out_idx=oi)
        for l in range(3):
            r_sv[l][:, f0:f0 + rows] = ssv[l].cpu()
            r_bits[l][:, s] = sb[l].cpu()
        r_rs[:, f0:f0 + rows] = srs.cpu()
    _per_segment(T, run_seg)
    want_out = r_out.cpu()
    want_out[out_idx.long()] = _zero_dead(want_out[out_idx.long()], T, lens)
    assert torch.equal(out.cpu(), want_out)                      # (untouched tiles keep the sentinel in both)
    assert torch.equal(rs.cpu(), _zero_dead(r_rs, T, lens))
    for l in range(3):
        assert torch.equal(sv[l].cpu(), _zero_dead(r_sv[l], T, lens)), l
        for s, f0, rows in _segs(T):
            real = _exists_words(rows)
            for i in range(cnt):
                want = (r_bits[l][i, s] & real) if _live(lens, i, f0) else torch.zeros(H, dtype=torch.int64)
                assert torch.equal(bits[l].cpu().reshape(cnt, S, H)[i, s] & real, want), (l, s, i)
        _check_bits(bits[l], sv[l], T, cnt, lens, l)
    # fp64, the live frames
    f = _mlp_ref(x[x_idx.long()], 2)[1]
    a = torch.sigmoid(f @ vw.double() + extra.double().unsqueeze(1) + vb.double())
    w3, b3 = _lin(2)
    ref = torch.relu((a.unsqueeze(-1) * f) @ w3.double().t() + b3.double())
    keep = _zero_dead(torch.ones(cnt, T, 1), T, lens).double()
    _close(out.cpu()[out_idx.long()], ref * keep, 3e-5, 'out')
    _close(sv[1], f * keep, 1e-4, 'f')
    assert float((rs.cpu().double() - a * keep[..., 0]).abs().max()) < 1e-5


@cases
def test_localize_shape(T, cnt, lens):
    """2 layers + cosine against each instance's own keyword rows: K = 1 and 2 (and 0 when there are three instances or more)"""
    g = _gen(T, cnt, 3)
    x = torch.randn(cnt + 1, T, H, generator=g)
    x_idx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    K = [(2, 1, 0)[i % 3] for i in range(cnt)]
    first = np.concatenate([[0], np.cumsum(K)])[:-1]
    kb = torch.randn(sum(K) + 1, H, generator=g)
    att_idx = _perm(sum(K) + 3, sum(K), g)
    xd, xi, kbd, pf, pc, ai = d(x), d(x_idx), d(kb), i32(first), i32(K), d(att_idx)
    ln = i32(lens) if lens else None
    layers = _fwd_layers(2, last_relu=False)
    att = torch.full((sum(K) + 3, T), -3.0, device=DEV)
    _launch(cnt, T, layers, tail=3, X=xd, x_gstride=T * H, x_idx=xi, kb=kbd, pair_first=pf, pair_cnt=pc, att_idx=ai, att=att, len=ln)
    torch.cuda.synchronize()
    r_att = torch.full((sum(K) + 3, T), -3.0)

    def run_seg(s, f0, rows):
        satt = torch.full((sum(K) + 3, rows), -3.0, device=DEV)
        _launch(cnt, rows, layers, tail=3, X=_at(xd, f0 * H), x_gstride=T * H, x_idx=xi, kb=kbd, pair_first=pf, pair_cnt=pc, att_idx=ai, att=satt)
        r_att[:, f0:f0 + rows] = satt.cpu()
    _per_segment(T, run_seg)
    f = _mlp_ref(x[x_idx.long()], 2, last_relu=False)[1]
    written = torch.zeros(sum(K) + 3, dtype=torch.bool)
    for i in range(cnt):
        for j in range(K[i]):
            row = int(att_idx[first[i] + j])
            written[row] = True
            ref = (torch.nn.functional.cosine_similarity(f[i], kb[first[i] + j].double().unsqueeze(0).expand(T, -1), dim=-1, eps=1e-8) + 1) * 0.49
            for _, f0, rows in _segs(T):
                if not _live(lens, i, f0):
                    r_att[row, f0:f0 + rows] = 0
                    ref[f0:f0 + rows] = 0
            assert float((att[row].cpu().double() - ref).abs().max()) < 2e-5, (i, j)
    assert torch.equal(att.cpu(), r_att)
    assert bool((att.cpu()[~written] == -3.0).all())


@cases
def test_hasitem_shape(T, cnt, lens):
    """1 layer + sigmoid(w . row + b + extra of the instance), one float per frame: out_gstride = T"""
    g = _gen(T, cnt, 4)
    x = torch.randn(cnt, T, H, generator=g)
    vw = torch.randn(H, generator=g) / H ** 0.5; vb = torch.randn(1, generator=g); extra = torch.randn(cnt, generator=g)
    out_idx = _perm(cnt + 3, cnt, g)
    xd, oi, vwd, vbd, exd = d(x), d(out_idx), d(vw), d(vb), d(extra)
    ln = i32(lens) if lens else None
    layers = _fwd_layers(1)
    att = torch.full((cnt + 3, T), -3.0, device=DEV)
    sv = torch.full((cnt, T, H), -3.0, device=DEV)
    _launch(cnt, T, layers, tail=4, X=xd, x_gstride=T * H, vw=vwd, vb=vbd, extra=exd, out=att, out_gstride=T, out_idx=oi, save=[sv], len=ln)
    torch.cuda.synchronize()
    r_att = torch.full((cnt + 3, T), -3.0, device=DEV)

    def run_seg(s, f0, rows):
        _launch(cnt, rows, layers, tail=4, X=_at(xd, f0 * H), x_gstride=T * H, vw=vwd, vb=vbd, extra=exd, out=_at(r_att, f0), out_gstride=T, out_idx=oi)
    _per_segment(T, run_seg)
    want = r_att.cpu()
    want[out_idx.long()] = _zero_dead(want[out_idx.long()], T, lens)
    assert torch.equal(att.cpu(), want)
    fa = _mlp_ref(x, 1)[0]
    keep = _zero_dead(torch.ones(cnt, T), T, lens).double()
    ref = torch.sigmoid(fa @ vw.double() + extra.double().unsqueeze(1) + vb.double()) * keep
    assert float((att.cpu()[out_idx.long()].double() - ref).abs().max()) < 1e-5
    _close(sv, fa * keep.unsqueeze(-1), 1e-4, 'save')


@cases
def test_temporal_shape(T, cnt, lens):
    """row-scaled input (scale rows shared through rs_idx), 1 layer, LayerNorm through out_idx"""
    g = _gen(T, cnt, 5)
    x = torch.randn(cnt + 1, T, H, generator=g)
    x_idx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    r = torch.rand(cnt + 1, T, generator=g)
    rs_idx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g); beta = 0.1 * torch.randn(H, generator=g)
    out_idx = _perm(cnt + 2, cnt, g)
    xd, xi, rd, ri, oi, gd, bd = d(x), d(x_idx), d(r), d(rs_idx), d(out_idx), d(gamma), d(beta)
    ln = i32(lens) if lens else None
    layers = _fwd_layers(1)
    out = torch.full((cnt + 2, T, H), -3.0, device=DEV)
    sv = torch.full((cnt, T, H), -3.0, device=DEV)
    _launch(cnt, T, layers, tail=5, X=xd, x_gstride=T * H, x_idx=xi, row_scale=rd, rs_idx=ri, save=[sv], out=out, out_gstride=T * H, out_idx=oi,
            gamma=gd, beta=bd, ln_eps=1e-5, len=ln)
    torch.cuda.synchronize()
    r_out = torch.full((cnt + 2, T, H), -3.0, device=DEV)
    r_sv = torch.zeros(cnt, T, H)

    def run_seg(s, f0, rows):
        ssv = torch.zeros(cnt, rows, H, device=DEV)
        rseg = r[:, f0:f0 + rows].contiguous().to(DEV)               # the scale rows of the segment, [*, rows]
        _launch(cnt, rows, layers, tail=5, X=_at(xd, f0 * H), x_gstride=T * H, x_idx=xi, row_scale=rseg, rs_idx=ri, save=[ssv],
                out=_at(r_out, f0 * H), out_gstride=T * H, out_idx=oi, gamma=gd, beta=bd, ln_eps=1e-5)
        r_sv[:, f0:f0 + rows] = ssv.cpu()
    _per_segment(T, run_seg)
    want = r_out.cpu()
    want[out_idx.long()] = _zero_dead(want[out_idx.long()], T, lens)
    assert torch.equal(out.cpu(), want)
    assert torch.equal(sv.cpu(), _zero_dead(r_sv, T, lens))
    w, b = _lin(0)
    y = torch.relu((r[rs_idx.long()].double().unsqueeze(-1) * x[x_idx.long()].double()) @ w.double().t() + b.double())
    keep = _zero_dead(torch.ones(cnt, T, 1), T, lens).double()
    ref = torch.nn.functional.layer_norm(y, (H,), gamma.double(), beta.double(), 1e-5) * keep
    assert float((out.cpu()[out_idx.long()].double() - ref).abs().max()) < 5e-5
    _close(sv, y * keep, 1e-4, 'y')


def _filter_launch(T, cnt, lens, g):
    S = len(_segs(T))
    x = torch.randn(cnt + 2, T, H, generator=g)
    x_idx = torch.randint(0, cnt + 2, (cnt,), generator=g, dtype=torch.int32)
    out_idx = _perm(cnt + 2, cnt, g)
    xd, xi, oi = d(x), d(x_idx), d(out_idx)
    ln = i32(lens) if lens else None

    def run():
        out = torch.full((cnt + 2, H), -3.0, device=DEV)
        sv = [torch.full((cnt, T, H), -3.0, device=DEV) for _ in range(2)]
        bits = [torch.full((cnt * S, H), -1, dtype=torch.int64, device=DEV) for _ in range(2)]
        _launch(cnt, T, _fwd_layers(2), tail=2, X=xd, x_gstride=T * H, x_idx=xi, out=out, out_gstride=H, out_idx=oi, len=ln, save=sv, save_bits=bits)
        torch.cuda.synchronize()
        return dict(out=out, s0=sv[0], s1=sv[1], b0=bits[0], b1=bits[1])
    return x, x_idx, out_idx, xd, xi, run


@cases
def test_filter_sum_over_frames_crosses_segments(T, cnt, lens):
    """2 layers + the sum over each instance's own frames (SUM_ROWS: one workgroup walks the instance's segments): fp64, run to run,
    the saves and bits against the per-segment launches.  (stair_tile_mlp_fwd always deals its tiles out round robin; the work queue
    against the round robin is test_long_clip_forward_is_the_same_with_the_work_queue_and_round_robin below, through a plan.)"""
    g = _gen(T, cnt, 1)
    x, x_idx, out_idx, xd, xi, run = _filter_launch(T, cnt, lens, g)
    a, b = run(), run()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    acts = _mlp_ref(x[x_idx.long()], 2)
    for i in range(cnt):
        ref = acts[1][i][:(lens[i] if lens else T)].sum(0)
        _close(a['out'][int(out_idx[i])], ref, 2e-5, ('sum', i))
    untouched = torch.ones(cnt + 2, dtype=torch.bool); untouched[out_idx.long()] = False
    assert bool((a['out'].cpu()[untouched] == -3.0).all())
    r_sv = [torch.zeros(cnt, T, H) for _ in range(2)]

    def run_seg(s, f0, rows):
        ssv = [torch.zeros(cnt, rows, H, device=DEV) for _ in range(2)]
        _launch(cnt, rows, _fwd_layers(2), tail=0, X=_at(xd, f0 * H), x_gstride=T * H, x_idx=xi, save=ssv)
        for l in range(2):
            r_sv[l][:, f0:f0 + rows] = ssv[l].cpu()
    _per_segment(T, run_seg)
    keep = _zero_dead(torch.ones(cnt, T, 1), T, lens).double()
    for l in range(2):
        assert torch.equal(a['s%d' % l].cpu(), _zero_dead(r_sv[l], T, lens)), l
        _close(a['s%d' % l], acts[l] * keep, 1e-4, l)
        _check_bits(a['b%d' % l], a['s%d' % l], T, cnt, lens, l)


# ---------------------------------------------------------------------------------------------
# dropout, the switch, the work-item count
# ---------------------------------------------------------------------------------------------
@cases
def test_dropout_drops_the_elements_of_the_row_kernel(T, cnt, lens):
    """nn.Dropout(0.25) behind both activations of a segmented launch: element (instance * T + frame) * H + column is kept exactly where
    stair_dropout_fwd keeps it for the same (seed, site) on a [cnt, T, H] tensor -- the launch-per-layer form at the same T"""
    from stair_amd import ops
    p, seed = 0.25, 11
    g = _gen(T, cnt, 6)
    x = torch.randn(cnt, T, H, generator=g)
    sv = [torch.zeros(cnt, T, H, device=DEV) for _ in range(2)]
    _launch(cnt, T, _fwd_layers(2), X=d(x), x_gstride=T * H, save=sv, drop_site=[1, 2], drop_p=p, drop_seed=seed, len=i32(lens) if lens else None)
    keep = []
    for site in (0, 1):
        ones = torch.ones(cnt, T, H, device=DEV)
        check(lib.stair_dropout_fwd(ones.data_ptr(), T * H, None, cnt, T * H, p, seed, site, ops._stream()))
        keep.append(ones.cpu().double())                   # 0 or 1 / (1 - p)
    torch.cuda.synchronize()
    live = _zero_dead(torch.ones(cnt, T, 1), T, lens).double()
    w0, b0 = _lin(0); w1, b1 = _lin(1)
    h0 = torch.relu(x.double() @ w0.double().t() + b0.double()) * keep[0] * live
    _close(sv[0], h0, 1e-4, 's0')
    h1 = torch.relu(h0 @ w1.double().t() + b1.double()) * keep[1] * live
    _close(sv[1], h1, 1e-4, 's1')
    # exactly the row kernel's elements: a clearly positive activation is zero in the save if and only if its bit says dropped
    for l, h in ((0, torch.relu(x.double() @ w0.double().t() + b0.double())),):
        pos = (h > 1e-3) & (live > 0)
        assert torch.equal((sv[l].cpu() != 0)[pos], (keep[l] != 0)[pos])
        rate = 1.0 - float((keep[l] != 0)[pos].double().mean())
        n = int(pos.sum())
        assert abs(rate - p) < 5 * (p * (1 - p) / n) ** 0.5 + 1e-3, (rate, n)


def test_switch_off_refuses_more_than_64_frames_as_before():
    x = torch.randn(1, 65, H, device=DEV)
    out = torch.zeros(1, 65, H, device=DEV)
    lib.stair_set_tile_split(0)
    with pytest.raises(RuntimeError, match='a tile holds 1..64 frames'):
        _launch(1, 65, _fwd_layers(1), tail=1, X=x, x_gstride=65 * H, out=out, out_gstride=65 * H)
    lib.stair_set_tile_split(1)
    _launch(1, 65, _fwd_layers(1), tail=1, X=x, x_gstride=65 * H, out=out, out_gstride=65 * H)
    with pytest.raises(RuntimeError, match='141'):
        _launch(1, 142, _fwd_layers(1), tail=1, X=x, x_gstride=65 * H, out=out, out_gstride=65 * H)
    torch.cuda.synchronize()
    assert float(out.abs().max()) > 0


@pytest.mark.parametrize('T,cnt,want', [(65, 3, 6), (129, 2, 6), (64, 3, 3)])
def test_work_items_count_segments(T, cnt, want):
    x = torch.randn(cnt, T, H, device=DEV)
    out = torch.empty(cnt, T, H, device=DEV)
    osum = torch.empty(cnt, H, device=DEV)
    _work_items()
    _launch(cnt, T, _fwd_layers(1), tail=1, X=x, x_gstride=T * H, out=out, out_gstride=T * H)
    assert _work_items() == want == cnt * lib.stair_tile_segments(T)
    _launch(cnt, T, _fwd_layers(1), tail=2, X=x, x_gstride=T * H, out=osum, out_gstride=H)        # (SUM_ROWS: cnt work items, cnt S tiles)
    assert _work_items() == want
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# backward chains
# ---------------------------------------------------------------------------------------------


def _seg_bits(bits, cnt, T, s):
    """the words of segment s of every instance, [cnt, 512], as a launch of that segment alone indexes them"""
    return bits.reshape(cnt, len(_segs(T)), H)[:, s].contiguous()


def _chain_layers():
    return [(_planes(1, True), None, 3), (_planes(0, True), None, 0)]


@pytest.mark.parametrize('T,cnt,lens,exclusive', [pytest.param(*c, e, id='%s-%s' % (eid, cid)) for c, cid in zip(CASES, IDS) for e, eid in ((1, 'exclusive'), (0, 'atomic'))] +
                         [pytest.param(*CASES[0], 'store', id='store-' + IDS[0])])
def test_backward_chain_bits_and_first_touch_stores(T, cnt, lens, exclusive):
    """form 3 fed by the bits of a segmented forward launch: dZ saves (save_in, save[0]), ACCUMULATE into targets of the instances' own
    -- read - add - write (acc_exclusive) or float atomics, one add per address -- some marked STORE_FIRST (sentinel targets).
    `store`: the same chain ending in STORE (tail 1), which writes dX over every target whatever it held"""
    tail, exclusive = (1, 0) if exclusive == 'store' else (6, exclusive)
    g = _gen(T, cnt, 7)
    dy = torch.randn(cnt, T, H, generator=g)
    tgt = _perm(cnt + 2, cnt, g)
    first = [(i % 3) != 1 for i in range(cnt)]
    base = torch.randn(cnt + 2, T, H, generator=g)
    for i in range(cnt):
        if first[i]:
            base[int(tgt[i])] = float('nan')
    out_idx = i32([int(tgt[i]) | (STORE_FIRST if first[i] else 0) for i in range(cnt)])
    _, sv, bits = _fwd2(T, cnt, g, lens)
    dyd = d(dy)
    ln = i32(lens) if lens else None
    out = d(base.clone())
    gB, gA = torch.full((cnt, T, H), -3.0, device=DEV), torch.full((cnt, T, H), -3.0, device=DEV)
    _launch(cnt, T, _chain_layers(), tail=tail, X=dyd, x_gstride=T * H, in_bits=bits[1], in_scale=1.0, save_in=gB,
            act_bits=[bits[0]], act_scale=1.0, save=[gA], out=out, out_gstride=T * H, out_idx=out_idx, acc_exclusive=exclusive, len=ln)
    torch.cuda.synchronize()
    r_out = d(base.clone())
    r_gB, r_gA = torch.zeros(cnt, T, H), torch.zeros(cnt, T, H)

    def run_seg(s, f0, rows):
        sB, sA = torch.zeros(cnt, rows, H, device=DEV), torch.zeros(cnt, rows, H, device=DEV)
        _launch(cnt, rows, _chain_layers(), tail=tail, X=_at(dyd, f0 * H), x_gstride=T * H, in_bits=_seg_bits(bits[1], cnt, T, s), in_scale=1.0, save_in=sB,
                act_bits=[_seg_bits(bits[0], cnt, T, s)], act_scale=1.0, save=[sA], out=_at(r_out, f0 * H), out_gstride=T * H, out_idx=out_idx,
                acc_exclusive=exclusive)
        r_gB[:, f0:f0 + rows] = sB.cpu(); r_gA[:, f0:f0 + rows] = sA.cpu()
    _per_segment(T, run_seg)
    # a segment behind its clip's end: its forward bits are zero, so the per-segment launches compute zeros there as well -- and a
    # target that adds gets + 0.0
    got, want = out.cpu()[tgt.long()], r_out.cpu()[tgt.long()]
    assert not bool(got.isnan().any())
    assert torch.equal(got, want) and torch.equal(gA.cpu(), r_gA) and torch.equal(gB.cpu(), r_gB)
    rest = torch.ones(cnt + 2, dtype=torch.bool); rest[tgt.long()] = False
    assert torch.equal(out.cpu()[rest], base[rest])
    dz2, dz1, dx = _chain_ref(dy, sv)
    _close(gB, dz2, 3e-5, 'dZ2'); _close(gA, dz1, 3e-5, 'dZ1')
    for i in range(cnt):
        ref = dx[i] if first[i] or tail == 1 else dx[i] + base[int(tgt[i])].double()
        _close(got[i], ref, 3e-5, ('dX', i))


@cases
def test_backward_chain_broadcast_input(T, cnt, lens):
    """form 3 with Filter's input -- ONE gradient row per instance, broadcast over its own frames (len) -- and plain ACCUMULATE (float
    atomics, no first-touch marks) into zeroed targets of the instances' own"""
    g = _gen(T, cnt, 8)
    rows_ = torch.randn(cnt + 1, H, generator=g)
    x_idx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    lens_ = list(lens) if lens else [(T, T - 3, min(66, T), 1)[i % 4] for i in range(cnt)]
    tgt = _perm(cnt + 1, cnt, g)
    _, sv, bits = _fwd2(T, cnt, g)
    rd, xi, ln, oi = d(rows_), d(x_idx), i32(lens_), d(tgt)
    out = torch.zeros(cnt + 1, T, H, device=DEV)
    gB, gA = torch.full((cnt, T, H), -3.0, device=DEV), torch.full((cnt, T, H), -3.0, device=DEV)
    _launch(cnt, T, _chain_layers(), tail=6, X=rd, x_gstride=H, x_idx=xi, x_broadcast=1, len=ln, in_bits=bits[1], in_scale=1.0, save_in=gB,
            act_bits=[bits[0]], act_scale=1.0, save=[gA], out=out, out_gstride=T * H, out_idx=oi, acc_exclusive=0)
    torch.cuda.synchronize()
    r_out = torch.zeros(cnt + 1, T, H, device=DEV)
    r_gB, r_gA = torch.zeros(cnt, T, H), torch.zeros(cnt, T, H)

    def run_seg(s, f0, rows):
        sB, sA = torch.zeros(cnt, rows, H, device=DEV), torch.zeros(cnt, rows, H, device=DEV)
        sl = i32([max(0, min(rows, l - f0)) for l in lens_])
        _launch(cnt, rows, _chain_layers(), tail=6, X=rd, x_gstride=H, x_idx=xi, x_broadcast=1, len=sl, in_bits=_seg_bits(bits[1], cnt, T, s), in_scale=1.0,
                save_in=sB, act_bits=[_seg_bits(bits[0], cnt, T, s)], act_scale=1.0, save=[sA], out=_at(r_out, f0 * H), out_gstride=T * H, out_idx=oi,
                acc_exclusive=0)
        r_gB[:, f0:f0 + rows] = sB.cpu(); r_gA[:, f0:f0 + rows] = sA.cpu()
    _per_segment(T, run_seg)
    assert torch.equal(out.cpu(), r_out.cpu()) and torch.equal(gA.cpu(), r_gA) and torch.equal(gB.cpu(), r_gB)
    dy = rows_[x_idx.long()].unsqueeze(1).expand(-1, T, -1).clone()
    for i in range(cnt):
        dy[i, lens_[i]:] = 0.0
    dz2, dz1, dx = _chain_ref(dy, sv)
    _close(gB, dz2, 3e-5, 'dZ2'); _close(gA, dz1, 3e-5, 'dZ1')
    _close(out.cpu()[tgt.long()], dx, 3e-5, 'dX')


@cases
def test_backward_chain_float_masks(T, cnt, lens):
    """form 3 with the relu' masks as fp32 activations -- the input's through in_mask_idx / in_mask_gstride (mask tiles shared by
    instances), the layer's as act_mask [cnt, T, H] -- X through x_idx, read - add - write with some first-touch stores"""
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
    dyd, xi, mind, mi, mactd = d(dy), d(x_idx), d(m_in), d(m_idx), d(m_act)
    ln = i32(lens) if lens else None
    out = d(base.clone())
    gB, gA = torch.full((cnt, T, H), -3.0, device=DEV), torch.full((cnt, T, H), -3.0, device=DEV)
    _launch(cnt, T, _chain_layers(), tail=6, X=dyd, x_gstride=T * H, x_idx=xi, in_mask=mind, in_mask_gstride=T * H, in_mask_idx=mi, in_scale=1.0,
            save_in=gB, act_mask=[mactd], act_scale=1.0, save=[gA], out=out, out_gstride=T * H, out_idx=out_idx, acc_exclusive=1, len=ln)
    torch.cuda.synchronize()
    r_out = d(base.clone())
    r_gB, r_gA = torch.zeros(cnt, T, H), torch.zeros(cnt, T, H)

    def run_seg(s, f0, rows):
        sB, sA = torch.zeros(cnt, rows, H, device=DEV), torch.zeros(cnt, rows, H, device=DEV)
        mseg = m_act[:, f0:f0 + rows].contiguous().to(DEV)
        _launch(cnt, rows, _chain_layers(), tail=6, X=_at(dyd, f0 * H), x_gstride=T * H, x_idx=xi, in_mask=_at(mind, f0 * H), in_mask_gstride=T * H,
                in_mask_idx=mi, in_scale=1.0, save_in=sB, act_mask=[mseg], act_scale=1.0, save=[sA], out=_at(r_out, f0 * H), out_gstride=T * H,
                out_idx=out_idx, acc_exclusive=1)
        r_gB[:, f0:f0 + rows] = sB.cpu(); r_gA[:, f0:f0 + rows] = sA.cpu()
    _per_segment(T, run_seg)
    keep = _zero_dead(torch.ones(cnt, T, 1), T, lens)
    got = out.cpu()[tgt.long()]
    want = r_out.cpu()[tgt.long()]
    for i in range(cnt):            # a segment behind the clip's end: zeros stored first, nothing added otherwise
        for _, f0, rows in _segs(T):
            if not _live(lens, i, f0):
                want[i, f0:f0 + rows] = 0.0 if first[i] else base[int(tgt[i]), f0:f0 + rows]
    assert not bool(got.isnan().any())
    assert torch.equal(got, want) and torch.equal(gA.cpu(), r_gA * keep) and torch.equal(gB.cpu(), r_gB * keep)
    dz2 = dy[x_idx.long()].double() * (m_in[m_idx.long()] > 0).double() * keep.double()
    dz1 = (dz2 @ _lin(1)[0].double()) * (m_act > 0).double()
    dx = dz1 @ _lin(0)[0].double()
    _close(gB, dz2, 3e-5, 'dZ2'); _close(gA, dz1, 3e-5, 'dZ1')
    for i in range(cnt):
        ref = dx[i] if first[i] else dx[i] + base[int(tgt[i])].double()
        _close(got[i], ref, 3e-5, ('dX', i))


@cases
@pytest.mark.parametrize('mode', ['exclusive_mixed', 'all_first', 'atomic_mixed'])
def test_temporal_backward_chain(T, cnt, lens, mode):
    """form 2: the LayerNorm adjoint in, the row-scale adjoint out (adj_feat, adj_rs, adj_drs entered at the segment's frame).  dZ,
    d feat and d r bit for bit against the per-segment launches; d gamma / d beta are float sums over a TILE's rows, the same tiles in
    both: against the per-segment launches within the bound of tests/test_gpu_tile_fused.py::
    test_fused_and_sequenced_paths_agree_forward_and_backward (2e-4 of the tensor's largest entry), against fp64 autograd at that file's
    3e-5.  Run to run everything is bit-identical, d gamma / d beta too as long as the launch has at most two tiles: outside a plan's
    backward pass they are float atomics, one per workgroup and column, and three addends do not commute (as in the unsegmented kernel;
    inside a plan they go through the fixed-point shadows -- tests/test_gpu_long_clip_plans.py checks that step bit for bit)."""
    g = _gen(T, cnt, 9)
    first = [{'all_first': True}.get(mode, (i % 3) != 1) for i in range(cnt)]
    feat = torch.randn(cnt + 1, T, H, generator=g)
    fidx = _perm(cnt + 1, cnt, g)
    rs = torch.rand(cnt + 2, T, generator=g)
    ridx = _perm(cnt + 2, cnt, g)
    w, b = _lin(0)
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g)
    dy = torch.randn(cnt + 1, T, H, generator=g)
    yidx = torch.randint(0, cnt + 1, (cnt,), generator=g, dtype=torch.int32)
    if lens:                                    # the gradient of a frame behind the clip's end is zero in a plan; here too
        dy = dy[yidx.long()].clone(); yidx = torch.arange(cnt, dtype=torch.int32)
        for i in range(cnt):
            dy[i, lens[i]:] = 0.0
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
            dfeat0[int(fidx[i])] = float('nan')
    ad, dyd, gd, fd, rd = d(a.detach().float()), d(dy), d(gamma), d(feat), d(rs)
    yi, fi, ri = d(yidx), d(fidx), d(ridx)
    oi = i32([int(fidx[i]) | (STORE_FIRST if first[i] else 0) for i in range(cnt)])
    ln = i32(lens) if lens else None
    wT = _planes(0, True)
    excl = 0 if mode == 'atomic_mixed' else 1

    def chain(rows, f0, Xp, maskp, featp, rsd, dfeat, drs, dgamma, dbeta, dz, len_):
        _launch(cnt, rows, [(wT, None, 0)], tail=8, X=Xp, x_gstride=T * H, x_idx=yi, ln_bwd=1, in_mask=maskp, in_mask_gstride=T * H, in_scale=1.0,
                save_in=dz, gamma=gd, dgamma=dgamma, dbeta=dbeta, ln_eps=1e-5, out=dfeat, out_gstride=T * H, out_idx=oi,
                adj_feat=featp, adj_feat_gstride=T * H, adj_feat_idx=fi, adj_rs=rsd, adj_rs_idx=ri, adj_drs=drs, acc_exclusive=excl, len=len_)

    def run():
        dfeat, drs = d(dfeat0.clone()), d(drs0.clone())
        dgamma, dbeta = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
        dz = torch.full((cnt, T, H), -3.0, device=DEV)
        chain(T, 0, dyd, ad, fd, rd, dfeat, drs, dgamma, dbeta, dz, ln)
        torch.cuda.synchronize()
        return dict(dz=dz, dfeat=dfeat[fi.long()], drs=drs, dgamma=dgamma, dbeta=dbeta)
    one, two = run(), run()
    tiles = cnt * len(_segs(T))
    for k in one:
        if tiles <= 2 or k not in ('dgamma', 'dbeta'):
            assert torch.equal(one[k], two[k]), k
    r_dfeat, r_drs = d(dfeat0.clone()), drs0.clone()
    r_dgamma, r_dbeta = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    r_dz = torch.zeros(cnt, T, H)

    def run_seg(s, f0, rows):
        sdz = torch.zeros(cnt, rows, H, device=DEV)
        rseg = rs[:, f0:f0 + rows].contiguous().to(DEV)
        sdrs = drs0[:, f0:f0 + rows].contiguous().to(DEV)
        chain(rows, f0, _at(dyd, f0 * H), _at(ad, f0 * H), _at(fd, f0 * H), rseg, _at(r_dfeat, f0 * H), sdrs, r_dgamma, r_dbeta, sdz, None)
        r_dz[:, f0:f0 + rows] = sdz.cpu(); r_drs[:, f0:f0 + rows] = sdrs.cpu()
    _per_segment(T, run_seg)
    assert not bool(one['dfeat'].isnan().any())
    keep = _zero_dead(torch.ones(cnt, T, 1), T, lens)
    # (ragged: the per-segment launches compute the segments behind a clip's end from zero gradient rows: zeros, as the skipped ones)
    assert torch.equal(one['dz'].cpu(), r_dz * keep)
    assert torch.equal(one['dfeat'].cpu(), r_dfeat.cpu()[fidx.long()])
    assert torch.equal(one['drs'].cpu(), r_drs)
    gmax = max(float(r_dgamma.abs().max()), float(r_dbeta.abs().max()))
    for k, ref in (('dgamma', r_dgamma), ('dbeta', r_dbeta)):
        assert float((one[k] - ref).abs().max()) < 2e-4 * max(float(ref.abs().max()), 1e-3 * gmax), k
    _close(one['dz'], z.grad, 3e-5, 'dZ')
    for i in range(cnt):
        ref = F.grad[fidx[i].long()] if first[i] else F.grad[fidx[i].long()] + dfeat0[fidx[i].long()].double()
        _close(one['dfeat'][i], ref, 3e-5, ('dfeat', i))
    _close(one['drs'].cpu() - drs0, R.grad, 3e-5, 'drs')
    _close(one['dgamma'], G.grad, 3e-5, 'dgamma')
    _close(one['dbeta'], Bt.grad, 3e-5, 'dbeta')


# ---------------------------------------------------------------------------------------------
# the work queue against the round robin (a plan's launches take the queue; stair_tile_mlp_fwd does not)
# ---------------------------------------------------------------------------------------------
def test_long_clip_forward_is_the_same_with_the_work_queue_and_round_robin():
    """T = 100, every program form (Filter's cross-segment sum among them): logits and every node bit for bit, queue on / off, twice"""
    from stair_amd.module_net import VideoNMN
    config = dict(spec.DEFAULT_CONFIG, video_size=128, answer_vocab_length=16, max_video_length=100, object_types=10)
    model = VideoNMN(config)
    w = synth.make_weights(config, 2)
    model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    model = model.to(DEV)
    qs = synth.make_questions(config, 5, 12, forms=synth.ALL_FORMS, T=100)
    runs = []
    for q_on in (1, 0, 1):
        lib.stair_set_tile_queue(q_on)
        _work_items()
        res = model.forward_batch(qs)
        nodes = [res.logits.cpu().clone()]
        for qi, q in enumerate(qs):
            for i in range(len(q['nmn_program_list'])):
                v = res.node(qi, i)
                if isinstance(v, torch.Tensor):
                    nodes.append(v.detach().cpu().clone())
        assert _work_items() > 0
        runs.append(nodes)
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
